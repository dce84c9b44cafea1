"""GPU: kernel-level checks of librpde_hip.so through its C ABI.

The GEMM is compared with a float64 torch matmul of the same operands (a plain
torch reference is right for a floating-point kernel); the DFT plan tables with
the float64 restatement in oracle/dft_math.py; the dropout masks of the three
places that regenerate them with each other."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GEMM_TOL = 2e-6     # fp32 MFMA (exact fp32 FMA chain) vs float64, rel-L2


def _gemm(dev, M, N, K, a_k, b_k, batch=1, ksplit=1, bias_mode=0, accumulate=False, act_a=0, act_b=0, seed=0,
          alpha=1.0, write_act=0):
    from rpde import _lib
    lib = _lib.load()
    g = torch.Generator(device="cpu").manual_seed(seed)
    A = torch.randn(batch, M, K, generator=g)
    B = torch.randn(batch, K, N, generator=g)
    Ad = (A if a_k else A.transpose(1, 2)).contiguous().to(dev)      # [b,M,K] or [b,K,M]
    Bd = (B.transpose(1, 2) if b_k else B).contiguous().to(dev)      # [b,N,K] or [b,K,N]
    C0 = torch.randn(batch, M, N, generator=g)
    Cd = C0.clone().to(dev) if ksplit == 1 else torch.zeros(ksplit, batch, M, N, device=dev)
    bias = torch.randn(N if bias_mode == 1 else M, generator=g)
    bd = bias.to(dev)
    d = _lib.GemmDesc()
    d.A, d.B, d.C = Ad.data_ptr(), Bd.data_ptr(), Cd.data_ptr()
    d.M, d.N, d.K = M, N, K
    d.a_kmajor, d.b_kmajor = int(a_k), int(b_k)
    d.lda = K if a_k else M
    d.ldb = K if b_k else N
    d.ldc = N
    d.batch, d.zdiv = batch, 1
    d.sA1, d.sB1, d.sC1 = M * K, K * N, M * N
    d.ksplit, d.sCk = ksplit, batch * M * N
    d.alpha, d.accumulate = alpha, int(accumulate)
    if bias_mode:
        d.bias, d.bias_mode = bd.data_ptr(), bias_mode
    d.act_a, d.act_b, d.write_act = act_a, act_b, write_act
    _lib.check(lib.rpde_gemm_f32(C.byref(d), _lib.stream_ptr()), "gemm")
    torch.cuda.synchronize()
    act = {0: lambda t: t, 1: torch.nn.functional.gelu, 2: torch.relu}
    ref = alpha * (act[act_a](A.double()) @ act[act_b](B.double()))
    if bias_mode == 1:
        ref = ref + bias.double()[None, None, :]
    elif bias_mode == 2:
        ref = ref + bias.double()[None, :, None]
    if accumulate:
        ref = ref + C0.double()
    ref = act[write_act](ref)
    got = Cd.cpu().double() if ksplit == 1 else Cd.cpu().double().sum(0)
    return float((got - ref).norm() / ref.norm())


LAYOUTS = [(1, 1), (1, 0), (0, 0), (0, 1)]
SHAPES = [(128, 128, 64), (256, 256, 256), (200, 72, 40), (33, 17, 5), (40, 64, 256), (64, 3, 7), (1000, 64, 3),
          (512, 1, 64), (31, 129, 130), (129, 31, 33), (300, 40, 36)]


@pytest.mark.parametrize("a_k,b_k", LAYOUTS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_layouts_and_edges(gpu_device, M, N, K, a_k, b_k):
    err = _gemm(gpu_device, M, N, K, a_k, b_k, seed=M + N + K)
    assert err < GEMM_TOL, err


def test_gemm_fuzz_shapes_layouts_splits(gpu_device):
    """120 seeded random problems: every layout, ragged and aligned extents (both the split-bf16 and the native
    kernels get picked), batches, K-splits that are / are not multiples of 8 (both workgroup orders)."""
    rng = np.random.default_rng(2024)
    worst = 0.0
    for it in range(120):
        aligned = rng.random() < 0.6
        q = 4 if aligned else 1
        M = int(rng.integers(1, 80)) * q
        N = int(rng.integers(1, 80)) * q
        K = int(rng.choice([32, 64, 96, 128, 256])) if (aligned and rng.random() < 0.7) else int(rng.integers(1, 300))
        a_k, b_k = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        batch = int(rng.choice([1, 1, 2, 5]))
        ksplit = int(rng.choice([1, 1, 1, 3, 8, 16]))
        if ksplit > 1:
            K = max(K, 64) * 4
            err = _gemm(gpu_device, M, N, K, a_k, b_k, batch=batch, ksplit=ksplit, seed=it)
        else:
            err = _gemm(gpu_device, M, N, K, a_k, b_k, batch=batch, seed=it, bias_mode=int(rng.integers(0, 3)),
                        accumulate=bool(rng.integers(0, 2)), alpha=float(rng.choice([1.0, 0.5, -2.0])))
        worst = max(worst, err)
        assert err < 4e-6, (it, M, N, K, a_k, b_k, batch, ksplit, err)
    assert worst > 0.0


def test_gemm_batched_bias_accumulate(gpu_device):
    assert _gemm(gpu_device, 130, 70, 50, 1, 0, batch=5, bias_mode=1, accumulate=True) < GEMM_TOL
    assert _gemm(gpu_device, 64, 200, 33, 1, 0, batch=3, bias_mode=2, alpha=0.5) < GEMM_TOL


def test_gemm_split_k(gpu_device):
    assert _gemm(gpu_device, 256, 256, 5000, 0, 0, ksplit=7) < 4e-6
    assert _gemm(gpu_device, 64, 3, 4097, 0, 0, ksplit=16, batch=2) < 4e-6
    # few tiles x many slabs: the XCD-grouped workgroup order (slabs of one tile set share an L2)
    assert _gemm(gpu_device, 256, 256, 8192, 0, 0, ksplit=16) < 4e-6
    assert _gemm(gpu_device, 200, 130, 4096, 0, 0, ksplit=8, batch=3) < 4e-6
    assert _gemm(gpu_device, 64, 256, 2048, 0, 0, ksplit=24) < 4e-6


def test_gemm_activation_prologue_and_store(gpu_device):
    assert _gemm(gpu_device, 200, 256, 64, 1, 1, act_a=1) < 1e-5
    assert _gemm(gpu_device, 128, 100, 300, 0, 0, act_b=1) < 1e-5
    assert _gemm(gpu_device, 77, 130, 40, 1, 0, act_b=2, write_act=2) < 1e-5


def test_gemm_dact_epilogue_matches_autograd(gpu_device):
    """C = (G @ W) * gelu'(Z) against torch autograd of gelu."""
    from rpde import _lib
    lib = _lib.load()
    P, N, K = 300, 96, 64
    g = torch.Generator().manual_seed(3)
    G, W, Z = torch.randn(P, K, generator=g), torch.randn(K, N, generator=g), torch.randn(P, N, generator=g)
    Gd, Wd, Zd = G.to(gpu_device), W.to(gpu_device), Z.to(gpu_device)
    out = torch.empty(P, N, device=gpu_device)
    d = _lib.GemmDesc()
    d.A, d.B, d.C = Gd.data_ptr(), Wd.data_ptr(), out.data_ptr()
    d.M, d.N, d.K, d.a_kmajor, d.b_kmajor = P, N, K, 1, 0
    d.lda, d.ldb, d.ldc, d.batch, d.zdiv, d.ksplit, d.alpha = K, N, N, 1, 1, 1, 1.0
    d.epi_dact, d.aux, d.ldaux = 1, Zd.data_ptr(), N
    _lib.check(lib.rpde_gemm_f32(C.byref(d), _lib.stream_ptr()), "gemm")
    z = Z.double().requires_grad_(True)
    torch.nn.functional.gelu(z).backward(G.double() @ W.double())
    err = float((out.cpu().double() - z.grad).norm() / z.grad.norm())
    assert err < 1e-5, err


def test_dropout_masks_agree_between_prologues_and_epilogue(gpu_device):
    """The forward staging (A operand), the weight-gradient staging (B operand)
    and the backward-data epilogue must regenerate one and the same mask."""
    from rpde import _lib
    lib = _lib.load()
    P, J, p, seed = 256, 128, 0.25, 1234567
    eye_j = torch.eye(J, device=gpu_device)
    eye_p = torch.eye(P, device=gpu_device)
    ones = torch.ones(P, J, device=gpu_device)

    def run(**kw):
        out = torch.empty(P, J, device=gpu_device)
        d = _lib.GemmDesc()
        d.batch, d.zdiv, d.ksplit, d.alpha = 1, 1, 1, 1.0
        d.C, d.ldc, d.M, d.N = out.data_ptr(), J, P, J
        d.drop_p, d.drop_seed, d.drop_ld = p, seed, J
        for k, v in kw.items():
            setattr(d, k, v)
        _lib.check(lib.rpde_gemm_f32(C.byref(d), _lib.stream_ptr()), "gemm")
        return out.cpu()

    # A-operand prologue: identity act + dropout of ones, times I
    m_a = run(A=ones.data_ptr(), lda=J, a_kmajor=1, B=eye_j.data_ptr(), ldb=J, b_kmajor=1, K=J, act_a=0, drop_where=1)
    # B-operand prologue: I[P,P] times dropout(ones[P,J]) with points along the reduction
    m_b = run(A=eye_p.data_ptr(), lda=P, a_kmajor=1, B=ones.data_ptr(), ldb=J, b_kmajor=0, K=P, act_b=0, drop_where=2)
    # epilogue: acc = ones, aux large so gelu'(aux*s) is 1 where kept
    big = torch.full((P, J), 30.0, device=gpu_device)
    m_e = run(A=ones.data_ptr(), lda=J, a_kmajor=1, B=eye_j.data_ptr(), ldb=J, b_kmajor=0, K=J, epi_dact=1,
              aux=big.data_ptr(), ldaux=J, drop_where=4)
    keep_a, keep_b, keep_e = m_a != 0, m_b != 0, m_e != 0
    assert torch.equal(keep_a, keep_b) and torch.equal(keep_a, keep_e)
    frac = 1.0 - keep_a.float().mean().item()
    assert abs(frac - p) < 0.02, frac
    scale = m_b[keep_b].unique()
    assert scale.numel() == 1 and abs(scale.item() - 1 / (1 - p)) < 1e-3


@pytest.mark.parametrize("n,k,norm", [(256, 20, "ortho"), (33, 17, "backward"), (64, 33, "ortho"), (1024, 16, "backward")])
def test_plan_tables_match_float64_restatement(gpu_device, n, k, norm):
    from oracle import dft_math as D
    from rpde import _lib
    lib = _lib.load()
    plan = C.c_void_p()
    _lib.check(lib.rpde_plan_create(C.byref(plan), n, k, _lib.NORM[norm], _lib.stream_ptr()), "plan_create")
    nn_, mm, kp, ldn = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _lib.check(lib.rpde_plan_info(plan, C.byref(nn_), C.byref(mm), C.byref(kp), C.byref(ldn)), "plan_info")
    fa = np.zeros((2 * kp.value, ldn.value), dtype=np.float32)
    fs = np.zeros((n, 2 * kp.value), dtype=np.float32)
    _lib.check(lib.rpde_plan_tables(plan, fa.ctypes.data, fs.ctypes.data), "plan_tables")
    _lib.check(lib.rpde_plan_destroy(plan), "plan_destroy")
    ra, rs = D.analysis(n, k, norm), D.synthesis(n, k, norm)
    assert np.abs(fa[:2 * k, :n] - ra).max() <= 6e-8 * max(1.0, np.abs(ra).max())
    assert np.abs(fs[:, :2 * k] - rs).max() <= 6e-8 * max(1.0, np.abs(rs).max())
    assert not fa[2 * k:].any() and not fa[:, n:].any() and not fs[:, 2 * k:].any()


def test_cpu_tensor_is_rejected_loudly(gpu_device):
    from rpde import RpdeError, ops
    with pytest.raises(RpdeError):
        ops.relative_l2(torch.randn(2, 8), torch.randn(2, 8))


def test_gemm_writes_activation_and_derivative_once(gpu_device):
    """write_act + aux_out: C = gelu(dropout(acc+bias)), aux_out = gelu'(dropout(.)) * scale; a second GEMM
    with RPDE_EPI_MULAUX multiplies by that stored derivative; column sums of the stored C come with it."""
    from rpde import _lib
    lib = _lib.load()
    P, N, K, p, seed = 640, 256, 64, 0.2, 99
    g = torch.Generator().manual_seed(5)
    X, W, b = torch.randn(P, K, generator=g), torch.randn(N, K, generator=g) * 0.2, torch.randn(N, generator=g)
    Xd, Wd, bd = X.to(gpu_device), W.to(gpu_device), b.to(gpu_device)
    h, dd = torch.empty(P, N, device=gpu_device), torch.empty(P, N, device=gpu_device)
    cs = torch.empty((P + 127) // 128, N, device=gpu_device)
    d = _lib.GemmDesc()
    d.A, d.B, d.C = Xd.data_ptr(), Wd.data_ptr(), h.data_ptr()
    d.M, d.N, d.K, d.a_kmajor, d.b_kmajor = P, N, K, 1, 1
    d.lda, d.ldb, d.ldc, d.batch, d.zdiv, d.ksplit, d.alpha = K, K, N, 1, 1, 1, 1.0
    d.bias, d.bias_mode, d.write_act, d.aux_out, d.colsum = bd.data_ptr(), 1, 1, dd.data_ptr(), cs.data_ptr()
    d.drop_p, d.drop_seed, d.drop_ld, d.drop_where = p, seed, N, 4
    _lib.check(lib.rpde_gemm_f32(C.byref(d), _lib.stream_ptr()), "gemm")
    torch.cuda.synchronize()
    z = X.double() @ W.double().T + b.double()
    hh, dv = h.cpu().double(), dd.cpu().double()
    keep = dv != 0                                   # gelu' is never exactly 0 where kept (|z| is moderate here)
    frac = 1 - keep.double().mean().item()
    assert abs(frac - p) < 0.02, frac
    scale = 1 / (1 - round(p * 65536) / 65536)
    zr = (z * scale * keep).requires_grad_(True)
    ref_h = torch.nn.functional.gelu(zr)
    ref_h.sum().backward()
    assert float((hh - ref_h.detach()).norm() / ref_h.detach().norm()) < 2e-6
    ref_d = zr.grad * scale * keep
    assert float((dv - ref_d).norm() / ref_d.norm()) < 2e-6
    assert float((cs.cpu().double().sum(0) - hh.sum(0)).abs().max()) < 1e-3
    # backward-data through the stored derivative: gx = (G @ W2) * d
    G = torch.randn(P, 96, generator=g)
    W2 = torch.randn(96, N, generator=g)
    Gd, W2d = G.to(gpu_device), W2.to(gpu_device)
    gx = torch.empty(P, N, device=gpu_device)
    e = _lib.GemmDesc()
    e.A, e.B, e.C = Gd.data_ptr(), W2d.data_ptr(), gx.data_ptr()
    e.M, e.N, e.K, e.a_kmajor, e.b_kmajor = P, N, 96, 1, 0
    e.lda, e.ldb, e.ldc, e.batch, e.zdiv, e.ksplit, e.alpha = 96, N, N, 1, 1, 1, 1.0
    e.epi_dact, e.aux, e.ldaux = 100, dd.data_ptr(), N
    _lib.check(lib.rpde_gemm_f32(C.byref(e), _lib.stream_ptr()), "gemm")
    ref = (G.double() @ W2.double()) * dv
    assert float((gx.cpu().double() - ref).norm() / ref.norm()) < 2e-6


@pytest.mark.parametrize("M,N,K,b_k", [(4096, 256, 256, 1), (4096, 256, 256, 0), (1500, 64, 256, 1), (1100, 200, 64, 0),
                                       (2048, 256, 96, 0)])
def test_presplit_weight_operand_is_bit_identical(gpu_device, M, N, K, b_k):
    """rpde_split_weights + rpde_gemm_desc.b_split: the weight is split into bf16 images once instead of in
    every workgroup.  Same arithmetic, so C must match the un-pre-split launch bit for bit (k-major B) and
    the float64 product to fp32-GEMM accuracy (either layout of the fp32 original)."""
    from rpde import _lib
    lib = _lib.load()
    dev = gpu_device
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * torch.logspace(-3, 3, N)[:, None]      # wide dynamic range
    Ad = A.to(dev)
    Wd = (W if b_k else W.t()).contiguous().to(dev)                              # [N,K] or [K,N]
    nbytes = lib.rpde_split_weights_bytes(N, K)
    assert nbytes == (K // 32) * 3 * ((N + 127) // 128 * 128) * 64
    img = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.rpde_split_weights(Wd.data_ptr(), b_k, K if b_k else N, N, K, img.data_ptr(), _lib.stream_ptr()), "split")

    def run(use_img):
        out = torch.empty(M, N, device=dev)
        d = _lib.GemmDesc()
        d.A, d.B, d.C = Ad.data_ptr(), Wd.data_ptr(), out.data_ptr()
        d.M, d.N, d.K, d.a_kmajor, d.b_kmajor = M, N, K, 1, b_k
        d.lda, d.ldb, d.ldc, d.batch, d.zdiv, d.ksplit, d.alpha = K, (K if b_k else N), N, 1, 1, 1, 1.0
        if use_img:
            d.b_split = img.data_ptr()
        _lib.check(lib.rpde_gemm_f32(C.byref(d), _lib.stream_ptr()), "gemm")
        torch.cuda.synchronize()
        return out.cpu()

    with_img, without = run(True), run(False)
    ref = A.double() @ W.double().t()
    assert float((with_img.double() - ref).norm() / ref.norm()) < GEMM_TOL
    assert float((without.double() - ref).norm() / ref.norm()) < GEMM_TOL
    import os
    if b_k and os.environ.get("RPDE_SPLIT_BF16") != "0":
        assert torch.equal(with_img, without)
    # the three images reconstruct the weights exactly: hi + mid + lo == w in fp32
    if K % 32 == 0:
        npad = (N + 127) // 128 * 128
        im = img.cpu().numpy().view(np.uint16).reshape(K // 32, 3, npad, 4, 8)
        rows = np.arange(npad)
        unsw = np.empty_like(im)
        for c in range(4):                      # undo the chunk swizzle
            unsw[:, :, rows, c, :] = im[:, :, rows, c ^ ((rows >> 2) & 3), :]
        f = (unsw.astype(np.uint32) << 16).view(np.float32).reshape(K // 32, 3, npad, 32)
        rec = (f[:, 0].astype(np.float64) + f[:, 1] + f[:, 2]).transpose(1, 0, 2).reshape(npad, K)
        np.testing.assert_array_equal(rec[:N].astype(np.float32), W.numpy())
        assert not rec[N:].any()


@pytest.mark.parametrize("M,N,K,a_k,acc", [(40, 64, 256, 1, False), (40, 64, 256, 0, False), (256, 64, 40, 1, True),
                                           (256, 64, 40, 0, False), (24, 32, 100, 1, False), (512, 128, 72, 1, True)])
def test_presplit_table_operand_with_k_tail(gpu_device, M, N, K, a_k, acc):
    """rpde_gemm_desc.a_split: a batch-shared A (a DFT table) pre-split once; B x-major per batch entry
    (a channels-last field line).  K need not be a multiple of 32 (the images are zero-padded)."""
    from rpde import _lib
    lib = _lib.load()
    dev = gpu_device
    batch = 7
    g = torch.Generator(device="cpu").manual_seed(M * 3 + N + K)
    A = torch.randn(M, K, generator=g)
    Bm = torch.randn(batch, K, N, generator=g)
    C0 = torch.randn(batch, M, N, generator=g)
    Ad = (A if a_k else A.t()).contiguous().to(dev)
    Bd, Cd = Bm.to(dev), C0.clone().to(dev)
    img = torch.empty(lib.rpde_split_weights_bytes(M, K), dtype=torch.uint8, device=dev)
    _lib.check(lib.rpde_split_weights(Ad.data_ptr(), a_k, K if a_k else M, M, K, img.data_ptr(), _lib.stream_ptr()), "split")
    d = _lib.GemmDesc()
    d.A, d.B, d.C = Ad.data_ptr(), Bd.data_ptr(), Cd.data_ptr()
    d.M, d.N, d.K, d.a_kmajor, d.b_kmajor = M, N, K, a_k, 0
    d.lda, d.ldb, d.ldc = (K if a_k else M), N, N
    d.batch, d.zdiv, d.ksplit, d.alpha = batch, 1, 1, 1.0
    d.sB1, d.sC1 = K * N, M * N
    d.accumulate = int(acc)
    d.a_split = img.data_ptr()
    _lib.check(lib.rpde_gemm_f32(C.byref(d), _lib.stream_ptr()), "gemm")
    torch.cuda.synchronize()
    ref = A.double()[None] @ Bm.double() + (C0.double() if acc else 0)
    assert float((Cd.cpu().double() - ref).norm() / ref.norm()) < GEMM_TOL


def test_native_fp32_mfma_path_stays_green(gpu_device):
    """The default dispatch sends NT problems to the split-bf16 kernel; one child process re-runs the
    kernel and golden parity tests with RPDE_SPLIT_BF16=0 so the native fp32-MFMA kernels stay covered."""
    import os
    import subprocess
    import sys
    if os.environ.get("RPDE_SPLIT_BF16") == "0":
        pytest.skip("already the native-fp32 leg")
    env = dict(os.environ, RPDE_SPLIT_BF16="0")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_kernels.py"),
                        os.path.join(here, "test_gpu_golden.py"), os.path.join(here, "test_gpu_gemm_descriptor.py"),
                        "-q", "-m", "gpu", "-p", "no:cacheprovider", "-x"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]


@pytest.mark.parametrize("shape", [(2, 32, 128, 1, 64 * 48), (1, 32, 100, 3, 256), (2, 64, 64, 2, 512), (1, 32, 16, 1, 16)])
@pytest.mark.parametrize("act_in", ["identity", "gelu"])
def test_fused_projection_mlp_matches_float64(gpu_device, shape, act_in):
    """csrc/conv_mlp.hip: mlp2(gelu(mlp1(act_in(x)))) in one pass (evaluation) against float64 and the two-convolution path"""
    import os
    import torch.nn.functional as F
    from rpde import ops
    B, Ci, Cm, Co, S = shape
    torch.manual_seed(Ci + Cm + S)
    x = torch.randn(B, Ci, S, device=gpu_device) * 3.0
    x[:, :, ::7] *= 1e-3                                   # tiles of very different magnitude
    w1 = torch.randn(Cm, Ci, 1, device=gpu_device) * 0.3
    b1 = torch.randn(Cm, device=gpu_device) * 0.2
    w2 = torch.randn(Co, Cm, 1, device=gpu_device) * 0.2
    b2 = torch.randn(Co, device=gpu_device)
    with torch.no_grad():
        got = ops.conv_mlp_eval(x, w1, b1, w2, b2, act_in)
        assert got is not None
        xa = F.gelu(x.double()) if act_in == "gelu" else x.double()
        ref = F.conv1d(F.gelu(F.conv1d(xa, w1.double(), b1.double())), w2.double(), b2.double())
        two = ops.conv1x1(ops.conv1x1(x, w1, b1, act_in), w2, b2, "gelu")
    e = float((got.double() - ref).norm() / ref.norm())
    e2 = float((two.double() - ref).norm() / ref.norm())
    assert e < 2e-6, (e, e2)
    old = os.environ.get("RPDE_CONV_MLP")
    os.environ["RPDE_CONV_MLP"] = "0"
    try:
        assert ops.conv_mlp_eval(x, w1, b1, w2, b2, act_in) is None
    finally:
        if old is None:
            os.environ.pop("RPDE_CONV_MLP")
        else:
            os.environ["RPDE_CONV_MLP"] = old


@pytest.mark.parametrize("shape", [(2, 32, 64, 64, 12, 12, 128, 1), (1, 20, 33, 128, 6, 8, 64, 2), (1, 32, 16, 512, 6, 12, 128, 1),
                                   (3, 32, 40, 192, 5, 9, 100, 3), (2, 17, 5, 64, 2, 3, 24, 4)])
@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_last_block_and_projection_in_one_pass(gpu_device, shape, act):
    """rpde_fnoblock2d_proj_eval_fwd (conv_proj_h2.hip): mlp2(gelu(mlp1(act(SpectralConv2d(x) + bypass(x))))) with the block's
    output never written, against the two-launch sequence it replaces and against float64 (reference models/fno.py:143-150)"""
    from rpde import ops
    B, Co, M, N, m1, m2, Cm, Cq = shape
    Ci = 32
    torch.manual_seed(M + N + Cm)
    x = torch.randn(B, Ci, M, N, device=gpu_device)
    w1 = (torch.rand(Ci, Co, m1, m2, dtype=torch.cfloat) / (Ci * Co)).to(gpu_device)
    w2 = (torch.rand(Ci, Co, m1, m2, dtype=torch.cfloat) / (Ci * Co)).to(gpu_device)
    wc = torch.randn(Co, Ci, 1, 1, device=gpu_device) * 0.2
    bc = torch.randn(Co, device=gpu_device) * 0.1
    p1 = torch.randn(Cm, Co, 1, 1, device=gpu_device) * 0.3
    q1 = torch.randn(Cm, device=gpu_device) * 0.1
    p2 = torch.randn(Cq, Cm, 1, 1, device=gpu_device) * 0.2
    q2 = torch.randn(Cq, device=gpu_device) * 0.1
    with torch.no_grad():
        got = ops.fnoblock2d_proj_eval(x, w1, w2, wc, bc, act, p1, q1, p2, q2)
        assert got is not None
        spec = ops.spectral2d(x, w1, w2)
        h = ops.conv1x1_act_eval(x, wc, bc, spec.clone(), act)
        two = ops.conv1x1(ops.conv1x1(h, p1, q1, "identity"), p2, q2, "gelu")
        xf = torch.fft.rfft2(x.double().cpu())
        o = torch.zeros(B, Co, M, N // 2 + 1, dtype=torch.complex128)
        o[:, :, :m1, :m2] = torch.einsum("bixy,ioxy->boxy", xf[:, :, :m1, :m2], w1.cpu().to(torch.complex128))
        o[:, :, -m1:, :m2] = torch.einsum("bixy,ioxy->boxy", xf[:, :, -m1:, :m2], w2.cpu().to(torch.complex128))
        pre = torch.fft.irfft2(o, s=(M, N)) + torch.nn.functional.conv2d(x.double().cpu(), wc.double().cpu(), bc.double().cpu())
        hr = torch.nn.functional.gelu(pre) if act == "gelu" else torch.relu(pre)
        ref = torch.nn.functional.conv2d(torch.nn.functional.gelu(torch.nn.functional.conv2d(hr, p1.double().cpu(), q1.double().cpu())),
                                         p2.double().cpu(), q2.double().cpu())
    assert got.shape == (B, Cq, M, N)
    assert float((got.cpu().double() - ref).norm() / ref.norm()) < 2e-6
    assert float((got - two).norm() / two.norm()) < 2e-6
    if shape == (2, 17, 5, 64, 2, 3, 24, 4):
        # this entry point's three GEMM-shaped steps in place of the column stage; m2 = 3 -> kp = 4: the padded modes are zeroed
        oldc = os.environ.get("RPDE_COL_FUSED")
        os.environ["RPDE_COL_FUSED"] = "0"
        try:
            with torch.no_grad():
                gemm_leg = ops.fnoblock2d_proj_eval(x, w1, w2, wc, bc, act, p1, q1, p2, q2)
        finally:
            if oldc is None:
                os.environ.pop("RPDE_COL_FUSED")
            else:
                os.environ["RPDE_COL_FUSED"] = oldc
        assert gemm_leg is not None
        assert float((got - gemm_leg).norm() / gemm_leg.norm()) < 2e-6


def test_fused_evaluation_fnoblock2d_narrow_grid_takes_the_two_step_path(gpu_device):
    """N = 32, width 32, 12 modes (the lowest grid of the default all-resolution sweep): the one-pass tail would keep
    32 rows x 24 spectrum entries x 32 channels = 96 KB of LDS beside its weights -- more than a launch gets.  The
    eligibility test must say so (round-3 advisor finding: the launch error made FNO2d evaluation fail hard) and the
    module falls back to spectral op + accumulating convolution."""
    from rpde import ops
    from models.fno_blocks import FNOBlock2d
    torch.manual_seed(2)
    x = torch.randn(2, 32, 32, 32, device=gpu_device)
    blk = FNOBlock2d(32, 32, 12, 12).to(gpu_device).eval()
    w1, w2 = blk.spectral_conv.weights1, blk.spectral_conv.weights2
    with torch.no_grad():
        assert ops.fnoblock2d_eval(x, w1, w2, blk.bypass_conv.weight, blk.bypass_conv.bias, "gelu") is None
        got = blk(x)
        xf = torch.fft.rfft2(x.double().cpu())
        o = torch.zeros(2, 32, 32, 17, dtype=torch.complex128)
        o[:, :, :12, :12] = torch.einsum("bixy,ioxy->boxy", xf[:, :, :12, :12], w1.cpu().to(torch.complex128))
        o[:, :, -12:, :12] = torch.einsum("bixy,ioxy->boxy", xf[:, :, -12:, :12], w2.cpu().to(torch.complex128))
        pre = torch.fft.irfft2(o, s=(32, 32)) + torch.nn.functional.conv2d(x.double().cpu(), blk.bypass_conv.weight.double().cpu(),
                                                                         blk.bypass_conv.bias.double().cpu())
        ref = torch.nn.functional.gelu(pre)
    assert float((got.cpu().double() - ref).norm() / ref.norm()) < 2e-6


# (width-32 shapes with N in {64..512} take the matrix-pipe tail k_conv_syn_h2, the others k_conv1x1_small<.., true>)
@pytest.mark.parametrize("shape", [(2, 32, 32, 64, 64, 12, 12), (1, 8, 6, 48, 256, 5, 9), (2, 4, 4, 16, 1024, 3, 4),
                                   (1, 32, 32, 40, 512, 12, 12), (3, 32, 20, 33, 128, 6, 8), (2, 32, 32, 7, 256, 4, 16),
                                   (5, 32, 9, 3, 64, 2, 3), (3, 32, 32, 300, 256, 6, 8), (2, 32, 17, 515, 128, 3, 5)])
@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_fused_evaluation_fnoblock2d_equals_the_two_step_path(gpu_device, shape, act):
    """rpde_fnoblock2d_eval_fwd (conv_syn_h2.hip / conv_small.hip SYN): act(SpectralConv2d(x) + bypass(x)) in one pass
    against the spectral op followed by the accumulating convolution, and against float64"""
    from rpde import ops
    B, Ci, Co, M, N, m1, m2 = shape
    torch.manual_seed(M + N + Ci)
    x = torch.randn(B, Ci, M, N, device=gpu_device)
    w1 = (torch.rand(Ci, Co, m1, m2, dtype=torch.cfloat) / (Ci * Co)).to(gpu_device)
    w2 = (torch.rand(Ci, Co, m1, m2, dtype=torch.cfloat) / (Ci * Co)).to(gpu_device)
    wc = torch.randn(Co, Ci, 1, 1, device=gpu_device) * 0.2
    bc = torch.randn(Co, device=gpu_device) * 0.1
    with torch.no_grad():
        got = ops.fnoblock2d_eval(x, w1, w2, wc, bc, act)
        assert got is not None
        spec = ops.spectral2d(x, w1, w2)
        two = ops.conv1x1_act_eval(x, wc, bc, spec.clone(), act)
        xf = torch.fft.rfft2(x.double().cpu())
        o = torch.zeros(B, Co, M, N // 2 + 1, dtype=torch.complex128)
        o[:, :, :m1, :m2] = torch.einsum("bixy,ioxy->boxy", xf[:, :, :m1, :m2], w1.cpu().to(torch.complex128))
        o[:, :, -m1:, :m2] = torch.einsum("bixy,ioxy->boxy", xf[:, :, -m1:, :m2], w2.cpu().to(torch.complex128))
        pre = torch.fft.irfft2(o, s=(M, N)) + torch.nn.functional.conv2d(x.double().cpu(), wc.double().cpu(), bc.double().cpu())
        ref = torch.nn.functional.gelu(pre) if act == "gelu" else torch.relu(pre)
    assert float((got.cpu().double() - ref).norm() / ref.norm()) < 2e-6
    assert float((got - two).norm() / two.norm()) < 2e-6
    # the column stage (k_col_analysis + k_col_mix_synthesis) against the three GEMM-shaped steps it replaces
    oldc = os.environ.get("RPDE_COL_FUSED")
    os.environ["RPDE_COL_FUSED"] = "0"
    try:
        with torch.no_grad():
            gemm_leg = ops.fnoblock2d_eval(x, w1, w2, wc, bc, act)
            spec_gemm = ops.spectral2d(x, w1, w2)
    finally:
        if oldc is None:
            os.environ.pop("RPDE_COL_FUSED")
        else:
            os.environ["RPDE_COL_FUSED"] = oldc
    assert float((got - gemm_leg).norm() / gemm_leg.norm()) < 2e-6
    assert float((spec - spec_gemm).norm() / spec_gemm.norm()) < 2e-6
    # samples / rows of very different magnitude: the per-slab scales of the matrix-pipe tail must not leak
    xs = x * torch.logspace(-3, 3, M, device=gpu_device).view(1, 1, M, 1)
    old = os.environ.get("RPDE_CONV_SYN_H2")
    with torch.no_grad():
        a = ops.fnoblock2d_eval(xs, w1, w2, wc, bc, act)
        os.environ["RPDE_CONV_SYN_H2"] = "0"
        try:
            b_ = ops.fnoblock2d_eval(xs, w1, w2, wc, bc, act)
        finally:
            if old is None:
                os.environ.pop("RPDE_CONV_SYN_H2")
            else:
                os.environ["RPDE_CONV_SYN_H2"] = old
    rows = (a - b_).flatten(0, 1).transpose(0, 1).flatten(1).norm(dim=1) / b_.flatten(0, 1).transpose(0, 1).flatten(1).norm(dim=1).clamp_min(1e-30)
    assert float(rows.max()) < 5e-6, float(rows.max())


@pytest.mark.parametrize("B,n,C,K", [(16, 512, 128, 64), (4, 512, 128, 64), (1, 64, 32, 9), (17, 48, 64, 30),
                                     (40, 32, 32, 64), (64, 100, 64, 21), (3, 24, 128, 5)])
def test_few_row_mode_mix_reads_the_weights_in_place(gpu_device, B, n, C, K):
    """mix1d.hip (k_mix1d / k_mix1d_wgrad): the 1-D layer's per-mode channel mixing without the [k][2C][2C] weight
    repack -- forward, data gradient and weight gradient against the float64 restatement of
    models/spectral_convolution.py:158-204 (row tiles of 16 incl. partial ones, mode counts that are no multiple of 8
    or of 4, modes clamped at n/2+1: the unused weight slices must get a zero gradient)."""
    from oracle import reference_path as R
    from rpde import ops
    torch.manual_seed(B * 1000 + C + K)
    x = torch.randn(B, n, C, device=gpu_device, requires_grad=True)
    w = (torch.randn(C, C, K, 2, device=gpu_device) / C ** 0.5).requires_grad_()
    probe = torch.randn(B, n, C, device=gpu_device)
    out = ops.fspectral1d(x, w, K)
    (out * probe).sum().backward()
    xd = x.detach().double().cpu().requires_grad_()
    wd = w.detach().double().cpu().requires_grad_()
    ref = R.fspectral1d_fourier(xd, wd, K)
    (ref * probe.double().cpu()).sum().backward()

    def rel(a, b):
        return float((a.double().cpu() - b).norm() / b.norm().clamp_min(1e-30))

    assert rel(out.detach(), ref.detach()) < 2e-6
    assert rel(x.grad, xd.grad) < 2e-6
    assert rel(w.grad, wd.grad) < 2e-6
    keff = min(K, n // 2 + 1)
    assert not w.grad[:, :, keff:].any()


@pytest.mark.parametrize("out_f,in_f", [(128, 1), (1, 128), (64, 64), (5, 200), (33, 7)])
def test_weight_norm_kernels_match_autograd(gpu_device, out_f, in_f):
    """rpde_weight_norm_fwd / _bwd against the expression the reference's WNLinear evaluates
    (models/custom_layer.py:70-108: torch.nn.utils.weight_norm, w = v * (g / |v|_row)) and its autograd gradient."""
    from rpde import ops
    torch.manual_seed(out_f * 7 + in_f)
    v = torch.randn(out_f, in_f, device=gpu_device, requires_grad=True)
    g = (torch.rand(out_f, 1, device=gpu_device) + 0.5).requires_grad_()
    probe = torch.randn(out_f, in_f, device=gpu_device)
    w = ops.weight_norm(v, g)
    (w * probe).sum().backward()
    vd, gd = v.detach().double().requires_grad_(), g.detach().double().requires_grad_()
    wd = vd * (gd / vd.norm(2, dim=1, keepdim=True))
    (wd * probe.double()).sum().backward()
    assert float((w.detach().double() - wd.detach()).abs().max()) < 1e-6 * float(wd.detach().abs().max())
    # (with one input feature the gradient of v cancels exactly in exact arithmetic: measure against the terms' size)
    size = float((gd.detach() / vd.detach().norm(2, dim=1, keepdim=True) * probe.double()).norm())
    assert float((v.grad.double() - vd.grad).norm()) <= 2e-6 * size
    assert float((g.grad.double() - gd.grad).norm()) <= 2e-6 * float(probe.double().norm())
