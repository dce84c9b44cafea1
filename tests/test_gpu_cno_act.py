"""The fused CNO activation (rpde_cno_act1d_fwd / _bwd, csrc/cno.hip) through the C ABI against tests/cno_ref.py in
float64, whose resampling matrices come from F.interpolate on an identity.

Shapes (n_in, n_mid, n_out): the deepest levels real configurations reach (1, 2, 1), (1, 2, 2), (2, 4, 1); (8, 16, 8)
where every row of both tables is a border row; the regular levels (32, 64, 32), (32, 64, 16), (16, 32, 32) -- the last
with an exactly-identity D; non-integer ratios with varying tap counts (24, 32, 16), (20, 32, 12); and rows of 2500 and
2501 points: the kernel tiles long rows CNO_TILE = 1024 written points at a time (halved to 512 where n_mid is four
times n_out), so these are two full tiles and a ragged third (the forward of the second: two of 512 and a ragged
third), once on the 16-byte path and once, with odd lengths, on the 4-byte path.  Short rows are packed
CNO_PACK_WORK / n_mid = 2048 / n_mid to a workgroup; B * C is chosen just above one pack and not a multiple of it, so the
last workgroup is ragged.  Each case runs with and without the per-channel affine prologue, at slope 0.01.

Bounds: forward rel-L2 <= 1e-5, gradient <= 2e-5 (the project's budgets, README.md).  The LeakyReLU kink: for the randn
gradient cases the test first asserts in float64 that no mid pre-activation lies within 1e-5 of its rms from zero (the
seeds below were chosen on the CPU so that it holds), so the derivative is the same on both sides at every point.

Measured on an MI355X, worst over all cases: forward rel-L2 8.0e-8 (at (32, 64, 16), no prologue), gradient 6.8e-8 (at
(2, 4, 1), zero input); smallest kink margin 3.5e-5 rms (the 2500-point rows).
"""
import pytest
import torch

from tests import cno_ref

pytestmark = pytest.mark.gpu

SLOPE = 0.01
FWD_TOL, GRAD_TOL = 1e-5, 2e-5
CNO_TILE, CNO_PACK_WORK = 1024, 2048
KINK_MARGIN = 1e-5

# (n_in, n_mid, n_out) -> seed for which the randn input keeps every mid pre-activation off the kink, with and without
# the prologue
CASES = {
    (1, 2, 1): 0, (1, 2, 2): 0, (2, 4, 1): 0, (8, 16, 8): 0,
    (32, 64, 32): 0, (32, 64, 16): 0, (16, 32, 32): 0,
    (24, 32, 16): 1, (20, 32, 12): 0,
    (2500, 5000, 2500): 36, (2501, 5002, 1251): 24,
}
_WORST = {"fwd": [0.0, None], "bwd": [0.0, None]}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for k, (e, where) in _WORST.items():
        print(f"\n[cno_act] worst {k} rel-L2 {e:.3e} (at {where})")


def batch_of(shape):
    """(B, C): long rows as B = 3, C = 5; short rows just above one pack of rows, the last workgroup ragged"""
    n_in, n_mid, n_out = shape
    if n_mid > CNO_PACK_WORK:
        return 3, 5
    return 3, CNO_PACK_WORK // n_mid // 3 + 2


def inputs(shape, affine, seed, zero=False):
    """fp32 CPU tensors x, g, scale, shift"""
    n_in, n_mid, n_out = shape
    B, C = batch_of(shape)
    gen = torch.Generator().manual_seed(1000 * seed + 17)
    x = torch.randn(B, C, n_in, generator=gen)
    g = torch.randn(B, C, n_out, generator=gen)
    scale = shift = None
    if affine:
        scale = 0.5 + torch.rand(C, generator=gen)
        shift = torch.zeros(C) if zero else 0.3 * torch.randn(C, generator=gen)
    if zero:
        x = torch.zeros_like(x)
    return x, g, scale, shift


def _rel(got, ref):
    return float((got.double().cpu() - ref).norm() / ref.norm())


def _note(kind, e, where):
    if e > _WORST[kind][0]:
        _WORST[kind][0], _WORST[kind][1] = e, where


def _fwd(x, scale, shift, n_mid, n_out, slope=SLOPE):
    from rpde import _lib, ops
    lib = _lib.load()
    B, C, n_in = x.shape
    U, D = ops.cno_tables(x.device, n_in, n_mid), ops.cno_tables(x.device, n_mid, n_out)
    out = torch.full((B, C, n_out), float("nan"), device=x.device)
    _lib.check(lib.rpde_cno_act1d_fwd(_lib.ptr(x), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(out), B, C, n_in, n_mid, n_out,
                                      slope, U.fwd.span.data_ptr(), _lib.ptr(U.fwd.weights), U.fwd.taps,
                                      D.fwd.span.data_ptr(), _lib.ptr(D.fwd.weights), D.fwd.taps, _lib.stream_ptr()), "fwd")
    return out


def _bwd(x, scale, shift, g, n_mid, slope=SLOPE):
    from rpde import _lib, ops
    lib = _lib.load()
    B, C, n_in = x.shape
    n_out = g.shape[-1]
    U, D = ops.cno_tables(x.device, n_in, n_mid), ops.cno_tables(x.device, n_mid, n_out)
    gy = torch.full((B, C, n_in), float("nan"), device=x.device)
    _lib.check(lib.rpde_cno_act1d_bwd(_lib.ptr(x), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(g), _lib.ptr(gy), B, C, n_in,
                                      n_mid, n_out, slope, U.fwd.span.data_ptr(), _lib.ptr(U.fwd.weights), U.fwd.taps,
                                      U.bwd.span.data_ptr(), _lib.ptr(U.bwd.weights), U.bwd.taps,
                                      D.bwd.span.data_ptr(), _lib.ptr(D.bwd.weights), D.bwd.taps, _lib.stream_ptr()), "bwd")
    return gy


def _dev(t, dev):
    return None if t is None else t.to(dev)


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("shape", list(CASES), ids=["-".join(map(str, s)) for s in CASES])
def test_forward_and_backward_match_float64(gpu_device, shape, affine):
    n_in, n_mid, n_out = shape
    x, g, scale, shift = inputs(shape, affine, CASES[shape])
    ref, u = cno_ref.act_parts(x, n_mid, n_out, SLOPE, scale, shift)
    margin = cno_ref.min_margin(u)
    assert margin >= KINK_MARGIN, f"unsuitable input: a mid pre-activation {margin:.2e} rms from the kink; pick another seed"
    ref_gy = cno_ref.act_bwd(x, g, n_mid, n_out, SLOPE, scale, shift)
    xd, gd, sc, sh = (_dev(t, gpu_device) for t in (x, g, scale, shift))

    out = _fwd(xd, sc, sh, n_mid, n_out)
    gy = _bwd(xd, sc, sh, gd, n_mid)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gy).all())
    e, eg = _rel(out, ref), _rel(gy, ref_gy)
    print(f"{shape} B,C={batch_of(shape)} affine={affine}: fwd rel-L2 {e:.3e}, bwd rel-L2 {eg:.3e}, kink margin {margin:.1e}")
    _note("fwd", e, (shape, affine))
    _note("bwd", eg, (shape, affine))
    assert e <= FWD_TOL and eg <= GRAD_TOL
    # the same inputs give the same bits
    assert torch.equal(out, _fwd(xd, sc, sh, n_mid, n_out))
    assert torch.equal(gy, _bwd(xd, sc, sh, gd, n_mid))


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("shape", [(2, 4, 1), (32, 64, 16), (20, 32, 12), (2500, 5000, 2500)],
                         ids=lambda s: "-".join(map(str, s)))
def test_zero_input_takes_the_slope_branch(gpu_device, shape, affine):
    """u == 0 everywhere: out is exactly zero and the derivative is slope (torch's convention), gy = slope U^T D^T g"""
    n_in, n_mid, n_out = shape
    x, g, scale, shift = inputs(shape, affine, 1, zero=True)
    U, D = cno_ref.resample_matrix(n_in, n_mid), cno_ref.resample_matrix(n_mid, n_out)
    ref_gy = SLOPE * ((g.double() @ D) @ U)
    xd, gd, sc, sh = (_dev(t, gpu_device) for t in (x, g, scale, shift))
    out = _fwd(xd, sc, sh, n_mid, n_out)
    gy = _bwd(xd, sc, sh, gd, n_mid)
    assert bool((out == 0).all())
    eg = _rel(gy, ref_gy)
    print(f"{shape} zero input, affine={affine}: bwd rel-L2 {eg:.3e}")
    _note("bwd", eg, (shape, affine, "zero"))
    assert eg <= GRAD_TOL


def test_autograd_function_matches_the_abi(gpu_device):
    """rpde.ops.cno_act1d: same bits as the entry points, the gradient is the one with respect to the affine's output"""
    from rpde import ops
    shape = (24, 32, 16)
    x, g, scale, shift = inputs(shape, True, CASES[shape])
    xd, gd, sc, sh = (t.to(gpu_device) for t in (x, g, scale, shift))
    xr = xd.clone().requires_grad_(True)
    out = ops.cno_act1d(xr, 16, 16, sc, sh)
    out.backward(gd)
    assert torch.equal(out.detach(), _fwd(xd, sc, sh, 32, 16))
    assert torch.equal(xr.grad, _bwd(xd, sc, sh, gd, 32))
    with pytest.raises(ValueError):
        ops.cno_act1d(xd, 16, 16, sc, None)
    with pytest.raises(ValueError):
        ops.cno_act1d(xd[0], 16, 16)


def test_bad_arguments_are_refused(gpu_device):
    from rpde import _lib, ops
    lib = _lib.load()
    x = torch.zeros(2, 3, 16, device=gpu_device)
    out = torch.zeros(2, 3, 16, device=gpu_device)
    v = torch.ones(3, device=gpu_device)
    U, D = ops.cno_tables(x.device, 16, 32), ops.cno_tables(x.device, 32, 16)
    u = (U.fwd.span.data_ptr(), _lib.ptr(U.fwd.weights), U.fwd.taps)
    d = (D.fwd.span.data_ptr(), _lib.ptr(D.fwd.weights), D.fwd.taps)
    ut = (U.bwd.span.data_ptr(), _lib.ptr(U.bwd.weights), U.bwd.taps)
    dt = (D.bwd.span.data_ptr(), _lib.ptr(D.bwd.weights), D.bwd.taps)
    px, po, pv, st = _lib.ptr(x), _lib.ptr(out), _lib.ptr(v), _lib.stream_ptr()

    def refused(status, word):
        assert status == _lib.ERR_ARG
        assert word in lib.rpde_last_error().decode(), lib.rpde_last_error()

    refused(lib.rpde_cno_act1d_fwd(None, None, None, po, 2, 3, 16, 32, 16, SLOPE, *u, *d, st), "null")
    refused(lib.rpde_cno_act1d_fwd(px, None, None, po, 2, 3, 16, 0, 16, SLOPE, *u, *d, st), "bad sizes")
    refused(lib.rpde_cno_act1d_fwd(px, pv, None, po, 2, 3, 16, 32, 16, SLOPE, *u, *d, st), "come together")
    refused(lib.rpde_cno_act1d_fwd(px, None, None, po, 2, 3, 16, 32, 16, SLOPE, u[0], u[1], 3, *d, st), "taps")
    refused(lib.rpde_cno_act1d_fwd(px, None, None, po, 2, 3, 16, 32, 16, SLOPE, *u, None, d[1], d[2], st), "null D table")
    # 65536 mid points onto 16 outputs: the sources of one line of outputs do not fit a workgroup
    refused(lib.rpde_cno_act1d_fwd(px, None, None, po, 2, 3, 16, 1 << 16, 16, SLOPE, *u, *d, st), "do not fit")
    refused(lib.rpde_cno_act1d_bwd(px, None, None, None, po, 2, 3, 16, 32, 16, SLOPE, *u, *ut, *dt, st), "null")
    refused(lib.rpde_cno_act1d_bwd(px, None, pv, po, po, 2, 3, 16, 32, 16, SLOPE, *u, *ut, *dt, st), "come together")
    refused(lib.rpde_cno_act1d_bwd(px, None, None, po, po, 2, 3, 16, 32, 16, SLOPE, *u, ut[0], ut[1], 6, *dt, st), "taps")
    refused(lib.rpde_cno_act1d_bwd(px, None, None, po, po, 2, 3, 1 << 16, 32, 16, SLOPE, *u, *ut, *dt, st), "does not fit")
    torch.cuda.synchronize()
