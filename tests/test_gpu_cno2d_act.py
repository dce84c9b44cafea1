"""The fused 2-D CNO activation (rpde_cno_act2d_fwd / _bwd, csrc/cno2d.hip) through the C ABI against tests/cno2d_ref.py
in float64, whose per-axis resampling matrices come from F.interpolate on an identity.

Shapes (h_in, w_in) -> (h_mid, w_mid) -> (h_out, w_out): the deepest levels real configurations reach, (1,1)->(2,2)->(1,1),
(1,1)->(2,2)->(2,2), (2,2)->(4,4)->(1,1); (8,8)->(16,16)->(8,8) where every row of every table is a border row; the regular
levels (32,32)->(64,64)->(32,32), (32,32)->(64,64)->(16,16) and (16,16)->(32,32)->(32,32), the last with an
exactly-identity D; and a rectangular plane with non-integer ratios and varying tap counts, (24,20)->(32,32)->(16,12).
All of these fit a workgroup whole and are packed C2_PACK_WORK / (h_mid w_mid) = 4096 / (h_mid w_mid) planes to one
(fewer where the LDS, whose rows are padded to whole float4s, holds fewer: 480 planes of 1 x 1, 240 of 2 x 2); B * C is chosen just above one pack and not a multiple of it, so the last workgroup
is ragged.

Tiled planes: the kernels tile the written plane (the output in the forward, the input in the backward) 32 x 32 points
at a time where out = in, so (80,80)->(160,160)->(80,80) is two full tiles and a ragged third of 16 in each direction
on the 16-byte path, and (75,77)->(150,154)->(75,77) two full tiles and a ragged third of 11 rows and 13 columns on the
4-byte path.  Where the mid plane is four times the output, (72,72)->(144,144)->(36,36), the forward's tile is halved to
16 x 16 (two full tiles and a ragged third of 4) while the backward keeps 32 x 32 (two and a ragged third of 8).  The
test asserts these tile sizes through rpde_cno_act2d_plan.  B * C is 3, 3 and 2 planes there.

Each case runs with and without the per-channel affine prologue, at slope 0.01, output buffers pre-filled with NaN.

Bounds: forward rel-L2 <= 1e-5, gradient <= 2e-5 (the project's budgets, README.md).  The LeakyReLU kink: before the
gradients are compared the test asserts in float64 that no mid pre-activation lies within 1e-5 of its rms from zero
(the seeds below were chosen on the CPU, for the reference alone, so that it holds), so the derivative is the same on
both sides at every point.  It is a condition of the test, not a tolerance.

Measured on an MI355X, worst over all cases: forward rel-L2 8.5e-8 (at (32,32)->(64,64)->(16,16), no prologue), gradient
9.8e-8 (at (2,2)->(4,4)->(1,1), zero input); smallest kink margin 1.2e-5 rms (the 75 x 77 planes, no prologue).
"""
import ctypes

import pytest
import torch

from tests import cno2d_ref

pytestmark = pytest.mark.gpu

SLOPE = 0.01
FWD_TOL, GRAD_TOL = 1e-5, 2e-5
KINK_MARGIN = 1e-5

# ((h_in, w_in), (h_mid, w_mid), (h_out, w_out)) -> seed for which the randn input keeps every mid pre-activation off the
# kink, with and without the prologue
CASES = {
    ((1, 1), (2, 2), (1, 1)): 0, ((1, 1), (2, 2), (2, 2)): 0, ((2, 2), (4, 4), (1, 1)): 0, ((8, 8), (16, 16), (8, 8)): 0,
    ((32, 32), (64, 64), (32, 32)): 0, ((32, 32), (64, 64), (16, 16)): 0, ((16, 16), (32, 32), (32, 32)): 0,
    ((24, 20), (32, 32), (16, 12)): 0,
    ((80, 80), (160, 160), (80, 80)): 3, ((75, 77), (150, 154), (75, 77)): 0, ((72, 72), (144, 144), (36, 36)): 1,
}
# the tiled cases: planes B * C, and the (th, tw) the forward / the backward use
TILED = {
    ((80, 80), (160, 160), (80, 80)): ((1, 3), (32, 32), (32, 32)),
    ((75, 77), (150, 154), (75, 77)): ((3, 1), (32, 32), (32, 32)),
    ((72, 72), (144, 144), (36, 36)): ((1, 2), (16, 16), (32, 32)),
}
_WORST = {"fwd": [0.0, None], "bwd": [0.0, None], "margin": [float("inf"), None]}


def _id(shape):
    return "-".join("x".join(map(str, s)) for s in shape)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for k, (e, where) in _WORST.items():
        print(f"\n[cno2d_act] worst {k} {e:.3e} (at {where})")


def plan(shape, backward, B=1, C=1 << 20):
    """(th, tw, pack) the kernels use for the shape (no device needed)"""
    from rpde import _lib
    lib = _lib.load()
    th, tw, pack = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    (hi, wi), (hm, wm), (ho, wo) = shape
    _lib.check(lib.rpde_cno_act2d_plan(int(backward), B, C, hi, wi, hm, wm, ho, wo, ctypes.byref(th), ctypes.byref(tw),
                                       ctypes.byref(pack)), "plan")
    return th.value, tw.value, pack.value


def batch_of(shape):
    """(B, C): the tiled planes as listed; whole planes just above one pack of them, the last workgroup ragged"""
    if shape in TILED:
        return TILED[shape][0]
    pack = plan(shape, False)[2]
    B = 3 if pack % 3 else 2
    return B, max(2, pack // B + 1)


def inputs(shape, affine, seed, zero=False):
    """fp32 CPU tensors x, g, scale, shift"""
    (hi, wi), _, (ho, wo) = shape
    B, C = batch_of(shape)
    gen = torch.Generator().manual_seed(1000 * seed + 23)
    x = torch.randn(B, C, hi, wi, generator=gen)
    g = torch.randn(B, C, ho, wo, generator=gen)
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
    if (e < _WORST[kind][0]) if kind == "margin" else (e > _WORST[kind][0]):
        _WORST[kind][0], _WORST[kind][1] = e, where


def _band(t):
    from rpde import _lib
    return t.span.data_ptr(), _lib.ptr(t.weights), t.taps


def _tables(dev, shape):
    from rpde import ops
    (hi, wi), (hm, wm), (ho, wo) = shape
    return (ops.cno_tables(dev, hi, hm), ops.cno_tables(dev, wi, wm), ops.cno_tables(dev, hm, ho), ops.cno_tables(dev, wm, wo))


def _fwd(x, scale, shift, shape, slope=SLOPE):
    from rpde import _lib
    lib = _lib.load()
    B, C = x.shape[:2]
    (hi, wi), (hm, wm), (ho, wo) = shape
    Uy, Ux, Dy, Dx = _tables(x.device, shape)
    out = torch.full((B, C, ho, wo), float("nan"), device=x.device)
    _lib.check(lib.rpde_cno_act2d_fwd(_lib.ptr(x), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(out), B, C, hi, wi, hm, wm, ho, wo,
                                      slope, *_band(Uy.fwd), *_band(Ux.fwd), *_band(Dy.fwd), *_band(Dx.fwd), _lib.stream_ptr()),
               "fwd")
    return out


def _bwd(x, scale, shift, g, shape, slope=SLOPE):
    from rpde import _lib
    lib = _lib.load()
    B, C = x.shape[:2]
    (hi, wi), (hm, wm), (ho, wo) = shape
    Uy, Ux, Dy, Dx = _tables(x.device, shape)
    gy = torch.full((B, C, hi, wi), float("nan"), device=x.device)
    _lib.check(lib.rpde_cno_act2d_bwd(_lib.ptr(x), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(g), _lib.ptr(gy), B, C, hi, wi,
                                      hm, wm, ho, wo, slope, *_band(Uy.fwd), *_band(Ux.fwd), *_band(Uy.bwd), *_band(Ux.bwd),
                                      *_band(Dy.bwd), *_band(Dx.bwd), _lib.stream_ptr()), "bwd")
    return gy


def _dev(t, dev):
    return None if t is None else t.to(dev)


@pytest.mark.parametrize("shape", list(TILED), ids=_id)
def test_tiled_cases_use_the_stated_tiles(shape):
    (B, C), fwd_tile, bwd_tile = TILED[shape]
    assert plan(shape, False, B, C) == fwd_tile + (1,)
    assert plan(shape, True, B, C) == bwd_tile + (1,)
    for (th, tw), (H, W) in ((fwd_tile, shape[2]), (bwd_tile, shape[0])):      # two full tiles and a ragged third
        assert 2 * th < H < 3 * th and 2 * tw < W < 3 * tw


@pytest.mark.parametrize("shape", [s for s in CASES if s not in TILED], ids=_id)
def test_whole_planes_are_packed(shape):
    for backward in (False, True):
        th, tw, pack = plan(shape, backward)
        assert (th, tw) == (shape[0] if backward else shape[2])
        assert 1 <= pack <= max(1, 4096 // (shape[1][0] * shape[1][1]))
    B, C = batch_of(shape)
    pack = plan(shape, False)[2]
    assert B * C > pack and (pack == 1 or (B * C) % pack != 0)
    if shape[1] == (4, 4) or shape[1] == (2, 2):                # the smallest planes do not cost a workgroup each
        assert pack >= 128


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("shape", list(CASES), ids=_id)
def test_forward_and_backward_match_float64(gpu_device, shape, affine):
    x, g, scale, shift = inputs(shape, affine, CASES[shape])
    ref, u = cno2d_ref.act_parts(x, shape[1], shape[2], SLOPE, scale, shift)
    margin = cno2d_ref.min_margin(u)
    assert margin >= KINK_MARGIN, f"unsuitable input: a mid pre-activation {margin:.2e} rms from the kink; pick another seed"
    ref_gy = cno2d_ref.act_bwd(x, g, shape[1], SLOPE, scale, shift)
    xd, gd, sc, sh = (_dev(t, gpu_device) for t in (x, g, scale, shift))

    out = _fwd(xd, sc, sh, shape)
    gy = _bwd(xd, sc, sh, gd, shape)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gy).all())
    e, eg = _rel(out, ref), _rel(gy, ref_gy)
    print(f"{_id(shape)} B,C={batch_of(shape)} affine={affine}: fwd rel-L2 {e:.3e}, bwd rel-L2 {eg:.3e}, kink margin {margin:.1e}")
    _note("fwd", e, (_id(shape), affine))
    _note("bwd", eg, (_id(shape), affine))
    _note("margin", margin, (_id(shape), affine))
    assert e <= FWD_TOL and eg <= GRAD_TOL
    # the same inputs give the same bits
    assert torch.equal(out, _fwd(xd, sc, sh, shape))
    assert torch.equal(gy, _bwd(xd, sc, sh, gd, shape))


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("shape", [((2, 2), (4, 4), (1, 1)), ((32, 32), (64, 64), (16, 16)), ((24, 20), (32, 32), (16, 12)),
                                   ((75, 77), (150, 154), (75, 77))], ids=_id)
def test_zero_input_takes_the_slope_branch(gpu_device, shape, affine):
    """u == 0 everywhere: out is exactly zero and the derivative is slope (torch's convention), gy = slope U^T D^T g"""
    x, g, scale, shift = inputs(shape, affine, 1, zero=True)
    ref_gy = SLOPE * cno2d_ref.resample_t(cno2d_ref.resample_t(g.double(), shape[1]), shape[0])
    xd, gd, sc, sh = (_dev(t, gpu_device) for t in (x, g, scale, shift))
    out = _fwd(xd, sc, sh, shape)
    gy = _bwd(xd, sc, sh, gd, shape)
    assert bool((out == 0).all())
    eg = _rel(gy, ref_gy)
    print(f"{_id(shape)} zero input, affine={affine}: bwd rel-L2 {eg:.3e}")
    _note("bwd", eg, (_id(shape), affine, "zero"))
    assert eg <= GRAD_TOL


def test_autograd_function_matches_the_abi(gpu_device):
    """rpde.ops.cno_act2d: same bits as the entry points, the gradient is the one with respect to the affine's output"""
    from rpde import ops
    shape = ((24, 20), (32, 32), (16, 16))
    gen = torch.Generator().manual_seed(5)
    x, g = torch.randn(2, 3, 24, 20, generator=gen), torch.randn(2, 3, 16, 16, generator=gen)
    scale, shift = 0.5 + torch.rand(3, generator=gen), 0.3 * torch.randn(3, generator=gen)
    xd, gd, sc, sh = (t.to(gpu_device) for t in (x, g, scale, shift))
    xr = xd.clone().requires_grad_(True)
    out = ops.cno_act2d(xr, 16, 16, sc, sh)
    out.backward(gd)
    assert torch.equal(out.detach(), _fwd(xd, sc, sh, shape))
    assert torch.equal(xr.grad, _bwd(xd, sc, sh, gd, shape))
    with pytest.raises(ValueError):
        ops.cno_act2d(xd, 16, 16, sc, None)
    with pytest.raises(ValueError):
        ops.cno_act2d(xd[0], 16, 16)


def test_bad_arguments_are_refused(gpu_device):
    from rpde import _lib
    lib = _lib.load()
    x = torch.zeros(2, 3, 16, 16, device=gpu_device)
    out = torch.zeros(2, 3, 16, 16, device=gpu_device)
    v = torch.ones(3, device=gpu_device)
    shape = ((16, 16), (32, 32), (16, 16))
    Uy, Ux, Dy, Dx = _tables(x.device, shape)
    u, d = _band(Uy.fwd), _band(Dy.fwd)
    ut, dt = _band(Uy.bwd), _band(Dy.bwd)
    px, po, pv, st = _lib.ptr(x), _lib.ptr(out), _lib.ptr(v), _lib.stream_ptr()
    S = (16, 16, 32, 32, 16, 16)

    def refused(status, word):
        assert status == _lib.ERR_ARG
        assert word in lib.rpde_last_error().decode(), lib.rpde_last_error()

    fwd, bwd = lib.rpde_cno_act2d_fwd, lib.rpde_cno_act2d_bwd
    refused(fwd(None, None, None, po, 2, 3, *S, SLOPE, *u, *u, *d, *d, st), "null")
    refused(fwd(px, None, None, None, 2, 3, *S, SLOPE, *u, *u, *d, *d, st), "null")
    refused(fwd(px, None, None, po, 2, 3, 16, 16, 32, 0, 16, 16, SLOPE, *u, *u, *d, *d, st), "bad sizes")
    refused(fwd(px, None, None, po, 2, 3, 0, 16, 32, 32, 16, 16, SLOPE, *u, *u, *d, *d, st), "bad sizes")
    refused(fwd(px, pv, None, po, 2, 3, *S, SLOPE, *u, *u, *d, *d, st), "come together")
    refused(fwd(px, None, None, po, 2, 3, *S, SLOPE, *u, u[0], u[1], 3, *d, *d, st), "taps")
    refused(fwd(px, None, None, po, 2, 3, *S, SLOPE, *u, *u, *d, None, d[1], d[2], st), "null D_x table")
    # 65536 x 65536 mid points onto 16 x 16 outputs: the sources of four outputs do not fit a workgroup
    refused(fwd(px, None, None, po, 2, 3, 16, 16, 1 << 16, 1 << 16, 16, 16, SLOPE, *u, *u, *d, *d, st), "does not fit")
    assert "65536" in lib.rpde_last_error().decode()            # the message names the sizes
    refused(bwd(px, None, None, None, po, 2, 3, *S, SLOPE, *u, *u, *ut, *ut, *dt, *dt, st), "null")
    refused(bwd(px, None, pv, po, po, 2, 3, *S, SLOPE, *u, *u, *ut, *ut, *dt, *dt, st), "come together")
    refused(bwd(px, None, None, po, po, 2, 3, *S, SLOPE, *u, *u, *ut, ut[0], ut[1], 6, *dt, *dt, st), "taps")
    refused(bwd(px, None, None, po, po, 2, 3, 16, 16, 1 << 16, 1 << 16, 16, 16, SLOPE, *u, *u, *ut, *ut, *dt, *dt, st),
            "does not fit")
    torch.cuda.synchronize()
