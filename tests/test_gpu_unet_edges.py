"""The U-Net kernels past one workgroup, one slice and one tile, on the GPU against float64 (tests/unet_ref.py); the
shapes of tests/test_gpu_unet_layers.py all fit inside one unit of every decomposition the kernels use.
tests/test_unet_edges_ref_cpu.py proves without a device that the shapes below land where this text says.

* tanh_pool over two to nine workgroups of 256 patches, both ranks and both access widths: a ragged last workgroup, a
  workgroup boundary inside a row and inside a plane, a trailing odd row / column, an exact multiple of 256.  Forward
  1e-5, gradient 2e-5; the pooled output is a selection from the kernel's own act, so it equals torch's MaxPool of that
  act exactly.  The tie test of the layer file again at three of these shapes.  A tensor at a storage offset of one float
  (W % 4 == 0, the pointer not 16-byte aligned) takes the 4-byte kernel and gives the aligned run's bits.  A plane of one
  row passes through without pooling.
* the backward's argmax through the C ABI on operands that make every product exact (act a multiple of 1/4, integer
  gradients): gy equals the float64 formula bit for bit, windows with a late single maximum, a shared maximum and one
  value throughout included.  The same entries in guarded buffers: no word outside a tensor is written.
* norm_tanh (BatchNorm) and groupnorm_tanh, the layer file's tests at shapes of several workgroups.
* upconv's weight gradient over 2, 3 and 7 slices (a slice of 257 points, a boundary at the batch boundary, inside a
  plane and inside a row, a shorter last slice), with and without bias: integer operands give y, dx, dw, db bit-equal to
  float64; random operands meet the budgets and repeat to the bit.  The weight gradient again through the C ABI with
  guard words behind x and g: a point loop that runs past the last point adds them in.  The same for Conv2d(k = 3),
  whose slices are whole image rows: a short last slice, and a last slice that starts past the last row and must
  contribute zeros.
* upconv and Conv(k = 3) at the shipped channel counts on a few points (1024 -> 512: 32 row tiles and 64 K steps of
  k_unet_upconv, a 256 x 128 grid of k_wgrad_sliced), and Conv1d's point loop over four and eight trips: budgets on
  random operands; on integer operands dw and db (fmaf chains, fixed-order sums) are bit-equal to float64.
* UNet2d at width 16 and UNet1d at width 32 (BatchNorm and GroupNorm), one training step against the float64
  stock_forward of tests/unet_ref.py: per tensor max(budget, 3 x floor), the floor being the float32 CPU stock run's own
  distance from float64.

Measured on an MI355X, worst rel-L2 per group: tanh_pool act 3.1e-8, pooled 3.0e-8, gy 6.4e-8, one row act 2.9e-8, gy
5.0e-8; norm_tanh (BatchNorm) act 4.1e-8, pooled 4.1e-8, dz 7.6e-8, dgamma 1.2e-7, dbeta 8.3e-8, running mean 7.0e-8,
running variance 5.1e-8; groupnorm_tanh act 4.0e-8, pooled 3.9e-8, dz 6.6e-8, dgamma 1.5e-7, dbeta 8.9e-8; upconv over
several slices y 6.0e-8, dx 8.3e-8, dw 1.1e-7, db 2.0e-7, at the shipped channel counts y 5.8e-7, dx 7.9e-7, dw 4.6e-8,
db 5.8e-8; conv_k3 y 3.9e-7, dx 4.0e-7, dw 9.4e-8, db 1.4e-7; the models' worst tensor (its floor; y): UNet2d 32 x 32
2.6e-6 (3.1e-6; 3.6e-7), 32 x 48 2.8e-6 (3.3e-6; 3.6e-7), UNet1d BatchNorm 3.6e-6 (3.1e-6; 8.3e-7), GroupNorm 2.2e-6
(1.6e-6; 6.9e-7), the worst floor of any tensor 4.7e-6; every exact comparison (pooled against act, ties, misaligned
runs, the argmax, integer operands, second runs, guard zones) without a differing element.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests import test_gpu_unet_layers as L
from tests import unet_ref as R
from tests.golden import synth

pytestmark = pytest.mark.gpu

FWD, GRAD = 1e-5, 2e-5

# shape -> patches (threads) of the launch; 256 make a workgroup
TP_EDGE = {(3, 5, 67): 510, (2, 7, 100): 350, (2, 3, 11, 18): 324, (2, 3, 11, 19): 360, (3, 3, 11, 24): 324,
           (4, 6, 16, 48): 2304}
TIE_SHAPES = [(3, 5, 67), (2, 3, 11, 19), (4, 6, 16, 48)]
MISALIGNED = [(2, 3, 8, 16), (2, 4, 64)]
ONE_ROW = [(2, 3, 1, 10), (2, 3, 1, 8)]
ARGMAX_SHAPES = [(3, 5, 67), (2, 3, 11, 19), (3, 3, 11, 24)]
BN_SHAPES = [(3, 5, 67), (3, 3, 11, 24)]
GN_CASES = [((3, 8, 67), 4), ((3, 8, 10, 14), 4), ((2, 8, 8, 24), 2)]

# (rank, B, Cin, Cout, H, W) -> (slices, points per slice) of the weight gradient
UP_SLICED = {(1, 3, 5, 6, 1, 171): (2, 257), (1, 2, 4, 4, 1, 300): (2, 300), (1, 4, 8, 4, 1, 500): (7, 286),
             (2, 3, 5, 6, 13, 17): (2, 332), (2, 1, 4, 4, 25, 40): (3, 334)}
UP_WIDE = [(2, 1, 512, 256, 2, 2), (2, 1, 1024, 512, 1, 2), (1, 2, 1024, 512, 1, 2)]
# (B, Cin, Cout, *sizes)
CONV_1D = [(3, 5, 6, 300), (2, 8, 8, 1024), (2, 1024, 512, 4)]
CONV_2D = [(2, 512, 256, 2, 2)]
# (B, Cin, Cout, H, W) -> (slices, image rows per slice) of Conv2d(k = 3)'s weight gradient
CONV_SLICED = {(3, 5, 6, 33, 20): (7, 15), (3, 5, 6, 3, 180): (6, 2)}
# (kind, constructor arguments, input, seed); of the seeds 0 .. 5 the one with the lowest worst floor (1.7e-6 to 3.6e-6
# where they were scanned, 3.1e-6 to 8.1e-6 over all six): the condition floor <= 1e-5 keeps a margin on another host
MODELS = [("UNet2d", dict(in_channels=3, out_channels=2, width=16), (2, 3, 32, 32), 0),
          ("UNet2d", dict(in_channels=3, out_channels=2, width=16), (2, 3, 32, 48), 4),
          ("UNet1d", dict(in_channels=2, out_channels=1, width=32), (4, 2, 64), 1),
          ("UNet1d", dict(in_channels=2, out_channels=1, width=32, use_groupnorm=True), (4, 2, 64), 3)]

_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for k, (e, where) in sorted(_WORST.items()):
        print(f"\n[unet_edges] worst {k} {e:.3e} (at {where})")


def _note(errs, prefix, where):
    for k, e in errs.items():
        if e > _WORST.get(f"{prefix} {k}", (0.0, None))[0]:
            _WORST[f"{prefix} {k}"] = (e, where)


def _opt(t, f):
    return None if t is None else f(t)


# ---- 1. tanh_pool across workgroups -----------------------------------------------------------------------------------
@pytest.mark.parametrize("use", ["pool", "act", "both"])
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("shape", list(TP_EDGE))
def test_tanh_pool_across_workgroups(gpu_device, shape, affine, use):
    from rpde import ops
    dev, seed = gpu_device, 700 + len(shape)
    z = synth.rand_tensor(shape, seed, "z")
    scale = 1.0 + 0.3 * synth.rand_tensor((shape[1],), seed, "scale") if affine else None
    shift = 0.2 * synth.rand_tensor((shape[1],), seed, "shift") if affine else None
    g_act = synth.rand_tensor(shape, seed, "g_act") if use != "pool" else None
    g_pool = synth.rand_tensor(R.pool_shape(shape), seed, "g_pool") if use != "act" else None

    z64 = z.double().requires_grad_(True)
    act64, pool64 = R.tanh_pool(z64, _opt(scale, torch.Tensor.double), _opt(shift, torch.Tensor.double))
    R.loss_of(act64, pool64, _opt(g_act, torch.Tensor.double), _opt(g_pool, torch.Tensor.double)).backward()
    # the op returns the gradient with respect to scale z + shift: the caller owns the affine's chain rule
    gy64 = z64.grad if scale is None else z64.grad / scale.double().view((1, -1) + (1,) * (len(shape) - 2))

    zg = z.to(dev).requires_grad_(True)
    act, pooled = ops.tanh_pool(zg, _opt(scale, lambda t: t.to(dev)), _opt(shift, lambda t: t.to(dev)), pool=True)
    R.loss_of(act, pooled, _opt(g_act, lambda t: t.to(dev)), _opt(g_pool, lambda t: t.to(dev))).backward()
    errs = dict(act=R.rel_l2(act, act64), pooled=R.rel_l2(pooled, pool64), gy=R.rel_l2(zg.grad, gy64))
    print(f"tanh_pool {shape} affine={affine} use={use}: {errs}")
    _note(errs, "tanh_pool", shape)
    assert tuple(pooled.shape) == R.pool_shape(shape)
    assert errs["act"] <= FWD and errs["pooled"] <= FWD and errs["gy"] <= GRAD
    assert torch.equal(pooled.detach().cpu(), R.max_pool(act.detach().cpu()))     # a selection from act: exact


@pytest.mark.parametrize("shape", TIE_SHAPES)
def test_ties_scatter_as_torch_does_across_workgroups(gpu_device, shape):
    L.test_ties_scatter_as_torch_does(gpu_device, shape)


def _at_offset(t: torch.Tensor, device, floats: int = 1) -> torch.Tensor:
    """t's values on the device, contiguous, `floats` floats into a larger buffer"""
    buf = torch.zeros(t.numel() + floats + 3, device=device)
    view = buf[floats:floats + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _plane(shape):
    """(B, C, H, W, ky) as the C entries take a shape"""
    return (shape[0], shape[1], 1, shape[2], 1) if len(shape) == 3 else (shape[0], shape[1], shape[2], shape[3], 2)


def _abi_bwd(act, g_act, g_pool):
    """rpde_unet_tanh_pool_bwd on device tensors as they lie; gy starts as NaN: an element nobody writes shows"""
    from rpde import _lib
    gy = torch.full(act.shape, float("nan"), device=act.device)
    _lib.check(_lib.load().rpde_unet_tanh_pool_bwd(_lib.ptr(act), _lib.ptr(g_act), _lib.ptr(g_pool), _lib.ptr(gy),
                                                   *_plane(act.shape), _lib.stream_ptr()), "unet_tanh_pool_bwd")
    return gy


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("shape", MISALIGNED)
def test_misaligned_pointers_take_the_4_byte_kernel(gpu_device, shape, affine):
    """W % 4 == 0 but z (then g_act alone) sits one float off a 16-byte boundary: the same bits as the aligned run"""
    from rpde import ops
    dev, seed = gpu_device, 710
    z = synth.rand_tensor(shape, seed, "z")
    coeff = [(1.0 + 0.3 * synth.rand_tensor((shape[1],), seed, "scale")).to(dev),
             (0.2 * synth.rand_tensor((shape[1],), seed, "shift")).to(dev)] if affine else [None, None]
    g_act, g_pool = synth.rand_tensor(shape, seed, "g_act"), synth.rand_tensor(R.pool_shape(shape), seed, "g_pool").to(dev)
    aligned, off = z.to(dev), _at_offset(z, dev)
    assert aligned.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4 and off.is_contiguous() and torch.equal(aligned, off)
    act, pooled = ops.tanh_pool(aligned, *coeff, pool=True)
    act_off, pooled_off = ops.tanh_pool(off, *coeff, pool=True)
    assert torch.equal(act, act_off) and torch.equal(pooled, pooled_off)
    assert R.rel_l2(act, R.tanh_pool(z.double(), *[_opt(c, lambda t: t.double().cpu()) for c in coeff])[0]) <= FWD
    assert torch.equal(ops.tanh_pool(off, *coeff), act)
    ga, ga_off = g_act.to(dev), _at_offset(g_act, dev)
    assert ga.data_ptr() % 16 == 0 and ga_off.data_ptr() % 16 == 4
    for gp in (g_pool, None):
        gy = _abi_bwd(act, ga, gp)
        assert torch.equal(_abi_bwd(act, ga_off, gp), gy)
        assert R.rel_l2(gy, R.tanh_pool_bwd(act.cpu(), g_act, _opt(gp, torch.Tensor.cpu))) <= GRAD


@pytest.mark.parametrize("shape", ONE_ROW)
def test_one_row_passes_without_pooling(gpu_device, shape):
    from rpde import ops
    z, g = synth.rand_tensor(shape, 720, "z"), synth.rand_tensor(shape, 720, "g_act")
    z64 = z.double().requires_grad_(True)
    act64 = torch.tanh(z64)
    (act64 * g.double()).sum().backward()
    zg = z.to(gpu_device).requires_grad_(True)
    act = ops.tanh_pool(zg)
    (act * g.to(gpu_device)).sum().backward()
    errs = dict(act=R.rel_l2(act, act64), gy=R.rel_l2(zg.grad, z64.grad))
    print(f"tanh_pool {shape} without pool: {errs}")
    _note(errs, "one row", shape)
    assert tuple(act.shape) == shape and errs["act"] <= FWD and errs["gy"] <= GRAD
    with pytest.raises(ValueError, match="nothing left to pool"):
        ops.tanh_pool(z.to(gpu_device), pool=True)


# ---- 2. the backward's argmax, exactly --------------------------------------------------------------------------------
@pytest.mark.parametrize("use", ["pool", "act", "both"])
@pytest.mark.parametrize("shape", ARGMAX_SHAPES)
def test_backward_argmax_is_torchs_bit_for_bit(gpu_device, shape, use):
    """act a multiple of 1/4 and integer gradients: 1 - act^2 and the product are exact in fp32, so every element of gy
    equals the float64 formula (torch's CPU max_pool backward on act, times the chain factor) -- which a first-maximum
    rule other than torch's breaks wherever the maximum is not a window's first element"""
    act, g_act, g_pool = R.argmax_operands(shape, 730)
    g_act, g_pool = (g_act if use != "pool" else None), (g_pool if use != "act" else None)
    want = R.tanh_pool_bwd(act, g_act, g_pool)
    gy = _abi_bwd(act.to(gpu_device), _opt(g_act, lambda t: t.to(gpu_device)), _opt(g_pool, lambda t: t.to(gpu_device)))
    wrong = int((gy.cpu().double() != want).sum())
    print(f"tanh_pool_bwd argmax {shape} use={use}: {wrong} of {want.numel()} elements differ, windows {R.window_patterns(act)}")
    assert torch.equal(gy.cpu().double(), want)


def _guarded(t: torch.Tensor, guard: int, device, fill: float):
    """(view, buffer): t's values between two zones of `guard` floats holding `fill`; the view stays 16-byte aligned"""
    guard = (guard + 3) // 4 * 4
    buf = torch.full((t.numel() + 2 * guard,), fill, device=device)
    view = buf[guard:guard + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def _guards_intact(buf: torch.Tensor, view: torch.Tensor, fill: float) -> bool:
    guard = (buf.numel() - view.numel()) // 2
    return bool((buf[:guard] == fill).all()) and bool((buf[guard + view.numel():] == fill).all())


@pytest.mark.parametrize("shape", [(3, 5, 67), (2, 7, 100), (2, 3, 11, 19), (3, 3, 11, 24)])
def test_tanh_pool_writes_nothing_outside_its_tensors(gpu_device, shape):
    """the C entries on act, pooled and gy inside guard zones wide enough for every thread of the ragged last workgroup
    (the patches 256 further items would address): the threads past the last item must leave them alone"""
    from rpde import _lib
    lib, dev, FILL = _lib.load(), gpu_device, 7.0
    B, C, H, W, ky = _plane(shape)
    items, _ = R.tp_items(shape)
    per_plane = items // (B * C)
    assert items % 256, "the last workgroup has idle threads"
    guard = (256 // per_plane + 2) * H * W + 2 * W + 4
    z, zbuf = _guarded(synth.rand_tensor(shape, 740, "z"), guard, dev, FILL)
    ga, _ = _guarded(synth.rand_tensor(shape, 740, "g_act"), guard, dev, FILL)
    gp, _ = _guarded(synth.rand_tensor(R.pool_shape(shape), 740, "g_pool"), guard, dev, FILL)
    act, act_buf = _guarded(torch.zeros(shape), guard, dev, FILL)
    pooled, pooled_buf = _guarded(torch.zeros(R.pool_shape(shape)), guard, dev, FILL)
    gy, gy_buf = _guarded(torch.zeros(shape), guard, dev, FILL)
    _lib.check(lib.rpde_unet_tanh_pool_fwd(_lib.ptr(z), None, None, _lib.ptr(act), _lib.ptr(pooled), B, C, H, W, ky,
                                           _lib.stream_ptr()), "unet_tanh_pool_fwd")
    _lib.check(lib.rpde_unet_tanh_pool_bwd(_lib.ptr(act), _lib.ptr(ga), _lib.ptr(gp), _lib.ptr(gy), B, C, H, W, ky,
                                           _lib.stream_ptr()), "unet_tanh_pool_bwd")
    assert _guards_intact(act_buf, act, FILL) and _guards_intact(pooled_buf, pooled, FILL) and _guards_intact(gy_buf, gy, FILL)
    act64, pool64 = R.tanh_pool(z.double().cpu())
    assert R.rel_l2(act, act64) <= FWD and R.rel_l2(pooled, pool64) <= FWD
    assert R.rel_l2(gy, R.tanh_pool_bwd(act.cpu(), ga.cpu(), gp.cpu())) <= GRAD


# ---- 3. the fused norms across workgroups -----------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape", BN_SHAPES)
def test_norm_tanh_batchnorm_across_workgroups(gpu_device, shape, training):
    L.test_norm_tanh_batchnorm(gpu_device, shape, training)


@pytest.mark.parametrize("shape,groups", GN_CASES)
def test_groupnorm_tanh_across_workgroups(gpu_device, shape, groups):
    """GroupNorm folds the batch into the channel index: the per-(sample, channel) coefficient lookup past one workgroup"""
    L.test_groupnorm_tanh(gpu_device, shape, groups)


# ---- 4. / 5. upconv over several slices and at the shipped channel counts ---------------------------------------------
def _up_shapes(case):
    rank, B, Cin, Cout, H, W = case
    sizes = (W,) if rank == 1 else (H, W)
    return (B, Cin, *sizes), (Cin, Cout) + (2,) * rank, (B, Cout, *[2 * s for s in sizes])


def upconv_int_operands(case, with_bias, seed=750):
    """x, w, b, upstream as integers in [-3, 3]: every product and sum is an integer far below 2^24, exact in fp32"""
    xs, ws, ys = _up_shapes(case)
    b = R.int_tensor((ws[1],), seed, "b") if with_bias else None
    return R.int_tensor(xs, seed, "x"), R.int_tensor(ws, seed, "w"), b, R.int_tensor(ys, seed, "upstream")


def _upconv_ref(x, w, b, up):
    leaves = [t.double().requires_grad_(True) for t in (x, w) + (() if b is None else (b,))]
    y = R.upconv(*leaves)
    (y * up.double()).sum().backward()
    return [y.detach()] + [t.grad for t in leaves]


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("case", list(UP_SLICED) + UP_WIDE)
def test_upconv_integer_operands_are_exact(gpu_device, case, with_bias):
    from rpde import ops
    op = ops.upconv1d if case[0] == 1 else ops.upconv2d
    x, w, b, up = upconv_int_operands(case, with_bias)
    want = _upconv_ref(x, w, b, up)
    leaves = [t.to(gpu_device).requires_grad_(True) for t in (x, w) + (() if b is None else (b,))]
    y = op(*leaves)
    (y * up.to(gpu_device)).sum().backward()
    got = [y.detach()] + [t.grad for t in leaves]
    names = ["y", "dx", "dw"] + (["db"] if with_bias else [])
    wrong = {n: int((g.cpu().double() != r).sum()) for n, g, r in zip(names, got, want)}
    print(f"upconv integers {case} bias={with_bias}: elements that differ {wrong}, largest |value| "
          f"{max(float(r.abs().max()) for r in want):.0f}")
    assert all(torch.equal(g.cpu().double(), r) for g, r in zip(got, want)), wrong


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("case", list(UP_SLICED) + UP_WIDE)
def test_upconv_random_operands(gpu_device, case, with_bias):
    """the layer file's test (its draws, its budgets, a second run bit for bit) at these cases"""
    rank, B, Cin, Cout, H, W = case
    L.test_upconv(gpu_device, (Cin, Cout, W, B) if rank == 1 else (Cin, Cout, H, W, B), with_bias)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("case", [c for c, (s, per) in UP_SLICED.items() if s * per > c[1] * c[4] * c[5]])
def test_upconv_weight_gradient_reads_no_point_past_the_last(gpu_device, case, with_bias):
    """slices x points-per-slice exceeds the points: the last slice is shorter.  Through the C ABI with integer operands
    and guard words of 3 behind x and g, where a point loop that ran to the slice's nominal end would read: dw and db
    stay bit-equal to float64"""
    from rpde import _lib
    lib, dev = _lib.load(), gpu_device
    rank, B, Cin, Cout, H, W = case
    slices, per = UP_SLICED[case]
    assert lib.rpde_unet_upconv_bwd_weight_slices(B, Cin, Cout, H, W) == slices
    x, w, b, up = upconv_int_operands(case, with_bias)
    want = _upconv_ref(x, w, b, up)
    samples_past = (slices * per - 1) // (H * W) + 1 - B                  # whole samples the nominal end reaches into
    assert samples_past >= 1
    xg, _ = _guarded(x, samples_past * Cin * H * W, dev, 3.0)
    gg, _ = _guarded(up, samples_past * Cout * 2 * rank * H * W, dev, 3.0)
    gw, gw_buf = _guarded(torch.zeros_like(w), 64, dev, 7.0)
    gb, gb_buf = _guarded(torch.zeros(Cout), 64, dev, 7.0) if with_bias else (None, None)
    part, part_buf = _guarded(torch.zeros(slices, w.numel() + Cout), 64, dev, 7.0)
    _lib.check(lib.rpde_unet_upconv_bwd_weight(_lib.ptr(xg), _lib.ptr(gg), _lib.ptr(gw), _lib.ptr(gb), B, Cin, Cout, H, W, rank,
                                               _lib.ptr(part), slices, _lib.stream_ptr()), "unet_upconv_bwd_weight")
    assert torch.equal(gw.cpu().double(), want[2])
    assert _guards_intact(gw_buf, gw, 7.0) and _guards_intact(part_buf, part, 7.0)
    if with_bias:
        assert torch.equal(gb.cpu().double(), want[3]) and _guards_intact(gb_buf, gb, 7.0)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("case", list(CONV_SLICED))
def test_conv_weight_gradient_reads_no_row_past_the_last(gpu_device, case, with_bias):
    """slices x rows-per-slice exceeds the image rows B H: the last slice is short (7 x 15 = 105 > 99) or starts past the
    last row (slice 5 of 6 x 2 starts at row 10 > 9) and must leave zeros in its partial sums, which start as 5.  Through
    the C ABI with integer operands (no sum above 1980 x 3 x 3 < 2^24) and guard words of 3 behind x and g, where a point
    loop that ran to the slice's nominal end would read: dw and db stay bit-equal to float64"""
    from rpde import _lib
    lib, dev = _lib.load(), gpu_device
    B, Cin, Cout, H, W = case
    slices, rows = CONV_SLICED[case]
    assert lib.rpde_conv_k3_bwd_weight_slices(B, Cin, Cout, H, W, 3) == slices and slices * rows > B * H
    x, w, b, up = conv_operands(case, True)
    ref = _conv_run(lambda *a: F.conv2d(*a, padding=1), *[t.double() for t in (x, w, b, up)])
    samples_past = (slices * rows - 1) // H + 1 - B                      # whole samples the nominal end reaches into
    assert samples_past >= 1
    xg, _ = _guarded(x, samples_past * Cin * H * W, dev, 3.0)
    gg, _ = _guarded(up, samples_past * Cout * H * W, dev, 3.0)
    gw, gw_buf = _guarded(torch.full_like(w, 5.0), 64, dev, 7.0)
    gb, gb_buf = _guarded(torch.full((Cout,), 5.0), 64, dev, 7.0) if with_bias else (None, None)
    part, part_buf = _guarded(torch.full((slices, w.numel() + Cout), 5.0), 64, dev, 7.0)
    _lib.check(lib.rpde_conv_k3_bwd_weight(_lib.ptr(xg), _lib.ptr(gg), _lib.ptr(gw), _lib.ptr(gb), B, Cin, Cout, H, W, 3,
                                           _lib.ptr(part), slices, _lib.stream_ptr()), "conv_k3_bwd_weight")
    assert torch.equal(gw.cpu().double(), ref["dw"])
    assert _guards_intact(gw_buf, gw, 7.0) and _guards_intact(part_buf, part, 7.0)
    if with_bias:
        assert torch.equal(gb.cpu().double(), ref["db"]) and _guards_intact(gb_buf, gb, 7.0)


# ---- 5. Conv(k = 3): the point loop over several trips, the shipped channel counts ------------------------------------
def conv_operands(case, integers: bool, seed=760):
    B, Cin, Cout, *sizes = case
    shapes = dict(x=(B, Cin, *sizes), w=(Cout, Cin) + (3,) * len(sizes), b=(Cout,), upstream=(B, Cout, *sizes))
    if integers:
        return [R.int_tensor(s, seed, n) for n, s in shapes.items()]
    x, w, b, up = [synth.rand_tensor(s, seed, n) for n, s in shapes.items()]
    return x, w / (3 ** len(sizes) * Cin) ** 0.5, b, up


def _conv_run(conv, x, w, b, up):
    leaves = [t.requires_grad_(True) for t in (x, w, b)]
    y = conv(*leaves)
    y.backward(up)
    return dict(y=y.detach(), dx=leaves[0].grad, dw=leaves[1].grad, db=leaves[2].grad)


@pytest.mark.parametrize("case", CONV_1D + CONV_2D)
def test_conv_k3_trips_and_shipped_widths(gpu_device, case):
    from rpde import ops
    one_d = len(case) == 4
    op, stock = (ops.conv1d_k3, F.conv1d) if one_d else (ops.conv2d_k3, F.conv2d)
    for integers in (False, True):
        operands = conv_operands(case, integers)
        ref = _conv_run(lambda x, w, b: stock(x, w, b, padding=1), *[t.double() for t in operands])
        got = _conv_run(op, *[t.to(gpu_device) for t in operands])
        errs = {k: R.rel_l2(got[k], ref[k]) for k in ref}
        print(f"conv{1 if one_d else 2}d_k3 {case} integers={integers}: {errs}")
        _note(errs, "conv_k3", case)
        assert errs["y"] <= FWD and max(errs["dx"], errs["dw"], errs["db"]) <= GRAD
        if integers:                       # the weight gradient is an fmaf chain with fixed-order sums: exact on integers
            assert torch.equal(got["dw"].cpu().double(), ref["dw"]) and torch.equal(got["db"].cpu().double(), ref["db"])


# ---- 6. whole models at mid widths ------------------------------------------------------------------------------------
def model_key(kind, ctor, x_shape, seed):
    return kind, tuple(sorted(ctor.items())), tuple(x_shape), seed


@pytest.mark.parametrize("kind,ctor,x_shape,seed", MODELS)
def test_model_step_against_float64_stock_layers(gpu_device, kind, ctor, x_shape, seed):
    module, x, g, ref, floors = R.model_reference(*model_key(kind, ctor, x_shape, seed))
    ours = copy.deepcopy(module).to(gpu_device)
    got = R.model_step(lambda m, t: m(t), ours, x.to(gpu_device), g.to(gpu_device))
    errs = R.model_errors(got, ref)
    worst = max(errs, key=lambda k: errs[k] / max(FWD, 3.0 * floors[k]))
    print(f"{kind} {ctor} on {x_shape}: {len(errs)} tensors, worst {errs[worst]:.3e} ({worst}, floor {floors[worst]:.2e}), "
          f"y {errs['y']:.2e}, worst floor {max(floors.values()):.2e}")
    _note({"worst tensor": max(errs.values()), "y": errs["y"]}, f"{kind} gn={bool(ctor.get('use_groupnorm'))}", x_shape)
    assert any(k.startswith("buf/") and k.endswith("running_var") for k in errs) == (not ctor.get("use_groupnorm"))
    for k, e in errs.items():
        budget = FWD if k == "y" or k.startswith("buf/") else GRAD
        assert floors[k] <= 1e-5, (k, floors[k])
        assert e <= max(budget, 3.0 * floors[k]), f"{k}: rel-L2 {e:.3e}, floor {floors[k]:.2e}"
