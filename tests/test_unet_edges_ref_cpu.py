"""CPU: the shapes of tests/test_gpu_unet_edges.py land in the regimes its docstring claims -- by the launch arithmetic
of csrc/unet.hip and csrc/cno_layers.hip restated in tests/unet_ref.py and, for the slices, by the library's own query,
which needs no device -- and its exact comparisons are entitled to exactness: the integer operands stay far below 2^24
at every partial sum, the argmax operands are exact in fp32 and hold every kind of window, the whole-model floors stay
at or below 1e-5, and stock_forward is the U-Net the fixtures were written from."""
import pytest
import torch

from tests import test_gpu_unet_edges as E
from tests import test_gpu_unet_layers as L
from tests import unet_ref as R
from tests.golden import synth
from tests.golden.unet_cases import load_case, run_case, state_for


def _workgroups(items):
    return (items + 255) // 256


def test_tanh_pool_shapes_span_workgroups():
    for shape, items in E.TP_EDGE.items():
        got, vec = R.tp_items(shape)
        assert got == items and vec == (shape[-1] % 4 == 0), shape
        assert _workgroups(items) >= 2, shape
    wg = {s: _workgroups(i) for s, i in E.TP_EDGE.items()}
    assert wg[(3, 5, 67)] == 2 and 510 % 256 and 256 % 34                     # ragged, the boundary inside a row of 34 patches
    assert wg[(4, 6, 16, 48)] == 9 and 2304 % 256 == 0                        # an exact multiple: no ragged workgroup
    assert {len(s) for s in E.TP_EDGE} == {3, 4}
    assert {(len(s), R.tp_items(s)[1]) for s in E.TP_EDGE} == {(3, False), (3, True), (4, False), (4, True)}
    # the boundary between the first two workgroups falls inside a plane, not between two
    for shape, items in E.TP_EDGE.items():
        assert 256 % (items // (shape[0] * shape[1])), shape
    # what the layer file reaches, so that the claim stays checked: never a second workgroup
    assert max(R.tp_items(s)[0] for s in L.TP_1D + L.TP_2D + [(2, 3, 64), (2, 3, 31), (2, 2, 16, 32), (1, 2, 9, 14)]) == 256
    for shape in E.TIE_SHAPES + E.ARGMAX_SHAPES:
        assert shape in E.TP_EDGE
    for shape, _ in [(s, None) for s in E.BN_SHAPES] + E.GN_CASES:
        assert _workgroups(R.tp_items(shape)[0]) >= 2, shape
    # misaligned: W % 4 == 0, so only the pointer keeps the 16-byte kernel away; its 4-byte launch has twice the patches
    for shape in E.MISALIGNED:
        assert shape[-1] % 4 == 0 and R.tp_items(shape, vec=False)[0] == 2 * R.tp_items(shape)[0]
    for shape in E.ONE_ROW:
        assert shape[2] == 1 and R.pool_shape(shape)[2] == 0
    assert {s[-1] % 4 == 0 for s in E.ONE_ROW} == {True, False}


def test_upconv_slice_table():
    from rpde import _lib
    query = _lib.load().rpde_unet_upconv_bwd_weight_slices
    for (rank, B, Cin, Cout, H, W), (slices, per) in E.UP_SLICED.items():
        assert (rank == 1) == (H == 1)
        assert query(B, Cin, Cout, H, W) == slices and R.upconv_slices(B, Cin, Cout, H, W) == (slices, per)
        assert slices >= 2 and per > 256                          # a second trip of the thread loop in every slice
    assert E.UP_SLICED[(1, 3, 5, 6, 1, 171)] == (2, 257)          # one point in the second trip
    assert E.UP_SLICED[(1, 2, 4, 4, 1, 300)] == (2, 1 * 300)      # a slice is a sample: the boundary is the batch boundary
    assert 332 % (13 * 17) and 332 % 17                           # mid-plane and mid-row
    assert 1000 - 2 * 334 == 332                                  # the shorter last slice
    shorter = [c for c, (s, per) in E.UP_SLICED.items() if s * per > c[1] * c[4] * c[5]]
    assert len(shorter) == 4 and {c[0] for c in shorter} == {1, 2}
    for rank, B, Cin, Cout, H, W in E.UP_WIDE:
        assert query(B, Cin, Cout, H, W) == 1
    rank, B, Cin, Cout, H, W = E.UP_WIDE[1]
    assert (4 * Cout + 63) // 64 == 32 and Cin // 16 == 64        # k_unet_upconv: row tiles of 64, K steps of 16
    # the layer file's cases all run one slice
    for Cin, Cout, n, B in L.UP_1D:
        assert query(B, Cin, Cout, 1, n) == 1 == R.upconv_slices(B, Cin, Cout, 1, n)[0]
    for Cin, Cout, H, W, B in L.UP_2D:
        assert query(B, Cin, Cout, H, W) == 1 == R.upconv_slices(B, Cin, Cout, H, W)[0]


def test_conv_slice_table():
    from rpde import _lib
    query = _lib.load().rpde_conv_k3_bwd_weight_slices
    for (B, Cin, Cout, H, W), (slices, rows) in E.CONV_SLICED.items():
        assert query(B, Cin, Cout, H, W, 3) == slices and R.conv_slices(B, Cin, Cout, H, W) == (slices, rows)
        assert slices * rows > B * H and rows * W > 256           # past the last row; a second trip of the thread loop
    assert E.CONV_SLICED[(3, 5, 6, 33, 20)] == (7, 15) and 6 * 15 < 99 < 7 * 15        # the last slice is short
    assert E.CONV_SLICED[(3, 5, 6, 3, 180)] == (6, 2) and 5 * 2 > 9                    # the last slice is empty
    # Conv1d keeps its one slice whatever the shape
    for B, Cin, Cout, n in E.CONV_1D:
        assert query(B, Cin, Cout, 1, n, 1) == 1


def test_conv_cases_reach_the_trips_and_the_grid():
    trips = [(B * n + 255) // 256 for B, _, _, n in E.CONV_1D]
    assert trips == [4, 8, 1] and (3 * 300) % 256                 # four trips, the last one ragged; eight whole ones
    B, Cin, Cout, n = E.CONV_1D[2]
    assert ((Cin + 3) // 4, (Cout + 3) // 4) == (256, 128)        # the weight-gradient grid of the decoder's 1024 -> 512
    assert E.CONV_2D == [(2, 512, 256, 2, 2)]


def _abs(ts):
    return [None if t is None else t.abs() for t in ts]


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("case", list(E.UP_SLICED) + E.UP_WIDE)
def test_upconv_integer_operands_stay_exact_in_fp32(case, with_bias):
    """the same products with every operand replaced by its magnitude bound every partial sum, in whatever order"""
    ops = E.upconv_int_operands(case, with_bias)
    assert all(t is None or (torch.equal(t, t.round()) and float(t.abs().max()) <= 3.0) for t in ops)
    assert float(ops[0].abs().max()) == 3.0 and float(ops[1].abs().max()) == 3.0
    bound = max(float(r.abs().max()) for r in E._upconv_ref(*_abs(ops)))
    print(f"upconv integers {case} bias={with_bias}: no partial sum above {bound:.0f}")
    assert bound < 2 ** 24


@pytest.mark.parametrize("case", E.CONV_1D + E.CONV_2D + list(E.CONV_SLICED))
def test_conv_integer_operands_stay_exact_in_fp32(case):
    import torch.nn.functional as F
    x, w, b, up = _abs(E.conv_operands(case, True))
    assert float(max(t.max() for t in (x, w, b, up))) == 3.0
    ref = E._conv_run(lambda *a: (F.conv1d if len(case) == 4 else F.conv2d)(*a, padding=1), x.double(), w.double(), b.double(), up.double())
    assert max(float(ref["dw"].max()), float(ref["db"].max())) < 2 ** 24


@pytest.mark.parametrize("shape", E.ARGMAX_SHAPES)
def test_argmax_operands_are_exact_and_hold_every_kind_of_window(shape):
    act, g_act, g_pool = R.argmax_operands(shape, 730)
    assert set((4.0 * act).unique().tolist()) <= set(range(-3, 4)) and len(act.unique()) == 7
    assert torch.equal(g_act, g_act.round()) and torch.equal(g_pool, g_pool.round()) and float(g_act.abs().max()) == 3.0
    # the fp32 result of the kernel's own operation order equals float64's: nothing is rounded
    a = act.clone().requires_grad_(True)
    (R.max_pool(a) * g_pool).sum().backward()
    g32 = (g_act + a.grad) * torch.addcmul(torch.ones_like(act), -act, act)
    assert g32.dtype == torch.float32 and torch.equal(g32.double(), R.tanh_pool_bwd(act, g_act, g_pool))
    pat = R.window_patterns(act)
    print(f"argmax operands {shape}: {pat} of {R.windows(act).shape[2] * shape[0] * shape[1]} windows")
    assert pat["distinct_late"] >= 20 and pat["full"] >= 20
    if len(shape) == 4:
        assert pat["partial"] >= 20 and pat["partial_late"] >= 10
    # a last-maximum rule would move a gradient in every window with a shared maximum
    w = R.windows(act)
    shared = (w == w.max(-1, keepdim=True).values).sum(-1) > 1
    assert int((shared & (g_pool.reshape(shape[0], shape[1], -1) != 0)).sum()) >= 20


@pytest.mark.parametrize("kind,ctor,x_shape,seed", E.MODELS)
def test_model_floors(kind, ctor, x_shape, seed):
    module, x, g, ref, floors = R.model_reference(*E.model_key(kind, ctor, x_shape, seed))
    worst = max(floors, key=floors.get)
    print(f"{kind} {ctor} on {x_shape}, seed {seed}: forward floor {floors['y']:.2e}, worst floor {floors[worst]:.2e} ({worst})")
    assert max(floors.values()) <= 1e-5
    assert set(ref) == {"y", "dx"} | {"grad/" + n for n, _ in module.named_parameters()} | {"buf/" + n for n, _ in module.named_buffers()}
    assert module.upconv4.in_channels == 16 * ctor["width"] and all(int(b) == 0 for n, b in module.named_buffers() if n.endswith("tracked"))
    assert all(float(r.double().norm()) > 0.0 for r in ref.values())


@pytest.mark.parametrize("name", ["unet2d_rect_train", "unet1d_gn_3ch", "unet1d_small_train"])
def test_stock_forward_is_the_fixtures_unet(name):
    """stock_forward on the project's module tree against the fixtures written from the reference's U-Net (CPU, float32):
    the same torch layers in the same data flow, so far inside the fixtures' budgets"""
    from models import unet
    case, spec, digests = load_case(name)
    module = getattr(unet, case["kind"])(**case["ctor"])
    module.load_state_dict(state_for(spec, case["seed"]), strict=True)
    module.forward = lambda x: R.stock_forward(module, x)
    errs = synth.check_results(run_case(module, case), digests, tol=1e-5, grad_tol=2e-5, label=name)
    assert max(errs.values()) <= 2e-5 and errs["y"] <= 1e-6
