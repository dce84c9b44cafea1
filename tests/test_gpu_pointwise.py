"""The small kernels at the model boundary, each against a plain host statement of the same operation.

GELU / ReLU (csrc/rpde_internal.h act_f / dact_f, probed directly through ops.activation: rpde_act_fwd / rpde_act_bwd
evaluate exactly these): the 14-instruction Abramowitz-Stegun GELU on 4e6 evenly spaced fp32 points of [-14, 14] plus
+-0, +-1e-30, +-1e-38, +-65504, +-3e38 and +-inf, against torch.nn.functional.gelu and its autograd in float64.
On |x| <= 9 the bound is absolute (outputs and derivatives are O(1)): 1.5 x the header's own figures, 4.2e-7 for gelu
and 3.1e-7 for gelu' (a CPU emulation of the formula with correctly rounded rcp and exp2 reaches 4.20e-7 at x = 3.07 and
3.08e-7 at x = 0.074; v_rcp_f32 / v_exp_f32 are 1-ulp approximations, hence the factor).  Beyond 9 the function has
saturated: gelu(x) is x or 0, gelu' is 1 or 0, and nothing finite may give a NaN.
The test prints the device maxima and where they sit (pytest -s).  Measured on an MI355X:
    max |gelu error| 4.21e-7 at x = 3.07496,   max |gelu' error| 2.76e-7 at x = 0.25471.

ReLU and its derivative, the channels-first / channels-last transposes and concat_grid produce exactly representable
results: compared bit for bit, on sizes that are not multiples of the 32 x 32 tile or the 256-thread block, with
M != N so that a swapped axis length shows."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GELU_TOL, DGELU_TOL = 1.5 * 4.2e-7, 1.5 * 3.1e-7
SATURATED = 1e-12
GRID_POINTS = 4_000_000
SMALL = [0.0, -0.0, 1e-30, -1e-30, 1e-38, -1e-38]
LARGE = [65504.0, -65504.0, 3e38, -3e38]
INF = [float("inf"), -float("inf")]


def _points():
    """fp32 [4e6 + 12]: the grid, then SMALL, LARGE, INF"""
    grid = torch.linspace(-14.0, 14.0, GRID_POINTS, dtype=torch.float64).float()
    return torch.cat([grid, torch.tensor(SMALL + LARGE + INF, dtype=torch.float32)])


@pytest.fixture(scope="module")
def gelu_reference():
    """(x fp32, gelu float64, gelu' float64) on the CPU, computed once"""
    x = _points()
    xd = x.double().requires_grad_(True)
    y = F.gelu(xd)
    finite = torch.isfinite(xd.detach())
    d, = torch.autograd.grad(y[finite].sum(), xd)
    return x, y.detach(), d


def _act(x, act):
    """-> (act(x), act'(x)) from the device kernels; the derivative is the backward of an all-ones gradient"""
    from rpde import ops
    xs = x.detach().clone().requires_grad_(True)
    out = ops.activation(xs, act)
    out.backward(torch.ones_like(out))
    return out.detach(), xs.grad


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_gelu_and_its_derivative_on_the_full_grid(gpu_device, gelu_reference):
    x, y_ref, d_ref = gelu_reference
    half = x.numel() // 2                                     # two launches of 2e6 + 6 points: not a multiple of 256
    assert half % 256 != 0 and (x.numel() - half) % 256 != 0
    parts = [_act(x[a:b].to(gpu_device), "gelu") for a, b in ((0, half), (half, x.numel()))]
    y = torch.cat([p[0] for p in parts]).cpu()
    d = torch.cat([p[1] for p in parts]).cpu()
    finite = torch.isfinite(x)
    assert not bool(torch.isnan(y[finite]).any()) and not bool(torch.isnan(d[finite]).any())
    assert bool(torch.isfinite(y[finite]).all()) and bool(torch.isfinite(d[finite]).all())
    assert float(y[x == float("inf")][0]) == float("inf")

    core = x.abs() <= 9.0
    ey, ed = (y.double() - y_ref).abs()[core], (d.double() - d_ref).abs()[core]
    xc = x[core]
    iy, idd = int(ey.argmax()), int(ed.argmax())
    print(f"\n[gelu] |x| <= 9: max |gelu error| {float(ey[iy]):.3e} at x = {float(xc[iy]):.5f} (bound {GELU_TOL:.2e}); "
          f"max |gelu' error| {float(ed[idd]):.3e} at x = {float(xc[idd]):.5f} (bound {DGELU_TOL:.2e})")
    assert float(ey[iy]) <= GELU_TOL, (float(ey[iy]), float(xc[iy]))
    assert float(ed[idd]) <= DGELU_TOL, (float(ed[idd]), float(xc[idd]))

    tail = finite & ~core
    assert int(tail.sum()) > 1_000_000 and int((tail & (x.abs() > 14.5)).sum()) == len(LARGE)
    pos, neg = tail & (x > 0), tail & (x < 0)
    assert torch.equal(_bits(y[pos]), _bits(x[pos]))          # gelu(x) == x
    assert float(y[neg].abs().max()) <= SATURATED
    assert float((d[pos].double() - 1.0).abs().max()) <= SATURATED
    assert float(d[neg].abs().max()) <= SATURATED


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_gelu_small_sizes(gpu_device, gelu_reference, n):
    """one element, one block minus one, exactly one block, one block plus one: the tail guard of k_act_fwd / k_act_bwd"""
    x, y_ref, d_ref = gelu_reference
    idx = torch.nonzero(x.abs() <= 9.0).flatten()
    idx = idx[torch.linspace(idx.numel() // 3, idx.numel() - 1, n).long()]
    y, d = _act(x[idx].to(gpu_device), "gelu")
    assert tuple(y.shape) == (n,) and tuple(d.shape) == (n,)
    assert float((y.double().cpu() - y_ref[idx]).abs().max()) <= GELU_TOL
    assert float((d.double().cpu() - d_ref[idx]).abs().max()) <= DGELU_TOL


@pytest.mark.parametrize("n", [1, 255, 256, 257, None])
def test_relu_and_its_derivative_are_bit_exact(gpu_device, n):
    """x > 0 ? x : +0 and x > 0 ? 1 : 0, as rpde_internal.h states them (relu(-0.0) is +0.0; torch's own CPU relu keeps
    the sign of a zero, so against torch.relu the comparison is by value)"""
    x = _points()
    if n is None:
        x = x[GRID_POINTS // 2:]                              # 2e6 + 12 points (not a multiple of 256), every special
        assert x.numel() % 256 != 0
    else:
        first = torch.tensor([-0.0, 0.0, float("inf"), -float("inf"), 1e-38, -1e-38])
        x = torch.cat([first, x[torch.linspace(0, GRID_POINTS - 1, 260).long()]])[:n]
        assert x.numel() == n
    y, d = _act(x.to(gpu_device), "relu")
    want = torch.where(x > 0, x, torch.zeros_like(x))
    assert torch.equal(_bits(y.cpu()), _bits(want))
    assert torch.equal(y.cpu(), torch.relu(x))
    assert torch.equal(_bits(d.cpu()), _bits((x > 0).float()))


# ---- layout ----------------------------------------------------------------------------------------------------------
LAYOUT_SHAPES = [(1, (1,), 2), (2, (33,), 31), (3, (32,), 32), (2, (1000,), 3), (1, (65,), 64), (2, (7, 9), 5),
                 (2, (5,), 1)]                                # the last one: C == 1 is the reshape shortcut


@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=lambda s: f"B{s[0]}-" + "x".join(map(str, s[1])) + f"-C{s[2]}")
def test_channels_first_and_last_transposes_are_exact(gpu_device, shape):
    from rpde import ops
    B, sp, Cc = shape
    nd = len(sp)
    g = torch.Generator().manual_seed(B + Cc + sum(sp))
    to_first, to_last = (0, nd + 1, *range(1, nd + 1)), (0, *range(2, nd + 2), 1)
    xl = torch.randn(B, *sp, Cc, generator=g).to(gpu_device)                 # channels-last
    xf = torch.randn(B, Cc, *sp, generator=g).to(gpu_device)                 # channels-first
    yf, yl = ops.to_channels_first(xl), ops.to_channels_last(xf)
    assert yf.is_contiguous() and yl.is_contiguous()
    assert torch.equal(yf, xl.permute(*to_first).contiguous())
    assert torch.equal(yl, xf.permute(*to_last).contiguous())
    assert torch.equal(ops.to_channels_last(yf), xl) and torch.equal(ops.to_channels_first(yl), xf)
    # autograd of one direction is the other
    gf, gl = torch.randn(B, Cc, *sp, generator=g).to(gpu_device), torch.randn(B, *sp, Cc, generator=g).to(gpu_device)
    a = xl.clone().requires_grad_(True)
    ops.to_channels_first(a).backward(gf)
    assert torch.equal(a.grad, gf.permute(*to_last).contiguous())
    b = xf.clone().requires_grad_(True)
    ops.to_channels_last(b).backward(gl)
    assert torch.equal(b.grad, gl.permute(*to_first).contiguous())


GRIDS = [(1,), (2,), (40,), (1023,), (5, 9), (64, 48), (1, 7), (9, 1)]


@pytest.mark.parametrize("user_grid", [False, True], ids=["generated", "user-grid"])
@pytest.mark.parametrize("lohi", [(0.0, 1.0), (-1.0, 2.5)], ids=["0-1", "m1-2.5"])
@pytest.mark.parametrize("channels_last", [True, False], ids=["last", "first"])
@pytest.mark.parametrize("cin", [1, 3])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda s: "x".join(map(str, s)))
def test_concat_grid_is_exact(gpu_device, grid, cin, channels_last, lohi, user_grid):
    """cat(x, coordinates) with the coordinates numpy.linspace(lo, hi, len) cast to fp32 (or the caller's tables), built
    on the host; the backward hands back exactly the first Cin channels"""
    from rpde import ops
    nd, B = len(grid), 2
    lo, hi = lohi
    g = torch.Generator().manual_seed(sum(grid) + cin)
    x = torch.randn(B, cin, *grid, generator=g)
    if user_grid:
        rs = np.random.RandomState(sum(grid))
        axes = [np.sort(rs.uniform(lo, hi, n)).astype(np.float32) for n in grid]
    else:
        axes = [np.linspace(lo, hi, n).astype(np.float32) for n in grid]
    coords = []
    for ax, tab in enumerate(axes):
        view = [1, 1] + [1] * nd
        view[2 + ax] = grid[ax]
        coords.append(torch.from_numpy(tab).view(*view).expand(B, 1, *grid))
    want = torch.cat([x] + coords, dim=1)
    if channels_last:
        want = want.permute(0, *range(2, nd + 2), 1)
    want = want.contiguous()

    tabs = [torch.from_numpy(t).to(gpu_device) for t in axes] if user_grid else [None] * nd
    xs = x.to(gpu_device).requires_grad_(True)
    out = ops.concat_grid(xs, nd, lo, hi, channels_last, gridx=tabs[0], gridy=tabs[1] if nd == 2 else None)
    assert tuple(out.shape) == tuple(want.shape)
    assert torch.equal(_bits(out.cpu()), _bits(want))
    gout = torch.randn(*want.shape, generator=g).to(gpu_device)
    out.backward(gout)
    gx = gout[..., :cin].permute(0, nd + 1, *range(1, nd + 1)) if channels_last else gout[:, :cin]
    assert tuple(xs.grad.shape) == tuple(x.shape) and torch.equal(xs.grad, gx.contiguous())
