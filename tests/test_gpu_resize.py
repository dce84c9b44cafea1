"""The spectral resizers (rpde_resize1d / rpde_resize2d through utils.res_utils) against oracle.reference_path in
float64 on the same fp32 inputs, on every shape of tests/resize_ref.py: the h2 fast path of csrc/cf_dft.hip on either
side (analysis when the source is a multiple of 128 and at most 31 points survive, synthesis -- the only caller with
alpha != 1 -- when the target is), the shapes just outside it, and the generic GEMM path at every parity combination,
identity sizes, mixed up / down and axes of 2 or 3 points.  Inputs: randn, and randn whose rows differ by 2^+-10 inside
one 16-row tile (one shared power-of-two scale per tile in the h2 kernels), the latter also judged row by row.

That a shape really took the fast path is shown by a second leg under RPDE_FUSED_CF=0: both legs meet the bound and
their bits DIFFER; for the shapes just outside, and below 16 rows, the bits are equal.  (A plan built while the switch
is off never gets fast-path tables and stays cached for the process -- core.hip, build_plan -- so every test runs its
default leg first, and no other test builds one of these (n, k) plans with the switch off.)

Bound: rel <= 1e-5, the project's forward budget (torch's own fp32 FFT sits at 1.7e-7 against float64 on these shapes).
Every test prints its worst rel and row_rel, the module the worst of each table (pytest -s).  Measured on an MI355X,
worst over each table, every row count, both inputs and both legs:
    1-D   rel 8.5e-7   row_rel 1.2e-6   (640 -> 16, one row: the generic path; the h2 shapes sit below it)
    2-D   rel 4.8e-7   row_rel 5.0e-7   (256x128 -> 24x20, the GEMM leg)
"""
import os

import pytest
import torch

from oracle import reference_path as R
from tests import resize_ref as RR

pytestmark = pytest.mark.gpu

_WORST = {"1-D": [0.0, 0.0, None], "2-D": [0.0, 0.0, None]}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for table, (e, er, where) in _WORST.items():
        print(f"\n[resize] {table} table: worst rel {e:.3e}, worst row_rel {er:.3e} (at {where})")


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _resize(x, out, dims):
    from utils import res_utils
    return res_utils.resize_1d(x, out) if dims == 1 else res_utils.resize(x, out)


def _oracle(x, out, dims):
    return R.resize_1d(x.double(), out) if dims == 1 else R.resize_2d(x.double(), out)


def _judge(table, tag, got, ref, dims, want_shape, by_row, bad):
    if tuple(got.shape) != want_shape:
        bad.append((tag, "shape", tuple(got.shape)))
        return
    if not bool(torch.isfinite(got).all()):
        bad.append((tag, "not finite"))
        return
    e, er = RR.rel(got, ref), RR.row_rel(got, ref, dims)
    w = _WORST[table]
    if e > w[0] or er > w[1]:
        w[0], w[1], w[2] = max(w[0], e), max(w[1], er), tag
    if e > RR.FWD_TOL:
        bad.append((tag, "rel", e))
    if by_row and er > RR.FWD_TOL:
        bad.append((tag, "row_rel", er))
    return e, er


def _run_shape(dev, table, dims, spatial_in, out_size, rows_table, fast_rows, outside):
    """every row count x both inputs: default leg (twice: determinism) against float64; then, where a second leg is
    asked for, the same under RPDE_FUSED_CF=0.  fast_rows(rows) -> whether the h2 kernel must have run."""
    want_sp = (out_size,) if dims == 1 else tuple(out_size)
    bad, runs, worst = [], [], [0.0, 0.0]
    for rows, lead in rows_table.items():
        for kind in ("randn", "scaled"):
            tag = f"{RR.shape_id((spatial_in, out_size))} rows={rows} {kind}"
            x = RR.make_input(lead + tuple(spatial_in if dims == 2 else (spatial_in,)), kind, dims)
            ref = _oracle(x, out_size, dims)
            xd = x.to(dev)
            got = _resize(xd, out_size, dims)
            again = _resize(xd, out_size, dims)
            if not torch.equal(got, again):
                bad.append((tag, "two identical calls differ"))
            m = _judge(table, tag, got, ref, dims, lead + want_sp, kind == "scaled", bad)
            if m:
                worst = [max(worst[0], m[0]), max(worst[1], m[1])]
            runs.append((tag, rows, kind, xd, ref, got, lead))
    if fast_rows is not None or outside:
        with _env(RPDE_FUSED_CF="0"):
            for tag, rows, kind, xd, ref, got, lead in runs:
                plain = _resize(xd, out_size, dims)
                _judge(table, tag + " RPDE_FUSED_CF=0", plain, ref, dims, lead + want_sp, kind == "scaled", bad)
                same = torch.equal(got, plain)
                if not outside and fast_rows(rows) and same:
                    bad.append((tag, "bit-identical to the GEMM leg: the h2 kernel did not run"))
                if (outside or not fast_rows(rows)) and not same:
                    bad.append((tag, "differs from the GEMM leg: a fast path ran where none is expected"))
    print(f"[resize] {RR.shape_id((spatial_in, out_size))}: worst rel {worst[0]:.3e}, worst row_rel {worst[1]:.3e}")
    assert not bad, bad


@pytest.mark.parametrize("shape", RR.SHAPES_1D, ids=RR.shape_id)
def test_resize_1d_against_float64(gpu_device, shape):
    n_in, n_out = shape
    fast = (lambda rows: rows >= 16) if shape in RR.H2_1D else None
    _run_shape(gpu_device, "1-D", 1, n_in, n_out, RR.ROWS_1D, fast, shape in RR.OUTSIDE_1D)


@pytest.mark.parametrize("shape", RR.SHAPES_2D, ids=RR.shape_id)
def test_resize_2d_against_float64(gpu_device, shape):
    (M, N), out = shape
    # the N-axis transforms see rows * M (analysis) and rows * Mo (synthesis) lines: at least 16 for every h2 shape
    fast = None
    if shape in RR.H2_2D:
        lines = M if shape in RR.H2_ANALYSIS_2D else out[0]
        assert lines >= 16
        fast = lambda rows: True          # noqa: E731
    _run_shape(gpu_device, "2-D", 2, (M, N), out, RR.ROWS_2D, fast, False)


@pytest.mark.parametrize("form", [RR.closed_form_up, RR.closed_form_down], ids=["up-from-even", "down-onto-even-nyquist"])
def test_resize_closed_forms(gpu_device, form):
    """64 -> 96 of cos(pi j) is 2 cos(2 pi 32 t / 96) (the source Nyquist bin becomes an ordinary bin of weight 2);
    96 -> 64 of cos(2 pi 32 j / 96 + 0.7) is 0.5 cos(0.7) cos(pi t) (imaginary part dropped, weight 1)"""
    x, want = form()
    n_in, n_out = x.shape[0], want.shape[0]
    bad = []
    for rows, lead in ((1, (1, 1)), (17, (1, 17))):
        xd = x.float().expand(*lead, n_in).contiguous().to(gpu_device)
        got = _resize(xd, n_out, 1)
        ref = want.expand(*lead, n_out)
        e, er = RR.rel(got, ref), RR.row_rel(got, ref)
        amax = float((got.double().cpu() - ref).abs().max())
        print(f"[resize] closed form {n_in}->{n_out} rows={rows}: rel {e:.3e} row_rel {er:.3e} max abs {amax:.3e}")
        if not (e <= RR.FWD_TOL and er <= RR.FWD_TOL):
            bad.append((rows, e, er))
    # along N of the 2-D resizer, M kept
    x2 = x.float().expand(1, 2, 6, n_in).contiguous().to(gpu_device)
    got = _resize(x2, (6, n_out), 2)
    ref = want.expand(1, 2, 6, n_out)
    e, er = RR.rel(got, ref), RR.row_rel(got, ref, 2)
    print(f"[resize] closed form 6x{n_in}->6x{n_out}: rel {e:.3e} row_rel {er:.3e}")
    if not (tuple(got.shape) == (1, 2, 6, n_out) and e <= RR.FWD_TOL and er <= RR.FWD_TOL):
        bad.append(("2-D", e, er))
    assert not bad, bad
