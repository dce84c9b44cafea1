"""The float64 reference of the resize tests, checked against itself on the CPU: oracle.reference_path.resize_1d /
resize_2d (torch.fft, what tests/test_gpu_resize.py compares the kernels with) equals the truncated-DFT matrix statement
of tests/resize_ref.py on every shape of the tables, and both give the two closed forms."""
import pytest
import torch

from oracle import reference_path as R
from tests import resize_ref as RR

TOL = 1e-12


@pytest.mark.parametrize("shape", RR.SHAPES_1D, ids=RR.shape_id)
def test_oracle_resize_1d_equals_the_matrix_statement(shape):
    n_in, n_out = shape
    for kind in ("randn", "scaled"):
        x = RR.make_input((3, 7, n_in), kind, 1).double()
        ref = R.resize_1d(x, n_out)
        mat = RR.matrix_resize_1d(x, n_out)
        assert ref.dtype == torch.float64 and tuple(ref.shape) == (3, 7, n_out) == tuple(mat.shape)
        assert RR.rel(ref, mat) <= TOL and RR.row_rel(ref, mat) <= TOL, (kind, RR.rel(ref, mat), RR.row_rel(ref, mat))


@pytest.mark.parametrize("shape", RR.SHAPES_2D, ids=RR.shape_id)
def test_oracle_resize_2d_equals_the_matrix_statement(shape):
    (M, N), out = shape
    for kind in ("randn", "scaled"):
        x = RR.make_input((2, 3, M, N), kind, 2).double()
        ref = R.resize_2d(x, out)
        mat = RR.matrix_resize_2d(x, out)
        assert ref.dtype == torch.float64 and tuple(ref.shape) == (2, 3) + tuple(out) == tuple(mat.shape)
        assert RR.rel(ref, mat) <= TOL and RR.row_rel(ref, mat, 2) <= TOL, (kind, RR.rel(ref, mat), RR.row_rel(ref, mat, 2))


@pytest.mark.parametrize("form", [RR.closed_form_up, RR.closed_form_down], ids=["up-from-even", "down-onto-even-nyquist"])
def test_closed_forms(form):
    x, want = form()
    n_out = want.shape[0]
    for got in (R.resize_1d(x[None], n_out)[0], RR.matrix_resize_1d(x[None], n_out)[0]):
        assert float((got - want).abs().max()) <= TOL
    # the same along the half-spectrum axis N of the 2-D resizer, M kept at its size (along M the reference moves the
    # source Nyquist row to the negative-frequency slot only, which is another rule)
    x2 = torch.ones(1, 6, 1, dtype=torch.float64) * x[None, None, :]
    for got in (R.resize_2d(x2, (6, n_out)), RR.matrix_resize_2d(x2, (6, n_out))):
        assert float((got - want[None, None, :]).abs().max()) <= TOL


def test_tables_hold_what_they_say():
    """the path labels of the tables, restated from cf_h2_eligible / cf_h2_syn_eligible (csrc/cf_dft.hip)"""
    def ana(n, k):
        R2 = 2 * ((k + 3) // 4 * 4)
        return n % 128 == 0 and R2 <= 32 and (n // 32) * ((R2 + 15) // 16) * 2048 <= 65536

    def syn(n, k):
        return ana(n, k) and (n // 16) * 2048 <= 65536

    def paths(n_in, n_out):
        k = min(n_in // 2 + 1, n_out // 2 + 1)
        return ana(n_in, k), syn(n_out, k)

    for s in RR.H2_ANALYSIS_1D:
        assert paths(*s) == (True, False), s
    for s in RR.H2_SYNTHESIS_1D:
        assert paths(*s) == (False, True), s
    for s in RR.OUTSIDE_1D + RR.GENERIC_1D:
        assert paths(*s) == (False, False), s
    for (M, N), (Mo, No) in RR.H2_ANALYSIS_2D:
        assert paths(N, No) == (True, False)
    for (M, N), (Mo, No) in RR.H2_SYNTHESIS_2D:
        assert paths(N, No) == (False, True)
    for (M, N), (Mo, No) in RR.GENERIC_2D:
        assert paths(N, No) == (False, False)
    assert len(set(RR.SHAPES_1D)) == len(RR.SHAPES_1D) == 29 and len(set(RR.SHAPES_2D)) == len(RR.SHAPES_2D) == 17
