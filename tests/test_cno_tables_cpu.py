"""CPU: the banded resampling tables of the CNO activation (rpde.ops.cno_resample_table) against
F.interpolate(mode="bicubic", antialias=True) applied to a float64 identity, which is what the reference's CNO_LReLu
calls (models/CNO1d.py:42-44).  The tables are built in float64 by a closed rule; the bound is a few ulp of the
weights (<= 1e-14), far below anything fp32 can see."""
import pytest
import torch

from tests import cno_ref

PAIRS = [(16, 32), (32, 16), (32, 8), (32, 32), (24, 32), (30, 16), (17, 32), (64, 16), (7, 32),
         (1, 2), (2, 1), (2, 4), (4, 1), (48, 64)]


@pytest.mark.parametrize("n_in,n_out", PAIRS, ids=[f"{a}to{b}" for a, b in PAIRS])
def test_table_is_torchs_antialiased_bicubic(n_in, n_out):
    from rpde import ops
    start, count, w = ops.cno_resample_table(n_in, n_out)
    assert start.shape == (n_out,) and count.shape == (n_out,) and w.shape[0] == n_out and w.dtype == torch.float64
    assert int(start.min()) >= 0 and int((start + count).max()) <= n_in and int(count.min()) >= 1
    for i in range(n_out):
        assert torch.all(w[i, int(count[i]):] == 0), "taps past the count are zero padding"
    M = ops.cno_dense(start, count, w, n_in)
    ref = cno_ref.resample_matrix(n_in, n_out)
    err = float((M - ref).abs().max())
    print(f"{n_in}->{n_out}: taps {int(count.max())}, max |table - interpolate| {err:.2e}")
    assert err <= 1e-14
    assert float((M.sum(1) - 1).abs().max()) <= 1e-14                        # rows sum to 1
    ts, tc, tw = ops.cno_transpose_band(start, count, w, n_in)
    assert ts.shape == (n_in,) and int((ts + tc).max()) <= n_out
    assert torch.equal(ops.cno_dense(ts, tc, tw, n_out, transposed=True), M)  # the transposed band is the same matrix


@pytest.mark.parametrize("n", [1, 2, 7, 32])
def test_equal_sizes_are_the_identity_exactly(n):
    from rpde import ops
    start, count, w = ops.cno_resample_table(n, n)
    assert torch.equal(ops.cno_dense(start, count, w, n), torch.eye(n, dtype=torch.float64))


def test_tap_counts():
    from rpde import ops
    assert int(ops.cno_resample_table(16, 32)[1].max()) == 4
    assert int(ops.cno_resample_table(32, 16)[1].max()) == 8
    assert int(ops.cno_resample_table(32, 8)[1].max()) == 16


def test_bad_sizes_are_refused():
    from rpde import ops
    with pytest.raises(ValueError):
        ops.cno_resample_table(0, 4)
