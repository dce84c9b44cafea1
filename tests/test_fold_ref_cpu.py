"""What tests/test_gpu_slab_fold.py rests on: the numpy statement of the slab fold's summation order (tests/fold_ref.py).

1. It is a sum: against float64 it stays within S float32 roundoffs of sum |x|, the a-priori bound of any order of S
   terms ((S - 1) u / (1 - (S - 1) u) <= S u for S (S - 1) u <= 1).
2. The order without the 32-deep loop gives the same bits at every slab count of S = 1 .. 299, 511, 512, 513, 1024, 1300:
   that is why the segment fold of the fused FeedForward backward could become jobs of the one kernel without moving a bit.
3. It is not the serial order: somewhere among the slab counts of the GPU test the two differ in bits, so that test can
   tell a serial fold from the kernel's."""
import numpy as np
import pytest

from tests import fold_ref as R

S_LIST = list(range(1, 300)) + [511, 512, 513, 1024, 1300]
N = 96


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("S", R.S_EDGES + [511, 1024, 1300])
def test_fold_is_a_sum(S):
    x = R.slabs(S, N)
    assert not (x == 0).any()
    err = np.abs(R.fold_f32(x).astype(np.float64) - R.fold_f64(x))
    bound = S * R.EPS32 * np.abs(x.astype(np.float64)).sum(axis=0)
    print(f"S={S}: max error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), (S, float((err / bound).max()))


def test_deep_loop_does_not_move_a_bit():
    differ = [S for S in S_LIST if not np.array_equal(_bits(R.fold_f32(R.slabs(S, N))), _bits(R.fold_f32_no32(R.slabs(S, N))))]
    assert not differ, differ


def test_order_differs_from_serial():
    differ = [S for S in R.S_EDGES if not np.array_equal(_bits(R.fold_f32(R.slabs(S, N))), _bits(R.fold_serial(R.slabs(S, N))))]
    print("slab counts at which the kernel's order and a serial sum differ in bits:", differ)
    # from five slabs on two waves hold more than one term each; with 96 outputs per count a rounding differs
    assert set(differ) >= {S for S in R.S_EDGES if S >= 28}, differ
    # up to four slabs every wave holds one term: (x0 + x1) + (x2 + x3) against ((x0 + x1) + x2) + x3, the same for S <= 3
    assert not set(differ) & {1, 2, 3}
