"""The slab fold (csrc/pointwise.hip, k_fold_jobs) alone, bit for bit against its stated order (tests/fold_ref.py).

rpde_conv1x1_bwd with a spatial size of 1, Cin = 1, grad_w = grad_x = NULL and grad_b set is a pure fold: k_rowsum of a
row of one value returns that value exactly (the other 255 lanes add zeros to it; no zero is among the data, so no
signed zero can differ), and grad_b[c] is then the fold of B slabs of Cout values, the rows of grad_out [B, Cout, 1].

Slab counts: the edges of the walker's 32-deep, 8-deep and single loops for each of the four waves; output counts: the
edges of the 64-output workgroup.  Every buffer is guarded and poisoned as in tests/ff_abi.py and the workspace has
exactly the queried size.  Asserted: the bits of the emulation, intact guards, and the same bits from a second call.
A serial fold fails this from four slabs on (tests/test_fold_ref_cpu.py::test_order_differs_from_serial)."""
import numpy as np
import pytest
import torch

from tests import ff_abi as A
from tests import fold_ref as R

pytestmark = pytest.mark.gpu


def _fold_on_device(x: np.ndarray):
    """grad_b of the pure-fold call for the slabs x [B, Cout], twice -> two int32 views of the result"""
    from rpde import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, Cout = x.shape
    bufs = A.Buffers(dev)
    X = bufs.new("x", (B, 1, 1), torch.ones(B, 1, 1))
    W = bufs.new("w", (Cout, 1), torch.ones(Cout, 1))
    G = bufs.new("grad_out", (B, Cout, 1), torch.from_numpy(x))
    gb = bufs.new("grad_b", (Cout,))
    nws = int(lib.rpde_conv1x1_ws_bytes(B, 1, Cout, 1))
    ws = bufs.new_bytes("ws", nws)
    got = []
    for call in range(2):
        gb.poison()
        ws.poison()
        _lib.check(lib.rpde_conv1x1_bwd(X.ptr, W.ptr, G.ptr, None, None, gb.ptr, B, 1, Cout, 1, 0, 0, ws.ptr, nws,
                                        _lib.stream_ptr()), "conv1x1_bwd")
        torch.cuda.synchronize()
        bufs.check(["grad_b"], f"fold B={B} Cout={Cout} call {call}")
        got.append(gb.t.cpu().numpy().view(np.int32).copy())
    return got


@pytest.mark.parametrize("Cout", R.N_EDGES)
@pytest.mark.parametrize("B", R.S_EDGES)
def test_fold_bits(B, Cout):
    x = R.slabs(B, Cout)
    assert not (x == 0).any()
    want = R.fold_f32(x).view(np.int32)
    first, second = _fold_on_device(x)
    bad = np.nonzero(first != want)[0]
    assert bad.size == 0, (f"{bad.size} of {Cout} outputs differ from the stated order, first at {int(bad[0])}: "
                           f"{first[bad[0]]:#x} vs {want[bad[0]]:#x}")
    assert np.array_equal(first, second), "a second call gave other bits"
