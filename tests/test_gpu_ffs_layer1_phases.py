"""GPU: k_ffs_layer1 (csrc/ff_bwd_split.hip) with a pass's phases overlapping -- the next tile's du2 slices are staged in
front of this tile's consumer, the du2 loads of the tile after it start right behind, x's in front of barrier 2 and
d1's behind the consumer, and two lo fragments of W2^T are read back from LDS -- through rpde_feedforward_bwd at the C
ABI in the guarded, poisoned buffers of tests/ff_abi.py: dim 64, factor 4, three layers, dropout 0.1, LayerNorm on,
weights at the scales of bench.py:time_feedforward, the library's own forward stash.

Shapes, for a grid of G = min(CUs, 256) workgroups (the numbers are those of a 256-CU part):
  64 G          = 16384   two tiles per workgroup: the smallest steady state, tile 2 staged under the consumer of tile 1
  32 G + 167    =  8359   one and two tiles side by side, a partial tile (7 points) at the end
  96 G + 1      = 24577   769 tiles: workgroup 0 runs four, the others three (odd and even trip counts); the last tile
                          holds one point
One point of grad_out is 1e4 times the rest and sits in a tile that is not its workgroup's first; the largest shape has
a second one in the middle round.  The running exponent of a du1 panel then moves, and the accumulators of gW1 are
rescaled, in a pass whose staging has already run.

Per shape: (a) two calls give identical bits in every output, the second with a copy stream hammering HBM beside it
(later arrivals: an LDS race or a load used before it landed shows here); (b) db of the first layer has the bits of
RPDE_FF_BWD_SPLIT=0 in the same run (the chain's order of summation; asserted where the part has at most 256 CUs, as the
slab regions assume); (c) dx and the first layer's dW against float64 from the same stash: relative L2 at most 2 x the
old path's in the same run -- the rule of tests/test_gpu_ff_bwd_split.py, the factor covers another scaling unit of du1
and nothing more; (d) every output finite and every guard zone intact (ff_abi.Buffers.check, in each backward call)."""
import functools

import pytest
import torch

from tests import ff_abi as A
from tests.test_gpu_ff_bwd_split import DIM, HID, OLD, OUTPUTS, _bits_equal, _Call, _reference

pytestmark = pytest.mark.gpu

MIN_P = 8192                                   # below it rpde_feedforward_bwd keeps the chain (wgrad_h2_dgrad_ok)


def _grid(dev):
    return min(torch.cuda.get_device_properties(dev).multi_processor_count, 256)


def _shapes(G):
    """name -> (P, tiles that hold a point of grad_out at 1e4 x the rest); tile t belongs to workgroup t % G"""
    return {"two-tiles": (64 * G, [G + 7]),
            "one-and-two": (32 * G + 5 * 32 + 7, [G + 3]),
            "three-and-four": (96 * G + 1, [2 * G + 200 % G, G + 9])}


@functools.lru_cache(maxsize=1)
def _problem(P, huge_tiles):
    g = torch.Generator(device="cpu").manual_seed(77000 + P)
    mk = lambda *shape, s=1.0: torch.randn(*shape, generator=g) * s          # noqa: E731
    w = [mk(HID, DIM, s=0.12), mk(HID, HID, s=0.06), mk(DIM, HID, s=0.06)]
    b = [mk(HID, s=0.1), mk(HID, s=0.1), mk(DIM, s=0.1)]
    gamma, beta = 1.0 + mk(DIM, s=0.1), mk(DIM, s=0.1)
    x, res, gout = mk(P, DIM), mk(P, DIM), mk(P, DIM)
    for i, t in enumerate(huge_tiles):
        row = 32 * t + 5 + 16 * i                                            # both point blocks of a tile get one
        assert row < P
        gout[row] *= 1e4
    return dict(P=P, p=0.1, layer_norm=True, w=w, b=b, gamma=gamma, beta=beta, x=x, res=res, gout=gout)


class _Hammer:
    """a side stream copying 128 MB back and forth while the kernels run (tests/test_gpu_counted_waits.py)"""

    def __init__(self, dev):
        self.side = torch.cuda.Stream()
        self.junk = torch.empty(32 << 20, device=dev)

    def __call__(self, rounds=20):
        with torch.cuda.stream(self.side):
            for _ in range(rounds):
                self.junk.copy_(self.junk.flip(0))


@pytest.mark.parametrize("shape", ["two-tiles", "one-and-two", "three-and-four"])
def test_layer1_phases(gpu_device, shape):
    G = _grid(gpu_device)
    P, huge = _shapes(G)[shape]
    if P < MIN_P:
        pytest.skip(f"{G} workgroups: P = {P} is below the split path's minimum of {MIN_P} points")
    tiles = (P + 31) // 32
    assert all(G <= t < tiles for t in huge)
    prob = _problem(P, tuple(huge))
    call = _Call(gpu_device, prob)
    ref = _reference(prob, call.stash())
    hammer = _Hammer(gpu_device)
    new = call.backward()                                                    # (d): finite, guards intact, in every call
    hammer()
    again = call.backward()
    torch.cuda.synchronize()
    old = call.backward(env=OLD)
    names = [k for k in OUTPUTS if k in ref]
    assert set(new) == set(again) == set(old) == set(names)
    e_new = {k: A.rel(new[k], ref[k]) for k in names}
    e_old = {k: A.rel(old[k], ref[k]) for k in names}
    print(f"\n[ffs-layer1-phases] {shape}: P={P} tiles={tiles} grid={G} huge tiles={huge}")
    for k in names:
        print(f"[ffs-layer1-phases]   {k:7s} split {e_new[k]:.3e}  old {e_old[k]:.3e}  ratio {e_new[k] / max(e_old[k], 1e-300):.2f}"
              f"  bits as old: {_bits_equal(new[k], old[k])}  repeats: {_bits_equal(new[k], again[k])}")
    assert not (_bits_equal(new["dx"], old["dx"]) and _bits_equal(new["dW0"], old["dW0"])), "RPDE_FF_BWD_SPLIT=0 changed nothing"
    for k in names:                                                          # (a)
        assert _bits_equal(new[k], again[k]), (k, "not reproducible")
    if torch.cuda.get_device_properties(gpu_device).multi_processor_count <= 256:
        assert _bits_equal(new["db0"], old["db0"]), "db of the first layer: not the chain's bits"       # (b)
    for k in ("dx", "dW0"):                                                  # (c)
        assert e_new[k] <= 2.0 * e_old[k], (k, e_new[k], e_old[k])
