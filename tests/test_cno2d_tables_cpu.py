"""CPU: 2-D antialiased bicubic resampling is the tensor product of two of the banded 1-D tables
(rpde.ops.cno_resample_table), against F.interpolate(mode="bicubic", antialias=True) on float64 planes -- what the
reference's 2-D CNO_LReLu calls (models/CNO2d.py:43-45).  Bound: a few ulp of the weights (<= 1e-14 on unit-size data).
And the backward's gather: the transposed bands, composed per axis, are the transposed dense matrices."""
import pytest
import torch
import torch.nn.functional as F

SHAPES = [((8, 8), (16, 16)), ((16, 16), (8, 8)), ((12, 20), (32, 32)), ((32, 32), (12, 9)), ((1, 1), (2, 2)),
          ((2, 2), (1, 1)), ((64, 64), (16, 16))]
_IDS = [f"{a[0]}x{a[1]}to{b[0]}x{b[1]}" for a, b in SHAPES]


def _dense(n_in, n_out):
    from rpde import ops
    return ops.cno_dense(*ops.cno_resample_table(n_in, n_out), n_in)


@pytest.mark.parametrize("src,dst", SHAPES, ids=_IDS)
def test_tensor_product_of_the_bands_is_2d_interpolate(src, dst):
    My, Mx = _dense(src[0], dst[0]), _dense(src[1], dst[1])
    x = torch.randn(2, 3, *src, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    got = torch.einsum("oh,bchw,pw->bcop", My, x, Mx)
    ref = F.interpolate(x, size=dst, mode="bicubic", antialias=True)
    err = float((got - ref).abs().max())
    print(f"{src}->{dst}: max |bands - interpolate| {err:.2e}")
    assert got.shape == ref.shape and err <= 1e-14


@pytest.mark.parametrize("src,dst", SHAPES, ids=_IDS)
def test_composed_transposed_bands_are_the_transposed_matrices(src, dst):
    """the backward gathers  M_y^T g M_x  through cno_transpose_band's tables, one per axis"""
    from rpde import ops
    dense, dense_t = [], []
    for n_in, n_out in zip(src, dst):
        s, c, w = ops.cno_resample_table(n_in, n_out)
        ts, tc, tw = ops.cno_transpose_band(s, c, w, n_in)
        dense.append(ops.cno_dense(s, c, w, n_in))
        T = ops.cno_dense(ts, tc, tw, n_out)                      # [n_in, n_out]: row j lists the outputs that read j
        assert torch.equal(T, dense[-1].t())
        dense_t.append(T)
    g = torch.randn(2, 3, *dst, dtype=torch.float64, generator=torch.Generator().manual_seed(8))
    got = torch.einsum("ho,bcop,wp->bchw", dense_t[0], g, dense_t[1])
    x = torch.randn(2, 3, *src, dtype=torch.float64, generator=torch.Generator().manual_seed(9)).requires_grad_(True)
    (F.interpolate(x, size=dst, mode="bicubic", antialias=True) * g).sum().backward()
    assert float((got - x.grad).abs().max()) <= 1e-14
