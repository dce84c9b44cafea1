"""tests/spectral_cf_ref.py checked on the CPU: the float64 oracle against an independent dense-matrix statement (explicit
DFT matrices, no torch.fft), the case tables against the layers' mode limits, and the three statistics against planted
defects -- one wrong line or one wrong mode that the whole-tensor relative L2 cannot see."""
import math

import numpy as np
import pytest
import torch

from tests import spectral_cf_ref as S


# ---- the dense statement ---------------------------------------------------------------------------------------------
def _dft(n, rows, sign):
    """[rows, n] complex128: exp(sign 2 pi i k y / n)"""
    k, y = np.arange(rows)[:, None], np.arange(n)[None, :]
    return torch.from_numpy(np.exp(sign * 2j * math.pi * ((k * y) % n) / n))


def _c2r(z, n):
    """z [..., n//2+1] complex -> [..., n] real: (1/n) sum_k c_k (Re z_k cos - Im z_k sin), c = 1 for DC and Nyquist"""
    kn = n // 2 + 1
    c = np.full(kn, 2.0)
    c[0] = 1.0
    if n % 2 == 0:
        c[n // 2] = 1.0
    ang = 2.0 * math.pi * ((np.arange(kn)[:, None] * np.arange(n)[None, :]) % n) / n
    cos, sin = torch.from_numpy(c[:, None] * np.cos(ang) / n), torch.from_numpy(c[:, None] * np.sin(ang) / n)
    return z.real @ cos - z.imag @ sin


def _pad_modes(w, kn):
    return torch.cat([w, w.new_zeros(*w.shape[:-1], kn - w.shape[-1])], dim=-1)


def _dense_1d(x, w):
    n, kn = x.shape[-1], x.shape[-1] // 2 + 1
    spec = x.to(torch.complex128) @ _dft(n, kn, -1.0).T                              # [B,Ci,kn]
    return _c2r(torch.einsum("bik,iok->bok", spec, _pad_modes(w, kn)), n)


def _dense_2d(x, w1, w2):
    M, N = x.shape[-2], x.shape[-1]
    kn, m1 = N // 2 + 1, w1.shape[2]
    spec = torch.einsum("pm,bimn,kn->bipk", _dft(M, M, -1.0), x.to(torch.complex128), _dft(N, kn, -1.0))
    # row p of the output spectrum: weights2 where p falls in the last m1 rows, else weights1 in the first m1, else nothing
    rows = []
    for p in range(M):
        if p >= M - m1:
            rows.append(_pad_modes(w2[:, :, p - (M - m1)], kn))
        elif p < m1:
            rows.append(_pad_modes(w1[:, :, p], kn))
        else:
            rows.append(w1.new_zeros(w1.shape[0], w1.shape[1], kn))
    o = torch.einsum("bipk,iopk->bopk", spec, torch.stack(rows, dim=2))
    z = torch.einsum("mp,bopk->bomk", _dft(M, M, 1.0), o) / M
    return _c2r(z, N)


def _dense(kind, inp):
    t = S._widen(inp, torch.float64)
    out = _dense_2d(t["x"], t["w1"], t["w2"]) if kind == "2d" else _dense_1d(t["x"], t["w"])
    out.backward(t["g"])
    res = {"out": out.detach(), "dx": t["x"].grad}
    res.update({"dW1": t["w1"].grad, "dW2": t["w2"].grad} if kind == "2d" else {"dW": t["w"].grad})
    # (weights1 does not enter the dense statement of L at all: no gradient is a zero gradient)
    return {k: torch.zeros_like(t["w1"]) if v is None else v for k, v in res.items()}


@pytest.mark.parametrize("kind,name", [("2d", "C"), ("2d", "L"), ("1d", "n16")])
def test_oracle_equals_the_dense_matrix_statement(kind, name):
    """overlap with a Nyquist column and odd M (C), full overlap (L), 1-D with its Nyquist bin kept (n = 16, K = 9)"""
    case = S.by_name(S.CASES_2D if kind == "2d" else S.CASES_1D, name)
    inp = S.inputs_2d(case) if kind == "2d" else S.inputs_1d(case)
    ref, dense = S.run_oracle(kind, inp, "identity"), _dense(kind, inp)
    scale = max(float(S._d(v).norm()) for k, v in ref.items() if k.startswith("dW"))
    for k, r in ref.items():
        d = float((S._d(dense[k]) - S._d(r)).norm())
        # (a gradient that vanishes -- dW1 of L -- is held to the other weight's scale)
        assert d <= 1e-12 * max(float(S._d(r).norm()), scale if k.startswith("dW") else 0.0), (name, k, d)


# ---- the tables --------------------------------------------------------------------------------------------------------
def test_every_case_fits_the_spectrum():
    for c in S.CASES_2D:
        B, Ci, Co, M, N, m1, m2 = c.dims
        assert m2 <= N // 2 + 1 and m1 <= M, c
        assert c.act in S.ACTS and c.cf in ("differ", "same", None) and c.col in ("differ", "same", None)
    for c in S.CASES_1D:
        B, Ci, Co, n, K = c.dims
        assert K <= n // 2 + 1, c
    for table in (S.CASES_2D, S.CASES_1D):
        assert len({c.name for c in table}) == len(table)
    assert [c.name for c in S.BLOCK_CASES] == ["A", "D"]


# ---- planted defects ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case_b():
    case = S.by_name(S.CASES_2D, "B")
    inp = S.inputs_2d(case)
    ref = S.run_oracle("2d", inp, "identity")
    return ref, S.floor("2d", inp, "identity", ref)


def test_the_float32_oracle_meets_the_whole_tensor_bounds(case_b):
    """the yardstick itself is inside the bounds the device is held to, and none of its statistics is degenerate"""
    _, fl = case_b
    assert 0 < fl["out"]["rel"] <= S.FWD_TOL and 0 < fl["out"]["line_rel"] <= S.FWD_TOL
    for k in ("dx", "dW1", "dW2"):
        assert 0 < fl[k]["rel"] <= S.GRAD_TOL, (k, fl[k])
    assert 0 < fl["dx"]["line_rel"] <= S.GRAD_TOL
    assert 0 < fl["dW1"]["mode_rel"] <= S.GRAD_TOL and 0 < fl["dW2"]["mode_rel"] <= S.GRAD_TOL


@pytest.mark.parametrize("which", ["out", "dx"])
def test_one_wrong_line_is_caught_by_line_rel_only(case_b, which):
    """B has 19 * 4 * 16 = 1216 lines.  A line that is off by 1e-3 of its norm stands hundreds of times above the line_rel
    bound but moves rel by only 1e-3 / sqrt(1216) = 2.9e-5, six times its bound; the same defect at 1e-4 (still 25 times the
    line_rel bound) is invisible to rel at 5e-6."""
    ref, fl = case_b
    r = ref[which]
    bound = S.FLOOR_FACTOR * fl[which]["line_rel"]
    assert bound <= 4e-6                                       # FLOOR_FACTOR x a float32 error
    for size, hidden in ((1e-3, False), (1e-4, True)):
        bad = r.clone().reshape(-1, r.shape[-1])
        line = 16 * 37 + 15                                    # the clamped tail line of a 16-line tile
        bad[line] += size * bad[line].norm() * torch.nn.functional.normalize(torch.ones_like(bad[line]), dim=0)
        bad = bad.reshape(r.shape)
        e, el = S.rel(bad, r), S.line_rel(bad, r)
        assert el > 25 * bound, (size, el, bound)
        assert 0.5 * size <= el <= 2 * size                    # all lines have about the RMS norm
        assert (e <= S.GRAD_TOL) == hidden, (size, e)
        assert e <= 2 * size / math.sqrt(1216)                 # rel dilutes the line by the square root of their number


@pytest.mark.parametrize("which", ["dW1", "dW2"])
def test_one_wrong_mode_is_caught_by_mode_rel_only(case_b, which):
    """a weight gradient of B has 8 * 16 = 128 modes: one mode off by 5e-5 of the RMS mode norm leaves rel at 4.4e-6, below
    its bound of 5e-6, and stands ten times above the mode_rel bound; at 1e-3 mode_rel sees it hundreds of times above"""
    ref, fl = case_b
    r = ref[which]
    scale = S.mode_scale(ref["dW1"], ref["dW2"])
    bound = S.FLOOR_FACTOR * fl[which]["mode_rel"]
    assert bound <= 4e-6
    for size, hidden in ((1e-3, False), (5e-5, True)):
        bad = r.clone()
        delta = torch.ones_like(bad[:, :, 5, 9])
        bad[:, :, 5, 9] += size * scale * delta / delta.abs().square().sum().sqrt()
        e = S.rel(bad, r)
        em, zero, stray = S.mode_rel(bad, r, scale)
        assert not zero and stray == 0.0
        assert abs(em - size) <= 1e-9 * size + 1e-15 and em > 10 * bound, (size, em, bound)
        assert (e <= S.GRAD_TOL) == hidden, (size, e)


def test_zero_modes_are_the_overwritten_slots_of_weights1():
    """C: M = 15, m1 = 8 -- row 7 of weights1 is row M - m1 = 7 of the spectrum, which weights2 overwrites.  L: m1 = M,
    every weights1 slot is overwritten.  weights2 never has a zero mode."""
    for name, want in (("C", {(7, ky) for ky in range(13)}), ("L", {(r, ky) for r in range(6) for ky in range(4)})):
        case = S.by_name(S.CASES_2D, name)
        ref = S.run_oracle("2d", S.inputs_2d(case), "identity")
        scale = S.mode_scale(ref["dW1"], ref["dW2"])
        assert scale > 0
        _, z1, _ = S.mode_rel(ref["dW1"], ref["dW1"], scale)
        _, z2, _ = S.mode_rel(ref["dW2"], ref["dW2"], scale)
        assert z1 == want and z2 == set(), (name, sorted(z1), sorted(z2))
    # a value on a zero mode is reported relative to the RMS mode norm
    bad = ref["dW1"].clone()
    bad[0, 0, 2, 1] = 3e-6 * scale
    _, _, stray = S.mode_rel(bad, ref["dW1"], scale)
    assert abs(stray - 3e-6) < 1e-12 and stray > S.VANISH
