"""tests/fspectral_ref.py checked on the CPU: the float64 oracle against an independent dense-matrix statement (explicit DFT
matrices, no torch.fft), the case tables against the dispatch rules they are there for, the float32 floor, and the checker
against planted faults -- a test that cannot tell right from wrong must fail, not pass."""
import math

import numpy as np
import pytest
import torch

from tests import fspectral_ref as S


# ---- the dense statement ---------------------------------------------------------------------------------------------
def _scales(n, norm):
    return {"ortho": (n ** -0.5, n ** -0.5), "forward": (1.0 / n, 1.0), "backward": (1.0, 1.0 / n)}[norm]


def _axis(x, w, n, keff, norm, lowpass):
    """x [..., n, C] float64 (the transformed axis second to last), w [C, C, K, 2] -> the layer along that axis.  The
    synthesis uses Re z cos - Im z sin with weight 1 for DC and Nyquist, 2 otherwise: sin vanishes at DC and Nyquist, so the
    imaginary parts of those two bins of the mixed spectrum cannot have an effect"""
    sf, si = _scales(n, norm)
    k, y = np.arange(keff)[:, None], np.arange(n)[None, :]
    ang = 2.0 * math.pi * ((k * y) % n) / n
    cos, sin = torch.from_numpy(np.cos(ang)), torch.from_numpy(np.sin(ang))
    re, im = sf * torch.einsum("ky,...yc->...kc", cos, x), -sf * torch.einsum("ky,...yc->...kc", sin, x)
    if not lowpass:
        wr, wi = w[:, :, :keff, 0], w[:, :, :keff, 1]
        re, im = (torch.einsum("...ki,iok->...ko", re, wr) - torch.einsum("...ki,iok->...ko", im, wi),
                  torch.einsum("...ki,iok->...ko", re, wi) + torch.einsum("...ki,iok->...ko", im, wr))
    c = np.full(keff, 2.0)
    c[0] = 1.0
    if n % 2 == 0 and keff == n // 2 + 1:
        c[n // 2] = 1.0
    c = torch.from_numpy(c)[:, None]
    return si * (torch.einsum("ky,...kc->...yc", c * cos, re) - torch.einsum("ky,...kc->...yc", c * sin, im))


def _dense(case, t):
    K, lp = case.dims[-1], case.mode == "low-pass"
    if case.kind == "1d":
        n = case.dims[1]
        return _axis(t["x"], t.get("w"), n, min(K, n // 2 + 1), case.norm, lp)
    B, M, N, C, _ = case.dims
    oy = _axis(t["x"], t.get("wy"), N, min(K, N // 2 + 1), "ortho", lp)
    ox = _axis(t["x"].transpose(1, 2), t.get("wx"), M, min(K, M // 2 + 1), "ortho", lp).transpose(1, 2)
    return oy + ox


DENSE = [
    # Nyquist along M (keff_x = 6 = 10/2+1), a clamp along N (odd: keff_y = 4 < K)
    S.Case("dense-2d", "2d", (2, 10, 7, 3, 6)),
    # norm "forward", Nyquist (keff = 7 = 12/2+1), K > keff
    S.Case("dense-1d", "1d", (2, 12, 3, 9), "gauss", "full", True, "forward"),
    # low-pass, Nyquist along N
    S.Case("dense-lowpass", "2d", (2, 8, 6, 3, 4), "gauss", "low-pass", True),
]


@pytest.mark.parametrize("case", DENSE, ids=lambda c: c.name)
def test_oracle_equals_the_dense_matrix_statement(case):
    ref, dense = S.run_oracle(case), S.run_oracle(case, fn=_dense)
    assert set(ref) == set(dense) == {"out", "dx"} | (set(S.keffs(case)) if case.mode == "full" else set())
    wscale = max([float(v.norm()) for k, v in ref.items() if k.startswith("dW")] or [0.0])
    for k, r in ref.items():
        d = float((dense[k] - r).norm())
        assert d <= 1e-12 * (wscale if k.startswith("dW") else float(r.norm())), (case.name, k, d)
    for k, keff in S.keffs(case).items():
        if k in ref:
            assert float(ref[k][:, :, keff:].abs().max() if ref[k].shape[2] > keff else 0.0) == 0.0, k


@pytest.mark.parametrize("case", DENSE[:2], ids=lambda c: c.name)
def test_imaginary_parts_of_dc_and_nyquist_have_no_effect(case):
    """x is real, so its DC and Nyquist bins are real and Im W there moves only the imaginary part of the mixed bin, which
    the real inverse transform ignores: the output does not depend on it and its gradient is zero"""
    inp = dict(S.inputs(case))
    ref = S.run_oracle(case, inp=inp)
    bins = {"dWx": (0, 5), "dWy": (0,), "dW": (0, 6)}                       # DC; Nyquist where the axis keeps it
    moved = dict(inp)
    for wk, gk in S.GRADS.items():
        if wk in inp:
            moved[wk] = inp[wk].clone()
            for b in bins[gk]:
                moved[wk][:, :, b, 1] += 3.0
                scale = float(ref[gk].abs().max())
                assert float(ref[gk][:, :, b, 1].abs().max()) <= 1e-13 * scale, (gk, b)
                assert float(ref[gk][:, :, b, 0].abs().max()) > 1e-3 * scale
    out = S.run_oracle(case, inp=moved)
    assert S.rel(out["out"], ref["out"]) <= 1e-13 and S.rel(out["dx"], ref["dx"]) <= 1e-13
    moved["w" if case.kind == "1d" else "wy"][:, :, 1, 1] += 3.0            # (an interior bin does matter)
    assert S.rel(S.run_oracle(case, inp=moved)["out"], ref["out"]) > 1e-2


# ---- the tables --------------------------------------------------------------------------------------------------------
def test_case_tables_reach_the_branches_they_name():
    names = [c.name for c in S.CASES_2D + S.CASES_1D]
    assert len(set(names)) == len(names)
    for c in S.CASES_2D:
        assert S.fused_ok(c) == c.name.startswith("F-"), c
        B, M, N, C, K = c.dims
        assert B * M * N * C <= 5 * 256 * 256 * 64                          # no case larger than F-chunk
    sw = {c.name: dict(S.legs(c)) for c in S.CASES_2D}
    assert all(not sw[c.name] for c in S.CASES_2D if not S.fused_ok(c))
    assert sw["F-r48"]["RPDE_SYN3"] == "same" and sw["F-r8"]["RPDE_SYN3"] == "same"
    assert "RPDE_SYN3" not in sw["F-nyq"] and "RPDE_ANA_SQ" not in sw["F-rect24"]
    assert sw["F-chunk"]["RPDE_ANA_SQ"] == "differ" and sw["F-lowpass"]["RPDE_FUSED_MIX"] == "same"
    # Nyquist on the fused path; the clamp per axis; the partial last chunk of the two-read analysis
    assert S.keffs(S.by_name("F-nyq")) == {"dWy": 17, "dWx": 17}
    assert S.keffs(S.by_name("G-clamp")) == {"dWy": 17, "dWx": 20}
    B, M, N, C, K = S.by_name("F-chunk").dims
    chunk = (64 << 20) // (M * N * C * 4)
    assert 1 < chunk < B and B % chunk != 0
    # mixw_slabs at both clamps, and between them
    slabs = lambda c: min(12, max(1, min(c.dims[0] * c.dims[1], c.dims[0] * c.dims[2]) // 32 // 4))
    assert [slabs(S.by_name(n)) for n in ("F-nyq", "F-r40", "F-many")] == [1, 4, 12]
    assert (25 * 64 // 32) % 12 != 0                                        # uneven slabs
    # mix1d: rows <= 64 and C in {32, 64, 128}
    rows = lambda c: max(c.dims[0] * c.dims[1], c.dims[0] * c.dims[2]) if c.kind == "2d" else c.dims[0]
    mix1d = lambda c: rows(c) <= 64 and c.dims[-2] in (32, 64, 128)
    assert [mix1d(S.by_name(n)) for n in ("G-mix1d", "G-gemm32", "G-c48", "H-bwd", "H-fwd", "H-rows", "H-c48", "H-lowpass")] == \
        [True, False, False, True, True, False, False, True]
    assert S.keffs(S.by_name("H-fwd")) == {"dW": 25} and S.by_name("H-fwd").dims[-1] == 30
    assert {c.norm for c in S.CASES_1D} == {"ortho", "forward", "backward"}
    assert all(S.skips(c) == (True,) for c in S.CASES_1D)


def test_ramp_exceeds_the_running_scale_at_every_chunk():
    """each later 32-point chunk of a line is 2^3 larger than the one before, along both axes: its largest magnitude has a
    larger exponent than everything the line has shown so far"""
    x = S.inputs(S.by_name("F-ramp"))["x"]
    B, M, N, C = x.shape
    for lines in (x.reshape(B, M, N // 32, 32 * C), x.transpose(1, 2).reshape(B, N, M // 32, 32 * C)):
        e = torch.frexp(lines.abs().amax(dim=3))[1]
        assert bool((e[:, :, 1:] > e[:, :, :-1]).all())
    assert float(x.abs().max()) < 2.0 ** 24


# ---- the floor ---------------------------------------------------------------------------------------------------------
FLOOR_CASES = [c.name for c in S.CASES_2D + S.CASES_1D]


@pytest.mark.parametrize("name", FLOOR_CASES)
def test_the_float32_floor_is_a_float32_error(name):
    """every statistic of the float32 oracle is a float32 rounding error: above zero, below 1e-6, and inside the
    whole-tensor bounds the device is held to -- a degenerate floor cannot loosen or void a bound unnoticed"""
    case = S.by_name(name)
    for skip in S.skips(case):
        fl = S.floor(case, skip)
        assert set(fl) == {"out", "dx"} | (set(S.keffs(case)) if case.mode == "full" else set())
        assert not S.check(fl, fl, case)
        for k, s in fl.items():
            for stat in ("rel", "point_rel", "mode_rel"):
                if stat in s:
                    assert 2e-8 < s[stat] < 1e-6, (name, skip, k, stat, s[stat])
            assert s.get("stray", 0.0) == 0.0


# ---- planted faults ----------------------------------------------------------------------------------------------------
def _planted(case, skip, edit):
    """statistics of the float32 oracle's results after edit(results) -> the checker's failures"""
    got = {k: v.clone() for k, v in S.add_skip(S.oracle32(case), case, skip).items()}
    edit(got)
    return S.stats(case, got, S.oracle(case, skip))


MID = S.by_name("F-r40")._replace(name="F-r40/B2", dims=(2, 64, 64, 64, 20))


def test_one_wrong_point_is_caught_by_point_rel_only():
    """one of the 2 * 64 * 64 grid points of `out` off by 1e-4 of its norm moves rel by 1e-4 / sqrt(8192) = 1.1e-6, inside
    the bound of 2e-6, and stands more than ten times above the point_rel bound"""
    fl = S.floor(MID)

    def edit(got):
        p = got["out"][1, 37, 15]
        p += 1e-4 * p.norm() / 8.0                                          # (64 channels: the shift has norm 1e-4 |p|)
    st = _planted(MID, False, edit)
    bound = S.factor(MID, "out", "point_rel") * fl["out"]["point_rel"]
    assert st["out"]["rel"] <= S.FWD_TOL, st["out"]
    assert st["out"]["point_rel"] > 10 * bound, (st["out"], bound)
    bad = S.check(st, fl, MID)
    assert [b[:2] for b in bad] == [("out", "point_rel")], bad


def test_one_wrong_mode_is_caught_by_mode_rel_only():
    """one mode of dWx multiplied by 1 + 1e-4.  rel sees 1e-4 |mode| / |dWx| and mode_rel 1e-4 |mode| / RMS mode norm, which
    is sqrt(keff) times as much when every mode has the RMS norm: on F-r40 rel would stand at 1e-4 / sqrt(20) = 2.2e-5 and see
    the fault too.  Both conditions -- rel <= 5e-6, mode_rel ten times above a bound of up to 8 floors of 2.5e-7 -- need a
    mode whose share s = |mode| / RMS lies in 0.2 <= s <= 0.05 sqrt(keff): here keff = 65 (a 128 x 128 grid off the fused
    path), and the cotangent is damped at x-frequency 7 to leave that mode a share of 0.27"""
    case = S.Case("mode-fault", "2d", (1, 128, 128, 16, 65))
    inp = dict(S.inputs(case))
    G = torch.fft.rfft(inp["g"], dim=1)
    G[:, 7] *= 0.27
    inp["g"] = torch.fft.irfft(G, n=128, dim=1).contiguous()
    ref = S.run_oracle(case, inp=inp)
    got = S.run_oracle(case, torch.float32, inp=inp)
    fl = S.stats(case, got, ref)
    scale = S.mode_scale(ref["dWy"], ref["dWx"])
    share = float(S.mode_norms(ref["dWx"])[7]) / scale
    bound = S.factor(case, "dWx", "mode_rel") * fl["dWx"]["mode_rel"]
    assert 10 * bound / 1e-4 < 0.9 * share and share < 0.9 * S.GRAD_TOL * float(ref["dWx"].norm()) / scale / 1e-4, (share, bound)
    assert not S.check(fl, fl, case)
    got["dWx"][:, :, 7] *= 1.0 + 1e-4
    st = S.stats(case, got, ref)
    assert st["dWx"]["rel"] <= S.GRAD_TOL, st["dWx"]
    assert st["dWx"]["mode_rel"] > 10 * bound, (st["dWx"], bound)
    bad = S.check(st, fl, case)
    assert [b[:2] for b in bad] == [("dWx", "mode_rel")], bad


def _variant(case, fn, skip=False):
    got = S.add_skip(S.run_oracle(case, torch.float32, fn=fn), case, skip)
    return S.check(S.stats(case, got, S.oracle(case, skip)), S.floor(case, skip), case)


def test_a_single_clamp_for_both_axes_is_caught():
    """min(K, min(M, N) // 2 + 1) for both axes on G-clamp: the x axis loses its modes 17 .. 19"""
    case = S.by_name("G-clamp")
    B, M, N, C, K = case.dims

    def one_clamp(c, t):
        return S.R.fspectral2d_fourier(t["x"], t["wy"], t["wx"], min(K, min(M, N) // 2 + 1), "full")
    bad = _variant(case, one_clamp)
    assert {b[0] for b in bad} >= {"out", "dx", "dWx"} and ("dWx", "mode_rel") in [b[:2] for b in bad], bad
    assert not _variant(case, S.layer)


def test_a_kept_imaginary_nyquist_part_is_caught():
    """a complex inverse transform of the Hermitian extension in place of irfft, on F-nyq: the imaginary part of the
    Nyquist bin of the mixed spectrum comes out as an imaginary field that a real inverse never forms; here it is added"""
    case = S.by_name("F-nyq")

    def c2c(z, n, dim):
        z = z.movedim(dim, -1)
        full = torch.cat([z, z[..., 1:n // 2].conj().flip(-1)], dim=-1)
        y = torch.fft.ifft(full, dim=-1, norm="ortho")
        return (y.real + y.imag).movedim(-1, dim)

    def layer(c, t):
        B, M, N, C, K = c.dims
        xt = t["x"].permute(0, 3, 1, 2)
        fy = torch.fft.rfft(xt, dim=-1, norm="ortho")
        oy = torch.einsum("bixy,ioy->boxy", fy, torch.view_as_complex(t["wy"].contiguous()))
        fx = torch.fft.rfft(xt, dim=-2, norm="ortho")
        ox = torch.einsum("bixy,iox->boxy", fx, torch.view_as_complex(t["wx"].contiguous()))
        return (c2c(oy, N, -1) + c2c(ox, M, -2)).permute(0, 2, 3, 1)
    bad = _variant(case, layer)
    assert {b[0] for b in bad} == {"out", "dx", "dWy", "dWx"}, bad
    # (with the Nyquist weights real the same transform is the layer: the variant differs in nothing else)
    inp = dict(S.inputs(case))
    for k in ("wy", "wx"):
        inp[k] = inp[k].clone()
        inp[k][:, :, (0, 16), 1] = 0.0
    a, b = S.run_oracle(case, inp=inp, fn=layer), S.run_oracle(case, inp=inp)
    assert all(S.rel(a[k], b[k]) < 1e-12 for k in ("out", "dx"))


def test_a_dropped_skip_gradient_is_caught():
    for case in (MID, S.by_name("H-bwd")):
        got = S.oracle32(case)                                              # dx without g2
        bad = S.check(S.stats(case, got, S.oracle(case, True)), S.floor(case, True), case)
        assert {b[:2] for b in bad} == {("dx", "rel"), ("dx", "point_rel")}, bad


def test_a_gradient_in_a_mode_past_keff_is_caught():
    for name, k in (("G-clamp", "dWy"), ("H-fwd", "dW")):
        case = S.by_name(name)
        skip = S.skips(case)[-1]
        keff = S.keffs(case)[k]

        def edit(got):
            got[k][3, 5, keff, 1] = 1e-30
        bad = S.check(_planted(case, skip, edit), S.floor(case, skip), case)
        assert [b[:2] for b in bad] == [(k, "modes >= keff are not exactly zero")], bad


def test_a_non_finite_value_is_caught():
    def edit(got):
        got["dx"][0, 0, 0, 0] = float("nan")
    bad = S.check(_planted(MID, False, edit), S.floor(MID), MID)
    assert bad == [("dx", "wrong shape or not finite")]
