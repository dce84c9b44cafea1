"""What the complex-symbol path of the 1-D exponential-time-differencing generator decides without a GPU: the tables of
rpde.ops.etd1d_tables_cx against the restatement tests/etd1d_cx_ref.py, the restatement itself against two closed forms
(so that the yardstick of the device tests is pinned), that the parity inputs tell wrong tables from right ones, the
argument errors of rpde_etd1d_steps_cx, and the host side of data_generation/kdv_1d.py."""
import math
import os

import pytest
import torch

from tests import etd1d_cx_ref as C
from tests import etd1d_ref as R
from tests.conftest import DROPIN

FAKE = 1 << 20      # a pointer that is never dereferenced: argument errors come before any device work


# ---- 1. tables -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sym", [("kdv", (0.0, 0.0, 1.0, 0.0)), ("advburg", (-1.0, -0.1, 0.0, 0.0)),
                                      ("all four", (0.7, 1.0, -0.3, -0.05))])
def test_tables_equal_the_restatement_rounded_once(name, sym):
    from rpde import ops
    N, length, dt = 48, 12.0, 0.01
    K, kp = N // 2 + 1, 28
    c1, c2, c3, c4 = sym
    got = ops.etd1d_tables_cx(N, length, c1, c2, c3, c4, dt)
    want = C.tables(N, length, c1, c2, c3, c4, dt)
    assert len(got) == 7
    for tn, t, w in zip("E E2 Q f1 f2 f3".split(), got[:6], want[:6]):
        assert t.dtype == torch.float32 and tuple(t.shape) == (2, kp) and t.is_contiguous() and not t.is_cuda, tn
        assert not t[:, K:].any(), tn                                           # padding zero
        assert torch.equal(t[0, :K], w.real.float()) and torch.equal(t[1, :K], w.imag.float()), tn
        assert float(t[1, N // 2]) == 0.0 and float(t[1, 0]) == 0.0, tn         # Nyquist and mean: real
        assert t[1, 1:N // 2].any(), tn                                         # and the rest is not
    g = got[6]
    assert g.dtype == torch.float32 and tuple(g.shape) == (kp,) and not g[K:].any()
    assert torch.equal(g, ops.etd1d_tables(N, length, c2, c4, dt)[6])           # g does not depend on the symbol
    assert torch.equal(g[:K], want[6].float())
    E = got[0]
    assert float(E[0, 0]) == 1.0                                                # the mean mode: conserved
    # |E| = exp(h Re l): the odd terms only turn the phase
    mod = torch.hypot(E[0, :K].double(), E[1, :K].double())
    kappa = 2 * math.pi * torch.arange(K, dtype=torch.float64) / length
    assert torch.allclose(mod, torch.exp(dt * (c2 * kappa ** 2 + c4 * kappa ** 4)), rtol=2e-7, atol=0)
    with pytest.raises(ValueError):
        ops.etd1d_tables_cx(31, 2.0, 0.0, -1.0, 1.0, 0.0, dt)
    with pytest.raises(ValueError):
        ops.etd1d_tables_cx(32, 2.0, 0.0, -1.0, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        ops.etd1d_tables_cx(32, -2.0, 0.0, -1.0, 1.0, 0.0, dt)


@pytest.mark.parametrize("pde", ["ks", "burgers"])
def test_even_symbol_gives_the_real_tables(pde):
    """c1 = c3 = 0: z is real, the full circle is symmetric about the real axis, so its mean is real -- exactly, the
    imaginary plane rounds to zero -- and equals Re of the half-circle mean: another quadrature of the same integral,
    both exact to float64 rounding, so the fp32 values agree within 2 ulp"""
    from rpde import ops
    N, dt = 48, 0.01
    length, (c2, c4) = (12.0, R.ks_symbol(0.05)) if pde == "ks" else (2.0, R.burgers_symbol(0.1 / math.pi))
    K = N // 2 + 1
    cx = ops.etd1d_tables_cx(N, length, 0.0, c2, 0.0, c4, dt)
    re = ops.etd1d_tables(N, length, c2, c4, dt)
    for name, a, b in zip("E E2 Q f1 f2 f3".split(), cx[:6], re[:6]):
        assert not a[1].any(), name
        ulp = torch.maximum(b.abs(), torch.full_like(b, 2.0 ** -126)) * 2.0 ** -23
        assert bool(((a[0] - b).abs() <= 2 * ulp).all()), (name, float(((a[0] - b).abs() / ulp).max()))
        assert a[0, :K].any(), name
    assert torch.equal(cx[6], re[6])


# ---- 2. the restatement against closed forms -------------------------------------------------------------------------
def test_restatement_carries_the_kdv_soliton():
    """u = 3 c sech^2(sqrt(c) (x - x0 - c t) / 2) solves u_t + u u_x + u_xxx = 0; c = 4 on L = 32 (tails 1e-27 at the
    period), 256 points, 1000 steps of 1e-3.  Measured 2.3e-9 .. 5.2e-9 over the four snapshots; the unmoved profile is
    1.41 away at the last."""
    N, L, c, x0, dt = 256, 32.0, 4.0, 8.0, 1e-3
    u0 = C.soliton(N, L, c, x0, 0.0)
    sol = C.solve(u0, L, 0.0, 0.0, 1.0, 0.0, dt, 1000, 250)
    errs = [R.rel(sol[:, k], C.soliton(N, L, c, x0, 0.25 * (k + 1))) for k in range(4)]
    print(f"[etd1d cx soliton] float64 restatement rel-L2 {['%.2e' % e for e in errs]}")
    assert all(e < 1e-7 for e in errs), errs
    assert R.rel(u0, C.soliton(N, L, c, x0, 1.0)) > 1.0


def test_restatement_advects_and_diffuses_in_closed_form():
    """advect = 0 with c1 = -a, c2 = -nu.  Measured 8e-16; the profile at t = 0 is 0.43 away."""
    p = C.ADV
    T = p["steps"] * p["dt"]
    u0, exact = C.advection_diffusion(p["N"], p["L"], p["a"], p["nu"], 0.0), C.advection_diffusion(p["N"], p["L"], p["a"], p["nu"], T)
    sol = C.solve(u0, p["L"], -p["a"], -p["nu"], 0.0, 0.0, p["dt"], p["steps"], p["steps"], advect=0.0)
    err = R.rel(sol[:, 0], exact)
    print(f"[etd1d cx advection-diffusion] float64 restatement rel-L2 {err:.2e}")
    assert err < 1e-12, err
    assert R.rel(u0, exact) > 0.3


# ---- 3. the parity inputs tell wrong tables from right ones ----------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_wrong_tables_miss_the_kdv_parity_cases(case):
    """the real path's contour (upper half circle, Re<.>) and full-circle tables without their imaginary parts, on the
    kdv family: each is further from the float64 run than 100 times the bound of the device test, at the last snapshot.
    Measured: half circle 2.7e-3 (N = 512) .. 0.16, real parts only 0.078 .. 1.4; 100 x 4 x floor32 is 5.5e-4 .. 1.1e-3."""
    ref = C.parity_reference("kdv", case)
    sym = (ref["c1"], ref["c2"], ref["c3"], ref["c4"])
    every = C.STEPS // C.SNAPSHOTS
    bound = 100 * C.FLOOR_FACTOR * ref["floor32"][-1]
    for variant in ("half", "real"):
        wrong = C.solve(ref["u0"], ref["length"], *sym, ref["dt"], C.STEPS, every, variant=variant)
        miss = R.rel(wrong[:, -1], ref["sol64"][:, -1])
        print(f"[etd1d cx wrong tables] {variant} {C.case_id(case)}: {miss:.2e} against {bound:.2e}")
        assert miss > bound or not math.isfinite(miss), (variant, miss, bound)


# ---- 4. ABI ----------------------------------------------------------------------------------------------------------
def test_steps_cx_argument_errors_are_reported_without_a_gpu():
    from rpde import _lib as L
    lib = L.load()
    nws = lib.rpde_etd1d_ws_bytes(2, 48)

    def steps(B=2, N=48, nsteps=1, U=FAKE, tab=FAKE, ws=FAKE, n=nws, g=FAKE):
        return lib.rpde_etd1d_steps_cx(U, tab, FAKE, FAKE, FAKE, FAKE, FAKE, g, B, N, nsteps, ws, n, None)

    assert lib.rpde_etd1d_steps_cx(None, *([FAKE] * 7), 2, 48, 1, FAKE, nws, None) == L.ERR_ARG
    assert b"etd1d_steps_cx" in lib.rpde_last_error() and b"null" in lib.rpde_last_error()
    for kw in (dict(tab=None), dict(g=None), dict(ws=None)):
        assert steps(**kw) == L.ERR_ARG and b"null" in lib.rpde_last_error(), kw
    for B, N in ((2, 47), (2, 2), (2, 4098), (0, 48), (-1, 48), (65536, 48)):
        assert steps(B=B, N=N) == L.ERR_ARG, (B, N)
        assert b"etd1d_steps_cx" in lib.rpde_last_error() and b"bad B=" in lib.rpde_last_error()
    assert steps(n=nws // 16) == L.ERR_WORKSPACE and b"workspace too small" in lib.rpde_last_error()
    assert steps(ws=FAKE + 64) == L.ERR_ARG and b"aligned" in lib.rpde_last_error()
    assert steps(nsteps=-1) == L.ERR_ARG and b"nsteps" in lib.rpde_last_error()
    for kw in (dict(U=FAKE + 4), dict(tab=FAKE + 8), dict(g=FAKE + 4)):
        assert steps(**kw) == L.ERR_ARG and b"aligned" in lib.rpde_last_error(), kw
    # zero steps with good arguments: nothing to do, no device touched; the arguments are still checked
    assert steps(nsteps=0) == 0
    assert steps(nsteps=0, n=nws // 16) == L.ERR_WORKSPACE
    assert steps(N=47, nsteps=0) == L.ERR_ARG


# ---- 5. host side ----------------------------------------------------------------------------------------------------
def test_solve_rejects_malformed_table_sets():
    from rpde import ops
    from rpde._lib import RpdeError
    N, kp = 16, 12
    re = ops.etd1d_tables(N, 4.0, -0.1, 0.0, 1e-3)
    cx = ops.etd1d_tables_cx(N, 4.0, 0.0, -0.1, 1.0, 0.0, 1e-3)
    u0 = torch.zeros(1, N)
    bad = [re[:6], cx[:6], re + re[:1], cx[:6] + (cx[0],),                      # counts; g complex
           cx[:5] + (re[5], cx[6]), re[:6] + (cx[0],),                          # mixed kinds
           tuple(t[:, :kp - 4] for t in cx[:6]) + (cx[6],),                     # another grid's
           tuple(t.t().contiguous() for t in cx[:6]) + (cx[6],)]                # [kp, 2]
    for tabs in bad:
        with pytest.raises(ValueError, match="etd1d_tables_cx"):
            ops.etd1d_solve(u0, tabs, 1, 1)
    for tabs in (re, cx):                                                       # well formed: refused as CPU tensors only
        with pytest.raises(RpdeError, match="GPU"):
            ops.etd1d_solve(u0, tabs, 1, 1)


def test_kdv_functions_check_their_arguments_before_the_device():
    from data_generation.etd1d import integrate
    from data_generation.kdv_1d import kdv_1d, kdv_path
    u0 = torch.zeros(1, 16)                                                     # a CPU tensor: never reached
    with pytest.raises(ValueError, match="whole number"):
        kdv_1d(u0, 4.0, 1.0, 0.3, 2)
    with pytest.raises(ValueError, match="viscosity"):
        kdv_1d(u0, 4.0, 1.0, 0.1, 2, viscosity=-1.0)
    with pytest.raises(ValueError, match="dispersion"):
        kdv_1d(u0, 4.0, 1.0, 0.1, 2, dispersion=0.0)
    with pytest.raises(ValueError, match="whole number"):
        integrate(u0, 4.0, -0.1, 0.0, 1.0, 0.3, 2, c1=-1.0)
    assert kdv_path("o", "train", 64, 10) == os.path.join("o", "res_64", "KdV_train_10.npz")
    assert kdv_path("o", "valid", 64, 10) == os.path.join("o", "res_64", "KdV_valid.npz")
    assert kdv_path("o", "test", 64, 10, flat=True) == os.path.join("o", "KdV_test.npz")


def test_kdv_script_reports_argument_errors_before_the_device(tmp_path, capsys, monkeypatch):
    from data_generation import kdv_1d
    out = str(tmp_path)
    bad = [["--out", out, "--nte", "52"],                                       # nte > nt
           ["--out", out, "--nt", "52"],                                        # 5 / 51 is no whole number of steps
           ["--out", out, "--dt", "0.03"],                                      # 3.33 steps per snapshot
           ["--out", out, "--flat", "--resolutions", "64,32"],
           ["--out", out, "--resolutions", "64,64"],
           ["--out", out, "--resolution", "63"],
           ["--out", out, "--split", "validation"],
           ["--out", out, "--dispersion", "0"],
           ["--out", out, "--viscosity", "-0.1"],
           ["--out", out, "--amplitude", "0"],
           ["--out", out, "--samples", "0"]]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            kdv_1d.main(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="GPU"):
        kdv_1d.main(["--out", out, "--samples", "2", "--resolution", "32"])
    assert os.listdir(out) == []


def test_kdv_config_composes_and_its_target_resolves():
    import importlib
    from rpde.config import compose
    cfg = compose(os.path.join(DROPIN, "conf"), "config", ["dataset=kdv/kdv_generated"])
    assert cfg.dataset.pde == "kdv" and cfg.dataset.dims == 1
    p = cfg.dataset.dataset_params
    assert (p.filename, p.val_filename, p.test_filename) == ("KdV_train_2048.npz", "KdV_valid.npz", "KdV_test.npz")
    mod, _, name = p["_target_"].rpartition(".")
    assert callable(getattr(importlib.import_module(mod), name))
    ks = compose(os.path.join(DROPIN, "conf"), "config", ["dataset=ks/ks_generated"]).dataset
    assert set(dict(p)) == set(dict(ks.dataset_params)) and p["_target_"] == ks.dataset_params["_target_"]
    from dataloaders.ks_naive_markov import _split_of
    assert [_split_of(f, print) for f in (p.filename, p.val_filename, p.test_filename)] == ["train", "valid", "test"]
