"""What the active-scalar Navier-Stokes generator decides without a GPU: the float64 restatement tests/nsc_solver_ref.py
against a closed form that uses none of its nonlinear code, the conservation of the scalar's mean, the coefficient
tables, the conditions on the parity inputs, utils.res_utils.downsample against the reference's operator
(tests/golden/downsample2d.npz) and the argument errors of the C ABI."""
import os

import numpy as np
import pytest
import torch

from tests import ns_solver_ref as R
from tests import nsc_solver_ref as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "downsample2d.npz")


def test_restatement_matches_the_closed_form():
    w0, c0, f, theta, par = C.closed_form_inputs()
    w, c = C.closed_form(theta, **par)
    fields, vort, _ = C.solve(w0, c0, f, par["visc"], par["kappa"], par["beta"], par["steps"] * par["dt"], par["dt"], 1)
    ew, ec = C.rel(vort[0, 0], w), C.rel(fields[0, 0, 0], c)
    print(f"[nsc closed form] float64 restatement: w {ew:.1e}, c {ec:.1e}")
    assert ew <= 1e-12 and ec <= 1e-12, (ew, ec)
    assert C.rel(w, w0[0]) > 0.5                           # buoyancy moved the vorticity: the recurrence is not the decay


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_scalar_mean_is_conserved_and_inputs_exercise_both_terms(case):
    ref = C.parity_reference(case)
    m0 = ref["c0"].mean(dim=(-2, -1))
    drift = max(float((ref["fields64"][:, n, 0].mean(dim=(-2, -1)) - m0).abs().max()) for n in range(C.RECORD_STEPS))
    print(f"[nsc inputs] {C.case_id(case)}: mean drift {drift:.1e}, buoyancy share {ref['buoyancy_share']:.2f}, "
          f"advection share {ref['advection_share']:.2f}, floor32 {[['%.1e' % v for v in ch] for ch in ref['floor32']]}")
    assert drift <= 1e-12, drift
    assert ref["buoyancy_share"] >= 0.1, ref["buoyancy_share"]
    assert ref["advection_share"] >= 0.1, ref["advection_share"]


def test_step_tables():
    from rpde import ops
    M, N, dt = 16, 24, C.DT
    K = N // 2 + 1
    got = ops.nsc2d_tables(M, N, C.VISC, C.KAPPA, dt)
    want = C.tables(M, N, C.VISC, C.KAPPA, dt)
    assert len(got) == 6
    for name, g, w in zip(("c_w", "c_f", "d_w", "d_f", "c_g", "inv_lap"), got, want):
        assert g.dtype == torch.float32 and tuple(g.shape) == (M, 16) and not g[:, K:].any(), name
        assert torch.equal(g[:, :K], w.float()), name
    assert not torch.equal(got[0], got[2]) and not torch.equal(got[1], got[3])      # visc != kappa: the tables differ


def test_beta_zero_is_the_vorticity_solver():
    ref = C.parity_reference((2, 16, 24))
    _, vort, t = C.solve(ref["w0"], ref["c0"], ref["f"], C.VISC, C.KAPPA, 0.0, C.T_FINAL, C.DT, C.RECORD_STEPS)
    sol, sol_t = R.solve(ref["w0"], ref["f"], C.VISC, C.T_FINAL, C.DT, C.RECORD_STEPS)
    assert torch.equal(vort.permute(0, 2, 3, 1), sol) and torch.equal(t, sol_t)
    assert not torch.equal(vort, ref["vort64"])


def _resize_formula(x, n):
    """the reference-formula resize restated: rfft2, the bins both sizes share, irfft2 at n x n, scaled by (n / H)^2"""
    from oracle.reference_path import resize_2d
    return resize_2d(torch.from_numpy(x).double(), (n, n)).numpy()


def test_downsample_matches_the_reference_operator():
    from utils.res_utils import downsample
    with np.load(GOLDEN) as z:
        names = sorted({k.split("|")[0] for k in z.files if "|" in k})
        assert names == ["12to6", "16to10", "16to8", "8to8"]
        for name in names:
            x, y = z[name + "|x"], z[name + "|y"]
            assert x.shape[:2] == (2, 2) and x.dtype == np.float32
            got = downsample(x, y.shape[-1])
            assert got.shape == y.shape and got.dtype == np.float32
            err = float(np.linalg.norm(got.astype(np.float64) - y) / np.linalg.norm(y))
            print(f"[downsample] {name}: rel {err:.1e}")
            assert err <= 1e-6, (name, err)
        x, same = z["16to8|x"], z["8to8|x"]
        assert np.allclose(downsample(same, 8), same, rtol=0, atol=1e-6)       # the identity keeps every frequency
    # two operators: the Nyquist lines are treated differently
    a, b = downsample(x, 8).astype(np.float64), _resize_formula(x, 8)
    gap = float(np.linalg.norm(a - b) / np.linalg.norm(b))
    print(f"[downsample] against the resize formula, 16 -> 8: rel {gap:.3f}")
    assert gap > 0.05, gap
    with pytest.raises(ValueError):
        downsample(np.zeros((2, 8, 8), dtype=np.float32), 4)


# a pointer that is never dereferenced: argument errors come before any device work
FAKE = 1 << 20


def test_argument_errors_are_reported_without_a_gpu():
    from rpde import _lib as L
    lib = L.load()
    nws = lib.rpde_nsc2d_ws_bytes(2, 16, 24)
    assert nws > 0
    # the ws query: odd or out-of-range axes, no batch, and 6 B derivative images beyond a grid dimension
    for B, M, N in ((2, 15, 24), (2, 16, 23), (2, 2, 16), (2, 16, 2), (2, 4098, 16), (2, 16, 4098), (0, 16, 16), (-1, 16, 16),
                    (10923, 4, 4), (65535, 4, 4), (1 << 30, 4, 4)):
        assert lib.rpde_nsc2d_ws_bytes(B, M, N) == 0, (B, M, N)
    assert lib.rpde_nsc2d_ws_bytes(10922, 4, 4) > 0                              # 6 B = 65532
    sizes = [lib.rpde_nsc2d_ws_bytes(B, 32, 48) for B in (1, 2, 8)]
    assert 0 < sizes[0] < sizes[1] < sizes[2]
    # at least the 16 B spectra and the 8 B fields of a step
    assert lib.rpde_nsc2d_ws_bytes(4, 32, 48) >= 4 * (16 * lib.rpde_ns2d_spec_elems(4, 32, 48) + 8 * 4 * 32 * 48)
    steps = lambda B, M, N, ws=FAKE, n=nws, k=1, S=FAKE, g=FAKE: lib.rpde_nsc2d_steps(            # noqa: E731
        S, g, 0, FAKE, FAKE, FAKE, FAKE, FAKE, 5.0, B, M, N, k, ws, n, None)
    fields = lambda B, M, N, ws=FAKE, n=nws, **_: lib.rpde_nsc2d_fields(FAKE, FAKE, FAKE, B, M, N, ws, n, None)   # noqa: E731
    for name, call in (("nsc2d_steps", steps), ("nsc2d_fields", fields)):
        for B, M, N in ((2, 15, 24), (2, 16, 23), (2, 2, 16), (2, 4098, 16), (0, 16, 16), (10923, 16, 16)):
            assert call(B, M, N) == L.ERR_ARG, (name, B, M, N)
            assert name.encode() in lib.rpde_last_error() and b"bad B=" in lib.rpde_last_error()
        assert call(2, 16, 24, n=nws // 64) == L.ERR_WORKSPACE, name           # short workspace
        assert b"workspace too small" in lib.rpde_last_error()
        assert call(2, 16, 24, ws=FAKE + 64) == L.ERR_ARG, name                # misaligned workspace
        assert b"aligned" in lib.rpde_last_error()
        assert call(2, 16, 24, ws=None) == L.ERR_ARG, name                     # null workspace
        assert b"null" in lib.rpde_last_error()
    assert steps(2, 16, 24, g=None) == L.ERR_ARG and b"null" in lib.rpde_last_error()
    assert steps(2, 16, 24, k=-1) == L.ERR_ARG and b"nsteps" in lib.rpde_last_error()
    assert steps(2, 16, 24, S=FAKE + 4) == L.ERR_ARG and b"aligned" in lib.rpde_last_error()
    assert lib.rpde_nsc2d_fields(FAKE, FAKE, FAKE + 4, 2, 16, 24, FAKE, nws, None) == L.ERR_ARG
    # zero steps with good arguments: nothing to do, no device touched
    assert steps(2, 16, 24, k=0) == 0


def test_cpu_tensors_are_refused():
    from rpde import ops
    from rpde._lib import RpdeError
    z = torch.zeros(1, 16, 16)
    with pytest.raises(RpdeError, match="GPU"):
        ops.nsc2d_solve(z, z, z[0], 1e-3, 1e-3, 1.0, 1e-3, 1, 1)
    with pytest.raises(RpdeError, match="GPU"):
        ops.nsc2d_fields(z, z)
    from data_generation.active_scalar_2d import active_scalar_2d, file_name
    with pytest.raises(ValueError, match="snapshots"):                         # the schedule comes before the device
        active_scalar_2d(z, z, z[0], 1e-3, 1e-3, 1.0, 0.01, 1e-3, 20)
    assert file_name(1e-3, 2e-3, 5.0, 1) == "active_scalar_visc_0.001_kappa_0.002_beta_5_1.npz"
