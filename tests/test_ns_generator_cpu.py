"""What the Navier-Stokes generator decides without a GPU: argument errors of the C ABI, workspace sizes, the errors of
GaussianRF, the record arithmetic of navier_stokes_2d and the coefficient tables of the step."""
import math

import pytest
import torch

from tests import ns_solver_ref as R


def _lib():
    from rpde import _lib
    return _lib, _lib.load()


# a pointer that is never dereferenced: argument errors come before any device work
FAKE = 1 << 20


def test_argument_errors_are_reported_without_a_gpu():
    L, lib = _lib()
    nws = lib.rpde_ns2d_ws_bytes(2, 16, 24)
    calls = {
        "ns2d_rfft2": lambda B, M, N, ws=FAKE, n=nws: lib.rpde_ns2d_rfft2(FAKE, FAKE, B, M, N, ws, n, None),
        "ns2d_irfft2": lambda B, M, N, ws=FAKE, n=nws: lib.rpde_ns2d_irfft2(FAKE, FAKE, B, M, N, ws, n, None),
        "ns2d_steps": lambda B, M, N, ws=FAKE, n=nws: lib.rpde_ns2d_steps(FAKE, FAKE, 0, FAKE, FAKE, FAKE, B, M, N, 1, ws, n, None),
        "grf2d": lambda B, M, N, ws=FAKE, n=nws: lib.rpde_grf2d(FAKE, FAKE, FAKE, B, M, N, ws, n, None),
    }
    for name, call in calls.items():
        for B, M, N in ((2, 15, 24), (2, 16, 23), (2, 2, 16), (2, 16, 2), (2, 4098, 16), (2, 16, 4098), (0, 16, 16)):
            assert call(B, M, N) == L.ERR_ARG, (name, B, M, N)
            assert name.encode() in lib.rpde_last_error() and b"bad B=" in lib.rpde_last_error()
        assert call(2, 16, 24, n=nws // 16) == L.ERR_WORKSPACE, name           # short workspace
        assert b"workspace too small" in lib.rpde_last_error()
        assert call(2, 16, 24, ws=FAKE + 64) == L.ERR_ARG, name                # misaligned workspace
        assert b"aligned" in lib.rpde_last_error()
        assert call(2, 16, 24, ws=None) == L.ERR_ARG, name                     # null workspace
        assert b"null" in lib.rpde_last_error()
    assert lib.rpde_ns2d_rfft2(None, FAKE, 2, 16, 24, FAKE, nws, None) == L.ERR_ARG
    assert lib.rpde_ns2d_irfft2(FAKE, None, 2, 16, 24, FAKE, nws, None) == L.ERR_ARG
    assert lib.rpde_ns2d_steps(FAKE, None, 0, FAKE, FAKE, FAKE, 2, 16, 24, 1, FAKE, nws, None) == L.ERR_ARG
    assert lib.rpde_ns2d_scale(FAKE, None, FAKE, 2, 16, 24, None) == L.ERR_ARG
    assert lib.rpde_grf2d(FAKE, None, FAKE, 2, 16, 24, FAKE, nws, None) == L.ERR_ARG
    assert b"null" in lib.rpde_last_error()
    assert lib.rpde_ns2d_steps(FAKE, FAKE, 0, FAKE, FAKE, FAKE, 2, 16, 24, -1, FAKE, nws, None) == L.ERR_ARG
    assert b"nsteps" in lib.rpde_last_error()
    assert lib.rpde_ns2d_steps(FAKE + 4, FAKE, 0, FAKE, FAKE, FAKE, 2, 16, 24, 1, FAKE, nws, None) == L.ERR_ARG
    assert b"aligned" in lib.rpde_last_error()
    # the batch is a grid dimension (B <= 65535), which also keeps 4 B max(M, N) below 2^31
    assert lib.rpde_ns2d_steps(FAKE, FAKE, 0, FAKE, FAKE, FAKE, 65536, 16, 16, 1, FAKE, nws, None) == L.ERR_ARG
    assert lib.rpde_ns2d_ws_bytes(65536, 16, 16) == 0 and lib.rpde_ns2d_ws_bytes(65535, 4, 4) > 0
    # zero steps with good arguments: nothing to do, no device touched
    assert lib.rpde_ns2d_steps(FAKE, FAKE, 0, FAKE, FAKE, FAKE, 2, 16, 24, 0, FAKE, nws, None) == 0


def test_workspace_and_spectrum_sizes():
    _, lib = _lib()
    assert lib.rpde_ns2d_spec_elems(3, 16, 24) == 3 * 16 * 2 * 16              # kp = 13 rounded up to 16
    assert lib.rpde_ns2d_spec_elems(1, 64, 64) == 64 * 2 * 36
    for q in (lib.rpde_ns2d_ws_bytes, lib.rpde_grf2d_ws_bytes):
        sizes = [q(B, 32, 48) for B in (1, 2, 8)]
        assert sizes[0] > 0 and sizes[0] < sizes[1] < sizes[2]
        assert q(2, 31, 48) == 0 and q(2, 32, 2) == 0 and q(2, 4098, 32) == 0 and q(0, 32, 32) == 0
    # the step's workspace holds at least the 8 B derivative spectra and the 5 B fields
    B, M, N = 4, 32, 48
    assert lib.rpde_ns2d_ws_bytes(B, M, N) >= 4 * (10 * lib.rpde_ns2d_spec_elems(B, M, N) + 5 * B * M * N)


def test_gaussian_rf_refuses_what_is_not_built():
    from data_generation.random_fields import GaussianRF
    with pytest.raises(ValueError, match="dim"):
        GaussianRF(1, 64)
    with pytest.raises(ValueError, match="dim"):
        GaussianRF(3, 16)
    with pytest.raises(ValueError, match="periodic"):
        GaussianRF(2, 64, boundary="dirichlet")
    grf = GaussianRF(2, 16, alpha=2.5, tau=7)                                  # tables are host work
    assert grf.size == (16, 16) and grf.sigma == 7 ** 1.5
    assert torch.equal(grf._sqrt_eig_host, R.sqrt_eig(16, 16, 2.5, 7).float())
    assert float(grf._sqrt_eig_host[0, 0]) == 0.0


def test_record_arithmetic():
    from data_generation.ns_2d import record_schedule
    steps, record_time, times = record_schedule(3.2, 1e-4, 32)
    assert (steps, record_time, len(times)) == (32000, 1000, 32)
    assert (steps, record_time, times) == R.schedule(3.2, 1e-4, 32)
    assert abs(times[-1] - 3.2) < 1e-9 and abs(times[0] - 0.1) < 1e-9
    assert record_schedule(0.05, 1e-3, 5)[:2] == (50, 10)
    assert record_schedule(0.05, 1e-3, 5) == R.schedule(0.05, 1e-3, 5)
    # 7 steps, 2 snapshots: after steps 3 and 6
    steps, record_time, times = record_schedule(0.7, 0.1, 2)
    assert (steps, record_time, len(times)) == (7, 3, 2)
    with pytest.raises(ValueError):
        record_schedule(0.01, 1e-3, 20)                                        # 10 steps cannot hold 20 snapshots
    with pytest.raises(ValueError):
        record_schedule(1.0, 1e-3, 0)


def test_navier_stokes_2d_checks_the_schedule_before_the_device():
    from data_generation.ns_2d import navier_stokes_2d
    w0 = torch.zeros(1, 16, 16)                                                # a CPU tensor: never reached
    with pytest.raises(ValueError, match="snapshots"):
        navier_stokes_2d(w0, w0[0], 1e-3, 0.01, 1e-3, 20)


def test_cpu_tensors_are_refused():
    from rpde import ops
    from rpde._lib import RpdeError
    with pytest.raises(RpdeError, match="GPU"):
        ops.ns2d_solve(torch.zeros(1, 16, 16), torch.zeros(16, 16), 1e-3, 1e-3, 1, 1)
    with pytest.raises(RpdeError, match="GPU"):
        ops.grf2d(torch.zeros(1, 16, 16, 2), torch.zeros(16, 16))
    with pytest.raises(ValueError, match="sqrt_eig"):
        ops.grf2d(torch.zeros(1, 16, 16, 2), torch.zeros(16, 8))


def test_step_tables():
    from rpde import ops
    M, N, visc, dt = 16, 24, 1e-3, 2e-3
    c_w, c_f, c_g, inv_lap = ops.ns2d_tables(M, N, visc, dt)
    K = N // 2 + 1
    for t in (c_w, c_f, c_g, inv_lap):
        assert t.dtype == torch.float32 and tuple(t.shape) == (M, 16) and not t[:, K:].any()
    k1, k2 = R.wavenumbers(M, N)
    assert float(k1[M // 2]) == -M / 2                                         # the Nyquist row is negative
    lap = 4 * math.pi ** 2 * (k1 ** 2 + k2 ** 2)
    a = 0.5 * dt * visc * lap
    assert torch.equal(c_w[:, :K], ((1 - a) / (1 + a)).float())
    assert torch.equal(c_g[:, :K], (dt / (1 + a)).float())
    assert float(inv_lap[0, 0]) == 1.0 and float(c_w[0, 0]) == 1.0             # lap[0, 0] -> 1 in the Poisson division only
    assert torch.equal(inv_lap[:, :K].flatten()[1:], (1 / lap).flatten()[1:].float())
    # 2/3 rule: |k1| <= 5.33 of 8, |k2| <= 8 of 12
    live = c_f[:, :K] != 0
    assert live[5, 8] and live[-5, 8] and not live[6, 0] and not live[-6, 0] and not live[0, 9] and not live[8, 0]
    assert torch.equal(c_f[:, :K][live], c_g[:, :K][live])
