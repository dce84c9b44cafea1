"""What the 1-D exponential-time-differencing generator decides without a GPU: argument errors of the C ABI, workspace
sizes, the ETDRK4 tables, the 1-D Gaussian random field's table and errors, the schedule and path arithmetic of the two
scripts, and the restatement's own order of convergence (tests/etd1d_ref.py)."""
import math
import os

import pytest
import torch

from tests import etd1d_ref as R


def _lib():
    from rpde import _lib
    return _lib, _lib.load()


# a pointer that is never dereferenced: argument errors come before any device work
FAKE = 1 << 20


def _steps(lib, B, N, nsteps=1, U=FAKE, tab=FAKE, ws=FAKE, n=None, g=FAKE):
    n = lib.rpde_etd1d_ws_bytes(2, 48) if n is None else n
    return lib.rpde_etd1d_steps(U, tab, FAKE, FAKE, FAKE, FAKE, FAKE, g, B, N, nsteps, ws, n, None)


def test_argument_errors_are_reported_without_a_gpu():
    L, lib = _lib()
    nws, gws = lib.rpde_etd1d_ws_bytes(2, 48), lib.rpde_grf1d_ws_bytes(2, 48)
    assert nws > 0 and gws > 0
    calls = {
        "etd1d_rfft": lambda B, N: lib.rpde_etd1d_rfft(FAKE, FAKE, B, N, None),
        "etd1d_irfft": lambda B, N: lib.rpde_etd1d_irfft(FAKE, FAKE, B, N, None),
        "etd1d_steps": lambda B, N: _steps(lib, B, N),
        "grf1d": lambda B, N: lib.rpde_grf1d(FAKE, FAKE, FAKE, B, N, FAKE, gws, None),
    }
    for name, call in calls.items():
        for B, N in ((2, 47), (2, 2), (2, 4098), (0, 48), (-1, 48), (65536, 48)):
            assert call(B, N) == L.ERR_ARG, (name, B, N)
            assert name.encode() in lib.rpde_last_error() and b"bad B=" in lib.rpde_last_error()
    # the calls with a workspace: short, misaligned, null
    assert _steps(lib, 2, 48, n=nws // 16) == L.ERR_WORKSPACE and b"workspace too small" in lib.rpde_last_error()
    assert lib.rpde_grf1d(FAKE, FAKE, FAKE, 2, 48, FAKE, gws // 16, None) == L.ERR_WORKSPACE
    assert b"workspace too small" in lib.rpde_last_error()
    assert _steps(lib, 2, 48, ws=FAKE + 64) == L.ERR_ARG and b"aligned" in lib.rpde_last_error()
    assert lib.rpde_grf1d(FAKE, FAKE, FAKE, 2, 48, FAKE + 64, gws, None) == L.ERR_ARG and b"aligned" in lib.rpde_last_error()
    assert _steps(lib, 2, 48, ws=None) == L.ERR_ARG and b"null" in lib.rpde_last_error()
    assert lib.rpde_grf1d(FAKE, FAKE, FAKE, 2, 48, None, gws, None) == L.ERR_ARG and b"null" in lib.rpde_last_error()
    # null operands
    assert lib.rpde_etd1d_rfft(None, FAKE, 2, 48, None) == L.ERR_ARG and b"null" in lib.rpde_last_error()
    assert lib.rpde_etd1d_irfft(FAKE, None, 2, 48, None) == L.ERR_ARG and b"null" in lib.rpde_last_error()
    assert _steps(lib, 2, 48, U=None) == L.ERR_ARG and b"null" in lib.rpde_last_error()
    assert _steps(lib, 2, 48, tab=None) == L.ERR_ARG and b"null" in lib.rpde_last_error()
    assert _steps(lib, 2, 48, g=None) == L.ERR_ARG and b"null" in lib.rpde_last_error()
    assert lib.rpde_grf1d(FAKE, None, FAKE, 2, 48, FAKE, gws, None) == L.ERR_ARG and b"null" in lib.rpde_last_error()
    # negative step count; misaligned state and tables
    assert _steps(lib, 2, 48, nsteps=-1) == L.ERR_ARG and b"nsteps" in lib.rpde_last_error()
    assert _steps(lib, 2, 48, U=FAKE + 4) == L.ERR_ARG and b"aligned" in lib.rpde_last_error()
    assert _steps(lib, 2, 48, tab=FAKE + 8) == L.ERR_ARG and b"aligned" in lib.rpde_last_error()
    assert _steps(lib, 2, 48, g=FAKE + 4) == L.ERR_ARG and b"aligned" in lib.rpde_last_error()
    # the largest batch is a grid dimension
    assert _steps(lib, 65535, 4, n=lib.rpde_etd1d_ws_bytes(65535, 4), nsteps=0) == 0
    # zero steps with good arguments: nothing to do, no device touched
    assert _steps(lib, 2, 48, nsteps=0) == 0
    # ... but the arguments are still checked
    assert _steps(lib, 2, 48, nsteps=0, n=nws // 16) == L.ERR_WORKSPACE
    assert _steps(lib, 2, 47, nsteps=0) == L.ERR_ARG


def test_workspace_and_spectrum_sizes():
    _, lib = _lib()
    assert lib.rpde_etd1d_spec_elems(3, 48) == 3 * 2 * 28                      # kp = 25 rounded up to 28
    assert lib.rpde_etd1d_spec_elems(1, 256) == 2 * 132
    for q in (lib.rpde_etd1d_ws_bytes, lib.rpde_grf1d_ws_bytes, lib.rpde_etd1d_spec_elems):
        sizes = [q(B, 48) for B in (1, 2, 64)]
        assert sizes[0] > 0 and sizes[0] <= sizes[1] < sizes[2]
        assert q(2, 47) == 0 and q(2, 2) == 0 and q(2, 4098) == 0 and q(0, 48) == 0 and q(65536, 48) == 0
        assert q(65535, 4) > 0 and q(1, 4096) > 0
    # the step's workspace holds Nv, a, the running sum, b / c, the product spectrum and the field
    for B, N in ((4, 48), (3, 10), (512, 256)):
        assert lib.rpde_etd1d_ws_bytes(B, N) >= 4 * (5 * lib.rpde_etd1d_spec_elems(B, N) + B * N)
        assert lib.rpde_grf1d_ws_bytes(B, N) >= 4 * lib.rpde_etd1d_spec_elems(B, N)


@pytest.mark.parametrize("pde", ["ks", "burgers"])
def test_tables_equal_the_restatement_rounded_once(pde):
    from rpde import ops
    N, dt = 48, 0.01
    length, (c2, c4) = (12.0, R.ks_symbol(0.05)) if pde == "ks" else (2.0, R.burgers_symbol(0.1 / math.pi))
    K, kp = N // 2 + 1, 28
    got = ops.etd1d_tables(N, length, c2, c4, dt)
    want = R.tables(N, length, c2, c4, dt)
    assert len(got) == 7
    for name, t, w in zip("E E2 Q f1 f2 f3 g".split(), got, want):
        assert t.dtype == torch.float32 and tuple(t.shape) == (kp,) and not t.is_cuda, name
        assert not t[K:].any(), name                                            # padding zero
        assert torch.equal(t[:K], w.float()), name
    E, E2, Q, f1, f2, f3, g = got
    assert float(E[0]) == 1.0 and float(E2[0]) == 1.0 and float(g[0]) == 0.0    # the mean mode: conserved
    assert float(g[N // 2]) == 0.0
    # 2/3 rule: n <= 16 of 24 lives
    assert g[1:17].all() and not g[17:].any()
    assert torch.equal(g[:17], (-0.5 * (2 * math.pi / length) * torch.arange(17, dtype=torch.float64)).float())
    full = ops.etd1d_tables(N, length, c2, c4, dt, dealias=False)[6]
    assert full[1:N // 2].all() and float(full[N // 2]) == 0.0
    assert torch.equal(ops.etd1d_tables(N, length, c2, c4, dt, advect=0.0)[6], torch.zeros(kp))
    for t, w in zip(ops.etd1d_tables(N, length, c2, c4, dt, advect=0.0)[:6], got[:6]):
        assert torch.equal(t, w)                                                # the linear tables do not depend on c


def test_table_limits_for_a_vanishing_symbol():
    """c4 = 0, c2 -> 0: Q -> h/2, f1, f2, f3 -> h/6 -- where the closed forms divide 0 by 0 and fp32 loses everything"""
    from rpde import ops
    h = 0.01
    for c2 in (-1e-6, -1e-10, 0.0):
        E, E2, Q, f1, f2, f3, g = ops.etd1d_tables(32, 2.0, c2, 0.0, h)
        K = 17
        assert torch.allclose(E[:K], torch.ones(K), atol=1e-4, rtol=0)                 # |z| <= 2.6e-5
        assert torch.allclose(Q[:K], torch.full((K,), h / 2), rtol=1e-4, atol=0)
        for f in (f1, f2, f3):
            assert torch.allclose(f[:K], torch.full((K,), h / 6), rtol=1e-4, atol=0)
    # at the mean mode z = 0 exactly, for every symbol: the contour mean gives the limits to float64 rounding
    t64 = R.tables(32, 2.0, *R.ks_symbol(0.05), h)
    assert abs(float(t64[2][0]) - h / 2) < 1e-15 and all(abs(float(t64[i][0]) - h / 6) < 1e-15 for i in (3, 4, 5))
    with pytest.raises(ValueError):
        ops.etd1d_tables(31, 2.0, -1.0, 0.0, h)
    with pytest.raises(ValueError):
        ops.etd1d_tables(32, 2.0, -1.0, 0.0, 0.0)


def test_gaussian_rf_1d_table_and_errors():
    from data_generation.random_fields import GaussianRF, GaussianRF1d, sqrt_eig_1d
    for N, alpha, tau, sigma in ((32, 2, 3, None), (200, 2.0, 5.0, 25.0)):
        grf = GaussianRF1d(N, alpha=alpha, tau=tau, sigma=sigma)               # tables are host work
        want = R.sqrt_eig(N, alpha, tau, sigma)
        assert torch.equal(grf._sqrt_eig_host, want.float()) and float(grf._sqrt_eig_host[0]) == 0.0
        assert torch.equal(sqrt_eig_1d(N, alpha, tau, grf.sigma), want.float())
        assert grf.size == N and grf.dim == 1
    assert GaussianRF1d(32, alpha=2, tau=3).sigma == 3 ** 1.5                   # tau^((2 alpha - 1) / 2)
    for bad in (31, 2, 4098):
        with pytest.raises(ValueError, match="size"):
            GaussianRF1d(bad)
    with pytest.raises(ValueError, match="noise"):
        GaussianRF1d(32).sample(2, noise=torch.zeros(2, 16, 2))
    with pytest.raises(ValueError, match="dim"):                                # the 2-D class still refuses dim = 1
        GaussianRF(1, 64)


@pytest.mark.parametrize("N", [4, 64, 200, 4096])
@pytest.mark.parametrize("alpha,tau,sigma", [(2, 3, None), (2, 5, 25)])
def test_sqrt_eig_1d_is_row_zero_of_the_2d_table(N, alpha, tau, sigma):
    """M = 1: k1 = 0 adds an exact zero and the factor M N is N, so the 2-D function is the 1-D one bit for bit"""
    from data_generation.random_fields import sqrt_eig_1d, sqrt_eig_2d
    if sigma is None:
        sigma = tau ** (0.5 * (2 * alpha - 1))
    one, two = sqrt_eig_1d(N, alpha, tau, sigma), sqrt_eig_2d(1, N, alpha, tau, sigma)
    assert tuple(one.shape) == (N,) and tuple(two.shape) == (1, N)
    assert torch.equal(one, two[0])
    assert torch.equal(one, R.sqrt_eig(N, alpha, tau, sigma).float())


def test_schedule_arithmetic():
    from data_generation.etd1d import snapshot_schedule
    from data_generation.ks_1d import ks_schedule
    steps, every, times = snapshot_schedule(2.0, 1e-3, 200)
    assert (steps, every, len(times)) == (2000, 10, 200) and abs(times[-1] - 2.0) < 1e-12 and abs(times[0] - 0.01) < 1e-12
    assert snapshot_schedule(0.4, 5e-3, 4)[:2] == (80, 20)
    with pytest.raises(ValueError, match="whole number"):
        snapshot_schedule(2.0, 3e-3, 200)                                       # 3.33 steps per snapshot
    with pytest.raises(ValueError, match="whole number"):
        snapshot_schedule(1.0, 0.3, 2)
    with pytest.raises(ValueError):
        snapshot_schedule(1.0, 0.1, 0)
    with pytest.raises(ValueError):
        snapshot_schedule(1.0, 2.0, 1)                                          # half a step
    steps, every, times = ks_schedule(5.0, 51, 51, 0.01)
    assert (steps, every, len(times)) == (500, 10, 51) and times[0] == 0.0 and abs(times[-1] - 5.0) < 1e-12
    with pytest.raises(ValueError, match="nte"):
        ks_schedule(5.0, 51, 52, 0.01)                                          # nte > nt
    with pytest.raises(ValueError, match="whole number"):
        ks_schedule(5.0, 52, 51, 0.01)


def test_ks_resolution_needs_a_damped_mode():
    from data_generation.ks_1d import damped_modes
    # nu = 0.05, L = 64: kappa_n^2 > 20 from n = 46; the 2/3 rule keeps n <= 85 of 256 points and n <= 42 of 128
    assert damped_modes(256, 64.0, 0.05) == 85 - 45 and damped_modes(128, 64.0, 0.05) == 0
    assert damped_modes(138, 64.0, 0.05) == 1 and damped_modes(136, 64.0, 0.05) == 0
    assert damped_modes(32, 8.0, 0.05) == 10 - 5                                # the end-to-end test's coarse grid


def test_solver_functions_check_the_schedule_before_the_device():
    from data_generation.burgers_1d import burgers_1d
    from data_generation.ks_1d import ks_1d
    u0 = torch.zeros(1, 16)                                                     # a CPU tensor: never reached
    with pytest.raises(ValueError, match="whole number"):
        burgers_1d(u0, 0.1 / math.pi, 2.0, 1.0, 0.3, 2)
    with pytest.raises(ValueError, match="whole number"):
        ks_1d(u0, 0.05, 4.0, 1.0, 0.3, 2)


def test_path_builders_agree_with_the_loaders(tmp_path):
    from data_generation.burgers_1d import burgers_path
    from data_generation.ks_1d import ks_path
    from dataloaders.burger_naive_true_multires import _burgers_path
    from dataloaders.ks_naive_true_multires import _ks_path
    out = str(tmp_path)
    key = dict(resolution=64, viscosity=0.05, L=8.0, lmax=8, et=0.5, nte=11, nt=11)
    p = ks_path(out, "train", samples=10, **key)
    assert p == os.path.join(out, "res_64", "visc_0.05_L8.0_lmax8_et0.5_nte11_nt11", "KS_train_10.npz")
    assert _ks_path(out, train_s=10, **key) is None                            # nothing there yet
    os.makedirs(os.path.dirname(p))
    open(p, "wb").close()
    assert _ks_path(out, train_s=10, **key) == p
    assert ks_path(out, "valid", samples=10, **key) == os.path.join(os.path.dirname(p), "KS_valid.npz")
    assert ks_path(out, "test", samples=10, flat=True, **key) == os.path.join(out, "KS_test.npz")
    assert ks_path(out, "train", samples=10, flat=True, **key) == os.path.join(out, "KS_train_10.npz")
    b = burgers_path(out, 128, 0.1)
    assert b == os.path.join(out, "burgers_128_0.1", "1D_Burgers_Sols_Nu0.1.npz")
    assert _burgers_path(out, 128, 0.1, "1D_Burgers_Sols_Nu*.hdf5") is None
    os.makedirs(os.path.dirname(b))
    open(b, "wb").close()
    assert _burgers_path(out, 128, 0.1, "1D_Burgers_Sols_Nu*.hdf5") == b


def test_scripts_report_argument_errors_before_the_device(tmp_path, capsys):
    from data_generation import burgers_1d, ks_1d
    out = str(tmp_path)
    bad = [
        (burgers_1d, ["--out", out, "--dt", "3e-3"]),                           # 3.33 steps per snapshot
        (burgers_1d, ["--out", out, "--snapshots", "1"]),
        (burgers_1d, ["--out", out, "--resolutions", "64,63"]),
        (burgers_1d, ["--out", out, "--samples", "0"]),
        (ks_1d, ["--out", out, "--nte", "52"]),                                 # nte > nt
        (ks_1d, ["--out", out, "--nt", "52"]),                                  # 5 / 51 is no whole number of steps
        (ks_1d, ["--out", out, "--resolutions", "64,64"]),
        (ks_1d, ["--out", out, "--flat", "--resolutions", "64,32"]),
        (ks_1d, ["--out", out, "--split", "validation"]),
        (ks_1d, ["--out", out, "--resolutions", "256,128"]),                    # 128 points keep no damped mode at L = 64
    ]
    for mod, argv in bad:
        with pytest.raises(SystemExit) as e:
            mod.main(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    assert os.listdir(out) == []


def test_scripts_refuse_to_run_without_a_gpu(tmp_path, monkeypatch):
    from data_generation import burgers_1d, ks_1d
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for mod, extra in ((burgers_1d, []), (ks_1d, ["--L", "8"])):
        with pytest.raises(RuntimeError, match="GPU"):
            mod.main(["--out", str(tmp_path), "--samples", "2", "--resolution", "32"] + extra)
    assert os.listdir(tmp_path) == []


def test_cpu_tensors_are_refused():
    from data_generation.burgers_1d import burgers_1d
    from rpde import ops
    from rpde._lib import RpdeError
    tabs = ops.etd1d_tables(16, 2.0, -0.1, 0.0, 1e-3)
    with pytest.raises(RpdeError, match="GPU"):
        ops.etd1d_solve(torch.zeros(1, 16), tabs, 1, 1)
    with pytest.raises(RpdeError, match="GPU"):
        ops.grf1d(torch.zeros(1, 16, 2), torch.zeros(16))
    with pytest.raises(RpdeError, match="GPU"):
        burgers_1d(torch.zeros(1, 16), 0.1, 2.0, 0.01, 1e-3, 1)
    with pytest.raises(ValueError, match="sqrt_eig"):
        ops.grf1d(torch.zeros(1, 16, 2), torch.zeros(8))
    with pytest.raises(ValueError, match="record_every"):
        ops.etd1d_solve(torch.zeros(1, 16), tabs, 1, 0)


def test_restatement_is_fourth_order_in_dt():
    """pins the scheme, not the device: the float64 restatement's error against a run at a far smaller step falls like
    dt^4 (measured orders 3.83 and 3.92 on this case, rising towards 4 as dt falls; 3.1 .. 3.7 at four to sixteen times
    the step, where the stiff modes still reduce the order)"""
    N, length, T = 64, 16.0, 0.4
    c2, c4 = R.ks_symbol(R.KS_NU)
    u0 = R.ks_initial(2, N, length, 8, seed=5)
    assert R.rel(R.solve(u0, length, c2, c4, T / 40, 40, 40, nonlinear=False)[:, 0],
                 R.solve(u0, length, c2, c4, T / 40, 40, 40)[:, 0]) > 0.1        # the nonlinear term matters here
    fine = R.solve(u0, length, c2, c4, T / 2560, 2560, 2560)[:, 0]
    errs = [R.rel(R.solve(u0, length, c2, c4, T / n, n, n)[:, 0], fine) for n in (80, 160, 320)]
    orders = [math.log2(errs[i] / errs[i + 1]) for i in range(2)]
    print(f"[etd1d order] errors {['%.2e' % e for e in errs]}, orders {['%.2f' % o for o in orders]}")
    assert all(3.7 <= o <= 4.3 for o in orders), (errs, orders)
    assert errs[-1] < 1e-8
