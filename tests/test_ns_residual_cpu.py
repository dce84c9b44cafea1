"""What the vorticity equation-residual loss decides without a GPU: the tables of rpde.ops.ns2d_residual_tables against
closed forms and against the restatement tests/ns_residual_ref.py, the restatement's hand-written gradient (the adjoint
the device implements) against float64 autograd, the range of validity of the rule as assertions, the workspace sizes
and argument errors of the C entries, and the host side: VorticityResidualLoss and training.loss=residual in 2-D."""
import math
import os

import pytest
import torch

from tests import ns_residual_ref as R
from tests import ns_solver_ref as S
from tests.conftest import DROPIN

FAKE = 1 << 20      # a pointer that is never dereferenced: argument errors come before any device work
GRIDS = [(4, 6), (4, 8), (6, 10), (4, 12), (12, 6), (16, 24), (48, 32), (64, 64)]


# ---- 1. tables -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS, ids=str)
def test_tables_against_closed_forms(grid):
    """E - 1, m0, m1 in float64 from the closed forms of phi1 and phi2 where they do not cancel (|z| > 1e-2), one fp32
    rounding away; 1 / lap; the mask on the edge grids"""
    from rpde import ops
    M, N = grid
    K, kp = N // 2 + 1, (N // 2 + 1 + 3) // 4 * 4
    visc, h = 1e-3, 0.05
    got = ops.ns2d_residual_tables(M, N, visc, h)
    assert len(got) == 4
    for t in got:
        assert t.dtype == torch.float32 and tuple(t.shape) == (M, kp) and t.is_contiguous() and not t.is_cuda
        assert not t[:, K:].any()                                               # padding zero
    em1, m0, m1, il = (t[:, :K].double() for t in got)
    k1 = (torch.fft.fftfreq(M, dtype=torch.float64) * M).round().view(M, 1)
    k2 = torch.arange(K, dtype=torch.float64).view(1, K)
    lap = 4 * math.pi ** 2 * (k1 ** 2 + k2 ** 2)
    z = -h * visc * lap
    keep = ((k1.abs() <= (2.0 / 3.0) * (M // 2)) & (k2 <= (2.0 / 3.0) * (N // 2))).double()
    assert torch.allclose(em1, torch.expm1(z), rtol=2.0 ** -23, atol=0)
    big = z.abs() > 1e-2
    phi1 = torch.where(big, torch.expm1(z) / torch.where(big, z, torch.ones_like(z)), 1.0 + z / 2)
    phi2 = torch.where(big, (torch.expm1(z) - z) / torch.where(big, z, torch.ones_like(z)) ** 2, 0.5 + z / 6)
    # closed forms: exact for |z| > 1e-2 up to their own cancellation (1e-12), two Taylor terms below (z^2 / 6 < 2e-5)
    tol = torch.where(big, torch.full_like(z, 1e-6), torch.full_like(z, 3e-5))
    assert bool(((m0 - h * (phi1 - phi2) * keep).abs() <= tol * h).all())
    assert bool(((m1 - h * phi2 * keep).abs() <= tol * h).all())
    assert float(em1[0, 0]) == 0.0 and float(m0[0, 0]) == pytest.approx(h / 2, rel=1e-6) and float(m1[0, 0]) == pytest.approx(h / 2, rel=1e-6)
    lap1 = lap.clone()
    lap1[0, 0] = 1.0
    assert torch.allclose(il, 1.0 / lap1, rtol=2.0 ** -23, atol=0) and float(il[0, 0]) == 1.0
    # the 2/3 mask: the Nyquist row and column are out, mode (1, 1) is in
    assert not m0[M // 2].any() and not m1[:, N // 2].any() and float(m1[1, 1]) > 0
    cut1, cut2 = int((2.0 / 3.0) * (M // 2)), int((2.0 / 3.0) * (N // 2))
    assert not m1[cut1 + 1:M - cut1].any() and not m1[:, cut2 + 1:].any() and bool((m1[:cut1 + 1, :cut2 + 1] > 0).all())
    full = ops.ns2d_residual_tables(M, N, visc, h, dealias=False)
    assert bool((full[2][:, :K] > 0).all()) and torch.equal(full[0], got[0]) and torch.equal(full[3], got[3])


def test_em1_does_not_cancel_at_small_z():
    """z -> 0: E - 1 = z to first order, where exp(z) - 1 in fp32 would have lost every digit; phi1 -> 1, phi2 -> 1/2"""
    from rpde import ops
    M, N, visc, h = 8, 8, 1e-9, 1e-3
    em1, m0, m1, _ = ops.ns2d_residual_tables(M, N, visc, h, dealias=False)
    T = R.tables(M, N, visc, h, dealias=False)
    z = -h * visc * 4 * math.pi ** 2 * (T["k1"] ** 2 + T["k2"] ** 2)
    assert float(z.abs().max()) < 1e-8
    assert torch.allclose(em1[:, :5].double(), z, rtol=1e-6, atol=0) and float(em1[1, 1]) < 0
    assert torch.allclose(m0[:, :5].double(), torch.full_like(z, h / 2), rtol=1e-6) and torch.allclose(m1[:, :5].double(), torch.full_like(z, h / 2), rtol=1e-6)


@pytest.mark.parametrize("grid", GRIDS, ids=str)
def test_tables_and_forcing_equal_the_restatement_rounded_once(grid):
    from rpde import ops
    M, N = grid
    K = N // 2 + 1
    got = ops.ns2d_residual_tables(M, N, S.VISC, R.INTERVAL)
    T = R.tables(M, N, S.VISC, R.INTERVAL)
    for name, t, w in zip(("em1", "m0", "m1", "inv_lap"), got, (T["em1"], T["m0"], T["m1"], 1.0 / T["poisson"])):
        assert torch.allclose(t[:, :K].double(), w, rtol=2.0 ** -23, atol=1e-300), name
    f = S.forcing(M, N)
    fs = ops.ns2d_residual_forcing(f, S.VISC, R.INTERVAL)
    want = R.forcing_term(f, T)
    assert fs.dtype == torch.float32 and tuple(fs.shape) == (M, 2, got[0].shape[1]) and fs.is_contiguous() and not fs[:, :, K:].any()
    assert torch.allclose(fs[:, 0, :K].double(), want.real, rtol=2.0 ** -23, atol=1e-30)
    assert torch.allclose(fs[:, 1, :K].double(), want.imag, rtol=2.0 ** -23, atol=1e-30)
    assert fs[1, :, 1].any()                                                    # the forcing lives on mode (1, 1)


def test_tables_check_their_arguments():
    from rpde import ops
    for bad in ((7, 8, 1e-3, 0.1), (8, 2, 1e-3, 0.1), (8, 8, -1.0, 0.1), (8, 8, 1e-3, 0.0), (8, 8, float("nan"), 0.1)):
        with pytest.raises(ValueError, match="ns2d_residual_tables"):
            ops.ns2d_residual_tables(*bad)
    with pytest.raises(ValueError, match="ns2d_residual_forcing"):
        ops.ns2d_residual_forcing(torch.zeros(2, 8, 8), 1e-3, 0.1)
    with pytest.raises(ValueError, match="ns2d_residual_forcing"):
        ops.ns2d_residual_forcing(torch.zeros(8, 7), 1e-3, 0.1)


def test_the_shared_helpers_left_the_older_tables_alone():
    """ns2d_tables and the 1-D contour now go through _ns2d_symbols and _contour: the same numbers as the restatements"""
    from rpde import ops
    from tests import etd_residual_ref as E1
    c_w, c_f, c_g, il = ops.ns2d_tables(16, 24, 1e-3, 2e-3)
    T = R.tables(16, 24, 1e-3, 2e-3)
    a = 0.5 * 2e-3 * 1e-3 * 4 * math.pi ** 2 * (T["k1"] ** 2 + T["k2"] ** 2)
    assert torch.equal(c_w[:, :13], ((1 - a) / (1 + a)).float()) and torch.equal(c_f[:, :13], (2e-3 * T["dealias"] / (1 + a)).float())
    assert torch.equal(il[:, :13], (1.0 / T["poisson"]).float())
    got = ops.etd1d_residual_tables(48, 12.0, -0.3, -0.02, 1.0, 0.0, 0.07)
    want = E1.tables(48, 12.0, -0.3, -0.02, 1.0, 0.0, 0.07)
    for t, w in zip(got, want):
        assert torch.allclose(t[0, :25].double(), w.real, rtol=2.0 ** -23, atol=1e-300)


# ---- 2. the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(2, 4, 6), (2, 12, 6), (3, 8, 8), (2, 16, 24)], ids=R.case_id)
def test_gradient_formula_against_autograd(case):
    """the adjoint the device implements against float64 autograd of the restatement, with the forcing, an affine decode
    and per-sample weights; and against central differences on the smallest grid"""
    B, M, N = case
    ref = R.parity_reference(case, "noisy", True)
    p, x, T, ft = ref["p"].double(), ref["x"].double(), ref["T64"], ref["fterm64"]
    affine = (1.3, -0.2, 0.7, 0.4)
    w = torch.tensor([0.6, -1.7, 0.9][:B], dtype=torch.float64)
    _, auto = R.rel_and_grad(p, x, T, ft, affine, w)
    form = R.grad_formula(p, x, T, ft, affine, w)
    assert float((form - auto).norm() / auto.norm()) < 1e-13
    exact = R.parity_reference(case, "exact", False)
    pe, xe = exact["p"].double(), exact["x"].double()
    assert float((R.grad_formula(pe, xe, T) - exact["grad64"]).norm() / exact["grad64"].norm()) < 1e-12
    if case == (2, 4, 6):
        eps, fd = 1e-6, torch.zeros_like(p)
        for i in range(p.numel()):
            d = torch.zeros(p.numel(), dtype=torch.float64)
            d[i] = eps
            d = d.view_as(p)
            fd.view(-1)[i] = ((R.rel(p + d, x, T, ft, affine) - R.rel(p - d, x, T, ft, affine)) * w).sum() / (2 * eps)
        assert float((form - fd).norm() / fd.norm()) < 1e-7


@pytest.mark.parametrize("case", [(2, 16, 24), (2, 32, 48), (2, 64, 64)], ids=R.case_id)
def test_exact_pair_is_far_below_persistence(case):
    """float64, ns_solver_ref at its own constants, consecutive snapshots 0.05 apart: rel(true pair) < 0.1 rel(p = x) per
    sample (measured shares 0.005 .. 0.04), with the forcing and without"""
    for forced in (True, False):
        ref = R.parity_reference(case, "exact", forced)
        print(case, forced, "true", ref["rel64"].tolist(), "persistence", ref["still64"].tolist())
        assert bool((ref["rel64"] < 0.1 * ref["still64"]).all())
        # the advective term matters in these pairs: without it (m0 = m1 = 0) the residual is ten times the true one
        T = dict(ref["T64"], m0=torch.zeros_like(ref["T64"]["m0"]), m1=torch.zeros_like(ref["T64"]["m1"]))
        lin = R.rel(ref["p"].double(), ref["x"].double(), T, ref["fterm64"])
        assert bool((lin > 10 * ref["rel64"]).all())


def test_the_rule_loses_its_range_by_interval_0_1():
    """16 x 24, the same trajectory: x = w(0.05), p = w(0.15), interval 0.1: the exact pair's share of p = x is several
    times that at 0.05 (third order: about 8 in the residual against 2 in p = x)"""
    case = (2, 16, 24)
    sol = R.trajectory(case, True)
    f = S.forcing(16, 24)
    T1, T2 = R.tables(16, 24, S.VISC, 0.05), R.tables(16, 24, S.VISC, 0.1)
    x = sol[..., 0]
    share1 = R.rel(sol[..., 1], x, T1, R.forcing_term(f, T1)) / R.rel(x, x, T1, R.forcing_term(f, T1))
    share2 = R.rel(sol[..., 2], x, T2, R.forcing_term(f, T2)) / R.rel(x, x, T2, R.forcing_term(f, T2))
    print("share at 0.05", share1.tolist(), "at 0.1", share2.tolist())
    assert bool((share2 > 2.5 * share1).all()) and bool((share2 < 0.5).all())


def test_forcing_pair_is_carried_by_the_forcing():
    """the pair of the GPU forcing-sign test: the forcing term is at least half of what the unforced tables leave, the
    forced tables bring the residual below a tenth of it, and the wrong sign doubles it"""
    x, p, f = R.forcing_pair()
    B, M, N = R.FORCING_CASE
    T = R.tables(M, N, S.VISC, R.INTERVAL)
    ft = R.forcing_term(f, T)
    r0, _, _ = R.spectrum(p, x, T, None)
    share = R._energy(ft.expand_as(r0), M, N).sqrt() / R._energy(r0, M, N).sqrt()
    unforced, forced, wrong = R.rel(p, x, T, None), R.rel(p, x, T, ft), R.rel(p, x, T, -ft)
    print("share", share.tolist(), "unforced", unforced.tolist(), "forced", forced.tolist(), "wrong sign", wrong.tolist())
    assert bool((share >= 0.5).all()) and bool((forced < 0.1 * unforced).all()) and bool((wrong > 1.5 * unforced).all())


# ---- 3. ABI ----------------------------------------------------------------------------------------------------------
def _hs_elems(B, M, N):
    return B * M * 2 * ((N // 2 + 1 + 3) // 4 * 4)


def test_workspace_and_spectrum_sizes_at_the_refusal_boundaries():
    from rpde import _lib as L
    lib = L.load()
    ws, se = lib.rpde_ns2d_residual_ws_bytes, lib.rpde_ns2d_residual_spec_elems
    assert se(2, 16, 24) == 2 * _hs_elems(2, 16, 24) and ws(2, 16, 24) > 0 and ws(2, 16, 24) % 256 == 0
    # at least the eight derivative spectra, their row stage and the eight fields
    assert ws(2, 16, 24) >= 4 * (16 * _hs_elems(2, 16, 24) + 8 * 2 * 16 * 24)
    # axes: even, 4 .. 4096
    for M, N in ((4, 4), (4096, 4), (4, 4096)):
        assert ws(1, M, N) > 0 and se(1, M, N) == 2 * _hs_elems(1, M, N), (M, N)
    for M, N in ((2, 8), (8, 2), (5, 8), (8, 5), (4098, 8), (8, 4098), (1, 8), (0, 8), (8, 0), (-4, 8)):
        assert ws(1, M, N) == 0 and se(1, M, N) == 0, (M, N)
    # the batch: 8 B images within gridDim.y, 32 B max(M, N) within the transforms' int rows
    assert ws(8191, 4, 4) > 0 and ws(8192, 4, 4) == 0 and se(8192, 4, 4) == 0
    for B in (0, -1):
        assert ws(B, 8, 8) == 0 and se(B, 8, 8) == 0
    # 32 B max(M, N) < 2^31 holds for every B <= 8191 at the longest axis: the image count is the limit that binds
    assert 32 * 8191 * 4096 < (1 << 31)
    assert se(8191, 4, 4096) == 2 * _hs_elems(8191, 4, 4096) and se(8192, 4, 4096) == 0
    assert se(8191, 4096, 4) > 0 and se(8192, 4096, 4) == 0 and ws(8192, 4096, 4) == 0 and ws(8191, 4096, 4) > 0
    # the size grows with every dimension
    assert ws(3, 16, 24) > ws(2, 16, 24) and ws(2, 18, 24) > ws(2, 16, 24) and ws(2, 16, 26) > ws(2, 16, 24)


@pytest.mark.parametrize("entry,dims", [("fwd", (2, 16, 24)), ("fwd", (3, 4, 6)), ("bwd", (2, 16, 24)), ("spectrum", (2, 16, 24))])
def test_query_and_entries_share_their_layouts(entry, dims):
    """DESIGN.md 10.11 for the three entries: each reports a short workspace before any device work, with its own
    measurement; the query is the largest of them, the forward's"""
    import re
    from rpde import _lib as L
    lib = L.load()
    need = lib.rpde_ns2d_residual_ws_bytes(*dims)
    assert need > 0 and need % 256 == 0

    def call(n):
        if entry == "fwd":
            return lib.rpde_ns2d_residual_fwd(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, None, FAKE, FAKE, FAKE, FAKE, *dims, 1, FAKE, n, None)
        if entry == "bwd":
            return lib.rpde_ns2d_residual_bwd(FAKE, FAKE, FAKE, None, FAKE, FAKE, None, FAKE, *dims, 1, FAKE, n, None)
        return lib.rpde_ns2d_residual_spectrum(FAKE, None, FAKE, FAKE, *dims, FAKE, n, None)

    def refused(given):
        assert call(given) == L.ERR_WORKSPACE, lib.rpde_last_error()
        m = re.fullmatch(rf"ns2d_residual_{entry}: workspace too small \((\d+) bytes, needs (\d+)\)", lib.rpde_last_error().decode())
        assert m, lib.rpde_last_error()
        return int(m.group(1)), int(m.group(2))

    given, own = refused(0)
    assert given == 0 and 0 < own <= need and own % 256 == 0 and (own == need) == (entry == "fwd")
    assert refused(own - 256) == (own - 256, own)


def test_argument_errors_are_reported_without_a_gpu():
    from rpde import _lib as L
    lib = L.load()
    nws = lib.rpde_ns2d_residual_ws_bytes(2, 16, 24)

    def fwd(B=2, M=16, N=24, p=FAKE, x=FAKE, em1=FAKE, m0=FAKE, m1=FAKE, il=FAKE, fs=None, stats=FAKE, spec=FAKE, ws=FAKE, n=nws):
        return lib.rpde_ns2d_residual_fwd(p, x, em1, m0, m1, il, fs, None, FAKE, FAKE, stats, spec, B, M, N, 1, ws, n, None)

    def bwd(B=2, M=16, N=24, spec=FAKE, m1=FAKE, il=FAKE, stats=FAKE, gl=FAKE, gr=None, gp=FAKE, ws=FAKE, n=nws):
        return lib.rpde_ns2d_residual_bwd(spec, m1, il, None, stats, gl, gr, gp, B, M, N, 1, ws, n, None)

    def spc(B=2, M=16, N=24, x=FAKE, s64=FAKE, s32=FAKE, ws=FAKE, n=nws):
        return lib.rpde_ns2d_residual_spectrum(x, None, s64, s32, B, M, N, ws, n, None)

    bad_dims = ((2, 15, 24), (2, 16, 23), (2, 2, 24), (2, 16, 4098), (0, 16, 24), (-1, 16, 24), (8192, 16, 24), (2, 1, 24))
    for call, name, nulls in ((fwd, b"ns2d_residual_fwd", ("p", "x", "em1", "m0", "m1", "il", "stats", "spec", "ws")),
                              (bwd, b"ns2d_residual_bwd", ("spec", "m1", "il", "stats", "gp", "ws")),
                              (spc, b"ns2d_residual_spectrum", ("x", "s64", "s32", "ws"))):
        for k in nulls:
            assert call(**{k: None}) == L.ERR_ARG, (name, k)
            assert name in lib.rpde_last_error() and b"null" in lib.rpde_last_error(), (name, k)
        for B, M, N in bad_dims:
            assert call(B=B, M=M, N=N) == L.ERR_ARG, (name, B, M, N)
            msg = lib.rpde_last_error()
            assert name in msg and b"bad B=" in msg and b"8 B <= 65535" in msg, msg      # the limit is in the message
        assert call(n=nws // 64) == L.ERR_WORKSPACE and b"workspace too small" in lib.rpde_last_error()
        assert call(n=0) == L.ERR_WORKSPACE
        assert call(ws=FAKE + 64) == L.ERR_ARG and b"aligned" in lib.rpde_last_error()
    for k in ("p", "x", "em1", "m0", "m1", "il", "fs", "spec"):
        assert fwd(**{k: FAKE + 4}) == L.ERR_ARG and b"aligned" in lib.rpde_last_error(), k
    for k in ("spec", "m1", "il", "gp"):
        assert bwd(**{k: FAKE + 8}) == L.ERR_ARG and b"aligned" in lib.rpde_last_error(), k
    assert bwd(gl=None, gr=None) == L.ERR_ARG and b"null" in lib.rpde_last_error()     # one of the two gradients is needed


def test_op_refuses_shapes_and_cpu_tensors():
    from rpde import ops
    from rpde._lib import RpdeError
    M, N = 8, 12
    tabs = ops.ns2d_residual_tables(M, N, 1e-3, 0.05)
    fs = ops.ns2d_residual_forcing(S.forcing(M, N), 1e-3, 0.05)
    z = torch.zeros(2, M, N)
    bad = [(torch.zeros(2, 2, M, N),) * 2,                                      # two channels
           (torch.zeros(2, 1, M, N), z), (torch.zeros(M, N),) * 2, (torch.zeros(2, 1, 1, M, N),) * 2,
           (z, torch.zeros(2, M, N + 2)), (z.double(), z.double())]
    for p, x in bad:
        with pytest.raises(ValueError, match="ns2d_residual"):
            ops.ns2d_residual(p, x, tabs)
    other = ops.ns2d_residual_tables(M, 16, 1e-3, 0.05)
    for t in (other, tabs[:3], tuple(t[0] for t in tabs)):
        with pytest.raises(ValueError, match="ns2d_residual_tables"):
            ops.ns2d_residual(z, z, t)
    with pytest.raises(ValueError, match="forcing_spec"):
        ops.ns2d_residual(z, z, tabs, fs[:, 0])
    with pytest.raises(ValueError, match="affine"):
        ops.ns2d_residual(z, z, tabs, None, (1.0, 0.0))
    for p, x in ((z, z), (z[:, None], z[:, None])):                             # well formed: refused as CPU tensors only
        with pytest.raises(RpdeError, match="GPU"):
            ops.ns2d_residual(p, x, tabs, fs)
    with pytest.raises(RpdeError, match="GPU"):
        ops.ns2d_residual_spectrum(z)


# ---- 4. host side ----------------------------------------------------------------------------------------------------
def test_loss_class():
    from utils.loss import EquationResidualLoss, SumLoss, VorticityResidualLoss, reference_forcing
    v = VorticityResidualLoss(1e-3, 0.05, forcing="reference")
    assert v.takes_input is True and v.dims == 2 and (v.viscosity, v.interval, v.forcing, v.dealias) == (1e-3, 0.05, "reference", True)
    assert VorticityResidualLoss(0.0, 0.1).forcing is None
    assert torch.equal(reference_forcing(8, 12), S.forcing(8, 12))
    for bad in (dict(viscosity=-1.0, interval=0.1), dict(viscosity=1e-3, interval=0.0), dict(viscosity=float("inf"), interval=0.1),
                dict(viscosity=1e-3, interval=0.1, forcing="sine"), dict(viscosity=1e-3, interval=0.1, forcing=torch.zeros(2, 8, 8))):
        with pytest.raises(ValueError, match="VorticityResidualLoss"):
            VorticityResidualLoss(**bad)
    v.set_affine(pred=(2.0, 1.0), inp=(3.0, -1.0))
    assert v._affine == (2.0, 1.0, 3.0, -1.0)
    v.set_affine()
    assert v._affine is None
    with pytest.raises(ValueError, match="set_affine"):
        v.set_affine(pred=(float("nan"), 0.0))
    with pytest.raises(ValueError, match="two-dimensional"):
        v.warm((8,), "cpu")
    with pytest.raises(ValueError, match="input"):
        v(torch.zeros(1, 8, 8), None, None)
    for shape in ((2, 2, 8, 8), (8, 8), (2, 1, 1, 8, 8)):
        with pytest.raises(ValueError, match="one channel"):
            v(torch.zeros(shape), None, torch.zeros(shape))
    # tables per (grid, device): two grids, two entries, built once each; the forcing follows the grid
    (t1, f1), (t2, f2) = v._table((8, 12), "cpu"), v._table((16, 8), "cpu")
    assert tuple(t1[0].shape) == (8, 8) and tuple(t2[0].shape) == (16, 8) and tuple(f1.shape) == (8, 2, 8) and tuple(f2.shape) == (16, 2, 8)
    assert v._table((8, 12), "cpu")[0][0] is t1[0] and len(v._tables) == 2
    assert VorticityResidualLoss(1e-3, 0.05)._table((8, 12), "cpu")[1] is None
    # an explicit forcing serves one grid
    e = VorticityResidualLoss(1e-3, 0.05, forcing=S.forcing(8, 12))
    assert torch.equal(e._table((8, 12), "cpu")[1], f1)
    with pytest.raises(ValueError, match="grid"):
        e._table((16, 8), "cpu")
    assert SumLoss([(1.0, torch.nn.MSELoss()), (0.1, v)]).takes_input is True
    # the 1-D class is as it was
    with pytest.raises(ValueError, match="one-dimensional"):
        EquationResidualLoss.ks(0.05, 64.0, 0.1).warm((8, 8), "cpu")


def test_training_loss_parses_the_vorticity_residual():
    from rpde.entry import residual_affine, training_loss
    from utils.loss import RelativeL2Loss, SumLoss, VorticityResidualLoss
    eq = {"kind": "ns_vorticity", "viscosity": 1e-3, "interval": 0.05, "forcing": "reference"}
    name, fn = training_loss({"loss": "residual"}, 2, {"equation": eq})
    assert name == "residual" and isinstance(fn, SumLoss) and fn.takes_input and fn.weights == [1.0, 0.1]
    assert isinstance(fn.terms[0], RelativeL2Loss) and isinstance(fn.terms[1], VorticityResidualLoss)
    r = fn.terms[1]
    assert (r.viscosity, r.interval, r.forcing) == (1e-3, 0.05, "reference")
    for none in ({k: v for k, v in eq.items() if k != "forcing"}, dict(eq, forcing=None), dict(eq, forcing="none")):
        _, fn2 = training_loss({"loss": "residual", "loss_lambda": 0.5}, 2, {"equation": none})
        assert fn2.weights == [1.0, 0.5] and fn2.terms[1].forcing is None
    one_d = {"c2": 1.0, "c4": -0.05, "length": 64.0, "interval": 0.1}
    for training, dims, dataset, word in (({"loss": "residual"}, 2, {"equation": one_d}, "one-dimensional"),
                                          ({"loss": "residual"}, 2, {}, "one-dimensional"),
                                          ({"loss": "residual"}, 2, None, "one-dimensional"),
                                          ({"loss": "residual"}, 2, {"equation": {"kind": "euler", "viscosity": 0.0, "interval": 0.1}}, "one-dimensional"),
                                          ({"loss": "residual"}, 2, {"equation": {"kind": "ns_vorticity", "interval": 0.1}}, "viscosity"),
                                          ({"loss": "residual"}, 2, {"equation": dict(eq, nu=1.0)}, "nu"),
                                          ({"loss": "residual"}, 2, {"equation": dict(eq, interval=-1.0)}, "positive"),
                                          ({"loss": "residual"}, 2, {"equation": dict(eq, forcing="sine")}, "forcing"),
                                          ({"loss": "residual"}, 1, {"equation": eq}, "kind")):
        with pytest.raises(SystemExit, match=word):
            training_loss(training, dims, dataset)

    class Simple:
        mean, std, eps = 0.5, 2.0, 1e-5

    class Pointwise:
        mean, std, eps = torch.zeros(4), torch.ones(4), 1e-5

    residual_affine(fn, Simple(), Simple(), use_normalizer=False)
    assert r._affine == (2.0 + 1e-5, 0.5, 2.0 + 1e-5, 0.5)
    residual_affine(fn, Simple(), Simple(), use_normalizer=True)                # train() decodes the prediction itself
    assert r._affine == (1.0, 0.0, 2.0 + 1e-5, 0.5)
    residual_affine(fn, None, None, use_normalizer=True)
    assert r._affine is None
    with pytest.raises(SystemExit, match="point-wise"):
        residual_affine(fn, Pointwise(), Pointwise(), use_normalizer=False)
    with pytest.raises(SystemExit, match="min-max"):
        residual_affine(fn, None, None, use_normalizer=False, minmax=True)


def test_generated_yaml_matches_the_generator_defaults(monkeypatch, tmp_path):
    from data_generation import ns_2d
    from rpde.config import compose
    from rpde.entry import training_loss
    from tests.test_etd_residual_cpu import _defaults
    conf = os.path.join(DROPIN, "conf")
    cfg = compose(conf, "config", ["dataset=ns/ns_generated", "training.loss=residual"])
    a = _defaults(ns_2d, monkeypatch, tmp_path / "x.npz")
    eq = dict(cfg.dataset.equation)
    assert eq == {"kind": "ns_vorticity", "viscosity": a.viscosity, "interval": eq["interval"], "forcing": "reference"}
    assert eq["interval"] == pytest.approx(a.T / a.record_steps, rel=1e-15)
    assert int(cfg.dataset.dims) == 2 and int(cfg.dataset.dataset_params.reduced_resolution_t) == 1
    assert str(cfg.dataset.dataset_params.normalization_type) == "simple"
    r = training_loss(cfg.training, 2, cfg.dataset)[1].terms[1]
    assert (r.viscosity, r.interval, r.forcing) == (a.viscosity, eq["interval"], "reference")
    # a 2-D data set without the block keeps its refusal
    plain = compose(conf, "config", ["dataset=ns/ns_file", "training.loss=residual"])
    with pytest.raises(SystemExit, match="one-dimensional"):
        training_loss(plain.training, 2, plain.dataset)
