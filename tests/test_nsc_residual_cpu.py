"""The active-scalar equation-residual loss without a device: the float64 restatement (tests/nsc_residual_ref.py)
against itself and against the generator's restatement, the host-side tables, the loss class, the config table and the
C ABI's refusals (argument errors and the workspace verdict come before any device work)."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import ns_solver_ref as S
from tests import nsc_residual_ref as R

DROPIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "resolution-pde_amd")
FAKE = 1 << 20


# ---- 1. the closed-form gradient is the adjoint ------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [R.IDENTITY, (1.75, 0.3, 1.3, -0.1)], ids=["identity", "affine"])
@pytest.mark.parametrize("forced", [True, False], ids=["forced", "free"])
@pytest.mark.parametrize("case", [(2, 4, 6), (2, 16, 24), (1, 48, 32)], ids=R.case_id)
def test_grad_formula_is_autograd(case, forced, affine):
    """the closed form the device implements against float64 autograd of the restatement: <= 1e-12 relative (measured
    2e-16 .. 6e-16), under per-sample weights and a scalar weight that is not 1"""
    B = case[0]
    ref = R.parity_reference(case, "noisy", forced)
    p, x = ref["p"].double(), ref["x"].double()
    if affine != R.IDENTITY:
        p, x = (p - affine[1]) / affine[0], (x - affine[3]) / affine[2]
    w = torch.tensor([0.3, 1.1][:B], dtype=torch.float64)
    for lam in (1.0, 0.5):
        _, g = R.rel_and_grad(p, x, ref["T64"], R.BETA, ref["fterm64"], affine, lam, w)
        gf = R.grad_formula(p, x, ref["T64"], R.BETA, ref["fterm64"], affine, lam, w)
        err = float((gf - g).norm() / g.norm())
        print(case, forced, affine, lam, f"{err:.2e}")
        assert err <= 1e-12


# ---- 2. range of validity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(2, 16, 24), (2, 32, 48), (2, 64, 64), (1, 48, 32)], ids=R.case_id)
def test_true_pairs_against_the_trivial_predictor_and_the_buoyancy(case):
    """consecutive snapshots of the generator's restatement: rel < 0.1 rel(p = x) per sample (measured <= 0.058), and
    without the buoyancy term the true pair is at least 5 times worse (measured >= 7.6)"""
    ref = R.parity_reference(case, "exact", True)
    p, x = ref["p"].double(), ref["x"].double()
    true, still = ref["rel64"], ref["still64"]
    flat = R.rel(p, x, ref["T64"], 0.0, ref["fterm64"])
    print(case, "true", true.tolist(), "still", still.tolist(), "beta = 0", flat.tolist())
    assert bool((true < 0.1 * still).all())
    assert bool((flat >= 5.0 * true).all())
    # each part against its own still value (measured <= 0.063)
    (tu, tc), (su, sc) = R.rel_parts(p, x, ref["T64"], R.BETA, ref["fterm64"]), R.rel_parts(x, x, ref["T64"], R.BETA, ref["fterm64"])
    assert bool((tu < 0.1 * su).all()) and bool((tc < 0.1 * sc).all())


def test_forcing_pair():
    """a pair that the forcing carries: forced < 1e-3 unforced < wrong sign (measured 4.3e-6 / 0.0224 / 0.0449)"""
    x, p, f = R.forcing_pair()
    B, M, N = R.FORCING_CASE
    T = R.tables(M, N, R.VISC, R.KAPPA, R.INTERVAL)
    ft = R.forcing_term(f, T)
    forced, free, wrong = (R.rel(p, x, T, R.BETA, t) for t in (ft, None, -ft))
    print("forced", forced.tolist(), "unforced", free.tolist(), "wrong sign", wrong.tolist())
    assert bool((forced < 1e-3 * free).all()) and bool((free < wrong).all())


# ---- 3. what a predicted velocity owes beyond its curl -----------------------------------------------------------------
@pytest.mark.parametrize("case", [(2, 16, 24), (2, 64, 64), (2, 4, 6)], ids=R.case_id)
def test_divergence_and_mean_shift_are_charged(case):
    """a pure gradient field of 1 % of the rms velocity, and 1 % of the rms added to the mean of q: neither has a curl,
    so the evolved equation cannot see them; delta and mu do.  Each raises the loss (the mean over the samples) by at
    least x 1.3: measured x 1.84 / 1.49 (16 x 24), 2.44 / 1.87 (64 x 64), 1.95 / 1.59 (4 x 6); per sample x 1.28 .. 4.5
    for the gradient field and 1.15 .. 3.2 for the mean, the smaller the larger the pair's own residual"""
    B, M, N = case
    ref = R.parity_reference(case, "exact", True)
    p, x = ref["p"].double(), ref["x"].double()
    rms = p[:, 1:].pow(2).mean().sqrt()
    div, shift = p.clone(), p.clone()
    div[:, 1:] += 0.01 * rms * R.gradient_field(M, N)
    shift[:, 1] += 0.01 * rms
    base = ref["rel64"]
    r_div, r_shift = (R.rel(t, x, ref["T64"], R.BETA, ref["fterm64"]) for t in (div, shift))
    print(case, "divergent x", (r_div / base).tolist(), float(r_div.mean() / base.mean()), "mean shift x", (r_shift / base).tolist(),
          float(r_shift.mean() / base.mean()))
    assert float(r_div.mean()) >= 1.3 * float(base.mean()) and float(r_shift.mean()) >= 1.3 * float(base.mean())
    assert bool((r_div > base).all()) and bool((r_shift > base).all())
    # and the curl is blind to both: the evolved parts alone do not move
    s0, s1, s2 = (R.spectrum(t, x, ref["T64"], R.BETA, ref["fterm64"]) for t in (p, div, shift))
    for s in (s1, s2):
        assert float((s["rw"] - s0["rw"]).abs().max()) <= 1e-9 * float(s0["rw"].abs().max())
        assert float((s["rc"] - s0["rc"]).abs().max()) <= 1e-9 * float(s0["rc"].abs().max())


# ---- 4. host tables ----------------------------------------------------------------------------------------------------
def test_tables_are_the_vorticity_tables_per_diffusivity():
    from rpde import ops
    for M, N in ((8, 12), (16, 8)):
        t = ops.nsc2d_residual_tables(M, N, 1e-3, 2e-3, 0.05)
        nu, ka = ops.ns2d_residual_tables(M, N, 1e-3, 0.05), ops.ns2d_residual_tables(M, N, 2e-3, 0.05)
        assert len(t) == 7 and all(torch.equal(a, b) for a, b in zip(t, nu + ka[:3]))
        assert all(tuple(a.shape) == (M, (N // 2 + 4) // 4 * 4) and a.dtype == torch.float32 for a in t)
        assert not torch.equal(t[0], t[4])
        # and those of the restatement, rounded once
        Tn, Tk = R.tables(M, N, 1e-3, 2e-3, 0.05)
        K = N // 2 + 1
        for got, want in zip(t, (Tn["em1"], Tn["m0"], Tn["m1"], 1 / Tn["poisson"], Tk["em1"], Tk["m0"], Tk["m1"])):
            assert torch.allclose(got[:, :K].double(), want, rtol=2.0 ** -23, atol=1e-30) and not got[:, K:].any()
    with pytest.raises(ValueError, match="ns2d_residual_tables"):
        ops.nsc2d_residual_tables(8, 12, 1e-3, -1.0, 0.05)


# ---- 5. the loss class -------------------------------------------------------------------------------------------------
def test_loss_class():
    from rpde._lib import RpdeError
    from utils.loss import ActiveScalarResidualLoss, SumLoss
    v = ActiveScalarResidualLoss(1e-3, 2e-3, 5.0, 0.05, forcing="reference")
    assert v.takes_input is True and v.dims == 2 and v.channels == 3
    assert (v.viscosity, v.diffusivity, v.buoyancy, v.interval, v.forcing, v.scalar_weight) == (1e-3, 2e-3, 5.0, 0.05, "reference", 1.0)
    assert ActiveScalarResidualLoss(0.0, 0.0, -1.0, 0.1, scalar_weight=0.0).forcing is None
    for bad in (dict(viscosity=-1.0), dict(diffusivity=-1.0), dict(interval=0.0), dict(buoyancy=float("nan")), dict(scalar_weight=-1.0),
                dict(forcing="sine"), dict(forcing=torch.zeros(2, 8, 8))):
        with pytest.raises(ValueError, match="ActiveScalarResidualLoss"):
            ActiveScalarResidualLoss(**dict(dict(viscosity=1e-3, diffusivity=1e-3, buoyancy=1.0, interval=0.1), **bad))
    v.set_affine(pred=(2.0, 1.0), inp=(3.0, -1.0))
    assert v._affine == (2.0, 1.0, 3.0, -1.0)
    v.set_affine()
    with pytest.raises(ValueError, match="two-dimensional"):
        v.warm((8,), "cpu")
    z = torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError, match="input"):                               # missing input
        v(z, None, None)
    for shape in ((2, 8, 8), (3, 8, 8), (2, 1, 3, 8, 8), (2, 2, 8, 8), (2, 1, 8, 8)):      # wrong rank, two channels, one
        with pytest.raises(ValueError, match=r"\(c, q, v\)"):
            v(torch.zeros(shape), None, torch.zeros(shape))
    with pytest.raises(ValueError, match=r"\(c, q, v\)"):
        v(z, None, torch.zeros(2, 2, 8, 8))
    # well formed: refused as CPU tensors only, there is no fallback
    with pytest.raises(RpdeError, match="GPU"):
        v(z, None, z)
    (t1, f1), (t2, f2) = v._table((8, 12), "cpu"), v._table((16, 8), "cpu")
    assert len(t1) == 7 and tuple(t1[0].shape) == (8, 8) and tuple(f1.shape) == (8, 2, 8) and tuple(f2.shape) == (16, 2, 8)
    assert v._table((8, 12), "cpu")[0][0] is t1[0] and len(v._tables) == 3       # with the 8 x 8 tables of the CPU call above
    assert ActiveScalarResidualLoss(1e-3, 2e-3, 5.0, 0.05)._table((8, 12), "cpu")[1] is None
    e = ActiveScalarResidualLoss(1e-3, 2e-3, 5.0, 0.05, forcing=S.forcing(8, 12))
    assert torch.equal(e._table((8, 12), "cpu")[1], f1)
    with pytest.raises(ValueError, match="grid"):
        e._table((16, 8), "cpu")
    assert SumLoss([(1.0, torch.nn.MSELoss()), (0.1, v)]).takes_input is True


def test_op_refuses_shapes_and_cpu_tensors():
    from rpde import ops
    from rpde._lib import RpdeError
    M, N = 8, 12
    tabs = ops.nsc2d_residual_tables(M, N, 1e-3, 2e-3, 0.05)
    z = torch.zeros(2, 3, M, N)
    for p, x in ((torch.zeros(2, 2, M, N),) * 2, (torch.zeros(2, M, N),) * 2, (z, torch.zeros(2, 3, M, N + 2)), (z.double(),) * 2):
        with pytest.raises(ValueError, match="nsc2d_residual"):
            ops.nsc2d_residual(p, x, tabs, 5.0)
    for t in (ops.nsc2d_residual_tables(M, 16, 1e-3, 2e-3, 0.05), tabs[:4]):
        with pytest.raises(ValueError, match="nsc2d_residual_tables"):
            ops.nsc2d_residual(z, z, t, 5.0)
    with pytest.raises(ValueError, match="forcing_spec"):
        ops.nsc2d_residual(z, z, tabs, 5.0, torch.zeros(M, 8))
    with pytest.raises(ValueError, match="scalar_weight"):
        ops.nsc2d_residual(z, z, tabs, 5.0, None, -1.0)
    with pytest.raises(RpdeError, match="GPU"):
        ops.nsc2d_residual(z, z, tabs, 5.0)
    with pytest.raises(RpdeError, match="GPU"):
        ops.nsc2d_residual_state(z, z)


# ---- 6. the config table -----------------------------------------------------------------------------------------------
def test_training_loss_parses_the_active_scalar_residual():
    from rpde.entry import residual_affine, training_loss
    from utils.loss import ActiveScalarResidualLoss, RelativeL2Loss, SumLoss
    eq = {"kind": "active_scalar", "viscosity": 1e-3, "diffusivity": 2e-3, "buoyancy": 5.0, "interval": 0.05, "forcing": "reference"}
    name, fn = training_loss({"loss": "residual"}, 2, {"equation": eq})
    assert name == "residual" and isinstance(fn, SumLoss) and fn.takes_input and fn.weights == [1.0, 0.1]
    assert isinstance(fn.terms[0], RelativeL2Loss) and isinstance(fn.terms[1], ActiveScalarResidualLoss)
    r = fn.terms[1]
    assert (r.viscosity, r.diffusivity, r.buoyancy, r.interval, r.forcing) == (1e-3, 2e-3, 5.0, 0.05, "reference")
    for none in ({k: v for k, v in eq.items() if k != "forcing"}, dict(eq, forcing=None), dict(eq, forcing="none")):
        assert training_loss({"loss": "residual"}, 2, {"equation": none})[1].terms[1].forcing is None
    for key in ("viscosity", "diffusivity", "buoyancy", "interval"):                # each missing required key
        with pytest.raises(SystemExit, match="needs viscosity, diffusivity, buoyancy and interval"):
            training_loss({"loss": "residual"}, 2, {"equation": {k: v for k, v in eq.items() if k != key}})
    with pytest.raises(SystemExit, match="kappa"):                                   # unknown key
        training_loss({"loss": "residual"}, 2, {"equation": dict(eq, kappa=1.0)})
    with pytest.raises(SystemExit, match="positive"):
        training_loss({"loss": "residual"}, 2, {"equation": dict(eq, interval=-1.0)})
    with pytest.raises(SystemExit, match="kind"):                                    # a 1-D data set names no kind
        training_loss({"loss": "residual"}, 1, {"equation": eq})
    with pytest.raises(SystemExit, match=r"kind: active_scalar, viscosity, diffusivity, buoyancy, interval, forcing"):
        training_loss({"loss": "residual"}, 2, {})                                   # the 2-D refusal names the new kind
    assert "active_scalar" in training_loss.__doc__

    # the loaders' min-max statistics are four scalars: one affine map per field
    residual_affine(fn, None, None, use_normalizer=False, minmax=True, ranges=(-1.0, 3.0, -2.0, 6.0))
    assert r._affine == (8.0, -2.0, 4.0, -1.0)
    residual_affine(fn, None, None, use_normalizer=False, minmax=True, ranges=(None,) * 4)      # not normalised
    assert r._affine is None
    with pytest.raises(SystemExit, match="min-max"):
        residual_affine(fn, None, None, use_normalizer=False, minmax=True, ranges=(torch.zeros(4),) * 4)


def test_generated_yaml_matches_the_generator_defaults(monkeypatch, tmp_path):
    from data_generation import active_scalar_2d
    from rpde.config import compose
    from rpde.entry import training_loss
    ap = {}

    class Stop(Exception):
        pass

    import argparse
    real = argparse.ArgumentParser.parse_args

    def grab(self, argv=None):
        ap["args"] = real(self, argv)
        raise Stop

    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", grab)
    with pytest.raises(Stop):
        active_scalar_2d.main(["--out-dir", str(tmp_path)])
    monkeypatch.undo()
    a = ap["args"]
    cfg = compose(os.path.join(DROPIN, "conf"), "config", ["dataset=ns/ns_active_generated", "model=ffno_2d/ffno_2d_3ch",
                                                           "training.loss=residual"])
    eq = dict(cfg.dataset.equation)
    assert eq == {"kind": "active_scalar", "viscosity": a.visc, "diffusivity": a.kappa, "buoyancy": a.beta,
                  "interval": eq["interval"], "forcing": "reference"}
    assert eq["interval"] == pytest.approx(a.T / a.record_steps, rel=1e-15)
    assert int(cfg.dataset.dataset_params.reduced_resolution_t) == 1
    r = training_loss(cfg.training, 2, cfg.dataset)[1].terms[1]
    assert (r.viscosity, r.diffusivity, r.buoyancy, r.interval, r.forcing) == (a.visc, a.kappa, a.beta, eq["interval"], "reference")


# ---- 7, 8. the C ABI ---------------------------------------------------------------------------------------------------
ENTRIES = {"state": ("nsc2d_residual_state", ()), "fwd": ("nsc2d_residual_fwd", (1.0, 5.0)), "bwd": ("nsc2d_residual_bwd", (5.0,))}


def _call(lib, entry, floats, dims, ws_bytes, affine, tail=()):
    """the entry with dummy pointers (non-null, 256-byte aligned), a real `affine`, these floats and dims"""
    from rpde import _lib as L
    floats, ints, args = list(floats), list(dims) + list(tail), []
    sig = L._SIGNATURES["rpde_" + entry][1][:-3]
    first_int = next(i for i, t in enumerate(sig) if t is L._I)
    aff_at = max(i for i, t in enumerate(sig[:first_int]) if t is L._P) - {"nsc2d_residual_state": 1, "nsc2d_residual_fwd": 4,
                                                                           "nsc2d_residual_bwd": 4}[entry]
    for i, t in enumerate(sig):
        if t is L._P:
            args.append(affine if i == aff_at else FAKE)
        elif t is L._F:
            args.append(floats.pop(0))
        else:
            args.append(ints.pop(0))
    assert not floats and not ints
    return getattr(lib, "rpde_" + entry)(*args, FAKE, ws_bytes, None)


def test_library_exports_and_the_arena_query():
    from rpde import _lib as L
    lib = L.load()
    for name in ("arena_bytes", "spec_elems", "state", "fwd", "bwd"):
        assert hasattr(lib, "rpde_nsc2d_residual_" + name)
    # the query's name does not end in _ws_bytes (include/rpde.h has the reason)
    assert not any(n.startswith("rpde_nsc2d_residual") and n.endswith("_ws_bytes") for n in L._SIGNATURES)
    for B, M, N in R.CASES + [(32, 64, 64), (1, 4096, 4)]:
        need = lib.rpde_nsc2d_residual_arena_bytes(B, M, N)
        assert need > 0 and need % 256 == 0
        assert lib.rpde_nsc2d_residual_spec_elems(B, M, N) == 5 * B * M * 2 * ((N // 2 + 4) // 4 * 4)
    for B, M, N in ((2, 15, 24), (2, 16, 23), (2, 2, 24), (2, 16, 4098), (0, 16, 24), (-1, 16, 24), (5462, 16, 24), (2, 1, 24)):
        assert lib.rpde_nsc2d_residual_arena_bytes(B, M, N) == 0 and lib.rpde_nsc2d_residual_spec_elems(B, M, N) == 0
    assert lib.rpde_nsc2d_residual_arena_bytes(5461, 16, 24) > 0                    # 12 B <= 65535


@pytest.mark.parametrize("which", sorted(ENTRIES))
@pytest.mark.parametrize("dims", [(2, 16, 24), (3, 8, 8), (1, 64, 64)], ids=R.case_id)
def test_query_covers_every_entry_and_the_verdict_comes_first(which, dims):
    """each entry reports `workspace too small (given, needs)` one byte short of its own layout and gets past that verdict
    with the query's size -- to the last argument check, of the affine map, which the call fails on purpose: nothing
    here reaches the device (the pointers are dummies).  The query is the largest of the three layouts"""
    from rpde import _lib as L
    lib = L.load()
    entry, floats = ENTRIES[which]
    tail = () if which == "state" else (1,)
    good, bad = (C.c_float * 4)(1.0, 0.0, 1.0, 0.0), (C.c_float * 4)(1.0, float("nan"), 1.0, 0.0)
    query = lib.rpde_nsc2d_residual_arena_bytes(*dims)

    def refused(given):
        assert _call(lib, entry, floats, dims, given, good, tail) == L.ERR_WORKSPACE, lib.rpde_last_error()
        m = re.fullmatch(rf"{entry}: workspace too small \((\d+) bytes, needs (\d+)\)", lib.rpde_last_error().decode())
        assert m, lib.rpde_last_error()
        return int(m.group(1)), int(m.group(2))

    _, own = refused(0)
    assert 0 < own <= query and own % 256 == 0
    assert refused(own - 1) == (own - 1, own)
    for given in (own, query):
        assert _call(lib, entry, floats, dims, given, bad, tail) == L.ERR_ARG
        assert lib.rpde_last_error().decode() == f"{entry}: the affine map (a_p, b_p, a_x, b_x) must be finite"
    if which == "fwd":
        assert own == query or _call(lib, "nsc2d_residual_bwd", (5.0,), dims, 0, good, (1,)) == L.ERR_WORKSPACE


def test_the_query_is_the_largest_layout():
    from rpde import _lib as L
    lib = L.load()
    good = (C.c_float * 4)(1.0, 0.0, 1.0, 0.0)
    for dims in ((2, 16, 24), (2, 4, 6), (1, 64, 64)):
        needs = []
        for which, (entry, floats) in ENTRIES.items():
            assert _call(lib, entry, floats, dims, 0, good, () if which == "state" else (1,)) == L.ERR_WORKSPACE
            needs.append(int(re.search(rb"needs (\d+)", lib.rpde_last_error()).group(1)))
        assert max(needs) == lib.rpde_nsc2d_residual_arena_bytes(*dims)


def test_entries_refuse_bad_arguments_before_any_device_work():
    from rpde import _lib as L
    lib = L.load()
    good = (C.c_float * 4)(1.0, 0.0, 1.0, 0.0)
    big = lib.rpde_nsc2d_residual_arena_bytes(2, 16, 24)
    for which, (entry, floats) in ENTRIES.items():
        tail = () if which == "state" else (1,)
        for B, M, N in ((2, 15, 24), (2, 16, 23), (2, 2, 24), (0, 16, 24), (5462, 16, 24)):
            assert _call(lib, entry, floats, (B, M, N), big, good, tail) == L.ERR_ARG
            msg = lib.rpde_last_error()
            assert entry.encode() in msg and b"bad B=" in msg and b"12 B <= 65535" in msg, msg
    for lam, beta in ((-1.0, 5.0), (float("nan"), 5.0), (1.0, float("inf"))):
        assert _call(lib, "nsc2d_residual_fwd", (lam, beta), (2, 16, 24), big, good, (1,)) == L.ERR_ARG
        assert b"scalar_weight" in lib.rpde_last_error()
