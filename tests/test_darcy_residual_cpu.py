"""What the Darcy equation-residual loss decides without a GPU: the C entries (exports, sizes, the workspace verdict of
each entry against rpde_darcy2d_ws_bytes, argument errors), the host tables against the restatement
tests/darcy_residual_ref.py and a closed form, the restatement's gradient formula against float64 autograd, the energy
sandwich a_min <= r.P^-1 r / e.A e <= a_max that the choice of the norm rests on, and the host side: DarcyResidualLoss,
training.loss=residual with `kind: darcy` and the shipped yaml."""
import os
import re

import numpy as np
import pytest
import torch

from tests import darcy_ref as R
from tests import darcy_residual_ref as Q
from tests.conftest import DROPIN, REPO

FAKE = 1 << 20      # a pointer that is never dereferenced: argument errors come before any device work
NAMES = ("rpde_darcy2d_residual_spec_elems", "rpde_darcy2d_residual_fwd", "rpde_darcy2d_residual_bwd")


# ---- 1. ABI ----------------------------------------------------------------------------------------------------------
def test_symbols_are_in_the_header_and_the_signatures():
    from rpde import _lib
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "rpde.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib._SIGNATURES and re.search(rf"\b{name}\(", header), name
    # no workspace query of its own: the Darcy family's serves it
    assert not any(n.startswith("rpde_darcy2d_residual") and n.endswith("_ws_bytes") for n in _lib._SIGNATURES)


def test_spec_elems_at_the_refusal_boundaries():
    from rpde import _lib
    se = _lib.load().rpde_darcy2d_residual_spec_elems
    assert se(2, 16) == 512 and se(1, 8) == 64 and se(1, 512) == 512 * 512 and se(65535, 8) == 65535 * 64
    for B, s in ((1, 6), (1, 10), (1, 516), (0, 16), (65536, 16), (-1, 16), (1, 4), (1, 0)):
        assert se(B, s) == 0, (B, s)


def _fwd(lib, B=2, s=16, p=FAKE, a=FAKE, f=FAKE, S=FAKE, il=FAKE, D=1.0, stats=FAKE, spec=FAKE, ws=FAKE, n=0):
    return lib.rpde_darcy2d_residual_fwd(p, a, f, S, il, D, None, FAKE, FAKE, stats, spec, B, s, 1, ws, n, None)


def _bwd(lib, B=2, s=16, a=FAKE, spec=FAKE, S=FAKE, stats=FAKE, gl=FAKE, gr=None, gp=FAKE, ws=FAKE, n=0):
    return lib.rpde_darcy2d_residual_bwd(a, spec, S, None, stats, gl, gr, gp, B, s, 1, ws, n, None)


@pytest.mark.parametrize("dims", [(2, 16), (3, 8), (1, 100), (5, 512)], ids=str)
@pytest.mark.parametrize("entry", ["fwd", "bwd"])
def test_each_entry_reports_a_short_workspace_from_its_own_layout(entry, dims):
    """before it plans or launches: dummy pointers, no device.  N is a multiple of 256 and fits the family's query"""
    from rpde import _lib as L
    lib = L.load()
    B, s = dims
    call = _fwd if entry == "fwd" else _bwd

    def refused(given, **kw):
        assert call(lib, B, s, n=given, **kw) == L.ERR_WORKSPACE, lib.rpde_last_error()
        m = re.fullmatch(rf"darcy2d_residual_{entry}: workspace too small \((\d+) bytes, needs (\d+)\)", lib.rpde_last_error().decode())
        assert m, lib.rpde_last_error()
        return int(m.group(1)), int(m.group(2))

    given, need = refused(0)
    assert given == 0 and need > 0 and need % 256 == 0 and need <= lib.rpde_darcy2d_ws_bytes(B, s)
    assert need >= 2 * B * s * s * 4                                             # two fields in the dual norm
    assert refused(need - 256) == (need - 256, need)
    if entry == "fwd":
        # L2 (no tables): the partial sums alone, less than the dual norm's
        _, l2 = refused(0, S=None, il=None)
        assert 0 < l2 < need and l2 % 256 == 0


def test_argument_errors_are_reported_without_a_gpu():
    from rpde import _lib as L
    lib = L.load()
    nws = lib.rpde_darcy2d_ws_bytes(2, 16)
    for call, name, nulls, aligned in ((_fwd, b"darcy2d_residual_fwd", ("p", "a", "f", "stats", "spec", "ws"), ("p", "a", "f", "S", "il", "spec")),
                                       (_bwd, b"darcy2d_residual_bwd", ("a", "spec", "stats", "gp", "ws"), ("a", "spec", "S", "gp"))):
        for k in nulls:
            assert call(lib, n=nws, **{k: None}) == L.ERR_ARG, (name, k)
            assert name in lib.rpde_last_error() and b"null" in lib.rpde_last_error(), (name, k)
        for B, s in ((2, 6), (2, 10), (2, 516), (0, 16), (65536, 16), (-1, 16)):
            assert call(lib, B, s, n=nws) == L.ERR_ARG, (name, B, s)
            msg = lib.rpde_last_error()
            assert name in msg and b"bad B=" in msg and b"8 .. 512" in msg and b"65535" in msg, msg
        for k in aligned:
            assert call(lib, n=nws, **{k: FAKE + 4}) == L.ERR_ARG and b"aligned" in lib.rpde_last_error(), (name, k)
        assert call(lib, n=nws, ws=FAKE + 64) == L.ERR_ARG and b"aligned" in lib.rpde_last_error()
    assert _fwd(lib, n=nws, S=None) == L.ERR_ARG and b"together" in lib.rpde_last_error()     # one table without the other
    assert _fwd(lib, n=nws, il=None) == L.ERR_ARG
    for D in (0.0, -1.0, float("inf"), float("nan")):
        assert _fwd(lib, n=nws, D=D) == L.ERR_ARG and b"positive" in lib.rpde_last_error(), D
    assert _bwd(lib, n=nws, gl=None, gr=None) == L.ERR_ARG and b"null" in lib.rpde_last_error()   # one upstream gradient is needed


# ---- 2. tables -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [8, 12, 20, 100])
def test_tables_equal_the_restatement_rounded_once(s):
    from rpde import ops
    f, S, il, D = ops.darcy2d_residual_tables(s)
    S64, il64 = Q.tables(s)
    for t in (f, S, il):
        assert t.dtype == torch.float32 and tuple(t.shape) == (s, s) and t.is_contiguous() and not t.is_cuda
    assert np.array_equal(f.numpy(), np.ones((s, s), np.float32)) and np.array_equal(S.numpy(), S64.astype(np.float32))
    assert np.allclose(il.numpy(), il64.astype(np.float32), rtol=2e-7, atol=0)
    assert torch.equal(S, ops.darcy2d_tables(s)[0]) and torch.equal(il, ops.darcy2d_tables(s)[1])     # the solver's own
    assert isinstance(D, float) and D == pytest.approx(Q.denominator(np.ones((s, s)), "dual"), rel=1e-13)
    f2, S2, il2, D2 = ops.darcy2d_residual_tables(s, forcing=2.5, norm="l2")
    assert S2 is None and il2 is None and D2 == pytest.approx(2.5 * s, rel=1e-15) and float(f2[3, 5]) == 2.5
    field = torch.from_numpy(R.neumann_field(1, s, seed=3)[0])
    f3, _, _, D3 = ops.darcy2d_residual_tables(s, forcing=field)
    assert torch.equal(f3, field.float()) and D3 == pytest.approx(Q.denominator(field.float().numpy(), "dual"), rel=1e-13)


@pytest.mark.parametrize("s", [8, 12])
def test_denominator_against_the_closed_form(s):
    """f = 1: (S 1)_k = sqrt(2/s) sum_i sin(pi (k+1) (i+1/2) / s) = sqrt(2/s) sin^2(pi (k+1) / 2) / sin(pi (k+1) / (2 s)) in
    closed form (the last row over sqrt 2), so D^2 = sum_{k1, k2} (S 1)_k1^2 (S 1)_k2^2 / (l_k1 + l_k2) without the table"""
    from rpde import ops
    k = np.arange(1, s + 1, dtype=np.float64)
    v = np.sqrt(2.0 / s) * np.sin(np.pi * k / 2) ** 2 / np.sin(np.pi * k / (2 * s))
    v[s - 1] /= np.sqrt(2.0)
    lam = float(s) ** 2 * (2.0 - 2.0 * np.cos(np.pi * k / s))
    want = np.sqrt(np.sum(np.outer(v * v, v * v) / (lam[:, None] + lam[None, :])))
    assert ops.darcy2d_residual_tables(s)[3] == pytest.approx(want, rel=1e-12)
    # and it is the energy norm of the a = 1 solution: f . P^-1 f = u . A(1) u
    u = R.direct(np.ones((1, s, s)), np.ones((s, s)))
    assert want ** 2 == pytest.approx(float(np.sum(u * R.apply(np.ones((1, s, s)), u))), rel=1e-11)


def test_tables_check_their_arguments():
    from rpde import ops
    for bad in (dict(s=6), dict(s=10), dict(s=516), dict(s=16, forcing=0.0), dict(s=16, forcing=torch.zeros(16, 16)),
                dict(s=16, norm="h1"), dict(s=16, forcing=torch.ones(8, 8)), dict(s=16, forcing=torch.ones(2, 16, 16)),
                dict(s=16, forcing=float("nan"))):
        with pytest.raises(ValueError, match="darcy2d_residual_tables"):
            ops.darcy2d_residual_tables(**bad)


def test_op_refuses_shapes_tables_and_cpu_tensors():
    from rpde import ops
    from rpde._lib import RpdeError
    s = 16
    tabs = ops.darcy2d_residual_tables(s)
    z = torch.ones(2, s, s)
    bad = [(torch.ones(2, 2, s, s),) * 2, (torch.ones(2, 1, s, s), z), (torch.ones(s, s),) * 2, (z, torch.ones(2, s, s + 4)),
           (z.double(), z.double()), (torch.ones(2, s, s + 4),) * 2, (torch.ones(2, 10, 10),) * 2, (torch.ones(2, 516, 516),) * 2]
    for p, a in bad:
        with pytest.raises(ValueError, match="darcy2d_residual"):
            ops.darcy2d_residual(p, a, tabs)
    with pytest.raises(ValueError, match="8 .. 512"):                            # the limits are in the message
        ops.darcy2d_residual(torch.ones(2, 10, 10), torch.ones(2, 10, 10), tabs)
    other = ops.darcy2d_residual_tables(20)
    for t in (other, tabs[:3], (tabs[0], tabs[1], None, tabs[3]), (None,) + tuple(tabs[1:]), tuple(tabs[:3]) + (0.0,),
              tuple(tabs[:3]) + (tabs[0],)):
        with pytest.raises(ValueError, match="darcy2d_residual"):
            ops.darcy2d_residual(z, z, t)
    with pytest.raises(ValueError, match="affine"):
        ops.darcy2d_residual(z, z, tabs, (1.0, 0.0))
    for p, a in ((z, z), (z[:, None], z[:, None])):                              # well formed: refused as CPU tensors only
        for t in (tabs, ops.darcy2d_residual_tables(s, norm="l2")):
            with pytest.raises(RpdeError, match="GPU"):
                ops.darcy2d_residual(p, a, t)


# ---- 3. the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", Q.NORMS)
@pytest.mark.parametrize("case", [(3, 8), (2, 12), (2, 20)], ids=Q.case_id)
def test_gradient_formula_against_autograd(case, norm):
    """the formula the device implements against float64 autograd of the same restatement written in torch, with an
    affine decode and per-sample weights; and against central differences on the smallest grid"""
    ref = Q.parity_reference(case, "12_3", "white", norm)
    a, f, p = ref["a"], ref["f"], ref["p"]
    affine = (1.3, -0.2, 0.7, 0.4)
    w = np.array([0.6, -1.7, 0.9][:case[0]])
    for aff in (None, affine):
        pt = torch.from_numpy(p).double().requires_grad_(True)
        v = Q.rel_torch(a, pt, f, norm, aff)
        (v * torch.from_numpy(w)).sum().backward()
        r, g = Q.rel_and_grad(a, p, f, np.float64, norm, aff, w)
        assert np.abs(v.detach().numpy() - r).max() <= 1e-13 * r.max()
        assert np.linalg.norm(pt.grad.numpy() - g) / np.linalg.norm(g) < 1e-12
    if case == (3, 8):
        p64, eps = p.astype(np.float64), 1e-6
        _, g = Q.rel_and_grad(a, p64, f, np.float64, norm, affine, w)
        fd = np.zeros_like(p64)
        for i in range(p64.size):
            d = np.zeros(p64.size)
            d[i] = eps
            d = d.reshape(p64.shape)
            fd.ravel()[i] = ((Q.rel(a, p64 + d, f, np.float64, norm, affine) - Q.rel(a, p64 - d, f, np.float64, norm, affine)) * w).sum() / (2 * eps)
        assert np.linalg.norm(g - fd) / np.linalg.norm(fd) < 1e-6


@pytest.mark.parametrize("contrast", Q.CONTRASTS)
@pytest.mark.parametrize("case", Q.CASES, ids=Q.case_id)
def test_energy_sandwich(case, contrast):
    """a_min e.A e <= r.P^-1 r <= a_max e.A e in float64, e = u* - p: what makes the dual norm the energy-norm error to
    within the contrast at every grid size.  And the floors of the float32 restatement on these inputs are small enough
    that FLOOR_FACTOR times them decides something: the condition of the device tests' bounds"""
    hi, lo = R.CONTRASTS[contrast][:2]
    for kind in Q.KINDS:
        ref = Q.parity_reference(case, contrast, kind, "dual")
        ratio = Q.energy_ratio(ref["a"], ref["p"], ref["u64"], ref["f"])
        print(case, contrast, kind, "E / e.Ae", ratio.tolist(), "rel", ref["rel64"].tolist())
        assert (ratio >= lo * (1 - 1e-9)).all() and (ratio <= hi * (1 + 1e-9)).all()
        for norm in Q.NORMS:
            ref = Q.parity_reference(case, contrast, kind, norm)
            assert ref["floor_rel"] <= 1e-5 and ref["floor_grad"] <= 1e-4, (norm, ref["floor_rel"], ref["floor_grad"])
            assert np.abs(ref["zero64"] - 1.0).max() < 1e-7                      # the trivial predictor p = 0 is rel = 1


def test_l2_grows_with_the_grid_and_the_dual_norm_does_not():
    """the same 5 % smooth error, float64, coefficients 12 / 3: L2 grows several times from s = 8 to s = 100, the dual
    norm stays within a factor two"""
    (d8, l8), (d100, l100) = ([Q.parity_reference(c, "12_3", "smooth", n)["rel64"].max() for n in ("dual", "l2")]
                              for c in ((3, 8), (1, 100)))
    print("dual", d8, d100, "l2", l8, l100)
    assert l100 > 5 * l8 and d100 < 2 * d8 and d8 < 2 * d100


# ---- 4. host side ----------------------------------------------------------------------------------------------------
def test_loss_class():
    from utils.loss import DarcyResidualLoss, SumLoss, _ResidualLoss
    v = DarcyResidualLoss()
    assert isinstance(v, _ResidualLoss) and v.takes_input is True and v.dims == 2 and (v.forcing, v.norm) == (1.0, "dual")
    assert DarcyResidualLoss(forcing=2, norm="l2").forcing == 2.0
    for bad in (dict(forcing=0.0), dict(forcing=float("inf")), dict(forcing="one"), dict(norm="h1"), dict(forcing=torch.zeros(8, 8)),
                dict(forcing=torch.ones(2, 8, 8)), dict(forcing=torch.ones(8, 12))):
        with pytest.raises(ValueError, match="DarcyResidualLoss"):
            DarcyResidualLoss(**bad)
    v.set_affine(pred=(2.0, 1.0), inp=(3.0, -1.0))
    assert v._affine == (2.0, 1.0, 3.0, -1.0)
    v.set_affine()
    assert v._affine is None
    with pytest.raises(ValueError, match="set_affine"):
        v.set_affine(inp=(float("nan"), 0.0))
    with pytest.raises(ValueError, match="two-dimensional"):
        v.warm((8,), "cpu")
    with pytest.raises(ValueError, match="input"):
        v(torch.ones(1, 8, 8), None, None)
    for shape in ((2, 2, 8, 8), (8, 8), (2, 1, 1, 8, 8)):
        with pytest.raises(ValueError, match="one channel"):
            v(torch.ones(shape), None, torch.ones(shape))
    for grid in ((8, 12), (10, 10), (516, 516)):
        with pytest.raises(ValueError):
            v._table(grid, "cpu")
    # tables per (grid, device): two grids, two entries, built once each
    t1, t2 = v._table((8, 8), "cpu"), v._table((16, 16), "cpu")
    assert tuple(t1[1].shape) == (8, 8) and tuple(t2[0].shape) == (16, 16) and isinstance(t1[3], float) and t2[3] != t1[3]
    assert v._table((8, 8), "cpu")[0] is t1[0] and len(v._tables) == 2
    l2 = DarcyResidualLoss(norm="l2")._table((8, 8), "cpu")
    assert l2[1] is None and l2[2] is None and l2[3] == 8.0
    assert SumLoss([(1.0, torch.nn.MSELoss()), (0.1, v)]).takes_input is True


def test_explicit_forcing_serves_one_grid():
    from utils.loss import DarcyResidualLoss
    field = torch.from_numpy(R.neumann_field(1, 8, seed=3)[0])
    e = DarcyResidualLoss(forcing=field)
    assert e.forcing == "explicit" and torch.equal(e._table((8, 8), "cpu")[0], field.float())
    with pytest.raises(ValueError, match="grid"):
        e._table((16, 16), "cpu")
    with pytest.raises(ValueError, match="grid"):
        DarcyResidualLoss(forcing=field)._table((16, 16), "cpu")                 # a first use on another grid as well


def test_training_loss_parses_the_darcy_residual():
    from rpde.entry import residual_affine, training_loss
    from utils.loss import DarcyResidualLoss, RelativeL2Loss, SumLoss
    name, fn = training_loss({"loss": "residual"}, 2, {"equation": {"kind": "darcy"}})
    assert name == "residual" and isinstance(fn, SumLoss) and fn.takes_input and fn.weights == [1.0, 0.1]
    assert isinstance(fn.terms[0], RelativeL2Loss) and isinstance(fn.terms[1], DarcyResidualLoss)
    r = fn.terms[1]
    assert (r.forcing, r.norm) == (1.0, "dual")
    _, fn2 = training_loss({"loss": "residual", "loss_lambda": 0.5}, 2,
                           {"equation": {"kind": "darcy", "forcing": 2.0, "norm": "l2"}, "dataset_params": {"reduced_resolution": 1}})
    assert fn2.weights == [1.0, 0.5] and (fn2.terms[1].forcing, fn2.terms[1].norm) == (2.0, "l2")
    eq = {"kind": "darcy", "forcing": 1.0, "norm": "dual"}
    for training, dims, dataset, word in (({"loss": "residual"}, 2, {"equation": dict(eq, viscosity=1.0)}, "viscosity"),
                                          ({"loss": "residual"}, 2, {"equation": dict(eq, norm="h1")}, "norm"),
                                          ({"loss": "residual"}, 2, {"equation": dict(eq, forcing=0.0)}, "zero"),
                                          ({"loss": "residual"}, 2, {"equation": eq, "dataset_params": {"reduced_resolution": 2}}, "reduced_resolution"),
                                          ({"loss": "residual"}, 1, {"equation": eq}, "kind"),
                                          ({"loss": "residual"}, 2, {"equation": {"kind": "stokes"}}, "one-dimensional"),
                                          ({"loss": "residual"}, 2, {"equation": {"forcing": 1.0}}, "one-dimensional")):
        with pytest.raises(SystemExit, match=word):
            training_loss(training, dims, dataset)

    class Simple:
        mean, std, eps = 0.5, 2.0, 1e-5

    residual_affine(fn, Simple(), Simple(), use_normalizer=False)
    assert r._affine == (2.0 + 1e-5, 0.5, 2.0 + 1e-5, 0.5)
    residual_affine(fn, Simple(), Simple(), use_normalizer=True)                 # train() decodes the prediction itself
    assert r._affine == (1.0, 0.0, 2.0 + 1e-5, 0.5)
    residual_affine(fn, None, None, use_normalizer=True)
    assert r._affine is None


def test_the_shipped_yaml_composes(monkeypatch, tmp_path):
    from data_generation import darcy_2d
    from rpde.config import compose
    from rpde.entry import training_loss
    from tests.test_etd_residual_cpu import _defaults
    conf = os.path.join(DROPIN, "conf")
    cfg = compose(conf, "config", ["dataset=darcy_flow/darcy_generated", "training.loss=residual"])
    a = _defaults(darcy_2d, monkeypatch, tmp_path / "x.npz")
    assert dict(cfg.dataset.equation) == {"kind": "darcy", "forcing": a.forcing, "norm": "dual"}
    assert int(cfg.dataset.dims) == 2 and int(cfg.dataset.dataset_params.reduced_resolution) == 1
    assert str(cfg.dataset.dataset_params.normalization_type) == "simple"
    r = training_loss(cfg.training, 2, cfg.dataset)[1].terms[1]
    assert (r.forcing, r.norm) == (a.forcing, "dual")
    strided = compose(conf, "config", ["dataset=darcy_flow/darcy_generated", "training.loss=residual",
                                       "dataset.dataset_params.reduced_resolution=2"])
    with pytest.raises(SystemExit, match="reduced_resolution"):
        training_loss(strided.training, 2, strided.dataset)
    # without training.loss=residual the mapping is not read
    assert training_loss(compose(conf, "config", ["dataset=darcy_flow/darcy_generated"]).training, 2, cfg.dataset) == ("l2", None)
