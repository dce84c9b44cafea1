"""What the equation-residual loss decides without a GPU: the tables of rpde.ops.etd1d_residual_tables against the
restatement tests/etd_residual_ref.py, the restatement's own gradient formula against finite differences, that the
residual tells an exact pair from the trivial predictor, the argument errors of the two C entries, and the host side:
training.loss=residual, SumLoss' routing of the input and the `equation:` blocks of the generated data sets."""
import argparse
import math
import os

import pytest
import torch

from tests import etd_residual_ref as R
from tests.conftest import DROPIN

FAKE = 1 << 20      # a pointer that is never dereferenced: argument errors come before any device work


# ---- 1. tables -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [6, 12, 48, 64])
@pytest.mark.parametrize("symbol", list(R.SYMBOLS))
def test_tables_equal_the_restatement_rounded_once(symbol, N):
    from rpde import ops
    c1, c2, c3, c4, length, h, _, _ = R.SYMBOLS[symbol]
    K, kp = N // 2 + 1, (N // 2 + 1 + 3) // 4 * 4
    got = ops.etd1d_residual_tables(N, length(N), c1, c2, c3, c4, h)
    want = R.tables(N, length(N), c1, c2, c3, c4, h)
    assert len(got) == 3
    for tn, t, w in zip(("E", "m0", "m1"), got, want):
        assert t.dtype == torch.float32 and tuple(t.shape) == (2, kp) and t.is_contiguous() and not t.is_cuda, tn
        assert not t[:, K:].any(), tn                                           # padding zero
        # formed in float64 and rounded once: one fp32 rounding of the float64 restatement
        assert torch.allclose(t[0, :K].double(), w.real, rtol=2.0 ** -23, atol=1e-300), tn
        assert torch.allclose(t[1, :K].double(), w.imag, rtol=2.0 ** -23, atol=1e-300), tn
    E, m0, m1 = got
    assert float(E[0, 0]) == 1.0 and float(E[1, 0]) == 0.0 and float(E[1, N // 2]) == 0.0
    if c1 == 0.0 and c3 == 0.0:
        assert not E[1].any()                                                   # z real: Im E stored as zero
    else:
        assert E[1, 1:N // 2].any()
    for t in (m0, m1):
        assert not t[:, 0].any() and not t[:, N // 2].any()                     # g_0 = g_{N/2} = 0
        assert t[:, 1].any()
    # g carries the de-aliasing: nothing above (2/3)(N/2)
    cut = int((2.0 / 3.0) * (N // 2))
    assert not m0[:, cut + 1:].any() and not m1[:, cut + 1:].any()
    full = ops.etd1d_residual_tables(N, length(N), c1, c2, c3, c4, h, dealias=False)
    assert full[1][:, N // 2 - 1].any() and torch.equal(full[0], E)
    half = ops.etd1d_residual_tables(N, length(N), c1, c2, c3, c4, h, advect=0.5)
    assert torch.allclose(half[2], 0.5 * m1, rtol=3e-7, atol=0)


def test_tables_check_their_arguments():
    from rpde import ops
    for bad in ((31, 2.0, 0.1), (2, 2.0, 0.1), (32, -2.0, 0.1), (32, 2.0, 0.0)):
        with pytest.raises(ValueError, match="etd1d_residual_tables"):
            ops.etd1d_residual_tables(bad[0], bad[1], 0.0, -0.1, 0.0, 0.0, bad[2])


def test_small_interval_limit_of_the_tables():
    """z -> 0: phi1 -> 1, phi2 -> 1/2, so m0 = m1 = (D/2) i g: the plain trapezoidal rule"""
    N, length, h = 16, 2.0, 1e-6
    E, m0, m1 = R.tables(N, length, 0.0, -0.1, 0.0, 0.0, h, dealias=False)
    kappa = 2 * math.pi * torch.arange(N // 2 + 1, dtype=torch.float64) / length
    g = -0.5 * kappa
    g[-1] = 0.0
    assert torch.allclose(m0.imag, 0.5 * h * g, rtol=1e-4, atol=0) and torch.allclose(m1.imag, 0.5 * h * g, rtol=1e-4, atol=0)
    assert float(m0.real.abs().max()) < 1e-18 and float((E - 1).abs().max()) < 1e-3


# ---- 2. the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symbol", list(R.SYMBOLS))
def test_gradient_formula_against_finite_differences(symbol):
    """the closed form the device implements, the restatement's autograd and central differences agree in float64, with
    an affine decode and per-sample weights"""
    case = (2, 12)
    ref = R.parity_reference(symbol, case, "noisy")
    p, x, tabs = ref["p"].double(), ref["x"].double(), ref["tabs64"]
    affine = (1.3, -0.2, 0.7, 0.4)
    w = torch.tensor([0.6, -1.7], dtype=torch.float64)
    _, auto = R.rel_and_grad(p, x, tabs, affine, w)
    form = R.grad_formula(p, x, tabs, affine, w)
    assert float((form - auto).norm() / auto.norm()) < 1e-13
    eps = 1e-6
    fd = torch.zeros_like(p)
    for b in range(p.shape[0]):
        for j in range(p.shape[1]):
            d = torch.zeros_like(p)
            d[b, j] = eps
            fd[b, j] = ((R.rel(p + d, x, tabs, affine) - R.rel(p - d, x, tabs, affine)) * w).sum() / (2 * eps)
    assert float((form - fd).norm() / fd.norm()) < 1e-7


@pytest.mark.parametrize("symbol", ["ks", "burgers"])
def test_exact_pair_is_far_below_persistence(symbol):
    """float64, N = 64, the truth from ETDRK4 at a tenth of the case's dt: rel(true next) < 0.1 rel(p = x) per sample
    (measured: more than 100 x on KS, 50 x on Burgers), and the true pair's residual falls about as interval^3"""
    case = (8, 64)
    c1, c2, c3, c4, length, h, _, _ = R.SYMBOLS[symbol]
    sol = R.trajectory(symbol, case, fine=10)
    tabs = R.tables(64, length(64), c1, c2, c3, c4, h)
    true, still = R.rel(sol[:, 2], sol[:, 1], tabs), R.rel(sol[:, 1], sol[:, 1], tabs)
    print(symbol, "true", true.tolist(), "persistence", still.tolist())
    assert bool((true < 0.1 * still).all())
    if symbol == "ks":
        # the same x = u(h) with p = u(3 h), twice the interval: third order gives 2^3 (measured 8.0 .. 8.8), second
        # order would give 4
        tabs2 = R.tables(64, length(64), c1, c2, c3, c4, 2 * h)
        ratio = R.rel(sol[:, 2], sol[:, 0], tabs2) / R.rel(sol[:, 1], sol[:, 0], tabs)
        print("interval x 2:", ratio.tolist())
        assert bool((ratio > 6.0).all()) and bool((ratio < 12.0).all())


# ---- 3. ABI ----------------------------------------------------------------------------------------------------------
def test_argument_errors_are_reported_without_a_gpu():
    from rpde import _lib as L
    lib = L.load()
    assert lib.rpde_etd_residual_ws_bytes(2, 48) > 0 and lib.rpde_etd_residual_spec_elems(2, 48) == 2 * 2 * 28
    for B, N in ((2, 47), (2, 2), (2, 4098), (0, 48), (-1, 48), (16384, 48)):
        assert lib.rpde_etd_residual_ws_bytes(B, N) == 0 and lib.rpde_etd_residual_spec_elems(B, N) == 0, (B, N)
    assert lib.rpde_etd_residual_ws_bytes(16383, 48) > 0
    nws = lib.rpde_etd_residual_ws_bytes(2, 48)

    def fwd(B=2, N=48, p=FAKE, x=FAKE, E=FAKE, m0=FAKE, m1=FAKE, stats=FAKE, spec=FAKE, ws=FAKE, n=nws):
        return lib.rpde_etd_residual_fwd(p, x, E, m0, m1, None, FAKE, FAKE, stats, spec, B, N, 1, ws, n, None)

    def bwd(B=2, N=48, p=FAKE, spec=FAKE, m1=FAKE, stats=FAKE, gl=FAKE, gr=None, gp=FAKE, ws=FAKE, n=nws):
        return lib.rpde_etd_residual_bwd(p, spec, m1, None, stats, gl, gr, gp, B, N, 1, ws, n, None)

    for call, name, nulls in ((fwd, b"etd_residual_fwd", ("p", "x", "E", "m0", "m1", "stats", "spec", "ws")),
                              (bwd, b"etd_residual_bwd", ("p", "spec", "m1", "stats", "gp", "ws"))):
        for k in nulls:
            assert call(**{k: None}) == L.ERR_ARG, (name, k)
            assert name in lib.rpde_last_error() and b"null" in lib.rpde_last_error(), (name, k)
        for B, N in ((2, 47), (2, 2), (2, 4098), (0, 48), (-1, 48), (16384, 48)):
            assert call(B=B, N=N) == L.ERR_ARG, (name, B, N)
            msg = lib.rpde_last_error()
            assert name in msg and b"bad B=" in msg and b"16383" in msg, msg               # the limit is in the message
        assert call(n=nws // 16) == L.ERR_WORKSPACE and b"workspace too small" in lib.rpde_last_error()
        assert call(ws=FAKE + 64) == L.ERR_ARG and b"aligned" in lib.rpde_last_error()
        assert call(m1=FAKE + 4) == L.ERR_ARG and b"aligned" in lib.rpde_last_error()
        assert call(spec=FAKE + 8) == L.ERR_ARG and b"aligned" in lib.rpde_last_error()
    assert fwd(E=FAKE + 4) == L.ERR_ARG and fwd(m0=FAKE + 4) == L.ERR_ARG
    assert bwd(gl=None, gr=None) == L.ERR_ARG and b"null" in lib.rpde_last_error()     # one of the two gradients is needed


def test_op_refuses_shapes_and_cpu_tensors():
    from rpde import ops
    from rpde._lib import RpdeError
    N = 16
    tabs = ops.etd1d_residual_tables(N, 4.0, 0.0, -0.1, 0.0, 0.0, 0.05)
    z = torch.zeros(2, N)
    bad = [(torch.zeros(2, 2, N), torch.zeros(2, 2, N)),                        # two channels
           (torch.zeros(2, 1, N), z), (torch.zeros(N), torch.zeros(N)), (torch.zeros(2, 1, 1, N),) * 2,
           (z, torch.zeros(2, N + 2)), (z.double(), z.double())]
    for p, x in bad:
        with pytest.raises(ValueError, match="etd1d_residual"):
            ops.etd1d_residual(p, x, tabs)
    other = ops.etd1d_residual_tables(32, 4.0, 0.0, -0.1, 0.0, 0.0, 0.05)
    for t in (other, tabs[:2], tuple(t[0] for t in tabs)):
        with pytest.raises(ValueError, match="etd1d_residual_tables"):
            ops.etd1d_residual(z, z, t)
    with pytest.raises(ValueError, match="affine"):
        ops.etd1d_residual(z, z, tabs, affine=(1.0, 0.0))
    for p, x in ((z, z), (z[:, None], z[:, None])):                             # well formed: refused as CPU tensors only
        with pytest.raises(RpdeError, match="GPU"):
            ops.etd1d_residual(p, x, tabs)


# ---- 4. host side ----------------------------------------------------------------------------------------------------
class _Sees(torch.nn.Module):
    takes_input = True

    def __init__(self):
        super().__init__()
        self.got = None

    def forward(self, x, y, inp):
        self.got = (x, y, inp)
        return (x * 0).sum() + 3.0


def test_sum_loss_routes_the_input():
    from utils.loss import EquationResidualLoss, SumLoss
    plain = lambda x, y: ((x - y) ** 2).sum()                                    # noqa: E731

    class Plain(torch.nn.Module):
        def forward(self, x, y):
            return plain(x, y)

    x, y, inp = torch.ones(2, 4), torch.zeros(2, 4), torch.full((2, 4), 5.0)
    old = SumLoss([(2.0, Plain())])
    assert old.takes_input is False and float(old(x, y)) == 16.0 and float(old(x, y, inp)) == 16.0
    sees = _Sees()
    both = SumLoss([(1.0, Plain()), (0.5, sees)])
    assert both.takes_input is True
    assert float(both(x, y, inp)) == 8.0 + 1.5 and sees.got[2] is inp and sees.got[0] is x
    with pytest.raises(ValueError, match="input"):
        both(x, y)
    assert EquationResidualLoss.takes_input is True
    assert SumLoss([(1.0, Plain()), (0.1, EquationResidualLoss.ks(0.05, 64.0, 0.1))]).takes_input is True


def test_loss_constructors_carry_the_generators_signs():
    from utils.loss import EquationResidualLoss as E
    b, k, v = E.burgers(0.1 / math.pi, 2.0, 0.01), E.ks(0.05, 64.0, 0.1), E.kdv(1.0, 0.25, 64.0, 0.1)
    assert (b.c1, b.c2, b.c3, b.c4, b.length, b.interval) == (0.0, -0.1 / math.pi, 0.0, 0.0, 2.0, 0.01)
    assert (k.c1, k.c2, k.c3, k.c4) == (0.0, 1.0, 0.0, -0.05)
    assert (v.c1, v.c2, v.c3, v.c4) == (0.0, -0.25, 1.0, 0.0)
    for bad in (dict(length=0.0, interval=0.1), dict(length=2.0, interval=-1.0), dict(length=2.0, interval=0.1, c2=float("nan"))):
        with pytest.raises(ValueError, match="EquationResidualLoss"):
            E(**bad)
    k.set_affine(pred=(2.0, 1.0), inp=(3.0, -1.0))
    assert k._affine == (2.0, 1.0, 3.0, -1.0)
    k.set_affine()
    assert k._affine is None
    with pytest.raises(ValueError, match="one-dimensional"):
        k.warm((8, 8), "cpu")
    with pytest.raises(ValueError, match="input"):
        k(torch.zeros(1, 8), None, None)


def test_training_loss_parses_residual():
    from rpde.entry import residual_affine, training_loss
    from utils.loss import EquationResidualLoss, RelativeL2Loss, SumLoss
    eq = {"c2": 1.0, "c4": -0.05, "length": 64.0, "interval": 0.1}
    name, fn = training_loss({"loss": "residual"}, 1, {"equation": eq})
    assert name == "residual" and isinstance(fn, SumLoss) and fn.takes_input and fn.weights == [1.0, 0.1]
    assert isinstance(fn.terms[0], RelativeL2Loss) and isinstance(fn.terms[1], EquationResidualLoss)
    r = fn.terms[1]
    assert (r.c1, r.c2, r.c3, r.c4, r.advect, r.length, r.interval) == (0.0, 1.0, 0.0, -0.05, 1.0, 64.0, 0.1)
    _, fn2 = training_loss({"loss": "residual", "loss_lambda": 0.5}, 1, {"equation": dict(eq, c1=-1.0, advect=2.0)})
    assert fn2.weights == [1.0, 0.5] and fn2.terms[1].c1 == -1.0 and fn2.terms[1].advect == 2.0
    for training, dims, dataset, word in (({"loss": "residual"}, 1, {}, "equation"),
                                          ({"loss": "residual"}, 1, None, "equation"),
                                          ({"loss": "residual"}, 2, {"equation": eq}, "one-dimensional"),
                                          ({"loss": "residual"}, 1, {"equation": {"c2": 1.0, "length": 64.0}}, "interval"),
                                          ({"loss": "residual"}, 1, {"equation": dict(eq, nu=1.0)}, "nu"),
                                          ({"loss": "residual"}, 1, {"equation": dict(eq, length=-1.0)}, "positive"),
                                          ({"loss": "pinn"}, 1, {"equation": eq}, "residual")):
        with pytest.raises(SystemExit, match=word):
            training_loss(training, dims, dataset)
    # the other objectives do not look at the data set
    assert training_loss({}, 1) == ("l2", None) and training_loss({"loss": "sobolev"}, 1)[0] == "sobolev"

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
    residual_affine(RelativeL2Loss(), Pointwise(), Pointwise(), False, True)    # no residual term: nothing to refuse


class _Parsed(Exception):
    pass


def _defaults(module, monkeypatch, tmp_path):
    """the argparse defaults of a generator script: its main() up to the end of parse_args"""
    real = argparse.ArgumentParser.parse_args

    def parse(self, *a, **kw):
        raise _Parsed(real(self, *a, **kw))

    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", parse)
    with pytest.raises(_Parsed) as e:
        module.main(["--out", str(tmp_path)])
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", real)
    return e.value.args[0]


def test_equation_blocks_match_the_generator_defaults(monkeypatch, tmp_path):
    from data_generation import burgers_1d, kdv_1d, ks_1d
    from rpde.config import compose
    from rpde.entry import training_loss
    conf = os.path.join(DROPIN, "conf")
    load = lambda name: compose(conf, "config", ["dataset=" + name, "training.loss=residual"])       # noqa: E731

    cfg = load("ks/ks_generated")
    a = _defaults(ks_1d, monkeypatch, tmp_path)
    assert dict(cfg.dataset.equation) == {"c2": 1.0, "c4": -a.viscosity, "length": a.L, "interval": a.et / (a.nt - 1)}
    assert dict(cfg.dataset.equation)["interval"] == 0.1
    r = training_loss(cfg.training, 1, cfg.dataset)[1].terms[1]
    k = type(r).ks(a.viscosity, a.L, a.et / (a.nt - 1))
    assert (r.c1, r.c2, r.c3, r.c4, r.length, r.interval) == (k.c1, k.c2, k.c3, k.c4, k.length, k.interval)

    cfg = load("kdv/kdv_generated")
    a = _defaults(kdv_1d, monkeypatch, tmp_path)
    assert dict(cfg.dataset.equation) == {"c2": -a.viscosity, "c3": a.dispersion, "length": a.L, "interval": a.et / (a.nt - 1)}
    r = training_loss(cfg.training, 1, cfg.dataset)[1].terms[1]
    k = type(r).kdv(a.dispersion, a.viscosity, a.L, a.et / (a.nt - 1))
    assert (r.c1, r.c2, r.c3, r.c4, r.length, r.interval) == (k.c1, k.c2, k.c3, k.c4, k.length, k.interval)

    cfg = load("burger/burger_generated")
    a = _defaults(burgers_1d, monkeypatch, tmp_path)
    eq = dict(cfg.dataset.equation)
    assert set(eq) == {"c2", "length", "interval"} and eq["length"] == a.length
    assert eq["c2"] == pytest.approx(-a.viscosity / math.pi, rel=1e-15) and eq["interval"] == pytest.approx(a.T / (a.snapshots - 1), rel=1e-15)
    assert int(cfg.dataset.dataset_params.reduced_resolution_t) == 1            # the interval is that of consecutive snapshots
    r = training_loss(cfg.training, 1, cfg.dataset)[1].terms[1]
    assert (r.c1, r.c2, r.c3, r.c4) == (0.0, eq["c2"], 0.0, 0.0)
    # a data set without the block says so
    plain = compose(conf, "config", ["dataset=ks/ks_naive", "training.loss=residual"])
    with pytest.raises(SystemExit, match="equation"):
        training_loss(plain.training, 1, plain.dataset)
