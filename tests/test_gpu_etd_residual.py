"""The equation-residual loss on the device (csrc/etd_residual.hip through rpde.ops.etd1d_residual and
utils.loss.EquationResidualLoss) against the float64 restatement tests/etd_residual_ref.py.

The bound of every parity check is etd1d_ref.FLOOR_FACTOR (4) times the float32 restatement's own error on the same fp32
inputs (never below 2^-22), as for the generators: rel per sample, the reductions, and the gradient as a whole tensor in
relative L2.

Measured on an MI355X: all 48 parity cases hold every bound.  The "exact" cases (p the true next snapshot, rel a
remainder 1e-3 .. 2e-2 of the field) are the tight ones; the three tightest, per-sample rel:

    case                   device error of rel   bound (4 x floor)   floor of the float32 restatement
    burgers 2x64 exact     5.32e-06              1.74e-05            4.4e-06
    complex 2x64 exact     9.10e-08              9.58e-07            2^-22 (the minimum)
    burgers 2x200 exact    2.66e-06              6.22e-06            1.6e-06

What is left is the rounding of the fp32 tables (alone 5e-06 on Burgers 2x64).  The forward forms its four spectra as
float64 sums because of these cases: with the fp32 matrix-product transforms of the half-spectrum layer the same three
had 5.00e-05, 1.83e-06 and 1.70e-05 -- the error of x^ there is absolute, about 2e-07 |x| whatever the mode's own size,
and enters r^ through E x^ at every mode whose E is far from 1, against a remainder of 1e-03 |x|."""
import copy
import math

import pytest
import torch

from tests import etd1d_ref
from tests import etd_residual_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = R.FLOOR_FACTOR


def _tables(ref, N):
    from rpde import ops
    return ops.etd1d_residual_tables(N, ref["length"], *ref["coefficients"], ref["interval"])


def _run(p, x, tabs, affine=None, size_average=True, reduction=True, weights=None):
    """(value, grad_p) on the device; reduction=False: the gradient of sum_b weights_b rel_b (weights default to 1)"""
    from rpde import ops
    p = p.to(DEV).requires_grad_(True)
    v = ops.etd1d_residual(p, x.to(DEV), tabs, affine, size_average, reduction)
    if reduction:
        v.backward()
    else:
        v.backward(torch.ones_like(v) if weights is None else weights.to(DEV))
    torch.cuda.synchronize()
    return v.detach().cpu(), p.grad.detach().cpu()


def _err(a, b):
    return float((a.double() - b).norm() / b.norm())


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("symbol", list(R.SYMBOLS))
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_parity_with_float64(gpu_device, case, symbol, kind):
    """rel, the mean / sum / vector reductions and grad_p against float64, every case x symbol x kind of p"""
    B, N = case
    ref = R.parity_reference(symbol, case, kind)
    tabs = _tables(ref, N)
    rel64, grad64 = ref["rel64"], ref["grad64"]
    b_rel, b_grad = F * ref["floor_rel"], F * ref["floor_grad"]
    rel, g_vec = _run(ref["p"], ref["x"], tabs, reduction=False)
    mean, g_mean = _run(ref["p"], ref["x"], tabs, size_average=True)
    total, g_sum = _run(ref["p"], ref["x"], tabs, size_average=False)
    e_rel = float(((rel.double() - rel64).abs() / rel64).max())
    e_mean = abs(float(mean) - float(rel64.mean())) / float(rel64.mean())
    e_sum = abs(float(total) - float(rel64.sum())) / float(rel64.sum())
    e_g = _err(g_vec, grad64)
    print(f"{symbol} {case} {kind}: rel {e_rel:.2e} mean {e_mean:.2e} sum {e_sum:.2e} (bound {b_rel:.2e})  "
          f"grad {e_g:.2e} mean {_err(g_mean, grad64 / B):.2e} sum {_err(g_sum, grad64):.2e} (bound {b_grad:.2e})")
    assert tuple(rel.shape) == (B,) and mean.dim() == 0 and total.dim() == 0
    assert e_rel <= b_rel and e_mean <= b_rel and e_sum <= b_rel
    assert e_g <= b_grad and _err(g_mean, grad64 / B) <= b_grad and _err(g_sum, grad64) <= b_grad
    if case == (3, 16):
        # [B, 1, N] is the same call, and per-sample upstream gradients scale the samples' gradients
        rel3, g3 = _run(ref["p"][:, None], ref["x"][:, None], tabs, reduction=False)
        assert tuple(g3.shape) == (B, 1, N) and torch.equal(rel3, rel) and torch.equal(g3[:, 0], g_vec)
        w = torch.tensor([0.5, -2.0, 3.0])
        _, gw = _run(ref["p"], ref["x"], tabs, reduction=False, weights=w)
        assert _err(gw, grad64 * w.double()[:, None]) <= b_grad


def test_parity_beyond_256_samples(gpu_device):
    """300 samples: the one workgroup of the family's final kernel (csrc/rel_loss.hip) strides over the samples and its
    tree adds threads that hold more than one.  The checks and the bound rule of test_parity_with_float64; the floors
    of the float32 restatement here are 7.7e-7 on rel and 7.6e-7 on the gradient"""
    test_parity_with_float64(gpu_device, (300, 16), "complex", "noisy")


@pytest.mark.parametrize("case", [(2, 10), (2, 48)], ids=R.case_id)
def test_affine_decode_is_folded_in(gpu_device, case):
    B, N = case
    ref = R.parity_reference("ks", case, "noisy")
    tabs = _tables(ref, N)
    p, x = ref["p"], ref["x"]
    # one map for both fields: (p, x; a, b) is (a p + b, a x + b; identity), and grad_p carries a
    a, b = 1.75, 0.3
    aff = (a, b, a, b)
    rel64, grad64 = R.rel_and_grad(p.double(), x.double(), ref["tabs64"], aff)
    rel32, grad32 = R.rel_and_grad(p, x, R.tables(N, ref["length"], *ref["coefficients"], ref["interval"], dtype=torch.float32), aff)
    b_rel = F * max(R.MIN_FLOOR, float(((rel32.double() - rel64).abs() / rel64).max()))
    b_grad = F * max(R.MIN_FLOOR, _err(grad32, grad64))
    rel_a, g_a = _run(p, x, tabs, affine=aff, reduction=False)
    rel_i, g_i = _run(a * p + b, a * x + b, tabs, reduction=False)
    e_rel = float(((rel_a - rel_i).abs() / rel_i).max())
    print(f"affine {case}: rel {e_rel:.2e} (bound {b_rel:.2e}) grad {_err(g_a, a * g_i.double()):.2e} (bound {b_grad:.2e})")
    assert e_rel <= b_rel and _err(g_a, a * g_i.double()) <= b_grad
    assert float(((rel_a.double() - rel64).abs() / rel64).max()) <= b_rel and _err(g_a, grad64) <= b_grad
    # two different maps, against float64
    aff2 = (0.6, -0.2, 1.3, 0.1)
    rel64, grad64 = R.rel_and_grad(p.double(), x.double(), ref["tabs64"], aff2)
    rel32, grad32 = R.rel_and_grad(p, x, R.tables(N, ref["length"], *ref["coefficients"], ref["interval"], dtype=torch.float32), aff2)
    rel_2, g_2 = _run(p, x, tabs, affine=aff2, reduction=False)
    assert float(((rel_2.double() - rel64).abs() / rel64).max()) <= F * max(R.MIN_FLOOR, float(((rel32.double() - rel64).abs() / rel64).max()))
    assert _err(g_2, grad64) <= F * max(R.MIN_FLOOR, _err(grad32, grad64))


@pytest.mark.parametrize("case", [(3, 16), (3, 10), (3, 512)], ids=R.case_id)
def test_bitwise_repeatable_and_independent_of_the_batch(gpu_device, case):
    B, N = case
    ref = R.parity_reference("complex", case, "noisy")
    tabs = _tables(ref, N)
    p, x = ref["p"], ref["x"]
    first = _run(p, x, tabs, reduction=False)
    again = _run(p, x, tabs, reduction=False)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    m1, m2 = _run(p, x, tabs), _run(p, x, tabs)
    assert torch.equal(m1[0], m2[0]) and torch.equal(m1[1], m2[1])
    for b in range(B):
        alone = _run(p[b:b + 1], x[b:b + 1], tabs, reduction=False)
        assert torch.equal(alone[0][0], first[0][b]) and torch.equal(alone[1][0], first[1][b]), b


@pytest.mark.parametrize("N", [10, 16])
def test_zero_fields(gpu_device, N):
    from rpde import ops
    tabs = ops.etd1d_residual_tables(N, 4.0, 0.0, 1.0, 0.0, -0.05, 0.05)
    z = torch.zeros(2, N)
    for kw in (dict(reduction=False), dict(size_average=True), dict(size_average=False)):
        v, g = _run(z, z, tabs, **kw)
        assert bool(torch.isfinite(v).all()) and not v.any() and bool(torch.isfinite(g).all()) and not g.any()


@pytest.mark.parametrize("pde", ["ks", "burgers", "kdv"])
def test_consecutive_generator_snapshots_satisfy_the_equation(gpu_device, pde):
    """x and p are consecutive snapshots of the device generator: rel < 0.1 rel(persistence) per sample (float64
    restatement: 100 x, 50 x and 30 x below).  This pins the sign and de-aliasing conventions of the loss to the
    generator's, not merely to its own restatement."""
    from rpde import ops
    from utils.loss import EquationResidualLoss
    B, N, h = 8, 64, 0.05
    if pde == "ks":
        length, dt = 16.0, etd1d_ref.KS_DT
        u0 = etd1d_ref.ks_initial(B, N, length, 8, seed=5)
        gen = ops.etd1d_tables(N, length, 1.0, -etd1d_ref.KS_NU, dt)
        loss = EquationResidualLoss.ks(etd1d_ref.KS_NU, length, h, reduction=False)
    elif pde == "burgers":
        length, dt = etd1d_ref.BURGERS_L, etd1d_ref.BURGERS_DT
        u0 = etd1d_ref.burgers_initial(B, N, seed=5)
        gen = ops.etd1d_tables(N, length, -etd1d_ref.BURGERS_NU, 0.0, dt)
        loss = EquationResidualLoss.burgers(etd1d_ref.BURGERS_NU, length, h, reduction=False)
    else:
        length, dt = 16.0, 0.01
        u0 = 2.0 * etd1d_ref.ks_initial(B, N, length, 8, seed=5)
        gen = ops.etd1d_tables_cx(N, length, 0.0, 0.0, 1.0, 0.0, dt)
        loss = EquationResidualLoss.kdv(1.0, 0.0, length, h, reduction=False)
    every = int(round(h / dt))
    snaps = ops.etd1d_solve(u0.float().to(DEV), gen, 3 * every, every)
    x, p = snaps[:, 1].contiguous(), snaps[:, 2].contiguous()
    true, still = loss(p, None, x).cpu(), loss(x, None, x).cpu()
    print(pde, "true", true.tolist(), "persistence", still.tolist())
    assert tuple(true.shape) == (B,) and bool(torch.isfinite(true).all()) and bool((true < 0.1 * still).all())


def _sum_loss():
    from utils.loss import EquationResidualLoss, RelativeL2Loss, SumLoss
    return SumLoss([(1.0, RelativeL2Loss()), (0.1, EquationResidualLoss.ks(0.05, 16.0, 0.05))])


def test_graphed_step_matches_eager(gpu_device):
    """a tiny FNO1d trained on data + residual: three eager steps against three replays of
    rpde.graph.GraphedTrainStep(loss_takes_input=True), after warm(); the bounds of
    tests/test_gpu_spectral_loss.py::test_graphed_step_matches_eager"""
    from models.fno import FNO1d
    from rpde.graph import GraphedTrainStep
    from rpde.optim import FlatAdamW
    torch.manual_seed(3)
    m_e = FNO1d(1, 1, modes=4, width=8).to(gpu_device).train()
    m_g = copy.deepcopy(m_e)
    xs = [torch.randn(4, 1, 64, device=gpu_device) for _ in range(3)]
    ys = [torch.randn(4, 1, 64, device=gpu_device) for _ in range(3)]
    loss_fn = _sum_loss()
    loss_fn.warm((64,), gpu_device)
    o_e = FlatAdamW(m_e.parameters(), lr=1e-3, capturable=True)
    o_g = FlatAdamW(m_g.parameters(), lr=1e-3, capturable=True)
    warm = 2
    for _ in range(warm):
        o_e.zero_grad(set_to_none=False)
        loss_fn(m_e(xs[0]), ys[0], xs[0]).backward()
        o_e.step()
    step = GraphedTrainStep(m_g, loss_fn, o_g, xs[0], ys[0], warmup=warm, loss_takes_input=True)
    for x, y in zip(xs, ys):
        o_e.zero_grad(set_to_none=False)
        le = loss_fn(m_e(x), y, x)
        le.backward()
        o_e.step()
        lg = step(x, y)
        assert abs(float(le.detach()) - float(lg)) <= 1e-6 * max(1.0, abs(float(le.detach())))
        del le
    for pe, pg in zip(m_e.parameters(), m_g.parameters()):
        a, b = torch.view_as_real(pe) if pe.is_complex() else pe, torch.view_as_real(pg) if pg.is_complex() else pg
        assert float((a - b).norm() / (a.norm() + 1e-30)) < 1e-6
    # the residual term reached the step: with the data term alone the loss is another number
    with torch.no_grad():
        both = float(loss_fn(m_e(xs[0]), ys[0], xs[0]))
        data = float(loss_fn.terms[0](m_e(xs[0]), ys[0]))
    assert both > data


def test_train_takes_a_loss_that_takes_the_input(gpu_device):
    """train(loss_fn=SumLoss(data + residual)) runs an epoch eagerly and with graph=True and returns finite histories"""
    from models.fno import FNO1d
    from rpde.optim import FlatAdamW
    from train.training import train
    torch.manual_seed(11)
    m0 = FNO1d(1, 1, modes=4, width=8).to(gpu_device)
    g = torch.Generator().manual_seed(5)
    data = [(torch.randn(1, 64, generator=g), torch.randn(1, 64, generator=g)) for _ in range(16)]
    loader = lambda: torch.utils.data.DataLoader(data, batch_size=4, shuffle=False)   # noqa: E731
    for graph in (False, True):
        m = copy.deepcopy(m0)
        loss_fn = _sum_loss()
        loss_fn.warm((64,), gpu_device)
        opt = FlatAdamW(m.parameters(), lr=2e-3, capturable=graph)
        tl, vl = train(m, loader(), loader(), opt, None, epochs=1, device=gpu_device, graph=graph, loss_fn=loss_fn)
        assert len(tl) == 1 and len(vl) == 1 and all(math.isfinite(v) for v in tl + vl)


@pytest.mark.parametrize("graph,use_normalizer", [(False, False), (True, True)])
def test_entry_point_residual_on_generated_ks(gpu_device, tmp_path, capsys, graph, use_normalizer):
    """training.loss=residual trains main_1d on a generated KS set, eagerly and as a hipGraph, with the prediction
    decoded by the loss (use_normalizer false) or by train() (true); the `equation:` block is overridden to the
    arguments the data was generated with, and the reported scores stay relative L2"""
    import json
    from data_generation import ks_1d
    from rpde.entry import run
    flat = str(tmp_path / "flat")
    common = ["--L", "16", "--nt", "11", "--nte", "11", "--et", "0.5", "--batch", "16", "--resolution", "64", "--flat", "--out", flat]
    for split, n in (("train", "16"), ("valid", "8"), ("test", "8")):
        ks_1d.main(common + ["--split", split, "--samples", n])
    l2 = run(1, ["model=fno_1d/fno_1d", "dataset=ks/ks_generated", "dataset.dataset_params.filename=KS_train_16.npz",
                 f"dataset.dataset_params.saved_folder={flat}",
                 "dataset.rollout_steps=4", "dataset.equation.length=16.0", "dataset.equation.interval=0.05",
                 "model.width=16", "model.modes=8", "training.epochs=2", "training.batch_size=16",
                 "training.loss=residual", "training.loss_lambda=0.2", f"training.graph={str(graph).lower()}",
                 f"training.use_normalizer={str(use_normalizer).lower()}", f"checkpoint_dir={tmp_path}"])
    out = capsys.readouterr().out
    rec = [json.loads(ln) for ln in out.splitlines() if '"test_rel_l2"' in ln]
    assert math.isfinite(l2) and 0 < l2 < 2.0 and rec and rec[0]["test_rel_l2"] == l2
    assert math.isfinite(rec[0]["final_train_loss"]) and rec[0]["final_train_loss"] > 0
    # a data set without the block is refused in words
    with pytest.raises(SystemExit, match="equation"):
        run(1, ["model=fno_1d/fno_1d", "dataset=synthetic/ks_512", "dataset.resolutions={64: 16}", "dataset.n_val=8",
                "dataset.n_test=8", "training.loss=residual", f"checkpoint_dir={tmp_path}"])
