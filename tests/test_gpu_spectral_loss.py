"""GPU: the mode-weighted relative L2 loss (csrc/spectral_loss.hip rpde_wrel_l2_* -> rpde.ops.weighted_relative_l2 ->
utils.loss.SpectralRelativeL2Loss) against the float64 restatement of tests/spectral_loss_ref.py.

Tolerances are the project's parity budgets: 1e-5 on the loss (rel-L2 over the per-sample vector), 2e-5 on the gradient
(rel-L2 over the tensor).  The float32 floor of the same restatement on these cases (``floor32``, printed by the parity
test) is at most 9.6e-8 on the loss and 2.1e-7 on the gradient, and 1.1e-6 on both for s = 2 at n = 64."""
import copy
import functools

import pytest
import torch

from tests import spectral_loss_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _inputs(shape, s_err):
    return S.make_inputs(shape, s_err, S.SEED)


@functools.lru_cache(maxsize=None)
def _reference(dims, shape, s, s_err):
    """float64 loss vector and gradient of the mean, and the float32 floor of the restatement: computed once per case"""
    x, y = _inputs(shape, s_err)
    omega = S.sobolev(shape[2:], s)
    r64, g64 = S.loss_and_grad(x, y, omega, dims)
    r32, g32 = S.loss_and_grad(x, y, omega, dims, dtype=torch.float32)
    return r64, g64, (S.rel_l2(r32, r64), S.rel_l2(g32, g64))


@functools.lru_cache(maxsize=None)
def _device(dims, shape, s, s_err):
    """device loss vector (reduction=False) and gradient of the mean through the public loss objects"""
    from utils.loss import SpectralRelativeL2Loss
    x, y = _inputs(shape, s_err)
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV)
    r = SpectralRelativeL2Loss(dims, "sobolev", s=s, reduction=False)(xd, yd).detach().cpu()
    SpectralRelativeL2Loss(dims, "sobolev", s=s)(xd, yd).backward()
    return r, xd.grad.detach().cpu()


@pytest.mark.parametrize("case", S.PARITY, ids=S.case_id)
def test_parity_with_the_float64_restatement(gpu_device, case):
    r64, g64, floor = _reference(*case)
    r, g = _device(*case)
    e = (S.rel_l2(r, r64), S.rel_l2(g, g64))
    print(f"{S.case_id(case)}: device vs float64 loss {e[0]:.2e} gradient {e[1]:.2e}; floor32 {floor[0]:.2e} {floor[1]:.2e}")
    assert r.dtype == torch.float32 and tuple(r.shape) == (case[1][0],) and g.shape == g64.shape
    assert e[0] <= S.LOSS_TOL and e[1] <= S.GRAD_TOL, e


def test_parity_beyond_256_samples(gpu_device):
    """300 samples: the one workgroup of the family's final kernel (csrc/rel_loss.hip) strides over the samples and its
    tree adds threads that hold more than one.  The rel vector, the mean and the gradient of the mean against float64
    under the parity budgets; the float32 floor of the restatement here is 8.3e-8 on the loss, 1.4e-7 on the gradient"""
    from utils.loss import SpectralRelativeL2Loss
    case = (1, (300, 1, 64), 1.0, 1e-2)
    r64, g64, floor = _reference(*case)
    r, g = _device(*case)
    x, y = _inputs(case[1], case[3])
    mean = float(SpectralRelativeL2Loss(1, "sobolev", s=1.0)(x.to(DEV), y.to(DEV)))
    e = (S.rel_l2(r, r64), abs(mean - float(r64.mean())) / float(r64.mean()), S.rel_l2(g, g64))
    print(f"{S.case_id(case)}: device vs float64 loss {e[0]:.2e} mean {e[1]:.2e} gradient {e[2]:.2e}; "
          f"floor32 {floor[0]:.2e} {floor[1]:.2e}")
    assert r.dtype == torch.float32 and tuple(r.shape) == (300,) and g.shape == g64.shape
    assert e[0] <= S.LOSS_TOL and e[1] <= S.LOSS_TOL and e[2] <= S.GRAD_TOL, e


@pytest.mark.parametrize("case", [c for c in S.CASES if c[1][-1] <= 96 and c[2] == 1.0], ids=S.case_id)
def test_unit_weights_are_relative_l2(gpu_device, case):
    """omega == 1: Parseval makes the loss RelativeL2Loss -- against float64 and against the device's own"""
    from utils.loss import RelativeL2Loss, SpectralRelativeL2Loss
    dims, shape, _ = case
    x, y = _inputs(shape, 1e-2)
    ones = torch.ones(shape[-1] // 2 + 1) if dims == 1 else torch.ones(shape[-2], shape[-1] // 2 + 1)
    got, plain = [], []
    for fn, out in ((SpectralRelativeL2Loss(dims, weights=ones, reduction=False), got), (RelativeL2Loss(reduction=False), plain)):
        xd = x.to(DEV).requires_grad_(True)
        r = fn(xd, y.to(DEV))
        r.mean().backward()
        out += [r.detach().cpu(), xd.grad.cpu()]
    x64 = x.double().requires_grad_(True)
    r64 = S.relative_l2(x64, y)
    g64, = torch.autograd.grad(r64.mean(), x64)
    e = (S.rel_l2(got[0], r64.detach()), S.rel_l2(got[1], g64), S.rel_l2(got[0], plain[0]), S.rel_l2(got[1], plain[1]))
    print(f"{S.case_id(case)}: omega = 1 vs float64 rel-L2 {e[0]:.2e} {e[1]:.2e}; vs device RelativeL2Loss {e[2]:.2e} {e[3]:.2e}")
    assert e[0] <= S.LOSS_TOL and e[2] <= S.LOSS_TOL and e[1] <= S.GRAD_TOL and e[3] <= S.GRAD_TOL, e


@pytest.mark.parametrize("case", [c for c in S.CASES if c[2] == 1.0], ids=S.case_id)
def test_the_comparison_sees_a_wrong_answer(gpu_device, case):
    """restatements with multiplicity 2 on DC / Nyquist, or (2-D) an unsigned ky in the weights, miss the device by at
    least 1e-2 = 1000 x the loss tolerance, on the loss and on the gradient"""
    dims, shape, s = case
    x, y = _inputs(shape, 1e-2)
    r, g = _device(dims, shape, s, 1e-2)
    for label, (kw_w, kw_r) in S.wrong_variants(dims).items():
        rw, gw = S.loss_and_grad(x, y, S.sobolev(shape[2:], s, **kw_w), dims, **kw_r)
        miss = (S.rel_l2(rw, r), S.rel_l2(gw, g))
        print(f"{S.case_id(case)}: variant ({label}) misses the device by {miss[0]:.3f} (loss) {miss[1]:.3f} (gradient)")
        assert miss[0] >= 1e-2 and miss[1] >= 1e-2, (label, miss)


@pytest.mark.parametrize("dims,shape", [(1, (5, 2, 48)), (2, (5, 2, 12, 20))])
def test_reductions_and_upstream_gradients(gpu_device, dims, shape):
    """mean, sum, none; none with a non-uniform upstream gradient; an explicit random symmetric table"""
    from utils.loss import SpectralRelativeL2Loss
    x, y = S.make_inputs(shape, 1e-2, 9)
    table = S.symmetric_random_table(shape[2:], 4)
    up = torch.linspace(0.5, 2.0, shape[0])
    for weights, omega in (("sobolev", S.sobolev(shape[2:], 1.0)), (table, table)):
        for kw in (dict(size_average=True), dict(size_average=False), dict(reduction=False), dict(reduction=False, upstream=up)):
            ctor = {k: v for k, v in kw.items() if k != "upstream"}
            xd = x.to(DEV).requires_grad_(True)
            out = SpectralRelativeL2Loss(dims, weights=weights, **ctor)(xd, y.to(DEV))
            r64, g64 = S.loss_and_grad(x, y, omega, dims, **kw)
            want = S.reduce(r64, **ctor)
            assert out.shape == want.shape and out.dtype == torch.float32
            if out.dim():
                out.backward(kw.get("upstream", torch.ones(shape[0])).to(DEV))
            else:
                out.backward()
            e = (S.rel_l2(out.detach().cpu().reshape(-1), want.reshape(-1)), S.rel_l2(xd.grad.cpu(), g64))
            assert e[0] <= S.LOSS_TOL and e[1] <= S.GRAD_TOL, (kw, e)


@pytest.mark.parametrize("dims,shape", [(1, (3, 2, 64)), (2, (3, 1, 16, 24))])
def test_edge_cases_stay_finite(gpu_device, dims, shape):
    """a sample with x = y: loss 0, gradient 0; a zero target: finite (the fixture loss_none_zero_target's case)"""
    from utils.loss import SpectralRelativeL2Loss
    x, y = S.make_inputs(shape, 1e-2, 2)
    x[1] = y[1]
    fn = SpectralRelativeL2Loss(dims, reduction=False)
    xd = x.to(DEV).requires_grad_(True)
    r = fn(xd, y.to(DEV))
    r.sum().backward()
    r, g = r.detach().cpu(), xd.grad.cpu()
    r64 = S.rel(x, y, S.sobolev(shape[2:]), dims)
    assert float(r[1]) == 0.0 and bool((g[1] == 0).all()) and bool(torch.isfinite(r).all()) and bool(torch.isfinite(g).all())
    assert S.rel_l2(r, r64) <= S.LOSS_TOL
    keep = [0, 2]
    g64 = S.closed_form_grad(x[keep], y[keep], S.sobolev(shape[2:]), dims, torch.ones(2))
    assert S.rel_l2(g[keep], g64) <= S.GRAD_TOL
    # zero target: rel = sqrt(E_d) / 1e-8, large and finite; the gradient too
    y0 = torch.zeros_like(y)
    xd = x.to(DEV).requires_grad_(True)
    r = fn(xd, y0.to(DEV))
    r.mean().backward()
    r64, g64 = S.loss_and_grad(x, y0, S.sobolev(shape[2:]), dims)
    assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(xd.grad).all())
    assert S.rel_l2(r.detach().cpu(), r64) <= S.LOSS_TOL and S.rel_l2(xd.grad.cpu(), g64) <= S.GRAD_TOL


def test_identical_calls_give_identical_bits(gpu_device):
    from utils.loss import SpectralRelativeL2Loss
    outs = []
    for dims, shape in ((1, (3, 2, 96)), (2, (4, 1, 64, 64))):
        x, y = S.make_inputs(shape, 1e-2, 7)
        for _ in range(2):
            xd = x.to(DEV).requires_grad_(True)
            loss = SpectralRelativeL2Loss(dims)(xd, y.to(DEV))
            loss.backward()
            outs.append((loss.detach().cpu(), xd.grad.cpu()))
        (l0, g0), (l1, g1) = outs[-2:]
        assert torch.equal(l0, l1) and torch.equal(g0, g1)


def test_one_object_serves_several_grids(gpu_device):
    """one loss object called at 32^2, 64^2 and 32^2 again gives what fresh objects give; an explicit table serves one
    grid and raises on another"""
    from utils.loss import SpectralRelativeL2Loss
    shared = SpectralRelativeL2Loss(2, reduction=False)
    for n in (32, 64, 32):
        x, y = S.make_inputs((2, 1, n, n), 1e-2, n)
        res = []
        for fn in (shared, SpectralRelativeL2Loss(2, reduction=False)):
            xd = x.to(DEV).requires_grad_(True)
            r = fn(xd, y.to(DEV))
            r.sum().backward()
            res.append((r.detach().cpu(), xd.grad.cpu()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert len(shared._tables) == 2
    fixed = SpectralRelativeL2Loss(2, weights=S.symmetric_random_table((32, 32), 1))
    x, y = S.make_inputs((2, 1, 32, 32), 1e-2, 1)
    fixed(x.to(DEV), y.to(DEV))
    with pytest.raises(ValueError):
        fixed(torch.zeros(2, 1, 16, 16, device=DEV), torch.ones(2, 1, 16, 16, device=DEV))


def test_graphed_step_matches_eager(gpu_device):
    """a tiny FNO1d trained on the H^1 loss: four eager steps against four replays of rpde.graph.GraphedTrainStep,
    after warm(); the bounds of test_graphed_train_step_matches_eager"""
    from models.fno import FNO1d
    from rpde.graph import GraphedTrainStep
    from rpde.optim import FlatAdamW
    from utils.loss import SpectralRelativeL2Loss
    torch.manual_seed(3)
    m_e = FNO1d(1, 1, modes=8, width=16).to(gpu_device).train()
    m_g = copy.deepcopy(m_e)
    xs = [torch.randn(4, 1, 64, device=gpu_device) for _ in range(4)]
    ys = [torch.randn(4, 1, 64, device=gpu_device) for _ in range(4)]
    loss_fn = SpectralRelativeL2Loss(1, "sobolev", s=1.0)
    loss_fn.warm((64,), gpu_device)
    o_e = FlatAdamW(m_e.parameters(), lr=1e-3, capturable=True)
    o_g = FlatAdamW(m_g.parameters(), lr=1e-3, capturable=True)
    warm = 2
    for _ in range(warm):
        o_e.zero_grad(set_to_none=False)
        loss_fn(m_e(xs[0]), ys[0]).backward()
        o_e.step()
    step = GraphedTrainStep(m_g, loss_fn, o_g, xs[0], ys[0], warmup=warm)
    for x, y in zip(xs, ys):
        o_e.zero_grad(set_to_none=False)
        le = loss_fn(m_e(x), y)
        le.backward()
        o_e.step()
        lg = step(x, y)
        assert abs(float(le.detach()) - float(lg)) <= 1e-6 * max(1.0, abs(float(le.detach())))
        del le
    for pe, pg in zip(m_e.parameters(), m_g.parameters()):
        a, b = torch.view_as_real(pe) if pe.is_complex() else pe, torch.view_as_real(pg) if pg.is_complex() else pg
        assert float((a - b).norm() / (a.norm() + 1e-30)) < 1e-6


def test_train_takes_a_loss(gpu_device):
    """train(loss_fn=SpectralRelativeL2Loss(...), graph=True) runs and returns finite histories (the validation history
    stays plain relative L2); train(loss_fn=RelativeL2Loss()) is train() with the default"""
    import math
    from models.fno import FNO1d
    from rpde.optim import FlatAdamW
    from train.training import train
    from utils.loss import RelativeL2Loss, SpectralRelativeL2Loss
    torch.manual_seed(11)
    m0 = FNO1d(1, 1, modes=8, width=16).to(gpu_device)
    g = torch.Generator().manual_seed(5)
    data = [(torch.randn(1, 64, generator=g), torch.randn(1, 64, generator=g)) for _ in range(16)]
    loader = lambda: torch.utils.data.DataLoader(data, batch_size=4, shuffle=False)   # noqa: E731

    def run(graph, **kw):
        m = copy.deepcopy(m0)
        opt = FlatAdamW(m.parameters(), lr=2e-3, capturable=graph)
        hist = train(m, loader(), loader(), opt, None, epochs=2, device=gpu_device, graph=graph, **kw)
        return m, hist

    h1 = SpectralRelativeL2Loss(1, "sobolev", s=1.0)
    h1.warm((64,), gpu_device)
    m_s, (tl, vl) = run(True, loss_fn=h1)
    assert len(tl) == 2 and len(vl) == 2 and all(math.isfinite(v) for v in tl + vl)
    m_d, hist_d = run(False)
    m_p, hist_p = run(False, loss_fn=RelativeL2Loss())
    assert hist_d == hist_p
    for a, b in zip(m_d.parameters(), m_p.parameters()):
        assert torch.equal(a, b)
    # the objective really was another one: the H^1 run's weights differ, its validation metric is the same quantity
    assert any(not torch.equal(a, b) for a, b in zip(m_d.parameters(), m_s.parameters()))
    with torch.no_grad():
        xb = torch.stack([d[0] for d in data]).to(gpu_device)
        yb = torch.stack([d[1] for d in data]).to(gpu_device)
        plain = float(RelativeL2Loss()(m_s.eval()(xb), yb))
    assert abs(plain - vl[-1]) <= 1e-5 * max(1.0, plain)


def test_entry_point_override(gpu_device, tmp_path, capsys):
    """training.loss=sobolev (with training.loss_s / training.loss_length) trains main_1d on the H^s loss; the reported
    scores stay relative L2; an unknown name is refused"""
    import json
    from rpde.entry import run
    base = ["model=fno_1d/fno_1d", "dataset=synthetic/ks_512", "dataset.resolutions={64: 16}", "dataset.n_val=8",
            "dataset.n_test=8", "training.epochs=2", "training.batch_size=8", "model.width=16", "model.modes=8",
            f"checkpoint_dir={tmp_path}"]
    l2 = run(1, base + ["training.loss=sobolev", "training.loss_s=0.5", "training.loss_length=2.0"])
    out = capsys.readouterr().out
    rec = [json.loads(ln) for ln in out.splitlines() if '"test_rel_l2"' in ln]
    assert l2 == l2 and 0 < l2 < 2.0 and rec and rec[0]["test_rel_l2"] == l2
    assert rec[0]["final_train_loss"] == rec[0]["final_train_loss"] and rec[0]["final_train_loss"] > 0
    with pytest.raises(SystemExit):
        run(1, base + ["training.loss=h7"])
