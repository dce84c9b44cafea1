"""GPU: the optimizer state a captured training step reads from the device.  FlatAdamW(capturable=True) keeps step,
lr and weight decay in ``_step_dev``; a replayed step reads whatever lr / weight decay the device holds at that
moment.  Every step here -- eager or replayed, direct or inside train() -- is checked against one float64 AdamW step
(oracle/adamw.py) from the fp32 state the kernel started from, at the host's lr / weight decay of that moment, and the
device words are checked against the host values after it.  The scenarios are the ways the device can fall behind the
host: a capture right after a scheduler step, an lr value that comes back after another writer moved the device, and
load_state_dict under a live graph."""
import contextlib
import copy
import functools
import math

import numpy as np
import pytest
import torch

from oracle.adamw import adamw_step_f64

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
LR, WD = 1e-3, 1e-2


def _real(t):
    return torch.view_as_real(t) if t.is_complex() else t


def _flat64(tensors):
    """one float64 CPU vector of all tensors (complex as (re, im) pairs), in one device-to-host copy"""
    return torch.cat([_real(t.detach()).reshape(-1) for t in tensors]).double().cpu()


class AdamWChecker:
    """Per-step check of a FlatAdamW(capturable=True):  ``with chk.step(): <one optimizer step>``.

    Before the step: every parameter, exp_avg and exp_avg_sq (views into the optimizer's flat buffers) as float64, and
    the group's lr / weight decay.  After it: the gradients the step left in the bucket, then the new p, m, v against
    adamw_step_f64 at the test's own step count ``t``.  The betas are the fp32 values the kernel receives.  Elementwise
    tolerances: a few fp32 ulps of the values, plus 1e-5 of the reference update |dp| and a floor of 1e-6 lr for
    elements whose first moment cancels.  Every check also proves it could see a wrong rate: the same step at half or
    twice the lr, or at lr 0, and any ``distinct`` (lr, wd) pairs, must miss the tolerance by at least 100x.  lr 0
    must leave the parameters bit for bit unchanged."""

    def __init__(self, opt, t: int = 0):
        self.opt, self.t = opt, t
        self.params = opt.bucket.params
        g = opt.param_groups[0]
        self.betas = tuple(float(np.float32(b)) for b in g["betas"])
        self.eps = float(g["eps"])
        self.worst = 0.0                 # largest err / tol over the checked steps
        self.margin = math.inf           # smallest (wrong step's err) / tol
        self.n = 0

    @contextlib.contextmanager
    def step(self, distinct=()):
        g = self.opt.param_groups[0]
        lr, wd = float(g["lr"]), float(g["weight_decay"])
        st = self.opt.state
        p0 = _flat64(self.params)
        m0 = _flat64([st[p]["exp_avg"] for p in self.params])
        v0 = _flat64([st[p]["exp_avg_sq"] for p in self.params])
        yield
        torch.cuda.synchronize()
        self.t += 1
        self.n += 1
        t = self.t
        where = f"step {t} at lr={lr:g}, wd={wd:g}"
        dev = self.opt._step_dev.cpu()
        want = torch.tensor([lr, wd], dtype=torch.float32)
        assert torch.equal(dev[3:5], want), f"{where}: the device holds lr / wd {dev[3:5].tolist()}, the host {want.tolist()}"
        assert float(dev[0]) == float(t), f"{where}: device step counter {float(dev[0])}, expected {t}"
        grad = torch.cat([_real(v).reshape(-1) for v in self.opt.bucket._views]).double().cpu()
        p1 = _flat64(self.params)
        m1 = _flat64([st[p]["exp_avg"] for p in self.params])
        v1 = _flat64([st[p]["exp_avg_sq"] for p in self.params])
        pr, mr, vr = adamw_step_f64(p0, grad, m0, v0, t, lr, wd, self.betas, self.eps)
        b2 = self.betas[1]
        tol_p = 4 * EPS32 * torch.maximum(p0.abs(), pr.abs()) + 1e-5 * (pr - p0).abs() + 1e-6 * lr + 1e-30
        tol_m = 4 * EPS32 * (m0.abs() + grad.abs()) + 1e-30
        tol_v = 4 * EPS32 * (v0.abs() + (1.0 - b2) * grad * grad) + 1e-30
        for name, got, ref, tol in (("p", p1, pr, tol_p), ("exp_avg", m1, mr, tol_m), ("exp_avg_sq", v1, vr, tol_v)):
            ratio = (got - ref).abs() / tol
            k = int(ratio.argmax())
            assert float(ratio[k]) <= 1.0, (f"{where}: {name}[{k}] = {float(got[k])!r}, float64 AdamW step "
                                            f"{float(ref[k])!r} (err / tol = {float(ratio[k]):.3g})")
            self.worst = max(self.worst, float(ratio[k]))
        if lr == 0.0:
            assert torch.equal(p1, p0), f"{where}: lr 0 moved the parameters"
        wrong = [(lr * 0.5, wd), (lr * 2.0, wd), (0.0, wd)] if lr > 0.0 else []
        for lw, ww in wrong + list(distinct):
            pw, _, _ = adamw_step_f64(p0, grad, m0, v0, t, lw, ww, self.betas, self.eps)
            sep = float(((p1 - pw).abs() / tol_p).max())
            assert sep >= 100.0, f"{where}: a step at lr={lw:g}, wd={ww:g} is only {sep:.3g}x the tolerance away"
            self.margin = min(self.margin, sep)

    def report(self, name):
        print(f"[adamw-check] {name}: {self.n} steps, worst err/tol {self.worst:.3g}, "
              f"smallest wrong-step separation {self.margin:.3g}x")


def _model(dev, seed=0):
    """FNO1d width 16 (the graph tests' model) with every parameter ~ N(0, 0.1^2): dp ~ lr is far above one ulp"""
    from models.fno import FNO1d
    torch.manual_seed(seed)
    m = FNO1d(1, 1, modes=8, width=16).to(dev).train()
    with torch.no_grad():
        for p in m.parameters():
            r = _real(p)
            r.copy_(torch.randn_like(r) * 0.1)
    return m


def _opt(model, capturable=True, lr=LR, wd=WD):
    from rpde.optim import FlatAdamW
    return FlatAdamW(model.parameters(), lr=lr, weight_decay=wd, capturable=capturable)


def _batch(dev, b, seed, n=128):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, 1, n, generator=g).to(dev), torch.randn(b, 1, n, generator=g).to(dev)


def _loss_fn():
    from utils.loss import RelativeL2Loss
    return RelativeL2Loss(size_average=True)


def _eager_step(model, opt, x, y):
    """one eager step; nothing of its autograd graph outlives it (a capture may follow)"""
    opt.zero_grad()
    _loss_fn()(model(x), y).backward()
    opt.step()


def _graphed(model, opt, x, y):
    from rpde.graph import GraphedTrainStep
    return GraphedTrainStep(model, _loss_fn(), opt, x, y, warmup=0)


def _set(opt, lr=None, wd=None):
    if lr is not None:
        opt.param_groups[0]["lr"] = lr
    if wd is not None:
        opt.param_groups[0]["weight_decay"] = wd


def test_capture_right_after_a_scheduler_step(gpu_device):
    """a: the last eager step ran at the old lr / wd, the scheduler moved them, then the capture -- the replays must
    train at the new values, not at what the eager step left on the device"""
    model = _model(gpu_device)
    opt = _opt(model)
    chk = AdamWChecker(opt)
    x, y = _batch(gpu_device, 4, 1)
    for _ in range(2):
        with chk.step():
            _eager_step(model, opt, x, y)
    _set(opt, lr=LR * 0.5, wd=3e-2)                     # what a scheduler does at the end of an epoch
    step = _graphed(model, opt, x, y)
    for i in range(3):
        xi, yi = _batch(gpu_device, 4, 10 + i)
        with chk.step(distinct=[(LR, WD)]):          # the values the last eager step left behind
            step(xi, yi)
    assert [int(float(s["step"])) for s in opt.state_dict()["state"].values()] == [chk.t] * len(chk.params)
    chk.report("capture after scheduler step")


@pytest.mark.parametrize("other", ["instance", "eager"])
def test_lr_that_comes_back_after_another_writer(gpu_device, other):
    """c: instance A captured at lr a; something A never sees -- a second GraphedTrainStep on the same optimizer, or an
    eager step of a shape with no graph -- writes lr b to the device; the host returns to a: A must not replay at b"""
    a, b = LR, 2.5e-3
    model = _model(gpu_device)
    opt = _opt(model)
    chk = AdamWChecker(opt)
    xa, ya = _batch(gpu_device, 4, 1)
    xb, yb = _batch(gpu_device, 2, 2)                     # the other batch shape (a ragged tail)
    for x, y in ((xa, ya), (xa, ya), (xb, yb), (xb, yb)):
        with chk.step():
            _eager_step(model, opt, x, y)
    step_a = _graphed(model, opt, xa, ya)
    step_b = _graphed(model, opt, xb, yb) if other == "instance" else None
    with chk.step():
        step_a(xa, ya)
    _set(opt, lr=b)
    if other == "instance":
        with chk.step():
            step_a(xa, ya)
        _set(opt, lr=a)
        with chk.step(distinct=[(b, WD)]):
            step_b(xb, yb)                                # B was captured at a and last saw a
        with chk.step():
            step_b(xb, yb)
        _set(opt, lr=b)
        with chk.step():
            step_b(xb, yb)
        _set(opt, lr=a)
        with chk.step(distinct=[(b, WD)]):
            step_a(xa, ya)
    else:
        with chk.step():
            _eager_step(model, opt, xb, yb)              # writes b to the device outside any graph
        _set(opt, lr=a)
        with chk.step(distinct=[(b, WD)]):
            step_a(xa, ya)
        with chk.step():
            step_a(xa, ya)
    chk.report(f"lr comes back ({other})")


@pytest.mark.parametrize("lr_moves_after_save", [False, True])
def test_load_state_dict_under_a_live_graph(gpu_device, lr_moves_after_save):
    """d: capture, replay, save; more replays (at the same or at another lr); load the saved state and replay: the
    replays continue from the saved step with the saved lr / weight decay -- not with the zeros load_state_dict
    puts into the device state"""
    model = _model(gpu_device)
    opt = _opt(model)
    chk = AdamWChecker(opt)
    x, y = _batch(gpu_device, 4, 1)
    for _ in range(2):
        with chk.step():
            _eager_step(model, opt, x, y)
    step = _graphed(model, opt, x, y)
    for i in range(2):
        with chk.step():
            step(*_batch(gpu_device, 4, 10 + i))
    sd = copy.deepcopy(opt.state_dict())
    assert [int(float(s["step"])) for s in sd["state"].values()] == [chk.t] * len(chk.params)
    saved_p = [p.detach().clone() for p in model.parameters()]
    t_saved = chk.t
    if lr_moves_after_save:
        _set(opt, lr=4e-3, wd=0.1)
    for i in range(2):
        with chk.step():
            step(*_batch(gpu_device, 4, 20 + i))
    assert [int(float(s["step"])) for s in opt.state_dict()["state"].values()] == [chk.t] * len(chk.params)
    with torch.no_grad():
        for p, s in zip(model.parameters(), saved_p):
            p.copy_(s)
    opt.load_state_dict(copy.deepcopy(sd))
    chk.t = t_saved
    g = opt.param_groups[0]
    assert (g["lr"], g["weight_decay"]) == (LR, WD)
    for i, p in enumerate(chk.params):
        assert torch.equal(opt.state[p]["exp_avg"], sd["state"][i]["exp_avg"])
        assert torch.equal(opt.state[p]["exp_avg_sq"], sd["state"][i]["exp_avg_sq"])
    for i in range(2):
        with chk.step(distinct=[(4e-3, 0.1)] if lr_moves_after_save else ()):
            step(*_batch(gpu_device, 4, 30 + i))
    assert [int(float(s["step"])) for s in opt.state_dict()["state"].values()] == [chk.t] * len(chk.params)
    chk.report(f"load_state_dict (lr moves after save: {lr_moves_after_save})")


def test_weight_decay_alone_and_zero_lr(gpu_device):
    """f: weight decay moving alone changes the update by the decay factor only; lr 0 leaves the parameters exactly
    as they were (decoupled decay is lr * wd) while the moments and the step count advance"""
    model = _model(gpu_device)
    opt = _opt(model)
    chk = AdamWChecker(opt)
    x, y = _batch(gpu_device, 4, 1)
    for _ in range(2):
        with chk.step():
            _eager_step(model, opt, x, y)
    step = _graphed(model, opt, x, y)
    with chk.step():
        step(x, y)
    _set(opt, wd=0.5)
    with chk.step(distinct=[(LR, WD)]):
        step(x, y)
    _set(opt, lr=0.0)
    with chk.step(distinct=[(LR, 0.5)]):
        step(x, y)
    _set(opt, wd=0.0)
    with chk.step(distinct=[(LR, 0.5)]):
        step(x, y)
    _set(opt, lr=LR)
    with chk.step(distinct=[(LR, 0.5), (0.0, 0.0)]):
        step(x, y)
    _set(opt, lr=0.0, wd=0.5)
    with chk.step(distinct=[(LR, 0.5)]):                  # the eager kernel at lr 0, too
        _eager_step(model, opt, x, y)
    chk.report("weight decay alone / lr 0")


# ---- through train(graph=True): every step of both loops checked ---------------------------------------------------

def _watch(monkeypatch, opt, chk):
    """route every eager optimizer step and every GraphedTrainStep replay of `opt` through `chk` (a step that is being
    captured executes nothing and is not checked)"""
    from rpde.graph import GraphedTrainStep
    inner = opt.step

    @functools.wraps(inner)              # (keeps the lr scheduler's mark: it still counts the steps)
    def step(*args, **kwargs):
        if torch.cuda.is_current_stream_capturing():
            return inner(*args, **kwargs)
        with chk.step():
            return inner(*args, **kwargs)
    monkeypatch.setattr(opt, "step", step)
    call = GraphedTrainStep.__call__

    def replay(self, x, y):
        if self.optimizer is not opt:
            return call(self, x, y)
        with chk.step():
            return call(self, x, y)
    monkeypatch.setattr(GraphedTrainStep, "__call__", replay)


def _batches(shapes, seed):
    """a re-iterable loader: a list of CPU (x, y) batches with the given batch sizes, in this order"""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(b, 1, 128, generator=g), torch.randn(b, 1, 128, generator=g)) for b in shapes]


def _flat_params(model):
    return torch.cat([_real(p.detach()).reshape(-1) for p in model.parameters()])


def _train_both(monkeypatch, gpu_device, loader, make_sched, epochs, lr=2e-3):
    """train(graph=False) and train(graph=True) from the same weights, each step checked; -> per run (losses, model,
    optimizer, lr after each epoch)"""
    from train.training import train
    base = _model(gpu_device, seed=11)
    val = _batches([4, 4], 99)
    out = []
    for graph in (False, True):
        m = copy.deepcopy(base)
        opt = _opt(m, lr=lr)
        sched = make_sched(opt)
        chk = AdamWChecker(opt)
        with monkeypatch.context() as mp:
            _watch(mp, opt, chk)
            lrs = []
            hist = train(m, loader, val, opt, sched, epochs=epochs, device=gpu_device, graph=graph,
                         log=lambda rec, o=opt: lrs.append(o.param_groups[0]["lr"]))
        chk.report(f"train(graph={graph})")
        assert chk.n == epochs * len(loader)
        out.append((hist, m, lrs))
    (tl_e, vl_e), m_e, lrs_e = out[0][0], out[0][1], out[0][2]
    (tl_g, vl_g), m_g, lrs_g = out[1][0], out[1][1], out[1][2]
    assert lrs_e == lrs_g
    for a, b in zip(tl_e + vl_e, tl_g + vl_g):
        assert abs(a - b) <= 2e-6 * max(1.0, abs(a)), (tl_e, tl_g, vl_e, vl_g)
    for pe, pg in zip(m_e.parameters(), m_g.parameters()):
        a, b = _real(pe.detach()), _real(pg.detach())
        assert float((a - b).norm() / (a.norm() + 1e-30)) < 2e-6
    return base, m_e, lrs_e


@pytest.mark.parametrize("shapes", [[4, 4], [2, 4, 4]], ids=["graph_after_batches", "ragged_tail_first"])
def test_train_graph_capture_first_in_an_epoch_follows_step_lr(gpu_device, monkeypatch, shapes):
    """b: a batch shape with exactly GRAPH_AFTER batches per epoch is captured as the first step after a scheduler step;
    with a ragged tail drawn first, the tail's capture is.  StepLR(gamma 0.5) over 4 epochs: same losses and weights as
    the eager loop, every step at the scheduled rate"""
    from train.training import GRAPH_AFTER, train
    assert shapes.count(4) == GRAPH_AFTER
    loader = _batches(shapes, 5)
    step_lr = lambda o: torch.optim.lr_scheduler.StepLR(o, step_size=1, gamma=0.5)     # noqa: E731
    base, m_e, lrs = _train_both(monkeypatch, gpu_device, loader, step_lr, epochs=4)
    assert lrs == [2e-3 * 0.5 ** (k + 1) for k in range(4)]
    # an epoch at the previous epoch's rate -- what a stale replay does -- moves the weights far beyond the tolerance
    m_w = copy.deepcopy(base)
    opt = _opt(m_w, capturable=False, lr=2e-3)
    stale = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: (1.0, 1.0, 0.25, 0.125)[min(e, 3)])
    train(m_w, loader, _batches([4, 4], 99), opt, stale, epochs=4, device=gpu_device, graph=False)
    pe, pw = _flat_params(m_e), _flat_params(m_w)
    assert float((pe - pw).norm() / pe.norm()) > 1e-4


def test_train_graph_follows_reduce_lr_on_plateau(gpu_device, monkeypatch):
    """e: ReduceLROnPlateau moves lr only on a plateau (train() passes it the validation loss).  threshold 0.999 makes
    every epoch after the first a plateau, min_lr stops at one reduction (after epoch 1); the ragged tail, drawn first,
    is captured as the first step of epoch 2"""
    loader = _batches([2, 4, 4, 4], 6)
    plateau = lambda o: torch.optim.lr_scheduler.ReduceLROnPlateau(o, factor=0.5, patience=0, threshold=0.999,   # noqa: E731
                                                                   min_lr=1e-3)
    _, _, lrs = _train_both(monkeypatch, gpu_device, loader, plateau, epochs=4)
    assert lrs == [2e-3, 1e-3, 1e-3, 1e-3]
