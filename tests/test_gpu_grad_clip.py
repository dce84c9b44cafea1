"""GPU: device-side gradient-norm clipping and non-finite step skipping of rpde.optim.FlatAdamW (csrc/adamw_clip.hip).

The norm kernel alone is held to float64 of the same bytes.  Every optimizer step -- eager with host scalars, eager
with the device-side step state, replayed from a hipGraph, inside train() -- is checked from the fp32 state it started
from against one float64 AdamW step (oracle/adamw.py) fed ``scale64 * g``: g the (unclipped) gradient the step left in
the bucket, scale64 the float64 restatement of torch's rule (tests/clip_ref.py) on exactly that gradient.

Tolerances are tests/test_gpu_optimizer_state.py's (AdamWChecker), elementwise, with every term in |g| taken at
|scale g|, plus the error of the fp32 scale: the norm is rounded to fp32 once (2^-24), then one add, one quotient and
one product of half an ulp each -- 2 EPS32 relative on scale*g in all.  exp_avg sees it as 2 EPS32 |scale g|,
exp_avg_sq through g^2 as 2 (1 - b2) |scale g| * 2 EPS32 |scale g|; in p the scale error rides inside m / sqrt(v),
far below the 1e-5 |dp| term the parameter tolerance already has.  A check that could not see a wrong scale proves
nothing, so wherever the scale is below 1 the same step at scale 1 must miss these tolerances by 100x."""
import copy
import math

import numpy as np
import pytest
import torch

from oracle.adamw import adamw_step_f64
from tests.clip_ref import clip_scale_f64, total_norm_f64

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
LR, WD = 1e-3, 1e-2
NORM_RTOL = 2.0 ** -22        # float64 sum, one square root, one rounding to fp32: derived, not measured


def _real(t):
    return torch.view_as_real(t) if t.is_complex() else t


def _flat64(tensors):
    return torch.cat([_real(t.detach()).reshape(-1) for t in tensors]).double().cpu()


# ---- the norm kernel alone ---------------------------------------------------------------------------------------------

def _sweep_floats():
    """floats in one full sweep of the norm kernel's largest grid (256 threads, one float4 each)"""
    from rpde import _lib
    blocks = _lib.load().rpde_grad_norm_ws_bytes(1 << 40) // 8
    return blocks * 256 * 4


def _values(kind, n):
    g = torch.Generator().manual_seed(n)
    if kind == "normal":
        return torch.randn(n, generator=g)
    if kind == "big":                       # fp32 squares overflow
        return torch.full((n,), 1e25) * torch.sign(torch.randn(n, generator=g))
    if kind == "tiny":                      # fp32 squares vanish
        return torch.full((n,), 1e-30)
    x = torch.full((n,), 1e-4)              # an outlier that swamps an fp32 sum
    x[n // 3] = 1e8
    return x


def _grad_norm(g, max_norm=0.0, skip=0, clip=None):
    """-> (record, partial sums) of one rpde_grad_norm call on the device tensor g"""
    from rpde import _lib
    lib = _lib.load()
    ws = torch.zeros(lib.rpde_grad_norm_ws_bytes(g.numel()) // 8, dtype=torch.float64, device=g.device)
    if clip is None:
        clip = torch.zeros(8, dtype=torch.float32, device=g.device)
    _lib.check(lib.rpde_grad_norm(g.data_ptr(), g.numel(), max_norm, skip, clip.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                  _lib.stream_ptr()), "grad_norm")
    torch.cuda.synchronize()
    return clip, ws


@pytest.mark.parametrize("kind", ["normal", "big", "tiny", "outlier"])
@pytest.mark.parametrize("n", [4, 252, 1028, "sweep+4"])
def test_norm_kernel_against_float64_of_the_same_bytes(gpu_device, kind, n):
    n = _sweep_floats() + 4 if n == "sweep+4" else n
    host = _values(kind, n)
    g = host.to(gpu_device)
    ref = math.sqrt(float((host.double() ** 2).sum()))
    assert 0.0 < ref < 3e38
    clip, ws = _grad_norm(g)
    got = float(clip[0])
    print(f"[grad-norm] {kind} n={n}: {got!r} vs float64 {ref!r}, relative error {abs(got - ref) / ref:.3g}")
    assert abs(got - ref) <= NORM_RTOL * ref
    assert clip.tolist()[1:] == [1.0, 0.0, 1.0, 0.0, 0.0, got, got]          # measure only: scale 1, one step seen
    clip2, ws2 = _grad_norm(g)
    assert torch.equal(clip.view(torch.int32), clip2.view(torch.int32))      # identical calls, identical bits
    assert torch.equal(ws.view(torch.int64), ws2.view(torch.int64))


def test_norm_record_scale_counters_and_nonfinite(gpu_device):
    """the finalise kernel's rule and book-keeping on hand-made gradients: norm exactly 10"""
    g = torch.zeros(1028, device=gpu_device)
    g[5], g[1027] = 6.0, -8.0
    clip, _ = _grad_norm(g, max_norm=20.0)
    assert clip.tolist() == [10.0, 1.0, 0.0, 1.0, 0.0, 0.0, 10.0, 10.0]
    clip, _ = _grad_norm(g, max_norm=2.5, clip=clip)
    want = float(np.float32(2.5) / (np.float32(10.0) + np.float32(1e-6)))
    assert clip.tolist() == [10.0, want, 0.0, 2.0, 1.0, 0.0, 10.0, 20.0]
    clip, _ = _grad_norm(g * 0.0, max_norm=2.5, clip=clip)                   # all-zero gradient: scale 1, not 2.5e6
    assert clip.tolist() == [0.0, 1.0, 0.0, 3.0, 1.0, 0.0, 10.0, 20.0]
    clip, _ = _grad_norm(g, max_norm=float("inf"), clip=clip)                # +inf: measure only
    assert clip.tolist()[:5] == [10.0, 1.0, 0.0, 4.0, 1.0]
    for bad, scale_is in ((float("inf"), lambda s: s == 0.0), (float("nan"), math.isnan)):
        gb = g.clone()
        gb[100] = bad
        for skip in (0, 1):
            c, _ = _grad_norm(gb, max_norm=2.5, skip=skip)
            c = c.tolist()
            assert (math.isnan(c[0]) if math.isnan(bad) else c[0] == bad) and scale_is(c[1])      # NaN is not clamped to 1
            # a non-finite norm enters neither the maximum nor the sum; an unskipped scale 0 counts as clipped
            assert c[2:] == [float(skip), 1.0, 0.0 if (skip or math.isnan(bad)) else 1.0, float(skip), 0.0, 0.0]
        c, _ = _grad_norm(gb, max_norm=0.0, skip=1)                          # measure only still skips
        assert c.tolist()[1:6] == [1.0, 1.0, 1.0, 0.0, 1.0]


# ---- steps against the float64 oracle ----------------------------------------------------------------------------------

class ClipChecker:
    """``chk.step(run)``: one optimizer step of ``opt`` through ``run()``, checked as the module docstring says.
    -> (norm64, scale64) of the step's gradient"""

    def __init__(self, opt, t=0):
        self.opt, self.t = opt, t
        self.params = opt.bucket.params
        g = opt.param_groups[0]
        # the betas each path implements: the device-state step receives them as fp32 and forms 1 - b there; the
        # host-scalar step forms 1 - b and the bias corrections in double on the host and rounds each scalar once
        self.betas = tuple(float(np.float32(b)) if opt._step_dev is not None else float(b) for b in g["betas"])
        self.eps = float(g["eps"])
        self.worst, self.margin = 0.0, math.inf
        self.scales = []

    def state(self):
        st = self.opt.state
        return (_flat64(self.params), _flat64([st[p]["exp_avg"] for p in self.params]),
                _flat64([st[p]["exp_avg_sq"] for p in self.params]))

    def step(self, run, idle=()):
        """idle: indices of parameters that get no gradient in this step (capturable=False): they must not move, and
        the float64 step is not asked about them"""
        g = self.opt.param_groups[0]
        lr, wd = float(g["lr"]), float(g["weight_decay"])
        p0, m0, v0 = self.state()
        run()
        torch.cuda.synchronize()
        self.t += 1
        t = self.t
        grad = _flat64(self.opt.bucket._views)                 # the bucket keeps the UNCLIPPED gradient
        norm64 = total_norm_f64([grad])
        scale64 = clip_scale_f64(norm64, self.opt.max_grad_norm)
        where = f"step {t} (norm {norm64:.6g}, scale {scale64:.6g})"
        rec = self.opt.grad_stats().tolist()
        assert abs(rec[0] - norm64) <= NORM_RTOL * norm64, f"{where}: device norm {rec[0]!r}"
        assert abs(rec[1] - scale64) <= 2 * EPS32 * scale64, f"{where}: device scale {rec[1]!r}"
        assert (rec[1] == 1.0) == (scale64 == 1.0) and rec[2] == 0.0
        if self.opt._step_dev is not None:
            assert float(self.opt._step_dev[0]) == float(t), f"{where}: device step counter {float(self.opt._step_dev[0])}"
        sg = scale64 * grad
        b2 = self.betas[1]
        p1, m1, v1 = self.state()
        live = torch.cat([torch.full((_real(p).numel(),), i not in idle) for i, p in enumerate(self.params)])
        for a0, a1 in ((p0, p1), (m0, m1), (v0, v1)):
            assert torch.equal(a0[~live], a1[~live]), f"{where}: a parameter without a gradient moved"
        assert not bool(grad[~live].any())
        p0, m0, v0, p1, m1, v1, grad, sg = (a[live] for a in (p0, m0, v0, p1, m1, v1, grad, sg))
        pr, mr, vr = adamw_step_f64(p0, sg, m0, v0, t, lr, wd, self.betas, self.eps)
        tol_p = 4 * EPS32 * torch.maximum(p0.abs(), pr.abs()) + 1e-5 * (pr - p0).abs() + 1e-6 * lr + 1e-30
        tol_m = 4 * EPS32 * (m0.abs() + sg.abs()) + 2 * EPS32 * sg.abs() + 1e-30
        tol_v = 4 * EPS32 * (v0.abs() + (1.0 - b2) * sg * sg) + 2 * (1.0 - b2) * sg.abs() * (2 * EPS32 * sg.abs()) + 1e-30
        for name, got, ref, tol in (("p", p1, pr, tol_p), ("exp_avg", m1, mr, tol_m), ("exp_avg_sq", v1, vr, tol_v)):
            ratio = (got - ref).abs() / tol
            k = int(ratio.argmax())
            print(f"[clip-check] {where}: {name} worst err / tol {float(ratio[k]):.3g}")
            assert float(ratio[k]) <= 1.0, (f"{where}: {name}[{k}] = {float(got[k])!r}, float64 step on scale * g "
                                            f"{float(ref[k])!r} (err / tol = {float(ratio[k]):.3g})")
            self.worst = max(self.worst, float(ratio[k]))
        if scale64 < 1.0:
            # the same step with the gradient left unclipped: the moments must tell it apart at every step, the parameters
            # from the second step on when the two steps' scales differ (at step 1 Adam's m / sqrt(v) cancels the scale)
            pw, mw, vw = adamw_step_f64(p0, grad, m0, v0, t, lr, wd, self.betas, self.eps)
            seps = {"exp_avg": float(((m1 - mw).abs() / tol_m).max()), "exp_avg_sq": float(((v1 - vw).abs() / tol_v).max())}
            if t >= 2 and any(abs(s - scale64) > 0.1 * scale64 for s in self.scales):
                seps["p"] = float(((p1 - pw).abs() / tol_p).max())
            for name, sep in seps.items():
                print(f"[clip-check] {where}: unclipped step is {sep:.3g}x the {name} tolerance away")
                assert sep >= 100.0, f"{where}: the unclipped step is only {sep:.3g}x the {name} tolerance away"
                self.margin = min(self.margin, sep)
        self.scales.append(scale64)
        return norm64, scale64


SHAPES = [((3,), False), ((64, 3), False), ((5, 7), True), ((5,), False)]       # both regions, and padding in each


def _raw_params(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(*s, dtype=torch.complex64 if c else torch.float32, generator=g) * 0.1).to(dev))
            for s, c in SHAPES]


def _raw_grads(dev, seed, amp, bad=None):
    g = torch.Generator().manual_seed(1000 + seed)
    gs = [torch.randn(*s, dtype=torch.complex64 if c else torch.float32, generator=g) * amp for s, c in SHAPES]
    if bad is not None:
        gs[1][40, 2] = bad
    return [x.to(dev) for x in gs]


def _assign(opt, grads):
    opt.zero_grad()
    for p, g in zip(opt.bucket.params, grads):
        p.grad = g


def _raw_opt(dev, **kw):
    from rpde.optim import FlatAdamW
    return FlatAdamW(_raw_params(dev), lr=LR, weight_decay=WD, **kw)


def _raw_step(opt, grads):
    def run():
        _assign(opt, grads)
        opt.step()
    return run


# 270 floats of N(0, amp^2): norm ~ 16.4 amp against a bound of 1 -> scales ~ 0.03, ~ 0.5, and 1
AMPS = (2.0, 0.12, 0.01)


@pytest.mark.parametrize("capturable", [False, True])
def test_clipped_steps_against_float64(gpu_device, capturable):
    opt = _raw_opt(gpu_device, capturable=capturable, max_grad_norm=1.0)
    chk = ClipChecker(opt)
    scales = [chk.step(_raw_step(opt, _raw_grads(gpu_device, k, amp)))[1] for k, amp in enumerate(AMPS)]
    assert 0.02 < scales[0] < 0.05 and 0.35 < scales[1] < 0.7 and scales[2] == 1.0, scales
    rec = opt.grad_stats().tolist()
    assert rec[3:6] == [3.0, 2.0, 0.0]
    assert [int(float(s["step"])) for s in opt.state_dict()["state"].values()] == [3] * len(SHAPES)
    assert set(opt.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}          # torch's format, nothing added
    opt.reset_grad_stats()
    assert opt.grad_stats().tolist()[3:] == [0.0] * 5
    assert math.isfinite(chk.margin)


@pytest.mark.parametrize("capturable", [False, True])
def test_below_the_bound_is_bitwise_the_unclipped_optimizer(gpu_device, capturable):
    opt = _raw_opt(gpu_device, capturable=capturable, max_grad_norm=1.0)
    twin = _raw_opt(gpu_device, capturable=capturable)
    assert twin.grad_stats() is None and twin._clip_ws is None
    for k in range(3):
        for o in (opt, twin):
            _raw_step(o, _raw_grads(gpu_device, k, 0.01))()
        assert opt.grad_stats().tolist()[1] == 1.0
        for a, b in zip(opt.bucket.params, twin.bucket.params):
            assert torch.equal(_real(a.detach()).view(torch.int32), _real(b.detach()).view(torch.int32))
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(_real(opt.state[a][key]).view(torch.int32), _real(twin.state[b][key]).view(torch.int32))


def test_host_scalar_step_with_an_idle_parameter(gpu_device):
    """capturable=False: a parameter without a gradient splits the step into several update launches; its slot is zero
    in the norm, all launches read the one norm, and it neither moves nor counts a step"""
    opt = _raw_opt(gpu_device, max_grad_norm=1.0)
    chk = ClipChecker(opt)
    idle = opt.bucket.params[1]
    before = idle.detach().clone()
    for k, amp in enumerate(AMPS[:2]):
        grads = _raw_grads(gpu_device, k, amp)
        grads[1] = None
        chk.step(_raw_step(opt, grads), idle=(1,))
    assert torch.equal(idle.detach(), before)
    assert [int(float(s["step"])) for s in opt.state_dict()["state"].values()] == [2, 0, 2, 2]


# ---- skipping ----------------------------------------------------------------------------------------------------------

def _bits(opt):
    st = opt.state
    ts = list(opt.bucket.params) + [st[p]["exp_avg"] for p in opt.bucket.params] + [st[p]["exp_avg_sq"] for p in opt.bucket.params]
    return torch.cat([_real(t.detach()).reshape(-1) for t in ts]).view(torch.int32).cpu()


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_nonfinite_step_is_skipped_and_leaves_no_trace(gpu_device, bad):
    opt = _raw_opt(gpu_device, capturable=True, max_grad_norm=1.0, skip_nonfinite=True)
    chk = ClipChecker(opt)
    chk.step(_raw_step(opt, _raw_grads(gpu_device, 0, 2.0)))
    state0, dev0 = _bits(opt), opt._step_dev.view(torch.int32).cpu()
    skipped0 = opt.grad_stats().tolist()[5]
    _raw_step(opt, _raw_grads(gpu_device, 1, 0.12, bad=bad))()
    torch.cuda.synchronize()
    rec = opt.grad_stats().tolist()
    assert rec[2] == 1.0 and rec[5] == skipped0 + 1 and rec[3] == 2.0 and not math.isfinite(rec[0])
    assert torch.equal(_bits(opt), state0)
    dev1 = opt._step_dev.view(torch.int32).cpu()
    assert torch.equal(dev1[0:3], dev0[0:3]) and torch.equal(dev1[5], dev0[5])
    assert [int(float(s["step"])) for s in opt.state_dict()["state"].values()] == [1] * len(SHAPES)
    chk.step(_raw_step(opt, _raw_grads(gpu_device, 2, 0.12)))           # t = 2: the counter did not advance
    assert chk.t == 2 and opt.grad_stats().tolist()[2:6] == [0.0, 3.0, 2.0, 1.0]


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_without_skipping_a_nonfinite_gradient_reaches_the_parameters(gpu_device, bad):
    """torch's behaviour: a NaN norm makes the scale NaN and with it every element; an inf norm makes the scale 0, the
    inf entry NaN and every other gradient 0"""
    opt = _raw_opt(gpu_device, capturable=True, max_grad_norm=1.0)
    _raw_step(opt, _raw_grads(gpu_device, 0, 0.12, bad=bad))()
    torch.cuda.synchronize()
    rec = opt.grad_stats().tolist()
    assert rec[2] == 0.0 and rec[5] == 0.0 and float(opt._step_dev[0]) == 1.0
    hit = torch.isnan(opt.bucket.params[1].detach())
    assert bool(hit[40, 2])
    if math.isnan(bad):
        assert math.isnan(rec[1]) and all(bool(torch.isnan(_real(p.detach())).all()) for p in opt.bucket.params)
    else:
        assert rec[1] == 0.0 and int(hit.sum()) == 1
        assert all(not bool(torch.isnan(_real(p.detach())).any()) for i, p in enumerate(opt.bucket.params) if i != 1)


# ---- inside a captured step --------------------------------------------------------------------------------------------

def _model(dev, seed=0):
    """FNO1d width 16 (the graph tests' model) with every parameter ~ N(0, 0.1^2); its spectral weights are complex"""
    from models.fno import FNO1d
    torch.manual_seed(seed)
    m = FNO1d(1, 1, modes=8, width=16).to(dev).train()
    with torch.no_grad():
        for p in m.parameters():
            r = _real(p)
            r.copy_(torch.randn_like(r) * 0.1)
    return m


def _batch(dev, b, seed, n=128):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, 1, n, generator=g).to(dev), torch.randn(b, 1, n, generator=g).to(dev)


def _loss_fn():
    from utils.loss import RelativeL2Loss
    return RelativeL2Loss(size_average=True)


def _plain_grad_norm(model, x, y):
    """float64 norm of the model's gradient on (x, y) through autograd alone -- sizes the bound, touches no optimizer"""
    grads = torch.autograd.grad(_loss_fn()(model(x), y), list(model.parameters()))
    return total_norm_f64(grads)


# the relative L2 loss divides by |y|: a target scaled by SMALL has a gradient ~ 1 / SMALL times larger
SMALL = 0.05


def test_graph_replays_clip_by_their_own_gradient_and_skip_nonfinite_ones(gpu_device):
    from rpde.graph import GraphedTrainStep
    from rpde.optim import FlatAdamW
    model = _model(gpu_device)
    x, y = _batch(gpu_device, 4, 1)
    bound = float(np.float32(3.0 * _plain_grad_norm(model, x, y)))          # above an ordinary batch's norm, far below a SMALL target's
    opt = FlatAdamW(model.parameters(), lr=LR, weight_decay=WD, capturable=True, max_grad_norm=bound, skip_nonfinite=True)
    chk = ClipChecker(opt)

    def eager():
        opt.zero_grad()
        _loss_fn()(model(x), y).backward()
        opt.step()
    for _ in range(2):
        assert chk.step(eager)[1] == 1.0
    step = GraphedTrainStep(model, _loss_fn(), opt, x, y, warmup=0)
    assert opt.grad_stats().tolist()[3] == 2.0            # the capture ran nothing
    want = [True, False, True, False]
    for i, clipped in enumerate(want):
        xi, yi = _batch(gpu_device, 4, 10 + i)
        if clipped:
            yi = yi * SMALL
        _, scale = chk.step(lambda: step(xi, yi))
        assert (scale < 1.0) == clipped, (i, scale)
    assert opt.grad_stats().tolist()[3:6] == [6.0, 2.0, 0.0]
    state0, dev0 = _bits(opt), opt._step_dev.view(torch.int32).cpu()
    xi, yi = _batch(gpu_device, 4, 20)
    step(xi * float("inf"), yi)                           # data only: the forward carries inf / NaN into the gradient
    torch.cuda.synchronize()
    rec = opt.grad_stats().tolist()
    assert rec[2] == 1.0 and rec[3:6] == [7.0, 2.0, 1.0] and not math.isfinite(rec[0])
    assert torch.equal(_bits(opt), state0)
    dev1 = opt._step_dev.view(torch.int32).cpu()
    assert torch.equal(dev1[0:3], dev0[0:3]) and torch.equal(dev1[5], dev0[5])
    xi, yi = _batch(gpu_device, 4, 21)
    _, scale = chk.step(lambda: step(xi, yi * SMALL))     # the replay after it: right, at the un-advanced step count
    assert scale < 1.0 and chk.t == 7
    assert opt.grad_stats().tolist()[3:6] == [8.0, 3.0, 1.0]
    assert [int(float(s["step"])) for s in opt.state_dict()["state"].values()] == [7] * len(chk.params)


# ---- through train() ---------------------------------------------------------------------------------------------------

def test_train_eager_and_graph_agree_and_report_the_record(gpu_device):
    from rpde.optim import FlatAdamW
    from train.training import train
    base = _model(gpu_device, seed=11)
    g = torch.Generator().manual_seed(5)
    loader = [(torch.randn(4, 1, 128, generator=g), torch.randn(4, 1, 128, generator=g) * (SMALL if k % 2 else 1.0))
              for k in range(4)]
    val = [(torch.randn(4, 1, 128, generator=g), torch.randn(4, 1, 128, generator=g)) for _ in range(2)]
    # the bound sits in the widest gap between the batches' gradient norms at the starting weights (autograd alone, no
    # optimizer): the SMALL targets lie above it, the others below -- some steps clip, not all
    norms = sorted(_plain_grad_norm(base, x.to(gpu_device), y.to(gpu_device)) for x, y in loader)
    gap, k = max((norms[i + 1] / norms[i], i) for i in range(len(norms) - 1))
    assert gap > 2.0, norms
    bound = float(np.float32(math.sqrt(norms[k] * norms[k + 1])))
    out = []
    for graph in (False, True):
        m = copy.deepcopy(base)
        opt = FlatAdamW(m.parameters(), lr=2e-3, weight_decay=WD, capturable=True, max_grad_norm=bound)
        recs = []
        hist = train(m, loader, val, opt, None, epochs=2, device=gpu_device, graph=graph, log=recs.append)
        assert opt.grad_stats().tolist()[3:] == [0.0] * 5            # reset after the last epoch's read
        out.append((hist, m, recs))
    (he, me, re_), (hg, mg, rg) = out
    for a, b in zip(he[0] + he[1], hg[0] + hg[1]):
        assert abs(a - b) <= 2e-6 * max(1.0, abs(a)), (he, hg)
    for pe, pg in zip(me.parameters(), mg.parameters()):
        a, b = _real(pe.detach()), _real(pg.detach())
        assert float((a - b).norm() / (a.norm() + 1e-30)) < 2e-6
    for e, gr in zip(re_, rg):
        for rec in (e, gr):
            assert {"grad_norm_mean", "grad_norm_max", "clipped_steps", "skipped_steps"} <= set(rec)
            assert rec["skipped_steps"] == 0 and 0.0 < rec["grad_norm_mean"] <= rec["grad_norm_max"]
        assert e["clipped_steps"] == gr["clipped_steps"]
        assert abs(e["grad_norm_mean"] - gr["grad_norm_mean"]) <= 1e-4 * e["grad_norm_mean"]
    clipped = sum(r["clipped_steps"] for r in re_)
    assert 0 < clipped < 2 * len(loader), [r["clipped_steps"] for r in re_]      # some steps, not all
    assert max(r["grad_norm_max"] for r in re_) > bound
