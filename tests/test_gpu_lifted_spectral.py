"""GPU: FFNO2D's first layer on the unlifted input (csrc/lifted_spectral.hip) against the 64-channel path
it replaces (RPDE_LIFTED_SPECTRAL=0) and against the float64 composed reference (oracle/reference_path.py).

Tolerance.  The lifted path replaces a 64-channel h2 analysis, an h2 mix and their adjoints by exact fp32 algebra on
Cin + 1 channels, so its error against float64 should be no larger than the old path's.  Every check measures the old
path's relative L2 error at the same shape, inputs and dropout masks and requires the new path's to stay within
FACTOR = 2 of it -- for the forward output, for the whole gradient (all parameters as one vector) and, one by one, for
the gradients the new kernels produce themselves (in_proj.*, the first layer's fourier weights).  The remaining
parameters see the change only as rounding noise of their cotangents; one by one they are held to the golden-case
tolerances (tests/test_gpu_golden.py), as is the loss (one number: its error is a single fp32 rounding either way)."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FACTOR = 2.0
MODEL_FWD_TOL, MODEL_GRAD_TOL = 1e-5, 2e-5
CFG3 = dict(in_channels=1, out_channels=1, width=64, n_layers=4, n_modes=20, factor=4, ff_weight_norm=True,
            n_ff_layers=3, layer_norm=True, dropout=0.0)
OWN = ("in_proj.", "fourier_layers.0.fourier_weight.")


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _flat(d, keys):
    return torch.cat([d[k].detach().double().cpu().reshape(-1) for k in keys])


class _Spy:
    """counts rpde.ops.lifted_fspectral2d calls and records the FeedForward seeds (models/custom_layer.py draws them)"""

    def __init__(self, monkeypatch):
        from rpde import ops
        self.lifted, self.ff = 0, []
        lifted, ff = ops.lifted_fspectral2d, ops.feedforward

        def spy_lifted(*a, **k):
            self.lifted += 1
            return lifted(*a, **k)

        def spy_ff(x, residual, weights, biases, ln, dim, factor, dropout_p, seed, *a, **k):
            self.ff.append(dict(seed=int(seed), P=x.numel() // dim, dim=dim, factor=factor, L=len(weights), p=float(dropout_p)))
            return ff(x, residual, weights, biases, ln, dim, factor, dropout_p, seed, *a, **k)
        monkeypatch.setattr(ops, "lifted_fspectral2d", spy_lifted)
        monkeypatch.setattr(ops, "feedforward", spy_ff)


def _masks(calls, epoch):
    """(block, layer) -> restated dropout mask of the block's FeedForward call at the device epoch the step read"""
    from oracle import dropout_mask as D
    cache = {}

    def get(block, layer):
        c = calls[block]
        if (block, layer) not in cache:
            out = c["dim"] if layer == c["L"] - 1 else c["dim"] * c["factor"]
            cache[(block, layer)] = D.layer_mask(c["seed"], layer, epoch, c["p"], c["P"], out)
        return cache[(block, layer)]
    return get


def _step(model, x, y, lifted, spy, x_grad=False):
    from rpde import ops
    from utils.loss import RelativeL2Loss
    epoch = int(ops.drop_epoch(x.device).item())            # eager steps read it and leave it (a graphed step advances it)
    model.zero_grad(set_to_none=True)
    torch.manual_seed(77)                                   # the FeedForward seeds: the same masks on both paths
    spy.lifted, spy.ff = 0, []
    xg = x.clone().requires_grad_(x_grad)
    with _env(RPDE_LIFTED_SPECTRAL="1" if lifted else "0"):
        pred = model(xg)
        loss = RelativeL2Loss()(pred, y)
        loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    return dict(pred=pred.detach(), loss=float(loss.detach()), grads=grads, gx=xg.grad, calls=list(spy.ff), lifted=spy.lifted,
                epoch=epoch)


def _reference(sd, cfg, x, y, calls, epoch, x_grad=False):
    from oracle import reference_path as R
    params = {k: v.detach().double().cpu().requires_grad_(True) for k, v in sd.items()}
    xd = x.double().cpu().requires_grad_(x_grad)
    ref = R.ffno2d_forward(params, xd, cfg["n_layers"], cfg["n_modes"], cfg["n_ff_layers"], cfg["layer_norm"],
                           masks=_masks(calls, epoch) if cfg["dropout"] > 0 else None)
    loss = R.relative_l2(ref, y.double().cpu())
    loss.backward()
    return dict(pred=ref.detach(), loss=float(loss.detach()), grads={k: v.grad for k, v in params.items()}, gx=xd.grad)


# (name, grid side, weight-normed in_proj, dropout): 20 modes clamp to 17 at 32^2
MODEL_CASES = [("wn-64", 64, True, 0.0), ("wn-64-drop", 64, True, 0.1), ("linear-64-drop", 64, False, 0.1),
               ("wn-32-clamp", 32, True, 0.0), ("linear-32-clamp-drop", 32, False, 0.1)]


@pytest.mark.parametrize("case", MODEL_CASES, ids=[c[0] for c in MODEL_CASES])
def test_ffno2d_cfg3_lifted_first_layer_matches_old_path_and_float64(gpu_device, monkeypatch, case):
    from models.custom_layer import WNLinear
    from models.ffno import FFNO2D
    from utils.synthetic import advance, random_fields
    name, res, wn, dropout = case
    cfg = dict(CFG3, ff_weight_norm=wn, dropout=dropout)
    torch.manual_seed(res + int(wn) + int(10 * dropout))
    m = FFNO2D(**cfg).train()
    assert isinstance(m.in_proj, WNLinear) == wn
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(gpu_device)
    x = random_fields(2, res, 2, seed=res)
    y = advance(x, 2)
    xg, yg = x.to(gpu_device), y.to(gpu_device)
    spy = _Spy(monkeypatch)
    new = _step(m, xg, yg, True, spy)
    old = _step(m, xg, yg, False, spy)
    assert new["lifted"] == 1 and old["lifted"] == 0
    assert [c["seed"] for c in new["calls"]] == [c["seed"] for c in old["calls"]] and len(new["calls"]) == 4
    assert new["epoch"] == old["epoch"]
    ref = _reference(sd, cfg, x, y, new["calls"], new["epoch"])            # one reference serves both paths

    keys = [k for k, _ in m.named_parameters()]
    own = [k for k in keys if k.startswith(OWN)]
    assert len(own) == (5 if wn else 4), own
    fig = {"fwd": (_rel(new["pred"], ref["pred"]), _rel(old["pred"], ref["pred"])),
           "grad": (_rel(_flat(new["grads"], keys), _flat(ref["grads"], keys)), _rel(_flat(old["grads"], keys), _flat(ref["grads"], keys)))}
    for k in own:
        fig[k] = (_rel(new["grads"][k], ref["grads"][k]), _rel(old["grads"][k], ref["grads"][k]))
    print(f"\n[lifted-spectral] {name} new-vs-old fwd={_rel(new['pred'], old['pred']):.3g} "
          f"grad={_rel(_flat(new['grads'], keys), _flat(old['grads'], keys)):.3g} loss {new['loss']:.9g} {old['loss']:.9g} "
          f"ref {ref['loss']:.9g} | (new, old) vs float64: " + " ".join(f"{k}=({a:.3g}, {b:.3g})" for k, (a, b) in fig.items()))
    for k, (e_new, e_old) in fig.items():
        assert e_new <= FACTOR * e_old, (name, k, e_new, e_old)
    gmax = max(float(g.norm()) for g in ref["grads"].values())
    for run in (new, old):
        assert _rel(run["pred"], ref["pred"]) < MODEL_FWD_TOL
        assert abs(run["loss"] - ref["loss"]) < MODEL_FWD_TOL * abs(ref["loss"])
        for k in keys:
            r = ref["grads"][k]
            e = float((run["grads"][k].double().cpu() - r).norm() / max(float(r.norm()), 1e-6 * gmax))
            assert e < MODEL_GRAD_TOL, (name, k, e)


def test_input_that_requires_grad_keeps_the_old_path(gpu_device, monkeypatch):
    """the lifted backward returns no input gradient: an input that asks for one must not take it, switch or no switch"""
    from models.ffno import FFNO2D
    from utils.synthetic import advance, random_fields
    cfg = dict(CFG3, dropout=0.1)
    torch.manual_seed(3)
    m = FFNO2D(**cfg).train()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(gpu_device)
    x = random_fields(2, 64, 2, seed=5)
    y = advance(x, 2)
    spy = _Spy(monkeypatch)
    got = _step(m, x.to(gpu_device), y.to(gpu_device), True, spy, x_grad=True)
    assert got["lifted"] == 0 and got["gx"] is not None
    ref = _reference(sd, cfg, x, y, got["calls"], got["epoch"], x_grad=True)
    assert _rel(got["pred"], ref["pred"]) < MODEL_FWD_TOL
    assert _rel(got["gx"], ref["gx"]) < MODEL_GRAD_TOL
    gmax = max(float(g.norm()) for g in ref["grads"].values())
    for k, _ in m.named_parameters():
        r = ref["grads"][k]
        e = float((got["grads"][k].double().cpu() - r).norm() / max(float(r.norm()), 1e-6 * gmax))
        assert e < MODEL_GRAD_TOL, (k, e)


# (name, B, M, N, Cin, K, bias): a rectangular grid (the two axes' lines differ in number, length and stride), every
# channel count the kernels are instantiated for, a mode count with a packed tail only (K = 4, 12) and with a full
# 32-row fragment (K = 16, 20), the clamp, a single slab (B = 1 at 32^2) and several
OP_CASES = [("64x64-k20", 2, 64, 64, 3, 20, True), ("32x32-clamp", 2, 32, 32, 3, 20, True),
            ("32x64-k12-nobias", 2, 32, 64, 3, 12, False), ("96x64-k16-c4", 1, 96, 64, 4, 16, True),
            ("32x32-k4-c1", 1, 32, 32, 1, 4, True), ("64x32-k12-c2", 3, 64, 32, 2, 12, False)]


@pytest.mark.parametrize("case", OP_CASES, ids=[c[0] for c in OP_CASES])
def test_lifted_op_matches_float64_within_the_old_paths_error_and_repeats_bitwise(gpu_device, case):
    """ops.lifted_fspectral2d alone: output and the four gradients against float64 autograd of
    forward_fourier(linear(u)), within FACTOR of ops.fspectral2d(ops.linear(u)) at the same inputs; a second run on
    the same inputs is bitwise the same (the line sums fold fixed-order partials, no atomics)."""
    from oracle import reference_path as R
    from rpde import ops
    name, B, M, N, cin, K, bias = case
    torch.manual_seed(sum(map(ord, name)))
    u = torch.randn(B, M, N, cin)
    w_in = torch.randn(64, cin) / cin ** 0.5
    b_in = torch.randn(64) if bias else None
    w_y, w_x = torch.randn(64, 64, K, 2) / 64, torch.randn(64, 64, K, 2) / 64
    g = torch.randn(B, M, N, 64)
    leaves = [t for t in (w_in, b_in, w_y, w_x) if t is not None]
    names = [n for n, t in zip(("w_in", "b_in", "w_y", "w_x"), (w_in, b_in, w_y, w_x)) if t is not None]

    def run(fn, dtype, dev):
        ls = [t.to(device=dev, dtype=dtype).requires_grad_() for t in leaves]
        it = iter(ls)
        wi = next(it)
        bi = next(it) if bias else None
        out = fn(u.to(device=dev, dtype=dtype), wi, bi, next(it), next(it))
        return out.detach(), torch.autograd.grad(out, ls, g.to(device=dev, dtype=dtype))

    assert ops.lifted_fspectral2d_ok(u.to(gpu_device), w_in.to(gpu_device), K)
    ref_out, ref_g = run(lambda a, wi, bi, wy, wx: R.fspectral2d_fourier(F.linear(a, wi, bi), wy, wx, K), torch.float64, "cpu")
    new_out, new_g = run(lambda a, wi, bi, wy, wx: ops.lifted_fspectral2d(a, wi, bi, wy, wx, K), torch.float32, gpu_device)
    rep_out, rep_g = run(lambda a, wi, bi, wy, wx: ops.lifted_fspectral2d(a, wi, bi, wy, wx, K), torch.float32, gpu_device)
    old_out, old_g = run(lambda a, wi, bi, wy, wx: ops.fspectral2d(ops.linear(a, wi, bi), wy, wx, K), torch.float32, gpu_device)
    assert torch.equal(new_out, rep_out) and all(torch.equal(a, b) for a, b in zip(new_g, rep_g))
    fig = {"out": (_rel(new_out, ref_out), _rel(old_out, ref_out))}
    for n, a, b, r in zip(names, new_g, old_g, ref_g):
        fig[n] = (_rel(a, r), _rel(b, r))
    print(f"\n[lifted-spectral] op {name} (new, old) vs float64: " + " ".join(f"{k}=({a:.3g}, {b:.3g})" for k, (a, b) in fig.items()))
    for k, (e_new, e_old) in fig.items():
        assert e_new <= FACTOR * e_old, (name, k, e_new, e_old)
        assert e_new < MODEL_GRAD_TOL, (name, k, e_new)
    for gw, n in ((new_g[-2], N), (new_g[-1], M)):           # modes the clamp drops: exactly zero
        assert not gw[:, :, min(K, n // 2 + 1):].any()
