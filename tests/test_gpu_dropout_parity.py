"""GPU: dropout-on training steps against the float64 oracle fed the kernels' own masks, element by element.

The masks come from a counter hash (csrc/drop_hash.h); oracle/dropout_mask.py restates it (pinned bit for bit on the
CPU by tests/test_oracle_dropout_cpu.py).  Every check here runs the forward and every gradient of a dropout-on
FeedForward or model in float64 with the restated masks of the seed the call used and the device epoch it read.
Each comparison also evaluates the oracle with one fault -- epoch +- 1, a neighbouring layer's seed, the mask applied
after the activation / LayerNorm -- and requires it to miss by at least MISS x the tolerance, so that a test that
cannot tell the right masks from wrong ones fails instead of passing."""
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FF_FWD_TOL, FF_GRAD_TOL = 5e-6, 2e-5           # as test_feedforward_depths_around_the_one_launch_limits
MODEL_FWD_TOL, MODEL_GRAD_TOL = 1e-5, 2e-5     # the golden-case tolerances (tests/test_gpu_golden.py)
MISS = 100.0


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


def _report(name, **kv):
    print(f"\n[dropout-parity] {name} " + " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}"
                                               for k, v in kv.items()))


def _post(name, t):
    return {"identity": lambda v: v, "gelu": F.gelu, "relu": F.relu}[name](t)


def _ff_masks(seed, epoch, p, P, dim, factor, L, layer_shift=0):
    from oracle import dropout_mask as D
    outs = [dim * factor] * (L - 1) + [dim]
    return [D.layer_mask(seed, l + layer_shift, epoch, p, P, o) for l, o in enumerate(outs)]


def _ff_after(x, sd, L, ln, masks):
    """fault: the mask multiplied in after GELU on hidden layers and after LayerNorm on the last"""
    for i in range(L):
        x = F.linear(x, sd[f"layers.{i}.0.weight"], sd[f"layers.{i}.0.bias"])
        if i < L - 1:
            x = F.gelu(x) * masks[i]
        else:
            if ln:
                g = sd[f"layers.{i}.3.weight"]
                x = F.layer_norm(x, (g.shape[0],), g, sd[f"layers.{i}.3.bias"], 1e-5)
            x = x * masks[i]
    return x


# (name, dim, factor, n_layers, points, p, layer_norm, residual, post_act, epoch, env)
FUSED_ENVS = {"default": {}, "stash_u": {"RPDE_FF_STASH": "u"}, "per_gemm": {"RPDE_FUSED_FF": "0", "RPDE_WGRAD_H2": "0"}}
FF_CASES = []
for _env_name in FUSED_ENVS:
    FF_CASES += [
        (f"fused-{_env_name}-big", 64, 4, 3, 25789, 0.1, True, True, "identity", 3, _env_name),
        (f"fused-{_env_name}-tail", 64, 4, 3, 1000, 0.3, False, False, "gelu", (1 << 32) + 5, _env_name),
    ]
FF_CASES += [
    ("w32x2-l3", 32, 2, 3, 1000, 0.1, True, False, "identity", 0, "default"),
    ("w32x2-l3-big", 32, 2, 3, 25789, 0.3, False, True, "gelu", (1 << 40) + 3, "default"),
    ("w48x4-l4", 48, 4, 4, 2500, 0.1, True, True, "identity", 7, "default"),
    ("w48x4-l4-noln", 48, 4, 4, 777, 0.3, False, False, "identity", 1, "default"),
    ("w10x3-l2", 10, 3, 2, 1000, 0.1, True, False, "identity", 4, "default"),
    ("w10x3-l2-noln", 10, 3, 2, 333, 0.3, False, False, "relu", (1 << 33) + 1, "default"),
    ("w128x4-l3-ffno1d", 128, 4, 3, 8192, 0.2, True, True, "gelu", 9, "default"),
    ("w32x2-l1", 32, 2, 1, 1000, 0.1, True, True, "identity", 2, "default"),
    ("w32x2-l1-noln", 32, 2, 1, 700, 0.3, False, False, "identity", (1 << 32), "default"),
    ("w16x2-l7", 16, 2, 7, 1500, 0.1, True, False, "identity", 5, "default"),
    ("w16x2-l8", 16, 2, 8, 1500, 0.3, False, False, "identity", 6, "default"),
    ("w16x2-l9", 16, 2, 9, 1500, 0.1, True, True, "identity", (1 << 32) + 7, "default"),
]


@pytest.mark.parametrize("case", FF_CASES, ids=[c[0] for c in FF_CASES])
def test_feedforward_dropout_matches_float64_with_restated_masks(gpu_device, case):
    """Every mask producer of the FeedForward: the GEMM epilogue that writes h / d of the hidden layers, the tail
    kernels (k_ff_tail_fwd / _any, k_ff_tail_bwd / _vec), the fused forward and backward in both stash modes."""
    from models.custom_layer import FeedForward
    from oracle import reference_path as R
    from rpde import ops
    name, dim, factor, L, P, p, ln, res, post, epoch, env = case
    seed = 0xD1B54A32D192ED03 ^ zlib.crc32(name.encode())
    torch.manual_seed(sum(map(ord, name)))
    ff = FeedForward(dim, factor, n_layers=L, layer_norm=ln, dropout=p).to(gpu_device).train()
    if ln:
        with torch.no_grad():                              # a LayerNorm with non-trivial affine parameters
            ff.layers[-1][3].weight.add_(0.3 * torch.randn(dim, device=gpu_device))
            ff.layers[-1][3].bias.add_(0.3 * torch.randn(dim, device=gpu_device))
    x = torch.randn(P, dim, device=gpu_device, requires_grad=True)
    r = torch.randn(P, dim, device=gpu_device, requires_grad=True) if res else None
    probe = torch.randn(P, dim, device=gpu_device)
    lin = [blk[0] for blk in ff.layers]
    lnp = (ff.layers[-1][3].weight, ff.layers[-1][3].bias) if ln else None
    ep = ops.drop_epoch(gpu_device)
    try:
        ep.fill_(epoch)
        with _env(**FUSED_ENVS[env]):
            out = ops.feedforward(x, r, [l.weight for l in lin], [l.bias for l in lin], lnp, dim, factor, p, seed, post)
            (out * probe).sum().backward()
        torch.cuda.synchronize()
        assert int(ep.item()) == epoch
    finally:
        ep.zero_()

    sd = {k: v.detach().double().cpu().requires_grad_() for k, v in ff.state_dict().items()}
    xd = x.detach().double().cpu().requires_grad_()
    rd = r.detach().double().cpu().requires_grad_() if res else None
    masks = _ff_masks(seed, epoch, p, P, dim, factor, L)

    def oracle(ms, after=False):
        y = _ff_after(xd, sd, L, ln, ms) if after else R.feedforward(xd, sd, "", L, ln, masks=ms)
        y = _post(post, y)
        return y + rd if res else y

    ref = oracle(masks)
    (ref * probe.double().cpu()).sum().backward()
    ef = _rel(out, ref)
    eg = {"x": _rel(x.grad, xd.grad)}
    if res:
        eg["residual"] = _rel(r.grad, rd.grad)
    for k, prm in ff.named_parameters():
        eg[k] = _rel(prm.grad, sd[k].grad)
    assert ef < FF_FWD_TOL, ef
    for k, e in eg.items():
        assert e < FF_GRAD_TOL, (k, e)
    if not ln and not res and post != "relu":
        # no LayerNorm: the output is exactly zero where (and only where) the last layer's mask dropped
        assert torch.equal(out.detach().cpu() == 0, masks[-1] == 0)

    # sensitivity: the same oracle with one fault must miss by far more than the tolerance
    faults = {"epoch+1": _ff_masks(seed, epoch + 1, p, P, dim, factor, L),
              "neighbour layer seed": _ff_masks(seed, epoch, p, P, dim, factor, L, layer_shift=1)}
    if epoch > 0:
        faults["epoch-1"] = _ff_masks(seed, epoch - 1, p, P, dim, factor, L)
    miss = {}
    with torch.no_grad():
        for fname, fm in faults.items():
            miss[fname] = _rel(out, oracle(fm)) / FF_FWD_TOL
        if L > 1 or ln:
            miss["mask after act / LayerNorm"] = _rel(out, oracle(masks, after=True)) / FF_FWD_TOL
    for fname, m in miss.items():
        assert m >= MISS, (fname, m)
    _report(name, fwd=ef, grad=max(eg.values()), min_miss=min(miss.values()))


def test_feedforward_sixteen_layers_without_dropout(gpu_device):
    """the backward takes any depth the forward takes (it refused more than 8 layers)"""
    from models.custom_layer import FeedForward
    from oracle import reference_path as R
    torch.manual_seed(16)
    L, dim, P = 16, 16, 1200
    ff = FeedForward(dim, 2, n_layers=L, layer_norm=True, dropout=0.0).to(gpu_device).train()
    x = torch.randn(P, dim, device=gpu_device, requires_grad=True)
    probe = torch.randn(P, dim, device=gpu_device)
    out = ff(x)
    (out * probe).sum().backward()
    sd = {k: v.detach().double().cpu().requires_grad_() for k, v in ff.state_dict().items()}
    xd = x.detach().double().cpu().requires_grad_()
    ref = R.feedforward(xd, sd, "", L, True)
    (ref * probe.double().cpu()).sum().backward()
    assert _rel(out, ref) < FF_FWD_TOL
    assert _rel(x.grad, xd.grad) < FF_GRAD_TOL
    for k, prm in ff.named_parameters():
        assert _rel(prm.grad, sd[k].grad) < FF_GRAD_TOL, k


@pytest.mark.parametrize("drop_ld", [(1 << 32) + 4, (1 << 32) + 129], ids=["ld-2^32+4", "ld-odd"])
def test_gemm_mask_sites_with_high_word_ids(gpu_device, drop_ld):
    """Element ids >= 2^32 (the high word enters drop_base): the A / B staging prologues and the backward-data
    epilogue against the restated mask, bit for bit.  drop_ld % 4 == 0 takes the 4-wide hash, an odd drop_ld the
    scalar one; the ids are point * drop_ld + feature, so no memory of that size is touched."""
    import ctypes as C
    from oracle import dropout_mask as D
    from rpde import _lib
    lib = _lib.load()
    P, J, p, seed = 256, 128, 0.25, 0xA0761D6478BD642F
    eye_j = torch.eye(J, device=gpu_device)
    eye_p = torch.eye(P, device=gpu_device)
    ones = torch.ones(P, J, device=gpu_device)

    def run(**kw):
        out = torch.empty(P, J, device=gpu_device)
        d = _lib.GemmDesc()
        d.batch, d.zdiv, d.ksplit, d.alpha = 1, 1, 1, 1.0
        d.C, d.ldc, d.M, d.N = out.data_ptr(), J, P, J
        d.drop_p, d.drop_seed, d.drop_ld = p, seed, drop_ld
        for k, v in kw.items():
            setattr(d, k, v)
        _lib.check(lib.rpde_gemm_f32(C.byref(d), _lib.stream_ptr()), "gemm")
        return out.cpu().double()

    m_a = run(A=ones.data_ptr(), lda=J, a_kmajor=1, B=eye_j.data_ptr(), ldb=J, b_kmajor=1, K=J, act_a=0, drop_where=1)
    m_b = run(A=eye_p.data_ptr(), lda=P, a_kmajor=1, B=ones.data_ptr(), ldb=J, b_kmajor=0, K=P, act_b=0, drop_where=2)
    big = torch.full((P, J), 30.0, device=gpu_device)
    m_e = run(A=ones.data_ptr(), lda=J, a_kmajor=1, B=eye_j.data_ptr(), ldb=J, b_kmajor=0, K=J, epi_dact=1,
              aux=big.data_ptr(), ldaux=J, drop_where=4)
    ids = np.arange(P, dtype=np.uint64)[:, None] * np.uint64(drop_ld) + np.arange(J, dtype=np.uint64)[None, :]
    assert int(ids.max()) >= 1 << 32 and int(ids.min()) < 1 << 32
    want = torch.from_numpy(D.factor(seed, 0, p, ids))
    for site, m in (("A prologue", m_a), ("B prologue", m_b), ("epilogue", m_e)):
        assert torch.equal(m != 0, want != 0), site
        assert float((m - want).abs().max()) <= 1e-6 * D.scale(p), site
    # sensitivity: ids taken modulo 2^32 (the high word ignored) give another mask
    low = torch.from_numpy(D.factor(seed, 0, p, ids & np.uint64(0xFFFFFFFF)))
    assert float(((low != 0) != (want != 0)).double().mean()) > 0.2


# ---------------------------------------------------------------------------------------------------------------------
# whole models in training mode
# ---------------------------------------------------------------------------------------------------------------------
class _SeedRecorder:
    """wraps rpde.ops.feedforward (models/custom_layer.py draws the seed and calls it) to record (seed, P, dim, ...)"""

    def __init__(self, monkeypatch):
        from rpde import ops
        self.calls = []
        orig = ops.feedforward

        def rec(x, residual, weights, biases, ln, dim, factor, dropout_p, seed, *a, **k):
            self.calls.append(dict(seed=int(seed), P=x.numel() // dim, dim=dim, factor=factor, L=len(weights),
                                   p=float(dropout_p)))
            return orig(x, residual, weights, biases, ln, dim, factor, dropout_p, seed, *a, **k)
        monkeypatch.setattr(ops, "feedforward", rec)


def _model_masks(calls, epoch, layer_shift=0, block_perm=None):
    """(block, layer) -> restated mask of the block's FeedForward call"""
    from oracle import dropout_mask as D
    cache = {}

    def get(block, layer):
        c = calls[block_perm[block] if block_perm else block]
        key = (block, layer)
        if key not in cache:
            out = c["dim"] if layer == c["L"] - 1 else c["dim"] * c["factor"]
            cache[key] = D.layer_mask(c["seed"], layer + layer_shift, epoch, c["p"], c["P"], out)
        return cache[key]
    return get


def _grad_err(g, r, gmax):
    """relative error of one parameter's gradient; a gradient that vanishes analytically (|r| <= 1e-6 of the largest,
    e.g. weight_v of a weight-normed layer with one input feature) is held to the largest gradient's scale instead"""
    g, r = g.detach().double().cpu(), r.detach().double().cpu()
    return float((g - r).norm() / max(float(r.norm()), 1e-6 * gmax)) if float(r.norm()) > 1e-6 * gmax \
        else float((g - r).norm() / gmax)


def _check_model(name, pred, loss, model, sd, x, y, oracle_fwd, calls, epoch):
    """pred / loss / grads of a model step against oracle_fwd(params, x, masks) in float64, plus the fault oracles"""
    from oracle import reference_path as R
    params = {k: v.detach().double().requires_grad_(True) for k, v in sd.items()}
    xd, yd = x.double().cpu(), y.double().cpu()
    ref = oracle_fwd(params, xd, _model_masks(calls, epoch))
    ref_loss = R.relative_l2(ref, yd)
    ref_loss.backward()
    ef = max(_rel(pred, ref), abs(float(loss) - float(ref_loss)) / float(ref_loss))
    gmax = max(float(prm.grad.norm()) for prm in params.values())
    eg = {k: _grad_err(prm.grad, params[k].grad, gmax) for k, prm in model.named_parameters()}
    assert ef < MODEL_FWD_TOL, (name, ef)
    for k, e in eg.items():
        assert e < MODEL_GRAD_TOL, (name, k, e)
    faults = {"epoch+1": _model_masks(calls, epoch + 1), "epoch-1": _model_masks(calls, epoch - 1),
              "neighbour layer seed": _model_masks(calls, epoch, layer_shift=1),
              "blocks' seeds rotated": _model_masks(calls, epoch, block_perm=[(i + 1) % len(calls) for i in range(len(calls))])}
    miss = {}
    with torch.no_grad():
        p0 = {k: v.detach() for k, v in params.items()}
        for fname, fm in faults.items():
            miss[fname] = _rel(pred, oracle_fwd(p0, xd, fm)) / MODEL_FWD_TOL
    for fname, m in miss.items():
        assert m >= MISS, (name, fname, m)
    _report(name, fwd=ef, grad=max(eg.values()), min_miss=min(miss.values()))


@pytest.mark.parametrize("res,B", [(64, 4), (256, 1)])
def test_ffno2d_training_step_with_dropout_matches_float64(gpu_device, monkeypatch, res, B):
    """the headline model shape (width 64, 3 FeedForward layers, LayerNorm, dropout 0.1) through RelativeL2Loss"""
    from models.ffno import FFNO2D
    from oracle import reference_path as R
    from rpde import ops
    from utils.loss import RelativeL2Loss
    from utils.synthetic import advance, random_fields
    torch.manual_seed(res + B)
    cfg = dict(width=64, n_layers=4, n_modes=12, factor=4, ff_weight_norm=True, n_ff_layers=3, layer_norm=True,
               dropout=0.1)
    m = FFNO2D(1, 1, **cfg).train()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(gpu_device)
    x = random_fields(B, res, 2, seed=res)
    y = advance(x, 2)
    rec = _SeedRecorder(monkeypatch)
    epoch = (1 << 32) + 17
    ep = ops.drop_epoch(gpu_device)
    try:
        ep.fill_(epoch)
        pred = m(x.to(gpu_device))
        loss = RelativeL2Loss()(pred, y.to(gpu_device))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ep.zero_()
    assert len(rec.calls) == 4 and all(c["P"] == B * res * res and c["p"] == 0.1 for c in rec.calls)
    assert len({c["seed"] for c in rec.calls}) == 4

    def oracle(p, xx, masks):
        return R.ffno2d_forward(p, xx, 4, 12, 3, True, masks=masks)
    _check_model(f"ffno2d-{res}^2-B{B}", pred.detach().cpu(), loss.detach().cpu(), m, sd, x, y, oracle, rec.calls, epoch)


def test_ffno1d_yaml_training_step_with_dropout_matches_float64(gpu_device, monkeypatch):
    """FFNO1D from conf/model/ffno_1d/ffno_1d.yaml (width 128, dropout 0.2, GELU after each block) at 512 points"""
    import yaml
    from models.ffno import FFNO1D
    from oracle import reference_path as R
    from rpde import ops
    from utils.loss import RelativeL2Loss
    from utils.synthetic import advance, random_fields
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(here, "resolution-pde_amd", "conf", "model", "ffno_1d", "ffno_1d.yaml")) as f:
        y_cfg = yaml.safe_load(f)
    keys = ("width", "n_layers", "n_modes", "factor", "n_ff_layers", "ff_weight_norm", "layer_norm", "dropout", "mode",
            "activation")
    cfg = {k: y_cfg[k] for k in keys}
    assert cfg["dropout"] == 0.2 and cfg["width"] == 128
    torch.manual_seed(5)
    m = FFNO1D(1, 1, **cfg).train()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(gpu_device)
    B, n = 4, 512
    x = random_fields(B, n, 1, seed=12)
    y = advance(x, 1)
    rec = _SeedRecorder(monkeypatch)
    epoch = 41
    ep = ops.drop_epoch(gpu_device)
    try:
        ep.fill_(epoch)
        pred = m(x.to(gpu_device))
        loss = RelativeL2Loss()(pred, y.to(gpu_device))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ep.zero_()
    assert len(rec.calls) == cfg["n_layers"] and all(c["P"] == B * n and c["p"] == 0.2 for c in rec.calls)

    def oracle(p, xx, masks):
        return R.ffno1d_forward(p, xx, cfg["n_layers"], cfg["n_modes"], cfg["n_ff_layers"], cfg["layer_norm"],
                                mode=cfg["mode"], activation=cfg["activation"], masks=masks)
    _check_model("ffno1d-yaml-512-B4", pred.detach().cpu(), loss.detach().cpu(), m, sd, x, y, oracle, rec.calls, epoch)


def test_graphed_step_replays_match_float64_at_their_epochs(gpu_device, monkeypatch):
    """GraphedTrainStep with FlatAdamW(capturable=True): each replay's loss and gradients equal the oracle's at the
    epoch that replay read, with the seeds recorded at capture; two replays use two epochs"""
    from models.ffno import FFNO2D
    from oracle import reference_path as R
    from rpde import ops
    from rpde.graph import GraphedTrainStep
    from rpde.optim import FlatAdamW
    from utils.loss import RelativeL2Loss
    from utils.synthetic import advance, random_fields
    torch.manual_seed(9)
    m = FFNO2D(1, 1, width=64, n_layers=4, n_modes=12, factor=4, ff_weight_norm=True, n_ff_layers=3, layer_norm=True,
               dropout=0.1).to(gpu_device).train()
    opt = FlatAdamW(m.parameters(), lr=1e-3, capturable=True)
    x = random_fields(4, 64, 2, seed=21)
    y = advance(x, 2)
    xg, yg = x.to(gpu_device), y.to(gpu_device)
    rec = _SeedRecorder(monkeypatch)
    ep = ops.drop_epoch(gpu_device)
    try:
        ep.fill_(100)
        step = GraphedTrainStep(m, RelativeL2Loss(), opt, xg, yg, warmup=2)
        calls = rec.calls[-4:]                               # the capture's draws: what every replay repeats
        assert len(rec.calls) == 3 * 4
        seen = []

        def grads_of(params, masks):
            loss_ = R.relative_l2(R.ffno2d_forward(params, x.double(), 4, 12, 3, True, masks=masks), y.double())
            return loss_, torch.autograd.grad(loss_, [params[k] for k, _ in m.named_parameters()])

        for i in range(2):
            sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
            loss = float(step(xg, yg))
            torch.cuda.synchronize()
            epoch = int(ep.item())
            seen.append(epoch)
            got = [p_.grad.double().cpu() for _, p_ in m.named_parameters()]
            params = {k: v.detach().double().requires_grad_(True) for k, v in sd.items()}
            ref_loss, ref_g = grads_of(params, _model_masks(calls, epoch))
            el = abs(loss - float(ref_loss)) / float(ref_loss)
            gmax = max(float(g.norm()) for g in ref_g)
            eg = {k: _grad_err(a_, r_, gmax) for (k, _), a_, r_ in zip(m.named_parameters(), got, ref_g)}
            assert el < MODEL_FWD_TOL, (i, el)
            for k, e in eg.items():
                assert e < MODEL_GRAD_TOL, (i, k, e)
            # sensitivity on the whole gradient (a loss is one number: a changed mask moves it only in second order)
            flat_got = torch.cat([g.reshape(-1) for g in got])
            miss = {}
            for fname, fm in (("epoch+1", _model_masks(calls, epoch + 1)), ("epoch-1", _model_masks(calls, epoch - 1)),
                              ("neighbour layer seed", _model_masks(calls, epoch, layer_shift=1))):
                _, fg = grads_of(params, fm)
                miss[fname] = _rel(flat_got, torch.cat([g.reshape(-1) for g in fg])) / MODEL_GRAD_TOL
            for fname, mm in miss.items():
                assert mm >= MISS, (i, fname, mm)
            _report(f"graphed-replay-{i}", epoch=epoch, loss=el, grad=max(eg.values()), min_miss=min(miss.values()))
        assert seen[0] != seen[1], seen
    finally:
        ep.zero_()
