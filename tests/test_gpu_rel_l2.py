"""RelativeL2Loss / ops.relative_l2 (csrc/rel_loss.hip: k_rel_l2_partial, k_rel_l2_final, k_rel_l2_bwd) against float64
on the same fp32 inputs:

    rel_b = |x - y| / (|y| + 1e-8),    d loss / d x_b = g_b (x - y) / (|x - y| (|y| + 1e-8)),  0 where x == y,
    g_b = grad_rel[b] (reduction=False) or the upstream scalar, divided by B for the mean

at the sizes where the kernels change path: per % 4 != 0 and a base pointer that is only 4-byte aligned (the scalar branch
of k_rel_l2_partial), per below one block and below one float4, B > 256 (the stride loop of k_rel_l2_final), 2^20 points
per sample; with a good model (x = y (1 + 1e-4 randn)), a sample with x == y exactly (coef = 0) and a sample with y == 0;
mean / sum / none with a non-unit upstream gradient.

Bounds: per-sample rel within 1e-5 relative, per-sample gradient within 2e-5 relative L2 (the project's forward and
gradient budgets).  torch's own fp32 norm on the CPU sits between 1e-8 and 9.8e-7 against float64 on these sizes.
Every test prints the worst figures so far (pytest -s).  Measured on an MI355X, worst over all cases, regimes and modes:
    rel 2.1e-7   reduced loss 1.0e-7   gradient 1.9e-7   misaligned against aligned 1.5e-7
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

LOSS_TOL, GRAD_TOL = 1e-5, 2e-5          # FWD_TOL / GRAD_TOL of tests/test_gpu_golden.py
UPSTREAM = 3.7
CASES = [(1, 1), (3, 5), (2, 255), (4, 4096), (2, 4099), (2, 16388), (300, 7), (2, 1 << 20)]
REGIMES = ["randn", "good", "equal-sample", "zero-target-sample"]
MODES = [("mean", True, True), ("sum", False, True), ("none", True, False)]

_WORST = {"rel": 0.0, "loss": 0.0, "grad": 0.0, "misaligned": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\n[rel_l2] worst: " + ", ".join(f"{k} {v:.3e}" for k, v in _WORST.items()))


def _note(key, v):
    _WORST[key] = max(_WORST[key], v)
    return v


def make_pair(B, per, regime, seed=0):
    """fp32 CPU (x, y) [B, per] and the index of the special sample (or None)"""
    g = torch.Generator().manual_seed(1000 * seed + 31 * B + per)
    y = torch.randn(B, per, generator=g)
    if regime == "good":
        x = y * (1.0 + 1e-4 * torch.randn(B, per, generator=g))
    else:
        x = torch.randn(B, per, generator=g)
    special = None
    if regime == "equal-sample":
        special = B // 2
        x[special] = y[special]
    elif regime == "zero-target-sample":
        special = B // 2
        y[special] = 0.0
    return x, y, special


def reference(x, y, gb):
    """float64: (rel [B], gradient [B, per]) for per-sample upstream gradients gb [B]"""
    x, y, gb = x.double(), y.double(), gb.double()
    d = x - y
    dn, yn = d.norm(dim=1), y.norm(dim=1)
    rel = dn / (yn + 1e-8)
    coef = torch.where(dn > 0, gb / (dn * (yn + 1e-8)), torch.zeros_like(dn))
    return rel, coef[:, None] * d


def run(xd, yd, size_average, reduction, upstream):
    """-> (value, grad) on the device; upstream: the scalar, or a [B] device vector for reduction=False"""
    from utils.loss import RelativeL2Loss
    xs = xd.detach().requires_grad_(True)
    out = RelativeL2Loss(size_average=size_average, reduction=reduction)(xs, yd)
    ((out * upstream).sum() if not reduction else out * upstream).backward()
    return out.detach(), xs.grad


def check(tag, x, y, special, regime, xd, yd, bad, store=None):
    """all three modes of one (x, y) against float64; appends what misses to `bad`"""
    B, per = x.shape
    g = torch.Generator().manual_seed(B + per)
    v = torch.randn(B, generator=g)
    for mode, size_average, reduction in MODES:
        gb = v if not reduction else torch.full((B,), UPSTREAM / B if size_average else UPSTREAM)
        rel_ref, grad_ref = reference(x, y, gb)
        up = v.to(xd.device) if not reduction else UPSTREAM
        out, grad = run(xd, yd, size_average, reduction, up)
        out2, grad2 = run(xd, yd, size_average, reduction, up)
        if not (torch.equal(out, out2) and torch.equal(grad, grad2)):
            bad.append((tag, mode, "two identical calls differ"))
        if store is not None:
            store[mode] = (out, grad)
        if not (bool(torch.isfinite(out).all()) and bool(torch.isfinite(grad).all())):
            bad.append((tag, mode, "not finite"))
            continue
        o = out.double().cpu()
        if reduction:
            want = rel_ref.mean() if size_average else rel_ref.sum()
            e = _note("loss", float((o - want).abs() / want.abs().clamp_min(1e-300)))
            if e > LOSS_TOL:
                bad.append((tag, mode, "loss", e))
        else:
            if tuple(o.shape) != (B,):
                bad.append((tag, mode, "shape", tuple(o.shape)))
                continue
            err = (o - rel_ref).abs() / rel_ref.clamp_min(1e-300)
            if regime == "equal-sample":
                if float(o[special]) != 0.0:
                    bad.append((tag, mode, "rel of the x == y sample", float(o[special])))
                err[special] = 0.0
            if regime == "zero-target-sample":
                xn = float(x[special].double().norm())
                if abs(float(o[special]) * 1e-8 - xn) > LOSS_TOL * xn:
                    bad.append((tag, mode, "rel * 1e-8 against |x| where y == 0", float(o[special]) * 1e-8, xn))
            e = _note("rel", float(err.max()))
            if e > LOSS_TOL:
                bad.append((tag, mode, "rel", e))
        gd = grad.double().cpu()
        gn = grad_ref.norm(dim=1)
        gerr = (gd - grad_ref).norm(dim=1) / gn.clamp_min(1e-300)
        if regime == "equal-sample":
            if not bool((grad[special] == 0).all()):
                bad.append((tag, mode, "gradient of the x == y sample is not 0"))
            gerr[special] = 0.0
        e = _note("grad", float(gerr.max()))
        if e > GRAD_TOL:
            bad.append((tag, mode, "grad", e))


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[0]}-per{c[1]}")
def test_relative_l2_against_float64(gpu_device, case):
    B, per = case
    bad = []
    for regime in REGIMES:
        x, y, special = make_pair(B, per, regime)
        check(f"B={B} per={per} {regime}", x, y, special, regime, x.to(gpu_device), y.to(gpu_device), bad)
    print(f"[rel_l2] B={B} per={per}: worst so far " + ", ".join(f"{k} {v:.3e}" for k, v in _WORST.items()))
    assert not bad, bad


@pytest.mark.parametrize("which", ["x", "y", "both"])
def test_relative_l2_misaligned_base_takes_the_scalar_branch(gpu_device, which):
    """flat[1 : 1 + B per].view(B, per) is contiguous and 4-byte aligned: per % 4 == 0, but float4 loads are out, so the
    scalar loop must run, and give the numbers of the aligned copy to 1e-6 relative (and of float64 to the budgets)"""
    B, per = 4, 4096
    bad = []
    for regime in REGIMES:
        x, y, special = make_pair(B, per, regime, seed=1)

        def shifted(t):
            flat = torch.zeros(B * per + 8, device=gpu_device)
            v = flat[1:1 + B * per].view(B, per)
            v.copy_(t)
            assert v.is_contiguous() and v.data_ptr() % 16 == 4
            return v

        xa, ya = x.to(gpu_device), y.to(gpu_device)
        assert xa.data_ptr() % 16 == 0 and ya.data_ptr() % 16 == 0
        xm = shifted(x) if which in ("x", "both") else xa
        ym = shifted(y) if which in ("y", "both") else ya
        mis, ali = {}, {}
        check(f"misaligned {which} {regime}", x, y, special, regime, xm, ym, bad, mis)
        check(f"aligned {regime}", x, y, special, regime, xa, ya, bad, ali)
        for mode in mis:
            for name, a, b in zip(("value", "grad"), mis[mode], ali[mode]):
                a, b = a.double().reshape(B, -1) if a.dim() else a.double().reshape(1, 1), \
                    b.double().reshape(B, -1) if b.dim() else b.double().reshape(1, 1)
                d = ((a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-300))
                d = torch.where(b.norm(dim=1) == 0, (a - b).norm(dim=1), d)
                e = _note("misaligned", float(d.max()))
                if e > 1e-6:
                    bad.append((which, regime, mode, name, "misaligned against aligned", e))
    assert not bad, bad
