"""Cost of the Darcy equation-residual loss (utils.loss.DarcyResidualLoss, csrc/darcy_residual.hip), both norms, on the
GPU, in one process:

    python profiles/darcy_residual_cost.py [--rounds 15] [--inner 20] [--out profiles/darcy_residual_cost.json]

Shapes (B, s, s), one channel: (64, 32, 32), (64, 64, 64) and (32, 128, 128).  Timed: the forward alone (no gradient:
what validation pays), forward + backward, and RelativeL2 + 0.1 x residual forward + backward.  Beside them, in the same
process: the same loss written in stock torch ops on the same GPU (slicing and padding for the operator, two matmul
pairs for the sine transforms, autograd for the backward) and plain RelativeL2Loss, the unit of what a loss costs here.
Every variant is warmed up, then the variants run in turn `rounds` times, each turn timing `inner` back-to-back calls
between two device events; reported: median [min - max] of the per-call milliseconds.

--floors adds the exact pair on the device (p = the float64 direct solve rounded to fp32, coefficients 12 / 3, f = 1) at
s = 32, 64, 128 in both norms next to the float64 restatement (tests/darcy_residual_ref.py; needs scipy)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "resolution-pde_amd"))

from rpde import ops                                             # noqa: E402
from utils.loss import DarcyResidualLoss, RelativeL2Loss, SumLoss    # noqa: E402

DEV = "cuda:0"
NORMS = ("dual", "l2")


def torch_residual(s, norm):
    """the loss in stock torch ops, fp32 on the device; the backward is autograd's"""
    f, S, il, D = ops.darcy2d_residual_tables(s, 1.0, norm)
    f = f.to(DEV)
    S, il = (None, None) if S is None else (S.to(DEV), il.to(DEV))
    walls = torch.zeros(s, s, device=DEV)
    for edge in (walls[0], walls[-1], walls[:, 0], walls[:, -1]):
        edge += 2.0                                              # a wall face weighs 2 a_c, u = 0 behind it
    hm = lambda x, y: 2 * x * y / (x + y)                        # noqa: E731

    def loss(p, target, a):
        a, u = a[:, 0], p[:, 0]
        fx = hm(a[:, :, 1:], a[:, :, :-1]) * (u[:, :, 1:] - u[:, :, :-1])
        fy = hm(a[:, 1:, :], a[:, :-1, :]) * (u[:, 1:, :] - u[:, :-1, :])
        Au = F.pad(fx, (1, 0)) - F.pad(fx, (0, 1)) + F.pad(fy, (0, 0, 1, 0)) - F.pad(fy, (0, 0, 0, 1)) + walls * a * u
        r = f - float(s * s) * Au
        if S is None:
            E = (r * r).sum((1, 2))
        else:
            rh = S @ r @ S.T
            E = (il * rh * rh).sum((1, 2))
        return (torch.sqrt(E) / (D + 1e-8)).mean()

    return loss


def variants(B, s):
    g = torch.Generator(device=DEV).manual_seed(0)
    a = torch.where(torch.randn(B, 1, s, s, device=DEV, generator=g) >= 0, 12.0, 3.0)
    u, _, _ = ops.darcy2d_solve(a[:, 0].contiguous(), torch.ones(s, s, device=DEV), iterations=24)
    y = u[:, None].contiguous()
    x = (y * (1.0 + 0.05 * torch.randn(B, 1, s, s, device=DEV, generator=g))).requires_grad_(True)

    def step(fn, takes_input=True):
        def go():
            x.grad = None
            (fn(x, y, a) if takes_input else fn(x, y)).backward()
        return go

    fns, check = {}, {}
    for norm in NORMS:
        res, ref = DarcyResidualLoss(norm=norm), torch_residual(s, norm)
        fns[f"DarcyResidualLoss({norm}) forward (no gradient)"] = lambda res=res: res(x.detach(), None, a)
        fns[f"DarcyResidualLoss({norm}) fwd+bwd"] = step(res)
        fns[f"RelativeL2 + 0.1 DarcyResidual({norm}) fwd+bwd"] = step(SumLoss([(1.0, RelativeL2Loss()), (0.1, res)]))
        fns[f"torch restatement ({norm}) forward (no gradient)"] = lambda ref=ref: ref(x.detach(), None, a)
        fns[f"torch restatement ({norm}) fwd+bwd"] = step(ref)
        # the two compute the same thing
        step(res)()
        g_dev, v_dev = x.grad.clone(), float(res(x.detach(), None, a))
        step(ref)()
        check[norm] = {"value_device": v_dev, "value_torch": float(ref(x.detach(), None, a)),
                       "grad_rel_l2": float((x.grad - g_dev).norm() / g_dev.norm())}
    fns["RelativeL2Loss fwd+bwd"] = step(RelativeL2Loss(), False)
    return fns, check


def measure(fns, rounds, inner):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / inner)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}


def floors():
    import numpy as np
    sys.path.insert(0, REPO)
    from tests import darcy_ref as R
    from tests import darcy_residual_ref as Q
    out = []
    for s in (32, 64, 128):
        a = R.threshold(R.neumann_field(2, s, seed=1000 + s), 12.0, 3.0).astype(np.float32)
        f = np.ones((s, s), np.float32)
        p = R.direct(a, f).astype(np.float32)
        ad, pd = torch.from_numpy(a).to(DEV), torch.from_numpy(p).to(DEV)
        for norm in NORMS:
            loss = DarcyResidualLoss(norm=norm, reduction=False)
            row = {"s": s, "norm": norm, "exact_float64": Q.rel(a, p, f, np.float64, norm).tolist(),
                   "exact_device": loss(pd, None, ad).cpu().tolist(), "zero_device": loss(torch.zeros_like(pd), None, ad).cpu().tolist()}
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--floors", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "darcy_residual_cost.json"))
    a = ap.parse_args()
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner, "cases": []}
    for B, s in ((64, 32), (64, 64), (32, 128)):
        fns, check = variants(B, s)
        measure(fns, 3, a.inner)                                 # discarded: the clocks and the caches settle
        res = measure(fns, a.rounds, a.inner)
        med = {k: v["median_ms"] for k, v in res.items()}
        unit = med["RelativeL2Loss fwd+bwd"]
        case = {"shape": [B, s, s], "timings": res, "device_against_torch": check,
                "ratio_to_relative_l2": {k: med[k] / unit for k in med if "fwd+bwd" in k},
                "torch_over_device": {f"{norm} {what}": med[f"torch restatement ({norm}) {what}"] / med[f"DarcyResidualLoss({norm}) {what}"]
                                      for norm in NORMS for what in ("forward (no gradient)", "fwd+bwd")}}
        doc["cases"].append(case)
        for k, v in res.items():
            print(f"{(B, s, s)} {k:52s} {v['median_ms']:.4f} ms [{v['min_ms']:.4f} - {v['max_ms']:.4f}]", flush=True)
        print(json.dumps(case["torch_over_device"]), json.dumps(check), flush=True)
    if a.floors:
        doc["exact_pair"] = floors()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
