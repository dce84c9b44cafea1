"""Cost of the active-scalar equation-residual loss, forward + backward and forward alone, next to
VorticityResidualLoss and SpectralRelativeL2Loss(2) at the same grids, on the GPU, in one process:

    python profiles/nsc_residual_cost.py [--rounds 15] [--inner 10] [--out profiles/nsc_residual_cost.json]

Shapes (B, M, N): (32, 256, 256) and (32, 64, 64); the active-scalar loss takes three channels (c, q, v), the two
yardsticks one.  Its forward analyses 6 B images in float64 (3 B of x~, 3 B of d), transforms 12 B images back and 4 B
forward; the backward 8 B + 3 B back and 6 B forward.  The vorticity loss analyses 2 B, transforms 8 B back and 2 B
forward, then 5 B + B back and 4 B forward.  Every variant is warmed up, then the variants run in turn `rounds` times,
each turn timing `inner` back-to-back calls between two device events; reported: median [min - max] of the per-call
milliseconds.  The float64 analysis of 6 B images alone (rpde.ops.ns2d_residual_spectrum, the same kernels) and the
layer's inverse transform of 12 B images alone (through the generator's entry, which runs the same plans) are timed
beside them."""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "resolution-pde_amd"))

from rpde import _lib, ops                                       # noqa: E402
from rpde._lib import ptr, run, workspace                        # noqa: E402
from utils.loss import ActiveScalarResidualLoss, SpectralRelativeL2Loss, VorticityResidualLoss    # noqa: E402

DEV = "cuda:0"


def inverse_transform(images, M, N):
    lib = _lib.load()
    z = torch.randn(images, M, N, device=DEV)
    spec = torch.zeros(lib.rpde_ns2d_spec_elems(images, M, N), device=DEV)
    nws = lib.rpde_ns2d_ws_bytes(images, M, N)
    ws = workspace(nws, DEV)
    return lambda: run("ns2d_irfft2", nws, ws, ptr(spec), ptr(z), images, M, N)


def variants(B, M, N):
    g = torch.Generator(device=DEV).manual_seed(0)
    y3 = torch.randn(B, 3, M, N, device=DEV, generator=g)
    inp3 = torch.randn(B, 3, M, N, device=DEV, generator=g)
    x3 = (y3 + 0.3 * torch.randn(B, 3, M, N, device=DEV, generator=g)).requires_grad_(True)
    y1, inp1 = y3[:, :1].contiguous(), inp3[:, :1].contiguous()
    x1 = x3.detach()[:, :1].contiguous().requires_grad_(True)
    active = ActiveScalarResidualLoss(1e-3, 2e-3, 5.0, 0.05, forcing="reference")
    vort = VorticityResidualLoss(1e-3, 0.05, forcing="reference")
    six = torch.randn(6 * B, M, N, device=DEV, generator=g)

    def step(fn, x, y, inp=None):
        def go():
            x.grad = None
            (fn(x, y) if inp is None else fn(x, y, inp)).backward()
        return go

    return {
        "ActiveScalarResidualLoss fwd+bwd": step(active, x3, y3, inp3),
        "VorticityResidualLoss fwd+bwd": step(vort, x1, y1, inp1),
        "yardstick: SpectralRelativeL2Loss fwd+bwd": step(SpectralRelativeL2Loss(2), x1, y1),
        "ActiveScalarResidualLoss forward (no gradient)": lambda: active(x3.detach(), None, inp3),
        "VorticityResidualLoss forward (no gradient)": lambda: vort(x1.detach(), None, inp1),
        "float64 analysis of 6 B images alone": lambda: ops.ns2d_residual_spectrum(six),
        "inverse transform of 12 B images alone": inverse_transform(12 * B, M, N),
    }


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(HERE, "nsc_residual_cost.json"))
    a = ap.parse_args()
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner, "cases": []}
    for B, M, N in ((32, 64, 64), (32, 256, 256)):
        res = measure(variants(B, M, N), a.rounds, a.inner)
        med = {k: v["median_ms"] for k, v in res.items()}
        yard = med["yardstick: SpectralRelativeL2Loss fwd+bwd"]
        case = {"shape": [B, M, N], "timings": res,
                "ratio_to_yardstick": {k: med[k] / yard for k in med if "fwd+bwd" in k},
                "ratio_to_vorticity": med["ActiveScalarResidualLoss fwd+bwd"] / med["VorticityResidualLoss fwd+bwd"],
                "forward_share": med["ActiveScalarResidualLoss forward (no gradient)"] / med["ActiveScalarResidualLoss fwd+bwd"],
                "analysis_share_of_forward": med["float64 analysis of 6 B images alone"] / med["ActiveScalarResidualLoss forward (no gradient)"]}
        doc["cases"].append(case)
        for k, v in res.items():
            print(f"{(B, M, N)} {k:52s} {v['median_ms']:.4f} ms [{v['min_ms']:.4f} - {v['max_ms']:.4f}]", flush=True)
        print(json.dumps(case["ratio_to_yardstick"]), case["ratio_to_vorticity"], case["forward_share"],
              case["analysis_share_of_forward"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
