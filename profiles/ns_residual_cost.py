"""Cost of the vorticity equation-residual loss, forward + backward, next to SpectralRelativeL2Loss(2) and
RelativeL2Loss at the same shapes, on the GPU, in one process:

    python profiles/ns_residual_cost.py [--rounds 15] [--inner 10] [--out profiles/ns_residual_cost.json]

Shapes (B, M, N), one channel: (32, 256, 256) and (32, 64, 64).  The residual's forward transforms 8 B images back and
3 B forward and forms x^ by a float64 analysis of its own, the backward 5 B + B back and 4 B forward; the mode-weighted
loss transforms 2 B forward and B back.  Every variant is warmed up, then the variants run in turn `rounds` times, each
turn timing `inner` back-to-back calls between two device events; reported: median [min - max] of the per-call
milliseconds.  The float64 analysis alone (rpde.ops.ns2d_residual_spectrum) and the layer's transforms alone (through
the generator's entries, which run the same plans) are timed beside them."""
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
from utils.loss import RelativeL2Loss, SpectralRelativeL2Loss, SumLoss, VorticityResidualLoss    # noqa: E402

DEV = "cuda:0"


def transforms(images, M, N):
    lib = _lib.load()
    z = torch.randn(images, M, N, device=DEV)
    spec = torch.empty(lib.rpde_ns2d_spec_elems(images, M, N), device=DEV)
    nws = lib.rpde_ns2d_ws_bytes(images, M, N)
    ws = workspace(nws, DEV)
    fwd = lambda: run("ns2d_rfft2", nws, ws, ptr(z), ptr(spec), images, M, N)       # noqa: E731
    inv = lambda: run("ns2d_irfft2", nws, ws, ptr(spec), ptr(z), images, M, N)      # noqa: E731
    return fwd, inv


def variants(B, M, N):
    g = torch.Generator(device=DEV).manual_seed(0)
    y = torch.randn(B, 1, M, N, device=DEV, generator=g)
    inp = torch.randn(B, 1, M, N, device=DEV, generator=g)
    x = (y + 0.3 * torch.randn(B, 1, M, N, device=DEV, generator=g)).requires_grad_(True)
    residual = VorticityResidualLoss(1e-3, 0.05, forcing="reference")
    decoded = VorticityResidualLoss(1e-3, 0.05, forcing="reference")
    decoded.set_affine(pred=(1.5, 0.2), inp=(1.5, 0.2))
    both = SumLoss([(1.0, RelativeL2Loss()), (0.1, residual)])
    x3 = inp.detach().reshape(B, M, N)

    def step(fn, takes_input=False):
        def go():
            x.grad = None
            (fn(x, y, inp) if takes_input else fn(x, y)).backward()
        return go

    f3, _ = transforms(3 * B, M, N)
    _, i8 = transforms(8 * B, M, N)
    return {
        "VorticityResidualLoss fwd+bwd": step(residual, True),
        "VorticityResidualLoss with an affine decode fwd+bwd": step(decoded, True),
        "RelativeL2 + 0.1 VorticityResidual fwd+bwd": step(both, True),
        "yardstick: SpectralRelativeL2Loss fwd+bwd": step(SpectralRelativeL2Loss(2)),
        "RelativeL2Loss fwd+bwd": step(RelativeL2Loss()),
        "VorticityResidualLoss forward (no gradient)": lambda: residual(x.detach(), None, inp),
        "float64 analysis of B images alone": lambda: ops.ns2d_residual_spectrum(x3),
        "forward transform of 3 B images alone": f3,
        "inverse transform of 8 B images alone": i8,
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
    ap.add_argument("--out", default=os.path.join(HERE, "ns_residual_cost.json"))
    a = ap.parse_args()
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner, "cases": []}
    for B, M, N in ((32, 256, 256), (32, 64, 64)):
        res = measure(variants(B, M, N), a.rounds, a.inner)
        med = {k: v["median_ms"] for k, v in res.items()}
        yard = med["yardstick: SpectralRelativeL2Loss fwd+bwd"]
        case = {"shape": [B, M, N], "timings": res,
                "ratio_to_yardstick": {k: med[k] / yard for k in med if "fwd+bwd" in k},
                "forward_share_of_residual": med["VorticityResidualLoss forward (no gradient)"] / med["VorticityResidualLoss fwd+bwd"],
                "analysis_share_of_forward": med["float64 analysis of B images alone"] / med["VorticityResidualLoss forward (no gradient)"]}
        doc["cases"].append(case)
        for k, v in res.items():
            print(f"{(B, M, N)} {k:52s} {v['median_ms']:.4f} ms [{v['min_ms']:.4f} - {v['max_ms']:.4f}]", flush=True)
        print(json.dumps(case["ratio_to_yardstick"]), case["forward_share_of_residual"], case["analysis_share_of_forward"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
