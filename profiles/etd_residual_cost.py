"""Cost of the equation-residual loss, forward + backward, next to SpectralRelativeL2Loss and RelativeL2Loss at the same
shapes, on the GPU, in one process:

    python profiles/etd_residual_cost.py [--rounds 15] [--inner 20] [--out profiles/etd_residual_cost.json]

Shapes (B, N), one channel: (64, 1024) and (512, 256).  The residual forms four spectra per sample forward (float64 sums
in its own kernel) and transforms 2 B images back, the mode-weighted loss 2 B and B: about twice its time is the
expectation.  Every variant is warmed up, then the variants run in turn `rounds` times, each turn timing `inner`
back-to-back calls between two device events; reported: median [min - max] of the per-call milliseconds.  The layer's
transforms alone (through the generators' entries, which run the same plans): the inverse of 2 B images is the
backward's, the forward of 4 B images is what the float64 analysis stands in for."""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "resolution-pde_amd"))

from rpde import _lib                                            # noqa: E402
from rpde._lib import check, ptr, stream_ptr                     # noqa: E402
from utils.loss import EquationResidualLoss, RelativeL2Loss, SpectralRelativeL2Loss, SumLoss    # noqa: E402

DEV = "cuda:0"


def transforms(images, N):
    lib = _lib.load()
    z = torch.randn(images, N, device=DEV)
    spec = torch.empty(lib.rpde_etd1d_spec_elems(images, N), device=DEV)
    fwd = lambda: check(lib.rpde_etd1d_rfft(ptr(z), ptr(spec), images, N, stream_ptr()))      # noqa: E731
    inv = lambda: check(lib.rpde_etd1d_irfft(ptr(spec), ptr(z), images, N, stream_ptr()))     # noqa: E731
    return fwd, inv


def variants(B, N):
    g = torch.Generator(device=DEV).manual_seed(0)
    y = torch.randn(B, 1, N, device=DEV, generator=g)
    inp = torch.randn(B, 1, N, device=DEV, generator=g)
    x = (y + 0.3 * torch.randn(B, 1, N, device=DEV, generator=g)).requires_grad_(True)
    residual = EquationResidualLoss.ks(0.05, N / 4.0, 0.05)
    decoded = EquationResidualLoss.ks(0.05, N / 4.0, 0.05)
    decoded.set_affine(pred=(1.5, 0.2), inp=(1.5, 0.2))
    both = SumLoss([(1.0, RelativeL2Loss()), (0.1, residual)])

    def step(fn, takes_input=False):
        def run():
            x.grad = None
            (fn(x, y, inp) if takes_input else fn(x, y)).backward()
        return run

    f4, _ = transforms(4 * B, N)
    _, i2 = transforms(2 * B, N)
    return {
        "EquationResidualLoss fwd+bwd": step(residual, True),
        "EquationResidualLoss with an affine decode fwd+bwd": step(decoded, True),
        "RelativeL2 + 0.1 EquationResidual fwd+bwd": step(both, True),
        "yardstick: SpectralRelativeL2Loss fwd+bwd": step(SpectralRelativeL2Loss(1)),
        "RelativeL2Loss fwd+bwd": step(RelativeL2Loss()),
        "EquationResidualLoss forward (no gradient)": lambda: residual(x.detach(), None, inp),
        "forward transform of 4 B images alone": f4,
        "inverse transform of 2 B images alone": i2,
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
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(HERE, "etd_residual_cost.json"))
    a = ap.parse_args()
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner, "cases": []}
    for B, N in ((64, 1024), (512, 256)):
        res = measure(variants(B, N), a.rounds, a.inner)
        med = {k: v["median_ms"] for k, v in res.items()}
        yard = med["yardstick: SpectralRelativeL2Loss fwd+bwd"]
        case = {"shape": [B, N], "timings": res,
                "ratio_to_yardstick": {k: med[k] / yard for k in med if "fwd+bwd" in k},
                "forward_share_of_residual": med["EquationResidualLoss forward (no gradient)"] / med["EquationResidualLoss fwd+bwd"]}
        doc["cases"].append(case)
        for k, v in res.items():
            print(f"{(B, N)} {k:52s} {v['median_ms']:.4f} ms [{v['min_ms']:.4f} - {v['max_ms']:.4f}]", flush=True)
        print(json.dumps(case["ratio_to_yardstick"]), case["forward_share_of_residual"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
