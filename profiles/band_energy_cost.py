"""Cost of the band energies and the two losses on them against the yardstick, SpectralRelativeL2Loss forward + backward
(the same two transforms over the same spectrum with a static table), on the GPU, in one process:

    python profiles/band_energy_cost.py [--rounds 15] [--inner 20] [--out profiles/band_energy_cost.json]

Shapes (B, C, M, N): (32, 1, 256, 256) with 64 radial bins, (256, 1, 1, 1024) with octave bands.  Every variant is warmed
up, then the variants run in turn `rounds` times, each turn timing `inner` back-to-back calls between two device
events; reported: median [min - max] of the per-call milliseconds.  The primitive's parts come from differences of
medians: reduction = forward - forward transform alone, scale = backward - inverse transform alone (the transforms
through the generators' entries, which run the same plans)."""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "resolution-pde_amd"))

from rpde import _lib, ops                                       # noqa: E402
from rpde._lib import check, ptr, stream_ptr, workspace          # noqa: E402
from utils.loss import (BandRelativeL2Loss, RelativeL2Loss, SpectralRelativeL2Loss, SpectrumMatchingLoss,    # noqa: E402
                        SumLoss)

DEV = "cuda:0"


def transforms(B, M, N):
    """(forward, inverse) transform calls of B images on the half-spectrum layer alone"""
    lib = _lib.load()
    z = torch.randn(B, M, N, device=DEV) if M > 1 else torch.randn(B, N, device=DEV)
    if M > 1:
        spec = torch.empty(lib.rpde_ns2d_spec_elems(B, M, N), device=DEV)
        nws = lib.rpde_ns2d_ws_bytes(B, M, N)
        ws = workspace(nws, DEV)
        fwd = lambda: check(lib.rpde_ns2d_rfft2(ptr(z), ptr(spec), B, M, N, ws.data_ptr(), nws, stream_ptr()))      # noqa: E731
        inv = lambda: check(lib.rpde_ns2d_irfft2(ptr(spec), ptr(z), B, M, N, ws.data_ptr(), nws, stream_ptr()))     # noqa: E731
    else:
        spec = torch.empty(lib.rpde_etd1d_spec_elems(B, N), device=DEV)
        fwd = lambda: check(lib.rpde_etd1d_rfft(ptr(z), ptr(spec), B, N, stream_ptr()))      # noqa: E731
        inv = lambda: check(lib.rpde_etd1d_irfft(ptr(spec), ptr(z), B, N, stream_ptr()))     # noqa: E731
    return fwd, inv


def variants(B, C, M, N, bands, nb):
    dims = 1 if M == 1 else 2
    shape = (B, C, N) if M == 1 else (B, C, M, N)
    g = torch.Generator(device=DEV).manual_seed(0)
    y = torch.randn(shape, device=DEV, generator=g)
    x = (y + 0.3 * torch.randn(shape, device=DEV, generator=g)).requires_grad_(True)
    xn = x.detach()
    T = ops.resolve_bands(bands if nb is None else (bands, nb), shape[2:], DEV)
    gE = torch.rand(B, T.J, device=DEV, generator=g) + 0.5

    def step(fn):
        def run():
            x.grad = None
            fn(x, y).backward()
        return run

    def prim_both():
        x.grad = None
        ops.band_energy(x, T, dims).backward(gE)

    fwd_t, inv_t = transforms(B * C, M, N)
    return {
        "yardstick: SpectralRelativeL2Loss fwd+bwd": step(SpectralRelativeL2Loss(dims)),
        "BandRelativeL2Loss fwd+bwd": step(BandRelativeL2Loss(dims, bands, nb)),
        "SpectrumMatchingLoss fwd+bwd": step(SpectrumMatchingLoss(dims, bands, nb)),
        "RelativeL2 + 0.1 SpectrumMatching fwd+bwd": step(SumLoss([(1.0, RelativeL2Loss()), (0.1, SpectrumMatchingLoss(dims, bands, nb))])),
        "band_energy forward (no gradient)": lambda: ops.band_energy(xn, T, dims),
        "band_energy forward + backward": prim_both,
        "forward transform alone": fwd_t,
        "inverse transform alone": inv_t,
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
    ap.add_argument("--out", default=os.path.join(HERE, "band_energy_cost.json"))
    a = ap.parse_args()
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner, "cases": []}
    for B, C, M, N, bands, nb in ((32, 1, 256, 256, "radial", 64), (256, 1, 1, 1024, "octave", None)):
        res = measure(variants(B, C, M, N, bands, nb), a.rounds, a.inner)
        med = {k: v["median_ms"] for k, v in res.items()}
        yard = med["yardstick: SpectralRelativeL2Loss fwd+bwd"]
        fwd, both = med["band_energy forward (no gradient)"], med["band_energy forward + backward"]
        case = {"shape": [B, C, M, N], "bands": bands, "num_bands": nb, "timings": res,
                "ratio_to_yardstick": {k: med[k] / yard for k in med if "fwd+bwd" in k},
                "primitive_parts_ms": {"forward transform": med["forward transform alone"],
                                       "forward reduction (+ launches)": fwd - med["forward transform alone"],
                                       "backward (total)": both - fwd,
                                       "inverse transform": med["inverse transform alone"],
                                       "backward scale (+ launches)": both - fwd - med["inverse transform alone"]}}
        doc["cases"].append(case)
        for k, v in res.items():
            print(f"{(B, C, M, N)} {k:45s} {v['median_ms']:.4f} ms [{v['min_ms']:.4f} - {v['max_ms']:.4f}]", flush=True)
        print(json.dumps(case["ratio_to_yardstick"]), json.dumps(case["primitive_parts_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
