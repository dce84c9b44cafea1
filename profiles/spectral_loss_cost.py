"""What the mode-weighted relative L2 loss costs per step: forward + backward of
utils.loss.SpectralRelativeL2Loss (H^1 preset) and of RelativeL2Loss on the headline NS batch [32, 1, 256, 256] and the
Burgers batch [16, 1, 1024], alternating in one process, device events around windows of calls after warm-up.

Eager figures include the host's launches (7 + 4 kernels in 2-D, 5 + 2 in 1-D against 2 + 1); the same forward +
backward captured in a hipGraph and replayed is the device's share alone, which is what a graphed training step pays.

    python profiles/spectral_loss_cost.py [--rounds 5] [--calls 100]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "resolution-pde_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "spectral_loss_cost.py measures on the GPU"
    from utils.loss import RelativeL2Loss, SpectralRelativeL2Loss
    dev = "cuda:0"
    for shape in ((32, 1, 256, 256), (16, 1, 1024)):
        dims = len(shape) - 2
        g = torch.Generator(device=dev).manual_seed(1)
        y = torch.randn(shape, device=dev, generator=g)
        x = (y + 1e-2 * torch.randn(shape, device=dev, generator=g)).requires_grad_(True)
        h1 = SpectralRelativeL2Loss(dims, "sobolev", s=1.0)
        h1.warm(shape[2:], dev)
        losses = {"relative_l2": RelativeL2Loss(), "spectral_h1": h1}

        def fwd_bwd(fn):
            def run():
                x.grad = None
                fn(x, y).backward()
            return run
        ways = {k: fwd_bwd(fn) for k, fn in losses.items()}
        for fn in ways.values():
            window(fn, 20)
        eager = {k: [] for k in ways}
        for _ in range(args.rounds):
            for k, fn in ways.items():
                eager[k].append(window(fn, args.calls))
        graphs = {}
        for k in ways:
            xg = x.detach().clone().requires_grad_(True)       # a leaf no eager step has touched
            torch.cuda.synchronize()
            graphs[k] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[k]):
                losses[k](xg, y).backward()
            window(graphs[k].replay, 20)
        replayed = {k: [] for k in graphs}
        for _ in range(args.rounds):
            for k, gr in graphs.items():
                replayed[k].append(window(gr.replay, args.calls))
        fmt = lambda v: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}  # noqa: E731
        print(json.dumps({"shape": list(shape), "calls_per_window": args.calls, "rounds": args.rounds,
                          "us_per_fwd_bwd_eager": {k: fmt(v) for k, v in eager.items()},
                          "us_per_fwd_bwd_replayed": {k: fmt(v) for k, v in replayed.items()}}), flush=True)


if __name__ == "__main__":
    main()
