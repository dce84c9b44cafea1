"""What gradient clipping costs per optimizer step: FlatAdamW.step() on the buckets of the headline
FFNO2D (cfg3) and of the FFNO1D yaml, three ways, alternating in one process, device events around windows of steps:

    off    the plain step
    clip   FlatAdamW(max_grad_norm=...): norm -> finalise -> update on scale * g
    torch  what a user could do before: torch.nn.utils.clip_grad_norm_ on the bucket's views, then the plain step

The gradients are random numbers put into the bucket once and reused (clip_grad_norm_ is given a bound that never
clips; it runs all its passes regardless, the multiplication by 1 included).  Only the optimizers are built; no
model runs.
With capturable=True the plain and the clipped step are also captured in a hipGraph each and replayed: the eager
figures include the host's launches, the replayed ones are the device's share.

    python profiles/clip_cost.py [--rounds 5] [--steps 200]
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


def models():
    from models.ffno import FFNO1D, FFNO2D
    yield "FFNO2D cfg3 (headline)", lambda: FFNO2D(in_channels=1, out_channels=1, width=64, n_layers=4, n_modes=20, factor=4,
                                                   ff_weight_norm=True, n_ff_layers=3, layer_norm=True, dropout=0.1)
    yield "FFNO1D yaml", lambda: FFNO1D(1, 1, width=128, n_layers=4, n_modes=64, factor=4, ff_weight_norm=True, n_ff_layers=3,
                                        layer_norm=True, dropout=0.2)


def build(make, dev, **kw):
    from rpde.optim import FlatAdamW
    torch.manual_seed(0)
    model = make().to(dev)
    opt = FlatAdamW(model.parameters(), lr=1e-3, **kw)
    g = torch.Generator(device=dev).manual_seed(1)
    opt.bucket.flat.copy_(torch.randn(opt.bucket.flat.numel(), device=dev, generator=g) * 1e-3)
    for p, v in zip(opt.bucket.params, opt.bucket._views):
        p.grad = v
    opt.bucket._gathered = True
    return model, opt


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps          # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "clip_cost.py measures on the GPU"
    dev = "cuda:0"
    for name, make in models():
        for capturable in (False, True):
            m_off, o_off = build(make, dev, capturable=capturable)
            m_clip, o_clip = build(make, dev, capturable=capturable, max_grad_norm=1e9)
            m_t, o_t = build(make, dev, capturable=capturable)
            params_t = list(m_t.parameters())

            def torch_route():
                torch.nn.utils.clip_grad_norm_(params_t, 1e9)
                o_t.step()
            ways = {"off": o_off.step, "clip": o_clip.step, "torch": torch_route}
            for fn in ways.values():
                window(fn, 20)
            times = {k: [] for k in ways}
            for _ in range(args.rounds):
                for k, fn in ways.items():
                    times[k].append(window(fn, args.steps))
            replayed = {}
            if capturable:                         # the device's share alone: the same step captured and replayed
                graphs = {}
                for k, o in (("off", o_off), ("clip", o_clip)):
                    torch.cuda.synchronize()
                    graphs[k] = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graphs[k]):
                        o.step()
                    window(graphs[k].replay, 20)
                replayed = {k: [] for k in graphs}
                for _ in range(args.rounds):
                    for k, gr in graphs.items():
                        replayed[k].append(window(gr.replay, args.steps))
            n = o_off.bucket.flat.numel()
            print(json.dumps({"bucket": name, "floats": n, "mbytes": round(n * 4 / 1e6, 2), "tensors": len(params_t),
                              "capturable": capturable, "steps_per_window": args.steps,
                              "us_per_step": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2),
                                                  "max": round(max(v), 2)} for k, v in times.items()},
                              "us_per_replayed_step": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2),
                                                           "max": round(max(v), 2)} for k, v in replayed.items()},
                              "clip_extra_read_mbytes": round(n * 4 / 1e6, 2)}), flush=True)
            del m_off, o_off, m_clip, o_clip, m_t, o_t


if __name__ == "__main__":
    main()
