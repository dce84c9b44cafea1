"""Cost of a U-Net training step on the GPU, in one process:

    python profiles/unet_cost.py [--warmup 10] [--steps 50] [--out profiles/unet_cost.json]

1. tanh_pool against its byte model, beside rpde_cno_affine (the plain one-read-one-write pass) on the same tensor:
   the first encoder level of the two models below.  Bytes per element, fp32:
       forward   read z 4, write act 4, write pooled 4 / (2 ky)                   8 without the pool; 10 (1-D), 9 (2-D)
       backward  read act 4, read g_act 4, read g_pool 4 / (2 ky), write gy 4      12 without the pool; 14 (1-D), 13 (2-D)
       affine    read a 4, write out 4                                             8
2. One training step (forward, relative L2, backward, AdamW) of the shipped yamls -- UNet1d at n = 1024, B = 16 and
   UNet2d at 128 x 128, B = 8 -- split by C entry of librpde_hip.so: every call of an entry is bracketed by two device
   events (a pass of its own: the events cost time), the per-step sums are taken and their medians over the timed steps
   reported; `other` is what the step spends outside the library's entries (torch.cat, the float64 coefficient
   arithmetic of the norms, the loss, allocation).
3. The step time of the same module tree run through stock torch.nn layers with torch.optim.AdamW.

Measurements to report, not thresholds."""
import argparse
import collections
import copy
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "resolution-pde_amd"))

from rpde import _lib, ops                                       # noqa: E402
from rpde.cno import _affine                                     # noqa: E402

DEV = "cuda:0"


def timed(fn, warmup, steps):
    """median [min, max] milliseconds of fn() over `steps` calls, each between two device events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def tanh_pool_rows(shape, warmup, steps):
    g = torch.Generator(device=DEV).manual_seed(0)
    z = torch.randn(*shape, device=DEV, generator=g)
    C, ky = shape[1], 1 if len(shape) == 3 else 2
    scale, shift = torch.rand(C, device=DEV, generator=g) + 0.5, torch.randn(C, device=DEV, generator=g)
    one, zero = torch.ones(C, dtype=torch.float64, device=DEV), torch.zeros(C, dtype=torch.float64, device=DEV)
    act, pooled = ops.tanh_pool(z, scale, shift, pool=True)
    g_act, g_pool = torch.randn_like(act), torch.randn_like(pooled)
    from rpde.unet import _tanh_pool_bwd, _tanh_pool_fwd
    n = z.numel()
    rows = {
        "affine (one read, one write)": (lambda: _affine(z, None, one, None, zero), 8.0),
        "tanh forward": (lambda: _tanh_pool_fwd(z, scale, shift, False, False), 8.0),
        "tanh + pool forward": (lambda: _tanh_pool_fwd(z, scale, shift, True, False), 8.0 + 4.0 / (2 * ky)),
        "tanh backward": (lambda: _tanh_pool_bwd(act, g_act, None), 12.0),
        "tanh + pool backward": (lambda: _tanh_pool_bwd(act, g_act, g_pool), 12.0 + 4.0 / (2 * ky)),
    }
    out = {}
    for name, (fn, bytes_per_element) in rows.items():
        t = timed(fn, warmup, steps)
        t["bytes"] = bytes_per_element * n
        t["GBps"] = t["bytes"] / t["median_ms"] / 1e6
        out[name] = t
        print(f"{tuple(shape)} {name:30s} {t['median_ms']:.4f} ms  {t['GBps']:.0f} GB/s", flush=True)
    return out


class EntryTimer:
    """stands in for the loaded library: every rpde_* call runs between two device events"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("rpde_") or name in ("rpde_last_error", "rpde_version") or name.endswith(("_slices", "_bytes", "_elems")):
            return fn

        def call(*args):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            status = fn(*args)
            b.record()
            self.calls.append((name, a, b))
            return status
        return call

    def drain(self):
        torch.cuda.synchronize()
        per = collections.defaultdict(float)
        count = collections.Counter()
        for name, a, b in self.calls:
            per[name] += a.elapsed_time(b)
            count[name] += 1
        self.calls = []
        return per, count


def stock_forward(m, x):
    """the reference's forward on the project's module tree: nn.Sequential blocks, nn.MaxPool, nn.ConvTranspose"""
    e1 = m.encoder1(x)
    e2 = m.encoder2(m.pool1(e1))
    e3 = m.encoder3(m.pool2(e2))
    e4 = m.encoder4(m.pool3(e3))
    d = m.bottleneck(m.pool4(e4))
    for up, dec, skip in ((m.upconv4, m.decoder4, e4), (m.upconv3, m.decoder3, e3), (m.upconv2, m.decoder2, e2), (m.upconv1, m.decoder1, e1)):
        d = dec(torch.cat((up(d), skip), dim=1))
    return m.conv(d)


def step_rows(yaml, shape, warmup, steps):
    from rpde.config import compose, instantiate
    from rpde.optim import FlatAdamW
    from utils.loss import RelativeL2Loss
    cfg = compose(os.path.join(os.path.dirname(HERE), "resolution-pde_amd", "conf"), "config", ["model=" + yaml]).model
    torch.manual_seed(0)
    ours = instantiate(cfg).to(DEV).train()
    stock = copy.deepcopy(ours)
    g = torch.Generator(device=DEV).manual_seed(1)
    x, y = torch.randn(*shape, device=DEV, generator=g), torch.randn(*shape, device=DEV, generator=g)
    opt_o = FlatAdamW(ours.parameters(), lr=1e-4, weight_decay=1e-4)
    opt_s = torch.optim.AdamW(stock.parameters(), lr=1e-4, weight_decay=1e-4)
    loss_o = RelativeL2Loss()

    def step_ours():
        opt_o.zero_grad()
        loss_o(ours(x), y).backward()
        opt_o.step()

    def step_stock():
        opt_s.zero_grad()
        p = stock_forward(stock, x)
        ((p - y).flatten(1).norm(dim=1) / y.flatten(1).norm(dim=1)).mean().backward()
        opt_s.step()

    with torch.no_grad():
        ours.eval(), stock.eval()
        ref = stock_forward(stock, x)
        diff = float((ours(x) - ref).norm() / ref.norm())
        ours.train(), stock.train()
    doc = {"model": cfg["_target_"], "shape": list(shape), "params": sum(p.numel() for p in ours.parameters()),
           "eval_forward_rel_l2_between_the_two": diff,
           "step, this library": timed(step_ours, warmup, steps), "step, stock torch.nn": timed(step_stock, warmup, steps)}
    doc["speedup"] = doc["step, stock torch.nn"]["median_ms"] / doc["step, this library"]["median_ms"]
    # per entry: a pass of its own, every library call between two events
    real = _lib.load()
    timer = _lib._lib = EntryTimer(real)
    try:
        for _ in range(warmup):
            step_ours()
        timer.drain()
        per_step, totals, counts = collections.defaultdict(list), [], None
        for _ in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step_ours()
            b.record()
            per, counts = timer.drain()
            totals.append(a.elapsed_time(b))
            for name, ms in per.items():
                per_step[name].append(ms)
    finally:
        _lib._lib = real
    entries = {name: {"median_ms_per_step": statistics.median(v), "calls_per_step": counts[name]} for name, v in per_step.items()}
    inside = sum(e["median_ms_per_step"] for e in entries.values())
    doc["per_entry"] = dict(sorted(entries.items(), key=lambda kv: -kv[1]["median_ms_per_step"]))
    doc["per_entry_pass_step_ms"] = statistics.median(totals)
    doc["other_ms"] = doc["per_entry_pass_step_ms"] - inside
    print(f"{yaml} {tuple(shape)}: step {doc['step, this library']['median_ms']:.2f} ms, stock {doc['step, stock torch.nn']['median_ms']:.2f} ms, "
          f"eval rel-L2 between them {diff:.2e}", flush=True)
    for name, e in doc["per_entry"].items():
        print(f"    {name:40s} {e['median_ms_per_step']:9.3f} ms  {e['calls_per_step']:4d} calls", flush=True)
    print(f"    {'other (timed pass: ' + format(doc['per_entry_pass_step_ms'], '.2f') + ' ms)':40s} {doc['other_ms']:9.3f} ms", flush=True)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(HERE, "unet_cost.json"))
    a = ap.parse_args()
    doc = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "steps": a.steps, "tanh_pool": {}, "step": {}}
    for shape in ((16, 64, 1024), (8, 64, 128, 128)):
        doc["tanh_pool"]["x".join(map(str, shape))] = tanh_pool_rows(shape, a.warmup, a.steps)
    for yaml, shape in (("unet/unet_1d", (16, 1, 1024)), ("unet/unet_2d", (8, 1, 128, 128))):
        doc["step"][yaml] = step_rows(yaml, shape, a.warmup, a.steps)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
