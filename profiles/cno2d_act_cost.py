"""Cost of the fused 2-D CNO activation (rpde_cno_act2d_fwd / _bwd) against the stock ATen sequence it replaces --
F.interpolate(bicubic, antialias) -> leaky_relu -> F.interpolate on planes, backward by autograd -- on the GPU, in one
process:

    python profiles/cno2d_act_cost.py [--rounds 15] [--inner 10] [--out profiles/cno2d_act_cost.json] [--no-step]

Shapes: the shipped yaml (conf/model/cno_2d/cno_2d.yaml) at size 128 and 256 and batch 4: the lifting level (64 latent
channels, out = in) and the first (D) block (16 channels, out = in / 2).  Every variant is warmed up, then the variants
run in turn `rounds` times, each turn timing `inner` back-to-back calls between two device events; reported: median
[min - max] of the per-call milliseconds, the bytes each side must move under the model of DESIGN.md 10.17 and the
resulting GB/s (n = in plane, m = mid plane, o = out plane, in floats per plane).

    fused  forward: read x, write out                          4 planes (n + o)
           backward: read x and g, write gy                    4 planes (2 n + o)
    ATen   forward: three ops, the mid plane written twice and read twice
                                                               4 planes (n + 4 m + o)
           backward: three ops, the saved mid plane read once  4 planes (o + 5 m + n)

Last, one whole training step of the shipped CNO2d (size 128, batch 8; forward, relative L2, backward, AdamW) against
the same module tree run through stock torch.nn / torch.nn.functional calls with torch.optim.AdamW."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "resolution-pde_amd"))

from rpde import ops                                             # noqa: E402

DEV = "cuda:0"
SLOPE = 0.01


def aten_act(x, in_size, out_size):
    u = F.interpolate(x, size=(2 * in_size, 2 * in_size), mode="bicubic", antialias=True)
    return F.interpolate(F.leaky_relu(u, SLOPE), size=(out_size, out_size), mode="bicubic", antialias=True)


def act_variants(B, C, n, n_out):
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(B, C, n, n, device=DEV, generator=g).requires_grad_(True)
    up = torch.randn(B, C, n_out, n_out, device=DEV, generator=g)
    xn = x.detach()

    def both(fn):
        def run():
            x.grad = None
            fn(x, n, n_out).backward(up)
        return run

    with torch.no_grad():
        diff = float((ops.cno_act2d(xn, n, n_out) - aten_act(xn, n, n_out)).norm() / aten_act(xn, n, n_out).norm())
    return {"fused forward": lambda: ops.cno_act2d(xn, n, n_out), "ATen forward": lambda: aten_act(xn, n, n_out),
            "fused forward + backward": both(ops.cno_act2d), "ATen forward + backward": both(aten_act)}, diff


# ---- the shipped model through stock torch calls, on the project's module tree (same parameters, same buffers) --------
def stock_block(m, x):
    return aten_act(m.batch_norm(m.convolution(x)), m.in_size, m.out_size)


def stock_lift_project(m, x):
    return m.convolution(stock_block(m.inter_CNOBlock, x))


def stock_resnet(m, x):
    for blk in m.res_nets:
        h = aten_act(blk.batch_norm1(blk.convolution1(x)), blk.size, blk.size)
        x = x + blk.batch_norm2(blk.convolution2(h))
    return x


def stock_cno2d(m, x):
    L = m.N_layers
    x = stock_lift_project(m.lift, x)
    skip = []
    for i in range(L):
        skip.append(stock_resnet(m.res_nets[i], x))
        x = stock_block(m.encoder[i], x)
    x = stock_resnet(m.res_net_neck, x)
    for i in range(L):
        x = stock_block(m.ED_expansion[L], x) if i == 0 else torch.cat((x, stock_block(m.ED_expansion[L - i], skip[-i])), 1)
        x = stock_block(m.decoder[i], x)
    return stock_lift_project(m.project, torch.cat((x, stock_block(m.ED_expansion[0], skip[0])), 1))


def step_variants(size, B):
    import copy
    from models.CNO2d import CNO2d
    from rpde.config import compose
    from rpde.optim import FlatAdamW
    from utils.loss import RelativeL2Loss
    cfg = compose(os.path.join(os.path.dirname(HERE), "resolution-pde_amd", "conf"), "config", ["model=cno_2d/cno_2d"]).model
    torch.manual_seed(0)
    ours = CNO2d(size=size, **{k: v for k, v in cfg.items() if not k.startswith("_")}).to(DEV).train()
    stock = copy.deepcopy(ours)
    g = torch.Generator(device=DEV).manual_seed(1)
    x, y = torch.randn(B, 3, size, size, device=DEV, generator=g), torch.randn(B, 3, size, size, device=DEV, generator=g)
    opt_o = FlatAdamW(ours.parameters(), lr=1e-4)
    opt_s = torch.optim.AdamW(stock.parameters(), lr=1e-4)
    loss_o = RelativeL2Loss()

    def step_ours():
        opt_o.zero_grad()
        loss_o(ours(x), y).backward()
        opt_o.step()

    def step_stock():
        opt_s.zero_grad()
        p = stock_cno2d(stock, x)
        ((p - y).flatten(1).norm(dim=1) / y.flatten(1).norm(dim=1)).mean().backward()
        opt_s.step()

    with torch.no_grad():
        ours.eval(), stock.eval()
        diff = float((ours(x) - stock_cno2d(stock, x)).norm() / stock_cno2d(stock, x).norm())
        ours.train(), stock.train()
    params = sum(p.numel() for p in ours.parameters())
    return {"CNO2d step, this library": step_ours, "CNO2d step, stock torch.nn": step_stock}, diff, params


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
    ap.add_argument("--out", default=os.path.join(HERE, "cno2d_act_cost.json"))
    ap.add_argument("--no-step", action="store_true", help="activation shapes only (for a kernel-trace run of its own)")
    a = ap.parse_args()
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner, "activation": [], "step": None}
    B = 4
    for C, n, n_out in ((64, 128, 128), (64, 256, 256), (16, 128, 64), (16, 256, 128)):
        fns, diff = act_variants(B, C, n, n_out)
        res = measure(fns, a.rounds, a.inner)
        planes, n_mid = B * C, 2 * n
        pi, pm, po = n * n, n_mid * n_mid, n_out * n_out
        nbytes = {"fused forward": 4 * planes * (pi + po), "ATen forward": 4 * planes * (pi + 4 * pm + po),
                  "fused backward": 4 * planes * (2 * pi + po), "ATen backward": 4 * planes * (po + 5 * pm + pi)}
        med = {k: v["median_ms"] for k, v in res.items()}
        table = {}
        for side in ("fused", "ATen"):
            fwd, bwd = med[f"{side} forward"], med[f"{side} forward + backward"] - med[f"{side} forward"]
            table[side] = {"forward_ms": fwd, "backward_ms": bwd, "forward_bytes": nbytes[f"{side} forward"],
                           "backward_bytes": nbytes[f"{side} backward"],
                           "forward_GBps": nbytes[f"{side} forward"] / fwd / 1e6, "backward_GBps": nbytes[f"{side} backward"] / bwd / 1e6}
        case = {"shape": {"B": B, "C": C, "in": [n, n], "mid": [n_mid, n_mid], "out": [n_out, n_out]}, "timings": res,
                "by_side": table,
                "speedup_forward": table["ATen"]["forward_ms"] / table["fused"]["forward_ms"],
                "speedup_forward_backward": med["ATen forward + backward"] / med["fused forward + backward"],
                "speedup_backward": table["ATen"]["backward_ms"] / table["fused"]["backward_ms"],
                "fused_vs_aten_rel_l2": diff}
        doc["activation"].append(case)
        for k, v in res.items():
            print(f"B={B} C={C} {n}^2->{n_mid}^2->{n_out}^2 {k:28s} {v['median_ms']:.4f} ms [{v['min_ms']:.4f} - {v['max_ms']:.4f}]", flush=True)
        print(json.dumps({k: case[k] for k in ("speedup_forward", "speedup_forward_backward", "speedup_backward", "fused_vs_aten_rel_l2")}), json.dumps(table), flush=True)
    if not a.no_step:
        step(doc, a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


def step(doc, a):
    size, B = 128, 8
    fns, diff, params = step_variants(size, B)
    res = measure(fns, max(3, a.rounds // 3), max(2, a.inner // 4))
    doc["step"] = {"size": size, "B": B, "params": params, "timings": res, "eval_forward_rel_l2_between_the_two": diff,
                   "speedup": res["CNO2d step, stock torch.nn"]["median_ms"] / res["CNO2d step, this library"]["median_ms"]}
    for k, v in res.items():
        print(f"{k:30s} {v['median_ms']:.3f} ms [{v['min_ms']:.3f} - {v['max_ms']:.3f}]", flush=True)
    print(json.dumps({"step_speedup": doc["step"]["speedup"], "params": params, "eval_rel_l2": diff}), flush=True)


if __name__ == "__main__":
    main()
