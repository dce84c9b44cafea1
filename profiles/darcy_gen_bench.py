"""Time the Darcy generator's solve (csrc/darcy.hip, rpde.ops.darcy2d_solve) against the same preconditioned CG written
with stock torch ops (torch.matmul for the sine transforms) on the same GPU, and against the float64 sparse direct solve
on the host.  Does not touch bench.py.

    python profiles/darcy_gen_bench.py [--sizes 64,128,256] [--batch 64] [--iterations 24] [--repeats 7] [--out FILE.json]
    rocprofv3 --kernel-trace --stats -d DIR -o darcy -- python profiles/darcy_gen_bench.py --target 128
        (the per-kernel share of an iteration: 5 solves at one size with tol = 0, nothing else; counters, if wanted, in
         a run of their own)

Per size s (B samples, 12 / 3 coefficient from the cosine-series field, f = 1): warm-up, then `repeats` windows between
device events, alternating the implementations; ms per solve is the median.  `hip` is the solve as the script calls it
(tol 1e-6: frozen samples leave the streaming kernels early), `hip_no_freeze` the same with tol = 0 (all `iterations`
iterations in full), `torch` the stock-ops loop without a freeze.  bytes_per_iteration is a hand count of what the nine
launches of one un-frozen iteration move per sample, in units of one field (4 s^2 bytes):
  apply 3 (a, p in; Ap out)   update 8 (u, ul, r, p, Ap in; u, ul, r out)   two sep2d 8 (r, T, T, rh; rh, T, T, z)
  scale 2   dot 2   direction 3 (z, p in; p out)    -> 26 fields
against the copy rate of profiles/hbm_calibrate.py (5.2 TB/s, profiles/r03_hbm_calibrate.txt).  The fields of a batch
of 64 fit the 256 MB last-level cache up to s = 256, so the count is an upper bound on HBM traffic.  The direct solve runs scipy's spsolve on `--cpu-samples`
samples in a pool of 16 processes and reports samples/s of the whole box."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "resolution-pde_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FIELDS_PER_ITERATION = 26
HBM_GBPS = 5200.0                      # profiles/r03_hbm_calibrate.txt: copy rate of one MI355X


def _window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_pcg(a, f, S, il, iterations):
    """the same loop with stock ops, no freeze, scalars kept on the device"""
    s = a.shape[-1]
    s2 = float(s * s)

    def hm(x, y):
        return (2 * x * y) / (x + y)

    wl, wr, wn, ws = (2 * a for _ in range(4))
    wl[..., :, 1:] = hm(a[..., :, 1:], a[..., :, :-1]); wr[..., :, :-1] = wl[..., :, 1:]
    wn[..., 1:, :] = hm(a[..., 1:, :], a[..., :-1, :]); ws[..., :-1, :] = wn[..., 1:, :]

    def apply(u):
        p = torch.nn.functional.pad(u, (1, 1, 1, 1))
        c = p[..., 1:-1, 1:-1]
        return s2 * (wl * (c - p[..., 1:-1, :-2]) + wr * (c - p[..., 1:-1, 2:]) + wn * (c - p[..., :-2, 1:-1]) + ws * (c - p[..., 2:, 1:-1]))

    def prec(r):
        return torch.matmul(torch.matmul(S.t(), il * torch.matmul(torch.matmul(S, r), S.t())), S)

    dot = lambda x, y: (x * y).sum(dim=(1, 2), keepdim=True)        # noqa: E731
    u, r = torch.zeros_like(a), f.expand_as(a).clone()
    z = prec(r)
    p, rz = z.clone(), dot(r, z)
    for _ in range(iterations):
        Ap = apply(p)
        alpha = rz / dot(p, Ap)
        u, r = u + alpha * p, r - alpha * Ap
        z = prec(r)
        rz_new = dot(r, z)
        p, rz = z + (rz_new / rz) * p, rz_new
    return u


def _direct_one(args):
    from tests import darcy_ref as R
    a, s = args
    return R.direct(a[None], np.ones((s, s)))[0]


def bench(s, B, iterations, repeats, cpu_samples):
    from data_generation.darcy_2d import piecewise_constant
    from data_generation.random_fields import GaussianRFNeumann
    from rpde import ops
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    a = piecewise_constant(GaussianRFNeumann(s, device=dev).sample(B, generator=gen))
    f = torch.ones(s, s, device=dev)
    S, il = (t.to(dev) for t in ops.darcy2d_tables(s))
    out = {}
    runs = {"hip": lambda: out.__setitem__("hip", ops.darcy2d_solve(a, f, iterations, 1e-6)),
            "hip_no_freeze": lambda: ops.darcy2d_solve(a, f, iterations, 0.0),
            "torch": lambda: out.__setitem__("torch", torch_pcg(a, f, S, il, iterations))}
    for fn in runs.values():
        fn(); fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(repeats):
        for k, fn in runs.items():
            ms[k].append(_window(fn))
    u, rel, frozen_at = out["hip"]
    med = {k: statistics.median(v) for k, v in ms.items()}
    hist = {}
    for k in frozen_at.cpu().tolist():
        hist[str(k)] = hist.get(str(k), 0) + 1
    per_iter_ms = med["hip_no_freeze"] / iterations
    bytes_it = FIELDS_PER_ITERATION * 4 * s * s * B
    # the host's direct solve, 16 processes
    import multiprocessing as mp
    an = a[:cpu_samples].cpu().numpy()
    t0 = time.time()
    with mp.get_context("spawn").Pool(16) as pool:
        sol = pool.map(_direct_one, [(an[i], s) for i in range(len(an))])
    cpu_s = time.time() - t0
    err = float(np.linalg.norm(u[:len(an)].double().cpu().numpy() - np.stack(sol)) / np.linalg.norm(np.stack(sol)))
    return {"s": s, "B": B, "iterations": iterations, "windows": repeats,
            "ms_per_solve": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in ms.items()},
            "samples_per_s_hip": B / med["hip"] * 1e3, "torch_over_hip": med["torch"] / med["hip"],
            "torch_over_hip_no_freeze": med["torch"] / med["hip_no_freeze"],
            "ms_per_iteration_no_freeze": per_iter_ms, "bytes_per_iteration": bytes_it,
            "ms_per_iteration_at_hbm_rate": bytes_it / (HBM_GBPS * 1e9) * 1e3,
            "worst_rel_residual": float(rel.max()), "frozen_at_histogram": hist,
            "rel_l2_hip_vs_torch": float((u - out["torch"]).norm() / out["torch"].norm()),
            "cpu_direct": {"samples": len(an), "seconds_incl_pool_start": cpu_s, "samples_per_s": len(an) / cpu_s,
                           "hip_over_cpu_samples_per_s": (B / med["hip"] * 1e3) / (len(an) / cpu_s), "rel_l2_hip_vs_direct": err}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,256")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cpu-samples", type=int, default=16)
    ap.add_argument("--target", type=int, default=0, help="profiling target: 5 solves at this size, tol = 0, nothing else")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("darcy_gen_bench.py needs the GPU")
    if args.target:
        from rpde import ops
        a = 3.0 + 9.0 * (torch.rand(args.batch, args.target, args.target, device="cuda") > 0.5).float()
        f = torch.ones(args.target, args.target, device="cuda")
        for _ in range(5):
            ops.darcy2d_solve(a, f, args.iterations, 0.0)
        torch.cuda.synchronize()
        return
    lines = []
    for s in (int(v) for v in args.sizes.split(",")):
        lines.append(json.dumps(bench(s, args.batch, args.iterations, args.repeats, args.cpu_samples)))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
