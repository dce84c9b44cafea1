"""Time one step of the active-scalar Navier-Stokes generator (csrc/ns_solver.hip, rpde_nsc2d_steps) against one step of
the vorticity generator (csrc/ns_solver.hip, rpde_ns2d_steps) on the same GPU in the same run.  Does not touch bench.py.

    python profiles/nsc_gen_bench.py [--steps 50] [--repeats 7] [--sizes 256x50,64x50] [--out profiles/nsc_gen_bench.json]

Per (resolution s, batch B): warm-up (plans, code objects), then `repeats` windows of `steps` steps each between device
events, alternating the two solvers; reported are the median, minimum and maximum of the windows in ms per step and the
ratio of the medians.  The coupled step transforms 6B + 2B images where the vorticity step transforms 4B + B, and its
streaming kernels move bytes in about that proportion: the ratio to expect is 8/5 = 1.6.  The parts of the coupled step
are timed the same way through the C ABI: the inverse transform of 6B spectra, the forward transform of 2B products, and
the rest (k_ns_advect<true> + k_ns_update_fanout<MODE, true>) as the difference.  Needs the GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "resolution-pde_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def _windows(fn, steps, repeats):
    """ms per step of `repeats` windows of fn(steps)"""
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(steps)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return out


def _stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def bench(s, B, steps, repeats, visc=1e-4, kappa=1e-4, beta=1.0, dt=1e-4):
    from data_generation.ns_2d import forcing
    from data_generation.random_fields import GaussianRF
    from rpde import ops
    from rpde._lib import check, load, ptr, stream_ptr, workspace
    lib = load()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    grf = GaussianRF(2, s, alpha=2.5, tau=7, device=dev)
    w0, c0 = grf.sample(B, generator=gen), grf.sample(B, generator=gen)
    f = forcing(s, dev)
    M = N = s
    c_w, c_f, d_w, d_f, c_g, inv_lap = (t.to(dev) for t in ops.nsc2d_tables(M, N, visc, kappa, dt))
    nws = max(lib.rpde_nsc2d_ws_bytes(B, M, N), lib.rpde_ns2d_ws_bytes(6 * B, M, N))
    ws = workspace(nws, dev)
    st = stream_ptr()
    spec = lib.rpde_ns2d_spec_elems(B, M, N)
    S0 = torch.empty(2 * spec, dtype=torch.float32, device=dev)
    f_h = torch.empty(lib.rpde_ns2d_spec_elems(1, M, N), dtype=torch.float32, device=dev)
    g_h = torch.empty_like(f_h)
    check(lib.rpde_ns2d_rfft2(ptr(torch.cat([w0, c0])), ptr(S0), 2 * B, M, N, ws.data_ptr(), nws, st), "rfft2")
    check(lib.rpde_ns2d_rfft2(ptr(f), ptr(f_h), 1, M, N, ws.data_ptr(), nws, st), "rfft2")
    check(lib.rpde_ns2d_scale(ptr(f_h), ptr(c_g), ptr(g_h), 1, M, N, st), "scale")
    S, W = S0.clone(), S0[:spec].clone()
    D = torch.zeros(6 * spec, dtype=torch.float32, device=dev)
    P = torch.empty(6 * B, M, N, dtype=torch.float32, device=dev)

    def nsc_steps(n):
        check(lib.rpde_nsc2d_steps(ptr(S), ptr(g_h), 0, ptr(c_w), ptr(c_f), ptr(d_w), ptr(d_f), ptr(inv_lap), beta, B, M, N, n,
                                   ws.data_ptr(), nws, st), "nsc2d_steps")

    def ns_steps(n):
        check(lib.rpde_ns2d_steps(ptr(W), ptr(g_h), 0, ptr(c_w), ptr(c_f), ptr(inv_lap), B, M, N, n, ws.data_ptr(), nws, st), "ns2d_steps")

    def inverse(n):
        for _ in range(n):
            check(lib.rpde_ns2d_irfft2(ptr(D), ptr(P), 6 * B, M, N, ws.data_ptr(), nws, st), "irfft2")

    def forward(n):
        for _ in range(n):
            check(lib.rpde_ns2d_rfft2(ptr(P), ptr(D), 2 * B, M, N, ws.data_ptr(), nws, st), "rfft2")

    for fn in (nsc_steps, ns_steps, inverse, forward):                       # warm-up of every timed shape
        fn(3)
    torch.cuda.synchronize()
    S.copy_(S0)
    W.copy_(S0[:spec])
    t_nsc, t_ns = [], []
    for _ in range(repeats):                                                 # alternate the two solvers
        t_nsc += _windows(nsc_steps, steps, 1)
        t_ns += _windows(ns_steps, steps, 1)
    t_inv = _windows(inverse, steps, repeats)
    t_fwd = _windows(forward, steps, repeats)
    finite = bool(torch.isfinite(S).all()) and bool(torch.isfinite(W).all())
    nsc, ns, inv, fwd = _stats(t_nsc), _stats(t_ns), _stats(t_inv), _stats(t_fwd)
    return {"s": s, "B": B, "steps_per_window": steps, "windows": repeats, "visc": visc, "kappa": kappa, "beta": beta, "dt": dt,
            "nsc_step": nsc, "ns_step": ns, "nsc_over_ns": nsc["median_ms"] / ns["median_ms"],
            "nsc_inverse_6B": inv, "nsc_forward_2B": fwd,
            "nsc_pointwise_ms": nsc["median_ms"] - inv["median_ms"] - fwd["median_ms"],
            "states_finite": finite, "steps_taken": steps * repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", default="256x50,64x50")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nsc_gen_bench.py needs the GPU")
    lines = []
    for item in args.sizes.split(","):
        s, B = (int(v) for v in item.split("x"))
        r = bench(s, B, args.steps, args.repeats)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
