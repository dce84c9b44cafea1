"""2-D Navier-Stokes vorticity data on the periodic unit square, generated on the GPU (reference:
data_generation/ns_2d.py, written for the removed torch.rfft / irfft and so not runnable on a current torch).

    navier_stokes_2d(w0, f, visc, T, delta_t, record_steps) -> sol [B, M, N, record_steps], sol_t [record_steps]

keeps the reference's signature and return shapes; the solver is rpde.ops.ns2d_solve (csrc/ns_solver.hip).  As a
script it writes one .npz archive with members a [N, s, s] (initial vorticity), u [N, s, s, T] (snapshots) and t [T],
which dataloaders/ns_naive_markov.py reads as it is:

    python data_generation/ns_2d.py --resolution 64 --samples 100 --batch 50 --out ns_64.npz
"""
from __future__ import annotations

import argparse
import math
import os
import sys
from typing import List, Optional, Tuple

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from data_generation.random_fields import GaussianRF  # noqa: E402


def record_schedule(T: float, delta_t: float, record_steps: int) -> Tuple[int, int, List[float]]:
    """(steps, record_time, times) with the reference's expressions: steps = ceil(T / delta_t), record_time =
    floor(steps / record_steps), a snapshot after step j when (j + 1) % record_time == 0, its time the running sum of
    delta_t.  Host arithmetic only.  Only the first record_steps snapshots are kept (the reference's arrays hold no
    more), so the steps after the last of them are not taken."""
    record_steps = int(record_steps)
    if record_steps < 1:
        raise ValueError(f"record_steps must be >= 1, got {record_steps}")
    if not (delta_t > 0 and T > 0):
        raise ValueError(f"T and delta_t must be positive, got T={T} delta_t={delta_t}")
    steps = math.ceil(T / delta_t)
    record_time = math.floor(steps / record_steps)
    if record_time < 1:
        raise ValueError(f"{steps} steps cannot hold {record_steps} snapshots: lower record_steps or delta_t")
    times, t = [], 0.0
    for j in range(record_steps * record_time):
        t += delta_t
        if (j + 1) % record_time == 0:
            times.append(t)
    return steps, record_time, times


def navier_stokes_2d(w0, f, visc, T, delta_t=1e-4, record_steps=1):
    """w0 [B, M, N] initial vorticity, f [M, N] or [B, M, N] forcing, visc = 1/Re, T final time, delta_t the solver's
    step, record_steps snapshots.  GPU tensors; fp32 state and transforms."""
    steps, record_time, times = record_schedule(T, delta_t, record_steps)
    from rpde import ops
    sol = ops.ns2d_solve(w0, f, visc, delta_t, record_steps * record_time, record_time)
    sol_t = torch.tensor(times, dtype=torch.float32, device=sol.device)
    return sol, sol_t


def forcing(s: int, device) -> torch.Tensor:
    """0.1 (sin 2 pi (x + y) + cos 2 pi (x + y)) on the s x s grid of [0, 1)^2, formed in float64"""
    t = torch.arange(s, dtype=torch.float64) / s
    xy = t.view(s, 1) + t.view(1, s)
    return (0.1 * (torch.sin(2 * math.pi * xy) + torch.cos(2 * math.pi * xy))).to(torch.float32).to(device)


def main(argv: Optional[List[str]] = None) -> str:
    ap = argparse.ArgumentParser(description="Generate 2-D Navier-Stokes vorticity trajectories on the GPU")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--viscosity", type=float, default=1e-4)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--T", type=float, default=3.2)
    ap.add_argument("--dt", type=float, default=1e-4)
    ap.add_argument("--record-steps", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True, help="output .npz (members a, u, t)")
    args = ap.parse_args(argv)
    if args.samples < 1 or args.batch < 1:
        ap.error("--samples and --batch must be positive")
    if not args.out.endswith(".npz"):
        ap.error("--out must end in .npz")
    record_schedule(args.T, args.dt, args.record_steps)            # argument errors before any device work
    if not torch.cuda.is_available():
        raise RuntimeError("ns_2d.py generates on the GPU; there is no CPU path")
    dev = torch.device("cuda")
    s = args.resolution
    grf = GaussianRF(2, s, alpha=2.5, tau=7, device=dev)
    f = forcing(s, dev)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    a = np.empty((args.samples, s, s), dtype=np.float32)
    u = np.empty((args.samples, s, s, args.record_steps), dtype=np.float32)
    t = None
    for c in range(0, args.samples, args.batch):
        b = min(args.batch, args.samples - c)
        w0 = grf.sample(b, generator=gen)
        sol, sol_t = navier_stokes_2d(w0, f, args.viscosity, args.T, args.dt, args.record_steps)
        a[c:c + b] = w0.cpu().numpy()
        u[c:c + b] = sol.cpu().numpy()
        t = sol_t.cpu().numpy()
        print(f"[ns_2d] {c + b}/{args.samples} samples", flush=True)
    np.savez(args.out, a=a, u=u, t=t)
    print(f"[ns_2d] wrote {args.out}: a {a.shape}, u {u.shape}, t {t.shape}", flush=True)
    return args.out


if __name__ == "__main__":
    main()
