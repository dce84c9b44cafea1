"""1-D viscous Burgers data on a periodic interval, generated on the GPU:

    u_t + u u_x = (nu / pi) u_xx   on [-length/2, length/2),   length = 2 by default

nu is the data set's "viscosity" name (PDEBench's convention, kept so that the loaders' folder and file names apply); the
diffusion coefficient is nu_eff = nu / pi.

    burgers_1d(u0, nu_eff, length, T, dt, record_steps) -> sol [B, record_steps, N], sol_t [record_steps]

integrates with the device ETDRK4 integrator (rpde.ops.etd1d_solve, csrc/etd1d.hip; symbol -nu_eff kappa^2).  This is a
RESOLVED spectral method, not a shock-capturing one: nu / pi has to be resolvable on the grid -- the front of width
~ nu_eff / |u| must span a few grid cells -- or the spectrum piles up at the de-aliasing cut and the solution rings.
PDEBench's nu = 0.001 set at 1024 points is not resolvable this way; the defaults here (nu = 0.1) are, down to a few
dozen points.  The initial condition is a periodic Gaussian random field, GaussianRF1d(alpha = 2, tau = 5, sigma = 25),
not PDEBench's sum of sines.

As a script it writes, per resolution,

    <out>/burgers_<resolution>_<viscosity>/1D_Burgers_Sols_Nu<viscosity>.npz

with members ``tensor`` [samples, T, X] float32 (the initial condition first), ``x-coordinate`` [X] (cell centres
-length/2 + (i + 1/2) length / X) and ``t-coordinate`` [T] -- what dataloaders/burger_naive_markov.py (saved_folder = that
folder) and burger_naive_true_multires.py (saved_folder = <out>) read:

    python data_generation/burgers_1d.py --out data/burgers_gen --resolutions 256,128,64 --samples 1000

--resolutions runs one solve per entry, each SIMULATED at that resolution (true multi-resolution data, not a subsampled
fine run), with the seed `seed + resolution`."""
from __future__ import annotations

import argparse
import math
import os
import sys
from typing import List, Optional

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from data_generation.etd1d import check_samples, integrate, resolutions_of, snapshot_schedule  # noqa: E402
from data_generation.random_fields import GaussianRF1d  # noqa: E402

IC_ALPHA, IC_TAU, IC_SIGMA = 2.0, 5.0, 25.0


def burgers_1d(u0, nu_eff, length, T, dt=1e-3, record_steps=1):
    """u0 [B, N] initial condition, nu_eff the diffusion coefficient, length the period, T final time, dt the solver's
    step, record_steps equally spaced snapshots over (0, T].  GPU tensors; fp32 state and transforms."""
    if not nu_eff >= 0:
        raise ValueError(f"nu_eff must be non-negative, got {nu_eff}")
    return integrate(u0, length, -float(nu_eff), 0.0, T, dt, record_steps)


def burgers_path(out: str, resolution: int, viscosity: float) -> str:
    """the archive of one resolution, where burger_naive_true_multires._burgers_path looks for it"""
    return os.path.join(out, f"burgers_{resolution}_{viscosity}", f"1D_Burgers_Sols_Nu{viscosity}.npz")


def main(argv: Optional[List[str]] = None) -> List[str]:
    ap = argparse.ArgumentParser(description="Generate 1-D viscous Burgers trajectories on the GPU")
    ap.add_argument("--viscosity", type=float, default=0.1, help="nu; the diffusion coefficient is nu / pi")
    ap.add_argument("--length", type=float, default=2.0)
    ap.add_argument("--T", type=float, default=2.0)
    ap.add_argument("--snapshots", type=int, default=201, help="time levels in the archive, the initial condition first")
    ap.add_argument("--dt", type=float, default=1e-3)
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--resolutions", default="", help="comma-separated: one solve per entry, each at its own resolution")
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=500)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True, help="output folder")
    args = ap.parse_args(argv)
    check_samples(args, ap)
    if args.snapshots < 2:
        ap.error("--snapshots counts the initial condition: at least 2")
    if not (args.viscosity > 0 and args.length > 0):
        ap.error("--viscosity and --length must be positive")
    resolutions = resolutions_of(args, ap)
    try:                                                               # argument errors before any device work
        snapshot_schedule(args.T, args.dt, args.snapshots - 1)
    except ValueError as e:
        ap.error(str(e))
    if not torch.cuda.is_available():
        raise RuntimeError("burgers_1d.py generates on the GPU; there is no CPU path")
    dev = torch.device("cuda")
    written = []
    for X in resolutions:
        grf = GaussianRF1d(X, alpha=IC_ALPHA, tau=IC_TAU, sigma=IC_SIGMA, device=dev)
        gen = torch.Generator(device=dev).manual_seed(args.seed + X)
        u = np.empty((args.samples, args.snapshots, X), dtype=np.float32)
        t = np.zeros(args.snapshots, dtype=np.float32)
        for c in range(0, args.samples, args.batch):
            b = min(args.batch, args.samples - c)
            u0 = grf.sample(b, generator=gen)
            sol, sol_t = burgers_1d(u0, args.viscosity / math.pi, args.length, args.T, args.dt, args.snapshots - 1)
            u[c:c + b, 0] = u0.cpu().numpy()
            u[c:c + b, 1:] = sol.cpu().numpy()
            t[1:] = sol_t.cpu().numpy()
            print(f"[burgers_1d] resolution {X}: {c + b}/{args.samples} samples", flush=True)
        x = (-0.5 * args.length + (np.arange(X, dtype=np.float64) + 0.5) * (args.length / X)).astype(np.float32)
        path = burgers_path(args.out, X, args.viscosity)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.savez(path, **{"tensor": u, "x-coordinate": x, "t-coordinate": t})
        print(f"[burgers_1d] wrote {path}: tensor {u.shape}", flush=True)
        written.append(path)
    return written


if __name__ == "__main__":
    main()
