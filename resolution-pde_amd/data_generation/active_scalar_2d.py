"""2-D Navier-Stokes with an active scalar (Boussinesq) on the periodic unit square, generated on the GPU: a
concentration that the flow advects and that drives the flow back through buoyancy -- a concentration and a
two-component velocity, the three channels of the active-matter files the reference's dataloaders/active_matter_*.py
read, which cannot be regenerated (the reference has no generator for them).

    active_scalar_2d(w0, c0, f, visc, kappa, beta, T, delta_t, record_steps)
        -> fields [B, record_steps, 3, M, N] = (c, q, v), vorticity [B, record_steps, M, N], sol_t [record_steps]

with the schedule of data_generation/ns_2d.py; the solver is rpde.ops.nsc2d_solve (csrc/ns_solver.hip).  As a script it
writes --files .npz archives active_scalar_visc_<v>_kappa_<k>_beta_<b>_<i>.npz whose members carry the names of the HDF5
files' datasets ('/' separates groups; dataloaders/_store.py reads them as such), T = --record-steps:

    t0_fields/concentration [n, T+1, H, W]        frame 0 is the initial state
    t1_fields/velocity      [n, T+1, H, W, 2]     frame 0 is the velocity of w0
    t0_fields/vorticity     [n, T+1, H, W]
    scalars/visc, scalars/kappa, scalars/beta     the solver's parameters
    t                       [T+1]

    python data_generation/active_scalar_2d.py --resolution 64 --samples 100 --files 4 --out-dir data/active_scalar
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from data_generation.ns_2d import forcing, record_schedule  # noqa: E402
from data_generation.random_fields import GaussianRF  # noqa: E402


def active_scalar_2d(w0, c0, f, visc, kappa, beta, T, delta_t=1e-3, record_steps=1):
    """w0, c0 [B, M, N] initial vorticity and scalar, f [M, N] or [B, M, N] forcing on the vorticity, visc and kappa the
    two diffusivities, beta the buoyancy, T final time, delta_t the solver's step, record_steps snapshots.  GPU tensors;
    fp32 state and transforms."""
    _, record_time, times = record_schedule(T, delta_t, record_steps)
    from rpde import ops
    fields, vort = ops.nsc2d_solve(w0, c0, f, visc, kappa, beta, delta_t, record_steps * record_time, record_time)
    return fields, vort, torch.tensor(times, dtype=torch.float32, device=fields.device)


def file_name(visc: float, kappa: float, beta: float, i: int) -> str:
    return f"active_scalar_visc_{visc:g}_kappa_{kappa:g}_beta_{beta:g}_{i}.npz"


def main(argv: Optional[List[str]] = None) -> List[str]:
    ap = argparse.ArgumentParser(description="Generate 2-D active-scalar Navier-Stokes trajectories on the GPU")
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--samples", type=int, default=100, help="trajectories per file")
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--T", type=float, default=2.0)
    ap.add_argument("--dt", type=float, default=1e-3)
    ap.add_argument("--record-steps", type=int, default=20)
    ap.add_argument("--visc", type=float, default=1e-3)
    ap.add_argument("--kappa", type=float, default=1e-3)
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--files", type=int, default=1)
    ap.add_argument("--out-dir", required=True, help="directory of the .npz archives")
    args = ap.parse_args(argv)
    if args.samples < 1 or args.batch < 1 or args.files < 1:
        ap.error("--samples, --batch and --files must be positive")
    record_schedule(args.T, args.dt, args.record_steps)            # argument errors before any device work
    if not torch.cuda.is_available():
        raise RuntimeError("active_scalar_2d.py generates on the GPU; there is no CPU path")
    from rpde import ops
    dev = torch.device("cuda")
    s, n, T = args.resolution, args.samples, args.record_steps
    grf = GaussianRF(2, s, alpha=2.5, tau=7, device=dev)
    f = forcing(s, dev)
    gen = torch.Generator(device=dev).manual_seed(args.seed)       # one stream over every batch of every file
    os.makedirs(args.out_dir, exist_ok=True)
    paths = []
    for i in range(args.files):
        conc = np.empty((n, T + 1, s, s), dtype=np.float32)
        vel = np.empty((n, T + 1, s, s, 2), dtype=np.float32)
        vort = np.empty((n, T + 1, s, s), dtype=np.float32)
        t = None
        for c in range(0, n, args.batch):
            b = min(args.batch, n - c)
            w0 = grf.sample(b, generator=gen)
            c0 = grf.sample(b, generator=gen)
            fields, w, sol_t = active_scalar_2d(w0, c0, f, args.visc, args.kappa, args.beta, args.T, args.dt, T)
            first = ops.nsc2d_fields(w0, c0)
            conc[c:c + b, 0], conc[c:c + b, 1:] = c0.cpu().numpy(), fields[:, :, 0].cpu().numpy()
            vel[c:c + b, 0] = first[:, 1:].permute(0, 2, 3, 1).cpu().numpy()
            vel[c:c + b, 1:] = fields[:, :, 1:].permute(0, 1, 3, 4, 2).cpu().numpy()
            vort[c:c + b, 0], vort[c:c + b, 1:] = w0.cpu().numpy(), w.cpu().numpy()
            t = np.concatenate([np.zeros(1, dtype=np.float32), sol_t.cpu().numpy()])
        if not (np.isfinite(conc).all() and np.isfinite(vel).all()):
            raise RuntimeError(f"file {i}: the solution is not finite; lower --dt or --beta")
        path = os.path.join(args.out_dir, file_name(args.visc, args.kappa, args.beta, i))
        np.savez(path, **{"t0_fields/concentration": conc, "t1_fields/velocity": vel, "t0_fields/vorticity": vort,
                          "scalars/visc": np.float32(args.visc), "scalars/kappa": np.float32(args.kappa),
                          "scalars/beta": np.float32(args.beta), "t": t})
        print(f"[active_scalar_2d] wrote {path}: concentration {conc.shape}, velocity {vel.shape}", flush=True)
        paths.append(path)
    return paths


if __name__ == "__main__":
    main()
