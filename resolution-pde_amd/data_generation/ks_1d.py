"""1-D Kuramoto-Sivashinsky data on a periodic interval, generated on the GPU:

    u_t + u u_x + u_xx + nu u_xxxx = 0   on [0, L)

    ks_1d(u0, viscosity, length, T, dt, record_steps) -> sol [B, record_steps, N], sol_t [record_steps]

integrates with the device ETDRK4 integrator (rpde.ops.etd1d_solve, csrc/etd1d.hip; symbol kappa^2 - nu kappa^4).  The
initial condition is sum_{j<10} A_j sin(2 pi l_j x / L + phi_j), A in U(-1/2, 1/2), l in {1 .. lmax}, phi in U(0, 2 pi),
drawn on the host from a seeded generator in float64 and rounded once.  No per-trajectory jitter of the domain.

As a script its parameters are named after the path dataloaders/ks_naive_true_multires.py builds from them:
nt equally spaced snapshots over [0, et], the first being the initial condition, of which the last nte are kept.

    <out>/res_<resolution>/visc_<viscosity>_L<L>_lmax<lmax>_et<et>_nte<nte>_nt<nt>/KS_train_<samples>.npz

holds ``train/pde_<nte>-<X>`` [samples, nte, X] float32, ``train/t`` [nte], ``train/x`` [X], ``train/dx``, ``train/dt``
(the snapshot interval).  --split valid | test writes KS_valid.npz / KS_test.npz into the same folder with the group
named after the split; --flat puts the files straight into <out>, as ks_naive_markov.ks_markov_dataset wants them:

    python data_generation/ks_1d.py --out data/ks_gen --resolutions 256,192,160 --samples 2048
    python data_generation/ks_1d.py --out data/ks_gen/flat --flat --split valid --samples 128

--resolutions runs one solve per entry, each SIMULATED at that resolution, with the seed `seed + resolution` (and a
different stream per split); a resolution whose kept modes are all linearly unstable is refused (at the defaults:
below 138 points).  KS is chaotic: trajectories generated in fp32 are samples of the attractor, not
bit-reproductions of a float64 run (a float32 torch.fft run of the same scheme is of the order of 1e-1 from its float64
run at T = 5: 0.16 rel-L2 over eight trajectories at 256 points)."""
from __future__ import annotations

import argparse
import math
import os
import sys
from typing import List, Optional

import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from data_generation.etd1d import (add_trajectory_arguments, check_samples, integrate, ks_schedule,  # noqa: E402,F401
                                   trajectory_resolutions, write_trajectories)


def ks_1d(u0, viscosity, length, T, dt=0.01, record_steps=1):
    """u0 [B, N] initial condition, viscosity the coefficient of u_xxxx, length the period, T final time, dt the solver's
    step, record_steps equally spaced snapshots over (0, T].  GPU tensors; fp32 state and transforms."""
    if not viscosity > 0:
        raise ValueError(f"viscosity must be positive, got {viscosity}")
    return integrate(u0, length, 1.0, -float(viscosity), T, dt, record_steps)


def ks_initial_condition(samples: int, X: int, length: float, lmax: int, generator: torch.Generator) -> torch.Tensor:
    """[samples, X] float32 on the host: sum_{j<10} A_j sin(2 pi l_j x / L + phi_j) on x = i L / X, formed in float64 from
    a host generator and rounded once"""
    A = torch.rand(samples, 10, generator=generator, dtype=torch.float64) - 0.5
    l = torch.randint(1, int(lmax) + 1, (samples, 10), generator=generator).to(torch.float64)
    phi = 2.0 * math.pi * torch.rand(samples, 10, generator=generator, dtype=torch.float64)
    x = torch.arange(X, dtype=torch.float64) * (float(length) / X)
    u = (A[..., None] * torch.sin(2.0 * math.pi * l[..., None] * x / float(length) + phi[..., None])).sum(1)
    return u.to(torch.float32)


def damped_modes(X: int, length: float, viscosity: float) -> int:
    """how many of the modes the 2/3 rule keeps are linearly damped (kappa_n^2 > 1 / nu).  With none the energy that the
    unstable band feeds in has nowhere to go."""
    kept = int((2.0 / 3.0) * (X // 2))
    return sum(1 for n in range(1, kept + 1) if (2.0 * math.pi * n / float(length)) ** 2 > 1.0 / float(viscosity))


def ks_path(out: str, split: str, resolution: int, viscosity: float, L: float, lmax: int, et: float, nte: int, nt: int,
            samples: int, flat: bool = False) -> str:
    """the archive of one resolution and split.  The folder is the one ks_naive_true_multires looks in (its own path
    rule, with .npz in place of .h5); --flat drops the folders"""
    from dataloaders.ks_naive_true_multires import _ks_file
    train = os.path.splitext(_ks_file(out, resolution, viscosity, L, lmax, et, nte, nt, samples))[0] + ".npz"
    folder = out if flat else os.path.dirname(train)
    return os.path.join(folder, os.path.basename(train) if split == "train" else f"KS_{split}.npz")


def main(argv: Optional[List[str]] = None) -> List[str]:
    ap = argparse.ArgumentParser(description="Generate 1-D Kuramoto-Sivashinsky trajectories on the GPU")
    ap.add_argument("--viscosity", type=float, default=0.05)
    add_trajectory_arguments(ap)
    args = ap.parse_args(argv)
    check_samples(args, ap)
    if not (args.viscosity > 0 and args.L > 0 and args.lmax >= 1):
        ap.error("--viscosity and --L must be positive, --lmax at least 1")
    resolutions = trajectory_resolutions(args, ap)
    for X in resolutions:
        if damped_modes(X, args.L, args.viscosity) < 1:
            ap.error(f"resolution {X} is too coarse for viscosity {args.viscosity:g} on L = {args.L:g}: every mode the "
                     f"2/3 rule keeps is linearly unstable (kappa^2 < 1/nu), so nothing dissipates and the run blows up")

    def path_of(X):
        return ks_path(args.out, args.split, X, args.viscosity, args.L, args.lmax, args.et, args.nte, args.nt, args.samples,
                       args.flat)

    def found_by_loader(X, path):
        if args.split == "train" and not args.flat:                    # the loader's own lookup finds what was written
            from dataloaders.ks_naive_true_multires import _ks_path
            found = _ks_path(args.out, X, args.viscosity, args.L, args.lmax, args.et, args.nte, args.nt, args.samples)
            if found != path:
                raise RuntimeError(f"ks_naive_true_multires reads {found} for resolution {X}, not {path} "
                                   "(an .h5 file of the same stem takes precedence over the .npz archive)")

    return write_trajectories(
        "ks_1d", args, ap, resolutions,
        lambda b, X, gen: ks_initial_condition(b, X, args.L, args.lmax, gen),
        lambda u0, X: ks_1d(u0, args.viscosity, args.L, args.et, args.dt, args.nt - 1)[0].cpu(),
        path_of, found_by_loader)


if __name__ == "__main__":
    main()
