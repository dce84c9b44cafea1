"""1-D Korteweg-de Vries (and KdV-Burgers) data on a periodic interval, generated on the GPU:

    u_t + u u_x + delta u_xxx = nu u_xx   on [0, L)

    kdv_1d(u0, length, T, dt, record_steps, dispersion=delta, viscosity=nu) -> sol [B, record_steps, N], sol_t [record_steps]

integrates with the device ETDRK4 integrator on its complex tables (rpde.ops.etd1d_tables_cx / etd1d_solve,
csrc/etd1d.hip; symbol -nu kappa^2 + i delta kappa^3, the third derivative handled exactly by the exponentials).  With
nu = 0 nothing dissipates: mean and energy are conserved and fine scales do not decay, which is what this equation adds
to the Burgers and Kuramoto-Sivashinsky sets.  The initial condition is `--amplitude` times the KS one
(ks_1d.ks_initial_condition: ten sines of random amplitude, wavenumber l <= lmax and phase).

As a script it has the shape of ks_1d.py: nt equally spaced snapshots over [0, et], the first being the initial
condition, of which the last nte are kept, written as

    <out>/res_<resolution>/KdV_train_<samples>.npz        (--flat: <out>/KdV_train_<samples>.npz)

holding ``train/pde_<nte>-<X>`` [samples, nte, X] float32, ``train/t`` [nte], ``train/x`` [X], ``train/dx``, ``train/dt``
(the snapshot interval); --split valid | test writes KdV_valid.npz / KdV_test.npz beside it with the group named after
the split.  Every such folder is a `saved_folder` of dataloaders.ks_naive_markov.ks_markov_dataset, which tells the
split from the file name (conf/dataset/kdv/kdv_generated.yaml):

    python data_generation/kdv_1d.py --out data/kdv_gen/flat --flat --resolution 256 --samples 2048
    python data_generation/kdv_1d.py --out data/kdv_gen --resolutions 256,192,128 --samples 2048

--resolutions runs one solve per entry, each SIMULATED at that resolution, with the seed `seed + resolution` (and a
different stream per split), as ks_1d.py does.

The defaults (L = 64, lmax = 8, amplitude 2, delta = 1, nu = 0, et = 5 in 50 intervals, dt = 0.01, 256 points) are this
project's own choice, not taken from another generator.  What they were chosen for, measured with the float64
restatement of the scheme (tests/etd1d_cx_ref.py) on eight trajectories at T = 5: both terms shape the answer (dropping
the nonlinear term moves it by 1.3 in relative L2, dropping the dispersion by 1.1); the step is not what limits the
data (dt = 0.01 against dt = 0.0025: 7e-7, the float32 run of the same scheme against float64: 1.3e-5); the grid
resolves it (the upper quarter of the modes the 2/3 rule keeps holds 1e-8 of the energy at 256 points, 6e-5 at 128,
3e-2 at 64, where the tail is part of the data a coarse simulation gives); |u| stays below 7.  Amplitude 4 at 256 points
brings the step error to 1e-3 -- halve dt there.  A batch with a non-finite value aborts the run."""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from data_generation.etd1d import (add_trajectory_arguments, check_samples, integrate, trajectory_resolutions,  # noqa: E402
                                   write_trajectories)
from data_generation.ks_1d import ks_initial_condition  # noqa: E402


def kdv_1d(u0, length, T, dt=0.01, record_steps=1, dispersion=1.0, viscosity=0.0):
    """u0 [B, N] initial condition, length the period, T final time, dt the solver's step, record_steps equally spaced
    snapshots over (0, T]; dispersion the coefficient of u_xxx, viscosity that of u_xx on the right (0: KdV, > 0:
    KdV-Burgers).  GPU tensors; fp32 state and transforms."""
    if not viscosity >= 0:
        raise ValueError(f"viscosity must not be negative, got {viscosity}")
    if dispersion == 0:
        raise ValueError("dispersion must not be zero (burgers_1d integrates the equation without it)")
    return integrate(u0, length, -float(viscosity), 0.0, T, dt, record_steps, c3=float(dispersion))


def kdv_path(out: str, split: str, resolution: int, samples: int, flat: bool = False) -> str:
    """the archive of one resolution and split: <out>/res_<resolution>/, or <out> itself with --flat"""
    folder = out if flat else os.path.join(out, f"res_{resolution}")
    return os.path.join(folder, f"KdV_train_{samples}.npz" if split == "train" else f"KdV_{split}.npz")


def main(argv: Optional[List[str]] = None) -> List[str]:
    ap = argparse.ArgumentParser(description="Generate 1-D Korteweg-de Vries trajectories on the GPU")
    ap.add_argument("--dispersion", type=float, default=1.0, help="coefficient of u_xxx")
    ap.add_argument("--viscosity", type=float, default=0.0, help="coefficient of u_xx on the right (KdV-Burgers when > 0)")
    ap.add_argument("--amplitude", type=float, default=2.0, help="factor on the KS initial condition")
    add_trajectory_arguments(ap)
    args = ap.parse_args(argv)
    check_samples(args, ap)
    if not (args.L > 0 and args.lmax >= 1 and args.amplitude > 0):
        ap.error("--L and --amplitude must be positive, --lmax at least 1")
    if args.dispersion == 0 or not args.viscosity >= 0:
        ap.error("--dispersion must not be zero, --viscosity not negative")
    resolutions = trajectory_resolutions(args, ap)

    def solve(u0, X):
        sol = kdv_1d(u0, args.L, args.et, args.dt, args.nt - 1, args.dispersion, args.viscosity)[0].cpu()
        if not bool(torch.isfinite(sol).all()):
            raise RuntimeError(f"kdv_1d: non-finite values at resolution {X} with dt = {args.dt:g} (amplitude "
                               f"{args.amplitude:g}, dispersion {args.dispersion:g}): the step is too long for this "
                               "amplitude -- lower --dt")
        return sol

    return write_trajectories(
        "kdv_1d", args, ap, resolutions,
        lambda b, X, gen: (args.amplitude * ks_initial_condition(b, X, args.L, args.lmax, gen).double()).float(),
        solve, lambda X: kdv_path(args.out, args.split, X, args.samples, args.flat))


if __name__ == "__main__":
    main()
