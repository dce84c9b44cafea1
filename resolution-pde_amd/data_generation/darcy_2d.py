"""2-D Darcy flow data on the unit square, generated on the GPU: coefficient a -> solution u of -div(a grad u) = f with
u = 0 on the boundary (the steady-state benchmark the reference reads from piececonst_* .mat files through
dataloaders/load_data.py load_darcy_data_from_mat; it ships no generator).

    darcy_2d(a, f, iterations=24, tol=1e-6) -> u [B, s, s]

is rpde.ops.darcy2d_solve (csrc/darcy.hip): finite volumes on the s x s cell centres, conjugate gradients preconditioned
with the constant-coefficient operator.  piecewise_constant(g) thresholds a random field g at 0 into the two-valued
coefficient of the benchmark (12 where g >= 0, 3 elsewhere); with f = 1 this is the setting of the reference's files.
As a script it writes one archive with members coeff [N, s, s] and sol [N, s, s] -- the names load_darcy_data_from_mat
and dataloaders/darcy_loader.py read -- as .mat (scipy.io.savemat) or .npz:

    python data_generation/darcy_2d.py --resolution 32 --samples 1000 --batch 100 --out darcy_32.mat

and refuses to write anything if a sample's true residual |f - A u| / |f| exceeds 1e-5 (an unconverged solve: raise
--iterations, a contrast of 1 / 0.1 wants 32).  That residual has a floor no fp32 solution gets under: rounding u to
fp32 perturbs every cell by up to half an ulp, and A multiplies such noise by about 30 s^2 a.  For the 12 / 3 setting
the correctly rounded exact solution has 6e-6 at s = 32, 2.7e-5 at s = 64 and 1e-4 at s = 128 (float64 arithmetic on
rounded solutions), so the 1e-5 rule passes converged solves at s = 32 and refuses every grid from 64 up,
however many iterations are spent.  The solver itself is as accurate there (solution error 2e-8 .. 3e-8 at every size)."""
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

from data_generation.random_fields import GaussianRFNeumann  # noqa: E402

MAX_REL_RESIDUAL = 1e-5


def piecewise_constant(g: torch.Tensor, hi: float = 12.0, lo: float = 3.0) -> torch.Tensor:
    """hi where g >= 0, lo elsewhere, float32"""
    return torch.where(g >= 0, torch.full_like(g, float(hi)), torch.full_like(g, float(lo))).to(torch.float32)


def darcy_2d(a, f, iterations=24, tol=1e-6, return_info=False):
    """a [B, s, s] positive coefficient at the cell centres, f [s, s] or [B, s, s] right-hand side.  GPU tensors, fp32.
    return_info: (u, rel_residual [B], frozen_at [B]) instead of u."""
    from rpde import ops
    u, rel, frozen_at = ops.darcy2d_solve(a, f, iterations, tol)
    return (u, rel, frozen_at) if return_info else u


def check_args(resolution: int, samples: int, batch: int, hi: float, lo: float, forcing: float, iterations: int, out: str):
    """the script's argument errors as ValueError, host arithmetic only"""
    if resolution < 8 or resolution > 512 or resolution % 4:
        raise ValueError(f"--resolution must be a multiple of 4, 8 .. 512 (got {resolution})")
    if samples < 1 or batch < 1:
        raise ValueError("--samples and --batch must be positive")
    if not (hi > 0 and lo > 0 and np.isfinite(hi) and np.isfinite(lo)):
        raise ValueError(f"--hi and --lo must be positive and finite (got {hi}, {lo})")
    if not (np.isfinite(forcing) and forcing != 0):
        raise ValueError(f"--forcing must be finite and non-zero (got {forcing})")
    if iterations < 1:
        raise ValueError(f"--iterations must be positive (got {iterations})")
    if not out.endswith((".mat", ".npz")):
        raise ValueError("--out must end in .mat or .npz")


def main(argv: Optional[List[str]] = None) -> str:
    ap = argparse.ArgumentParser(description="Generate 2-D Darcy flow coefficient / solution pairs on the GPU")
    ap.add_argument("--resolution", type=int, default=32)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--hi", type=float, default=12.0)
    ap.add_argument("--lo", type=float, default=3.0)
    ap.add_argument("--forcing", type=float, default=1.0, help="the constant right-hand side f")
    ap.add_argument("--iterations", type=int, default=24)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True, help="output .mat or .npz (members coeff, sol)")
    args = ap.parse_args(argv)
    try:                                                       # argument errors before any device work
        check_args(args.resolution, args.samples, args.batch, args.hi, args.lo, args.forcing, args.iterations, args.out)
    except ValueError as e:
        ap.error(str(e))
    if not torch.cuda.is_available():
        raise RuntimeError("darcy_2d.py generates on the GPU; there is no CPU path")
    dev = torch.device("cuda")
    s = args.resolution
    grf = GaussianRFNeumann(s, alpha=2, tau=3, device=dev)
    f = torch.full((s, s), args.forcing, dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    coeff = np.empty((args.samples, s, s), dtype=np.float32)
    sol = np.empty((args.samples, s, s), dtype=np.float32)
    worst, hist = 0.0, {}
    for c in range(0, args.samples, args.batch):
        b = min(args.batch, args.samples - c)
        a = piecewise_constant(grf.sample(b, generator=gen), args.hi, args.lo)
        u, rel, frozen_at = darcy_2d(a, f, args.iterations, return_info=True)
        worst = max(worst, float(rel.max()))
        if not worst <= MAX_REL_RESIDUAL:
            raise RuntimeError(f"darcy_2d.py: a sample's residual |f - A u| / |f| is {worst:.2e} > {MAX_REL_RESIDUAL:.0e} "
                               f"after {args.iterations} iterations; nothing written (raise --iterations)")
        for k in frozen_at.cpu().tolist():
            hist[k] = hist.get(k, 0) + 1
        coeff[c:c + b] = a.cpu().numpy()
        sol[c:c + b] = u.cpu().numpy()
        print(f"[darcy_2d] {c + b}/{args.samples} samples", flush=True)
    if args.out.endswith(".mat"):
        from scipy.io import savemat
        savemat(args.out, {"coeff": coeff, "sol": sol})
    else:
        np.savez(args.out, coeff=coeff, sol=sol)
    print(f"[darcy_2d] wrote {args.out}: coeff {coeff.shape}, sol {sol.shape}; worst residual {worst:.2e}, "
          f"iterations to freeze {dict(sorted(hist.items()))}", flush=True)
    return args.out


if __name__ == "__main__":
    main()
