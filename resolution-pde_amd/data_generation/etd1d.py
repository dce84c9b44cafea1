"""What the three 1-D generator scripts (burgers_1d.py, ks_1d.py, kdv_1d.py) share: the snapshot arithmetic, the call
into the device integrator rpde.ops.etd1d_solve (csrc/etd1d.hip: ETDRK4 for u_t = L u - (1/2) (u^2)_x, pseudo-spectral,
2/3 de-aliasing; real tables for even symbols, complex ones when an odd derivative is present) and the handling of
--resolution / --resolutions.  Host arithmetic apart from `integrate`."""
from __future__ import annotations

from typing import List, Tuple

import torch


def snapshot_schedule(T: float, dt: float, record_steps: int) -> Tuple[int, int, List[float]]:
    """(steps, record_every, times): `record_steps` equally spaced snapshots over (0, T], the last at T, each a whole
    number of solver steps after the one before.  Raises ValueError when T / record_steps is not a whole number of
    steps of dt: the integrator's tables are built for one step size."""
    record_steps = int(record_steps)
    if record_steps < 1:
        raise ValueError(f"record_steps must be >= 1, got {record_steps}")
    if not (dt > 0 and T > 0):
        raise ValueError(f"T and dt must be positive, got T={T} dt={dt}")
    per = (float(T) / record_steps) / float(dt)
    every = int(round(per))
    if every < 1 or abs(per - every) > 1e-6 * max(1.0, per):
        raise ValueError(f"the snapshot interval T / record_steps = {float(T) / record_steps:g} is not a whole number of "
                         f"solver steps dt = {dt:g} ({per:.6f} steps)")
    return every * record_steps, every, [(c + 1) * every * float(dt) for c in range(record_steps)]


def integrate(u0: torch.Tensor, length: float, c2: float, c4: float, T: float, dt: float, record_steps: int,
              c1: float = 0.0, c3: float = 0.0):
    """u0 [B, N] on the GPU -> (sol [B, record_steps, N], sol_t [record_steps]) for the symbol c2 kappa^2 + c4 kappa^4
    + i (c1 kappa + c3 kappa^3).  With c1 = c3 = 0 the real tables and the real call, as before; otherwise the complex
    ones (rpde.ops.etd1d_tables_cx).  The schedule is checked before any device work."""
    steps, every, times = snapshot_schedule(T, dt, record_steps)
    if u0.dim() != 2:
        raise ValueError(f"expected u0 [B, N], got {tuple(u0.shape)}")
    from rpde import ops
    if c1 == 0.0 and c3 == 0.0:
        tables = ops.etd1d_tables(int(u0.shape[1]), length, c2, c4, dt)
    else:
        tables = ops.etd1d_tables_cx(int(u0.shape[1]), length, c1, c2, c3, c4, dt)
    sol = ops.etd1d_solve(u0, tables, steps, every)
    return sol, torch.tensor(times, dtype=torch.float32, device=sol.device)


def resolutions_of(args, ap) -> List[int]:
    """--resolutions a,b,c (one solve per entry, each simulated at its own resolution) or the single --resolution"""
    if args.resolutions:
        try:
            out = [int(v) for v in args.resolutions.split(",") if v.strip()]
        except ValueError:
            ap.error(f"--resolutions takes a comma-separated list of integers, got {args.resolutions!r}")
    else:
        out = [int(args.resolution)]
    if not out or len(set(out)) != len(out):
        ap.error("--resolutions needs distinct entries")
    for r in out:
        if r < 4 or r > 4096 or r % 2:
            ap.error(f"resolution {r}: must be even, 4 .. 4096")
    return out
