"""What the three 1-D generator scripts (burgers_1d.py, ks_1d.py, kdv_1d.py) share: the snapshot arithmetic, the call
into the device integrator rpde.ops.etd1d_solve (csrc/etd1d.hip: ETDRK4 for u_t = L u - (1/2) (u^2)_x, pseudo-spectral,
2/3 de-aliasing; real tables for even symbols, complex ones when an odd derivative is present), the handling of
--resolution / --resolutions, and the script that ks_1d.py and kdv_1d.py are: its arguments (add_trajectory_arguments)
and its body (write_trajectories).  Host arithmetic apart from `integrate` and the solves of `write_trajectories`."""
from __future__ import annotations

import os
from typing import List, Tuple

import numpy as np
import torch

SPLITS = ("train", "valid", "test")
_SPLIT_STREAM = {"train": 0, "valid": 100003, "test": 200003}


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


def check_samples(args, ap) -> None:
    if args.samples < 1 or args.batch < 1 or args.batch > 65535:
        ap.error("--samples and --batch must be positive, --batch at most 65535")


def ks_schedule(et: float, nt: int, nte: int, dt: float):
    """(steps, record_every, times [nt]) of nt snapshots over [0, et] with the first at 0; nte <= nt of them are kept"""
    nt, nte = int(nt), int(nte)
    if nt < 2:
        raise ValueError(f"nt counts the initial condition: at least 2, got {nt}")
    if nte < 2 or nte > nt:
        raise ValueError(f"nte must be 2 .. nt = {nt}, got {nte}")
    steps, every, times = snapshot_schedule(et, dt, nt - 1)
    return steps, every, [0.0] + times


def add_trajectory_arguments(ap) -> None:
    """the arguments ks_1d.py and kdv_1d.py share, after the script's own: nt equally spaced snapshots over [0, et], the
    initial condition first, of which the last nte are kept; one archive per resolution and split"""
    ap.add_argument("--L", type=float, default=64.0)
    ap.add_argument("--lmax", type=int, default=8)
    ap.add_argument("--et", type=float, default=5.0, help="end time")
    ap.add_argument("--nte", type=int, default=51, help="snapshots kept (the last nte of nt)")
    ap.add_argument("--nt", type=int, default=51, help="snapshots over [0, et], the initial condition first")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--resolutions", default="", help="comma-separated: one solve per entry, each at its own resolution")
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--samples", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--split", choices=SPLITS, default="train")
    ap.add_argument("--flat", action="store_true", help="write straight into --out (one resolution)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True, help="output folder")


def trajectory_resolutions(args, ap) -> List[int]:
    resolutions = resolutions_of(args, ap)
    if args.flat and len(resolutions) != 1:
        ap.error("--flat holds one resolution")
    return resolutions


def write_trajectories(name: str, args, ap, resolutions: List[int], initial, solve, path_of, written=None) -> List[str]:
    """The body of script `name` over the arguments of add_trajectory_arguments.  Per resolution X, with a host generator
    seeded by seed, X and the split: batches u0 = initial(b, X, generator) [b, X] float32 on the host, their nt - 1 later
    snapshots solve(u0 on the GPU, X) [b, nt - 1, X] on the host, and the archive path_of(X) with the members the
    scripts' docstrings list; written(X, path) after it.  Returns the paths."""
    try:                                                               # argument errors before any device work
        steps, every, times = ks_schedule(args.et, args.nt, args.nte, args.dt)
    except ValueError as e:
        ap.error(str(e))
    if not torch.cuda.is_available():
        raise RuntimeError(f"{name}.py generates on the GPU; there is no CPU path")
    nt, nte, s = args.nt, args.nte, args.split
    t = np.asarray(times[nt - nte:], dtype=np.float32)
    paths = []
    for X in resolutions:
        gen = torch.Generator().manual_seed(args.seed + X + _SPLIT_STREAM[s])
        u = np.empty((args.samples, nte, X), dtype=np.float32)
        for c in range(0, args.samples, args.batch):
            b = min(args.batch, args.samples - c)
            u0 = initial(b, X, gen)
            full = torch.cat([u0[:, None, :], solve(u0.cuda(), X)], dim=1)         # [b, nt, X]
            u[c:c + b] = full[:, nt - nte:].numpy()
            print(f"[{name}] {s} resolution {X}: {c + b}/{args.samples} samples", flush=True)
        path = path_of(X)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.savez(path, **{f"{s}/pde_{nte}-{X}": u, f"{s}/t": t,
                          f"{s}/x": (np.arange(X, dtype=np.float64) * (args.L / X)).astype(np.float32),
                          f"{s}/dx": np.float32(args.L / X), f"{s}/dt": np.float32(every * args.dt)})
        if written is not None:
            written(X, path)
        print(f"[{name}] wrote {path}: {s}/pde_{nte}-{X} {u.shape}", flush=True)
        paths.append(path)
    return paths
