"""Time one step of the 1-D exponential-time-differencing generator (csrc/etd1d.hip) against the same step written with
torch.fft (rocFFT) on the same GPU.  Does not touch bench.py.

    python profiles/etd1d_gen_bench.py [--steps 50] [--repeats 7] [--sizes 256x512,1024x256] [--out profiles/etd1d_gen_bench.json]
    python profiles/etd1d_gen_bench.py --sizes "" --kdv-sizes 256x512,1024x512 --out profiles/etd1d_gen_bench_kdv.json

Per (resolution N, batch B), Kuramoto-Sivashinsky with the generator script's defaults: warm-up (plans, code objects,
rocFFT's own plans), then `repeats` windows of `steps` steps each between device events, alternating the two
implementations; reported are the median, minimum and maximum of the windows in ms per step.  The parts of one step are
timed the same way through the C ABI: the four inverse and the four forward transforms of a step on their own, and the
pointwise rest (4 x k_etd_square + the four k_etd_stage kernels) as the difference.  A last figure compares the two
implementations' states after the timed steps.  The KdV rows (--kdv-sizes) time the complex-table step
(rpde_etd1d_steps_cx, Korteweg-de Vries with kdv_1d.py's defaults) against the real-table step (KS) at the same size,
the two alternating, and report their ratio: what the complex stage kernels add to a step.  Needs the GPU: there is no
fallback."""
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

LAUNCHES_PER_STEP = 16          # per stage: synthesis, k_etd_square, analysis, k_etd_stage<S>
TRANSFORMS_PER_STEP = 4         # of each direction


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


class TorchStep:
    """the same step with torch.fft in fp32; tables as the device path rounds them"""

    def __init__(self, N, tables, dev):
        K = N // 2 + 1
        self.E, self.E2, self.Q, self.f1, self.f2, self.f3, g = (t[:K].to(dev) for t in tables)
        self.ig = torch.complex(torch.zeros_like(g), g)
        self.N = N

    def nl(self, w):
        return self.ig * torch.fft.rfft(torch.fft.irfft(w, n=self.N) ** 2)

    def run(self, v, steps):
        for _ in range(steps):
            Nv = self.nl(v)
            a = self.E2 * v + self.Q * Nv
            Na = self.nl(a)
            b = self.E2 * v + self.Q * Na
            Nb = self.nl(b)
            c = self.E2 * a + self.Q * (2.0 * Nb - Nv)
            Nc = self.nl(c)
            v = self.E * v + self.f1 * Nv + 2.0 * self.f2 * (Na + Nb) + self.f3 * Nc
        return v


def bench(N, B, steps, repeats, viscosity=0.05, length=64.0, lmax=8, dt=0.01):
    from data_generation.ks_1d import ks_initial_condition
    from rpde import ops
    from rpde._lib import check, load, ptr, stream_ptr, workspace
    lib = load()
    dev = torch.device("cuda")
    u0 = ks_initial_condition(B, N, length, lmax, torch.Generator().manual_seed(0)).to(dev)
    tables = ops.etd1d_tables(N, length, 1.0, -viscosity, dt)
    tabs = [t.to(dev) for t in tables]
    nws = lib.rpde_etd1d_ws_bytes(B, N)
    ws = workspace(nws, dev)
    st = stream_ptr()
    U0 = torch.empty(lib.rpde_etd1d_spec_elems(B, N), dtype=torch.float32, device=dev)
    check(lib.rpde_etd1d_rfft(ptr(u0), ptr(U0), B, N, st), "rfft")
    U = U0.clone()
    S = U0.clone()
    P = torch.empty(B, N, dtype=torch.float32, device=dev)

    def hip_steps(n):
        check(lib.rpde_etd1d_steps(ptr(U), *(ptr(t) for t in tabs), B, N, n, ws.data_ptr(), nws, st), "steps")

    def hip_inverse(n):
        for _ in range(n * TRANSFORMS_PER_STEP):
            check(lib.rpde_etd1d_irfft(ptr(S), ptr(P), B, N, st), "irfft")

    def hip_forward(n):
        for _ in range(n * TRANSFORMS_PER_STEP):
            check(lib.rpde_etd1d_rfft(ptr(P), ptr(S), B, N, st), "rfft")

    ref = TorchStep(N, tables, dev)
    V0 = torch.fft.rfft(u0)
    state = {"v": V0}

    def torch_steps(n):
        state["v"] = ref.run(state["v"], n)

    for fn in (hip_steps, torch_steps, hip_inverse, hip_forward):          # warm-up of every timed shape
        fn(3)
    torch.cuda.synchronize()
    U.copy_(U0)
    S.copy_(U0)
    state["v"] = V0
    t_hip, t_torch = [], []
    for _ in range(repeats):                                                 # alternate the two implementations
        t_hip += _windows(hip_steps, steps, 1)
        t_torch += _windows(torch_steps, steps, 1)
    t_inv = _windows(hip_inverse, steps, repeats)
    S.copy_(U0)
    t_fwd = _windows(hip_forward, steps, repeats)
    # both advanced repeats * steps steps from the same state: compare them in physical space (KS is chaotic: this
    # distance grows with the number of steps and says only that the two run the same problem)
    u_hip = torch.empty(B, N, dtype=torch.float32, device=dev)
    check(lib.rpde_etd1d_irfft(ptr(U), ptr(u_hip), B, N, st), "irfft")
    u_t = torch.fft.irfft(state["v"], n=N)
    diff = float((u_hip - u_t).norm() / u_t.norm())
    hip, tor, inv, fwd = _stats(t_hip), _stats(t_torch), _stats(t_inv), _stats(t_fwd)
    pointwise = hip["median_ms"] - inv["median_ms"] - fwd["median_ms"]
    return {"N": N, "B": B, "pde": "ks", "steps_per_window": steps, "windows": repeats, "viscosity": viscosity,
            "length": length, "dt": dt, "launches_per_step": LAUNCHES_PER_STEP,
            "hip_step": hip, "torch_fft_step": tor, "hip_over_torch": hip["median_ms"] / tor["median_ms"],
            "hip_us_per_launch": 1e3 * hip["median_ms"] / LAUNCHES_PER_STEP,
            "hip_inverse_x4": inv, "hip_forward_x4": fwd, "hip_pointwise_ms": pointwise,
            "hip_pointwise_share": pointwise / hip["median_ms"],
            "state_bytes": 4 * int(U0.numel()), "finite": bool(torch.isfinite(u_hip).all()),
            "rel_l2_hip_vs_torch_after": diff, "steps_compared": steps * repeats}


def bench_kdv(N, B, steps, repeats, length=64.0, lmax=8, dt=0.01, amplitude=2.0, viscosity=0.05):
    """ms per step of the complex-table call (KdV) and of the real-table call (KS) on the same state size"""
    from data_generation.ks_1d import ks_initial_condition
    from rpde import ops
    from rpde._lib import check, load, ptr, stream_ptr, workspace
    lib = load()
    dev = torch.device("cuda")
    u0 = ks_initial_condition(B, N, length, lmax, torch.Generator().manual_seed(0)).to(dev)
    real = [t.to(dev) for t in ops.etd1d_tables(N, length, 1.0, -viscosity, dt)]
    cx = [t.to(dev) for t in ops.etd1d_tables_cx(N, length, 0.0, 0.0, 1.0, 0.0, dt)]
    nws = lib.rpde_etd1d_ws_bytes(B, N)
    ws = workspace(nws, dev)
    st = stream_ptr()
    U0 = torch.empty(lib.rpde_etd1d_spec_elems(B, N), dtype=torch.float32, device=dev)
    check(lib.rpde_etd1d_rfft(ptr(u0), ptr(U0), B, N, st), "rfft")
    Ur, Uc = U0.clone(), amplitude * U0

    def real_steps(n):
        check(lib.rpde_etd1d_steps(ptr(Ur), *(ptr(t) for t in real), B, N, n, ws.data_ptr(), nws, st), "steps")

    def cx_steps(n):
        check(lib.rpde_etd1d_steps_cx(ptr(Uc), *(ptr(t) for t in cx), B, N, n, ws.data_ptr(), nws, st), "steps_cx")

    for fn in (real_steps, cx_steps):                                        # warm-up of every timed shape
        fn(3)
    torch.cuda.synchronize()
    Ur.copy_(U0)
    Uc.copy_(amplitude * U0)
    t_real, t_cx = [], []
    for _ in range(repeats):                                                 # alternate the two calls
        t_real += _windows(real_steps, steps, 1)
        t_cx += _windows(cx_steps, steps, 1)
    r, c = _stats(t_real), _stats(t_cx)
    return {"N": N, "B": B, "pde": "kdv", "steps_per_window": steps, "windows": repeats, "length": length, "dt": dt,
            "amplitude": amplitude, "launches_per_step": LAUNCHES_PER_STEP, "real_step": r, "cx_step": c,
            "cx_over_real": c["median_ms"] / r["median_ms"], "cx_minus_real_us": 1e3 * (c["median_ms"] - r["median_ms"]),
            "state_bytes": 4 * int(U0.numel()), "table_bytes_real": 4 * sum(int(t.numel()) for t in real),
            "table_bytes_cx": 4 * sum(int(t.numel()) for t in cx),
            "finite": bool(torch.isfinite(Uc).all() and torch.isfinite(Ur).all()), "steps_timed": steps * repeats}


def _sizes(text):
    return [tuple(int(v) for v in item.split("x")) for item in text.split(",") if item.strip()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", default="256x512,1024x256", help="comma-separated NxB")
    ap.add_argument("--kdv-sizes", default="256x512,1024x512", help="comma-separated NxB of the complex-table rows")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("etd1d_gen_bench.py needs the GPU")
    lines = []
    for N, B in _sizes(args.sizes):
        lines.append(json.dumps(bench(N, B, args.steps, args.repeats)))
        print(lines[-1], flush=True)
    for N, B in _sizes(args.kdv_sizes):
        lines.append(json.dumps(bench_kdv(N, B, args.steps, args.repeats)))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
