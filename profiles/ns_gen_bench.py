"""Time one step of the Navier-Stokes vorticity generator (csrc/ns_solver.hip) against the same step written with
torch.fft (rocFFT) on the same GPU.  Does not touch bench.py.

    python profiles/ns_gen_bench.py [--steps 50] [--repeats 7] [--sizes 256x50,64x50] [--out profiles/ns_gen_bench.json]

Per (resolution s, batch B): warm-up (plans, code objects, rocFFT's own plans), then `repeats` windows of `steps` steps
each between device events, alternating the two implementations; reported are the median, minimum and maximum of the
windows in ms per step.  The parts of one step are timed the same way through the C ABI: the inverse transform of the
4B derivative spectra (rowdft + synthesis), the forward transform of the B products (analysis + rowdft), and the rest
(k_ns_advect + k_ns_update_fanout) as the difference.  A last line compares the two implementations' states after the
timed steps.  Needs the GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import math
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


class TorchStep:
    """the same step with torch.fft in fp32; tables as the device path rounds them"""

    def __init__(self, M, N, visc, dt, f, dev):
        from rpde import ops
        K = N // 2 + 1
        c_w, c_f, c_g, inv_lap = (t[:, :K].to(dev) for t in ops.ns2d_tables(M, N, visc, dt))
        k1 = (torch.fft.fftfreq(M) * M).round().view(M, 1).to(dev)
        k2 = torch.arange(K, dtype=torch.float32).view(1, K).to(dev)
        self.ik1, self.ik2 = (2j * math.pi * k1).to(torch.complex64), (2j * math.pi * k2).to(torch.complex64)
        self.c_w, self.c_f, self.inv_lap, self.s = c_w, c_f, inv_lap, (M, N)
        self.g_h = c_g * torch.fft.rfft2(f)

    def run(self, W, steps):
        inv = lambda z: torch.fft.irfft2(z, s=self.s)
        for _ in range(steps):
            psi = W * self.inv_lap
            q, v = inv(self.ik2 * psi), inv(-self.ik1 * psi)
            w_x, w_y = inv(self.ik1 * W), inv(self.ik2 * W)
            W = self.c_w * W - self.c_f * torch.fft.rfft2(q * w_x + v * w_y) + self.g_h
        return W


def bench(s, B, steps, repeats, visc=1e-4, dt=1e-4):
    from data_generation.ns_2d import forcing
    from data_generation.random_fields import GaussianRF
    from rpde import ops
    from rpde._lib import check, load, ptr, stream_ptr, workspace
    lib = load()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    w0 = GaussianRF(2, s, alpha=2.5, tau=7, device=dev).sample(B, generator=gen)
    f = forcing(s, dev)
    M = N = s
    c_w, c_f, c_g, inv_lap = (t.to(dev) for t in ops.ns2d_tables(M, N, visc, dt))
    nws = lib.rpde_ns2d_ws_bytes(4 * B, M, N)
    ws = workspace(nws, dev)
    st = stream_ptr()
    spec = lib.rpde_ns2d_spec_elems(B, M, N)
    W0 = torch.empty(spec, dtype=torch.float32, device=dev)
    f_h = torch.empty(lib.rpde_ns2d_spec_elems(1, M, N), dtype=torch.float32, device=dev)
    g_h = torch.empty_like(f_h)
    check(lib.rpde_ns2d_rfft2(ptr(w0), ptr(W0), B, M, N, ws.data_ptr(), nws, st), "rfft2")
    check(lib.rpde_ns2d_rfft2(ptr(f), ptr(f_h), 1, M, N, ws.data_ptr(), nws, st), "rfft2")
    check(lib.rpde_ns2d_scale(ptr(f_h), ptr(c_g), ptr(g_h), 1, M, N, st), "scale")
    W = W0.clone()
    D = torch.zeros(4 * spec, dtype=torch.float32, device=dev)
    P = torch.empty(4 * B, M, N, dtype=torch.float32, device=dev)

    def hip_steps(n):
        check(lib.rpde_ns2d_steps(ptr(W), ptr(g_h), 0, ptr(c_w), ptr(c_f), ptr(inv_lap), B, M, N, n, ws.data_ptr(), nws, st), "steps")

    def hip_inverse(n):
        for _ in range(n):
            check(lib.rpde_ns2d_irfft2(ptr(D), ptr(P), 4 * B, M, N, ws.data_ptr(), nws, st), "irfft2")

    def hip_forward(n):
        for _ in range(n):
            check(lib.rpde_ns2d_rfft2(ptr(P), ptr(D), B, M, N, ws.data_ptr(), nws, st), "rfft2")

    ref = TorchStep(M, N, visc, dt, f, dev)
    Wt0 = torch.fft.rfft2(w0)
    state = {"W": Wt0}

    def torch_steps(n):
        state["W"] = ref.run(state["W"], n)

    for fn in (hip_steps, torch_steps, hip_inverse, hip_forward):          # warm-up of every timed shape
        fn(3)
    torch.cuda.synchronize()
    W.copy_(W0)
    state["W"] = Wt0
    t_hip, t_torch = [], []
    for _ in range(repeats):                                                 # alternate the two implementations
        t_hip += _windows(hip_steps, steps, 1)
        t_torch += _windows(torch_steps, steps, 1)
    t_inv = _windows(hip_inverse, steps, repeats)
    t_fwd = _windows(hip_forward, steps, repeats)
    # both advanced repeats * steps steps from the same state: compare them in physical space
    w_hip = torch.empty(B, M, N, dtype=torch.float32, device=dev)
    check(lib.rpde_ns2d_irfft2(ptr(W), ptr(w_hip), B, M, N, ws.data_ptr(), nws, st), "irfft2")
    w_t = torch.fft.irfft2(state["W"], s=(M, N))
    diff = float((w_hip - w_t).norm() / w_t.norm())
    hip, tor, inv, fwd = _stats(t_hip), _stats(t_torch), _stats(t_inv), _stats(t_fwd)
    return {"s": s, "B": B, "steps_per_window": steps, "windows": repeats, "visc": visc, "dt": dt,
            "hip_step": hip, "torch_fft_step": tor, "hip_over_torch": hip["median_ms"] / tor["median_ms"],
            "hip_inverse_4B": inv, "hip_forward_B": fwd,
            "hip_pointwise_ms": hip["median_ms"] - inv["median_ms"] - fwd["median_ms"],
            "rel_l2_hip_vs_torch_after": diff, "steps_compared": steps * repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", default="256x50,64x50")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ns_gen_bench.py needs the GPU")
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
