#!/usr/bin/env python3
"""A/B: the fused per-frequency error evaluator against the reference's op sequence through stock ATen, same GPU, same
process, in alternation.

    python profiles/freq_error_ab.py [--rounds 5] [--out profiles/freq_error.txt]       (run it twice: the spread
                                                                                          between identical runs belongs
                                                                                          beside the difference)
ATen side, restated from the description of the reference's utils/frequency_error.py: rfft (rfft2) of prediction and
target; then per mode (per radial bin, boolean mask from a float32 radial-frequency tensor) copies of both spectra that
hold that mode (bin) only, irfft (irfft2) of both, torch.norm(difference).item() and torch.norm(target part).item() --
2 x 513 host round trips for Burgers [64, 1, 1024], 2 x 64 for NS [32, 1, 256, 256] with 64 bins.
Fused side: rpde.ops.freq_energy1d / freq_energy2d into a float64 device accumulator; sqrt and one copy at the end.

Timing: host clock around work that ends in a device synchronise.  The ATen sequence synchronises by itself at every
.item(); the fused side runs CALLS calls per window so that a window is not the measurement of one launch.  Bytes: the
call has to read prediction and target once (2 x 4 x numel); `hbm_floor_us` is that over the MI355X's 8 TB/s, and
`fused_input_GBps` the same bytes over the measured time of a call."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "resolution-pde_amd"))
from rpde import ops  # noqa: E402

CALLS = 200
HBM_BYTES_PER_S = 8.0e12


def aten_1d(y_hat, y):
    H = y.shape[-1]
    fh, f = torch.fft.rfft(y_hat, dim=-1), torch.fft.rfft(y, dim=-1)
    n = f.shape[-1]
    err, sol = np.zeros(n), np.zeros(n)
    for k in range(n):
        mh, m = torch.zeros_like(fh), torch.zeros_like(f)
        mh[..., k] = fh[..., k]
        m[..., k] = f[..., k]
        sh, s = torch.fft.irfft(mh, n=H, dim=-1), torch.fft.irfft(m, n=H, dim=-1)
        err[k] = torch.norm(sh - s).item()
        sol[k] = torch.norm(s).item()
    return err, sol


def aten_2d(y_hat, y, nb):
    H, W = y.shape[-2:]
    fh, f = torch.fft.rfft2(y_hat, dim=(-2, -1)), torch.fft.rfft2(y, dim=(-2, -1))
    r = torch.sqrt(torch.fft.fftfreq(H, device=y.device).view(-1, 1) ** 2 + torch.fft.rfftfreq(W, device=y.device).view(1, -1) ** 2)
    edges = np.linspace(0, 0.5, nb + 1)
    err, sol = np.zeros(nb), np.zeros(nb)
    for i in range(nb):
        mask = (r >= edges[i]) & (r < edges[i + 1])
        if mask.sum() == 0:
            continue
        sh = torch.fft.irfft2(fh * mask, s=(H, W), dim=(-2, -1))
        s = torch.fft.irfft2(f * mask, s=(H, W), dim=(-2, -1))
        err[i] = torch.norm(sh - s).item()
        sol[i] = torch.norm(s).item()
    return err, sol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda:0"
    lines = []
    for name, shape, nb in (("NS [32,1,256,256], 64 bins", (32, 1, 256, 256), 64), ("Burgers [64,1,1024], 513 modes", (64, 1, 1024), None)):
        g = torch.Generator().manual_seed(1)
        y = (torch.randn(shape, generator=g) + 1.0).to(dev)
        y_hat = y + 1e-2 * torch.randn(shape, generator=g).to(dev)
        if nb:
            aten = lambda: aten_2d(y_hat, y, nb)                                             # noqa: E731
            fused = lambda acc=None: ops.freq_energy2d(y_hat, y, nb, acc=acc)                # noqa: E731
        else:
            aten = lambda: aten_1d(y_hat, y)                                                 # noqa: E731
            fused = lambda acc=None: ops.freq_energy1d(y_hat, y, acc=acc)                    # noqa: E731
        # warm up both sides; agreement of the two on these inputs (fp32 ATen against the device: ATen's own floor)
        ref = aten()
        acc = fused()
        got = torch.sqrt(acc).cpu().numpy()
        agree = [float(np.linalg.norm(got[i] - ref[i]) / np.linalg.norm(ref[i])) for i in range(2)]
        for _ in range(20):
            fused(acc)
        torch.cuda.synchronize()
        ta, tf = [], []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            aten()
            torch.cuda.synchronize()
            ta.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fused(acc)
            torch.cuda.synchronize()
            tf.append((time.perf_counter() - t0) / CALLS)
        need = 2 * 4 * y.numel()
        rec = {"shape": name, "aten_ms": [round(t * 1e3, 3) for t in ta], "fused_us": [round(t * 1e6, 2) for t in tf],
               "aten_ms_median": round(float(np.median(ta)) * 1e3, 3), "fused_us_median": round(float(np.median(tf)) * 1e6, 2),
               "ratio": round(float(np.median(ta) / np.median(tf)), 1), "input_bytes": need,
               "hbm_floor_us": round(need / HBM_BYTES_PER_S * 1e6, 2),
               "fused_input_GBps": round(need / float(np.median(tf)) / 1e9, 1),
               "agreement_rel_l2": [float(f"{v:.2e}") for v in agree]}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        assert rec["ratio"] >= 1.0, f"the fused call is slower than the ATen sequence: {rec}"
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
