"""One AdamW step in float64 (TEST INFRASTRUCTURE ONLY).

Restates the update rule of ``torch.optim.AdamW`` (decoupled weight decay, bias-corrected moments, no amsgrad, no
maximize) as the reference builds it (main_1d.py:144, main_2d.py:173) and as ``csrc/adamw.hip`` implements it:

    p *= 1 - lr * wd
    m += (g - m)(1 - b1)
    v  = b2 v + (1 - b2) g^2
    p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)

Complex parameters are their (re, im) pairs, as ``torch.view_as_real`` presents them (torch's AdamW does the same).
Inputs of any dtype and device are taken to float64 on the CPU; the result is one step from exactly those values,
so a test that feeds the kernel's own starting state gets a reference that carries no error from earlier steps.
"""
from __future__ import annotations

import math

import torch


def _f64(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.to(torch.float64)


def adamw_step_f64(p, g, m, v, t: int, lr: float, wd: float, betas=(0.9, 0.999), eps: float = 1e-8):
    """-> (p, m, v) after step number ``t`` (1-based), float64 CPU tensors; complex inputs come back as
    ``view_as_real`` layout (a trailing axis of 2)"""
    if t < 1:
        raise ValueError("adamw_step_f64: the step number counts from 1")
    b1, b2 = float(betas[0]), float(betas[1])
    p, g, m, v = (_f64(x) for x in (p, g, m, v))
    if not (p.shape == g.shape == m.shape == v.shape):
        raise ValueError(f"adamw_step_f64: shapes differ {p.shape} {g.shape} {m.shape} {v.shape}")
    p = p * (1.0 - lr * wd)
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + g * g * (1.0 - b2)
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v
