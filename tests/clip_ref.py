"""Gradient-norm clipping in float64 (TEST INFRASTRUCTURE ONLY).

Restates ``torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2)`` for a list of gradients, without calling
it (tests/test_grad_clip_cpu.py compares the two):

    norm  = sqrt(sum g^2)            over every gradient; complex ones count as their (re, im) floats, None as nothing
    scale = min(1, max_norm / (norm + 1e-6))      NaN propagates (torch.clamp), an infinite norm gives 0
    g    <- scale * g

Inputs of any dtype and device are taken to float64 on the CPU.
"""
from __future__ import annotations

import math
from typing import Iterable, List, Optional

import torch

TORCH_EPS = 1e-6          # the constant in torch's clip coefficient


def _f64(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.to(torch.float64)


def total_norm_f64(grads: Iterable[Optional[torch.Tensor]]) -> float:
    s = 0.0
    for g in grads:
        if g is not None:
            g = _f64(g)
            s += float((g * g).sum())
    return math.sqrt(s)


def clip_scale_f64(norm: float, max_norm: Optional[float]) -> float:
    """the factor on the gradients; max_norm None: no clipping"""
    if max_norm is None:
        return 1.0
    q = float("nan") if math.isnan(norm) else max_norm / (norm + TORCH_EPS)
    return q if (math.isnan(q) or q < 1.0) else 1.0


def clipped_f64(grads: List[Optional[torch.Tensor]], max_norm: Optional[float]):
    """-> (norm, scale, [scale * g as float64, complex as view_as_real, None where the gradient is None])"""
    norm = total_norm_f64(grads)
    scale = clip_scale_f64(norm, max_norm)
    return norm, scale, [None if g is None else _f64(g) * scale for g in grads]
