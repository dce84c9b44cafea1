"""Restatement of the Darcy equation-residual loss (csrc/darcy_residual.hip, rpde.ops.darcy2d_residual,
utils.loss.DarcyResidualLoss) in numpy, in a chosen dtype, on tests/darcy_ref.py's apply, tables and inputs;
independent of the library.

With a~ = a_x a + b_x, u~ = a_p p + b_p and r_b = f - A(a~_b) u~_b:

  norm "dual":  E_b = sum_k inv_lambda_k (S r_b S^T)_k^2,  D = sqrt(sum_k inv_lambda_k (S f S^T)_k^2),  z_b = S^T (inv_lambda . S r_b S^T) S
  norm "l2":    E_b = |r_b|^2,                             D = |f|_2,                                   z_b = r_b
  rel_b = sqrt(E_b) / (D + 1e-8),   d (sum_b w_b rel_b) / d p_b = -a_p w_b A(a~_b) z_b / ((D + 1e-8) sqrt(E_b))

floor32 of a case is the relative difference of the float32 restatement from the float64 one on the same fp32 inputs:
the largest over the samples for the value, a relative L2 over the whole tensor for the gradient.  The device tests
allow FLOOR_FACTOR times max(floor32, 2^-24): 2^-24 is half an ulp of the fp32 result itself."""
from __future__ import annotations

import functools

import numpy as np

from tests import darcy_ref as R

FLOOR_FACTOR = R.FLOOR_FACTOR
HALF_ULP = 2.0 ** -24
NORMS = ("dual", "l2")
KINDS = ("smooth", "white")                 # the perturbed predictions; "exact" is p = u64 rounded to fp32
# darcy_ref.CASES up to 100: 8 the smallest grid (every 16-byte group touches a wall), 12 the first group with no wall,
# 20 and 36 no multiples of 8 / 16 / 32, 36 and up more than one block per sample
CASES = [c for c in R.CASES if c[1] <= 100]
CONTRASTS = tuple(R.CONTRASTS)


def case_id(case):
    return R.case_id(case)


def tables(s, dtype=np.float64):
    """(S, inv_lambda) in `dtype`, formed in float64 and rounded once"""
    S, lam = R.tables(s)
    return S.astype(dtype), (1.0 / (lam[:, None] + lam[None, :])).astype(dtype)


def denominator(f, norm):
    """D in float64 for one right-hand side f [s, s]"""
    f = np.asarray(f, dtype=np.float64)
    if norm == "l2":
        return float(np.sqrt(np.sum(f * f)))
    S, il = tables(f.shape[-1])
    return float(np.sqrt(np.sum(il * (S @ f @ S.T) ** 2)))


def decode(x, a, b, dtype):
    return dtype(a) * x.astype(dtype) + dtype(b)


def parts(a, p, f, dtype, norm, affine=None):
    """(E [B], D, z [B, s, s], a~) in `dtype`"""
    ap, bp, ax, bx = (1.0, 0.0, 1.0, 0.0) if affine is None else affine
    at, ut = decode(np.asarray(a), ax, bx, dtype), decode(np.asarray(p), ap, bp, dtype)
    f = np.asarray(f).astype(dtype)
    r = f - R.apply(at, ut)
    if norm == "l2":
        E, D, z = np.sum(r * r, axis=(1, 2), dtype=dtype), np.sqrt(np.sum(f * f, dtype=dtype)), r
    else:
        S, il = tables(at.shape[-1], dtype)
        rh, fh = S @ r @ S.T, S @ f @ S.T
        E = np.sum(il * rh * rh, axis=(1, 2), dtype=dtype)
        D = np.sqrt(np.sum(il * fh * fh, dtype=dtype))
        z = S.T @ (il * rh) @ S
    return E, D, z, at


def rel(a, p, f, dtype=np.float64, norm="dual", affine=None):
    E, D, _, _ = parts(a, p, f, dtype, norm, affine)
    return np.sqrt(E) / (D + dtype(1e-8))


def rel_and_grad(a, p, f, dtype=np.float64, norm="dual", affine=None, weights=None):
    """(rel [B], the gradient of sum_b weights_b rel_b with respect to p [B, s, s]) by the formula the device implements;
    0 where E_b = 0"""
    E, D, z, at = parts(a, p, f, dtype, norm, affine)
    num = np.sqrt(E)
    w = np.ones_like(num) if weights is None else np.asarray(weights).astype(dtype)
    ap = dtype(1.0 if affine is None else affine[0])
    safe = np.where(num > 0, num, dtype(1))
    coef = np.where(num > 0, w / (safe * (D + dtype(1e-8))), dtype(0))
    return num / (D + dtype(1e-8)), -ap * coef[:, None, None] * R.apply(at, z)


def rel_torch(a, p, f, norm="dual", affine=None):
    """the same value as a float64 torch expression of p (a torch tensor that may require grad): for autograd"""
    import torch
    import torch.nn.functional as F
    ap, bp, ax, bx = (1.0, 0.0, 1.0, 0.0) if affine is None else affine
    at = ax * np.asarray(a, dtype=np.float64) + bx
    s = at.shape[-1]
    wl, wr, wn, ws = (torch.from_numpy(np.ascontiguousarray(w)) for w in R.face_weights(at))
    u = ap * p.double() + bp
    up = F.pad(u, (1, 1, 1, 1))
    Au = float(s * s) * (wl * (u - up[..., 1:-1, :-2]) + wr * (u - up[..., 1:-1, 2:]) + wn * (u - up[..., :-2, 1:-1])
                         + ws * (u - up[..., 2:, 1:-1]))
    ft = torch.from_numpy(np.asarray(f, dtype=np.float64))
    r = ft - Au
    if norm == "l2":
        return torch.sqrt((r * r).sum((1, 2))) / (torch.sqrt((ft * ft).sum()) + 1e-8)
    S, il = (torch.from_numpy(t) for t in tables(s))
    rh, fh = S @ r @ S.T, S @ ft @ S.T
    return torch.sqrt((il * rh * rh).sum((1, 2))) / (torch.sqrt((il * fh * fh).sum()) + 1e-8)


def energy_ratio(a, p, u_star, f):
    """E_b / (e_b . A e_b) in float64, e = u* - p, E the dual norm's r . P^-1 r: within [a_min, a_max]"""
    a64, e = np.asarray(a, dtype=np.float64), np.asarray(u_star, dtype=np.float64) - np.asarray(p, dtype=np.float64)
    E, _, _, _ = parts(a64, np.asarray(p, dtype=np.float64), f, np.float64, "dual")
    return E / np.sum(e * R.apply(a64, e), axis=(1, 2))


# ---- inputs -----------------------------------------------------------------------------------------------------------
def prediction(case, contrast, kind):
    """p [B, s, s] float32 for darcy_ref.parity_reference's inputs: "exact" u64 rounded; "smooth" u64 (1 + 0.05 g), g a
    cosine-series field scaled to max |g| = 1; "white" u64 (1 + 0.01 N(0, 1))"""
    B, s = case
    u64 = R.parity_reference(case, contrast)["u64"]
    if kind == "exact":
        return u64.astype(np.float32)
    if kind == "smooth":
        g = R.neumann_field(B, s, seed=5 + s)
        return (u64 * (1.0 + 0.05 * g / np.abs(g).max())).astype(np.float32)
    if kind == "white":
        return (u64 * (1.0 + 0.01 * np.random.default_rng(7 + s).standard_normal(u64.shape))).astype(np.float32)
    raise ValueError(kind)


def floors(a, p, f, norm, affine=None, weights=None):
    """(rel64, grad64, floor of the value, floor of the gradient): the float64 restatement and the float32 one's
    distance from it on the same fp32 inputs"""
    r64, g64 = rel_and_grad(a, p, f, np.float64, norm, affine, weights)
    r32, g32 = rel_and_grad(a, p, f, np.float32, norm, affine, weights)
    fv = float(np.max(np.abs(r32.astype(np.float64) - r64) / r64))
    fg = float(np.linalg.norm(g32.astype(np.float64) - g64) / np.linalg.norm(g64))
    return r64, g64, fv, fg


@functools.lru_cache(maxsize=None)
def parity_reference(case, contrast, kind, norm):
    """one parity case, computed once: a, f, p (fp32), rel64 [B], grad64 of sum_b rel_b, floor_rel, floor_grad, zero64
    (the value of the trivial predictor p = 0)"""
    base = R.parity_reference(case, contrast)
    a, f = base["a"], base["f"]
    p = prediction(case, contrast, kind)
    r64, g64, fv, fg = floors(a, p, f, norm)
    return dict(a=a, f=f, p=p, u64=base["u64"], rel64=r64, grad64=g64, floor_rel=fv, floor_grad=fg,
                zero64=rel(a, np.zeros_like(p), f, np.float64, norm))


def bound(floor):
    return FLOOR_FACTOR * max(floor, HALF_ULP)
