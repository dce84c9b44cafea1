"""Restatement of the Darcy generator (csrc/darcy.hip, rpde.ops.darcy2d_*) in numpy / scipy, independent of the library.

-div(a grad u) = f on the unit square, u = 0 on the boundary, s x s cells with centres (i + 1/2) / s, finite volumes:
an interior face between cells c and n weighs w = 2 a_c a_n / (a_c + a_n), a boundary face of cell c weighs 2 a_c and has
u = 0 behind it, (A u)_c = s^2 sum_faces w (u_c - u_n).

  matrix(a)          the float64 sparse matrix of one sample;  direct(a, f) solves with it (scipy spsolve)
  apply(a, u)        the same operator matrix-free in the difference form, in the dtype of its arguments
  pcg(a, f, ...)     conjugate gradients preconditioned with the operator at a = 1 (dense DST-II table S), in a chosen
                     dtype, with the per-sample freeze of the device loop
  neumann_field(..)  the cosine-series Gaussian field N(0, sigma^2 (-Lap + tau^2)^-alpha) with zero-flux boundary

floor32 of a case is the relative L2 error of pcg in float32 against direct in float64 on the same inputs; the device
tests allow FLOOR_FACTOR times that."""
from __future__ import annotations

import functools
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

FLOOR_FACTOR = 4
# (B, s): 12, 20, 36 and 100 are no multiples of 8, 16 or 32 -- where a 16-byte-group stencil, a halo or a GEMM edge tile
# can go wrong; 8 is the smallest grid, 100 and 128 take more than one block per sample
CASES = [(3, 8), (2, 12), (2, 20), (2, 36), (2, 64), (1, 100), (1, 128)]
# name -> (hi, lo, iterations of the solve, the float32 restatement must freeze within `within`)
CONTRASTS = {"12_3": (12.0, 3.0, 24, 20), "1_0.1": (1.0, 0.1, 32, 32)}
TOL = 1e-6


def case_id(case):
    return f"B{case[0]}_s{case[1]}"


def rel(x, ref) -> float:
    """relative L2 error of x (numpy or torch) against ref, in float64"""
    x = np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(x - ref) / np.linalg.norm(ref))


# ---- the operator -----------------------------------------------------------------------------------------------------
def _hmean(x, y):
    return (2 * x * y) / (x + y)


def face_weights(a):
    """(wl, wr, wn, ws) of a [..., s, s]: the weights of each cell's faces towards j-1, j+1, i-1, i+1, in a's dtype"""
    wl, wr, wn, ws = (2 * a for _ in range(4))
    wl[..., :, 1:] = _hmean(a[..., :, 1:], a[..., :, :-1])
    wr[..., :, :-1] = _hmean(a[..., :, :-1], a[..., :, 1:])
    wn[..., 1:, :] = _hmean(a[..., 1:, :], a[..., :-1, :])
    ws[..., :-1, :] = _hmean(a[..., :-1, :], a[..., 1:, :])
    return wl, wr, wn, ws


def apply(a, u):
    """A u in the difference form, matrix-free, in the common dtype of a and u ([..., s, s])"""
    s = a.shape[-1]
    wl, wr, wn, ws = face_weights(a)
    z = np.zeros_like(u)
    ul, ur, un, us = z.copy(), z.copy(), z.copy(), z.copy()
    ul[..., :, 1:] = u[..., :, :-1]
    ur[..., :, :-1] = u[..., :, 1:]
    un[..., 1:, :] = u[..., :-1, :]
    us[..., :-1, :] = u[..., 1:, :]
    acc = wl * (u - ul) + wr * (u - ur) + wn * (u - un) + ws * (u - us)
    return u.dtype.type(s * s) * acc


def matrix(a):
    """the float64 sparse matrix of one sample a [s, s]; cell (i, j) is row i s + j"""
    a = np.asarray(a, dtype=np.float64)
    s = a.shape[-1]
    assert a.shape == (s, s)
    wl, wr, wn, ws = face_weights(a)
    idx = np.arange(s * s).reshape(s, s)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [(wl + wr + wn + ws).ravel()]
    # the cells that have a neighbour across each face, and that neighbour
    for w, own, nb in ((wl, np.s_[:, 1:], np.s_[:, :-1]), (wr, np.s_[:, :-1], np.s_[:, 1:]),
                       (wn, np.s_[1:, :], np.s_[:-1, :]), (ws, np.s_[:-1, :], np.s_[1:, :])):
        rows.append(idx[own].ravel())
        cols.append(idx[nb].ravel())
        vals.append(-w[own].ravel())
    m = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(s * s, s * s))
    return (float(s) ** 2) * m


def direct(a, f):
    """u [B, s, s] float64 from the sparse direct solve, sample by sample; f [s, s] or [B, s, s]"""
    a = np.asarray(a, dtype=np.float64)
    f = np.broadcast_to(np.asarray(f, dtype=np.float64), a.shape)
    s = a.shape[-1]
    return np.stack([spla.spsolve(matrix(a[b]).tocsc(), f[b].ravel()).reshape(s, s) for b in range(a.shape[0])])


# ---- the preconditioner -----------------------------------------------------------------------------------------------
def tables(s):
    """(S, lam) float64: the orthogonal DST-II table [s, s] and the eigenvalues l_k [s] of the a = 1 operator per axis"""
    k = np.arange(1, s + 1, dtype=np.float64)[:, None]
    x = (np.arange(s, dtype=np.float64) + 0.5)[None, :]
    S = math.sqrt(2.0 / s) * np.sin(math.pi * k * x / s)
    S[s - 1] /= math.sqrt(2.0)
    lam = float(s) ** 2 * (2.0 - 2.0 * np.cos(math.pi * k[:, 0] / s))
    return S, lam


def precondition(r, S, inv_lambda):
    """S^T (inv_lambda . (S r S^T)) S, in the dtype of its arguments"""
    return S.T @ (inv_lambda * (S @ r @ S.T)) @ S


def pcg(a, f, iterations, tol, dtype):
    """-> (u [B, s, s], frozen_at [B]) in `dtype`: the device loop restated -- u = 0, r = f, z = P^-1 r, p = z, then per
    iteration alpha = rz / pAp, u += alpha p, r -= alpha Ap, freeze where |r| <= tol |f| (or a denominator is not
    positive finite), z = P^-1 r, beta = rz_new / rz, p = z + beta p.  frozen_at = iterations: never froze."""
    a = np.asarray(a, dtype=dtype)
    f = np.ascontiguousarray(np.broadcast_to(np.asarray(f, dtype=dtype), a.shape))
    B, s = a.shape[0], a.shape[-1]
    S64, lam = tables(s)
    S, il = S64.astype(dtype), (1.0 / (lam[:, None] + lam[None, :])).astype(dtype)
    dot = lambda x, y: np.sum(x * y, axis=(1, 2))                    # noqa: E731
    ok = lambda v: np.isfinite(v) & (v > 0)                          # noqa: E731
    u, r = np.zeros_like(f), f.copy()
    ff = dot(f, f)
    z = precondition(r, S, il)
    rz = dot(r, z)
    p = z.copy()
    active = (ff > 0) & ok(rz)
    frozen_at = np.where(active, iterations, 0)
    tol2 = dtype(tol) * dtype(tol)
    for k in range(iterations):
        if not active.any():
            break
        Ap = apply(a, p)
        pap = dot(p, Ap)
        stop = active & ~ok(pap)
        frozen_at[stop], active = k, active & ok(pap)
        alpha = np.where(active, rz / np.where(active, pap, 1), 0).astype(dtype)
        u = u + alpha[:, None, None] * p
        r = r - alpha[:, None, None] * Ap
        z = precondition(r, S, il)
        rz_new = dot(r, z)
        stop = active & (~(dot(r, r) > tol2 * ff) | ~ok(rz_new))
        frozen_at[stop], active = k + 1, active & ~stop
        beta = np.where(active, rz_new / np.where(active, rz, 1), 0).astype(dtype)
        p = np.where(active[:, None, None], z + beta[:, None, None] * p, p)
        rz = np.where(active, rz_new, rz)
    return u, frozen_at


# ---- inputs -----------------------------------------------------------------------------------------------------------
def cosine_table(s):
    """C[i, k] = cos(pi k (i + 1/2) / s), float64 [s, s]"""
    i = (np.arange(s, dtype=np.float64) + 0.5)[:, None]
    k = np.arange(s, dtype=np.float64)[None, :]
    return np.cos(math.pi * k * i / s)


def neumann_coef(s, alpha=2.0, tau=3.0, sigma=None):
    """coef[k1, k2] = sigma (pi^2 (k1^2 + k2^2) + tau^2)^(-alpha/2), 0 at the mean mode; sigma = tau^(alpha - 1) by default"""
    sigma = tau ** (0.5 * (2 * alpha - 2)) if sigma is None else sigma
    k = np.arange(s, dtype=np.float64)
    coef = sigma * (math.pi ** 2 * (k[:, None] ** 2 + k[None, :] ** 2) + tau ** 2) ** (-alpha / 2.0)
    coef[0, 0] = 0.0
    return coef


def neumann_field(n, s, seed, alpha=2.0, tau=3.0, noise=None):
    """[n, s, s] float64 samples C (coef . xi) C^T, xi standard normal (from `seed`, or passed in)"""
    xi = np.random.default_rng(seed).standard_normal((n, s, s)) if noise is None else np.asarray(noise, dtype=np.float64)
    C = cosine_table(s)
    return C @ (neumann_coef(s, alpha, tau) * xi) @ C.T


def threshold(g, hi, lo):
    return np.where(g >= 0, hi, lo)


@functools.lru_cache(maxsize=None)
def parity_reference(case, contrast):
    """the inputs of one parity case and everything the tests compare against, computed once: a (float32 values),
    u64 (direct), u32 / frozen32 (the float32 restatement), floor32, gap (to the solution with a replaced by its mean)"""
    B, s = case
    hi, lo, iterations, within = CONTRASTS[contrast]
    a32 = threshold(neumann_field(B, s, seed=1000 + s), hi, lo).astype(np.float32)
    f = np.ones((s, s), dtype=np.float32)
    u64 = direct(a32, f)
    u32, frozen32 = pcg(a32, f, iterations, TOL, np.float32)
    mean = np.broadcast_to(a32.astype(np.float64).mean(axis=(1, 2), keepdims=True), a32.shape)
    ub = direct(mean, f)
    return dict(a=a32, f=f, u64=u64, u32=u32, frozen32=frozen32, iterations=iterations, within=within,
                floor32=[rel(u32[b], u64[b]) for b in range(B)], gap=[rel(ub[b], u64[b]) for b in range(B)])
