"""Restatement of the vorticity equation-residual loss with torch.fft (test infrastructure only; the product tree does
not import it), and the parity cases.

Grid, k1, k2, lap, dealias and the discrete advection are those of tests/ns_solver_ref.py (the generator's):

    A(w) = dealias rfft2(q w_x + v w_y),  psi = W / lap (lap[0, 0] -> 1),  q = irfft2(2 pi i k2 psi),  v = irfft2(-2 pi i k1 psi),
    w_x = irfft2(2 pi i k1 W),  w_y = irfft2(2 pi i k2 W)

D is the time between the input x = w(t) and the prediction p ~ w(t + D).  The exponential trapezoidal rule on
w_t = -visc lap w - A(w) + f, with z = -D visc lap (real), LR = z + r_m, r_m = exp(2 pi i (m - 1/2) / 64), <.> the mean:

    r^ = d^ - (E - 1) x^ - m0 (f^ - A(x)) - m1 (f^ - A(p)),   d = p - x formed in physical space,  p^ = x^ + d^
    E = e^z,  m0 = D (phi1 - phi2),  m1 = D phi2,  phi1 = Re<(e^LR - 1) / LR>,  phi2 = Re<(e^LR - 1 - LR) / LR^2>
    rel[b] = sqrt(E_r[b]) / (sqrt(E_x[b]) + 1e-8),  E(z)[b] = sum c |z^|^2 / (M N),  c = 1 on the columns kx = 0, N/2, else 2

on p~ = a_p p + b_p and x~ = a_x x + b_x.  The forcing is not de-aliased (the generator adds it as it stands).  The gradient
comes from autograd; `grad_formula` is the closed form the device implements, the exact adjoint of the discrete operator:
with g = irfft2(m1 dealias r^) and (q, v, w_x, w_y) of p~,

    G^ = r^ + conj(2 pi i k2 / lap) rfft2(g w_x) + conj(-2 pi i k1 / lap) rfft2(g w_y) + conj(2 pi i k1) rfft2(g q)
            + conj(2 pi i k2) rfft2(g v),     d rel[b] / d p = a_p coef_b irfft2(G^),  coef_b = 1 / (sqrt(E_r) (sqrt(E_x) + 1e-8)).

Everything in float64 / complex128 by default: the yardstick.  ``dtype=torch.float32`` runs the same restatement in single
precision, tables included (contour in complex64): its distance from the float64 run on the same fp32 inputs is the floor
the device is measured against."""
from __future__ import annotations

import math

import torch

from tests import ns_solver_ref as S
from tests.ns_solver_ref import CASES, EDGE_CASES, FLOOR_FACTOR, VISC, case_id  # noqa: F401

INTERVAL = 0.05                      # between consecutive snapshots of ns_solver_ref's schedule (25 steps of DT)
KINDS = ("noisy", "exact")           # p = the next snapshot plus 10 % Gaussian noise | the next snapshot itself
MIN_FLOOR = 2.0 ** -22               # four fp32 roundings of a stored scalar
IDENTITY = (1.0, 0.0, 1.0, 0.0)


def tables(M, N, visc, interval, dealias=True, dtype=torch.float64):
    """dict(em1, m0, m1, phi1, poisson, k1, k2, dealias) of real [M, K] tensors of `dtype` (m0, m1 carry the mask)"""
    cd = S._cdtype(dtype)
    k1, k2 = S.wavenumbers(M, N, dtype)
    lap = 4 * math.pi ** 2 * (k1 ** 2 + k2 ** 2)
    poisson = lap.clone()
    poisson[0, 0] = 1.0
    keep = ((k1.abs() <= (2.0 / 3.0) * (M // 2)) & (k2.abs() <= (2.0 / 3.0) * (N // 2))).to(dtype)
    if not dealias:
        keep = torch.ones_like(keep)
    h = float(interval)
    z = -h * float(visc) * lap
    m = torch.arange(1, 65, dtype=dtype)
    r = torch.polar(torch.ones(64, dtype=dtype), 2.0 * math.pi * (m - 0.5) / 64.0)
    LR = z.unsqueeze(-1).to(cd) + r
    eLR = torch.exp(LR)
    phi1 = ((eLR - 1.0) / LR).mean(dim=-1).real
    phi2 = ((eLR - 1.0 - LR) / LR ** 2).mean(dim=-1).real
    return dict(em1=torch.expm1(z), m0=h * (phi1 - phi2) * keep, m1=h * phi2 * keep, phi1=h * phi1, poisson=poisson, k1=k1,
                k2=k2, dealias=keep, M=M, N=N)


def forcing_term(f, T):
    """(m0 + m1) rfft2(f) = D phi1 rfft2(f), not de-aliased; None for no forcing"""
    return None if f is None else T["phi1"] * torch.fft.rfft2(f.to(T["phi1"].dtype))


def fields(W, T):
    """(q, v, w_x, w_y) of the spectrum W"""
    M, N = T["M"], T["N"]
    two_pi_i = torch.tensor(2j * math.pi, dtype=W.dtype)
    inv = lambda z: torch.fft.irfft2(z, s=(M, N))          # noqa: E731
    psi = W / T["poisson"]
    return inv(two_pi_i * T["k2"] * psi), inv(-two_pi_i * T["k1"] * psi), inv(two_pi_i * T["k1"] * W), inv(two_pi_i * T["k2"] * W)


def advection(W, T):
    """rfft2(q w_x + v w_y), before de-aliasing"""
    q, v, wx, wy = fields(W, T)
    return torch.fft.rfft2(q * wx + v * wy)


def spectrum(p, x, T, fterm=None, affine=IDENTITY):
    """(r^ [B, M, K], x~^, p~^) in the dtype of p"""
    ap, bp, ax, bx = affine
    pt, xt = ap * p + bp, ax * x + bx
    X = torch.fft.rfft2(xt)
    D = torch.fft.rfft2(pt - xt)
    P = X + D
    r = D - T["em1"] * X + T["m0"] * advection(X, T) + T["m1"] * advection(P, T)
    if fterm is not None:
        r = r - fterm
    return r, X, P


def _energy(s, M, N):
    """sum c |s|^2 / (M N) of half spectra [B, M, K]"""
    c = torch.full((N // 2 + 1,), 2.0, dtype=s.real.dtype)
    c[0] = c[N // 2] = 1.0
    return (c * (s.real ** 2 + s.imag ** 2)).sum((-2, -1)) / (M * N)


def _root(e):
    pos = e > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, e, torch.ones_like(e))), torch.zeros_like(e))


def rel(p, x, T, fterm=None, affine=IDENTITY):
    """rel [B] in the dtype of p; differentiable in p"""
    r, X, _ = spectrum(p, x, T, fterm, affine)
    return _root(_energy(r, T["M"], T["N"])) / (torch.sqrt(_energy(X, T["M"], T["N"])) + 1e-8)


def rel_and_grad(p, x, T, fterm=None, affine=IDENTITY, weights=None):
    """(rel [B], d (sum_b weights_b rel_b) / d p) through autograd, in the dtype of p; weights default to 1"""
    p = p.detach().clone().requires_grad_(True)
    v = rel(p, x, T, fterm, affine)
    w = torch.ones_like(v) if weights is None else weights.to(v.dtype)
    (grad,) = torch.autograd.grad((v * w).sum(), p)
    return v.detach(), grad


def grad_formula(p, x, T, fterm=None, affine=IDENTITY, weights=None):
    """the closed form of d (sum_b weights_b rel_b) / d p that the device implements"""
    M, N = T["M"], T["N"]
    r, X, P = spectrum(p, x, T, fterm, affine)
    rn, xn = torch.sqrt(_energy(r, M, N)), torch.sqrt(_energy(X, M, N))
    w = torch.ones_like(rn) if weights is None else weights.to(rn.dtype)
    coef = torch.where(rn > 0, w / (torch.where(rn > 0, rn, torch.ones_like(rn)) * (xn + 1e-8)), torch.zeros_like(rn))
    g = torch.fft.irfft2(T["m1"] * r, s=(M, N))
    q, v, wx, wy = fields(P, T)
    i2pi = torch.tensor(2j * math.pi, dtype=r.dtype)
    f = torch.fft.rfft2
    G = (r + torch.conj(i2pi * T["k2"] / T["poisson"]) * f(g * wx) + torch.conj(-i2pi * T["k1"] / T["poisson"]) * f(g * wy)
         + torch.conj(i2pi * T["k1"]) * f(g * q) + torch.conj(i2pi * T["k2"]) * f(g * v))
    return affine[0] * coef[:, None, None] * torch.fft.irfft2(G, s=(M, N))


_TRAJ: dict = {}


def trajectory(case, forced=True):
    """[B, M, N, 4] float64: ns_solver_ref's snapshots INTERVAL apart at its own constants, with its forcing or with none"""
    hit = _TRAJ.get((case, forced))
    if hit is None:
        if forced:
            hit = S.parity_reference(case)["sol64"]
        else:
            B, M, N = case
            w0 = S.initial_vorticity(B, M, N, seed=11 + M + N)
            hit, _ = S.solve(w0, torch.zeros(M, N, dtype=torch.float64), S.VISC, S.T_FINAL, S.DT, S.RECORD_STEPS)
        _TRAJ[(case, forced)] = hit
    return hit


_PARITY: dict = {}


def parity_reference(case, kind, forced):
    """{x, p (fp32 [B, M, N], what the device sees), f (float64 [M, N] or None), T64, fterm64, rel64, grad64 (of sum_b rel_b),
    still64 (rel of p = x), floor_rel, floor_grad}: computed once per case and shared; read-only.  x is the second recorded
    snapshot, p the third (kind "exact") or the third plus Gaussian noise of a tenth of its rms (kind "noisy"); `forced`: data
    and loss with ns_solver_ref's forcing, or both with none.  The floors are the float32 restatement's own errors on the
    same fp32 inputs -- rel: the largest relative error over the samples, grad: relative L2 of the whole tensor -- and never
    below MIN_FLOOR."""
    hit = _PARITY.get((case, kind, forced))
    if hit is not None:
        return hit
    B, M, N = case
    sol = trajectory(case, forced)
    x, p = sol[..., 1], sol[..., 2]
    if kind == "noisy":
        gen = torch.Generator().manual_seed(97 + M + N)
        p = p + 0.1 * p.pow(2).mean().sqrt() * torch.randn(B, M, N, generator=gen, dtype=torch.float64)
    elif kind != "exact":
        raise ValueError(kind)
    x, p = x.float().contiguous(), p.float().contiguous()
    f = S.forcing(M, N) if forced else None
    T64, T32 = tables(M, N, S.VISC, INTERVAL), tables(M, N, S.VISC, INTERVAL, dtype=torch.float32)
    ft64, ft32 = forcing_term(f, T64), forcing_term(f, T32)
    rel64, grad64 = rel_and_grad(p.double(), x.double(), T64, ft64)
    rel32, grad32 = rel_and_grad(p, x, T32, ft32)
    out = dict(x=x, p=p, f=f, T64=T64, fterm64=ft64, rel64=rel64, grad64=grad64,
               still64=rel(x.double(), x.double(), T64, ft64),
               floor_rel=max(MIN_FLOOR, float(((rel32.double() - rel64).abs() / rel64).max())),
               floor_grad=max(MIN_FLOOR, float((grad32.double() - grad64).norm() / grad64.norm())))
    _PARITY[(case, kind, forced)] = out
    return out


def floors(p, x, M, N, visc, interval, f=None, affine=IDENTITY):
    """(rel64, grad64, bound_rel, bound_grad) of fp32 inputs: FLOOR_FACTOR x the float32 restatement's own error, as above"""
    T64, T32 = tables(M, N, visc, interval), tables(M, N, visc, interval, dtype=torch.float32)
    rel64, grad64 = rel_and_grad(p.double(), x.double(), T64, forcing_term(f, T64), affine)
    rel32, grad32 = rel_and_grad(p, x, T32, forcing_term(f, T32), affine)
    return (rel64, grad64, FLOOR_FACTOR * max(MIN_FLOOR, float(((rel32.double() - rel64).abs() / rel64).max())),
            FLOOR_FACTOR * max(MIN_FLOOR, float((grad32.double() - grad64).norm() / grad64.norm())))


FORCING_CASE = (2, 16, 24)
FORCING_SCALE, FORCING_W0 = 20.0, 0.05


def forcing_pair():
    """(x, p [B, M, N] float64, f [M, N]): a small initial vorticity (FORCING_W0 x the GRF) under FORCING_SCALE x the
    reference forcing, so that the forcing carries most of the step; second and third snapshots as above"""
    hit = _TRAJ.get("forcing")
    if hit is None:
        B, M, N = FORCING_CASE
        w0 = (FORCING_W0 / S.W0_SCALE) * S.initial_vorticity(B, M, N, seed=5)
        f = FORCING_SCALE * S.forcing(M, N)
        sol, _ = S.solve(w0, f, S.VISC, S.T_FINAL, S.DT, S.RECORD_STEPS)
        hit = _TRAJ["forcing"] = (sol[..., 1].contiguous(), sol[..., 2].contiguous(), f)
    return hit
