"""Restatement of the active-scalar equation-residual loss with torch.fft (test infrastructure only; the product tree
does not import it), and the parity cases.

Grid, k1, k2, lap, dealias, the discrete advection and the buoyancy term are those of tests/nsc_solver_ref.py (the
generator's); the tables E - 1, m0, m1 are tests/ns_residual_ref.tables, once per diffusivity.  The data are not the
evolved variable: the network sees (c, q, v), the equation evolves (w, c) with w = curl u.  With x = (c, q, v)(t) and
p ~ (c, q, v)(t + D), both [B, 3, M, N], p~ = a_p p + b_p, x~ = a_x x + b_x, d = p~ - x~ formed in physical space:

    X_c = x^_c,  X_w = 2 pi i k1 x^_v - 2 pi i k2 x^_q      (likewise D_c, D_w from d^;  P = X + D)
    N_w(W, C) = dealias (rfft2(q w_1 + v w_2) - beta 2 pi i k1 C),   N_c(W, C) = dealias rfft2(q c_1 + v c_2),
        q, v from psi = W / lap: only the solenoidal part of a predicted velocity advects
    r^_w = D_w - (E_nu - 1) X_w + m0_nu N_w(X) + m1_nu N_w(P) - (m0_nu + m1_nu) f^          z = -D visc lap
    r^_c = D_c - (E_kappa - 1) X_c + m0_kappa N_c(X) + m1_kappa N_c(P)                      z = -D kappa lap
    delta^ = 2 pi i k1 P_q + 2 pi i k2 P_v      the divergence of the predicted velocity
    mu = (d^_q[0, 0], d^_v[0, 0])               the change of the mean velocity (the equation conserves it)
    E_ru = sum_{k != 0} c (|r^_w|^2 + |delta^|^2) / lap / (M N) + |mu|^2 / (M N),   E_rc = sum c |r^_c|^2 / (M N)
    E_xu = E(x^_q) + E(x^_v),  E_xc = E(x^_c),   c = 1 on the columns kx = 0, N/2, else 2
    rel[b] = sqrt(lambda E_rc + E_ru) / (sqrt(lambda E_xc + E_xu) + 1e-8)

The forcing is not de-aliased (the generator adds it as it stands).  The gradient comes from autograd; `grad_formula` is
the closed form the device implements, the exact adjoint of the discrete operator: with rho_w = r^_w / lap (0 at the
mean mode), rho_c = lambda r^_c, rho_d = delta^ / lap, g_w = irfft2(m1_nu rho_w), g_c = irfft2(m1_kappa rho_c) and the six
fields of P,

    G_w = rho_w + conj(2 pi i k2 / lap) rfft2(g_w w_1 + g_c c_1) + conj(-2 pi i k1 / lap) rfft2(g_w w_2 + g_c c_2)
                + conj(2 pi i k1) rfft2(g_w q) + conj(2 pi i k2) rfft2(g_w v)
    G_c = rho_c + conj(2 pi i k1) rfft2(g_c q) + conj(2 pi i k2) rfft2(g_c v) + conj(-beta 2 pi i k1) m1_nu rho_w
    grad p_c = irfft2(G_c),   grad p_q = irfft2(conj(-2 pi i k2) G_w + conj(2 pi i k1) rho_d + [k = 0] mu_q),
    grad p_v = irfft2(conj(2 pi i k1) G_w + conj(2 pi i k2) rho_d + [k = 0] mu_v),     all times a_p coef_b,
    coef_b = 1 / (sqrt(E_r) (sqrt(E_x) + 1e-8)).

Everything in float64 / complex128 by default: the yardstick.  ``dtype=torch.float32`` runs the same restatement in single
precision, tables included: its distance from the float64 run on the same fp32 inputs is the floor the device is
measured against."""
from __future__ import annotations

import math

import torch

from tests import ns_residual_ref as V
from tests import ns_solver_ref as S
from tests import nsc_solver_ref as G
from tests.ns_residual_ref import IDENTITY, KINDS, MIN_FLOOR  # noqa: F401
from tests.nsc_solver_ref import BETA, CASES, FLOOR_FACTOR, KAPPA, VISC, case_id  # noqa: F401

INTERVAL = 0.05                      # between consecutive snapshots of nsc_solver_ref's schedule (25 steps of DT)


def tables(M, N, visc, kappa, interval, dtype=torch.float64):
    """(T_nu, T_kappa): ns_residual_ref.tables once per diffusivity"""
    return V.tables(M, N, visc, interval, dtype=dtype), V.tables(M, N, kappa, interval, dtype=dtype)


def forcing_term(f, T):
    """(m0_nu + m1_nu) rfft2(f), not de-aliased, from T = (T_nu, T_kappa); None for no forcing"""
    return V.forcing_term(f, T[0])


def _i2pi(z):
    return torch.tensor(2j * math.pi, dtype=z.dtype)


def curl(Q, Vv, T):
    """W = 2 pi i k1 V - 2 pi i k2 Q of velocity spectra"""
    return _i2pi(Q) * (T["k1"] * Vv - T["k2"] * Q)


def six_fields(W, C, T):
    """(q, v, w_1, w_2, c_1, c_2) of the spectra W, C"""
    M, N = T["M"], T["N"]
    inv = lambda z: torch.fft.irfft2(z, s=(M, N))          # noqa: E731
    q, v, w1, w2 = V.fields(W, T)
    return q, v, w1, w2, inv(_i2pi(C) * T["k1"] * C), inv(_i2pi(C) * T["k2"] * C)


def nonlinear(W, C, T, beta):
    """(N_w, N_c) before de-aliasing (m0 and m1 carry the mask)"""
    q, v, w1, w2, c1, c2 = six_fields(W, C, T)
    return torch.fft.rfft2(q * w1 + v * w2) - beta * _i2pi(C) * T["k1"] * C, torch.fft.rfft2(q * c1 + v * c2)


def spectrum(p, x, T, beta, fterm=None, affine=IDENTITY):
    """dict(rw, rc, delta, mu [B, 2], Xc, Xq, Xv, Pw, Pc) in the dtype of p; p, x [B, 3, M, N] = (c, q, v)"""
    Tn, Tk = T
    ap, bp, ax, bx = affine
    pt, xt = ap * p + bp, ax * x + bx
    X = torch.fft.rfft2(xt)
    D = torch.fft.rfft2(pt - xt)
    Xc, Xw = X[:, 0], curl(X[:, 1], X[:, 2], Tn)
    Dc, Dw = D[:, 0], curl(D[:, 1], D[:, 2], Tn)
    Pc, Pw = Xc + Dc, Xw + Dw
    nwx, ncx = nonlinear(Xw, Xc, Tn, beta)
    nwp, ncp = nonlinear(Pw, Pc, Tn, beta)
    rw = Dw - Tn["em1"] * Xw + Tn["m0"] * nwx + Tn["m1"] * nwp
    if fterm is not None:
        rw = rw - fterm
    rc = Dc - Tk["em1"] * Xc + Tk["m0"] * ncx + Tk["m1"] * ncp
    Pq, Pv = X[:, 1] + D[:, 1], X[:, 2] + D[:, 2]
    delta = _i2pi(Pq) * (Tn["k1"] * Pq + Tn["k2"] * Pv)
    mu = torch.stack([D[:, 1, 0, 0].real, D[:, 2, 0, 0].real], dim=1)
    return dict(rw=rw, rc=rc, delta=delta, mu=mu, Xc=Xc, Xq=X[:, 1], Xv=X[:, 2], Pw=Pw, Pc=Pc)


def _inv_lap(T):
    il = 1.0 / T["poisson"]
    il = il.clone()
    il[0, 0] = 0.0
    return il


def energies(s, T, scalar_weight=1.0):
    """dict(ru, rc, xu, xc, r, x): the four energies [B] and the two weighted sums"""
    M, N = T[0]["M"], T[0]["N"]
    e = V._energy
    il = _inv_lap(T[0])
    ru = e(s["rw"] * torch.sqrt(il), M, N) + e(s["delta"] * torch.sqrt(il), M, N) + (s["mu"] ** 2).sum(1) / (M * N)
    rc = e(s["rc"], M, N)
    xu, xc = e(s["Xq"], M, N) + e(s["Xv"], M, N), e(s["Xc"], M, N)
    lam = float(scalar_weight)
    return dict(ru=ru, rc=rc, xu=xu, xc=xc, r=lam * rc + ru, x=lam * xc + xu)


def rel(p, x, T, beta, fterm=None, affine=IDENTITY, scalar_weight=1.0):
    """rel [B] in the dtype of p; differentiable in p"""
    E = energies(spectrum(p, x, T, beta, fterm, affine), T, scalar_weight)
    return V._root(E["r"]) / (torch.sqrt(E["x"]) + 1e-8)


def rel_parts(p, x, T, beta, fterm=None, affine=IDENTITY):
    """(rel of the velocity part, rel of the concentration part) [B] each, each against its own norm of x"""
    E = energies(spectrum(p, x, T, beta, fterm, affine), T)
    return V._root(E["ru"]) / (torch.sqrt(E["xu"]) + 1e-8), V._root(E["rc"]) / (torch.sqrt(E["xc"]) + 1e-8)


def rel_and_grad(p, x, T, beta, fterm=None, affine=IDENTITY, scalar_weight=1.0, weights=None):
    """(rel [B], d (sum_b weights_b rel_b) / d p) through autograd, in the dtype of p; weights default to 1"""
    p = p.detach().clone().requires_grad_(True)
    v = rel(p, x, T, beta, fterm, affine, scalar_weight)
    w = torch.ones_like(v) if weights is None else weights.to(v.dtype)
    (grad,) = torch.autograd.grad((v * w).sum(), p)
    return v.detach(), grad


def grad_formula(p, x, T, beta, fterm=None, affine=IDENTITY, scalar_weight=1.0, weights=None):
    """the closed form of d (sum_b weights_b rel_b) / d p that the device implements"""
    Tn, Tk = T
    M, N = Tn["M"], Tn["N"]
    s = spectrum(p, x, T, beta, fterm, affine)
    E = energies(s, T, scalar_weight)
    rn, xn = torch.sqrt(E["r"]), torch.sqrt(E["x"])
    w = torch.ones_like(rn) if weights is None else weights.to(rn.dtype)
    coef = torch.where(rn > 0, w / (torch.where(rn > 0, rn, torch.ones_like(rn)) * (xn + 1e-8)), torch.zeros_like(rn))
    il = _inv_lap(Tn)
    rho_w, rho_c, rho_d = s["rw"] * il, float(scalar_weight) * s["rc"], s["delta"] * il
    inv = lambda z: torch.fft.irfft2(z, s=(M, N))          # noqa: E731
    f = torch.fft.rfft2
    gw, gc = inv(Tn["m1"] * rho_w), inv(Tk["m1"] * rho_c)
    q, v, w1, w2, c1, c2 = six_fields(s["Pw"], s["Pc"], Tn)
    i2pi = _i2pi(rho_w)
    k1, k2 = Tn["k1"], Tn["k2"]
    cj = torch.conj
    Gw = (rho_w + cj(i2pi * k2 / Tn["poisson"]) * f(gw * w1 + gc * c1) + cj(-i2pi * k1 / Tn["poisson"]) * f(gw * w2 + gc * c2)
          + cj(i2pi * k1) * f(gw * q) + cj(i2pi * k2) * f(gw * v))
    Gc = rho_c + cj(i2pi * k1) * f(gc * q) + cj(i2pi * k2) * f(gc * v) + cj(-beta * i2pi * k1) * (Tn["m1"] * rho_w)
    Hq = cj(-i2pi * k2) * Gw + cj(i2pi * k1) * rho_d
    Hv = cj(i2pi * k1) * Gw + cj(i2pi * k2) * rho_d
    dc = torch.zeros_like(Hq)
    dc[:, 0, 0] = 1.0
    Hq = Hq + dc * s["mu"][:, 0, None, None]
    Hv = Hv + dc * s["mu"][:, 1, None, None]
    return affine[0] * coef[:, None, None, None] * torch.stack([inv(Gc), inv(Hq), inv(Hv)], dim=1)


_TRAJ: dict = {}


def trajectory(case, forced=True):
    """[B, RECORD_STEPS, 3, M, N] float64: nsc_solver_ref's snapshots INTERVAL apart at its own constants, with its
    forcing or with none"""
    hit = _TRAJ.get((case, forced))
    if hit is None:
        if forced:
            hit = G.parity_reference(case)["fields64"]
        else:
            B, M, N = case
            w0 = S.initial_vorticity(B, M, N, seed=11 + M + N)
            c0 = G.initial_scalar(B, M, N, seed=101 + M + N)
            hit, _, _ = G.solve(w0, c0, torch.zeros(M, N, dtype=torch.float64), VISC, KAPPA, BETA, G.T_FINAL, G.DT,
                                G.RECORD_STEPS)
        _TRAJ[(case, forced)] = hit
    return hit


def _floors(rel32, grad32, rel64, grad64):
    return (max(MIN_FLOOR, float(((rel32.double() - rel64).abs() / rel64).max())),
            max(MIN_FLOOR, float((grad32.double() - grad64).norm() / grad64.norm())))


_PARITY: dict = {}


def parity_reference(case, kind, forced):
    """{x, p (fp32 [B, 3, M, N], what the device sees), f (float64 [M, N] or None), T64, fterm64, rel64, grad64 (of
    sum_b rel_b), still64 (rel of p = x), floor_rel, floor_grad}: computed once per case and shared; read-only.  x is
    the second recorded snapshot, p the third (kind "exact") or the third plus Gaussian noise of a tenth of its rms
    (kind "noisy"); `forced`: data and loss with ns_solver_ref's forcing, or both with none.  The floors are the float32
    restatement's own errors on the same fp32 inputs -- rel: the largest relative error over the samples, grad: relative
    L2 of the whole tensor -- and never below MIN_FLOOR."""
    hit = _PARITY.get((case, kind, forced))
    if hit is not None:
        return hit
    B, M, N = case
    sol = trajectory(case, forced)
    x, p = sol[:, 1], sol[:, 2]
    if kind == "noisy":
        gen = torch.Generator().manual_seed(97 + M + N)
        p = p + 0.1 * p.pow(2).mean().sqrt() * torch.randn(B, 3, M, N, generator=gen, dtype=torch.float64)
    elif kind != "exact":
        raise ValueError(kind)
    x, p = x.float().contiguous(), p.float().contiguous()
    f = S.forcing(M, N) if forced else None
    T64, T32 = tables(M, N, VISC, KAPPA, INTERVAL), tables(M, N, VISC, KAPPA, INTERVAL, dtype=torch.float32)
    ft64, ft32 = forcing_term(f, T64), forcing_term(f, T32)
    rel64, grad64 = rel_and_grad(p.double(), x.double(), T64, BETA, ft64)
    rel32, grad32 = rel_and_grad(p, x, T32, BETA, ft32)
    floor_rel, floor_grad = _floors(rel32, grad32, rel64, grad64)
    out = dict(x=x, p=p, f=f, T64=T64, fterm64=ft64, rel64=rel64, grad64=grad64,
               still64=rel(x.double(), x.double(), T64, BETA, ft64), floor_rel=floor_rel, floor_grad=floor_grad)
    _PARITY[(case, kind, forced)] = out
    return out


def floors(p, x, M, N, visc, kappa, beta, interval, f=None, affine=IDENTITY, scalar_weight=1.0, weights=None):
    """(rel64, grad64, bound_rel, bound_grad) of fp32 inputs: FLOOR_FACTOR x the float32 restatement's own error, as above"""
    T64, T32 = tables(M, N, visc, kappa, interval), tables(M, N, visc, kappa, interval, dtype=torch.float32)
    rel64, grad64 = rel_and_grad(p.double(), x.double(), T64, beta, forcing_term(f, T64), affine, scalar_weight, weights)
    rel32, grad32 = rel_and_grad(p, x, T32, beta, forcing_term(f, T32), affine, scalar_weight, weights)
    fr, fg = _floors(rel32, grad32, rel64, grad64)
    return rel64, grad64, FLOOR_FACTOR * fr, FLOOR_FACTOR * fg


FORCING_CASE = (2, 16, 24)
FORCING_SCALE, FORCING_W0, FORCING_C0 = 20.0, 0.05, 0.05


def forcing_pair():
    """(x, p [B, 3, M, N] float64, f [M, N]): a small initial vorticity (FORCING_W0 x the GRF) and a nearly uniform scalar
    (0.5 + FORCING_C0 x the GRF) under FORCING_SCALE x the reference forcing, so that the forcing carries most of the
    step; second and third snapshots as above"""
    hit = _TRAJ.get("forcing")
    if hit is None:
        B, M, N = FORCING_CASE
        w0 = (FORCING_W0 / S.W0_SCALE) * S.initial_vorticity(B, M, N, seed=5)
        c0 = 0.5 + FORCING_C0 * S.grf(S.noise64(B, M, N, 7), S.sqrt_eig(M, N, 2.5, 7))
        f = FORCING_SCALE * S.forcing(M, N)
        sol, _, _ = G.solve(w0, c0, f, VISC, KAPPA, BETA, G.T_FINAL, G.DT, G.RECORD_STEPS)
        hit = _TRAJ["forcing"] = (sol[:, 1].contiguous(), sol[:, 2].contiguous(), f)
    return hit


def gradient_field(M, N, seed=3):
    """a pure gradient velocity (grad phi of a smooth random potential), [2, M, N] float64 with unit rms over both
    components: divergence without curl"""
    phi = torch.fft.rfft2(S.grf(S.noise64(1, M, N, seed), S.sqrt_eig(M, N, 2.5, 7))[0])
    k1, k2 = S.wavenumbers(M, N)
    # a potential without the Nyquist row and column: i k times them is not the spectrum of a real field
    phi = torch.where((k1.abs() == M // 2) | (k2 == N // 2), torch.zeros_like(phi), phi)
    g = torch.stack([torch.fft.irfft2(2j * math.pi * k1 * phi, s=(M, N)), torch.fft.irfft2(2j * math.pi * k2 * phi, s=(M, N))])
    return g / g.pow(2).mean().sqrt()
