"""Restatement of the equation-residual loss of the 1-D ETD family with torch.fft (test infrastructure only; the product
tree does not import it), and the parity cases.

Grid, kappa_n, the symbol l_n = c2 kappa_n^2 + c4 kappa_n^4 + i (c1 kappa_n + c3 kappa_n^3) (Im l_{N/2} = 0) and g are those
of tests/etd1d_cx_ref.py.  D is the time between the input x = u(t) and the prediction p ~ u(t + D).  The exact solution obeys

    u^(t + D) = e^(D l) u^(t) + int_0^D e^((D - s) l) Nhat(u(t + s)) ds,   Nhat(w) = i g rfft(w^2);

with Nhat interpolated linearly between the two ends (exponential trapezoidal rule, ETD2), z = D l_n, LR = z + r_m,
r_m = exp(2 pi i (m - 1/2) / 64), m = 1 .. 64, <.> the complex mean:

    r^ = p^ - E x^ - m0 rfft(x^2) - m1 rfft(p^2)
    E = e^z,  m0 = D (phi1 - phi2) i g,  m1 = D phi2 i g,  phi1 = <(e^LR - 1) / LR>,  phi2 = <(e^LR - 1 - LR) / LR^2>
    rel[b] = sqrt(E_r[b]) / (sqrt(E_x[b]) + 1e-8),  E(z)[b] = sum_n c_n |z^_n|^2 / N,  c_n = 1 at n = 0, N/2, else 2

on p~ = a_p p + b_p and x~ = a_x x + b_x.  The gradient comes from autograd; `grad_formula` is the closed form the device
implements,  d rel[b] / d p = a_p coef_b (irfft(r^) - 2 p~ irfft(conj(m1) r^)),  coef_b = g_b / (sqrt(E_r) (sqrt(E_x) + 1e-8)).

Everything in float64 / complex128 by default: the yardstick.  ``dtype=torch.float32`` runs the same restatement in single
precision, tables included (contour in complex64): its distance from the float64 run on the same fp32 inputs is the floor
the device is measured against, as in tests/etd1d_ref.py."""
from __future__ import annotations

import math

import torch

from tests import etd1d_cx_ref, etd1d_ref
from tests.etd1d_ref import FLOOR_FACTOR, _cdtype, case_id  # noqa: F401

# (B, N): K = N/2+1 = 4, 6, 7 and 1 (mod 4) -- every padding count of the last 16-byte group --, N % 4 != 0 (6, 10: the
# scalar tail of the physical-space kernels), odd B, and N = 512, the first grid with more than 64 groups per image
CASES = [(2, 6), (2, 10), (2, 12), (3, 16), (2, 48), (2, 64), (2, 200), (1, 512)]
# name -> (c1, c2, c3, c4, length(N), interval, the generating run's dt, amplitude of the initial condition)
SYMBOLS = {
    "burgers": (0.0, -0.1, 0.0, 0.0, lambda N: 2.0, 0.05, etd1d_ref.BURGERS_DT, 1.0),
    "ks":      (0.0, 1.0, 0.0, -0.05, lambda N: N / 4.0, 0.05, etd1d_ref.KS_DT, 1.0),
    "complex": (-0.3, -0.02, 1.0, 0.0, lambda N: N / 4.0, 0.07, 0.01, 2.0),
}
KINDS = ("noisy", "exact")           # p = the next snapshot plus 10 % Gaussian noise | the next snapshot itself
MIN_FLOOR = 2.0 ** -22               # four fp32 roundings of a stored scalar


def tables(N, length, c1, c2, c3, c4, interval, advect=1.0, dealias=True, dtype=torch.float64):
    """(E, m0, m1): complex [N/2 + 1] of the complex type of `dtype`"""
    K = N // 2 + 1
    n = torch.arange(K, dtype=dtype)
    kappa = (2.0 * math.pi / float(length)) * n
    odd = float(c1) * kappa + float(c3) * kappa ** 3
    odd[N // 2] = 0.0
    h = float(interval)
    z = h * torch.complex(float(c2) * kappa ** 2 + float(c4) * kappa ** 4, odd)
    m = torch.arange(1, 65, dtype=dtype)
    r = torch.polar(torch.ones(64, dtype=dtype), 2.0 * math.pi * (m - 0.5) / 64.0)
    LR = z.view(K, 1) + r.view(1, -1)
    eLR = torch.exp(LR)
    phi1 = ((eLR - 1.0) / LR).mean(dim=1)
    phi2 = ((eLR - 1.0 - LR) / LR ** 2).mean(dim=1)
    # real z: the circle's points pair up as conjugates, the mean is real and its imaginary rounding residue is dropped
    drop = lambda t: torch.complex(t.real, torch.where(z.imag == 0, torch.zeros_like(t.imag), t.imag))   # noqa: E731
    E, phi1, phi2 = drop(torch.exp(z)), drop(phi1), drop(phi2)
    keep = (n <= (2.0 / 3.0) * (N // 2)).to(dtype) if dealias else torch.ones(K, dtype=dtype)
    g = -(float(advect) / 2.0) * kappa * keep
    g[N // 2] = 0.0
    ig = torch.complex(torch.zeros_like(g), g)
    return E, h * (phi1 - phi2) * ig, h * phi2 * ig


def _energy(s, N):
    """sum_n c_n |s_n|^2 / N of half spectra [B, K]"""
    c = torch.full((N // 2 + 1,), 2.0, dtype=s.real.dtype)
    c[0] = c[N // 2] = 1.0
    return (c * (s.real ** 2 + s.imag ** 2)).sum(-1) / N


def spectrum(p, x, tabs, affine=(1.0, 0.0, 1.0, 0.0)):
    """(r^ [B, K], x~^ [B, K], p~ [B, N]) in the dtype of p"""
    E, m0, m1 = tabs
    ap, bp, ax, bx = affine
    pt, xt = ap * p + bp, ax * x + bx
    xs = torch.fft.rfft(xt)
    r = torch.fft.rfft(pt) - E * xs - m0 * torch.fft.rfft(xt * xt) - m1 * torch.fft.rfft(pt * pt)
    return r, xs, pt


def rel(p, x, tabs, affine=(1.0, 0.0, 1.0, 0.0)):
    """rel [B] in the dtype of p; differentiable in p"""
    N = p.shape[-1]
    r, xs, _ = spectrum(p, x, tabs, affine)
    e_r = _energy(r, N)
    pos = e_r > 0
    root = torch.where(pos, torch.sqrt(torch.where(pos, e_r, torch.ones_like(e_r))), torch.zeros_like(e_r))
    return root / (torch.sqrt(_energy(xs, N)) + 1e-8)


def rel_and_grad(p, x, tabs, affine=(1.0, 0.0, 1.0, 0.0), weights=None):
    """(rel [B], d (sum_b weights_b rel_b) / d p) through autograd, in the dtype of p; weights default to 1"""
    p = p.detach().clone().requires_grad_(True)
    v = rel(p, x, tabs, affine)
    w = torch.ones_like(v) if weights is None else weights.to(v.dtype)
    (grad,) = torch.autograd.grad((v * w).sum(), p)
    return v.detach(), grad


def grad_formula(p, x, tabs, affine=(1.0, 0.0, 1.0, 0.0), weights=None):
    """the closed form of d (sum_b weights_b rel_b) / d p that the device implements"""
    N = p.shape[-1]
    r, xs, pt = spectrum(p, x, tabs, affine)
    rn, xn = torch.sqrt(_energy(r, N)), torch.sqrt(_energy(xs, N))
    w = torch.ones_like(rn) if weights is None else weights.to(rn.dtype)
    coef = torch.where(rn > 0, w / (torch.where(rn > 0, rn, torch.ones_like(rn)) * (xn + 1e-8)), torch.zeros_like(rn))
    phys = torch.fft.irfft(r, n=N) - 2.0 * pt * torch.fft.irfft(torch.conj(tabs[2]) * r, n=N)
    return affine[0] * coef[:, None] * phys


def trajectory(symbol, case, interval=None, snapshots=3, fine=1, seed=None):
    """[B, snapshots, N] float64: snapshots of the float64 ETDRK4 restatement `interval` apart (the initial condition is
    not among them), the run's dt divided by `fine`"""
    B, N = case
    c1, c2, c3, c4, length, h, dt, amp = SYMBOLS[symbol]
    h = h if interval is None else float(interval)
    length = length(N)
    if symbol == "burgers":
        u0 = etd1d_ref.burgers_initial(B, N, seed=(71 + N) if seed is None else seed)
    else:
        u0 = amp * etd1d_ref.ks_initial(B, N, length, min(8, max(1, N // 5)), seed=(83 + N) if seed is None else seed)
    every = int(round(h / dt)) * fine
    assert abs(every * dt / fine - h) < 1e-12
    if c1 == 0.0 and c3 == 0.0:
        return etd1d_ref.solve(u0, length, c2, c4, dt / fine, snapshots * every, every)
    return etd1d_cx_ref.solve(u0, length, c1, c2, c3, c4, dt / fine, snapshots * every, every)


_PARITY: dict = {}


def parity_reference(symbol, case, kind):
    """{x, p (fp32 [B, N], what the device sees), tabs64, rel64, grad64 (of sum_b rel_b), floor_rel, floor_grad, length,
    interval, coefficients}: computed once per case and shared; read-only.  x is the second recorded snapshot, p the third
    (kind "exact") or the third plus Gaussian noise of a tenth of its rms (kind "noisy").  The floors are the float32
    restatement's own errors on the same fp32 inputs -- rel: the largest relative error over the samples, grad: relative L2
    of the whole tensor -- and never below MIN_FLOOR."""
    hit = _PARITY.get((symbol, case, kind))
    if hit is not None:
        return hit
    B, N = case
    c1, c2, c3, c4, length, h, _, _ = SYMBOLS[symbol]
    length = length(N)
    sol = trajectory(symbol, case)
    x, p = sol[:, 1], sol[:, 2]
    if kind == "noisy":
        gen = torch.Generator().manual_seed(97 + N)
        p = p + 0.1 * p.pow(2).mean().sqrt() * torch.randn(B, N, generator=gen, dtype=torch.float64)
    elif kind != "exact":
        raise ValueError(kind)
    x, p = x.float().contiguous(), p.float().contiguous()
    tabs64 = tables(N, length, c1, c2, c3, c4, h)
    tabs32 = tables(N, length, c1, c2, c3, c4, h, dtype=torch.float32)
    rel64, grad64 = rel_and_grad(p.double(), x.double(), tabs64)
    rel32, grad32 = rel_and_grad(p, x, tabs32)
    out = dict(x=x, p=p, tabs64=tabs64, rel64=rel64, grad64=grad64, length=length, interval=h, coefficients=(c1, c2, c3, c4),
               floor_rel=max(MIN_FLOOR, float(((rel32.double() - rel64).abs() / rel64).max())),
               floor_grad=max(MIN_FLOOR, float((grad32.double() - grad64).norm() / grad64.norm())))
    _PARITY[(symbol, case, kind)] = out
    return out
