"""Restatement of the 1-D exponential-time-differencing generator for a symbol with odd derivatives, with torch.fft
(test infrastructure only; the product tree does not import it), and the parity cases of the complex path.  Grid,
transforms, Nhat, g and the step sequence are those of tests/etd1d_ref.py; what changes is the symbol and the contour:

    l_n = c2 kappa_n^2 + c4 kappa_n^4 + i (c1 kappa_n + c3 kappa_n^3),  Im l_{N/2} = 0

    KdV            u_t + u u_x + delta u_xxx = nu u_xx      c3 = +delta, c2 = -nu
    advection      u_t + a u_x = ...                        c1 = -a

(d_x -> i kappa, so d_xxx -> -i kappa^3 and -delta u_xxx is +i delta kappa^3.)  An odd derivative of the Nyquist mode
vanishes on the grid, g_{N/2} = 0 already, and with a real E at N/2 the Nyquist bin of a real field stays real.

z = h l_n is complex, so the Kassam-Trefethen mean runs over the full circle and keeps its imaginary part:
LR = z + r_m, r_m = exp(2 pi i (m - 1/2) / 64), m = 1 .. 64, <.> the complex mean over m,

    E = e^z,  E2 = e^(z/2),  Q = h <(e^(LR/2) - 1) / LR>
    f1 = h <(-4 - LR + e^LR (4 - 3 LR + LR^2)) / LR^3>
    f2 = h <(2 + LR + e^LR (-2 + LR)) / LR^3>
    f3 = h <(-4 - 3 LR - LR^2 + e^LR (4 - LR)) / LR^3>

and where z is real (the mean and Nyquist modes, an even symbol) the imaginary part of all six is zero.

Two wrong variants are kept for the tests that show the inputs tell them apart: ``variant="half"`` takes Q, f1, f2, f3
as h Re<.> over the upper half circle (the real path's rule, right for real z only) beside the exact E, E2, and
``variant="real"`` drops the imaginary part of all six full-circle tables.

Everything in float64 / complex128 by default: the yardstick.  ``dtype=torch.float32`` runs the same restatement in
single precision, tables included (contour in complex64): its distance from the float64 run on the same inputs is the
floor (`floor32`) the device is measured against.  ``nonlinear=False`` drops Nhat."""
from __future__ import annotations

import math

import torch

from tests.etd1d_ref import CASES, FLOOR_FACTOR, SNAPSHOTS, STEPS, _cdtype, case_id, ks_initial, rel  # noqa: F401

# the two parity families, on CASES with L = N / 4 and lmax = min(8, N // 5); seed 59 + N
FAMILIES = {
    #           c1    c2    c3   c4   amplitude  dt
    "kdv":     (0.0,  0.0,  1.0, 0.0, 4.0,       0.01),
    "advburg": (-1.0, -0.1, 0.0, 0.0, 3.0,       0.005),
}


def tables(N, length, c1, c2, c3, c4, dt, advect=1.0, dealias=True, dtype=torch.float64, variant="full"):
    """(E, E2, Q, f1, f2, f3, g): six complex [N/2 + 1] of the complex type of `dtype`, g real [N/2 + 1]"""
    K = N // 2 + 1
    cd = _cdtype(dtype)
    n = torch.arange(K, dtype=dtype)
    kappa = (2.0 * math.pi / float(length)) * n
    odd = float(c1) * kappa + float(c3) * kappa ** 3
    odd[N // 2] = 0.0
    h = float(dt)
    z = h * torch.complex(float(c2) * kappa ** 2 + float(c4) * kappa ** 4, odd)
    if variant == "half":
        m = torch.arange(1, 33, dtype=dtype)
        r = torch.polar(torch.ones(32, dtype=dtype), math.pi * (m - 0.5) / 32.0)
        mean = lambda t: t.mean(dim=1).real.to(cd)                        # noqa: E731
    else:
        m = torch.arange(1, 65, dtype=dtype)
        r = torch.polar(torch.ones(64, dtype=dtype), 2.0 * math.pi * (m - 0.5) / 64.0)
        mean = lambda t: t.mean(dim=1)                                    # noqa: E731
    LR = z.view(K, 1) + r.view(1, -1)
    eLR = torch.exp(LR)
    six = [torch.exp(z), torch.exp(z / 2.0),
           h * mean((torch.exp(LR / 2.0) - 1.0) / LR),
           h * mean((-4.0 - LR + eLR * (4.0 - 3.0 * LR + LR ** 2)) / LR ** 3),
           h * mean((2.0 + LR + eLR * (-2.0 + LR)) / LR ** 3),
           h * mean((-4.0 - 3.0 * LR - LR ** 2 + eLR * (4.0 - LR)) / LR ** 3)]
    # real z: the circle's points pair up as conjugates, the mean is real and its imaginary rounding residue is dropped
    six = [torch.complex(t.real, torch.where(z.imag == 0, torch.zeros_like(t.imag), t.imag)) for t in six]
    if variant == "real":
        six = [t.real.to(cd) for t in six]
    elif variant not in ("full", "half"):
        raise ValueError(variant)
    keep = (n <= (2.0 / 3.0) * (N // 2)).to(dtype) if dealias else torch.ones(K, dtype=dtype)
    g = -(float(advect) / 2.0) * kappa * keep
    g[N // 2] = 0.0
    return (*six, g)


def solve(u0, length, c1, c2, c3, c4, dt, steps, record_every, dtype=torch.float64, advect=1.0, dealias=True,
          nonlinear=True, variant="full"):
    """u0 [B, N] -> [B, steps // record_every, N] of `dtype`: irfft of the state after every record_every-th step"""
    u0 = u0.to(dtype)
    B, N = u0.shape
    E, E2, Q, f1, f2, f3, g = tables(N, length, c1, c2, c3, c4, dt, advect, dealias, dtype, variant)
    ig = torch.complex(torch.zeros_like(g), g)
    inv = lambda w: torch.fft.irfft(w, n=N)                               # noqa: E731
    if nonlinear:
        nl = lambda w: ig * torch.fft.rfft(inv(w) ** 2)                   # noqa: E731
    else:
        nl = lambda w: torch.zeros_like(w)                                # noqa: E731
    v = torch.fft.rfft(u0)
    out = torch.zeros(B, steps // record_every, N, dtype=dtype)
    for j in range(steps):
        Nv = nl(v)
        a = E2 * v + Q * Nv
        Na = nl(a)
        b = E2 * v + Q * Na
        Nb = nl(b)
        c = E2 * a + Q * (2.0 * Nb - Nv)
        Nc = nl(c)
        v = E * v + f1 * Nv + 2.0 * f2 * (Na + Nb) + f3 * Nc
        if (j + 1) % record_every == 0 and (j + 1) // record_every <= out.shape[1]:
            out[:, (j + 1) // record_every - 1] = inv(v)
    return out


def soliton(N, length, c, x0, t):
    """the KdV soliton of u_t + u u_x + u_xxx = 0, u = 3 c sech^2(sqrt(c) (x - x0 - c t) / 2), on x = i L / N, wrapped
    to the period (its tails are below e^(-sqrt(c) L / 2) there); float64 [1, N]"""
    x = torch.arange(N, dtype=torch.float64) * (float(length) / N)
    s = torch.remainder(x - x0 - c * t + 0.5 * length, length) - 0.5 * length
    return (3.0 * c / torch.cosh(0.5 * math.sqrt(c) * s) ** 2)[None]


def advection_diffusion(N, L, a, nu, t):
    """0.5 + 0.3 cos(kappa_3 (x - a t)) e^(-nu kappa_3^2 t) + 0.2 cos(kappa_7 (x - a t) + 0.7) e^(-nu kappa_7^2 t): the
    solution of u_t + a u_x = nu u_xx from its value at t = 0 (mode n is multiplied by exp(t (-nu kappa^2 - i a kappa)))"""
    x = torch.arange(N, dtype=torch.float64) * (L / N)
    out = torch.full((N,), 0.5, dtype=torch.float64)
    for n, amp, ph in ((3, 0.3, 0.0), (7, 0.2, 0.7)):
        k = 2 * math.pi * n / L
        out = out + amp * math.exp(-nu * k * k * t) * torch.cos(k * (x - a * t) + ph)
    return out[None]


ADV = dict(N=64, L=2.0, a=1.5, nu=0.02, dt=0.01, steps=50)


def setup(family, case):
    """(u0 float64 [B, N], length, (c1, c2, c3, c4), dt) of a parity case"""
    B, N = case
    c1, c2, c3, c4, amp, dt = FAMILIES[family]
    length = N / 4.0
    return amp * ks_initial(B, N, length, min(8, N // 5), seed=59 + N), length, (c1, c2, c3, c4), dt


_PARITY: dict = {}


def parity_reference(family, case):
    """{u0, length, c1, c2, c3, c4, dt, sol64 [B, SNAPSHOTS, N], floor32 [SNAPSHOTS], nonlinear_share, imaginary_share}:
    computed once per case and shared; read-only.  The shares are relative distances at the last snapshot from the
    float64 run: of the run without Nhat, and of the run with c1 = c3 = 0."""
    hit = _PARITY.get((family, case))
    if hit is not None:
        return hit
    u0, length, (c1, c2, c3, c4), dt = setup(family, case)
    every = STEPS // SNAPSHOTS
    sol64 = solve(u0, length, c1, c2, c3, c4, dt, STEPS, every)
    # the floor sees what the device sees: float32 inputs
    sol32 = solve(u0.float(), length, c1, c2, c3, c4, dt, STEPS, every, dtype=torch.float32)
    lin = solve(u0, length, c1, c2, c3, c4, dt, STEPS, every, nonlinear=False)
    even = solve(u0, length, 0.0, c2, 0.0, c4, dt, STEPS, every)
    out = dict(u0=u0, length=length, c1=c1, c2=c2, c3=c3, c4=c4, dt=dt, sol64=sol64,
               floor32=[rel(sol32[:, c], sol64[:, c]) for c in range(SNAPSHOTS)],
               nonlinear_share=rel(lin[:, -1], sol64[:, -1]),
               imaginary_share=rel(even[:, -1], sol64[:, -1]))
    _PARITY[(family, case)] = out
    return out
