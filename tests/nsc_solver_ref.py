"""Restatement of the active-scalar Navier-Stokes generator with torch.fft (test infrastructure only; the product tree
does not import it), and the parity cases.  The grid, wavenumbers, lap, dealias, the schedule and the inputs' helpers
are those of tests/ns_solver_ref.py.  The state is (W, C) = (rfft2(w), rfft2(c)), unnormalised.  One step:

    psi = W / lap,  q = irfft2(2 pi i k2 psi),  v = irfft2(-2 pi i k1 psi)                     velocity u = (q, v)
    w_1, w_2 = irfft2(2 pi i k1 W), irfft2(2 pi i k2 W);   c_1, c_2 = irfft2(2 pi i k1 C), irfft2(2 pi i k2 C)
    F_w = dealias (rfft2(q w_1 + v w_2) - beta 2 pi i k1 C)       buoyancy along axis 2: curl = beta dc/dx1, old C
    F_c = dealias rfft2(q c_1 + v c_2)
    W <- (-dt F_w + dt f_h + (1 - a) W) / (1 + a),   a = dt visc lap / 2
    C <- (-dt F_c + (1 - b) C) / (1 + b),            b = dt kappa lap / 2

A snapshot holds (c, q, v) and the vorticity w.  Everything in float64 by default: the yardstick.
``dtype=torch.float32`` runs the same restatement in single precision: its distance from the float64 run is the floor
the device is measured against.  ``advection=False`` drops both advection terms, ``buoyancy=False`` the beta term: the
tests use them to show that the inputs make these terms matter."""
from __future__ import annotations

import math

import torch

from tests import ns_solver_ref as R

# (B, M, N): the NS generator's cases, then its edges of the group layout, K = N/2+1 = 4, 5, 6, 7, 4
CASES = list(R.CASES) + list(R.EDGE_CASES)
VISC, KAPPA, BETA = 1e-3, 2e-3, 5.0          # visc != kappa on purpose: swapped tables show
DT, T_FINAL, RECORD_STEPS = 2e-3, 0.2, 4
FLOOR_FACTOR = R.FLOOR_FACTOR
CHANNELS = ("c", "q", "v", "w")
case_id = R.case_id
rel = R.rel


def tables(M, N, visc, kappa, dt):
    """float64 [M, K]: (c_w, c_f, d_w, d_f, c_g, inv_lap)"""
    k1, k2 = R.wavenumbers(M, N)
    lap = 4 * math.pi ** 2 * (k1 ** 2 + k2 ** 2)
    dealias = ((k1.abs() <= (2.0 / 3.0) * (M // 2)) & (k2.abs() <= (2.0 / 3.0) * (N // 2))).to(torch.float64)
    a, b = 0.5 * dt * visc * lap, 0.5 * dt * kappa * lap
    poisson = lap.clone()
    poisson[0, 0] = 1.0
    return (1 - a) / (1 + a), dt * dealias / (1 + a), (1 - b) / (1 + b), dt * dealias / (1 + b), dt / (1 + a), 1 / poisson


def initial_scalar(B, M, N, seed):
    """0.5 + 2 x GRF(alpha = 2.5, tau = 7) from seeded float64 noise, float64 [B, M, N]"""
    return 0.5 + 2.0 * R.grf(R.noise64(B, M, N, seed), R.sqrt_eig(M, N, 2.5, 7))


def fields_of(W, C, M, N, dtype=torch.float64):
    """spectra [B, M, K] -> [B, 3, M, N] = (c, q, v)"""
    k1, k2 = R.wavenumbers(M, N, dtype)
    lap = 4 * math.pi ** 2 * (k1 ** 2 + k2 ** 2)
    lap[0, 0] = 1.0
    two_pi_i = torch.tensor(2j * math.pi, dtype=R._cdtype(dtype))
    inv = lambda z: torch.fft.irfft2(z, s=(M, N))                               # noqa: E731
    psi = W / lap
    return torch.stack([inv(C), inv(two_pi_i * k2 * psi), inv(-two_pi_i * k1 * psi)], dim=1)


def solve(w0, c0, f, visc, kappa, beta, T, dt, record_steps, dtype=torch.float64, advection=True, buoyancy=True):
    """-> fields [B, record_steps, 3, M, N] = (c, q, v), vorticity [B, record_steps, M, N], times [record_steps], of `dtype`"""
    w0, c0, f = w0.to(dtype), c0.to(dtype), f.to(dtype)
    B, M, N = w0.shape
    k1, k2 = R.wavenumbers(M, N, dtype)
    lap = 4 * math.pi ** 2 * (k1 ** 2 + k2 ** 2)
    poisson = lap.clone()
    poisson[0, 0] = 1.0
    dealias = ((k1.abs() <= (2.0 / 3.0) * (M // 2)) & (k2.abs() <= (2.0 / 3.0) * (N // 2))).to(dtype)
    a, b = 0.5 * dt * visc * lap, 0.5 * dt * kappa * lap
    W, C = torch.fft.rfft2(w0), torch.fft.rfft2(c0)
    f_h = torch.fft.rfft2(f)
    if f_h.dim() == 2:
        f_h = f_h.unsqueeze(0)
    steps, record_time, times = R.schedule(T, dt, record_steps)
    two_pi_i = torch.tensor(2j * math.pi, dtype=R._cdtype(dtype))
    inv = lambda z: torch.fft.irfft2(z, s=(M, N))                               # noqa: E731
    fields = torch.zeros(B, record_steps, 3, M, N, dtype=dtype)
    vort = torch.zeros(B, record_steps, M, N, dtype=dtype)
    n = 0
    for j in range(steps):
        if advection:
            psi = W / poisson
            q, v = inv(two_pi_i * k2 * psi), inv(-two_pi_i * k1 * psi)
            adv_w = torch.fft.rfft2(q * inv(two_pi_i * k1 * W) + v * inv(two_pi_i * k2 * W))
            adv_c = torch.fft.rfft2(q * inv(two_pi_i * k1 * C) + v * inv(two_pi_i * k2 * C))
        else:
            adv_w, adv_c = torch.zeros_like(W), torch.zeros_like(C)
        F_w = dealias * (adv_w - beta * (two_pi_i * k1 * C)) if buoyancy else dealias * adv_w
        F_c = dealias * adv_c
        W = (-dt * F_w + dt * f_h + (1.0 - a) * W) / (1.0 + a)
        C = (-dt * F_c + (1.0 - b) * C) / (1.0 + b)
        if (j + 1) % record_time == 0 and n < record_steps:
            fields[:, n] = fields_of(W, C, M, N, dtype)
            vort[:, n] = inv(W)
            n += 1
    return fields, vort, torch.tensor(times, dtype=dtype)


def channel(fields, vort, ch, n):
    """channel ch of CHANNELS at snapshot n, [B, M, N]"""
    return vort[:, n] if ch == 3 else fields[:, n, ch]


def floors(f32, v32, f64, v64):
    """[4][snapshots]: the rel-L2 distance of a run from the float64 run, per channel (c, q, v, w) and snapshot"""
    return [[rel(channel(f32, v32, ch, n), channel(f64, v64, ch, n)) for n in range(f64.shape[1])] for ch in range(4)]


def mean_free(c):
    return c - c.mean(dim=(-2, -1), keepdim=True)


# ---- a closed form that uses none of the code above ------------------------------------------------------------------
def closed_form_inputs():
    """w0 = cos theta, c0 = 0.5 + 0.7 cos theta, theta = 2 pi (3x + 2y) on 32 x 48, f = 0: every field is a function of
    theta, so both advection terms vanish.  -> (w0, c0, f [1, M, N] / [M, N] float64, parameters)"""
    M, N = 32, 48
    x = (torch.arange(M, dtype=torch.float64) / M).view(M, 1)
    y = (torch.arange(N, dtype=torch.float64) / N).view(1, N)
    theta = 2 * math.pi * (3 * x + 2 * y)
    par = dict(visc=1e-2, kappa=2e-3, beta=5.0, dt=1e-2, steps=50)
    return torch.cos(theta)[None], (0.5 + 0.7 * torch.cos(theta))[None], torch.zeros(M, N, dtype=torch.float64), theta, par


def closed_form(theta, visc, kappa, beta, dt, steps):
    """the coefficients of e^{i theta} (cos theta = Re e^{i theta}): W^ <- c_w W^ + c_f beta 2 pi i 3 C^, C^ <- d_w C^ with
    lap = 4 pi^2 13; the mean of c stays.  -> (w, c) [M, N] float64 after `steps` steps"""
    lap = 4 * math.pi ** 2 * 13
    a, b = 0.5 * dt * visc * lap, 0.5 * dt * kappa * lap
    c_w, c_f, d_w = (1 - a) / (1 + a), dt / (1 + a), (1 - b) / (1 + b)
    Wh, Ch = complex(1.0), complex(0.7)
    for _ in range(steps):
        Wh, Ch = c_w * Wh + c_f * beta * 2j * math.pi * 3 * Ch, d_w * Ch
    e = torch.exp(1j * theta)
    return (Wh * e).real, 0.5 + (Ch * e).real


_PARITY: dict = {}


def parity_reference(case):
    """{w0, c0, f, fields64, vort64, t64, floor32 [4][RECORD_STEPS], buoyancy_share, advection_share}: computed once per
    case and shared; read-only"""
    hit = _PARITY.get(case)
    if hit is not None:
        return hit
    B, M, N = case
    w0 = R.initial_vorticity(B, M, N, seed=11 + M + N)
    c0 = initial_scalar(B, M, N, seed=101 + M + N)
    f = R.forcing(M, N)
    args = (VISC, KAPPA, BETA, T_FINAL, DT, RECORD_STEPS)
    f64, v64, t64 = solve(w0, c0, f, *args)
    # the floor sees what the device sees: float32 inputs
    f32, v32, _ = solve(w0.float(), c0.float(), f.float(), *args, dtype=torch.float32)
    nb, _, _ = solve(w0, c0, f, *args, buoyancy=False)
    na, _, _ = solve(w0, c0, f, *args, advection=False)
    out = dict(w0=w0, c0=c0, f=f, fields64=f64, vort64=v64, t64=t64, floor32=floors(f32, v32, f64, v64),
               buoyancy_share=rel(nb[:, -1, 1:], f64[:, -1, 1:]),
               advection_share=rel(mean_free(na[:, -1, 0]), mean_free(f64[:, -1, 0])))
    _PARITY[case] = out
    return out
