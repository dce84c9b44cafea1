"""Restatement of the Navier-Stokes vorticity generator and its Gaussian random field with torch.fft (test
infrastructure only; the product tree does not import it), and the parity cases.

Unit periodic square, grid M x N (both even).  k1 = fftfreq(M) M (signed, Nyquist -M/2) on the first axis, k2 = 0 .. N/2
on the half axis, lap = 4 pi^2 (k1^2 + k2^2) with lap[0, 0] -> 1 in the Poisson division only,
dealias = |k1| <= (2/3)(M/2) and |k2| <= (2/3)(N/2).  One step, W = rfft2(w) unnormalised:

    psi = W / lap,  q = irfft2(2 pi i k2 psi),  v = irfft2(-2 pi i k1 psi),  w_x = irfft2(2 pi i k1 W),  w_y = irfft2(2 pi i k2 W)
    F = dealias rfft2(q w_x + v w_y)
    W <- (-dt F + dt f_h + (1 - a) W) / (1 + a),   a = dt visc lap / 2

steps = ceil(T / dt), record_time = floor(steps / record_steps), a snapshot irfft2(W) and its time (the running sum of
dt) after step j when (j + 1) % record_time == 0.

Everything in float64 by default: the yardstick.  ``dtype=torch.float32`` runs the same restatement in single precision:
its distance from the float64 run is the floor (`floor32`) the device is measured against.  ``advection=False`` drops the
nonlinear term: the tests use it to show that the inputs make that term matter."""
from __future__ import annotations

import math

import torch

# (B, M, N)
CASES = [(3, 8, 8), (2, 16, 24), (2, 32, 48), (1, 48, 32), (2, 64, 64)]
# the edges of the group layout, K = N/2+1 = 4, 5, 6, 7, 4: 0 .. 3 padded columns in the last 16-byte group, M above N
EDGE_CASES = [(2, 4, 6), (2, 4, 8), (2, 6, 10), (2, 4, 12), (2, 12, 6)]
VISC, DT, STEPS, RECORD_STEPS = 1e-3, 2e-3, 100, 4
T_FINAL = 0.2                      # STEPS * DT: ceil(0.2 / 2e-3) = 100
W0_SCALE, W0_ALPHA, W0_TAU = 8.0, 2.5, 7.0
FLOOR_FACTOR = 4.0                 # the bound on the device: FLOOR_FACTOR x the restatement's own float32 error


def case_id(c):
    return "x".join(str(v) for v in c)


def _cdtype(dtype):
    return torch.complex128 if dtype == torch.float64 else torch.complex64


def wavenumbers(M, N, dtype=torch.float64):
    k1 = (torch.fft.fftfreq(M, dtype=torch.float64) * M).round().view(M, 1)
    k2 = torch.arange(N // 2 + 1, dtype=torch.float64).view(1, -1)
    return k1.to(dtype), k2.to(dtype)


def forcing(M, N, dtype=torch.float64):
    """0.1 (sin 2 pi (x + y) + cos 2 pi (x + y)) on the grid x = i / M, y = j / N"""
    x = (torch.arange(M, dtype=torch.float64) / M).view(M, 1)
    y = (torch.arange(N, dtype=torch.float64) / N).view(1, N)
    return (0.1 * (torch.sin(2 * math.pi * (x + y)) + torch.cos(2 * math.pi * (x + y)))).to(dtype)


def schedule(T, dt, record_steps):
    """(steps, record_time, times of the first record_steps snapshots)"""
    steps = math.ceil(T / dt)
    record_time = math.floor(steps / record_steps)
    times, t = [], 0.0
    for j in range(steps):
        t += dt
        if (j + 1) % record_time == 0 and len(times) < record_steps:
            times.append(t)
    return steps, record_time, times


def solve(w0, f, visc, T, dt, record_steps, dtype=torch.float64, advection=True):
    """-> sol [B, M, N, record_steps], sol_t [record_steps], both of `dtype`"""
    w0 = w0.to(dtype)
    f = f.to(dtype)
    B, M, N = w0.shape
    k1, k2 = wavenumbers(M, N, dtype)
    lap = 4 * math.pi ** 2 * (k1 ** 2 + k2 ** 2)
    poisson = lap.clone()
    poisson[0, 0] = 1.0
    dealias = ((k1.abs() <= (2.0 / 3.0) * (M // 2)) & (k2.abs() <= (2.0 / 3.0) * (N // 2))).to(dtype)
    a = 0.5 * dt * visc * lap
    W = torch.fft.rfft2(w0)
    f_h = torch.fft.rfft2(f)
    if f_h.dim() == 2:
        f_h = f_h.unsqueeze(0)
    steps, record_time, times = schedule(T, dt, record_steps)
    two_pi_i = torch.tensor(2j * math.pi, dtype=_cdtype(dtype))
    inv = lambda z: torch.fft.irfft2(z, s=(M, N))
    sol = torch.zeros(B, M, N, record_steps, dtype=dtype)
    c = 0
    for j in range(steps):
        if advection:
            psi = W / poisson
            q = inv(two_pi_i * k2 * psi)
            v = inv(-two_pi_i * k1 * psi)
            w_x = inv(two_pi_i * k1 * W)
            w_y = inv(two_pi_i * k2 * W)
            F = dealias * torch.fft.rfft2(q * w_x + v * w_y)
        else:
            F = torch.zeros_like(W)
        W = (-dt * F + dt * f_h + (1.0 - a) * W) / (1.0 + a)
        if (j + 1) % record_time == 0 and c < record_steps:
            sol[..., c] = inv(W)
            c += 1
    return sol, torch.tensor(times, dtype=dtype)


def sqrt_eig(M, N, alpha, tau, sigma=None, dtype=torch.float64):
    """M N sqrt(2) sigma (4 pi^2 |k|^2 + tau^2)^(-alpha/2), 0 at the mean mode; sigma = tau^(alpha - 1) by default"""
    if sigma is None:
        sigma = tau ** (0.5 * (2 * alpha - 2))
    k1 = (torch.fft.fftfreq(M, dtype=torch.float64) * M).round().view(M, 1)
    k2 = (torch.fft.fftfreq(N, dtype=torch.float64) * N).round().view(1, N)
    e = M * N * math.sqrt(2.0) * sigma * (4 * math.pi ** 2 * (k1 ** 2 + k2 ** 2) + tau ** 2) ** (-alpha / 2.0)
    e[0, 0] = 0.0
    return e.to(dtype)


def grf(noise, se, dtype=torch.float64):
    """noise [B, M, N, 2], se [M, N] -> Re ifft2(se . (noise_re + i noise_im)) [B, M, N]"""
    noise, se = noise.to(dtype), se.to(dtype)
    coeff = torch.complex(se * noise[..., 0], se * noise[..., 1])
    return torch.fft.ifft2(coeff).real


def noise64(B, M, N, seed):
    return torch.randn(B, M, N, 2, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def initial_vorticity(B, M, N, seed):
    """8 x GRF(alpha = 2.5, tau = 7) from seeded float64 noise, float64 [B, M, N]"""
    return W0_SCALE * grf(noise64(B, M, N, seed), sqrt_eig(M, N, W0_ALPHA, W0_TAU))


def rel(x, y):
    """relative L2 error of x against y, in float64"""
    x, y = x.detach().double().cpu(), y.detach().double().cpu()
    return float((x - y).norm() / y.norm())


_PARITY: dict = {}


def parity_reference(case):
    """{w0, f, sol64, t64, floor32 [record_steps], advection_share}: computed once per case and shared; read-only"""
    hit = _PARITY.get(case)
    if hit is not None:
        return hit
    B, M, N = case
    w0 = initial_vorticity(B, M, N, seed=11 + M + N)
    f = forcing(M, N)
    sol64, t64 = solve(w0, f, VISC, T_FINAL, DT, RECORD_STEPS)
    # the floor sees what the device sees: float32 inputs
    sol32, _ = solve(w0.float(), f.float(), VISC, T_FINAL, DT, RECORD_STEPS, dtype=torch.float32)
    lin, _ = solve(w0, f, VISC, T_FINAL, DT, RECORD_STEPS, advection=False)
    out = dict(w0=w0, f=f, sol64=sol64, t64=t64,
               floor32=[rel(sol32[..., c], sol64[..., c]) for c in range(RECORD_STEPS)],
               advection_share=rel(lin[..., -1], sol64[..., -1]),
               moved=rel(sol64[..., -1], w0))
    _PARITY[case] = out
    return out
