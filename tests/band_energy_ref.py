"""float64 restatement of the per-sample band energies, their gradient and the two losses built on them (test
infrastructure only; the product tree does not import it), the parity cases and their inputs.

    Z = rfft(z) (dims=1) or rfft2(z) (dims=2), unnormalised;  c_kx = 1 at kx = 0 and (even N) kx = N/2, else 2
    E[b, j] = sum_c sum_{(ky,kx): band = j} c_kx / (M N) |Z[b,c,ky,kx]|^2          band -1: no band
    d sum(gE E) / d z[b, c] = 2 irfft2(gE[b, band] Z[b, c]),  weight 0 where band = -1
    band loss      rel[b] = (1/J_e) sum_j sqrt(E_j(x - y)) / (sqrt(E_j(y)) + floor sqrt(E_tot(y)) + 1e-8)
    spectrum loss  val[b] = (1/J_e) sum_j (log(E_j(x) + d_b) - log(E_j(y) + d_b))^2,  d_b = floor E_tot(y) + 1e-30
    J_e: the bands that own at least one entry

Everything in float64 by default (``dtype=torch.float32`` gives the float32 floor of the same restatement).  The keyword
arguments edge_weight=2 and unsigned_ky=True switch on deliberately WRONG variants: the tests use them to show that the
comparison can see a wrong answer."""
from __future__ import annotations

import functools

import torch

LOSS_TOL, GRAD_TOL = 1e-5, 2e-5          # the project's parity budgets (tests/test_gpu_spectral_loss.py): forward, gradient
FLOOR_FACTOR = 4.0                       # one GEMM-form transform against one FFT
SEED = 11

# (B, C, M, N, table): M = 1 is one-dimensional; table = (kind, num_bands or None), "one" = an explicit table with one band
CASES = [
    (3, 1, 1, 16, ("octave", None)),
    (2, 2, 1, 48, ("octave", None)),
    (2, 1, 1, 64, ("modes", 16)),
    (1, 1, 1, 200, ("octave", None)),
    (2, 1, 1, 256, ("octave", None)),
    (2, 1, 8, 8, ("octave", None)),
    (2, 2, 16, 12, ("radial", 6)),
    (1, 1, 32, 64, ("radial", 16)),
    (1, 2, 64, 32, ("radial", 64)),
    (2, 1, 16, 12, ("one", None)),
]


def case_id(c):
    B, C, M, N, (kind, nb) = c
    return f"{B}x{C}x" + (f"{N}" if M == 1 else f"{M}x{N}") + f"-{kind}" + (f"{nb}" if nb else "")


def dims_of(case):
    return 1 if case[2] == 1 else 2


def rel_l2(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm())


def bound(budget, floor32):
    """max(project budget, 4 x float32 floor of the restatement); the floor itself must stay within the budget"""
    assert floor32 <= budget, f"float32 floor {floor32:.2e} of the restatement exceeds the budget {budget:.0e}: change the input"
    return max(budget, FLOOR_FACTOR * floor32)


def signed(n):
    return [k if k <= (n - 1) // 2 else k - n for k in range(n)]


def octave_table(M, N, unsigned_ky=False):
    """explicit loops and int.bit_length; unsigned_ky=True is wrong on purpose (ky = 0 .. M-1)"""
    K = N // 2 + 1
    t = torch.zeros(M, K, dtype=torch.int64)
    k1s = list(range(M)) if unsigned_ky else signed(M)
    for r in range(M):
        for k in range(K):
            q = k1s[r] ** 2 + k ** 2
            t[r, k] = 0 if q == 0 else 1 + (q.bit_length() - 1) // 2
    return t, int(t.max()) + 1


@functools.lru_cache(maxsize=None)
def table_of(M, N, kind, nb, unsigned_ky=False):
    """(int64 table [M, N//2+1], J)"""
    K = N // 2 + 1
    if kind == "octave":
        return octave_table(M, N, unsigned_ky)
    if kind == "modes":
        k = torch.arange(K).view(1, K)
        return torch.where(k < nb, k, torch.full_like(k, -1)), nb
    if kind == "one":
        return torch.zeros(M, K, dtype=torch.int64), 1
    if kind == "radial":                     # the evaluator's bins ARE the definition: rpde.ops.radial_bins, a host function
        from rpde.ops import radial_bins
        return radial_bins(M, N, nb)[0].to(torch.int64), nb
    raise ValueError(kind)


def owned_bands(table, J):
    return int((torch.bincount(table[table >= 0].reshape(-1), minlength=J) > 0).sum())


def _field(shape, amplitude, gen):
    """a real field with the given amplitude spectrum (None: white), unit variance per image, float64"""
    z = torch.randn(shape, generator=gen, dtype=torch.float64)
    if amplitude is not None:
        z = torch.fft.ifft2(torch.fft.fft2(z) * amplitude).real
    return z / z.flatten(2).std(dim=2).view(*shape[:2], 1, 1)


@functools.lru_cache(maxsize=None)
def make_inputs(B, C, M, N, seed=SEED):
    """(x, y) fp32 [B, C, N] / [B, C, M, N]: y a unit-variance field with amplitude spectrum (1 + |k|^2)^(-1/2) plus 0.3,
    x = y + 0.3 x a unit-variance white field; built in float64, rounded once"""
    gen = torch.Generator().manual_seed(seed)
    k1 = torch.tensor(signed(M), dtype=torch.float64).view(M, 1)
    k2 = torch.tensor(signed(N), dtype=torch.float64).view(1, N)
    y = _field((B, C, M, N), (1.0 + k1 ** 2 + k2 ** 2) ** -0.5, gen) + 0.3
    x = y + 0.3 * _field((B, C, M, N), None, gen)
    shape = (B, C, N) if M == 1 else (B, C, M, N)
    return x.reshape(shape).float(), y.reshape(shape).float()


def multiplicity(N, edge_weight=1.0, dtype=torch.float64):
    c = torch.full((N // 2 + 1,), 2.0, dtype=dtype)
    c[0] = edge_weight
    if N % 2 == 0:
        c[N // 2] = edge_weight
    return c


def _as4(z):
    return z.unsqueeze(2) if z.dim() == 3 else z


def band_energies(z, table, J, edge_weight=1.0):
    """E [B, J] of z's dtype, differentiable in z; z [B, C, N] or [B, C, M, N]; edge_weight=2 is wrong on purpose"""
    z4 = _as4(z)
    M, N = z4.shape[-2:]
    Z = torch.fft.rfft2(z4, dim=(-2, -1))
    p = ((Z.real ** 2 + Z.imag ** 2) * multiplicity(N, edge_weight, z.dtype)).sum(1) / (M * N)        # [B, M, K]
    own = table >= 0
    E = torch.zeros(z.shape[0], J, dtype=z.dtype)
    return E.index_add(1, table[own], p[:, own])


def closed_form_grad(z, table, J, gE):
    """2 irfft2(gE[b, band] Z[b, c]) in float64"""
    z4 = _as4(z.double())
    Z = torch.fft.rfft2(z4, dim=(-2, -1))
    w = torch.zeros(z.shape[0], *table.shape, dtype=torch.float64)
    own = table >= 0
    w[:, own] = gE.double()[:, table[own]]
    return (2.0 * torch.fft.irfft2(Z * w.unsqueeze(1), s=z4.shape[-2:], dim=(-2, -1))).reshape(z.shape)


def band_rel(x, y, table, J, band_floor=1e-3, **wrong):
    """per-sample vector [B] of the band loss, of x's dtype"""
    e_d, e_y = band_energies(x - y, table, J, **wrong), band_energies(y, table, J, **wrong)
    pos = e_d > 0
    root = torch.where(pos, torch.sqrt(torch.where(pos, e_d, torch.ones_like(e_d))), torch.zeros_like(e_d))
    denom = torch.sqrt(e_y) + band_floor * torch.sqrt(e_y.sum(1, keepdim=True)) + 1e-8
    return (root / denom).sum(1) / owned_bands(table, J)


def spectrum_val(x, y, table, J, spectrum_floor=1e-6, **wrong):
    e_x, e_y = band_energies(x, table, J, **wrong), band_energies(y, table, J, **wrong)
    d = spectrum_floor * e_y.sum(1, keepdim=True) + 1e-30
    return ((torch.log(e_x + d) - torch.log(e_y + d)) ** 2).sum(1) / owned_bands(table, J)


def relative_l2(x, y):
    x, y = x.double(), y.double()
    return (x - y).flatten(1).norm(dim=1) / (y.flatten(1).norm(dim=1) + 1e-8)


def value_and_grad(fn, x, dtype=torch.float64):
    """fn(x as dtype, requiring grad) -> vector; returns (vector, gradient of its mean with respect to x)"""
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    v = fn(xx)
    g, = torch.autograd.grad(v.mean(), xx)
    return v.detach(), g


def upstream(B, J, seed=5):
    """a seeded positive gE [B, J] in (0.5, 1.5), fp32"""
    return (torch.rand(B, J, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) + 0.5).float()


QUANTITIES = ("E", "gE_grad", "E_diff", "E_diff_grad", "band", "band_grad", "spectrum", "spectrum_grad")


def budget(name):
    return GRAD_TOL if name.endswith("grad") else LOSS_TOL


def reference(case, dtype=torch.float64, **wrong):
    """every compared quantity of one case in one dtype: dict of
    E [B, J], gE_grad (gradient of sum(gE E)), E_diff / E_diff_grad (the same of the field x - y), band / band_grad,
    spectrum / spectrum_grad (value vectors and gradients of their means)"""
    B, C, M, N, (kind, nb) = case
    unsigned = bool(wrong.pop("unsigned_ky", False))
    table, J = table_of(M, N, kind, nb, unsigned)
    x, y = make_inputs(B, C, M, N)
    xd, yd = x.to(dtype), y.to(dtype)
    out = {}
    xx = xd.clone().requires_grad_(True)
    E = band_energies(xx, table, J, **wrong)
    out["E"] = E.detach()
    out["gE_grad"], = torch.autograd.grad((E * upstream(B, J).to(dtype)).sum(), xx)
    xx = xd.clone().requires_grad_(True)
    E = band_energies(xx - yd, table, J, **wrong)
    out["E_diff"] = E.detach()
    out["E_diff_grad"], = torch.autograd.grad((E * upstream(B, J).to(dtype)).sum(), xx)
    out["band"], out["band_grad"] = value_and_grad(lambda t: band_rel(t, yd, table, J, **wrong), x, dtype)
    out["spectrum"], out["spectrum_grad"] = value_and_grad(lambda t: spectrum_val(t, yd, table, J, **wrong), x, dtype)
    return out


def strong_band_error(E, E64):
    """largest relative error over the bands with E_j >= 1e-3 E_tot"""
    E, E64 = E.double(), E64.double()
    strong = E64 >= 1e-3 * E64.sum(1, keepdim=True)
    return float(((E - E64).abs() / E64.clamp_min(1e-300))[strong].max())
