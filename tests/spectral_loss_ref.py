"""float64 restatement of the mode-weighted relative L2 loss and its gradient (test infrastructure only; the product
tree does not import it), and the parity cases.

    Z = rfft(z) (dims=1) or rfft2(z) (dims=2), unnormalised;  N = n or H W
    c_kx = 1 at kx = 0 and (even W) kx = W/2, else 2          (Hermitian multiplicity along the half axis)
    E(z)[b] = sum_c sum_k omega_k c_kx / N |Z[b,c,k]|^2
    rel[b]  = sqrt(E(x - y)[b]) / (sqrt(E(y)[b]) + 1e-8)
    d rel[b] / d x = coef_b irfft(omega . rfft(x - y)),  coef_b = g_b / (sqrt(E_d[b]) (sqrt(E_y[b]) + 1e-8)),  0 where E_d = 0

    sobolev: omega = (1 + sum_axes (2 pi k_axis / L_axis)^2)^s, ky signed (fft order), kx = 0 .. W//2

Everything in float64 by default (``dtype=torch.float32`` gives the float32 floor of the same restatement).  The keyword
arguments switch on deliberately WRONG variants: the tests use them to show that the comparison can see a wrong answer."""
from __future__ import annotations

import math

import numpy as np
import torch

from tests.freq_error_ref import make_inputs, rel as rel_l2   # noqa: F401  (inputs and the error measure of 10.1)

SEED = 3          # the seed of tests.freq_error_ref.CASES
# (dims, shape, s): every case runs with s_err = 1e-2
CASES = [
    (1, (4, 1, 64), 1.0), (1, (4, 1, 64), 2.0),
    (1, (3, 2, 63), 1.0),
    (1, (3, 3, 96), 0.5), (1, (3, 3, 96), 1.0),
    (1, (2, 1, 1024), 1.0),
    (2, (3, 1, 32, 32), 1.0),
    (2, (2, 2, 24, 40), 1.0),
    (2, (3, 1, 31, 33), 1.0),
    (2, (2, 1, 64, 64), 2.0),
    (2, (2, 1, 256, 256), 1.0),
]
# the good-model cases (s_err = 1e-4): the ones that need the difference formed first
GOOD = [(1, (4, 1, 64), 1.0), (1, (4, 1, 64), 2.0), (2, (2, 1, 64, 64), 2.0)]
PARITY = [(d, sh, s, 1e-2) for d, sh, s in CASES] + [(d, sh, s, 1e-4) for d, sh, s in GOOD]
LOSS_TOL, GRAD_TOL = 1e-5, 2e-5          # the project's parity budgets (README): forward, gradient


def case_id(c):
    return f"{c[0]}d-" + "x".join(str(v) for v in c[1]) + f"-s{c[2]:g}" + (f"-err{c[3]:g}" if len(c) > 3 else "")


def sobolev(spatial_shape, s=1.0, length=1.0, unsigned_ky=False):
    """numpy float64, written with explicit loops over the modes; unsigned_ky=True is wrong on purpose (ky = 0 .. H-1)"""
    shape = tuple(spatial_shape)
    L = [float(length)] * len(shape) if np.isscalar(length) else [float(v) for v in length]
    nk = shape[-1] // 2 + 1
    if len(shape) == 1:
        return np.array([(1.0 + (2 * math.pi * k / L[0]) ** 2) ** s for k in range(nk)])
    H = shape[0]
    out = np.empty((H, nk))
    for r in range(H):
        ky = r if (unsigned_ky or r <= H // 2) else r - H          # even H: the Nyquist row H/2 counts with |k| = H/2
        for k in range(nk):
            out[r, k] = (1.0 + (2 * math.pi * ky / L[0]) ** 2 + (2 * math.pi * k / L[1]) ** 2) ** s
    return out


def multiplicity(W, edge_weight=1.0):
    c = torch.full((W // 2 + 1,), 2.0, dtype=torch.float64)
    c[0] = edge_weight
    if W % 2 == 0:
        c[W // 2] = edge_weight
    return c


def _rfft(z, dims):
    return torch.fft.rfft(z, dim=-1) if dims == 1 else torch.fft.rfft2(z, dim=(-2, -1))


def energy(z, omega, dims, edge_weight=1.0):
    """E(z) [B]; z [B, C, *grid], omega [*half spectrum] of z's dtype"""
    N = z.shape[-1] if dims == 1 else z.shape[-2] * z.shape[-1]
    w = omega * multiplicity(z.shape[-1], edge_weight).to(omega.dtype)
    Z = _rfft(z, dims)
    return ((Z.real ** 2 + Z.imag ** 2) * w).flatten(1).sum(1) / N


def rel(x, y, omega, dims, edge_weight=1.0, dtype=torch.float64):
    """per-sample vector [B] (differentiable in x); edge_weight=2 is wrong on purpose"""
    x, y = x.to(dtype), y.to(dtype)
    omega = torch.as_tensor(omega).to(dtype)
    return torch.sqrt(energy(x - y, omega, dims, edge_weight)) / (torch.sqrt(energy(y, omega, dims, edge_weight)) + 1e-8)


def reduce(r, size_average=True, reduction=True):
    if not reduction:
        return r
    return r.mean() if size_average else r.sum()


def loss_and_grad(x, y, omega, dims, size_average=True, reduction=True, upstream=None, dtype=torch.float64, **wrong):
    """-> (per-sample vector, gradient with respect to x of the reduced loss [or of sum(upstream * rel)]) by autograd"""
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    r = rel(xx, y, omega, dims, dtype=dtype, **wrong)
    out = reduce(r, size_average, reduction)
    if out.dim():
        out = (out * (torch.ones_like(out) if upstream is None else upstream.to(dtype))).sum()
    g, = torch.autograd.grad(out, xx)
    return r.detach(), g


def closed_form_grad(x, y, omega, dims, g_b):
    """coef_b irfft(omega . rfft(x - y)) in float64, g_b [B] the upstream gradient of rel[b]"""
    x, y = x.double(), y.double()
    omega = torch.as_tensor(omega).double()
    d = x - y
    ed, ey = energy(d, omega, dims), energy(y, omega, dims)
    coef = torch.where(ed > 0, g_b.double() / (torch.sqrt(ed) * (torch.sqrt(ey) + 1e-8)), torch.zeros_like(ed))
    WD = _rfft(d, dims) * omega
    back = torch.fft.irfft(WD, n=d.shape[-1], dim=-1) if dims == 1 else torch.fft.irfft2(WD, s=d.shape[-2:], dim=(-2, -1))
    return coef.view(-1, *([1] * (d.dim() - 1))) * back


def relative_l2(x, y):
    """the plain loss, float64, per sample"""
    x, y = x.double(), y.double()
    return (x - y).flatten(1).norm(dim=1) / (y.flatten(1).norm(dim=1) + 1e-8)


def symmetric_random_table(spatial_shape, seed):
    """a random table in [0.5, 1.5) that satisfies the symmetry the self-conjugate columns need; float64 torch"""
    g = torch.Generator().manual_seed(seed)
    shape = tuple(spatial_shape)
    if len(shape) == 1:
        return torch.rand(shape[0] // 2 + 1, generator=g, dtype=torch.float64) + 0.5
    H, W = shape
    w = torch.rand(H, W // 2 + 1, generator=g, dtype=torch.float64) + 0.5
    flip = (H - torch.arange(H)) % H
    for kx in [0] + ([W // 2] if W % 2 == 0 else []):
        w[:, kx] = 0.5 * (w[:, kx] + w[flip, kx])
    return w


def wrong_variants(dims):
    """{label: (kwargs of sobolev, kwargs of rel)} that give a wrong answer"""
    v = {"multiplicity 2 on DC and Nyquist": ({}, dict(edge_weight=2.0))}
    if dims == 2:
        v["unsigned ky"] = (dict(unsigned_ky=True), {})
    return v
