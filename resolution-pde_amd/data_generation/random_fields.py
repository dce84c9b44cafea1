"""Gaussian random fields on the periodic unit square, sampled on the GPU (reference: data_generation/random_fields.py,
whose sampler needs the removed torch.ifft).  Same constructor as the reference; only dim = 2 with periodic boundary is
built here.

    sqrt_eig[k] = size^2 sqrt(2) sigma (4 pi^2 |k|^2 + tau^2)^(-alpha/2),  0 at the mean mode,  sigma = tau^(alpha - 1)
    sample      = Re ifft2(sqrt_eig . (xi_re + i xi_im)),  xi standard normal,  torch's 1/size^2 in the inverse

The noise comes from torch.randn on the device; the transform is rpde.ops.grf2d (csrc/halfspec.hip).

The periodic 1-D field -- the reference's dim = 1 formula -- is a class of its own, GaussianRF1d, on rpde.ops.grf1d
(the same kernel at one row); GaussianRF itself still refuses dim = 1:

    sqrt_eig[k] = size sqrt(2) sigma (4 pi^2 k^2 + tau^2)^(-alpha/2),  0 at k = 0,  sigma = tau^((2 alpha - 1) / 2)
    sample      = Re ifft(sqrt_eig . (xi_re + i xi_im))

GaussianRFNeumann is the 2-D field with zero-flux boundary on cell centres, a cosine series through rpde.ops.sep2d
(csrc/darcy.hip); the reference's GaussianRF has no such boundary, and GaussianRF here still refuses anything but
'periodic'."""
from __future__ import annotations

import math
from typing import Optional

import torch


def sqrt_eig_2d(M: int, N: int, alpha: float, tau: float, sigma: float) -> torch.Tensor:
    """float32 [M, N] host tensor, formed in float64 and rounded once; signed wavenumbers in fft order on both axes
    (Nyquist -n/2); the factor M N is size^2 on the reference's square grid.  M = 1 is the 1-D field: k1 = 0 adds an
    exact zero and the factor is N"""
    k1 = (torch.fft.fftfreq(M, dtype=torch.float64) * M).round().view(M, 1)
    k2 = (torch.fft.fftfreq(N, dtype=torch.float64) * N).round().view(1, N)
    e = M * N * math.sqrt(2.0) * float(sigma) * (4.0 * math.pi ** 2 * (k1 ** 2 + k2 ** 2) + float(tau) ** 2) ** (-float(alpha) / 2.0)
    e[0, 0] = 0.0
    return e.to(torch.float32)


def sqrt_eig_1d(N: int, alpha: float, tau: float, sigma: float) -> torch.Tensor:
    """float32 [N] host tensor: signed integer wavenumbers in fft order (Nyquist -N/2), 0 at k = 0"""
    return sqrt_eig_2d(1, N, alpha, tau, sigma)[0]


class _DeviceRF(object):
    """what both fields share: the eigenvalue table of a grid (size,) or (size, size), and sampling on the device"""

    def _setup(self, grid, alpha, tau, sigma, device):
        self.dim = len(grid)
        self.device = torch.device("cuda" if device is None else device)
        if sigma is None:
            sigma = tau ** (0.5 * (2 * alpha - self.dim))
        self.alpha, self.tau, self.sigma = alpha, tau, sigma
        self._grid = grid
        self._sqrt_eig_host = sqrt_eig_2d(*((1,) * (2 - self.dim) + grid), alpha, tau, sigma).reshape(grid)
        self._sqrt_eig = None

    @property
    def sqrt_eig(self) -> torch.Tensor:
        """[*grid] fp32 on the device (moved there at first use)"""
        if self._sqrt_eig is None:
            self._sqrt_eig = self._sqrt_eig_host.to(self.device)
        return self._sqrt_eig

    def sample(self, N, generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[N, *grid] samples.  The noise [N, *grid, 2] is drawn with torch.randn on the device (from `generator`, a
        device generator, when given: equal seeds give equal samples) or passed in."""
        from rpde import ops
        shape = (int(N), *self._grid, 2)
        if noise is None:
            noise = torch.randn(shape, device=self.device, dtype=torch.float32, generator=generator)
        elif tuple(noise.shape) != shape:
            raise ValueError(f"{type(self).__name__}.sample: noise {tuple(noise.shape)}, expected {shape}")
        return (ops.grf1d if self.dim == 1 else ops.grf2d)(noise.to(self.device), self.sqrt_eig)


class GaussianRF(_DeviceRF):

    def __init__(self, dim, size, alpha=2, tau=3, sigma=None, boundary="periodic", device=None):
        if dim != 2:
            raise ValueError(f"GaussianRF: only dim=2 is built on the device (got dim={dim}); the 1-D and 3-D fields of "
                             "the reference are not ported")
        if boundary != "periodic":
            raise ValueError(f"GaussianRF: only boundary='periodic' is supported (got {boundary!r})")
        self.size = (int(size), int(size))
        self._setup(self.size, alpha, tau, sigma, device)


class GaussianRF1d(_DeviceRF):
    """the reference's GaussianRF(dim=1, size, ...) with periodic boundary, sampled on the device"""

    def __init__(self, size, alpha=2, tau=3, sigma=None, device=None):
        size = int(size)
        if size < 4 or size > 4096 or size % 2:
            raise ValueError(f"GaussianRF1d: size must be even, 4 .. 4096 (got {size})")
        if not tau > 0:
            raise ValueError(f"GaussianRF1d: tau must be positive (got {tau})")
        self.size = size
        self._setup((size,), alpha, tau, sigma, device)


def neumann_tables(size: int, alpha: float, tau: float, sigma: float):
    """(C, coef) float32 [size, size] host tensors, formed in float64 and rounded once: the cosine table
    C[i, k] = cos(pi k (i + 1/2) / size) on the cell centres and coef[k1, k2] = sigma (pi^2 (k1^2 + k2^2) + tau^2)^(-alpha/2),
    0 at the mean mode"""
    i = (torch.arange(size, dtype=torch.float64) + 0.5).view(size, 1)
    k = torch.arange(size, dtype=torch.float64).view(1, size)
    C = torch.cos(math.pi * k * i / size)
    coef = float(sigma) * (math.pi ** 2 * (k.view(size, 1) ** 2 + k ** 2) + float(tau) ** 2) ** (-float(alpha) / 2.0)
    coef[0, 0] = 0.0
    return C.to(torch.float32), coef.to(torch.float32)


class GaussianRFNeumann(object):
    """N(0, sigma^2 (-Laplacian + tau^2)^-alpha) on the unit square with zero-flux boundary, on the cell centres
    (i + 1/2) / size: the cosine series

        sample = C (coef . xi) C^T,  C[i, k] = cos(pi k (i + 1/2) / size),  xi standard normal [size, size],
        coef[k1, k2] = sigma (pi^2 (k1^2 + k2^2) + tau^2)^(-alpha/2),  coef[0, 0] = 0,  sigma = tau^(alpha - 1) by default

    (the coefficient fields of the Darcy benchmark are thresholds of it, data_generation/darcy_2d.py).  The two
    products are rpde.ops.sep2d (csrc/darcy.hip); sizes are the Darcy generator's, multiples of 4 in 8 .. 512."""

    def __init__(self, size, alpha=2, tau=3, sigma=None, device=None):
        size = int(size)
        if size < 8 or size > 512 or size % 4:
            raise ValueError(f"GaussianRFNeumann: size must be a multiple of 4, 8 .. 512 (got {size})")
        if not tau > 0:
            raise ValueError(f"GaussianRFNeumann: tau must be positive (got {tau})")
        self.dim, self.size = 2, (size, size)
        self.device = torch.device("cuda" if device is None else device)
        if sigma is None:
            sigma = tau ** (0.5 * (2 * alpha - self.dim))
        self.alpha, self.tau, self.sigma = alpha, tau, sigma
        self._host = neumann_tables(size, alpha, tau, sigma)
        self._dev = None

    @property
    def tables(self):
        """(C, coef) fp32 [size, size] on the device (moved there at first use)"""
        if self._dev is None:
            self._dev = tuple(t.to(self.device) for t in self._host)
        return self._dev

    def sample(self, N, generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[N, size, size] samples.  The noise [N, size, size] is drawn with torch.randn on the device (from `generator`,
        a device generator, when given: equal seeds give equal samples) or passed in."""
        from rpde import ops
        shape = (int(N), *self.size)
        if noise is None:
            noise = torch.randn(shape, device=self.device, dtype=torch.float32, generator=generator)
        elif tuple(noise.shape) != shape:
            raise ValueError(f"GaussianRFNeumann.sample: noise {tuple(noise.shape)}, expected {shape}")
        C, coef = self.tables
        return ops.sep2d(noise.to(self.device).to(torch.float32) * coef, C, C)
