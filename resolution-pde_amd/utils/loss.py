"""RelativeL2Loss (reference: utils/loss.py:17-59): per-sample
|x - y|_2 / (|y|_2 + 1e-8), then mean / sum / none -- one fused HIP pass over
prediction and target (wavefront-shuffle reductions, deterministic; csrc/rel_loss.hip, which also holds what the
relative losses below share).

SpectralRelativeL2Loss (no counterpart in the reference): the same ratio with a non-negative weight per Fourier
mode -- the H^s / Sobolev relative loss of operator learning is the preset -- forward and backward on the device
(rpde.ops.weighted_relative_l2, csrc/spectral_loss.hip).

BandRelativeL2Loss, SpectrumMatchingLoss (no counterpart in the reference): objectives whose weights depend on the
sample -- the relative error band by band, and the mismatch of the energy per wavenumber band -- as a few operations
on the [B, J] per-sample band energies of rpde.ops.band_energy (csrc/band_energy.hip, forward and backward on the
device).

EquationResidualLoss (no counterpart in the reference): the physics-informed term for the 1-D ETD family
u_t = L u - (c/2) (u^2)_x -- does the one-step map satisfy the equation itself? -- forward and backward on the device
(rpde.ops.etd1d_residual, csrc/etd_residual.hip).  It reads the network's input next to its prediction
(`takes_input`).  VorticityResidualLoss (no counterpart in the reference): the same term for the 2-D vorticity equation
of the Navier-Stokes generator (rpde.ops.ns2d_residual, csrc/ns_residual.hip).  DarcyResidualLoss (no counterpart in
the reference): the term for the steady Darcy generator, whose input is the operator's coefficient, in the dual norm of
the solver's preconditioner or in L2 (rpde.ops.darcy2d_residual, csrc/darcy_residual.hip).  ActiveScalarResidualLoss (no
counterpart in the reference): the term for the active-scalar generator, whose data (c, q, v) are not the evolved
variable (rpde.ops.nsc2d_residual, csrc/nsc_residual.hip).  SumLoss adds weighted losses into one callable."""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from rpde import ops


class RelativeL2Loss(nn.Module):
    def __init__(self, size_average=True, reduction=True):
        super().__init__()
        self.size_average = size_average
        self.reduction = reduction

    def forward(self, x, y):
        return ops.relative_l2(x, y, self.size_average, self.reduction)


def sobolev_weights(spatial_shape, s=1.0, length=1.0) -> torch.Tensor:
    """omega = (1 + sum_axes (2 pi k_axis / L_axis)^2)^s on the half spectrum of a grid: float64 [n//2+1] for (n,),
    [H, W//2+1] for (H, W) with ky signed in fft order (fftfreq(H) * H) and kx = 0 .. W//2; the Nyquist bin of an even
    axis counts with |k| = n/2.  s = 1 is H^1; length: one float, or one per axis."""
    shape = tuple(int(n) for n in spatial_shape)
    if len(shape) not in (1, 2) or min(shape) < 2:
        raise ValueError(f"sobolev_weights: spatial_shape {spatial_shape}, expected (n,) or (H, W) with every axis >= 2")
    L = [float(length)] * len(shape) if isinstance(length, (int, float)) else [float(v) for v in length]
    if len(L) != len(shape) or not all(math.isfinite(v) and v > 0 for v in L):
        raise ValueError(f"sobolev_weights: length {length} for a {len(shape)}-D grid")
    kx = torch.arange(shape[-1] // 2 + 1, dtype=torch.float64)
    q = (2.0 * math.pi * kx / L[-1]) ** 2
    if len(shape) == 2:
        ky = torch.fft.fftfreq(shape[0], dtype=torch.float64) * shape[0]
        q = (2.0 * math.pi * ky / L[0]).view(-1, 1) ** 2 + q.view(1, -1)
    return (1.0 + q) ** float(s)


def check_mode_weights(omega: torch.Tensor, spatial_shape) -> None:
    """ValueError unless omega is a finite, non-negative table of the half spectrum of this grid whose self-conjugate
    columns (kx = 0 and, for even W, kx = W/2) are symmetric in ky: otherwise omega * rfft2(d) is not the spectrum of
    a real field and the inverse transform is not the gradient"""
    shape = tuple(int(n) for n in spatial_shape)
    want = (shape[0] // 2 + 1,) if len(shape) == 1 else (shape[0], shape[1] // 2 + 1)
    if tuple(omega.shape) != want:
        raise ValueError(f"mode weights of shape {tuple(omega.shape)}: the grid {shape} needs {want}")
    w = omega.detach().double().cpu()
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
        raise ValueError("mode weights must be finite and >= 0")
    if len(shape) == 2:
        H, W = shape
        flip = (H - torch.arange(H)) % H
        for kx in [0] + ([W // 2] if W % 2 == 0 else []):
            if not torch.equal(w[:, kx], w[flip, kx]):
                raise ValueError(f"mode weights: column kx={kx} is not symmetric in ky (omega[ky] != omega[(H - ky) % H])")


class _GridTableLoss(nn.Module):
    """A loss with tables built on the host per grid: the cache of their device forms per (grid, device), the guard of
    an explicit table (it serves ONE grid), warm() for graph capture and the reduction of a per-sample vector.  A
    subclass supplies _build(grid, device) and forward; `dims` is the rank of its grids."""

    _explicit = None                  # the table given for one grid, if any, and the grid that took it
    _explicit_grid = None
    _explicit_kind = ""               # "weight" / "band", for the guard's message
    channels = 1                      # of the throw-away fields of warm()

    def __init__(self, size_average=True, reduction=True):
        super().__init__()
        self.size_average = size_average
        self.reduction = reduction
        self._tables: dict = {}

    def _table(self, grid, device):
        key = (grid, torch.device(device))
        t = self._tables.get(key)
        if t is None:
            if self._explicit is not None and self._explicit_grid not in (None, grid):
                raise ValueError(f"{type(self).__name__}: the explicit {self._explicit_kind} table serves the grid "
                                 f"{self._explicit_grid}, got {grid}")
            t = self._tables[key] = self._build(grid, device)
            if self._explicit is not None:
                self._explicit_grid = grid
        return t

    def _bad_rank(self, grid) -> str:
        return f"{type(self).__name__}.warm: grid {grid} for dims={self.dims}"

    def warm(self, spatial_shape, device="cuda") -> None:
        """plans, workspaces and the tables of one grid, outside any capture"""
        grid = tuple(int(n) for n in spatial_shape)
        if len(grid) != self.dims:
            raise ValueError(self._bad_rank(grid))
        z = torch.zeros((1, self.channels) + grid, dtype=torch.float32, device=device, requires_grad=True)
        ones = torch.ones_like(z.detach())
        call_loss(self, z, ones, ones).sum().backward()
        torch.cuda.synchronize(z.device)

    def _reduce(self, v):
        if not self.reduction:
            return v
        return v.mean() if self.size_average else v.sum()


class SpectralRelativeL2Loss(_GridTableLoss):
    """rel[b] = sqrt(E(x - y)[b]) / (sqrt(E(y)[b]) + 1e-8) with E(z)[b] = sum_c sum_k omega_k c_kx / N |rfft(z)[b,c,k]|^2
    (rfft2 for dims=2; c_kx the Hermitian multiplicity of the half axis), then mean / sum / per-sample vector as
    RelativeL2Loss.  omega == 1 is RelativeL2Loss by Parseval.  x, y: channels-first fp32 tensors on the GPU.

    weights="sobolev": sobolev_weights(grid, s, length), built per grid and cached per (grid, device), so one object
    serves mixed-resolution batches.  weights=Tensor: an explicit table for ONE grid ([n//2+1] or [H, W//2+1], rows
    in fft order), validated on the host at first use; another grid raises ValueError.

    The first call at a grid builds the transform plans and the device table (allocation, one synchronisation);
    warm(spatial_shape, device) does that ahead of a hipGraph capture."""

    _explicit_kind = "weight"

    def __init__(self, dims, weights="sobolev", s=1.0, length=1.0, size_average=True, reduction=True):
        super().__init__(size_average, reduction)
        if int(dims) not in (1, 2):
            raise ValueError(f"SpectralRelativeL2Loss: dims must be 1 or 2, got {dims}")
        self.dims = int(dims)
        if isinstance(weights, str):
            if weights != "sobolev":
                raise ValueError(f"SpectralRelativeL2Loss: unknown weights preset {weights!r} (presets: 'sobolev')")
            sobolev_weights((4,) * self.dims, s, length)          # validates s / length now
        elif torch.is_tensor(weights):
            if weights.dim() != self.dims:
                raise ValueError(f"SpectralRelativeL2Loss: a {weights.dim()}-D weight table for dims={self.dims}")
            self._explicit = weights.detach()
        else:
            raise ValueError("SpectralRelativeL2Loss: weights must be 'sobolev' or a tensor")
        self.s, self.length = float(s), length

    def _build(self, grid, device) -> torch.Tensor:
        if self._explicit is None:
            w = sobolev_weights(grid, self.s, self.length)
        else:
            w = self._explicit
            check_mode_weights(w, grid)
        return w.to(device=device, dtype=torch.float32).contiguous()

    def forward(self, x, y):
        if x.dim() != self.dims + 2:
            raise ValueError(f"SpectralRelativeL2Loss(dims={self.dims}): expected [B, C, *grid], got {tuple(x.shape)}")
        omega = self._table(tuple(x.shape[2:]), x.device)
        return ops.weighted_relative_l2(x, y, omega, self.dims, self.size_average, self.reduction)


def _safe_sqrt(e: torch.Tensor) -> torch.Tensor:
    """sqrt with the value 0 and the gradient 0 (not inf) at 0"""
    pos = e > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, e, torch.ones_like(e))), torch.zeros_like(e))


class _BandedLoss(_GridTableLoss):
    """What the two band losses share: the band table (a kind of rpde.ops.band_table built per grid, or one explicit
    integer table [n//2+1] / [H, W//2+1] with values -1 .. J-1 for ONE grid) and the check of the fields' shapes."""

    _explicit_kind = "band"

    def __init__(self, dims, bands="octave", num_bands=None, size_average=True, reduction=True):
        super().__init__(size_average, reduction)
        name = type(self).__name__
        if int(dims) not in (1, 2):
            raise ValueError(f"{name}: dims must be 1 or 2, got {dims}")
        self.dims = int(dims)
        if isinstance(bands, str):
            ops.band_table((8,) * self.dims, bands, num_bands)        # validates kind / num_bands / dims now
        elif torch.is_tensor(bands):
            if bands.dim() != self.dims or bands.is_floating_point():
                raise ValueError(f"{name}: an explicit band table is an integer tensor with {self.dims} dimension(s)")
            self._explicit = bands.detach().cpu()
            num_bands = int(num_bands) if num_bands is not None else max(int(self._explicit.max()), 0) + 1
        else:
            raise ValueError(f"{name}: bands must be one of {ops.BAND_KINDS} or an integer tensor")
        self.bands, self.num_bands = bands if isinstance(bands, str) else "explicit", num_bands

    def _build(self, grid, device) -> "ops.BandTables":
        if self._explicit is None:
            table, J = ops.band_table(grid, self.bands, self.num_bands)
        else:
            table, J = self._explicit.reshape(1 if self.dims == 1 else grid[0], -1), self.num_bands
        return ops.band_tables(table, J, grid, device)

    def _tables_for(self, x, y):
        if x.dim() != self.dims + 2 or x.shape != y.shape:
            raise ValueError(f"{type(self).__name__}(dims={self.dims}): expected equal [B, C, *grid] shapes, got "
                             f"{tuple(x.shape)} / {tuple(y.shape)}")
        return self._table(tuple(int(n) for n in x.shape[2:]), x.device)


class BandRelativeL2Loss(_BandedLoss):
    """Relative error band by band, so that a weak high-wavenumber band counts as much as the energetic low ones:

        rel[b] = (1/J_e) sum_j sqrt(E_j(x - y)[b]) / (sqrt(E_j(y)[b]) + band_floor sqrt(E_tot(y)[b]) + 1e-8)

    with E_j the per-sample band energies of rpde.ops.band_energy (x - y formed in fp32 before the transform), E_tot the
    sum over the bands and J_e the number of bands that own an entry on the grid; then mean / sum / per-sample vector as
    RelativeL2Loss.  One band that owns every entry and band_floor = 0 is RelativeL2Loss.  band_floor keeps a band the
    target leaves empty from dominating.  x, y: channels-first fp32 tensors on the GPU; gradient for x only."""

    def __init__(self, dims, bands="octave", num_bands=None, band_floor=1e-3, size_average=True, reduction=True):
        super().__init__(dims, bands, num_bands, size_average, reduction)
        if not (math.isfinite(float(band_floor)) and float(band_floor) >= 0):
            raise ValueError(f"BandRelativeL2Loss: band_floor {band_floor}")
        self.band_floor = float(band_floor)

    def forward(self, x, y):
        T = self._tables_for(x, y)
        y = y.detach()
        e_d = ops.band_energy(x, T, self.dims, y=y)
        e_y = ops.band_energy(y, T, self.dims)
        denom = torch.sqrt(e_y) + (self.band_floor * torch.sqrt(e_y.sum(1, keepdim=True)) + 1e-8)
        return self._reduce((_safe_sqrt(e_d) / denom).sum(1) / T.J_e)


class SpectrumMatchingLoss(_BandedLoss):
    """The prediction has the wrong amount of energy in band j (spectral blur), whatever the phases:

        val[b] = (1/J_e) sum_j (log(E_j(x)[b] + delta_b) - log(E_j(y)[b] + delta_b))^2,
        delta_b = spectrum_floor E_tot(y)[b] + 1e-30

    with the band energies of rpde.ops.band_energy; then mean / sum / per-sample vector.  It does not see a phase error:
    add it to a pointwise loss (SumLoss).  x, y: channels-first fp32 tensors on the GPU; gradient for x only."""

    def __init__(self, dims, bands="octave", num_bands=None, spectrum_floor=1e-6, size_average=True, reduction=True):
        super().__init__(dims, bands, num_bands, size_average, reduction)
        if not (math.isfinite(float(spectrum_floor)) and float(spectrum_floor) >= 0):
            raise ValueError(f"SpectrumMatchingLoss: spectrum_floor {spectrum_floor}")
        self.spectrum_floor = float(spectrum_floor)

    def forward(self, x, y):
        T = self._tables_for(x, y)
        e_x = ops.band_energy(x, T, self.dims)
        e_y = ops.band_energy(y.detach(), T, self.dims)
        delta = self.spectrum_floor * e_y.sum(1, keepdim=True) + 1e-30
        return self._reduce(((torch.log(e_x + delta) - torch.log(e_y + delta)) ** 2).sum(1) / T.J_e)


class _ResidualLoss(_GridTableLoss):
    """What the equation residuals share: forward(pred, target, inp) with the network's input (`takes_input`), the
    decode maps of set_affine and the refusals.  A subclass supplies `dims`, _build and forward, which raises
    _no_input() where inp is None."""

    takes_input = True
    _affine = None                    # (a_p, b_p, a_x, b_x), or None for the identity

    def set_affine(self, pred=(1.0, 0.0), inp=(1.0, 0.0)) -> None:
        """decode maps of the prediction and of the input, each (a, b) for a field + b; set before a capture"""
        aff = (float(pred[0]), float(pred[1]), float(inp[0]), float(inp[1]))
        if not all(math.isfinite(v) for v in aff):
            raise ValueError(f"{type(self).__name__}.set_affine: {pred} / {inp}")
        self._affine = None if aff == (1.0, 0.0, 1.0, 0.0) else aff

    def _bad_rank(self, grid) -> str:
        return f"{type(self).__name__}.warm: grid {grid}, the equation is {('one', 'two')[self.dims - 1]}-dimensional"

    def _no_input(self) -> ValueError:
        return ValueError(f"{type(self).__name__}: the network's input is needed next to its prediction")


class EquationResidualLoss(_ResidualLoss):
    """Does the prediction p ~ u(t + interval) follow from the input x = u(t) under

        u_t = L u - (advect/2) (u^2)_x,   l_n = c2 kappa_n^2 + c4 kappa_n^4 + i (c1 kappa_n + c3 kappa_n^3),  kappa_n = 2 pi n / length

    (the family and sign conventions of rpde.ops.etd1d_tables_cx and the generators)?  With the exponential trapezoidal
    rule -- exact in the linear part however stiff, the nonlinear term interpolated linearly between the two ends --

        r^ = rfft(p) - E rfft(x) - m0 rfft(x^2) - m1 rfft(p^2),   rel[b] = |r[b]|_2 / (|x[b]|_2 + 1e-8)

    then mean / sum / per-sample vector as RelativeL2Loss (rpde.ops.etd1d_residual_tables has E, m0, m1).  `interval` is
    the time between input and prediction: the snapshot interval of the data set, not the solver's step.  The rule is
    second order, so an exact pair leaves rel ~ interval^3 |N_tt|: the loss is for |interval N_tt| small.  Float64
    figures, exact pair against the trivial predictor p = x (DESIGN.md has the table): KS N = 64, length 16, nu 0.05:
    3.5e-4 .. 9.7e-4 against 0.15 .. 0.24 at interval 0.05, 4.8e-3 .. 1.2e-2 against 0.36 .. 0.56 at 0.1, and by
    interval ~ 0.4 the rule has lost its meaning (rel ~ 1 for both).

    forward(pred, target, inp): the target is unused and may be None; pred, inp [B, N] or [B, 1, N] fp32 tensors on the
    GPU, gradient for pred only.  set_affine(pred=(a, b), inp=(a, b)): the residual is formed on a pred + b and a inp + b
    (fields a SimpleNormalizer encoded, penalised in physical units); the gradient is still with respect to pred.
    Device tables are cached per (grid, device), so one object serves mixed-resolution batches; warm((N,), device) builds
    them, the plans and the workspaces ahead of a hipGraph capture."""

    dims = 1

    def __init__(self, length, interval, c1=0.0, c2=0.0, c3=0.0, c4=0.0, advect=1.0, dealias=True, size_average=True,
                 reduction=True):
        super().__init__(size_average, reduction)
        vals = [float(v) for v in (length, interval, c1, c2, c3, c4, advect)]
        if not all(math.isfinite(v) for v in vals) or not (vals[0] > 0 and vals[1] > 0):
            raise ValueError(f"EquationResidualLoss: length {length} and interval {interval} must be positive and every "
                             "coefficient finite")
        self.length, self.interval, self.c1, self.c2, self.c3, self.c4, self.advect = vals
        self.dealias = bool(dealias)

    @classmethod
    def burgers(cls, nu_eff, length, interval, **kw):
        """u_t + u u_x = nu_eff u_xx (data_generation/burgers_1d.py: nu_eff = nu / pi)"""
        return cls(length, interval, c2=-float(nu_eff), **kw)

    @classmethod
    def ks(cls, viscosity, length, interval, **kw):
        """u_t + u u_x + u_xx + viscosity u_xxxx = 0 (data_generation/ks_1d.py)"""
        return cls(length, interval, c2=1.0, c4=-float(viscosity), **kw)

    @classmethod
    def kdv(cls, dispersion, viscosity, length, interval, **kw):
        """u_t + u u_x + dispersion u_xxx = viscosity u_xx (data_generation/kdv_1d.py)"""
        return cls(length, interval, c2=-float(viscosity), c3=float(dispersion), **kw)

    def _build(self, grid, device):
        host = ops.etd1d_residual_tables(grid[0], self.length, self.c1, self.c2, self.c3, self.c4, self.interval,
                                         self.advect, self.dealias)
        return tuple(h.to(device).contiguous() for h in host)

    def forward(self, pred, target, inp):
        if inp is None:
            raise self._no_input()
        return ops.etd1d_residual(pred, inp, self._table((int(pred.shape[-1]),), pred.device), self._affine,
                                  self.size_average, self.reduction)


def reference_forcing(M: int, N: int) -> torch.Tensor:
    """0.1 (sin 2 pi (x + y) + cos 2 pi (x + y)) on the grid x = i / M, y = j / N: the forcing of
    data_generation/ns_2d.py, float64 [M, N]"""
    x = (torch.arange(int(M), dtype=torch.float64) / int(M)).view(-1, 1)
    y = (torch.arange(int(N), dtype=torch.float64) / int(N)).view(1, -1)
    return 0.1 * (torch.sin(2 * math.pi * (x + y)) + torch.cos(2 * math.pi * (x + y)))


class VorticityResidualLoss(_ResidualLoss):
    """Does the prediction p ~ w(t + interval) follow from the input x = w(t) under the 2-D vorticity equation of the
    generator (rpde.ops.ns2d_solve, data_generation/ns_2d.py) on the unit periodic square,

        w_t + u . grad w = viscosity lap w + f,   u = (psi_y, -psi_x),  lap psi = -w ?

    The advection is the generator's discrete one, A(w) = dealias rfft2(q w_x + v w_y), and the rule the exponential
    trapezoidal one of EquationResidualLoss with z = -interval viscosity lap:

        r^ = rfft2(p - x) - (E - 1) rfft2(x) - m0 (f^ - A(x)) - m1 (f^ - A(p)),   rel[b] = |r[b]|_2 / (|x[b]|_2 + 1e-8)

    then mean / sum / per-sample vector as RelativeL2Loss (rpde.ops.ns2d_residual_tables has E - 1, m0, m1).  `interval`
    is the time between input and prediction: the snapshot interval of the data set, not the solver's step.  The rule is
    second order, so an exact pair leaves rel ~ interval^3 |N_tt|.  Float64 figures at viscosity 1e-3, w0 = 8 x GRF(2.5, 7)
    and the reference forcing, exact pair against the trivial predictor p = x (DESIGN.md 10.12 has the table): at
    interval 0.05, 1.3e-3 .. 1.9e-3 against 0.06 .. 0.07 on 64 x 64; by interval 0.1 the exact pair reaches a tenth
    of p = x on 16 x 24.

    forcing: None, "reference" (the forcing of data_generation/ns_2d.py on each grid) or one [M, N] tensor for ONE grid.
    forward(pred, target, inp): the target is unused and may be None; pred, inp [B, M, N] or [B, 1, M, N] fp32 tensors
    on the GPU (more channels: ValueError), gradient for pred only.  set_affine, the per-(grid, device) table cache and
    warm((M, N), device) as in EquationResidualLoss."""

    dims = 2
    _explicit_kind = "forcing"

    def __init__(self, viscosity, interval, forcing=None, dealias=True, size_average=True, reduction=True):
        super().__init__(size_average, reduction)
        vals = [float(viscosity), float(interval)]
        if not all(math.isfinite(v) for v in vals) or vals[0] < 0 or not vals[1] > 0:
            raise ValueError(f"VorticityResidualLoss: viscosity {viscosity} must be >= 0 and interval {interval} positive")
        self.viscosity, self.interval = vals
        if torch.is_tensor(forcing):
            if forcing.dim() != 2:
                raise ValueError(f"VorticityResidualLoss: a forcing tensor is one [M, N] field, got {tuple(forcing.shape)}")
            self._explicit = forcing.detach().double().cpu()
            self.forcing = "explicit"
        elif forcing in (None, "reference"):
            self.forcing = forcing
        else:
            raise ValueError(f"VorticityResidualLoss: forcing must be None, 'reference' or an [M, N] tensor, got {forcing!r}")
        self.dealias = bool(dealias)

    def _build(self, grid, device):
        tabs = ops.ns2d_residual_tables(grid[0], grid[1], self.viscosity, self.interval, self.dealias)
        if self.forcing is None:
            f = None
        elif self._explicit is not None:
            if tuple(self._explicit.shape) != tuple(grid):
                raise ValueError(f"VorticityResidualLoss: the forcing of shape {tuple(self._explicit.shape)} does not serve "
                                 f"the grid {grid}")
            f = self._explicit
        else:
            f = reference_forcing(*grid)
        fs = None if f is None else ops.ns2d_residual_forcing(f, self.viscosity, self.interval).to(device).contiguous()
        return tuple(t.to(device).contiguous() for t in tabs), fs

    def forward(self, pred, target, inp):
        if inp is None:
            raise self._no_input()
        if pred.dim() not in (3, 4) or (pred.dim() == 4 and pred.shape[1] != 1):
            raise ValueError(f"VorticityResidualLoss: expected [B, M, N] or [B, 1, M, N] (the vorticity is one channel), got "
                             f"{tuple(pred.shape)}")
        tabs, fs = self._table((int(pred.shape[-2]), int(pred.shape[-1])), pred.device)
        return ops.ns2d_residual(pred, inp, tabs, fs, self._affine, self.size_average, self.reduction)


class DarcyResidualLoss(_ResidualLoss):
    """Does the prediction p ~ u solve the Darcy equation of the generator (rpde.ops.darcy2d_solve,
    data_generation/darcy_2d.py) for the coefficient a the network was given,

        -div(a grad u) = f on the unit square,  u = 0 on the boundary ?

    The equation is steady: the network's input is the operator's coefficient, not an earlier state.  With r = f - A(a) p,
    A the generator's finite-volume operator (harmonic face weights, wall faces 2 a_c, difference form),

        norm="dual" (default):  rel[b] = sqrt(r[b] . P^-1 r[b]) / (sqrt(f . P^-1 f) + 1e-8),  P = A(1)
        norm="l2":              rel[b] = |r[b]|_2 / (|f|_2 + 1e-8)

    then mean / sum / per-sample vector as RelativeL2Loss.  P is the solver's preconditioner, inverted exactly by two
    sine transforms.  Every face weight lies in [a_min, a_max], so a_min P <= A(a) <= a_max P and, with e = u* - p,
    a_min e.A e <= r.P^-1 r <= a_max e.A e: the dual norm is the energy-norm error of the prediction to within
    sqrt(a_max / a_min) at every grid size, without knowing u*.  The L2 form (the strong-form PINO term) multiplies
    cell-scale error by about 8 s^2 a and grows with the grid: float64, coefficients 12 / 3, f = 1, a prediction 1 %
    of white noise away from u*: 0.13 at s = 8 and 19 at s = 100 in L2, 0.041 and 0.46 in the dual norm; 5 % of a smooth
    perturbation: 0.043 and 0.41 against 0.026 and 0.033 (DESIGN.md 10.14 has the table).  p = 0 is rel = 1 in both.

    forcing: a constant (the generator's --forcing, default 1.0) or one [s, s] tensor for ONE grid; zero is refused.
    forward(pred, target, inp): the target is unused and may be None; pred, inp = a: [B, s, s] or [B, 1, s, s] fp32
    tensors on the GPU, s a multiple of 4 in 8 .. 512 (more channels: ValueError), gradient for pred only.  A decoded
    coefficient that is not positive makes the loss non-finite; it is not checked, and the optimizer's non-finite step
    skipping takes such a step.  set_affine matters here: an encoded coefficient is negative wherever a < mean, so the
    decode map is what makes the operator meaningful.  The samples must be the generator's cell centres: strided
    samples of a finer grid are not the cell centres of the coarse one.  set_affine, the per-(grid, device) table cache
    and warm((s, s), device) as in EquationResidualLoss."""

    dims = 2
    _explicit_kind = "forcing"

    def __init__(self, forcing=1.0, norm="dual", size_average=True, reduction=True):
        super().__init__(size_average, reduction)
        if norm not in ops.DARCY_NORMS:
            raise ValueError(f"DarcyResidualLoss: norm must be one of {ops.DARCY_NORMS}, got {norm!r}")
        self.norm = norm
        if torch.is_tensor(forcing):
            if forcing.dim() != 2 or forcing.shape[0] != forcing.shape[1]:
                raise ValueError(f"DarcyResidualLoss: a forcing tensor is one [s, s] field, got {tuple(forcing.shape)}")
            self._explicit = forcing.detach().double().cpu()
            if not bool(torch.isfinite(self._explicit).all()) or not bool(self._explicit.any()):
                raise ValueError("DarcyResidualLoss: the forcing must be finite and not zero")
            self.forcing = "explicit"
        else:
            try:
                self.forcing = float(forcing)
            except (TypeError, ValueError):
                raise ValueError(f"DarcyResidualLoss: forcing must be a number or an [s, s] tensor, got {forcing!r}")
            if not math.isfinite(self.forcing) or self.forcing == 0.0:
                raise ValueError(f"DarcyResidualLoss: the forcing must be finite and not zero, got {forcing}")

    def _build(self, grid, device):
        if grid[0] != grid[1]:
            raise ValueError(f"DarcyResidualLoss: the grid {grid} is not square")
        if self._explicit is not None and tuple(self._explicit.shape) != tuple(grid):
            raise ValueError(f"DarcyResidualLoss: the forcing of shape {tuple(self._explicit.shape)} does not serve the "
                             f"grid {grid}")
        f, S, il, D = ops.darcy2d_residual_tables(grid[0], self.forcing if self._explicit is None else self._explicit,
                                                  self.norm)
        return tuple(None if t is None else t.to(device).contiguous() for t in (f, S, il)) + (D,)

    def forward(self, pred, target, inp):
        if inp is None:
            raise self._no_input()
        if pred.dim() not in (3, 4) or (pred.dim() == 4 and pred.shape[1] != 1):
            raise ValueError(f"DarcyResidualLoss: expected [B, s, s] or [B, 1, s, s] (the pressure is one channel), got "
                             f"{tuple(pred.shape)}")
        tabs = self._table((int(pred.shape[-2]), int(pred.shape[-1])), pred.device)
        return ops.darcy2d_residual(pred, inp, tabs, self._affine, self.size_average, self.reduction)


class ActiveScalarResidualLoss(_ResidualLoss):
    """Does the prediction p ~ (c, q, v)(t + interval) follow from the input x = (c, q, v)(t) under the active-scalar
    system of the generator (rpde.ops.nsc2d_solve, data_generation/active_scalar_2d.py) on the unit periodic square,

        w_t + u . grad w = viscosity lap w + buoyancy dc/dx1 + f,   c_t + u . grad c = diffusivity lap c,   w = curl u ?

    The data are concentration and velocity, channels (c, q, v) with u = (q, v); the equation evolves (w, c).  The
    vorticity of a field is the curl of its velocity channels, only the solenoidal part of a predicted velocity advects,
    and the loss also charges what the equation cannot see: the divergence delta of the predicted velocity and the change
    mu of its mean (the equation conserves the mean velocity).  With the exponential trapezoidal rule of
    VorticityResidualLoss per evolved variable (z = -interval viscosity lap for w, -interval diffusivity lap for c; the
    buoyancy is not stiff and sits with the advection, as in the generator) giving r_w and r_c,

        E_ru = sum_{k != 0} c (|r^_w|^2 + |delta^|^2) / lap / (M N) + |mu|^2 / (M N),    E_rc = sum c |r^_c|^2 / (M N)
        rel[b] = sqrt(scalar_weight E_rc + E_ru) / (sqrt(scalar_weight |x_c|^2 + |x_q|^2 + |x_v|^2) + 1e-8)

    -- the vorticity's residual measured as the velocity it induces, in the norm of the data's channels -- then mean /
    sum / per-sample vector as RelativeL2Loss.  `interval` is the time between input and prediction: the snapshot
    interval of the data set, not the solver's step.  Float64 figures at viscosity 1e-3, diffusivity 2e-3, buoyancy 5,
    interval 0.05 (DESIGN.md 10.15 has the table): an exact pair gives 1.0e-3 .. 8.6e-3 against 0.074 .. 0.18 for the
    trivial predictor p = x; without the buoyancy term the exact pair is 7.6 .. 46 times worse.

    forcing: None, "reference" (the forcing of data_generation/ns_2d.py on each grid) or one [M, N] tensor for ONE grid.
    forward(pred, target, inp): the target is unused and may be None; pred, inp [B, 3, M, N] fp32 tensors on the GPU in
    the channel order (c, q, v) (anything else: ValueError), gradient for pred only.  set_affine takes one map for the
    three channels (the loaders' statistics are scalar); the per-(grid, device) table cache and warm((M, N), device) as
    in EquationResidualLoss."""

    dims = 2
    channels = 3
    _explicit_kind = "forcing"

    def __init__(self, viscosity, diffusivity, buoyancy, interval, forcing=None, scalar_weight=1.0, size_average=True,
                 reduction=True):
        super().__init__(size_average, reduction)
        vals = [float(viscosity), float(diffusivity), float(buoyancy), float(interval), float(scalar_weight)]
        if not all(math.isfinite(v) for v in vals) or vals[0] < 0 or vals[1] < 0 or not vals[3] > 0 or vals[4] < 0:
            raise ValueError(f"ActiveScalarResidualLoss: viscosity {viscosity}, diffusivity {diffusivity} and scalar_weight "
                             f"{scalar_weight} must be >= 0, interval {interval} positive and buoyancy {buoyancy} finite")
        self.viscosity, self.diffusivity, self.buoyancy, self.interval, self.scalar_weight = vals
        if torch.is_tensor(forcing):
            if forcing.dim() != 2:
                raise ValueError(f"ActiveScalarResidualLoss: a forcing tensor is one [M, N] field, got {tuple(forcing.shape)}")
            self._explicit = forcing.detach().double().cpu()
            self.forcing = "explicit"
        elif forcing in (None, "reference"):
            self.forcing = forcing
        else:
            raise ValueError(f"ActiveScalarResidualLoss: forcing must be None, 'reference' or an [M, N] tensor, got {forcing!r}")

    def _build(self, grid, device):
        tabs = ops.nsc2d_residual_tables(grid[0], grid[1], self.viscosity, self.diffusivity, self.interval)
        if self.forcing is None:
            f = None
        elif self._explicit is not None:
            if tuple(self._explicit.shape) != tuple(grid):
                raise ValueError(f"ActiveScalarResidualLoss: the forcing of shape {tuple(self._explicit.shape)} does not "
                                 f"serve the grid {grid}")
            f = self._explicit
        else:
            f = reference_forcing(*grid)
        fs = None if f is None else ops.ns2d_residual_forcing(f, self.viscosity, self.interval).to(device).contiguous()
        return tuple(t.to(device).contiguous() for t in tabs), fs

    def forward(self, pred, target, inp):
        if inp is None:
            raise self._no_input()
        for name, t in (("prediction", pred), ("input", inp)):
            if t.dim() != 4 or t.shape[1] != 3:
                raise ValueError(f"ActiveScalarResidualLoss: the {name} must be [B, 3, M, N] with the channels in the order "
                                 f"(c, q, v) -- concentration, then the velocity (q, v) -- got {tuple(t.shape)}")
        tabs, fs = self._table((int(pred.shape[-2]), int(pred.shape[-1])), pred.device)
        return ops.nsc2d_residual(pred, inp, tabs, self.buoyancy, fs, self.scalar_weight, self._affine, self.size_average,
                                  self.reduction)


def call_loss(fn, pred, target, inp):
    """fn(pred, target, inp) for an objective whose `takes_input` is true, fn(pred, target) for every other"""
    return fn(pred, target, inp) if getattr(fn, "takes_input", False) else fn(pred, target)


class SumLoss(nn.Module):
    """sum_i weight_i loss_i(x, y) as one callable: SumLoss([(1.0, RelativeL2Loss()), (0.1, SpectrumMatchingLoss(1))]).
    warm() goes to the terms that have one.  A term whose `takes_input` is true (EquationResidualLoss) is called as
    loss_i(x, y, inp) with the network's input; `takes_input` of the sum is true when any term's is."""

    def __init__(self, terms):
        super().__init__()
        terms = [(float(w), fn) for w, fn in terms]
        if not terms:
            raise ValueError("SumLoss: no terms")
        self.weights = [w for w, _ in terms]
        self.terms = nn.ModuleList([fn for _, fn in terms])
        self.takes_input = any(getattr(fn, "takes_input", False) for fn in self.terms)

    def warm(self, spatial_shape, device="cuda") -> None:
        for fn in self.terms:
            if hasattr(fn, "warm"):
                fn.warm(spatial_shape, device)

    def forward(self, x, y, inp=None):
        if self.takes_input and inp is None:
            raise ValueError("SumLoss: a term needs the network's input (call it as loss(pred, target, inp))")
        out = None
        for w, fn in zip(self.weights, self.terms):
            v = call_loss(fn, x, y, inp) * w
            out = v if out is None else out + v
        return out
