"""The CNO side of rpde.ops (re-exported there): the banded tables of torch's antialiased bicubic resampling, the
autograd Functions over the fused alias-free activation kernels in 1-D and 2-D, and the rest of a CNO block -- Conv1d /
Conv2d (k = 3), BatchNorm, the skip add -- over their kernels (csrc/cno.hip and csrc/cno2d.hip: the activation of each
rank; csrc/cno_layers.hip: the rest; the CNO groups of include/rpde.h).  One Function per operation serves both ranks
(the activation picks the C entry by the tensor's rank, the convolution's entries take both as a plane with ky rows of
taps); the public names below are the argument-checking fronts.

CNO_LReLu (reference models/CNO1d.py:30-45) is  resample to 2 in_size -> LeakyReLU -> resample to out_size, both
resamplings being F.interpolate(mode="bicubic", antialias=True, align_corners=False) on a (1, n) image: the identity
along the height axis and a fixed banded linear map along the width.  The tables below are those maps.  In 2-D
(reference models/CNO2d.py:31-46) the resampling of a plane is the tensor product of two of them, one per axis.
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional, Tuple

import torch

from ._lib import check, load, ptr, stream_ptr

LEAKY_SLOPE = 0.01          # nn.LeakyReLU()'s default, the only slope the reference uses


def _keys_cubic(t: float, a: float = -0.5) -> float:
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0
    if t < 2.0:
        return (((t - 5.0) * t + 8.0) * t - 4.0) * a
    return 0.0


def cno_resample_table(n_in: int, n_out: int):
    """The banded form of F.interpolate(mode="bicubic", antialias=True, align_corners=False) along one axis, n_in ->
    n_out points, in float64: (start [n_out] int64, count [n_out] int64, weights [n_out, T] float64, zero-padded to the
    widest row's T taps).  Output i is  sum_j weights[i, j] * x[start[i] + j],  j < count[i].

    The filter is the Keys cubic (a = -0.5), stretched by the ratio when downsampling (the antialiasing), clipped at
    the borders -- not replicated -- and normalised to sum 1 after clipping.  Equal sizes give the identity exactly."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"cno_resample_table: sizes must be positive, got {n_in} -> {n_out}")
    if n_in == n_out:
        i = torch.arange(n_out, dtype=torch.int64)
        return i, torch.ones(n_out, dtype=torch.int64), torch.ones(n_out, 1, dtype=torch.float64)
    scale = n_in / n_out
    support = 2.0 * scale if scale >= 1.0 else 2.0
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    rows = []
    for i in range(n_out):
        c = scale * (i + 0.5)
        xmin = max(0, int(c - support + 0.5))
        xmax = min(n_in, int(c + support + 0.5))
        w = [_keys_cubic((j + xmin - c + 0.5) * inv) for j in range(xmax - xmin)]
        total = math.fsum(w)
        rows.append((xmin, [v / total for v in w]))
    T = max(len(w) for _, w in rows)
    start = torch.tensor([s for s, _ in rows], dtype=torch.int64)
    count = torch.tensor([len(w) for _, w in rows], dtype=torch.int64)
    weights = torch.zeros(n_out, T, dtype=torch.float64)
    for i, (_, w) in enumerate(rows):
        weights[i, :len(w)] = torch.tensor(w, dtype=torch.float64)
    return start, count, weights


def cno_transpose_band(start, count, weights, n_in: int):
    """The same map listed by source: for source j the contiguous run of outputs that touch it, as (start [n_in],
    count [n_in], weights [n_in, T']) with weights[j, t] = M[start[j] + t, j].  What a backward pass gathers over
    instead of scattering.  Outputs inside a run whose own band does not reach j (none for these filters) hold zero."""
    n_out = int(start.numel())
    first = [n_out] * n_in
    last = [-1] * n_in
    for i in range(n_out):
        for j in range(int(start[i]), int(start[i]) + int(count[i])):
            first[j] = min(first[j], i)
            last[j] = max(last[j], i)
    t_start = torch.tensor([f if l >= 0 else 0 for f, l in zip(first, last)], dtype=torch.int64)
    t_count = torch.tensor([l - f + 1 if l >= 0 else 0 for f, l in zip(first, last)], dtype=torch.int64)
    T = max(1, int(t_count.max()))
    t_w = torch.zeros(n_in, T, dtype=torch.float64)
    for j in range(n_in):
        for t in range(int(t_count[j])):
            i = int(t_start[j]) + t
            k = j - int(start[i])
            if 0 <= k < int(count[i]):
                t_w[j, t] = weights[i, k]
    return t_start, t_count, t_w


def cno_dense(start, count, weights, n_in: int, transposed: bool = False) -> torch.Tensor:
    """the dense [n_out, n_in] matrix of a band (of cno_resample_table, or with transposed=True of cno_transpose_band,
    whose n_in is then the number of outputs)"""
    rows = int(start.numel())
    M = torch.zeros(rows, n_in, dtype=weights.dtype)
    for i in range(rows):
        s, c = int(start[i]), int(count[i])
        M[i, s:s + c] = weights[i, :c]
    return M.t().contiguous() if transposed else M


class CnoBand(NamedTuple):
    """one band on the device: span [rows, 2] int32 (start, count), weights [rows, T] float32, T a multiple of 4"""
    span: torch.Tensor
    weights: torch.Tensor
    taps: int


class CnoTables(NamedTuple):
    n_in: int
    n_out: int
    fwd: CnoBand            # per output: the sources it reads
    bwd: CnoBand            # per source: the outputs that read it


_CNO_TABLES_DEV: Dict[Tuple, CnoTables] = {}


def _device_band(start, count, weights, device) -> CnoBand:
    T = (int(weights.shape[1]) + 3) // 4 * 4
    w = torch.zeros(weights.shape[0], T, dtype=torch.float32)
    w[:, :weights.shape[1]] = weights.to(torch.float32)
    span = torch.stack([start, count], dim=1).to(torch.int32).contiguous()
    return CnoBand(span.to(device), w.to(device), T)


def cno_tables(device, n_in: int, n_out: int) -> CnoTables:
    """device tables of the n_in -> n_out resampling, built once per (device, n_in, n_out)"""
    key = (torch.device(device), int(n_in), int(n_out))
    t = _CNO_TABLES_DEV.get(key)
    if t is None:
        s, c, w = cno_resample_table(n_in, n_out)
        ts, tc, tw = cno_transpose_band(s, c, w, int(n_in))
        t = _CNO_TABLES_DEV[key] = CnoTables(int(n_in), int(n_out), _device_band(s, c, w, device),
                                             _device_band(ts, tc, tw, device))
    return t


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _bands(t: CnoBand):
    return t.span.data_ptr(), ptr(t.weights), t.taps


class _CnoAct(torch.autograd.Function):
    """the activation of x's rank: [B, C, n] through rpde_cno_act1d_*, [B, C, H, W] through rpde_cno_act2d_*, whose
    tables come one per axis (U_y, U_x; the mid and output planes are square, so D serves both axes)"""

    @staticmethod
    def forward(ctx, x, scale, shift, n_mid: int, n_out: int, slope: float):
        lib = load()
        x = _f32c(x)
        if scale is not None:
            scale, shift = _f32c(scale.detach()), _f32c(shift.detach())
        dev = x.device
        D = cno_tables(dev, n_mid, n_out)
        if x.dim() == 3:
            B, Cc, n_in = x.shape
            U = cno_tables(dev, n_in, n_mid)
            out = torch.empty(B, Cc, n_out, dtype=torch.float32, device=dev)
            check(lib.rpde_cno_act1d_fwd(ptr(x), ptr(scale), ptr(shift), ptr(out), B, Cc, n_in, n_mid, n_out, slope,
                                         *_bands(U.fwd), *_bands(D.fwd), stream_ptr()), "cno_act1d_fwd")
        else:
            B, Cc, h_in, w_in = x.shape
            Uy, Ux = cno_tables(dev, h_in, n_mid), cno_tables(dev, w_in, n_mid)
            out = torch.empty(B, Cc, n_out, n_out, dtype=torch.float32, device=dev)
            check(lib.rpde_cno_act2d_fwd(ptr(x), ptr(scale), ptr(shift), ptr(out), B, Cc, h_in, w_in, n_mid, n_mid, n_out, n_out,
                                         slope, *_bands(Uy.fwd), *_bands(Ux.fwd), *_bands(D.fwd), *_bands(D.fwd), stream_ptr()),
                  "cno_act2d_fwd")
        ctx.save_for_backward(x, scale, shift)
        ctx.meta = (n_mid, n_out, slope)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = load()
        x, scale, shift = ctx.saved_tensors
        n_mid, n_out, slope = ctx.meta
        g = _f32c(g)
        dev = x.device
        D = cno_tables(dev, n_mid, n_out)
        gy = torch.empty_like(x)
        if x.dim() == 3:
            B, Cc, n_in = x.shape
            U = cno_tables(dev, n_in, n_mid)
            check(lib.rpde_cno_act1d_bwd(ptr(x), ptr(scale), ptr(shift), ptr(g), ptr(gy), B, Cc, n_in, n_mid, n_out, slope,
                                         *_bands(U.fwd), *_bands(U.bwd), *_bands(D.bwd), stream_ptr()), "cno_act1d_bwd")
        else:
            B, Cc, h_in, w_in = x.shape
            Uy, Ux = cno_tables(dev, h_in, n_mid), cno_tables(dev, w_in, n_mid)
            check(lib.rpde_cno_act2d_bwd(ptr(x), ptr(scale), ptr(shift), ptr(g), ptr(gy), B, Cc, h_in, w_in, n_mid, n_mid, n_out,
                                         n_out, slope, *_bands(Uy.fwd), *_bands(Ux.fwd), *_bands(Uy.bwd), *_bands(Ux.bwd),
                                         *_bands(D.bwd), *_bands(D.bwd), stream_ptr()), "cno_act2d_bwd")
        return gy, None, None, None, None, None


def cno_act1d(x: torch.Tensor, in_size: int, out_size: int, scale: Optional[torch.Tensor] = None,
              shift: Optional[torch.Tensor] = None, slope: float = LEAKY_SLOPE) -> torch.Tensor:
    """CNO_LReLu(in_size, out_size) on x [B, C, n] in one kernel: resample n -> 2 in_size, LeakyReLU, resample to
    out_size; the 2 in_size signal never reaches memory.  scale / shift [C]: a per-channel affine applied to x first
    (a BatchNorm's apply step).  The gradient returned is the one with respect to scale * x + shift: the caller that
    passes an affine owns its chain rule (rpde.ops.batchnorm1d does)."""
    if x.dim() != 3:
        raise ValueError(f"cno_act1d: expected [B, C, n], got {tuple(x.shape)}")
    if (scale is None) != (shift is None):
        raise ValueError("cno_act1d: scale and shift come together")
    return _CnoAct.apply(x, scale, shift, 2 * int(in_size), int(out_size), float(slope))


def cno_act2d(x: torch.Tensor, in_size: int, out_size: int, scale: Optional[torch.Tensor] = None,
              shift: Optional[torch.Tensor] = None, slope: float = LEAKY_SLOPE) -> torch.Tensor:
    """CNO_LReLu(in_size, out_size) on x [B, C, H, W] in one kernel: resample the plane to (2 in_size)^2, LeakyReLU,
    resample to out_size^2, whatever (H, W) is; the (2 in_size)^2 plane never reaches memory.  scale / shift [C] and the
    gradient as in cno_act1d."""
    if x.dim() != 4:
        raise ValueError(f"cno_act2d: expected [B, C, H, W], got {tuple(x.shape)}")
    if (scale is None) != (shift is None):
        raise ValueError("cno_act2d: scale and shift come together")
    return _CnoAct.apply(x, scale, shift, 2 * int(in_size), int(out_size), float(slope))


# ----------------------------------------------------------------------------
# Conv1d / Conv2d (k = 3, padding = 1), BatchNorm and the skip add of a CNO block (the CNO groups of include/rpde.h)
# ----------------------------------------------------------------------------
def _bcn(x: torch.Tensor, what: str):
    if x.dim() != 3:
        raise ValueError(f"{what}: expected [B, C, n], got {tuple(x.shape)}")
    return int(x.shape[0]), int(x.shape[1]), int(x.shape[2])


def _bchw(x: torch.Tensor, what: str):
    if x.dim() != 4:
        raise ValueError(f"{what}: expected [B, C, H, W], got {tuple(x.shape)}")
    return tuple(int(v) for v in x.shape)


def _points(x: torch.Tensor) -> int:
    """values per (sample, channel): n of [B, C, n], H W of [B, C, H, W] -- what the per-channel kernels run over"""
    return int(x.shape[2]) if x.dim() == 3 else int(x.shape[2]) * int(x.shape[3])


def _plane(x: torch.Tensor, rows: int):
    """(H, W, ky) of a channels-first tensor as the kernels see it: [B, C, n] is a plane of one row with one row of taps
    or windows, [B, C, H, W] has `rows` of them"""
    return (1, int(x.shape[2]), 1) if x.dim() == 3 else (int(x.shape[2]), int(x.shape[3]), rows)


def _bwd_weight(entry: str, x, g, gw, gb, dims, ky: int, slice_args) -> None:
    """gw and gb (or None) from rpde_<entry>(x, g, gw, gb, *dims, ky, partial, slices, stream), the weight gradient of
    _ConvK3 and of rpde/unet.py's _UpConv: more than one slice leaves partial sums [slices][gw.numel() + Cout]"""
    lib = load()
    slices = getattr(lib, f"rpde_{entry}_slices")(*slice_args)
    part = torch.empty(slices, gw.numel() + dims[2], dtype=torch.float32, device=x.device) if slices > 1 else None
    check(getattr(lib, f"rpde_{entry}")(ptr(x), ptr(g), ptr(gw), ptr(gb), *dims, ky, ptr(part), slices, stream_ptr()), entry)


class _ConvK3(torch.autograd.Function):
    """Conv(k = 3, padding = 1) of x's rank through rpde_conv_k3_*: [B, Cin, n] with w [Cout, Cin, 3] is the plane
    [B, Cin, 1, n] with one row of taps, [B, Cin, H, W] with w [Cout, Cin, 3, 3] has three"""

    @staticmethod
    def forward(ctx, x, w, b):
        x = _f32c(x)
        H, W, ky = _plane(x, 3)
        B, Cin, Cout = int(x.shape[0]), int(x.shape[1]), int(w.shape[0])
        bias = None if b is None else _f32c(b.detach())
        wt = _f32c(w.detach()).reshape(Cout, Cin, 3 * ky).permute(2, 0, 1).contiguous()    # tap-major [3 ky, Cout, Cin]: a layout copy
        out = torch.empty((B, Cout) + x.shape[2:], dtype=torch.float32, device=x.device)
        check(load().rpde_conv_k3_fwd(ptr(x), ptr(wt), ptr(bias), ptr(out), B, Cin, Cout, H, W, ky, stream_ptr()), "conv_k3_fwd")
        ctx.save_for_backward(x, wt)
        ctx.has_bias = b is not None
        return out

    @staticmethod
    def backward(ctx, g):
        x, wt = ctx.saved_tensors
        H, W, ky = _plane(x, 3)
        dims = (int(x.shape[0]), int(x.shape[1]), int(wt.shape[1]), H, W)
        Cin, Cout = dims[1:3]
        g = _f32c(g)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            check(load().rpde_conv_k3_bwd_data(ptr(g), ptr(wt), ptr(gx), *dims, ky, stream_ptr()), "conv_k3_bwd_data")
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            gw = torch.empty((Cout, Cin) + (3,) * (x.dim() - 2), dtype=torch.float32, device=x.device)
            gb = torch.empty(Cout, dtype=torch.float32, device=x.device) if ctx.has_bias else None
            _bwd_weight("conv_k3_bwd_weight", x, g, gw, gb, dims, ky, dims + (ky,))
        return gx, gw, gb


def conv1d_k3(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.Conv1d(kernel_size=3, padding=1) on x [B, Cin, n] with weight [Cout, Cin, 3]"""
    B, Cin, n = _bcn(x, "conv1d_k3")
    if weight.dim() != 3 or weight.shape[1] != Cin or weight.shape[2] != 3:
        raise ValueError(f"conv1d_k3: weight {tuple(weight.shape)} does not fit {Cin} input channels and 3 taps")
    return _ConvK3.apply(x, weight, bias)


def conv2d_k3(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.Conv2d(kernel_size=3, padding=1) on x [B, Cin, H, W] with weight [Cout, Cin, 3, 3]"""
    Cin = _bchw(x, "conv2d_k3")[1]
    if weight.dim() != 4 or weight.shape[1] != Cin or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError(f"conv2d_k3: weight {tuple(weight.shape)} does not fit {Cin} input channels and 3 x 3 taps")
    return _ConvK3.apply(x, weight, bias)


def _moments(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[C, 4] float64: (sum a, sum b, sum a b, sum b^2) per channel"""
    B, Cc, n = a.shape[0], a.shape[1], _points(a)
    sums = torch.empty(Cc, 4, dtype=torch.float64, device=a.device)
    check(load().rpde_cno_moments(ptr(a), ptr(b), sums.data_ptr(), B, Cc, n, stream_ptr()), "cno_moments")
    return sums


def _affine(a, b, p0, p1, p2, residual=None) -> torch.Tensor:
    """p0 a + p1 b + p2 (+ residual), coefficients [C] taken in float64"""
    B, Cc, n = a.shape[0], a.shape[1], _points(a)
    out = torch.empty_like(a)
    p0, p1, p2 = (None if p is None else p.to(torch.float64).contiguous() for p in (p0, p1, p2))
    check(load().rpde_cno_affine(ptr(a), ptr(b), p0.data_ptr(), None if p1 is None else p1.data_ptr(), p2.data_ptr(),
                                 ptr(residual), ptr(out), B, Cc, n, stream_ptr()), "cno_affine")
    return out


class _BatchNorm(torch.autograd.Function):
    """BatchNorm on z [B, C, n] or [B, C, H, W] (the moments and affine kernels see the plane as n = H W points),
    followed by the CNO activation of z's rank (act = (n_mid, n_out, slope): the normalised tensor is never written, its
    apply step is the activation kernel's prologue) or by an optional skip add.  The per-channel coefficients -- C
    numbers each -- are formed in float64 by torch from the moments kernel's sums."""

    @staticmethod
    def forward(ctx, z, gamma, beta, mean, invstd, residual, act, batch_stats: bool):
        z = _f32c(z)
        g64 = gamma.detach().double()
        scale64 = g64 * invstd
        shift64 = beta.detach().double() - mean * scale64
        scale, shift = scale64.float(), shift64.float()
        if act is not None:
            out = _CnoAct.forward(ctx, z, scale, shift, *act)         # saves (z, scale, shift) and meta on ctx
        else:
            out = _affine(z, None, scale64, None, shift64, None if residual is None else _f32c(residual))
            ctx.save_for_backward(z, scale, shift)
        ctx.act = act
        ctx.stats = (g64, mean, invstd, scale64)
        ctx.has_residual = residual is not None
        ctx.batch_stats = batch_stats
        return out

    @staticmethod
    def backward(ctx, g):
        z, scale, shift = ctx.saved_tensors
        g64, mean, invstd, scale64 = ctx.stats
        g = _f32c(g)
        gy = _CnoAct.backward(ctx, g)[0] if ctx.act is not None else g
        dz, dgamma, dbeta = _bn_backward(gy, z, g64, mean, invstd, scale64, ctx.batch_stats)
        return dz, dgamma, dbeta, None, None, (g if ctx.has_residual else None), None, None


def _bn_backward(gy, z, g64, mean, invstd, scale64, batch_stats: bool):
    """(dz, dgamma, dbeta) of a BatchNorm from gy, the gradient with respect to its output: one moments pass over
    (gy, z), the C coefficients in float64 by torch, one affine pass"""
    N = float(z.shape[0] * _points(z))
    s = _moments(gy, z)
    sum_gy, sum_gyz = s[:, 0], s[:, 2]
    dbeta = sum_gy
    dgamma = invstd * (sum_gyz - mean * sum_gy)
    if batch_stats:
        # dz = (gamma / sigma) (gy - mean(gy) - zhat mean(gy zhat)),  zhat = (z - mean) / sigma
        k = g64 * invstd
        m1, m2 = sum_gy / N, dgamma / N
        p0, p1, p2 = k, -k * m2 * invstd, -k * m1 + k * m2 * invstd * mean
        dz = _affine(gy, z, p0, p1, p2)
    else:
        dz = _affine(gy, None, scale64, None, torch.zeros_like(scale64))
    return dz, dgamma.float(), dbeta.float()


def batchnorm1d(z: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, running_mean: Optional[torch.Tensor],
                running_var: Optional[torch.Tensor], num_batches_tracked: Optional[torch.Tensor] = None,
                training: bool = True, momentum: float = 0.1, eps: float = 1e-5, residual: Optional[torch.Tensor] = None,
                act: Optional[Tuple[int, int]] = None, slope: float = LEAKY_SLOPE) -> torch.Tensor:
    """nn.BatchNorm1d's forward on z [B, C, n], torch's semantics: batch statistics and the running-buffer update
    (unbiased running variance, num_batches_tracked + 1) in training mode, the running statistics in eval mode, a
    ValueError for training on one value per channel.  residual: added to the result (the residual block's skip).
    act = (in_size, out_size): CNO_LReLu(in_size, out_size) applied to the result in the same kernel."""
    _bcn(z, "batchnorm1d")
    return _batchnorm("batchnorm1d", z, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps,
                      residual, act, slope)


def batchnorm2d(z: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, running_mean: Optional[torch.Tensor],
                running_var: Optional[torch.Tensor], num_batches_tracked: Optional[torch.Tensor] = None,
                training: bool = True, momentum: float = 0.1, eps: float = 1e-5, residual: Optional[torch.Tensor] = None,
                act: Optional[Tuple[int, int]] = None, slope: float = LEAKY_SLOPE) -> torch.Tensor:
    """nn.BatchNorm2d's forward on z [B, C, H, W]: torch's semantics exactly as batchnorm1d states them, the statistics
    taken over (B, H, W).  act = (in_size, out_size): the 2-D CNO_LReLu(in_size, out_size) in the same kernel."""
    _bchw(z, "batchnorm2d")
    return _batchnorm("batchnorm2d", z, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps,
                      residual, act, slope)


def _bn_statistics(z, running_mean, running_var, num_batches_tracked, training, momentum, eps):
    """(mean, invstd, use_batch) of a BatchNorm on z, float64 [C]: the batch statistics with torch's running-buffer
    update in training mode (or without buffers), the running statistics otherwise"""
    B, n = int(z.shape[0]), _points(z)
    use_batch = training or running_mean is None
    if use_batch:
        if B * n <= 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(z.shape)}")
        zc = _f32c(z.detach())
        s = _moments(zc, zc)
        N = float(B * n)
        mean = s[:, 1] / N
        var = (s[:, 3] / N - mean * mean).clamp_min(0.0)
        if training and running_mean is not None:
            with torch.no_grad():
                running_mean.mul_(1.0 - momentum).add_((momentum * mean).to(running_mean.dtype))
                running_var.mul_(1.0 - momentum).add_((momentum * var * (N / (N - 1.0))).to(running_var.dtype))
                if num_batches_tracked is not None:
                    num_batches_tracked.add_(1)
    else:
        mean, var = running_mean.detach().double(), running_var.detach().double()
    return mean, torch.rsqrt(var + eps), use_batch


def _batchnorm(what, z, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps, residual, act,
               slope):
    if residual is not None and act is not None:
        raise ValueError(f"{what}: residual and act exclude each other")
    mean, invstd, use_batch = _bn_statistics(z, running_mean, running_var, num_batches_tracked, training, momentum, eps)
    fn_act = None if act is None else (2 * int(act[0]), int(act[1]), float(slope))
    return _BatchNorm.apply(z, weight, bias, mean, invstd, residual, fn_act, use_batch)


class _SkipAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, residual):
        a, residual = _f32c(a), _f32c(residual)
        one = torch.ones(a.shape[1], dtype=torch.float64, device=a.device)
        return _affine(a, None, one, None, torch.zeros_like(one), residual)

    @staticmethod
    def backward(ctx, g):
        return g, g


def skip_add(a: torch.Tensor, residual: torch.Tensor) -> torch.Tensor:
    """a + residual on [B, C, n] or [B, C, H, W] (a residual block without BatchNorm)"""
    if a.dim() not in (3, 4):
        raise ValueError(f"skip_add: expected [B, C, n] or [B, C, H, W], got {tuple(a.shape)}")
    return _SkipAdd.apply(a, residual)
