"""Spectral resize used by the resize-mode evaluators (reference:
utils/res_utils.py:29-50 ``resize``, :93-125 ``resize_1d``): rfft -> copy the
bins both sizes share -> irfft at the new size, scaled by out/in -- on the
MI355X through the same truncated-DFT plans as the spectral layers (analysis
at the source size, synthesis at the target size; nothing is zero-padded).

``downsample`` (reference :20-27) is another operator, used once at load time by
the active-matter loaders: it cuts the full complex spectrum to the signed
frequencies -N/2 .. N/2-1 on both axes, so the new Nyquist lines hold the old
-N/2 coefficients alone, where ``resize`` keeps the Hermitian pair of the half
spectrum.  Data preparation on the host, numpy only."""
from __future__ import annotations

import numpy as np

from rpde import ops


def downsample(u, N):
    """u [B, C, H, W] (numpy, H == W as the reference assumes) -> [B, C, N, N]: fft2 scaled by 1 / (H W), the signed
    frequencies -N/2 <= k <= N/2 - 1 of both axes in fft order, ifft2 without scaling, real part.  The dtype of u is kept
    for floating input (the transform runs in the precision numpy.fft gives it)."""
    u = np.asarray(u)
    if u.ndim != 4:
        raise ValueError(f"downsample: expected [B, C, H, W], got {u.shape}")
    H, N = u.shape[-2], int(N)
    if u.shape[-1] != H:
        raise ValueError(f"downsample: square images only, got {u.shape[-2:]}")
    k = np.rint(np.fft.fftfreq(H) * H)                     # signed frequencies in fft order
    keep = np.flatnonzero((2 * k >= -N) & (2 * k <= N - 2))
    spec = np.fft.fft2(u, norm="forward")[:, :, keep][:, :, :, keep]
    out = np.fft.ifft2(spec, norm="forward").real
    return out.astype(u.dtype) if np.issubdtype(u.dtype, np.floating) else out


def resize(x, out_size, permute=False):
    """x [B,C,M,N] (or [B,M,N,C] with ``permute``) -> spatial size ``out_size``"""
    if permute:
        x = x.permute(0, 3, 1, 2)
    y = ops.resize2d(x.contiguous(), out_size)
    return y.permute(0, 2, 3, 1) if permute else y


def resize_1d(x, out_size):
    """x [..., n] -> [..., out_size]"""
    return ops.resize1d(x, int(out_size))
