"""The U-Net side of rpde.ops (re-exported there): what the PDEBench U-Net (reference models/unet.py) needs beyond the
CNO layers of rpde/cno.py -- a norm's apply step, tanh and MaxPool(2) in one pass with a one-pass backward, and
ConvTranspose(kernel_size = 2, stride = 2) -- over the kernels of csrc/unet.hip (the U-Net group of include/rpde.h).
One Function per operation serves both ranks: [B, C, n] is the plane [B, C, 1, n] with windows and taps of one row.

BatchNorm's statistics, buffer semantics and chain rule are rpde/cno.py's (_bn_statistics, _bn_backward); GroupNorm needs
no kernel of its own: its statistics are rpde_cno_moments on the view [1, B G, (C / G) n], its apply step the tanh
kernel's prologue on the view [1, B C, n] with per-(sample, channel) coefficients, its backward rpde_cno_moments and
rpde_cno_affine on that view.
"""
from __future__ import annotations

from typing import Optional

import torch

from ._lib import check, load, ptr, stream_ptr
from .cno import _affine, _bn_backward, _bn_statistics, _bwd_weight, _f32c, _moments, _plane, _points


def _tanh_pool_fwd(z, scale, shift, pool: bool, fold_batch: bool):
    """act = tanh(scale z + shift) and, with pool, its MaxPool(2); fold_batch: scale / shift are per (sample, channel)"""
    H, W, ky = _plane(z, 2)
    B, Cc = int(z.shape[0]), int(z.shape[1])
    act = torch.empty_like(z)
    pooled = None
    if pool:
        if H // ky == 0 or W // 2 == 0:
            raise ValueError(f"tanh_pool: nothing left to pool from input size {tuple(z.shape)}")
        pooled = torch.empty(z.shape[:2] + ((W // 2,) if ky == 1 else (H // 2, W // 2)), dtype=torch.float32, device=z.device)
    Bk, Ck = (1, B * Cc) if fold_batch else (B, Cc)
    check(load().rpde_unet_tanh_pool_fwd(ptr(z), ptr(scale), ptr(shift), ptr(act), ptr(pooled), Bk, Ck, H, W, ky, stream_ptr()),
          "unet_tanh_pool_fwd")
    return act, pooled


def _tanh_pool_bwd(act, g_act, g_pool):
    H, W, ky = _plane(act, 2)
    gy = torch.empty_like(act)
    g_act, g_pool = (None if g is None else _f32c(g) for g in (g_act, g_pool))
    check(load().rpde_unet_tanh_pool_bwd(ptr(act), ptr(g_act), ptr(g_pool), ptr(gy), int(act.shape[0]), int(act.shape[1]), H, W,
                                         ky, stream_ptr()), "unet_tanh_pool_bwd")
    return gy


class _NormTanh(torch.autograd.Function):
    """norm -> tanh (-> MaxPool(2)) on z [B, C, n] or [B, C, H, W]; the normalised tensor is never written and both
    outputs share one backward launch.  mode: "none" (tanh alone, or behind the caller's own per-channel affine
    gamma z + beta, whose chain rule stays the caller's), "batch" / "running" (BatchNorm with batch / running statistics
    mean, invstd [C]), "group" (GroupNorm, mean, invstd [B G]).  Saved for backward: z (the norm's chain rule) and act."""

    @staticmethod
    def forward(ctx, z, gamma, beta, mean, invstd, pool: bool, mode: str):
        z = _f32c(z)
        B, Cc = int(z.shape[0]), int(z.shape[1])
        scale = shift = None
        if mode == "none":
            if gamma is not None:
                scale, shift = _f32c(gamma.detach()), _f32c(beta.detach())
        else:
            g64 = gamma.detach().double()
            if mode == "group":
                G = mean.numel() // B
                scale64 = (g64.view(1, G, Cc // G) * invstd.view(B, G, 1)).reshape(-1)
                shift64 = beta.detach().double().repeat(B) - mean.view(B, G, 1).expand(B, G, Cc // G).reshape(-1) * scale64
            else:
                scale64 = g64 * invstd
                shift64 = beta.detach().double() - mean * scale64
            scale, shift = scale64.float(), shift64.float()
            ctx.stats = (g64, mean, invstd, scale64)
        act, pooled = _tanh_pool_fwd(z, scale, shift, pool, mode == "group")
        ctx.save_for_backward(z if mode != "none" else None, act)
        ctx.mode = mode
        ctx.set_materialize_grads(False)
        if not pool:
            return act
        return act, pooled

    @staticmethod
    def backward(ctx, g_act, g_pool=None):
        z, act = ctx.saved_tensors
        mode = ctx.mode
        if g_act is None and g_pool is None:
            return (None,) * 7
        gy = _tanh_pool_bwd(act, g_act, g_pool)
        if mode == "none":
            return gy, None, None, None, None, None, None
        g64, mean, invstd, scale64 = ctx.stats
        if mode != "group":
            dz, dgamma, dbeta = _bn_backward(gy, z, g64, mean, invstd, scale64, mode == "batch")
            return dz, dgamma, dbeta, None, None, None, None
        # GroupNorm: with r, mu of the (sample, group) and zhat = (z - mu) r,
        #   dz = r (gamma gy - mean_g(gamma gy) - zhat mean_g(gamma gy zhat)),  the means over the group's Ng values
        B, Cc, n = int(z.shape[0]), int(z.shape[1]), _points(z)
        G = mean.numel() // B
        cg = Cc // G
        Ng = float(cg * n)
        s = _moments(gy.view(1, B * Cc, n), z.view(1, B * Cc, n)).view(B, G, cg, 4)
        sum_gy, sum_gyz = s[..., 0], s[..., 2]
        r, mu = invstd.view(B, G, 1), mean.view(B, G, 1)
        gam = g64.view(1, G, cg)
        gyzhat = r * (sum_gyz - mu * sum_gy)                      # sum gy zhat per (sample, channel)
        dgamma = gyzhat.sum(0).reshape(-1)
        dbeta = sum_gy.sum(0).reshape(-1)
        m1 = (gam * sum_gy).sum(2, keepdim=True) / Ng
        m2 = (gam * gyzhat).sum(2, keepdim=True) / Ng
        p0 = (r * gam).reshape(-1)
        p1 = (-r * r * m2).expand(B, G, cg).reshape(-1)
        p2 = (-r * m1 + r * r * mu * m2).expand(B, G, cg).reshape(-1)
        dz = _affine(gy.view(1, B * Cc, n), z.view(1, B * Cc, n), p0, p1, p2).view_as(z)
        return dz, dgamma.float(), dbeta.float(), None, None, None, None


def _rank_check(z: torch.Tensor, what: str) -> None:
    if z.dim() not in (3, 4):
        raise ValueError(f"{what}: expected [B, C, n] or [B, C, H, W], got {tuple(z.shape)}")


def tanh_pool(z: torch.Tensor, scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None, pool: bool = False):
    """act = tanh(scale z + shift) on [B, C, n] or [B, C, H, W] (scale, shift [C], or neither), and with pool=True also
    MaxPool(2) of it, written in the same pass: returns act, or (act, pooled).  The gradient returned is the one with
    respect to scale z + shift: a caller that passes an affine owns its chain rule (norm_tanh does)."""
    _rank_check(z, "tanh_pool")
    if (scale is None) != (shift is None):
        raise ValueError("tanh_pool: scale and shift come together")
    return _NormTanh.apply(z, scale, shift, None, None, bool(pool), "none")


def norm_tanh(z: torch.Tensor, bn: torch.nn.Module, pool: bool = False):
    """tanh(bn(z)) for an nn.BatchNorm1d / nn.BatchNorm2d `bn`, which owns the parameters and buffers: torch's semantics
    in training and eval mode (rpde.ops.batchnorm1d states them).  With pool=True returns (act, MaxPool(2)(act))."""
    _rank_check(z, "norm_tanh")
    momentum = 0.1 if bn.momentum is None else bn.momentum
    mean, invstd, use_batch = _bn_statistics(z, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.training, momentum,
                                             bn.eps)
    return _NormTanh.apply(z, bn.weight, bn.bias, mean, invstd, bool(pool), "batch" if use_batch else "running")


def groupnorm_tanh(z: torch.Tensor, num_groups: int, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5,
                   pool: bool = False):
    """tanh(GroupNorm(num_groups)(z)) with per-channel weight and bias, statistics per (sample, group) as in
    nn.GroupNorm (biased variance, the same in training and eval mode).  With pool=True returns (act, MaxPool(2)(act))."""
    _rank_check(z, "groupnorm_tanh")
    B, Cc, G = int(z.shape[0]), int(z.shape[1]), int(num_groups)
    if G < 1 or Cc % G:
        raise ValueError(f"groupnorm_tanh: {Cc} channels do not split into {G} groups")
    zc = _f32c(z.detach())
    Ng = float(Cc // G * _points(z))
    s = _moments(zc.view(1, B * G, -1), zc.view(1, B * G, -1))
    mean = s[:, 1] / Ng
    var = (s[:, 3] / Ng - mean * mean).clamp_min(0.0)
    return _NormTanh.apply(z, weight, bias, mean, torch.rsqrt(var + eps), bool(pool), "group")


class _UpConv(torch.autograd.Function):
    """ConvTranspose(kernel_size = 2, stride = 2) of x's rank: [B, Cin, n] with w [Cin, Cout, 2], [B, Cin, H, W] with
    w [Cin, Cout, 2, 2]; the weight is used as it lies"""

    @staticmethod
    def forward(ctx, x, w, b):
        x, wc = _f32c(x), _f32c(w.detach())
        bias = None if b is None else _f32c(b.detach())
        H, W, ky = _plane(x, 2)
        B, Cin, Cout = int(x.shape[0]), int(x.shape[1]), int(w.shape[1])
        out = torch.empty((B, Cout, 2 * W) if ky == 1 else (B, Cout, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
        check(load().rpde_unet_upconv_fwd(ptr(x), ptr(wc), ptr(bias), ptr(out), B, Cin, Cout, H, W, ky, stream_ptr()), "unet_upconv_fwd")
        ctx.save_for_backward(x, wc)
        ctx.has_bias = b is not None
        return out

    @staticmethod
    def backward(ctx, g):
        x, wc = ctx.saved_tensors
        H, W, ky = _plane(x, 2)
        dims = (int(x.shape[0]), int(x.shape[1]), int(wc.shape[1]), H, W)
        g = _f32c(g)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            check(load().rpde_unet_upconv_bwd_data(ptr(g), ptr(wc), ptr(gx), *dims, ky, stream_ptr()), "unet_upconv_bwd_data")
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            gw = torch.empty_like(wc)
            gb = torch.empty(dims[2], dtype=torch.float32, device=x.device) if ctx.has_bias else None
            _bwd_weight("unet_upconv_bwd_weight", x, g, gw, gb, dims, ky, dims)
        return gx, gw, gb


def upconv1d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.ConvTranspose1d(kernel_size=2, stride=2) on x [B, Cin, n] with weight [Cin, Cout, 2]: [B, Cout, 2 n]"""
    if x.dim() != 3:
        raise ValueError(f"upconv1d: expected [B, C, n], got {tuple(x.shape)}")
    if weight.dim() != 3 or weight.shape[0] != x.shape[1] or weight.shape[2] != 2:
        raise ValueError(f"upconv1d: weight {tuple(weight.shape)} does not fit {x.shape[1]} input channels and 2 taps")
    return _UpConv.apply(x, weight, bias)


def upconv2d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.ConvTranspose2d(kernel_size=2, stride=2) on x [B, Cin, H, W] with weight [Cin, Cout, 2, 2]: [B, Cout, 2 H, 2 W]"""
    if x.dim() != 4:
        raise ValueError(f"upconv2d: expected [B, C, H, W], got {tuple(x.shape)}")
    if weight.dim() != 4 or weight.shape[0] != x.shape[1] or tuple(weight.shape[2:]) != (2, 2):
        raise ValueError(f"upconv2d: weight {tuple(weight.shape)} does not fit {x.shape[1]} input channels and 2 x 2 taps")
    return _UpConv.apply(x, weight, bias)
