"""Float64 restatement of the U-Net pieces (rpde/unet.py over csrc/unet.hip) on the CPU, in torch functional calls:
what tests/test_gpu_unet_layers.py compares the kernels with.  Own code."""
from __future__ import annotations

import torch
import torch.nn.functional as F


def rel_l2(got: torch.Tensor, ref: torch.Tensor) -> float:
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).norm() / (ref.norm() + 1e-300))


def max_pool(a: torch.Tensor) -> torch.Tensor:
    """MaxPool(kernel_size=2, stride=2) of a's rank, torch's default floor mode"""
    return F.max_pool1d(a, 2, 2) if a.dim() == 3 else F.max_pool2d(a, 2, 2)


def tanh_pool(z: torch.Tensor, scale=None, shift=None):
    """(act, pooled) of tanh(scale z + shift), per-channel scale / shift"""
    shape = (1, -1) + (1,) * (z.dim() - 2)
    y = z if scale is None else z * scale.view(shape) + shift.view(shape)
    act = torch.tanh(y)
    return act, max_pool(act)


def upconv(x: torch.Tensor, w: torch.Tensor, b=None) -> torch.Tensor:
    """ConvTranspose(kernel_size=2, stride=2) of x's rank"""
    return F.conv_transpose1d(x, w, b, stride=2) if x.dim() == 3 else F.conv_transpose2d(x, w, b, stride=2)


def batchnorm_tanh(z, weight, bias, running_mean, running_var, training: bool, momentum: float = 0.1, eps: float = 1e-5):
    """tanh(BatchNorm(z)); updates the running buffers in place in training mode, as F.batch_norm does"""
    return torch.tanh(F.batch_norm(z, running_mean, running_var, weight, bias, training, momentum, eps))


def groupnorm_tanh(z, num_groups: int, weight, bias, eps: float = 1e-5):
    return torch.tanh(F.group_norm(z, num_groups, weight, bias, eps))


def loss_of(act, pooled, g_act, g_pool):
    """the scalar whose gradient feeds (g_act, g_pool) into the two outputs; either may be None: that output is unused"""
    total = 0.0
    if g_act is not None:
        total = total + (act * g_act).sum()
    if g_pool is not None:
        total = total + (pooled * g_pool).sum()
    return total
