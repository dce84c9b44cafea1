"""The PDEBench U-Net in 1-D and 2-D (reference models/unet.py; Takamoto et al., "PDEBench: An Extensive Benchmark for
Scientific Machine Learning", NeurIPS 2022): four encoder levels of Conv(k=3) -> norm -> tanh twice with MaxPool(2)
between them, a bottleneck, and four decoder levels of ConvTranspose(k=2, stride=2), skip concatenation and the same
block, closed by a 1 x 1 convolution.

The constructor signatures, attribute names and state_dict layout are the reference's -- nn.Conv*, nn.BatchNorm* /
nn.GroupNorm and nn.ConvTranspose* own the parameters and buffers inside the same nn.Sequential(OrderedDict) blocks, in
the reference's order of registration and of random draws, so a reference checkpoint loads with strict=True -- but no
forward here calls an ATen kernel for arithmetic: the convolutions, the norm, tanh and the pooling run in
librpde_hip.so (rpde.ops conv*_k3, norm_tanh / groupnorm_tanh, upconv*, conv1x1).  The norm's apply step, tanh and an
encoder level's MaxPool are one kernel: the block's last activation is written once, together with its pooled copy.
torch.cat stays torch's: it is a copy.

One tree serves both ranks: UNet1d and UNet2d give it their rank (`nd`) as a class attribute, the way models/cno_nd.py
binds its ranks.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Callable, NamedTuple, Type

import torch
import torch.nn as nn

from rpde import ops


class Rank(NamedTuple):
    """what differs between the ranks: torch's parameter-owning layers and the rpde.ops that compute with them"""
    Conv: Type[nn.Module]
    BatchNorm: Type[nn.Module]
    ConvTranspose: Type[nn.Module]
    MaxPool: Type[nn.Module]
    conv_k3: Callable
    upconv: Callable


RANK = {1: Rank(nn.Conv1d, nn.BatchNorm1d, nn.ConvTranspose1d, nn.MaxPool1d, ops.conv1d_k3, ops.upconv1d),
        2: Rank(nn.Conv2d, nn.BatchNorm2d, nn.ConvTranspose2d, nn.MaxPool2d, ops.conv2d_k3, ops.upconv2d)}

LEVELS = 4


def _norm_tanh(norm: nn.Module, z: torch.Tensor, pool: bool = False):
    if isinstance(norm, nn.GroupNorm):
        return ops.groupnorm_tanh(z, norm.num_groups, norm.weight, norm.bias, norm.eps, pool=pool)
    return ops.norm_tanh(z, norm, pool=pool)


class _UNet(nn.Module):
    nd: Rank

    def __init__(self, in_channels=3, out_channels=1, width=32, use_groupnorm=False):
        super().__init__()
        nd, f = self.nd, width
        for i in range(1, LEVELS + 1):              # encoder1, pool1, ..., encoder4, pool4
            setattr(self, f"encoder{i}", self._block(in_channels if i == 1 else f * 2 ** (i - 2), f * 2 ** (i - 1), f"enc{i}",
                                                     use_groupnorm))
            setattr(self, f"pool{i}", nd.MaxPool(kernel_size=2, stride=2))
        self.bottleneck = self._block(f * 8, f * 16, "bottleneck", use_groupnorm)
        for i in range(LEVELS, 0, -1):              # upconv4, decoder4, ..., upconv1, decoder1
            c = f * 2 ** (i - 1)
            setattr(self, f"upconv{i}", nd.ConvTranspose(2 * c, c, kernel_size=2, stride=2))
            setattr(self, f"decoder{i}", self._block(2 * c, c, f"dec{i}", use_groupnorm))
        self.conv = nd.Conv(in_channels=f, out_channels=out_channels, kernel_size=1)

    @classmethod
    def _block(cls, in_channels, features, name, use_groupnorm=False):
        nd = cls.nd

        def norm():                                 # GroupNorm with 8 groups, or fewer if features < 8
            return nn.GroupNorm(num_groups=min(8, features), num_channels=features) if use_groupnorm else nd.BatchNorm(num_features=features)

        norm1, norm2 = norm(), norm()
        return nn.Sequential(OrderedDict([
            (name + "conv1", nd.Conv(in_channels, features, kernel_size=3, padding=1, bias=False)),
            (name + "norm1", norm1),
            (name + "tanh1", nn.Tanh()),
            (name + "conv2", nd.Conv(features, features, kernel_size=3, padding=1, bias=False)),
            (name + "norm2", norm2),
            (name + "tanh2", nn.Tanh()),
        ]))

    def _run(self, block: nn.Sequential, x: torch.Tensor, pool: bool = False):
        """conv_k3 -> norm_tanh -> conv_k3 -> norm_tanh(pool): the activation, and with pool its MaxPool(2) as well"""
        conv1, norm1, _, conv2, norm2, _ = block
        h = _norm_tanh(norm1, self.nd.conv_k3(x, conv1.weight, conv1.bias))
        return _norm_tanh(norm2, self.nd.conv_k3(h, conv2.weight, conv2.bias), pool=pool)

    def forward(self, x):
        for size in x.shape[2:]:
            if size % 2 ** LEVELS:
                raise ValueError(f"{type(self).__name__}: the spatial sizes must be multiples of {2 ** LEVELS} (four "
                                 f"MaxPool(2) levels and their skip connections), got {size} in input size {tuple(x.shape)}")
        skips = []
        for i in range(1, LEVELS + 1):
            skip, x = self._run(getattr(self, f"encoder{i}"), x, pool=True)
            skips.append(skip)
        x = self._run(self.bottleneck, x)
        for i in range(LEVELS, 0, -1):
            up = getattr(self, f"upconv{i}")
            x = torch.cat((self.nd.upconv(x, up.weight, up.bias), skips[i - 1]), dim=1)
            x = self._run(getattr(self, f"decoder{i}"), x)
        return ops.conv1x1(x, self.conv.weight, self.conv.bias)


class UNet1d(_UNet):
    """in_channels -> out_channels on [B, C, n], n a multiple of 16; level i has width 2^(i-1) channels on n / 2^(i-1)
    points.  use_groupnorm: GroupNorm(min(8, channels)) in place of BatchNorm1d."""
    nd = RANK[1]


class UNet2d(_UNet):
    """in_channels -> out_channels on [B, C, H, W], H and W multiples of 16, BatchNorm2d"""
    nd = RANK[2]

    def __init__(self, in_channels=3, out_channels=1, width=32):
        super().__init__(in_channels, out_channels, width)
