"""The Convolutional Neural Operator's module tree, written once for both ranks (reference models/CNO1d.py and
models/CNO2d.py, which differ in `1d` / `2d` alone; Raonic et al., "Convolutional Neural Operators for robust and
accurate learning of PDEs", NeurIPS 2023): an operator U-Net whose every activation is applied at twice the sampling
rate between two antialiased resamplings, so that the nonlinearity does not alias.

The classes, constructor signatures, attribute names and state_dict layout are the reference's -- nn.Conv1d / nn.Conv2d
and nn.BatchNorm1d / nn.BatchNorm2d own the parameters and buffers, so a reference checkpoint loads with strict=True --
but no forward here calls an ATen kernel for arithmetic: convolutions, BatchNorm and the activation run in
librpde_hip.so (rpde.ops conv*_k3, batchnorm*, cno_act*).  Where a BatchNorm precedes the activation its apply step is
the activation kernel's prologue and the normalised tensor is never written.  torch.cat stays torch's: it is a copy.

Nothing here is instantiated directly.  models/CNO1d.py and models/CNO2d.py subclass every class below and give each
subclass its rank (`nd`, a Rank) and the classes of its own rank that it builds its children from, as class attributes:
the two ranks stay distinct classes that live, pickle and print under their own module.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Type

import torch
import torch.nn as nn

from rpde import ops


class Rank(NamedTuple):
    """what differs between the ranks: torch's parameter-owning layers and the rpde.ops that compute with them"""
    Conv: Type[nn.Module]
    BatchNorm: Type[nn.Module]
    conv_k3: Callable
    batchnorm: Callable
    cno_act: Callable

    def conv(self, layer, x):
        return self.conv_k3(x, layer.weight, layer.bias)

    def norm(self, bn, z, residual=None, act=None):
        """BatchNorm bn on z, then the skip add or CNO_LReLu(*act); bn may be nn.Identity (use_bn=False)"""
        if isinstance(bn, nn.Identity):
            if act is not None:
                return self.cno_act(z, act[0], act[1])
            return z if residual is None else ops.skip_add(z, residual)
        momentum = 0.1 if bn.momentum is None else bn.momentum
        return self.batchnorm(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.training,
                              momentum, bn.eps, residual=residual, act=act)


RANK = {1: Rank(nn.Conv1d, nn.BatchNorm1d, ops.conv1d_k3, ops.batchnorm1d, ops.cno_act1d),
        2: Rank(nn.Conv2d, nn.BatchNorm2d, ops.conv2d_k3, ops.batchnorm2d, ops.cno_act2d)}


class CNO_LReLu(nn.Module):
    """upsample to 2 in_size -> LeakyReLU -> downsample to out_size, one kernel (rpde.ops.cno_act1d / cno_act2d)"""
    nd: Rank

    def __init__(self, in_size, out_size):
        super().__init__()
        self.in_size, self.out_size = in_size, out_size
        self.act = nn.LeakyReLU()

    def forward(self, x):
        return self.nd.cno_act(x, self.in_size, self.out_size, slope=self.act.negative_slope)


class CNOBlock(nn.Module):
    """Conv(k=3) -> BatchNorm (optional) -> CNO_LReLu; the resampling in_size -> out_size happens in the activation"""
    nd: Rank
    CNO_LReLu: Type[CNO_LReLu]

    def __init__(self, in_channels, out_channels, in_size, out_size, use_bn=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.in_size, self.out_size = in_size, out_size
        self.convolution = self.nd.Conv(in_channels, out_channels, kernel_size=3, padding=1)
        self.batch_norm = self.nd.BatchNorm(out_channels) if use_bn else nn.Identity()
        self.act = self.CNO_LReLu(in_size=in_size, out_size=out_size)

    def forward(self, x):
        return self.nd.norm(self.batch_norm, self.nd.conv(self.convolution, x), act=(self.in_size, self.out_size))


class LiftProjectBlock(nn.Module):
    nd: Rank
    CNOBlock: Type[CNOBlock]

    def __init__(self, in_channels, out_channels, size, latent_dim=64):
        super().__init__()
        self.inter_CNOBlock = self.CNOBlock(in_channels, latent_dim, in_size=size, out_size=size, use_bn=False)
        self.convolution = self.nd.Conv(latent_dim, out_channels, kernel_size=3, padding=1)

    def forward(self, x):
        return self.nd.conv(self.convolution, self.inter_CNOBlock(x))


class ResidualBlock(nn.Module):
    """x + BN2(Conv2(CNO_LReLu(BN1(Conv1(x)))))"""
    nd: Rank
    CNO_LReLu: Type[CNO_LReLu]

    def __init__(self, channels, size, use_bn=True):
        super().__init__()
        self.channels, self.size = channels, size
        self.convolution1 = self.nd.Conv(channels, channels, kernel_size=3, padding=1)
        self.convolution2 = self.nd.Conv(channels, channels, kernel_size=3, padding=1)
        self.batch_norm1 = self.nd.BatchNorm(channels) if use_bn else nn.Identity()
        self.batch_norm2 = self.nd.BatchNorm(channels) if use_bn else nn.Identity()
        self.act = self.CNO_LReLu(in_size=size, out_size=size)

    def forward(self, x):
        nd = self.nd
        out = nd.norm(self.batch_norm1, nd.conv(self.convolution1, x), act=(self.size, self.size))
        return nd.norm(self.batch_norm2, nd.conv(self.convolution2, out), residual=x)


class ResNet(nn.Module):
    ResidualBlock: Type[ResidualBlock]

    def __init__(self, channels, size, num_blocks, use_bn=True):
        super().__init__()
        self.channels, self.size, self.num_blocks = channels, size, num_blocks
        self.res_nets = nn.Sequential(*[self.ResidualBlock(channels, size, use_bn) for _ in range(num_blocks)])

    def forward(self, x):
        return self.res_nets(x)


class CNO(nn.Module):
    """in_dim / out_dim channels on `size` points per axis; N_layers down- and up-sampling levels, N_res residual blocks
    per level and N_res_neck in the neck; level i has channel_multiplier 2^(i-1) channels on size / 2^i points per axis.
    Inputs of another size are resampled by the first activation (F.interpolate(size=...) in the reference does the
    same)."""
    LiftProjectBlock: Type[LiftProjectBlock]
    CNOBlock: Type[CNOBlock]
    ResNet: Type[ResNet]

    def __init__(self, in_dim, out_dim, size, N_layers, N_res=4, N_res_neck=4, channel_multiplier=16, use_bn=True):
        super().__init__()
        self.N_layers = int(N_layers)
        self.lift_dim = channel_multiplier // 2
        self.in_dim, self.out_dim = in_dim, out_dim
        self.channel_multiplier = channel_multiplier
        L = self.N_layers
        LiftProjectBlock, CNOBlock, ResNet = self.LiftProjectBlock, self.CNOBlock, self.ResNet

        self.encoder_features = [self.lift_dim] + [2 ** i * channel_multiplier for i in range(L)]
        self.decoder_features_in = self.encoder_features[1:][::-1]
        self.decoder_features_out = self.encoder_features[:-1][::-1]
        for i in range(1, L):                      # the skip connection is concatenated in front of every (U) block but the first
            self.decoder_features_in[i] *= 2
        self.encoder_sizes = [size // 2 ** i for i in range(L + 1)]
        self.decoder_sizes = [size // 2 ** (L - i) for i in range(L + 1)]

        enc, dec_in, dec_out = self.encoder_features, self.decoder_features_in, self.decoder_features_out
        self.lift = LiftProjectBlock(in_dim, enc[0], size)
        self.project = LiftProjectBlock(enc[0] + dec_out[-1], out_dim, size)
        self.encoder = nn.ModuleList([CNOBlock(enc[i], enc[i + 1], self.encoder_sizes[i], self.encoder_sizes[i + 1], use_bn)
                                      for i in range(L)])
        self.ED_expansion = nn.ModuleList([CNOBlock(enc[i], enc[i], self.encoder_sizes[i], self.decoder_sizes[L - i], use_bn)
                                           for i in range(L + 1)])
        self.decoder = nn.ModuleList([CNOBlock(dec_in[i], dec_out[i], self.decoder_sizes[i], self.decoder_sizes[i + 1], use_bn)
                                      for i in range(L)])
        self.N_res, self.N_res_neck = int(N_res), int(N_res_neck)
        # (built before the neck, registered after it: the reference's order of random draws and of state_dict keys)
        levels = [ResNet(enc[i], self.encoder_sizes[i], self.N_res, use_bn) for i in range(L)]
        self.res_net_neck = ResNet(enc[L], self.encoder_sizes[L], self.N_res_neck, use_bn)
        self.res_nets = nn.Sequential(*levels)

    def forward(self, x):
        L = self.N_layers
        x = self.lift(x)
        skip = []
        for i in range(L):                         # encoder: the level's ResNet feeds the skip, the (D) block goes down
            skip.append(self.res_nets[i](x))
            x = self.encoder[i](x)
        x = self.res_net_neck(x)
        for i in range(L):                         # decoder: (I) block on the neck / on the skip, concatenated, then (U)
            if i == 0:
                x = self.ED_expansion[L](x)
            else:
                x = torch.cat((x, self.ED_expansion[L - i](skip[-i])), 1)
            x = self.decoder[i](x)
        x = torch.cat((x, self.ED_expansion[0](skip[0])), 1)
        return self.project(x)
