"""FFNO1D / FFNO2D (reference: models/ffno.py:25-237): (grid) -> in_proj ->
n_layers x [x + FSpectralConv(x)] -> out_proj, channels-last inside.

The grid channels are generated on device inside the lifting kernel (the
reference rebuilds them with numpy on the host every forward) and the skip
connection is fused into the FeedForward tail kernel."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from models.custom_layer import WNLinear
from models.spectral_convolution import FSpectralConv1d, FSpectralConv2d
from rpde import ops


def _coord(c, device):
    if not isinstance(c, torch.Tensor):
        c = torch.tensor(c, dtype=torch.float)
    return c.to(device=device, dtype=torch.float32).contiguous()


class FFNO1D(nn.Module):
    def __init__(self, in_channels, out_channels, width=64, n_layers=4, n_modes=16, factor=4, ff_weight_norm=False,
                 n_ff_layers=2, layer_norm=False, dropout=0.0, grid=None, mode="full", fft_norm="ortho",
                 activation="identity", use_grid=True):
        super().__init__()
        self.in_channels, self.out_channels, self.hidden_dim = in_channels, out_channels, width
        self.n_layers, self.n_modes, self.grid = n_layers, n_modes, grid
        # The reference assigns ``self.use_grid = grid``: the grid
        # channel exists only when a (list / ndarray) grid is supplied.
        self.use_grid = grid
        lifted = in_channels + 1 if self.use_grid else in_channels
        self.in_proj = WNLinear(lifted, width, wnorm=ff_weight_norm)
        self.fourier_layers = nn.ModuleList([
            FSpectralConv1d(width, n_modes, factor=factor, ff_weight_norm=ff_weight_norm, n_ff_layers=n_ff_layers,
                            layer_norm=layer_norm, dropout=dropout, mode=mode, fft_norm=fft_norm, activation=activation)
            for _ in range(n_layers)])
        self.out_proj = WNLinear(width, out_channels, wnorm=ff_weight_norm)

    def get_grid(self, batch_size, seq_length, device):
        g = _coord(self.grid, device) if self.grid is not None else torch.tensor(
            np.linspace(0, 1, seq_length), dtype=torch.float).to(device)
        return g.reshape(1, seq_length, 1).repeat([batch_size, 1, 1])

    def forward(self, x):
        if self.use_grid:
            h = ops.concat_grid(x, 1, 0.0, 1.0, channels_last=True, gridx=_coord(self.grid, x.device))
        else:
            h = ops.to_channels_last(x)
        h = self.in_proj(h)
        for layer in self.fourier_layers:
            h, _ = layer(h, residual=h)          # x + layer(x)[0], skip fused into the FF tail
        return ops.to_channels_first(self.out_proj(h))


class FFNO2D(nn.Module):
    def __init__(self, in_channels, out_channels, width=64, n_layers=4, n_modes=16, factor=4, ff_weight_norm=False,
                 n_ff_layers=2, layer_norm=False, grid=None, dropout=0.0, mode="full", use_grid=True):
        super().__init__()
        self.in_channels, self.out_channels, self.hidden_dim = in_channels, out_channels, width
        self.n_layers, self.n_modes, self.ff_weight_norm = n_layers, n_modes, ff_weight_norm
        self.grid, self.use_grid = grid, use_grid
        lifted = in_channels + 2 if use_grid else in_channels
        # plain nn.Linear keys (``weight``) without weight norm, ``weight_g/_v`` with it (quirk Q2)
        self.in_proj = WNLinear(lifted, width, wnorm=True) if ff_weight_norm else nn.Linear(lifted, width)
        self.fourier_layers = nn.ModuleList([
            FSpectralConv2d(width, n_modes, factor=factor, ff_weight_norm=ff_weight_norm, n_ff_layers=n_ff_layers,
                            layer_norm=layer_norm, dropout=dropout, mode=mode)
            for _ in range(n_layers)])
        self.out_proj = WNLinear(width, out_channels, wnorm=True) if ff_weight_norm else nn.Linear(width, out_channels)

    def get_grid(self, shape, device):
        b, m, n = shape[0], shape[1], shape[2]
        if self.grid is not None:
            gx, gy = _coord(self.grid[0], device), _coord(self.grid[1], device)
        else:
            gx = torch.tensor(np.linspace(0, 1, m), dtype=torch.float).to(device)
            gy = torch.tensor(np.linspace(0, 1, n), dtype=torch.float).to(device)
        gx = gx.reshape(1, m, 1, 1).repeat([b, 1, n, 1])
        gy = gy.reshape(1, 1, n, 1).repeat([b, m, 1, 1])
        return torch.cat((gx, gy), dim=-1)

    @staticmethod
    def _apply_linear(mod, h):
        if isinstance(mod, WNLinear):
            return mod(h)
        return ops.linear(h, mod.weight, mod.bias)

    def _lifted_first_layer(self, u, w_in):
        """Whether the first layer's spectral branch runs on the unlifted input u (ops.lifted_fspectral2d): the lifting
        is a pointwise linear map, which commutes with the DFT, so it folds into the layer's mode-mix weights.  Needs
        the full mode mix, a shape of the fused 2-D path, gradients enabled (evaluation keeps the path it can prepare
        once, ops.frozen_weights) and an input that asks for none (the branch then feeds weights only);
        RPDE_LIFTED_SPECTRAL=0 keeps the 64-channel path."""
        if len(self.fourier_layers) == 0 or self.fourier_layers[0].mode != "full":
            return False
        if not isinstance(self.in_proj, nn.Linear) or u.requires_grad:
            return False
        return ops.lifted_fspectral2d_ok(u, w_in, self.n_modes)

    def forward(self, x):
        if self.use_grid:
            gx = gy = None
            if self.grid is not None:
                gx, gy = _coord(self.grid[0], x.device), _coord(self.grid[1], x.device)
            h = ops.concat_grid(x, 2, 0.0, 1.0, channels_last=True, gridx=gx, gridy=gy)
        else:
            h = ops.to_channels_last(x)
        # the effective lifting weight once (weight norm's own autograd carries both uses back to weight_g / weight_v)
        w_in = self.in_proj.effective_weight() if isinstance(self.in_proj, WNLinear) else self.in_proj.weight
        u, h = h, ops.linear(h, w_in, self.in_proj.bias)
        lifted = self._lifted_first_layer(u, w_in)
        for i, layer in enumerate(self.fourier_layers):
            if i == 0 and lifted:
                fw = layer.fourier_weight
                s = ops.lifted_fspectral2d(u, w_in, self.in_proj.bias, fw[0], fw[1], layer.n_modes)
                h, _ = layer(h, residual=h, spectral=s)
            else:
                h, _ = layer(h, residual=h)
        return ops.to_channels_first(self._apply_linear(self.out_proj, h))
