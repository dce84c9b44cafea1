"""Error decomposition by frequency (reference: utils/frequency_error.py, driven by frequency_evaluation.py and
utils/multiresolution_analysis.py): WHERE in the spectrum a model is wrong -- error and solution magnitude per Fourier
mode (1-D) or per radial frequency bin (2-D).

The reference reconstructs every mode / bin with an inverse FFT of the whole batch and takes its norm on the host.  By
Parseval that norm is the weighted energy of the retained modes, so here a batch is ONE fused device call
(rpde.ops.freq_energy1d / freq_energy2d) that adds into a float64 accumulator; a test set streams through in batches,
with one device-to-host copy at the end.  One deliberate difference: the error is formed as ``pred - target`` in fp32
BEFORE the transform (the reference subtracts two fp32 spectra and loses digits as the model gets better).  The
reference's plots and Gaussian smoothing are not carried over: the numbers are returned."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch


def decompose_error_by_frequency_1d(y_hat: torch.Tensor, y: torch.Tensor, num_modes: Optional[int] = None):
    """y_hat, y [B, C, H] -> (error_per_mode, solution_magnitude_per_mode, frequencies), numpy [num_modes]: the
    magnitudes float64, the frequencies float32 as torch.fft.rfftfreq gives them (and the reference returns them)"""
    fe = FrequencyError(dims=1, num_modes=num_modes)
    fe.update(y_hat, y)
    return fe.compute()


def decompose_error_by_frequency_2d(y_hat: torch.Tensor, y: torch.Tensor, num_radial_bins: int = 64):
    """y_hat, y [B, C, H, W] -> (error_per_bin, solution_magnitude_per_bin, radial_freqs), numpy float64
    [num_radial_bins]"""
    fe = FrequencyError(dims=2, num_radial_bins=num_radial_bins)
    fe.update(y_hat, y)
    return fe.compute()


class FrequencyError:
    """Streaming accumulator: ``update(pred, target)`` per batch (no host synchronisation; after one eager call at a
    grid size it can be captured in a ``torch.cuda.graph``), ``compute()`` once, ``reset()`` to start over.  One
    accumulator serves one grid size."""

    def __init__(self, dims: int, num_modes: Optional[int] = None, num_radial_bins: int = 64, channels_last: bool = False):
        if dims not in (1, 2):
            raise ValueError(f"FrequencyError: dims must be 1 or 2, got {dims}")
        self.dims, self.num_modes, self.num_radial_bins, self.channels_last = dims, num_modes, int(num_radial_bins), channels_last
        self.acc: Optional[torch.Tensor] = None
        self.grid: Optional[Tuple[int, ...]] = None

    def _grid_of(self, t: torch.Tensor) -> Tuple[int, ...]:
        return tuple(t.shape[1:-1]) if self.channels_last else tuple(t.shape[2:])

    def update(self, pred: torch.Tensor, target: torch.Tensor) -> None:
        from rpde import ops
        if pred.dim() != self.dims + 2:
            raise ValueError(f"FrequencyError({self.dims}-D): expected a {self.dims + 2}-D batch, got {tuple(pred.shape)}")
        grid = self._grid_of(pred)
        if self.grid is None:
            self.grid = grid
        elif grid != self.grid:
            raise ValueError(f"FrequencyError: grid {grid} after {self.grid}: one accumulator per grid size")
        if self.dims == 1:
            self.acc = ops.freq_energy1d(pred, target, acc=self.acc, num_modes=self.num_modes, channels_last=self.channels_last)
        else:
            self.acc = ops.freq_energy2d(pred, target, num_radial_bins=self.num_radial_bins, acc=self.acc,
                                         channels_last=self.channels_last)

    def frequencies(self) -> np.ndarray:
        if self.grid is None:
            raise RuntimeError("FrequencyError: no batch seen")
        if self.dims == 1:
            return torch.fft.rfftfreq(self.grid[0]).numpy()[:self.acc.shape[1]]
        from rpde.ops import radial_bins
        return np.array(radial_bins(self.grid[0], self.grid[1], self.num_radial_bins)[1])

    def compute(self):
        """(error, solution, frequencies) as the reference returns them; the one device-to-host copy"""
        if self.acc is None:
            raise RuntimeError("FrequencyError: no batch seen")
        amp = torch.sqrt(self.acc).cpu().numpy()
        return amp[0], amp[1], self.frequencies()

    def reset(self) -> None:
        """zero the accumulator in place (a captured ``update`` keeps pointing at it); the grid size stays"""
        if self.acc is not None:
            self.acc.zero_()


@torch.no_grad()
def evaluate_frequency_error(model, test_x: torch.Tensor, test_y: torch.Tensor, resolutions: Optional[List[int]] = None,
                             how: str = "naive_downsample", batch_size: int = 16, num_modes: Optional[int] = None,
                             num_radial_bins: int = 64, x_encode: Optional[Callable] = None,
                             y_decode: Optional[Callable] = None, device="cuda") -> Dict[int, tuple]:
    """{resolution: (error, solution, frequencies)} of the model over the test fields [N, C, n] / [N, C, M, N] at every
    resolution of ``resolutions`` (default: [32, .., full], as utils.resize_utils.evaluate_all_resolutions); encode /
    decode are the x / y normalisers.  With torch.distributed initialised every rank takes samples rank, rank + world,
    ... and the accumulators are summed by one all_reduce."""
    import torch.distributed as dist
    from rpde.ops import frozen_weights
    from utils.resize_utils import get_lower_resolutions, to_resolution
    on = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    rank, world = (dist.get_rank(), dist.get_world_size()) if on else (0, 1)
    model.eval()
    dims = test_x.dim() - 2
    full = int(test_x.shape[-1])
    mine_x, mine_y = test_x[rank::world], test_y[rank::world]
    resolutions = [int(r) for r in (resolutions or get_lower_resolutions(full, min(32, full)))]
    meters = []
    with frozen_weights():
        for res in resolutions:
            fe = FrequencyError(dims, num_modes=num_modes, num_radial_bins=num_radial_bins)
            n_out = (min(num_modes or res // 2 + 1, res // 2 + 1)) if dims == 1 else int(num_radial_bins)
            fe.acc = torch.zeros(2, n_out, dtype=torch.float64, device=device)      # a rank without samples still reduces
            fe.grid = (res,) * dims
            for i in range(0, mine_x.shape[0], batch_size):
                x = to_resolution(mine_x[i:i + batch_size].to(device), res, how)
                y = to_resolution(mine_y[i:i + batch_size].to(device), res, how)
                pred = model(x_encode(x) if x_encode else x)
                if y_decode:
                    pred = y_decode(pred)
                fe.update(pred, y)
            meters.append(fe)
    if on:
        flat = torch.cat([m.acc.reshape(-1) for m in meters])
        if dist.get_backend() == "gloo":            # gloo reduces host tensors
            host = flat.cpu()
            dist.all_reduce(host)
            flat = host.to(flat.device)
        else:
            dist.all_reduce(flat)
        o = 0
        for m in meters:
            m.acc.copy_(flat[o:o + m.acc.numel()].view_as(m.acc))
            o += m.acc.numel()
    return {res: m.compute() for res, m in zip(resolutions, meters)}
