"""Restatement of the counter-hash dropout masks (``resolution-pde_amd/csrc/drop_hash.h``).

TEST INFRASTRUCTURE ONLY (see ``oracle/__init__.py``).  numpy ``uint64`` / ``uint32`` arithmetic, so that the masks
of any kernel call can be rebuilt off the device and fed to the float64 oracle (``reference_path.feedforward`` and
the FFNO wrappers take them as an argument).  It restates the kernels as they are, quirks included:

- the drop probability is a float32 (``rpde_ff_params.dropout_p``); its threshold is quantised to 16 bits,
  ``thresh = floor(p * 65536 + 0.5)`` clamped to [1, 65535] (p <= 0: no mask at all);
- the keep factor is ``float32(1 / (1 - thresh / 65536))``, not ``1 / (1 - p)``;
- the device epoch counter is folded in as ``seed ^= epoch * 0x9E3779B97F4A7C15`` (mod 2^64);
- ids 4g .. 4g+3 share one base word, and each 32-bit hash gives two 16-bit uniforms.

Element ids are ``point * out_features + feature``; layer ``l`` of a FeedForward call with seed ``s`` uses
``layer_seed(s, l)``.  Verified bit for bit against the header by ``tests/test_oracle_dropout_cpu.py``.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np
import torch

M64 = (1 << 64) - 1
GOLDEN64 = 0x9E3779B97F4A7C15
SALT = 0x68E31DA4


def layer_seed(seed: int, layer: int) -> int:
    """splitmix64 finaliser of seed + (layer + 1) * golden ratio (drop_hash.h: layer_seed)"""
    z = (seed + GOLDEN64 * (layer + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def resolve(seed: int, epoch: int) -> int:
    """the seed with the device epoch counter folded in (drop_hash.h: drop_resolve)"""
    return (seed ^ ((epoch & M64) * GOLDEN64)) & M64


def threshold(p: float) -> int:
    """16-bit drop threshold of probability p (drop_hash.h: make_drop); 0 = dropout off"""
    p32 = float(np.float32(p))
    if p32 <= 0.0:
        return 0
    t = int(np.floor(p32 * 65536.0 + 0.5))
    return min(max(t, 1), 65535)


def scale(p: float) -> float:
    """the keep factor the kernels multiply by: float32(1 / (1 - thresh / 65536)); 1 when dropout is off"""
    t = threshold(p)
    if t == 0:
        return 1.0
    return float(np.float32(1.0 / (1.0 - t / 65536.0)))


def _mix32(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def uniforms(seed: int, epoch: int, ids) -> np.ndarray:
    """the 16-bit uniform (uint32 array) each element id is compared with, for an already layer-derived seed"""
    s = resolve(seed, epoch)
    ids = np.asarray(ids, dtype=np.uint64)
    with np.errstate(over="ignore"):
        group = ids >> np.uint64(2)
        lo = (group & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        hi = (group >> np.uint64(32)).astype(np.uint32)
        base = (lo ^ np.uint32(s & 0xFFFFFFFF)) + ((hi * np.uint32(0x9E3779B9)) ^ np.uint32(s >> 32))
        second = (ids & np.uint64(2)) != 0
        h = _mix32(np.where(second, base ^ np.uint32(SALT), base))
        odd = (ids & np.uint64(1)) != 0
        return np.where(odd, h >> np.uint32(16), h & np.uint32(0xFFFF)).astype(np.uint32)


def keep(seed: int, epoch: int, p: float, ids) -> np.ndarray:
    """bool array: element kept (seed already layer-derived)"""
    return uniforms(seed, epoch, ids) >= threshold(p)


def factor(seed: int, epoch: int, p: float, ids) -> np.ndarray:
    """float64 factor per element id: 0 (dropped) or scale(p) (kept); ones when dropout is off"""
    ids = np.asarray(ids, dtype=np.uint64)
    if threshold(p) == 0:
        return np.ones(ids.shape, dtype=np.float64)
    return np.where(keep(seed, epoch, p, ids), scale(p), 0.0)


def layer_mask(seed: int, layer: int, epoch: int, p: float, points: int, out_features: int,
               id_offset: int = 0) -> torch.Tensor:
    """float64 [points, out_features] factor of layer `layer` of a FeedForward call that drew `seed`
    (ids point * out_features + feature, shifted by id_offset)"""
    ids = (np.arange(points, dtype=np.uint64)[:, None] * np.uint64(out_features)
           + np.arange(out_features, dtype=np.uint64)[None, :] + np.uint64(id_offset))
    return torch.from_numpy(factor(layer_seed(seed, layer), epoch, p, ids))


def feedforward_masks(seed: int, epoch: int, p: float, points: int, dim: int, factor_: int,
                      n_layers: int) -> List[torch.Tensor]:
    """the masks of every layer of one FeedForward call: [points, dim*factor] for hidden layers, [points, dim] last"""
    outs: Sequence[int] = [dim * factor_] * (n_layers - 1) + [dim]
    return [layer_mask(seed, l, epoch, p, points, o) for l, o in enumerate(outs)]
