"""Active-matter style trajectories (a concentration and a two-component velocity) -> single-step (Markov) training
pairs with min-max statistics.  Same public names, arguments and seven return values as the reference's
dataloaders/active_matter_markov.py (ActiveMatterMarkovDataset :11-161, active_matter_markov_dataset :164-258).

One file with the members ``t0_fields/concentration`` [n, T, H, W] and ``t1_fields/velocity`` [n, T, H, W, 2], opened
through dataloaders/_store.Store: ``.hdf5`` / ``.h5`` when h5py is importable, ``.npz`` with the same member names
otherwise -- what data_generation/active_scalar_2d.py writes.  The target size ``s`` resizes every (sample, time,
channel) image once at load time: utils.res_utils.downsample on the host for s < H, utils.res_utils.resize on the GPU
for s > H.  The reference imports h5py at module level, so this loader is not pinned against it;
``downsample`` itself is (tests/golden/downsample2d.npz)."""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset, random_split

from dataloaders._store import Store

CONCENTRATION, VELOCITY = "t0_fields/concentration", "t1_fields/velocity"
RESIZE_CHUNK = 1024                       # images per device resize call


def read_member(f, key: str, path: str) -> np.ndarray:
    """member `key` ('/' separates groups) of an open Store as float32; KeyError names the file when it is missing"""
    node = f
    try:
        for part in key.split("/"):
            node = node[part]
    except KeyError:
        raise KeyError(f"'{key}' not found in {path}. Available keys: {list(f.keys())}") from None
    return np.array(node, dtype=np.float32)


def read_scalar(f, key: str):
    """scalar member `key` as a float, or None when the file has none"""
    node = f
    for part in key.split("/"):
        if part not in node:
            return None
        node = node[part]
    return float(np.asarray(node[()]).reshape(-1)[0])


def combine(concentration: np.ndarray, velocity: np.ndarray) -> np.ndarray:
    """[n, T, H, W] and [n, T, H, W, 2] -> [n, T, H, W, 3], the concentration in front"""
    return np.concatenate([concentration[..., None], velocity], axis=-1)


def resize_frames(data: np.ndarray, s: Optional[int]) -> np.ndarray:
    """data [n, T, H, W, C] -> [n, T, s, s, C], every (sample, time, channel) image on its own; s None or H: unchanged"""
    n, T, H, W, C = data.shape
    if s is None or int(s) == H:
        return data
    s = int(s)
    images = np.ascontiguousarray(data.transpose(0, 1, 4, 2, 3)).reshape(n * T * C, 1, H, W)
    if s < H:
        from utils.res_utils import downsample
        out = downsample(images, s)
    else:
        from utils.res_utils import resize
        dev = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")    # the op refuses CPU tensors
        out = np.empty((images.shape[0], 1, s, s), dtype=np.float32)
        for i in range(0, images.shape[0], RESIZE_CHUNK):
            chunk = torch.from_numpy(images[i:i + RESIZE_CHUNK]).to(dev)
            out[i:i + RESIZE_CHUNK] = resize(chunk, (s, s)).cpu().numpy()
    return np.ascontiguousarray(out.reshape(n, T, C, s, s).transpose(0, 1, 3, 4, 2))


def markov_pairs(data: np.ndarray) -> Tuple[torch.Tensor, torch.Tensor]:
    """data [n, T, H, W, C] -> x = frames[:-1], y = frames[1:], each flattened to [(n (T-1)), C, H, W]"""
    u = torch.from_numpy(np.ascontiguousarray(data)).float().permute(0, 1, 4, 2, 3)
    x, y = u[:, :-1], u[:, 1:]
    return x.reshape(-1, *x.shape[2:]).contiguous(), y.reshape(-1, *y.shape[2:]).contiguous()


def unit_grid(h: int, w: int) -> torch.Tensor:
    """[h, w, 2]: the points linspace(0, 1) of both axes, x first"""
    xx, yy = np.meshgrid(np.linspace(0, 1, w), np.linspace(0, 1, h))
    return torch.tensor(np.stack([xx, yy], axis=-1), dtype=torch.float)


class ActiveMatterMarkovDataset(Dataset):
    def __init__(self, filename, saved_folder, reduced_batch=1, reduced_resolution=1, reduced_resolution_t=1,
                 num_samples_max=-1, s=None, **kwargs):
        assert reduced_resolution == 1, "reduced_resolution must be 1: the spatial size is set with 's'"
        path = os.path.join(os.path.abspath(saved_folder), filename)
        with Store(path) as f:
            concentration, velocity = read_member(f, CONCENTRATION, path), read_member(f, VELOCITY, path)
            self.alpha, self.zeta = read_scalar(f, "scalars/alpha"), read_scalar(f, "scalars/zeta")
        data = combine(concentration[::reduced_batch, ::reduced_resolution_t], velocity[::reduced_batch, ::reduced_resolution_t])
        if num_samples_max > 0:
            data = data[:min(num_samples_max, data.shape[0])]
        self.data = resize_frames(data, s)
        self.grid = unit_grid(self.data.shape[2], self.data.shape[3])
        self.x, self.y = markov_pairs(self.data)
        assert len(self.x) == len(self.y), "Invalid input output pairs"

    def __len__(self):
        return len(self.x)

    def __getitem__(self, idx):
        return self.x[idx], self.y[idx]


class MinMaxNormalizedDataset(Dataset):
    """(x - min_data) / (max_data - min_data), (y - min_model) / (max_model - min_model)"""

    def __init__(self, dataset, min_data, max_data, min_model, max_model):
        self.dataset = dataset
        self.min_data, self.max_data, self.min_model, self.max_model = min_data, max_data, min_model, max_model

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, idx):
        x, y = self.dataset[idx]
        return (x - self.min_data) / (self.max_data - self.min_data), (y - self.min_model) / (self.max_model - self.min_model)


def split_and_normalize(full: Dataset, data_normalizer: bool):
    """-> train, val, test, min_data, max_data, min_model, max_model: int(0.8 n) / int(0.1 n) / rest by random_split with
    torch.Generator seed 42; the statistics are the scalar extrema of the training split's x and y"""
    n = len(full)
    n_train, n_val = int(0.8 * n), int(0.1 * n)
    train, val, test = random_split(full, [n_train, n_val, n - n_train - n_val], generator=torch.Generator().manual_seed(42))
    min_data = max_data = min_model = max_model = None
    if data_normalizer:
        xs, ys = zip(*(b for b in DataLoader(train, batch_size=512, shuffle=False)))
        x_all, y_all = torch.cat(xs, dim=0), torch.cat(ys, dim=0)
        min_data, max_data = float(x_all.min()), float(x_all.max())
        min_model, max_model = float(y_all.min()), float(y_all.max())
        train, val, test = (MinMaxNormalizedDataset(d, min_data, max_data, min_model, max_model) for d in (train, val, test))
    return train, val, test, min_data, max_data, min_model, max_model


def active_matter_markov_dataset(filename, saved_folder, data_normalizer=True, s=None, **kwargs):
    """-> train, val, test, min_data, max_data, min_model, max_model (four None without data_normalizer)"""
    return split_and_normalize(ActiveMatterMarkovDataset(filename, saved_folder, s=s, **kwargs), data_normalizer)
