"""Darcy flow: coefficient field a -> solution u, one pair per sample (reference: dataloaders/load_data.py
load_darcy_data_from_mat :182-260 for the .mat files, dataloaders/darcy_loader.py H5DarcyDataset for PDEBench's HDF5).

    darcy_dataset(filename, saved_folder, ...) -> train, val, test, x_normalizer, y_normalizer

the five-tuple rpde/entry.py unpacks for a 2-D dataset.  As load_darcy_data_from_mat: keys ``coeff`` or ``Kcoeff`` plus
``sol``, a second file stacked under the first, stride subsampling [::r, ::r], and the 80 / 10 / 10 split in FILE ORDER
(no shuffle).  As H5DarcyDataset: keys ``nu`` / ``tensor`` ([N, 1, s, s] or [N, T, s, s]: the first time level).  Files
are opened through dataloaders/_store.py: .mat, .npz, and .h5 / .hdf5 where h5py imports.  Items are (x [1, s, s],
y [1, s, s]).

A deliberate difference: the reference normalises with a point-wise UnitGaussianNormalizer, whose [s, s] statistics
cannot be applied at another resolution; the default here is the global one (one mean and std per field,
ns_naive_markov.SimpleNormalizer), "unit_gaussian" selects the point-wise one.  Statistics come from the training split
only.  Pinned against load_darcy_data_from_mat through tests/golden/darcy_loader.npz (split, stride, point-wise
statistics); the HDF5 leg is unpinned here, read as text."""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset

from dataloaders._store import Store
from dataloaders.ns_naive_markov import NormalizedDataset, SimpleNormalizer
from models.custom_layer import UnitGaussianNormalizer


def read_darcy(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """(coefficient, solution), both [N, s, s] float32, under either spelling of the .mat files or PDEBench's names"""
    with Store(path) as f:
        keys = list(f.keys())
        if "sol" in keys and ("coeff" in keys or "Kcoeff" in keys):
            x, y = np.asarray(f["coeff" if "coeff" in keys else "Kcoeff"]), np.asarray(f["sol"])
        elif "nu" in keys and "tensor" in keys:
            x, y = np.asarray(f["nu"]), np.asarray(f["tensor"])
            if y.ndim == 4:
                y = y[:, 0]                                   # [N, 1, s, s], or the first time level of [N, T, s, s]
        else:
            raise KeyError(f"{path}: expected 'coeff' (or 'Kcoeff') and 'sol', or 'nu' and 'tensor'; found {keys}")
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    if x.ndim != 3 or x.shape != y.shape:
        raise ValueError(f"{path}: coefficient {x.shape} and solution {y.shape}, expected two [N, s, s] arrays")
    return x, y


class DarcyDataset(Dataset):
    """pairs (x [1, s, s], y [1, s, s]) in file order"""

    def __init__(self, x: torch.Tensor, y: torch.Tensor):
        assert x.shape == y.shape and x.dim() == 4
        self.x, self.y = x, y

    def __len__(self):
        return len(self.x)

    def __getitem__(self, idx):
        return self.x[idx], self.y[idx]


def darcy_dataset(filename, saved_folder, filename2: Optional[str] = None, reduced_resolution=1, reduced_batch=1,
                  num_samples_max=-1, data_normalizer=True, normalization_type="simple"):
    """-> train, val, test, x_normalizer, y_normalizer.  filename2: a second file stacked under the first (the reference
    always reads two); num_samples_max caps the samples, reduced_batch then strides over them, both before the split."""
    x, y = read_darcy(os.path.join(saved_folder, filename))
    if filename2:
        x2, y2 = read_darcy(os.path.join(saved_folder, filename2))
        if x2.shape[1:] != x.shape[1:]:
            raise ValueError(f"{filename2}: grid {x2.shape[1:]}, but {filename} has {x.shape[1:]}")
        x, y = np.vstack([x, x2]), np.vstack([y, y2])
    r, rb = int(reduced_resolution), int(reduced_batch)
    if r < 1 or rb < 1:
        raise ValueError(f"reduced_resolution and reduced_batch must be >= 1, got {r} and {rb}")
    if num_samples_max > 0:                                   # the cap counts file samples, as H5DarcyDataset's [:N:rb]
        x, y = x[:num_samples_max], y[:num_samples_max]
    x, y = x[::rb, ::r, ::r], y[::rb, ::r, ::r]
    X = torch.from_numpy(np.ascontiguousarray(x)).float().unsqueeze(1)
    Y = torch.from_numpy(np.ascontiguousarray(y)).float().unsqueeze(1)
    n = X.shape[0]
    n_train, n_val = int(n * 0.8), int(n * 0.1)
    cuts = ((0, n_train), (n_train, n_train + n_val), (n_train + n_val, n))
    train, val, test = (DarcyDataset(X[lo:hi], Y[lo:hi]) for lo, hi in cuts)
    x_normalizer = y_normalizer = None
    if data_normalizer:
        if normalization_type == "simple":
            x_normalizer = SimpleNormalizer(train.x.mean(), train.x.std())
            y_normalizer = SimpleNormalizer(train.y.mean(), train.y.std())
        elif normalization_type == "unit_gaussian":
            x_normalizer, y_normalizer = UnitGaussianNormalizer(train.x), UnitGaussianNormalizer(train.y)
        else:
            raise ValueError(f"Invalid normalization_type: {normalization_type}. Must be 'simple' or 'unit_gaussian'")
        train, val, test = (NormalizedDataset(d, x_normalizer, y_normalizer) for d in (train, val, test))
    return train, val, test, x_normalizer, y_normalizer
