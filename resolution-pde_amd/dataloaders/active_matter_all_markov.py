"""Many active-matter style files -> one set of single-step (Markov) training pairs with min-max statistics.  Same
public names, arguments and seven return values as the reference's dataloaders/active_matter_all_markov.py
(MultiFileActiveMatterMarkovDataset :12-282, multi_file_active_matter_markov_dataset :285-380); the members, the
container formats, the resize at load time and the split are those of dataloaders/active_matter_markov.py.

Files are ``sorted(glob(file_pattern))`` under ``saved_folder`` and ``max_files`` keeps a prefix of them; a file whose
members lack the sample axis ([T, H, W] and [T, H, W, 2]) counts as one trajectory; the sample cap applies after the
files are concatenated.  ``file_parameters`` holds, per kept trajectory, L, zeta and alpha (from a name of the form
active_matter_L_<L>_zeta_<zeta>_alpha_<alpha>.<ext> when it matches, ``scalars/zeta`` / ``scalars/alpha`` in front when
the file has them, otherwise None), every other ``scalars/*`` member of the file and the file's name;
``parameter_stats`` their ranges."""
from __future__ import annotations

import glob
import os
import re

import numpy as np
from torch.utils.data import Dataset

from dataloaders._store import Store
from dataloaders.active_matter_markov import (CONCENTRATION, VELOCITY, combine, markov_pairs, read_member, read_scalar,
                                              resize_frames, split_and_normalize, unit_grid)

_NAME = re.compile(r"active_matter_L_([\d.]+)_zeta_([\d.]+)_alpha_([-\d.]+)\.(?:hdf5|h5|npz)$")


def parameters_from_filename(filename: str):
    """(L, zeta, alpha) of active_matter_L_10.0_zeta_17.0_alpha_-5.0.hdf5, or three None"""
    m = _NAME.search(filename)
    return (float(m.group(1)), float(m.group(2)), float(m.group(3))) if m else (None, None, None)


def _with_batch_axis(a: np.ndarray, ndim: int, what: str) -> np.ndarray:
    if a.ndim == ndim - 1:
        return a[None]
    if a.ndim != ndim:
        raise ValueError(f"Unexpected {what} shape: {a.shape}")
    return a


class MultiFileActiveMatterMarkovDataset(Dataset):
    def __init__(self, file_pattern, saved_folder, reduced_batch=1, reduced_resolution=1, reduced_resolution_t=1,
                 num_samples_max=-1, s=None, max_files=None, **kwargs):
        assert reduced_resolution == 1, "reduced_resolution must be 1: the spatial size is set with 's'"
        search = os.path.join(os.path.abspath(saved_folder), file_pattern)
        self.file_paths = sorted(glob.glob(search))
        if not self.file_paths:
            raise ValueError(f"No files found matching pattern: {search}")
        if max_files is not None and max_files > 0:
            self.file_paths = self.file_paths[:max_files]
        parts, self.file_parameters = [], []
        for path in self.file_paths:
            name = os.path.basename(path)
            L, zeta, alpha = parameters_from_filename(name)
            with Store(path) as f:
                concentration = _with_batch_axis(read_member(f, CONCENTRATION, path), 4, "concentration")
                velocity = _with_batch_axis(read_member(f, VELOCITY, path), 5, "velocity")
                file_alpha, file_zeta = read_scalar(f, "scalars/alpha"), read_scalar(f, "scalars/zeta")
                extra = {k: read_scalar(f, "scalars/" + k) for k in (f["scalars"].keys() if "scalars" in f else ())
                         if k not in ("alpha", "zeta")}
            part = combine(concentration[::reduced_batch, ::reduced_resolution_t], velocity[::reduced_batch, ::reduced_resolution_t])
            parts.append(part)
            self.file_parameters += [{"L": L, "zeta": zeta if file_zeta is None else file_zeta,
                                      "alpha": alpha if file_alpha is None else file_alpha, **extra, "filename": name}
                                     for _ in range(part.shape[0])]
        data = np.concatenate(parts, axis=0)
        if num_samples_max > 0:
            keep = min(num_samples_max, data.shape[0])
            data, self.file_parameters = data[:keep], self.file_parameters[:keep]
        self.parameter_stats = self._parameter_stats()
        self.data = resize_frames(data, s)
        self.grid = unit_grid(self.data.shape[2], self.data.shape[3])
        self.x, self.y = markov_pairs(self.data)
        assert len(self.x) == len(self.y), "Invalid input output pairs"

    def _parameter_stats(self):
        """{name: {min, max, unique}} over the trajectories that carry the parameter, and the two counts"""
        stats = {"total_trajectories": len(self.file_parameters), "total_files": len(self.file_paths)}
        for key in sorted({k for p in self.file_parameters for k in p} - {"filename"}):
            vals = [p[key] for p in self.file_parameters if p.get(key) is not None]
            stats[key] = {"min": min(vals), "max": max(vals), "unique": sorted(set(vals))} if vals else \
                {"min": None, "max": None, "unique": []}
        return stats

    def __len__(self):
        return len(self.x)

    def __getitem__(self, idx):
        return self.x[idx], self.y[idx]


def multi_file_active_matter_markov_dataset(file_pattern, saved_folder, data_normalizer=True, s=None, max_files=None, **kwargs):
    """-> train, val, test, min_data, max_data, min_model, max_model (four None without data_normalizer)"""
    full = MultiFileActiveMatterMarkovDataset(file_pattern, saved_folder, s=s, max_files=max_files, **kwargs)
    return split_and_normalize(full, data_normalizer)
