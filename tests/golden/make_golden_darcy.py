#!/usr/bin/env python3
"""Golden vectors for the Darcy loader, from the IMPORTED reference (build container only).

    RPDE_REFERENCE=<checkout of the reference> python tests/golden/make_golden_darcy.py      # darcy_loader.npz

The reference's load_darcy_data_from_mat (dataloaders/load_data.py) is run on two small synthetic ``.mat`` files written
here with scipy (``coeff`` / ``sol`` [N, s, s], numpy-seeded; the second case spells the key ``Kcoeff``) at res_scale 1
and 2.  Its .mat branch needs scipy only; ``matplotlib`` and ``h5py`` are stubbed when they do not import (unused on this
path).  Stored: the synthetic inputs' recipe, the split sizes, the encoded first / last pair of every split and the
point-wise normaliser statistics -- data only, nothing of the reference's text."""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# name -> (coefficient key, res_scale)
CASES = {"coeff_r1": ("coeff", 1), "kcoeff_r2": ("Kcoeff", 2)}
FILES = (dict(seed=31, n=13), dict(seed=32, n=10))          # 23 samples: 18 / 2 / 3
S = 16


def synthetic_pair(seed, n, s=S):
    """(coeff, sol) [n, s, s] float32: a two-valued field and a smooth companion, numpy-seeded"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, s, s))
    coeff = np.where(g >= 0, 12.0, 3.0).astype(np.float32)
    sol = (np.cumsum(np.cumsum(g, axis=1), axis=2) / s + rng.standard_normal((n, 1, 1))).astype(np.float32)
    return coeff, sol


def main():
    sys.dont_write_bytecode = True
    ref = os.environ.get("RPDE_REFERENCE")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("set RPDE_REFERENCE to a checkout of the reference")
    sys.path[:] = [ref] + [p for p in sys.path if os.path.abspath(p or ".") not in (os.path.dirname(os.path.dirname(HERE)),)]
    for name in ("matplotlib", "matplotlib.pyplot", "h5py"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    import torch
    from scipy.io import savemat
    with contextlib.redirect_stdout(io.StringIO()):
        from dataloaders.load_data import load_darcy_data_from_mat
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case, (key, scale) in CASES.items():
            paths = []
            for i, spec in enumerate(FILES):
                coeff, sol = synthetic_pair(**spec)
                paths.append(os.path.join(tmp, f"{case}_{i}.mat"))
                savemat(paths[-1], {key: coeff, "sol": sol})
            with contextlib.redirect_stdout(io.StringIO()):
                tr, va, te, xn, yn = load_darcy_data_from_mat(paths[0], paths[1], res_scale=scale, batch_size=4)
            for split, loader in (("train", tr), ("val", va), ("test", te)):
                x, y = loader.dataset.tensors
                out[f"{case}|{split}_n"] = np.array(len(x))
                out[f"{case}|{split}_x_first"], out[f"{case}|{split}_x_last"] = x[0].numpy(), x[-1].numpy()
                out[f"{case}|{split}_y_first"], out[f"{case}|{split}_y_last"] = y[0].numpy(), y[-1].numpy()
            for nm, norm in (("x", xn), ("y", yn)):
                out[f"{case}|{nm}_mean"], out[f"{case}|{nm}_std"] = norm.mean.numpy(), norm.std.numpy()
                out[f"{case}|{nm}_eps"] = np.array(float(norm.eps))
    out["meta"] = np.array(json.dumps({"cases": {k: list(v) for k, v in CASES.items()}, "files": list(FILES), "s": S,
                                       "torch": torch.__version__}))
    path = os.path.join(HERE, "darcy_loader.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
