#!/usr/bin/env python3
"""Golden vectors for utils.res_utils.downsample, from the IMPORTED reference (build container only).

    RPDE_REFERENCE=<checkout of the reference> python tests/golden/make_golden_downsample.py      # downsample2d.npz

The reference's utils.res_utils.downsample is run on numpy-seeded white noise, 2 images x 2 channels per case, float32.
Stored: the inputs and the reference's outputs -- data only, nothing of the reference's text."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# name -> (source size, target size): even halving twice, a target that is no divisor, the identity
CASES = {"16to8": (16, 8), "12to6": (12, 6), "16to10": (16, 10), "8to8": (8, 8)}


def main():
    sys.dont_write_bytecode = True
    ref = os.environ.get("RPDE_REFERENCE")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("set RPDE_REFERENCE to a checkout of the reference")
    sys.path[:] = [ref] + [p for p in sys.path if os.path.abspath(p or ".") not in (os.path.dirname(os.path.dirname(HERE)),)]
    from utils.res_utils import downsample
    out = {}
    for i, (name, (h, n)) in enumerate(CASES.items()):
        x = np.random.default_rng(70 + i).standard_normal((2, 2, h, h)).astype(np.float32)
        out[f"{name}|x"] = x
        out[f"{name}|y"] = np.asarray(downsample(x, n), dtype=np.float32)
    out["meta"] = np.array(json.dumps({"cases": {k: list(v) for k, v in CASES.items()}, "numpy": np.__version__}))
    path = os.path.join(HERE, "downsample2d.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
