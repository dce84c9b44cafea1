#!/usr/bin/env python3
"""Generate tests/golden/freq_*.npz from the IMPORTED reference (build container only).

Run:  python tests/golden/make_freq_golden.py [case-name ...]

The reference's utils/frequency_error.py is imported (it pulls matplotlib and scipy) and run on the seeded inputs of
tests/freq_error_ref.py; nothing from it is copied.  A fixture holds the case description and results only: the
reference's three arrays run in float64, the rel-L2 distance of its own float32 run from them (``floor32``, for the
record), and for 2-D the bin populations and the number of half-spectrum entries that belong to no bin.  It also
asserts that the deliberately wrong restatements miss the float64 result by at least 100 x the parity tolerance, so the
inputs are known to make them visible.
"""
from __future__ import annotations

import json
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
TOL = 1e-5


def _reference():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    warnings.filterwarnings("ignore")
    import matplotlib
    matplotlib.use("Agg")
    from utils.frequency_error import decompose_error_by_frequency_1d, decompose_error_by_frequency_2d
    sys.path.remove(REF)
    for name in [m for m in sys.modules if m.split(".")[0] in ("models", "utils")]:
        del sys.modules[name]
    return decompose_error_by_frequency_1d, decompose_error_by_frequency_2d


def main(argv):
    ref1, ref2 = _reference()
    sys.path.insert(0, REPO)
    import torch
    from tests import freq_error_ref as F

    torch.set_num_threads(8)
    for name, shape, k, s, seed in F.CASES_1D + F.CASES_2D:
        if argv and name not in argv:
            continue
        t0 = time.time()
        dims = len(shape) - 2
        pred, target = F.make_inputs(shape, s, seed)
        fn = ref1 if dims == 1 else ref2
        e64, s64, f64 = fn(pred.double(), target.double(), k)
        e32, s32, _ = fn(pred, target, k)
        floor = (F.rel(e32, e64), F.rel(s32, s64))
        blob = {"meta": np.array(json.dumps({"name": name, "shape": list(shape), "k": k, "s": s, "seed": seed,
                                             "torch": torch.__version__})),
                "error": np.asarray(e64, np.float64), "solution": np.asarray(s64, np.float64),
                "frequencies": np.asarray(f64, np.float64), "floor32": np.asarray(floor, np.float64)}
        if dims == 2:
            bins, _ = F.bin_table(shape[-2], shape[-1], k)
            blob["population"] = np.bincount(bins[bins >= 0], minlength=k).astype(np.int64)
            blob["unbinned"] = np.array(int((bins < 0).sum()), np.int64)
        own = (F.ref_1d if dims == 1 else F.ref_2d)(pred, target, k)
        d_own = max(F.rel(own[0], e64), F.rel(own[1], s64))
        assert d_own <= 1e-12, (name, d_own)
        miss = {}
        for label, kw in F.wrong_variants(dims).items():
            miss[label[0]] = F.rel((F.ref_1d if dims == 1 else F.ref_2d)(pred, target, k, **kw)[0], e64)
            assert miss[label[0]] >= 100 * TOL, (name, label, miss[label[0]])
        if s >= 1e-2:
            assert max(floor) <= TOL, f"{name}: floor32 {floor} above {TOL}: take another seed"
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **blob)
        print(f"{name:20s} floor32 err {floor[0]:.2e} sol {floor[1]:.2e}  restatement {d_own:.1e}  smallest miss "
              f"{min(miss.values()):.3f}  {os.path.getsize(path) / 1024:6.1f} KiB {time.time() - t0:6.1f}s", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
