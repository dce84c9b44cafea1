#!/usr/bin/env python3
"""Golden vectors for the 2-D CNO model family, from the IMPORTED reference (build container only).

    RPDE_REFERENCE=<checkout of the reference> python tests/golden/make_golden_cno2d.py [case-name ...]

The reference's models.CNO2d (CNO_LReLu, CNO2d) runs on the CPU in float32 with the seeded weights, buffers and inputs
of tests/golden/cno2d_cases.py; one forward and backward per case.  Stored per case: the case, the parameter layout
(names, shapes, dtypes) and digests of every result (tests/golden/synth.py: whole tensors up to 20 000 scalars, sampled
scalars and projections above), each with `floor`, the reference's own float32-versus-float64 disagreement on that
tensor (the LeakyReLU kink, BatchNorm's cancellation) -- data only, nothing of the reference's text."""
from __future__ import annotations

import json
import os
import sys
import time
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def _reference_classes():
    ref = os.environ.get("RPDE_REFERENCE")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("set RPDE_REFERENCE to a checkout of the reference")
    sys.dont_write_bytecode = True
    warnings.filterwarnings("ignore")
    sys.path.insert(0, ref)
    from models.CNO2d import CNO2d, CNO_LReLu
    sys.path.remove(ref)
    for name in [m for m in sys.modules if m.split(".")[0] in ("models", "utils")]:      # cannot shadow the project's
        del sys.modules[name]
    return types.SimpleNamespace(CNO2d=CNO2d, CNO_LReLu=CNO_LReLu)


def main(argv):
    ns = _reference_classes()
    sys.path.insert(0, REPO)
    import torch
    from tests.golden import synth
    from tests.golden.cno2d_cases import CASES, run_case, state_for

    torch.set_num_threads(8)
    want = set(argv)
    for case in CASES:
        if want and case["name"] not in want:
            continue
        t0 = time.time()

        def build(dtype):
            module = getattr(ns, case["kind"])(**case["ctor"])
            spec = synth.spec_of(module.state_dict())
            module.load_state_dict(state_for(spec, case["seed"]), strict=True)
            return module.to(dtype), spec

        module, spec = build(torch.float32)
        res = run_case(module, case)
        res64 = run_case(build(torch.float64)[0], case, dtype=torch.float64)
        blob = {"meta": np.array(json.dumps({"case": case, "spec": spec, "torch": torch.__version__}))}
        for name, t in res.items():
            for k, v in synth.digest(t).items():
                blob[f"{name}|{k}"] = v
            r64 = res64[name].to(torch.float64)
            blob[f"{name}|floor"] = np.array(float((t.to(torch.float64) - r64).norm() / (r64.norm() + 1e-300)))
        path = os.path.join(HERE, case["name"] + ".npz")
        np.savez_compressed(path, **blob)
        worst = max(float(blob[k]) for k in blob if k.endswith("|floor"))
        print(f"{case['name']:22s} {len(res):3d} tensors  {os.path.getsize(path) / 1024:8.1f} KiB  worst floor {worst:.2e}"
              f"  {time.time() - t0:6.1f}s", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
