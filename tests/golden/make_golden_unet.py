#!/usr/bin/env python3
"""Golden vectors for the U-Net model family, from the IMPORTED reference (build container only).

    RPDE_REFERENCE=<checkout of the reference> python tests/golden/make_golden_unet.py [case-name ...]

The reference's models.unet (UNet1d, UNet2d) runs on the CPU in float32 with the seeded weights, buffers and inputs of
tests/golden/unet_cases.py; one forward and backward per case.  Stored per case: the case, the parameter layout (names,
shapes, dtypes) and digests of every result (tests/golden/synth.py), each with `floor`, the reference's own
float32-versus-float64 disagreement on that tensor (BatchNorm's cancellation) -- data only, nothing of the reference's
text.  A fixture in which a tensor's floor exceeds FLOOR_LIMIT is not written: three times that floor would be a budget
above 1e-4, and such a case checks nothing."""
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
FLOOR_LIMIT = 3.3e-5
SIZE_LIMIT = 256 * 1024
PART_BYTES = 150 * 1024       # of uncompressed digests per file


def _reference_classes():
    ref = os.environ.get("RPDE_REFERENCE")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("set RPDE_REFERENCE to a checkout of the reference")
    sys.dont_write_bytecode = True
    warnings.filterwarnings("ignore")
    sys.path.insert(0, ref)
    from models.unet import UNet1d, UNet2d
    sys.path.remove(ref)
    for name in [m for m in sys.modules if m.split(".")[0] in ("models", "utils")]:      # cannot shadow the project's
        del sys.modules[name]
    return types.SimpleNamespace(UNet1d=UNet1d, UNet2d=UNet2d)


def main(argv):
    ns = _reference_classes()
    sys.path.insert(0, REPO)
    import torch
    from tests.golden import synth
    from tests.golden import unet_cases
    from tests.golden.unet_cases import CASES, run_case, state_for

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
        floors = {k: float(blob[k]) for k in blob if k.endswith("|floor") and float(blob[k]) < 1.0}
        worst = max(floors, key=floors.get)
        if floors[worst] > FLOOR_LIMIT:
            raise SystemExit(f"{case['name']}: the reference's own float32 floor of {worst} is {floors[worst]:.2e} > "
                             f"{FLOOR_LIMIT:.1e}; not written")
        # a case whose digests do not fit one file of SIZE_LIMIT goes into <name>.npz, <name>.part2.npz, ...: each holds
        # the meta record and whole results (unet_cases.load_case puts them together again)
        parts, room = [{}], PART_BYTES
        for name in res:
            keys = [k for k in blob if k.split("|")[0] == name]
            need = sum(blob[k].nbytes for k in keys)
            if need > room and parts[-1]:
                parts.append({})
                room = PART_BYTES
            parts[-1].update({k: blob[k] for k in keys})
            room -= need
        sizes = []
        for i, part in enumerate(parts):
            path = os.path.join(HERE, unet_cases.part_name(case["name"], i) + ".npz")
            np.savez_compressed(path, meta=blob["meta"], **part)
            sizes.append(os.path.getsize(path))
            if sizes[-1] >= SIZE_LIMIT:
                raise SystemExit(f"{path}: {sizes[-1]} bytes, {SIZE_LIMIT // 1024} KiB or more")
        print(f"{case['name']:22s} {len(res):3d} tensors  {' + '.join(f'{v / 1024:.1f}' for v in sizes)} KiB  worst floor "
              f"{floors[worst]:.2e} ({worst[:-6]})  {time.time() - t0:6.1f}s", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
