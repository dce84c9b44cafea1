#!/usr/bin/env python3
"""s_memtime phase timeline of k_ffs_layer1 (csrc/ff_bwd_split.hip) in the debug build:
    python resolution-pde_amd/rpde/build.py --stamps
    RPDE_LIB=resolution-pde_amd/rpde/lib/librpde_hip_stamps.so python profiles/ffs_layer1_stamps.py
FeedForward(64, 4, three layers, LayerNorm, dropout 0.1) backward at B = 32, 256 x 256; lane 0 of waves 0, 3 and 6 of
workgroup 100 stamps tiles 5 .. 12 of its 256 (s_memtime: shader clocks).  The stamps are stores of their own and the
compiler orders vector work around them freely: read the shares as those of the debug build."""
import ctypes as C
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "resolution-pde_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from rpde import _lib  # noqa: E402
from models.custom_layer import FeedForward  # noqa: E402

lib = _lib.load()
torch.manual_seed(0)
ff = FeedForward(64, 4, n_layers=3, layer_norm=True, dropout=0.1).to("cuda")
x = torch.randn(32, 256, 256, 64, device="cuda").requires_grad_(True)
res, g = torch.randn_like(x), torch.randn_like(x)
for _ in range(3):
    ff(x, residual=res).backward(g)
torch.cuda.synchronize()
buf = (C.c_ulonglong * (3 * 64))()
lib.rpde_debug_ffl_stamps.argtypes = [C.c_void_p]
_lib.check(lib.rpde_debug_ffl_stamps(buf), "stamps")
t = np.array(buf, dtype=np.uint64).reshape(3, 8, 8).astype(np.int64)
names = ["top", "barrier 1 passed", "products + scaling done", "panels written, x requested", "barrier 2 passed",
         "next du2 staged + requested", "gW1 done", "gx done"]
for wi, wn in enumerate(("wave 0", "wave 3", "wave 6")):
    print(wn)
    for ti in range(7):
        row = t[wi, ti]
        print("   tile", ti + 5, " ".join(f"{names[i]}:+{int(row[i] - row[0])}" for i in range(1, 8)),
              f" | tile period {int(t[wi, ti + 1, 0] - row[0])}")
per = (t[:, 1:, 0] - t[:, :-1, 0]).astype(np.float64)
seg = np.diff(np.concatenate([t[:, :7, :], t[:, 1:, :1]], axis=2), axis=2).astype(np.float64)     # [wave][tile][8 phases]
print("mean share of the tile period, waves 0 / 3 / 6:")
for i in range(8):
    what = f"{names[i]} -> {names[i + 1] if i < 7 else 'x maximum, next top'}"
    print(f"   {what:64s}", " ".join(f"{100 * (seg[wv, :, i] / per[wv]).mean():5.1f}%" for wv in range(3)))
print("mean tile period:", " ".join(f"{per[wv].mean():.0f}" for wv in range(3)))
