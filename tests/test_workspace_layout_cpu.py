"""Every workspace query against the entry that carves the workspace: one layout serves both, and an
entry reports a short workspace before it plans or launches anything -- which is why this needs no device.  The
pointers are dummies (non-null, 256-byte aligned); no call here gets past the workspace verdict.

Not covered, by design: rpde_feedforward_fwd_ws_bytes (optional scratch: a short workspace is no error there),
rpde_fspectral2d_prep_bytes (a prepared buffer; rpde_fspectral2d_prepare answers ERR_ARG) and rpde_grad_norm_ws_bytes
(no arena; tests/test_grad_clip_cpu.py)."""
import ctypes as C
import re

import pytest

from rpde import _lib

FAKE = 1 << 20
_PTRS = (C.c_void_p * 4)(FAKE, FAKE, FAKE, FAKE)
_FF = _lib.FFParams(2, 8, 2, 0, 1e-5, 0.0, 0, 0, C.cast(_PTRS, _lib._PP), C.cast(_PTRS, _lib._PP), None, None, None)

# query, its dims, the entry whose layout is the query's maximum at these dims, the entry's scalar arguments in order
# (pointers are filled in from the signature)
CASES = [
    ("fspectral1d", (2, 32, 8, 5), "fspectral1d_bwd", (2, 32, 8, 5, 0, 1)),
    ("fspectral2d", (1, 16, 16, 8, 4), "fspectral2d_bwd", (1, 16, 16, 8, 4, 0)),
    ("fspectral2d_eval", (1, 32, 32, 64, 4), "fspectral2d_fwd_prepared", (1, 32, 32, 64, 4)),
    ("spectral1d", (2, 3, 3, 32, 5), "spectral1d_bwd", (2, 3, 3, 32, 5, 0)),
    ("spectral2d", (1, 4, 4, 16, 16, 4, 4), "spectral2d_bwd", (1, 4, 4, 16, 16, 4, 4, 0)),
    ("fnoblock2d_eval", (1, 32, 32, 64, 64, 12, 12), "fnoblock2d_eval_fwd", (1, 32, 32, 64, 64, 12, 12, 1)),
    ("fno2d_lift_block_eval", (1, 32, 32, 64, 64, 12, 12), "fno2d_lift_block_eval_fwd", (1, 32, 32, 64, 64, 12, 12, 1)),
    ("feedforward", (64, 8, 2, 2), "feedforward_bwd", (64,)),
    ("linear", (100, 8, 16), "linear_bwd", (100, 8, 16)),
    ("conv1x1", (2, 4, 8, 64), "conv1x1_bwd", (2, 4, 8, 64, 0, 0)),
    ("resize1d", (6, 32, 20), "resize1d", (6, 32, 20)),
    ("resize2d", (6, 16, 16, 10, 24), "resize2d", (6, 16, 16, 10, 24)),
    ("freq_energy1d", (6, 32, 9), "freq_energy1d", (6, 32, 9)),
    ("freq_energy2d", (6, 16, 16), "freq_energy2d", (6, 16, 16, 8)),
    ("wrel_l2", (2, 3, 16, 10), "wrel_l2_fwd", (2, 3, 16, 10, 1)),
    ("band_energy", (2, 3, 16, 10, 4), "band_energy_fwd", (1, 2, 3, 16, 10, 4)),
    ("ns2d", (2, 16, 24), "ns2d_steps", (0, 2, 16, 24, 1)),
    ("nsc2d", (2, 16, 24), "nsc2d_steps", (0, 0.5, 2, 16, 24, 1)),
    ("grf2d", (2, 16, 24), "grf2d", (2, 16, 24)),
    ("grf1d", (2, 48), "grf1d", (2, 48)),
    ("etd1d", (2, 48), "etd1d_steps", (2, 48, 1)),
    ("etd_residual", (2, 1024), "etd_residual_bwd", (2, 1024, 1)),
    ("ns2d_residual", (2, 16, 24), "ns2d_residual_fwd", (2, 16, 24, 1)),
    ("darcy2d", (2, 16), "darcy2d_solve", (0, 2, 16, 4, 1e-6)),
]


def _call(lib, entry, scalars, ws_bytes):
    """the entry with dummy pointers, these scalars and a workspace of ws_bytes"""
    scalars, args = list(scalars), []
    for t in _lib._SIGNATURES["rpde_" + entry][1][:-3]:
        if t is _lib._P:
            args.append(FAKE)
        elif t is _lib._PP:
            args.append(C.cast(_PTRS, _lib._PP))
        elif t in (_lib._I, _lib._L, _lib._F):
            args.append(scalars.pop(0))
        else:
            args.append(C.byref(_FF))
    assert not scalars, (entry, scalars)
    return getattr(lib, "rpde_" + entry)(*args, FAKE, ws_bytes, None)


def test_every_workspace_query_is_covered():
    queries = {n[5:-9] for n in _lib._SIGNATURES if n.endswith("_ws_bytes")}
    assert queries - {c[0] for c in CASES} == {"feedforward_fwd", "grad_norm"}


@pytest.mark.parametrize("query,dims,entry,scalars", CASES, ids=[c[0] for c in CASES])
def test_query_and_entry_share_one_layout(query, dims, entry, scalars):
    lib = _lib.load()
    need = getattr(lib, f"rpde_{query}_ws_bytes")(*dims)
    assert need > 0 and need % 256 == 0, need

    def refused(given):
        assert _call(lib, entry, scalars, given) == _lib.ERR_WORKSPACE, lib.rpde_last_error()
        m = re.fullmatch(rf"{entry}: workspace too small \((\d+) bytes, needs (\d+)\)", lib.rpde_last_error().decode())
        assert m, lib.rpde_last_error()
        return int(m.group(1)), int(m.group(2))

    # an empty workspace first: the entry's own measurement is the query's value, so the next call cannot get further
    assert refused(0) == (0, need)
    assert refused(need - 256) == (need - 256, need)
