"""CPU (no GPU needed): the float64 restatement of gradient-norm clipping (tests/clip_ref.py) equals
torch.nn.utils.clip_grad_norm_ in float64, and the library declares, exports and argument-checks the entry points of
the device-side clip (include/rpde.h, csrc/adamw_clip.hip)."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from tests.clip_ref import clipped_f64
from tests.conftest import REPO

EPS64 = 2.0 ** -52
NEW = ("rpde_grad_norm_ws_bytes", "rpde_grad_norm", "rpde_adamw_step_clip", "rpde_adamw_step_dev_clip",
       "rpde_adamw_apply_dev_clip")


def _grads(kind):
    g = torch.Generator().manual_seed(3)
    real = [torch.randn(3, dtype=torch.float64, generator=g), torch.randn(64, 3, dtype=torch.float64, generator=g),
            torch.randn(5, dtype=torch.float64, generator=g)]
    if kind == "complex":
        return real + [torch.randn(5, 7, dtype=torch.complex128, generator=g)]
    if kind == "none":
        return [real[0], None, real[2]]
    if kind == "zero":
        return [torch.zeros_like(t) for t in real]
    if kind in ("inf", "nan"):
        real[1][7, 1] = float(kind)
    return real


@pytest.mark.parametrize("kind,max_norm", [("real", 0.5), ("real", 1e3), ("complex", 0.5), ("complex", 1e3), ("none", 0.25),
                                           ("zero", 1.0), ("inf", 1.0), ("nan", 1.0)])
def test_restatement_equals_torch_clip_grad_norm_in_float64(kind, max_norm):
    grads = _grads(kind)
    params = [torch.nn.Parameter(torch.zeros_like(g) if g is not None else torch.zeros(2, dtype=torch.float64)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.clone()
    norm_t = float(torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2))
    norm, scale, clipped = clipped_f64(grads, max_norm)
    # torch takes the norm of the per-tensor norms, this file one square root of one sum: a few float64 roundings apart
    assert (math.isnan(norm) and math.isnan(norm_t)) or norm == norm_t or abs(norm - norm_t) <= 8 * EPS64 * norm_t, (norm, norm_t)
    if kind == "real" or kind == "complex":
        assert (scale < 1.0) == (max_norm < norm)
    if kind == "zero":
        assert scale == 1.0
    if kind == "inf":
        assert scale == 0.0
    if kind == "nan":
        assert math.isnan(scale)
    for p, c in zip(params, clipped):
        if c is None:
            assert p.grad is None
            continue
        got = torch.view_as_real(p.grad) if p.grad.is_complex() else p.grad
        fin = ~c.isnan()
        assert bool(((got[fin] - c[fin]).abs() <= 16 * EPS64 * c[fin].abs()).all())
        assert torch.equal(got.isnan(), c.isnan())


def test_header_declares_and_library_exports_the_clip_entry_points():
    from rpde import _lib
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "rpde.h")).read()
    declared = set(re.findall(r"\b(rpde_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, f"{name} is not declared in rpde.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib._SIGNATURES
    # the signatures the plain steps had stay as they were
    assert _lib._SIGNATURES["rpde_adamw_step"][1] == _lib._SIGNATURES["rpde_adamw_step_clip"][1][:12] + [C.c_void_p]
    assert len(_lib._SIGNATURES["rpde_adamw_step_dev"][1]) + 1 == len(_lib._SIGNATURES["rpde_adamw_step_dev_clip"][1])
    assert len(_lib._SIGNATURES["rpde_adamw_apply_dev"][1]) + 1 == len(_lib._SIGNATURES["rpde_adamw_apply_dev_clip"][1])


def test_clip_argument_errors_are_reported_without_a_gpu():
    from rpde import _lib
    lib = _lib.load()
    # one double per workgroup, a grid that depends on the length alone and is capped
    assert lib.rpde_grad_norm_ws_bytes(4) == 8
    assert lib.rpde_grad_norm_ws_bytes(1028) == 16
    cap = lib.rpde_grad_norm_ws_bytes(1 << 40)
    assert cap % 8 == 0 and 8 < cap <= 8 * 4096 and lib.rpde_grad_norm_ws_bytes(1 << 41) == cap
    assert lib.rpde_grad_norm_ws_bytes(0) == 0 and lib.rpde_grad_norm_ws_bytes(6) == 0 and lib.rpde_grad_norm_ws_bytes(-4) == 0
    a = 4096                                     # a 16-byte aligned non-null address: every call below fails before using it
    assert lib.rpde_grad_norm(None, 4, 1.0, 0, a, a, 8, None) == _lib.ERR_ARG
    assert b"grad_norm" in lib.rpde_last_error()
    assert lib.rpde_grad_norm(a, 6, 1.0, 0, a, a, 8, None) == _lib.ERR_ARG
    assert b"multiple of 4" in lib.rpde_last_error()
    assert lib.rpde_grad_norm(a, 4, 1.0, 0, None, a, 8, None) == _lib.ERR_ARG
    assert lib.rpde_grad_norm(a, 4, float("nan"), 0, a, a, 8, None) == _lib.ERR_ARG
    assert b"NaN" in lib.rpde_last_error()
    assert lib.rpde_grad_norm(a + 4, 4, 1.0, 0, a, a, 8, None) == _lib.ERR_ARG
    assert b"aligned" in lib.rpde_last_error()
    assert lib.rpde_grad_norm(a, 1028, 1.0, 0, a, a, 8, None) == _lib.ERR_WORKSPACE
    assert b"workspace" in lib.rpde_last_error()
    s = (1.0, 0.1, 0.999, 0.001, 1e-3, 1.0, 1e-8)
    assert lib.rpde_adamw_step_clip(a, a, a, a, 4, *s, None, None) == _lib.ERR_ARG        # no record
    assert lib.rpde_adamw_step_clip(a, a, a, a, 6, *s, a, None) == _lib.ERR_ARG
    assert b"adamw_step_clip" in lib.rpde_last_error()
    assert lib.rpde_adamw_step_clip(a, a + 4, a, a, 4, *s, a, None) == _lib.ERR_ARG
    assert b"aligned" in lib.rpde_last_error()
    d = (1e-3, 0.9, 0.999, 1e-8, 1e-2)
    assert lib.rpde_adamw_step_dev_clip(a, a, a, a, 4, *d, a, None, None) == _lib.ERR_ARG
    assert lib.rpde_adamw_step_dev_clip(a, a, a, a, 4, *d, None, a, None) == _lib.ERR_ARG
    assert b"adamw_step_dev_clip" in lib.rpde_last_error()
    assert lib.rpde_adamw_apply_dev_clip(a, a, a, a, 4, *d, a, None, None) == _lib.ERR_ARG
    assert lib.rpde_adamw_apply_dev_clip(None, a, a, a, 4, *d, a, a, None) == _lib.ERR_ARG
    assert b"adamw_apply_dev_clip" in lib.rpde_last_error()


def test_flat_adamw_refuses_options_it_cannot_honour():
    """the checks come before anything touches a device"""
    from rpde.optim import FlatAdamW
    p = [torch.nn.Parameter(torch.zeros(4))]
    for bad in (-1.0, float("nan"), 0.0):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FlatAdamW(p, max_grad_norm=bad, capturable=True)
    with pytest.raises(ValueError, match="skip_nonfinite"):
        FlatAdamW(p, skip_nonfinite=True, capturable=False)
