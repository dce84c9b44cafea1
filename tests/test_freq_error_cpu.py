"""CPU (no GPU needed) side of the per-frequency error decomposition: the float64 restatement of the two formulas
(tests/freq_error_ref.py) reproduces every fixture recorded from the reference run in float64; the host-side radial bin
table of rpde.ops matches the reference's bin populations; the four C-ABI entry points report argument errors as
statuses without touching a GPU; the drop-in module and the entry point import without a GPU, matplotlib or scipy."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import freq_error_ref as F
from tests.conftest import DROPIN, REPO

ROUND_OFF = 1e-12        # float64 round-off of two ways to sum ~1e5 squares, not a measurement (the same comparison gave 4.6e-14)


@pytest.mark.parametrize("name", list(F.CASES))
def test_float64_restatement_reproduces_the_reference(name):
    _, shape, k, s, seed = F.CASES[name]
    fx = F.load(name)
    pred, target = F.make_inputs(shape, s, seed)
    err, sol, freq = (F.ref_1d if len(shape) == 3 else F.ref_2d)(pred, target, k)
    d = (F.rel(err, fx["error"]), F.rel(sol, fx["solution"]), F.rel(freq, fx["frequencies"]))
    print(name, "rel-L2 of restatement vs fixture (error, solution, frequencies):", d)
    assert err.shape == fx["error"].shape and max(d) <= ROUND_OFF, d


@pytest.mark.parametrize("name", [c[0] for c in F.CASES_2D])
def test_radial_bin_table_matches_the_reference(name):
    from rpde.ops import radial_bins
    _, shape, nb, _, _ = F.CASES[name]
    fx = F.load(name)
    bins, centres = radial_bins(shape[-2], shape[-1], nb)
    assert bins.dtype.is_floating_point is False and tuple(bins.shape) == (shape[-2], shape[-1] // 2 + 1)
    b = bins.numpy()
    assert b.min() >= -1 and b.max() < nb
    assert np.array_equal(np.bincount(b[b >= 0], minlength=nb), fx["population"])
    assert int((b < 0).sum()) == int(fx["unbinned"])
    assert np.array_equal(np.asarray(centres), fx["frequencies"])
    assert radial_bins(shape[-2], shape[-1], nb)[0] is bins                      # cached


def test_unbinned_count_at_256_with_64_bins():
    from rpde.ops import radial_bins
    b = radial_bins(256, 256, 64)[0].numpy()
    assert b.size == 33024 and int((b < 0).sum()) == 7182


def test_argument_errors_come_back_as_statuses_without_a_gpu():
    from rpde import _lib
    lib = _lib.load()
    ERR_MODES, ERR_WS = -4, -3
    buf = (C.c_double * 4096)()
    p = (C.addressof(buf) + 15) // 16 * 16                                    # never dereferenced: every call below fails before device work
    big = 1 << 30
    # 1-D
    assert lib.rpde_freq_energy1d(None, p, p, 4, 64, 33, p, big, None) == _lib.ERR_ARG
    assert b"null" in lib.rpde_last_error()
    assert lib.rpde_freq_energy1d(p, None, p, 4, 64, 33, p, big, None) == _lib.ERR_ARG
    assert lib.rpde_freq_energy1d(p, p, None, 4, 64, 33, p, big, None) == _lib.ERR_ARG
    assert lib.rpde_freq_energy1d(p, p, p, 4, 1, 1, p, big, None) == _lib.ERR_ARG            # n < 2
    assert lib.rpde_freq_energy1d(p, p, p, 0, 64, 33, p, big, None) == _lib.ERR_ARG
    assert lib.rpde_freq_energy1d(p, p, p, 4, 64, 0, p, big, None) == _lib.ERR_ARG
    assert lib.rpde_freq_energy1d(p, p, p, 4, 64, 34, p, big, None) == ERR_MODES             # n/2+1 = 33
    assert b"num_modes" in lib.rpde_last_error()
    assert lib.rpde_freq_energy1d(p, p, p, 4, 63, 33, p, big, None) == ERR_MODES             # odd n: 32 modes
    need = lib.rpde_freq_energy1d_ws_bytes(4, 64, 33)
    assert need > 0
    assert lib.rpde_freq_energy1d(p, p, p, 4, 64, 33, p, need - 1, None) == ERR_WS
    assert lib.rpde_freq_energy1d(p, p, p, 4, 64, 33, None, big, None) == ERR_WS
    assert lib.rpde_freq_energy1d(p, p, p, 4, 64, 33, p + 4, big, None) == _lib.ERR_ARG      # misaligned workspace
    assert lib.rpde_freq_energy1d(p, p, p, 4, 8192, 33, p, big, None) == _lib.ERR_ARG        # above the documented 4096
    assert lib.rpde_freq_energy1d_ws_bytes(4, 8192, 33) == 0
    # 2-D
    assert lib.rpde_freq_energy2d(None, p, p, p, 2, 32, 32, 8, p, big, None) == _lib.ERR_ARG
    assert lib.rpde_freq_energy2d(p, p, None, p, 2, 32, 32, 8, p, big, None) == _lib.ERR_ARG  # bin table
    assert lib.rpde_freq_energy2d(p, p, p, None, 2, 32, 32, 8, p, big, None) == _lib.ERR_ARG
    assert lib.rpde_freq_energy2d(p, p, p, p, 2, 1, 32, 8, p, big, None) == _lib.ERR_ARG      # H < 2
    assert lib.rpde_freq_energy2d(p, p, p, p, 2, 32, 1, 8, p, big, None) == _lib.ERR_ARG
    assert lib.rpde_freq_energy2d(p, p, p, p, 2, 32, 32, 0, p, big, None) == _lib.ERR_ARG     # n_bins < 1
    need = lib.rpde_freq_energy2d_ws_bytes(2, 32, 32)
    assert need > 0
    assert lib.rpde_freq_energy2d(p, p, p, p, 2, 32, 32, 8, p, need - 1, None) == ERR_WS
    assert lib.rpde_freq_energy2d(p, p, p, p, 2, 32, 32, 8, p + 4, big, None) == _lib.ERR_ARG
    assert lib.rpde_freq_energy2d(p, p, p, p, 2, 32, 8192, 8, p, big, None) == _lib.ERR_ARG


def test_2d_workspace_is_bounded_independently_of_the_batch():
    from rpde import _lib
    lib = _lib.load()
    assert lib.rpde_freq_energy2d_ws_bytes(64, 256, 256) == lib.rpde_freq_energy2d_ws_bytes(4096, 256, 256)
    assert lib.rpde_freq_energy2d_ws_bytes(4096, 256, 256) <= 20 << 20
    assert lib.rpde_freq_energy2d_ws_bytes(1, 64, 64) < lib.rpde_freq_energy2d_ws_bytes(64, 64, 64)
    assert lib.rpde_freq_energy2d_ws_bytes(10 ** 6, 64, 64) == lib.rpde_freq_energy2d_ws_bytes(10 ** 5, 64, 64)


def test_radial_bins_rejects_bad_arguments():
    from rpde.ops import radial_bins
    with pytest.raises(ValueError):
        radial_bins(32, 32, 0)
    with pytest.raises(ValueError):
        radial_bins(1, 32, 8)


def test_module_and_entry_point_import_without_gpu_matplotlib_or_scipy():
    code = (
        "import sys, importlib.abc\n"
        "class Block(importlib.abc.MetaPathFinder):\n"
        "    def find_spec(self, name, path=None, target=None):\n"
        "        if name.split('.')[0] in ('matplotlib', 'scipy'):\n"
        "            raise ImportError('blocked: ' + name)\n"
        "sys.meta_path.insert(0, Block())\n"
        f"sys.path.insert(0, {DROPIN!r})\n"
        "import runpy, utils.frequency_error as fe\n"
        "assert all(hasattr(fe, n) for n in ('decompose_error_by_frequency_1d', 'decompose_error_by_frequency_2d',\n"
        "                                    'FrequencyError', 'evaluate_frequency_error'))\n"
        f"ns = runpy.run_path({os.path.join(DROPIN, 'frequency_evaluation.py')!r}, run_name='not_main')\n"
        "assert callable(ns['run_frequency'])\n"
        "assert not any(m.split('.')[0] in ('matplotlib', 'scipy') for m in sys.modules)\n"
        "print('ok')\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=REPO)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
