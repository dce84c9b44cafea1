"""GPU: rpde_gemm_f32 over its whole descriptor, in guarded and poisoned buffers (tests/gemm_abi.py).

Every case of gemm_abi.CASES runs through the C ABI with every operand in an allocation of its own: padded leading
dimensions (vector and scalar routes), one operand at a time 4 bytes off a 16-byte boundary, two batch levels,
broadcast, pre-split and interleaved operands (the library's own DFT-line, mode-mix and weight-gradient patterns),
accumulate in place and from acc_src on the vector, scalar, split-bf16 and PREAUX routes, split-K into poisoned slabs
(the slabs past K must come back as exact zeros), gridDim.z = 2, the XCD tile orders with blocks past the last
M-tile, batched epilogues with aux / aux_out at C's batch offsets, per-tile column sums, and K in 0, 1, 31, 32, 33.

After every call: every word outside an output's footprint is still the guard word (row padding, the gap between
split-K slabs and the leading guard included), every word inside is finite, every input is unchanged.  The result is
held per batch entry to the project's bounds (2e-6; 4e-6 with split-K or alpha != 1 with accumulate; 1e-5 with an
activation) and per element to (K + 16) * 2^-24 * (|alpha| |A| @ |B| + |bias| + |C0|), against a float64 oracle that
gathers the operands through the same footprints.  tests/test_gemm_abi_ref_cpu.py shows that float32 torch keeps half
of each bound on these inputs and that the two-level and interleaved cases can tell a mis-indexed oracle.

tests/test_gpu_kernels.py::test_native_fp32_mfma_path_stays_green re-runs this file with RPDE_SPLIT_BF16=0, so every
case also runs on the native fp32-MFMA kernels.

Worst figures on an MI355X per family (relative L2 of the worst batch entry / share of the elementwise K + 16 units),
default dispatch, then RPDE_SPLIT_BF16=0:
    padded        1.88e-07 / 0.14    1.88e-07 / 0.14
    misaligned    1.85e-07 / 0.03    1.85e-07 / 0.03      against the all-aligned run: 2.18e-07, 0
    batch-levels  1.17e-07 / 0.09    1.52e-07 / 0.09
    accumulate    1.44e-07 / 0.11    1.80e-07 / 0.11
    split-k       3.20e-07 / 0.02    3.20e-07 / 0.02
    grid          1.03e-07 / 0.18    1.03e-07 / 0.18
    epilogue      1.66e-07 / 0.13    1.96e-07 / 0.13
    short-k       1.10e-07 / 0.11    1.10e-07 / 0.11
The whole file takes 4 s per leg.
"""
import os

import pytest
import torch

from tests import gemm_abi as G

pytestmark = pytest.mark.gpu

_SPLIT_MODE = 0 if os.environ.get("RPDE_SPLIT_BF16") == "0" else 2
_WORST = {}
_RESULTS = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print(f"\n[gemm-descriptor] RPDE_SPLIT_BF16={'0' if _SPLIT_MODE == 0 else 'default'} worst per family "
          "(relative L2 / share of the K + 16 units): " +
          ", ".join(f"{k} {v[0]:.2e} / {v[1]:.2f}" for k, v in sorted(_WORST.items())))


def _run(dev, c):
    """run and check one case (once per module: the misaligned and pre-split cases look at their twins' results)"""
    if c.name not in _RESULTS:
        got = G.run_case(c, dev)
        figs = G.check_result(c, got, _SPLIT_MODE)
        w = _WORST.setdefault(c.family, [0.0, 0.0])
        w[0], w[1] = max(w[0], figs["rel"]), max(w[1], figs["units_over_K16"])
        print(f"\n[gemm-descriptor] {c.name}: " + " ".join(f"{k}={v:.3g}" for k, v in figs.items()))
        _RESULTS[c.name] = got if c.family in ("misaligned", "batch-levels") else True
    return _RESULTS[c.name]


def _family(name):
    cs = [c for c in G.CASES if c.family == name]
    return pytest.mark.parametrize("case", cs, ids=[c.name for c in cs])


@_family("padded")
def test_padded_leading_dimensions(gpu_device, case):
    _run(gpu_device, case)


@_family("misaligned")
def test_one_misaligned_operand(gpu_device, case):
    got = _run(gpu_device, case)
    twin = _run(gpu_device, G.aligned_twin(case))
    for k in got:
        rel, _ = G.figures(case, got[k].flatten(0, -3), twin[k].flatten(0, -3), None)
        assert rel < G.GEMM_TOL, (case.name, k, "against the all-aligned run", rel)
        w = _WORST.setdefault("misaligned against aligned", [0.0, 0.0])
        w[0] = max(w[0], rel)


@_family("batch-levels")
def test_two_batch_levels_and_shared_operands(gpu_device, case):
    got = _run(gpu_device, case)
    if case.name == "broadcast-A-split":
        plain = _run(gpu_device, G.BY_NAME["broadcast-A"])
        assert torch.equal(got["C"], plain["C"]), "a pre-split A must not change a bit of the result"


@_family("accumulate")
def test_accumulate_in_place_and_from_acc_src(gpu_device, case):
    _run(gpu_device, case)


@_family("split-k")
def test_split_k_into_poisoned_slabs(gpu_device, case):
    _run(gpu_device, case)


@_family("grid")
def test_grid_edges(gpu_device, case):
    _run(gpu_device, case)


@_family("epilogue")
def test_batched_epilogues_and_column_sums(gpu_device, case):
    _run(gpu_device, case)


@_family("short-k")
def test_short_reductions(gpu_device, case):
    _run(gpu_device, case)


def test_every_family_has_a_test():
    assert set(G.FAMILIES) == {"padded", "misaligned", "batch-levels", "accumulate", "split-k", "grid", "epilogue", "short-k"}
