"""What tests/test_gpu_gemm_descriptor.py rests on, checked without a GPU on the harness alone (tests/gemm_abi.py):

  * footprints and oracle equal a plain torch.matmul on tight layouts and torch as_strided views on padded, two-level
    and interleaved ones;
  * the guard check sees a stray write into row padding, one element past N in the last row, into the neighbouring
    entry of an interleaved layout and one element before the view, and reports an element left poisoned;
  * for every case of the GPU table, float32 torch on the CPU stays within half of each bound the GPU test applies
    (same inputs, same float64 oracle): a condition on the inputs, not a calibration;
  * every case with two batch levels or interleaved entries tells a mistaken oracle (z1 / z2 swapped, sC2 taken for
    sC1, ldaux taken for ldc) from the right one by at least 100 x its bound;
  * the case table reaches every route of the host dispatch;
  * the descriptors the library must refuse are refused with RPDE_ERR_ARG and a message, before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ff_abi as F
from tests import gemm_abi as G

_IDS = [c.name for c in G.CASES]


# ---------------------------------------------------------------------------------------------------------------------
# footprints and oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a_k,b_k", G.LAYOUTS)
def test_tight_layouts_equal_a_plain_matmul(a_k, b_k):
    c = G.GemmCase("tight", "t", 9, 7, 5, a_k, b_k, batch=3, bias_mode=1, alpha=0.5, accumulate=True)
    d = G.make_data(c)
    A = d["A"].double().view(3, 9, 5) if a_k else d["A"].double().view(3, 5, 9).transpose(1, 2)
    B = d["B"].double().view(3, 7, 5).transpose(1, 2) if b_k else d["B"].double().view(3, 5, 7)
    want = 0.5 * (A @ B) + d["bias"].double()[None, None, :] + d["C0"].double().view(3, 9, 7)
    got = G.evaluate(c, d)
    assert torch.equal(got["C"], want)
    assert torch.equal(got["mag"], 0.5 * (A.abs() @ B.abs()) + d["bias"].double().abs() + d["C0"].double().abs().view(3, 9, 7))
    for op, n in (("A", 3 * 9 * 5), ("B", 3 * 5 * 7), ("C", 3 * 9 * 7)):
        assert sorted(G.footprints(c)[op].ravel().tolist()) == list(range(n))


def _strided(flat, shape, strides):
    return torch.as_strided(flat.double(), shape, strides)


@pytest.mark.parametrize("name", ["pad4-nn-72x40x64-mulaux", "pad1-tt-130x68x96-mulaux", "xlines-as-B", "xlines-as-C-mulaux",
                                  "mode-mix", "mode-mix-two-level", "mode-mix-wgrad", "broadcast-A"])
def test_padded_and_interleaved_layouts_equal_as_strided_views(name):
    c = G.BY_NAME[name]
    d = G.make_data(c)
    fp = G.footprints(c)
    n1, n2 = c.batch // c.zdiv, c.zdiv
    views = {}
    for op, rows, cols, kmaj in (("A", c.M, c.K, c.a_k), ("B", c.K, c.N, not c.b_k)):
        s1, s2 = c.strides(op)
        inner = (c.ld(op), 1) if kmaj else (1, c.ld(op))
        views[op] = _strided(d[op], (n1, n2, rows, cols), (s1, s2) + inner).reshape(c.batch, rows, cols)
        assert torch.equal(views[op], G._gather(d[op], fp[op], torch.float64))
    want = views["A"] @ views["B"]
    if c.has_aux:
        s1, s2 = c.strides("C")
        want = want * _strided(d["aux"], (n1, n2, c.M, c.N), (s1, s2, c.ld("aux"), 1)).reshape(c.batch, c.M, c.N)
    assert torch.equal(G.evaluate(c, d)["C"], want)
    # C: writing the logical result through the footprint gives what a strided view of the flat buffer shows
    s1, s2 = c.strides("C")
    flat = torch.zeros(G.span(fp["C"]), dtype=torch.float64)
    val = torch.arange(c.batch * c.ksplit * c.M * c.N, dtype=torch.float64).view(c.batch, c.ksplit, c.M, c.N)
    flat[torch.from_numpy(fp["C"].ravel())] = val.reshape(-1)
    seen = torch.as_strided(flat, (n1, n2, c.ksplit, c.M, c.N), (s1, s2, c.sck, c.ld("C"), 1))
    assert torch.equal(seen.reshape(val.shape), val)


def test_overlapping_c_entries_are_refused():
    bad = G.GemmCase("overlap", "t", 8, 8, 8, batch=2, sC1=32)
    with pytest.raises(AssertionError, match="overlap"):
        G.footprints(bad)
    bad = G.GemmCase("overlap-k", "t", 8, 8, 64, ksplit=2, sCk=60)
    with pytest.raises(AssertionError, match="overlap"):
        G.footprints(bad)


# ---------------------------------------------------------------------------------------------------------------------
# the guard check
# ---------------------------------------------------------------------------------------------------------------------
def _fresh(name):
    c = G.BY_NAME[name]
    slots = G.allocate(c, G.make_data(c), "cpu")
    s = slots["C"]
    s.g.t[s.idx] = 1.0                                   # what a correct kernel leaves: the footprint, nothing else
    for k in ("aux_out", "colsum"):
        if k in slots:
            slots[k].g.t[slots[k].idx] = 1.0
    return c, slots, s


def test_guard_check_accepts_a_clean_call_and_sees_every_stray_write():
    c, slots, s = _fresh("pad4-nn-72x40x64")
    G.check_slots(c, slots)
    ldc = c.ld("C")
    strays = {"row padding": 3 * ldc + c.N, "one past N in the last row": (c.M - 1) * ldc + c.N, "one before the view": -1}
    for what, at in strays.items():
        c, slots, s = _fresh("pad4-nn-72x40x64")
        s.g.raw[F._G + s.off + at] = 0
        with pytest.raises(AssertionError) as e:
            G.check_slots(c, slots)
        assert "C:" in str(e.value), what
    # one element before a misaligned view lies inside the allocation, not in the leading guard
    c, slots, s = _fresh("mis-C")
    assert s.off == 1
    s.g.t[0] = 0.0
    with pytest.raises(AssertionError, match="outside the footprint"):
        G.check_slots(c, slots)
    # the neighbouring entry of an interleaved layout is footprint: a write there must show in the values instead
    c, slots, s = _fresh("mode-mix")
    fp = G.footprints(c)["C"]
    assert fp[1, 0, 0, 0] == fp[0, 0, 0, c.N - 1] + 1
    G.check_slots(c, slots)
    s.g.t[s.off + int(fp[0, 0, 0, c.N - 1]) + 1] = 5.0    # entry 0 wrote one element past its N
    G.check_slots(c, slots)
    got = s.read().double()[:, 0]
    ref = torch.ones_like(got)
    assert got[1, 0, 0] == 5.0 and int((got != ref).sum()) == 1
    assert G.figures(c, got, ref, None)[0] > G.MISS * c.tol
    # ... and the gap after the last entry's row is padding of nobody: guarded
    c, slots, s = _fresh("splitk-gap")
    s.g.raw[F._G + c.batch * c.M * c.N + 5] = 0
    with pytest.raises(AssertionError, match="outside the footprint"):
        G.check_slots(c, slots)


def test_guard_check_reports_poison_left_and_changed_inputs():
    c, slots, s = _fresh("pad1-nt-33x17x5")
    s.words[s.idx[-1]] = -1
    with pytest.raises(AssertionError, match="not finite"):
        G.check_slots(c, slots)
    c, slots, s = _fresh("pad1-nt-33x17x5")
    slots["A"].g.t[0] += 1.0
    with pytest.raises(AssertionError, match="an input changed"):
        G.check_slots(c, slots)
    # inputs carry the guard word outside their footprint: a read of padding is a NaN
    a = slots["A"]
    assert int((~torch.isfinite(a.g.t)).sum()) == a.n - a.idx.numel() > 0


# ---------------------------------------------------------------------------------------------------------------------
# the float32 condition on every GPU case, and the sensitivity of the two-level / interleaved ones
# ---------------------------------------------------------------------------------------------------------------------
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\n[gemm-abi-ref] float32 torch on the CPU, worst per family (relative L2, share of the K + 16 units): " +
          ", ".join(f"{k} {v[0]:.2e} / {v[1]:.2f}" for k, v in sorted(_WORST.items())))


@pytest.mark.parametrize("name", _IDS)
def test_float32_on_the_cpu_keeps_half_of_every_bound(name):
    c = G.BY_NAME[name]
    d = G.make_data(c)
    ref, f32 = G.evaluate(c, d), G.evaluate(c, d, torch.float32)
    rel, units = G.assert_figures(c, f32["C"], ref["C"], ref["mag"], scale=0.5)
    if c.aux_out:
        r2, _ = G.assert_figures(c, f32["aux_out"], ref["aux_out"], None, scale=0.5, what="aux_out")
        rel = max(rel, r2)
    if c.colsum:
        s, a = G.colsum_ref(c, f32["C"][0])
        s32 = torch.stack([f32["C"][0][128 * t:128 * t + 128].sum(0) for t in range(s.shape[0])])
        assert float(((s32.double() - s).abs() / (G.UNIT * a).clamp_min(1e-300)).max()) <= (128 + G.UNIT_MARGIN) / 2
    w = _WORST.setdefault(c.family, [0.0, 0.0])
    w[0], w[1] = max(w[0], rel), max(w[1], units / (c.K + G.UNIT_MARGIN))


_SENSITIVE = [c.name for c in G.CASES if c.two_level_or_interleaved]


@pytest.mark.parametrize("name", _SENSITIVE)
def test_a_mistaken_oracle_misses_by_a_hundred_bounds(name):
    c = G.BY_NAME[name]
    mistakes = G.applicable_mistakes(c)
    assert mistakes, (name, "no mistake this case could tell from the right oracle")
    d = G.make_data(c)
    ref = G.evaluate(c, d)["C"]
    for m in mistakes:
        rel, _ = G.figures(c, G.evaluate(c, d, mistake=m)["C"], ref, None)
        assert rel >= G.MISS * c.tol, (name, m, rel)


def test_the_sensitive_cases_are_the_ones_the_issue_names():
    assert {"xlines-as-B", "xlines-as-C", "mode-mix", "mode-mix-wgrad"} <= set(_SENSITIVE)
    assert {m for n in _SENSITIVE for m in G.applicable_mistakes(G.BY_NAME[n])} == set(G.MISTAKES)
    mix = G.BY_NAME["mode-mix"]
    assert mix.ld("A") == mix.ld("C") == 2 * 4 * 18 and mix.strides("A")[0] == mix.strides("C")[0] == 36 == mix.N == mix.K
    wg = G.BY_NAME["mode-mix-wgrad"]
    assert (wg.a_k, wg.b_k) == (0, 0) and wg.ksplit > 1 and wg.sck == 4 * 4 * 18 * 18


# ---------------------------------------------------------------------------------------------------------------------
# route coverage
# ---------------------------------------------------------------------------------------------------------------------
def test_case_table_reaches_every_route():
    default = [(c, G.route(c, 2)) for c in G.CASES]
    native = [(c, G.route(c, 0)) for c in G.CASES]
    both = default + native

    def some(rows, **kv):
        return [c.name for c, r in rows if all(r[k] == v for k, v in kv.items())]

    assert some(both, vec=True) and some(both, vec=False)
    assert some(both, vec=True, cvec=False)
    for tile in [(128, 128), (128, 64), (64, 128), (64, 64), (128, 32), (32, 128)]:
        assert some(native, vec=True, tile=tile, kernel="native"), tile
    assert not some(native, kernel="bf16x3")
    for variant in ("single", "pipe", "preaux", "double"):
        assert some(native, kernel="native", variant=variant), variant
    # the default dispatch reaches the PREAUX and single-stage kernels too (K no multiple of 32)
    assert some(default, kernel="native", variant="preaux") and some(default, kernel="native", variant="single")
    for layout in ("nt", "nn", "tn", "tt"):
        assert some(default, kernel="bf16x3", layout=layout, img=None), layout
    assert some(default, kernel="bf16x3", img="a") and some(default, kernel="bf16x3", img="b")
    for tile in [(128, 128), (128, 64), (64, 128), (64, 64)]:
        assert some(default, kernel="bf16x3", tile=tile), tile
    for swz in (0, 1, 2):
        assert some(default, swz=swz) and some(native, swz=swz), swz
    assert some(both, swz=1, vec=True) and some(both, swz=1, vec=False)
    assert [c.name for c, r in both if r["grid"][2] > 1]
    assert some(both, pro=1) and some(both, pro=2)
    # the cases the issue spells out take the routes it names
    r = G.route(G.BY_NAME["acc-preaux-200-inplace"], 0)
    assert r["variant"] == "preaux" and r["tile"] == (128, 128) and r["kchunk"] <= 64
    r = G.route(G.BY_NAME["grid-xcd-vec"], 2)
    assert r["swz"] == 1 and (4228 + 63) // 64 % 8 != 0 and r["grid"][0] == 72 * 2
    r = G.route(G.BY_NAME["grid-z2"], 2)
    assert r["grid"] == (1, 32768, 2)
    assert G.route(G.BY_NAME["splitk-swz2"], 2)["swz"] == 2 and G.route(G.BY_NAME["splitk-swz2-plus1"], 2)["swz"] == 0
    assert G.route(G.BY_NAME["splitk-dead-vec"], 2)["kernel"] == "bf16x3" and G.route(G.BY_NAME["splitk-dead-vec"], 2)["kchunk"] == 32
    for op in ("A", "B"):
        assert not G.route(G.BY_NAME[f"mis-{op}"], 2)["vec"]
    for n in ("mis-C", "mis-aux", "mis-bias", "mis-acc_src", "mis2-aux_out"):
        r = G.route(G.BY_NAME[n], 2)
        assert r["vec"] and not r["cvec"], n
    assert max(c.batch * c.ksplit * c.M * c.N for c in G.CASES) <= 6.3e6


# ---------------------------------------------------------------------------------------------------------------------
# descriptors the library refuses (validation precedes any launch: fake non-null pointers)
# ---------------------------------------------------------------------------------------------------------------------
FAKE = 0x10000


def _refused(c: G.GemmCase, fragment: bytes, **ptr_overrides):
    from rpde import _lib
    lib = _lib.load()
    lib.rpde_last_error.restype = C.c_char_p
    ptrs = {op: FAKE * (i + 1) for i, op in enumerate(G.OPERANDS)}
    ptrs = {op: p for op, p in ptrs.items() if op in c.present()}
    ptrs.update(ptr_overrides)
    d = G.descriptor(c, ptrs)
    assert lib.rpde_gemm_f32(C.byref(d), None) == _lib.ERR_ARG, c
    msg = lib.rpde_last_error()
    assert msg and fragment in msg, (c.name, msg)


def test_rejected_descriptors():
    base = dict(M=200, N=40, K=64, a_k=1, b_k=1)
    for kw in (dict(bias_mode=1), dict(accumulate=True), dict(epi_dact=G.EPI_MULAUX), dict(write_act=G.ACT_GELU)):
        _refused(G.GemmCase("r", "r", ksplit=2, **base, **kw), b"split-K slabs take no epilogue")
    _refused(G.GemmCase("r", "r", act_a=1, act_b=1, **base), b"only one operand")
    _refused(G.GemmCase("r", "r", epi_dact=G.ACT_GELU, **base), b"epi_dact needs aux", aux=None)
    _refused(G.GemmCase("r", "r", aux_out=True, **base), b"aux_out needs write_act")
    _refused(G.GemmCase("r", "r", colsum=True, batch=2, **base), b"colsum needs")
    _refused(G.GemmCase("r", "r", colsum=True, **dict(base, M=64)), b"colsum needs")
    _refused(G.GemmCase("r", "r", colsum=True, **base), b"colsum needs", C=FAKE + 4)
    _refused(G.GemmCase("r", "r", act_b=G.ACT_GELU, **dict(base, a_k=0, b_k=1)), b"staged activation on operand 2 is not built")
    _refused(G.GemmCase("r", "r", act_a=G.ACT_GELU, **dict(base, a_k=1, b_k=0)), b"staged activation on operand 1 is not built")
    from rpde import _lib
    assert _lib.load().rpde_gemm_f32(None, None) == _lib.ERR_ARG
