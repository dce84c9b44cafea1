"""tests/eval_cf_ref.py checked without a device: what tests/test_gpu_eval_cf.py rests on.

Tables.  For 64, 256 and 304 compute units the geometry functions say which pass counts, template instances, activations
and FULL / LIFT values the case tables reach, and that is asserted here, so that an edit of a shape cannot silently lose
a branch; every case is accepted by the library's own host-only *_ok query and by the restated conditions, the cases meant
for the multiply-add tail are refused by the h2 conditions, and the documented eligibility edges are refused.

Oracle.  Float64 against an independent dense statement built from the matrices of oracle/dft_math.py (no torch.fft),
and bit for bit against spectral_cf_ref.run_oracle("block"); float32 against float64 is the floor, and it must itself be
inside the whole-tensor bound per line.

Planted faults -- the reason this file exists.  The older tests of these kernels assert one whole-tensor relative L2 below
2e-6.  On the float64 result of each kernel's 2T + T/2 + 3 case at 256 CUs four faults of a broken pass loop are planted
into ONE line: the line one pass earlier in the same wave (a stale prefetch), a line left unwritten, the last line of the
last pass dropped, a 64-point wave segment swapped with its neighbour.  Each stands 1.8e4 .. 4.8e5 times above the per-line
bound (FLOOR_FACTOR x the float32 oracle's line figure; 100 x is required).  What the whole-tensor figure does with them
is arithmetic: one line among n moves it by 1 / sqrt(n) of the line's own error, so the full-size faults measure 1.5e-3 ..
1.3e-2 there (n = 20 492 .. 163 936 lines) and could only fall below 2e-6 among 5e11 lines.  They are therefore shrunk,
ref + s (fault - ref), until the whole-tensor figure is just inside 2e-6 -- what the older tests let pass -- and must then
still stand above the per-line bound by MARGIN_AT_TOL = 10: with n >= 20 000 lines, a floor of at most 2e-6 per line
(both asserted) and at most two lines touched (the segment swap) the margin is at least sqrt(20 000 / 2) / FLOOR_FACTOR
= 12.5.  Measured, smallest over the four faults: 23 (lift), 41 (proj), 116 (syn), 121 (mlp).
(A full-size fault that stays below 2e-6 over the whole tensor, as one might wish to show, does not exist by the
arithmetic above; "hidden from the whole-tensor norm" is therefore asserted at the size where that norm just passes.)"""
import math
import os

import numpy as np
import pytest
import torch

from oracle import dft_math as D
from tests import eval_cf_ref as E
from tests import spectral_cf_ref as S

MARGIN_AT_TOL = 10.0
MIN_FAULT_LINES = 20000
PERSISTENT = ("syn", "lift", "proj", "mlp")


@pytest.fixture(scope="module")
def lib():
    from rpde import _lib
    return _lib.load()


def _resolved(cus):
    return [(c, E.resolve(c, cus)) for c in E.ALL_CASES]


# ---- tables ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", E.CU_COUNTS)
def test_every_case_is_accepted_and_small(lib, cus):
    names = [c.name for c in E.ALL_CASES]
    assert len(set(names)) == len(names)
    for c, sh in _resolved(cus):
        q, args = E.ok_query(c, sh)
        assert getattr(lib, q)(*args) == 1, (c.name, q, args, lib.rpde_last_error())
        assert E.ok_restated(c, sh), (c.name, sh)
        assert sh["m2"] <= c.N // 2 + 1 or c.kernel == "mlp", c.name
        assert 1 <= sh["m1"] <= sh["M"], c.name
        # (64 MiB at 256 CUs; the symbolic sizes grow with the device)
        assert E.tensor_bytes(c, sh) <= E.MAX_CASE_BYTES * max(256, cus) // 256, (c.name, E.tensor_bytes(c, sh))
        assert c.act in E.ACTS and c.content in ("randn", "scaled", "zero")
        if c.content != "randn":
            assert sh["B"] >= 3 and isinstance(c.rows, tuple), c.name
    for name in E.FAULT_CASES.values():
        assert E.by_name(name).rows == "3pass"


@pytest.mark.parametrize("cus", E.CU_COUNTS)
def test_the_tables_reach_every_pass_count_and_instance(cus):
    by = {k: [(c, E.resolve(c, cus)) for c in t] for k, t in E.TABLES.items()}
    for k in PERSISTENT:
        geo = {c.name: E.passes(c, sh, cus) for c, sh in by[k]}
        U = {c.name: E.unit(c) for c, _ in by[k]}
        rows = {c.name: sh["rows"] for c, sh in by[k]}
        sym = {c.rows: c for c, _ in by[k] if isinstance(c.rows, str)}
        # partial first pass: one row, and a workgroup with idle waves; one unit short of / past a workgroup's share
        assert any(r == 1 for r in rows.values()), k
        assert any(rows[n] % U[n] for n in rows), k
        assert any(g == (1, 1, 1) and rows[n] == U[n] - 1 for n, g in geo.items() if U[n] > 1), (k, geo)
        assert any(g == (2, 1, 1) and rows[n] == U[n] + 1 for n, g in geo.items()), (k, geo)
        # pass boundaries
        for s in E.BOUNDARY:
            assert s in sym, (k, s)
        T = {s: E.full_pass(sym[s], cus) for s in sym}
        assert geo[sym["T-1"].name][1:] == (1, 1) and rows[sym["T-1"].name] == T["T-1"] - 1
        assert geo[sym["T"].name] == (E.clamp(sym["T"], cus), 1, 1)
        assert geo[sym["T+1"].name] == (E.clamp(sym["T+1"], cus), 1, 2)            # one workgroup with a second pass
        three = [c for c, sh in by[k] if c.rows == "3pass"]
        assert len(three) >= (1 if k == "lift" else 2) and all(geo[c.name] == (E.clamp(c, cus), 2, 3) for c in three), (k, geo)
        # sample boundaries inside a pass: B > 1 and M no multiple of the unit
        assert any(sh["B"] > 1 and sh["M"] % E.unit(c) for c, sh in by[k] if E.unit(c) > 1), k
        assert sum(c.content == "scaled" for c, _ in by[k]) == (k != "lift") and sum(c.content == "zero" for c, _ in by[k]) == (k != "lift")
    if cus == 256:                                                   # ... and across passes, where the count factors
        for k in ("syn", "proj", "mlp"):
            assert any(sh["B"] > 1 and sh["M"] % E.unit(c) and E.passes(c, sh, cus)[2] >= 2 for c, sh in by[k]), k

    inst = {k: {E.instance(c, sh) for c, sh in by[k]} for k in by}
    # k_conv_syn_h2<ACT, FULL, LIFT>: all twelve
    assert inst["syn"] | inst["lift"] == {("k_conv_syn_h2", a, f, l) for a in E.ACTS for f in (True, False) for l in (True, False)}
    assert {c.N for c, _ in by["syn"]} == {64, 128, 256, 512}
    assert {c.Cout for c, _ in by["syn"]} >= {32, 31, 17, 16, 1}
    for k in ("syn", "proj"):
        assert {2 * E.r4(sh["m2"]) for _, sh in by[k]} == {8, 16, 24, 32}, k
    assert all(E.tail_of(c, sh) == "h2" and E.tail_of(c, sh, False) == "fma" for c, sh in by["syn"])
    lift = by["lift"]
    assert any(sh["M"] % 4 == 0 for _, sh in lift) and any(sh["M"] % 4 for _, sh in lift) and any(sh["M"] == 1024 for _, sh in lift)
    assert any("bl" in c.null for c, _ in lift) and any(c.grid == "user" for c, _ in lift)
    # k_conv_syn_proj_h2<MT, CO, ACT>
    assert {i[1:3] for i in inst["proj"]} == {(m, q) for m in (2, 4, 8) for q in (1, 4)}
    assert {i[3] for i in inst["proj"]} == set(E.ACTS)
    assert {c.Cmid for c, _ in by["proj"]} >= {16, 24, 48, 64, 100, 128} and {c.Cq for c, _ in by["proj"]} == {1, 2, 3, 4}
    assert {c.Cout for c, _ in by["proj"]} >= {32, 20, 16, 1}
    assert {c.N for c, _ in by["proj"]} >= {64, 128, 512, 1024}
    for c, sh in by["proj"]:
        if c.N == 1024:
            assert sh["rows"] <= 24 and E.proj_lds(c.N, c.Cmid) == 150016
        if E.passes(c, sh, cus)[2] > 1:
            assert c.N == 64
    assert any(c.N == 512 and E.proj_lds(c.N, c.Cmid) > 65536 for c, _ in by["proj"])
    # k_conv_mlp_h2<KS, MT, CO>
    assert {i[1:3] for i in inst["mlp"]} == {(1, 2), (1, 4), (1, 8), (2, 2), (2, 4)}
    assert {i[3] for i in inst["mlp"]} == {1, 2, 4} and {c.Cout for c, _ in by["mlp"]} == {1, 2, 3, 4}
    assert {c.act for c, _ in by["mlp"]} == set(E.ACTS)
    assert any(c.Cin == 32 and 33 <= c.Cmid <= 64 for c, _ in by["mlp"]) and any(c.Cin == 64 and c.Cmid <= 32 for c, _ in by["mlp"])
    nulls = {c.null for c, _ in by["mlp"]}
    assert ("pb1",) in nulls and ("pb2",) in nulls and ("pb1", "pb2") in nulls
    # k_conv1x1_small<CO, true>: the four instances with Cout = CO and Cout < CO
    assert {c.Cout for c, _ in by["fma"]} >= {1, 4, 5, 8, 9, 16, 17, 32}
    assert {i[1] for i in inst["fma"]} == {4, 8, 16, 32}
    assert {c.N for c, _ in by["fma"]} == {4, 32, 1024, 2048} and {c.Cin for c, _ in by["fma"]} == {1, 5, 32, 64}


def test_eligibility_edges(lib):
    for q, args in E.REFUSED:
        assert getattr(lib, q)(*args) == 0, (q, args)
    # the multiply-add cases are refused by the h2 conditions (which the lifted entry's query exposes), the h2 cases are not
    for c, sh in _resolved(256):
        if c.kernel in ("fma", "syn"):
            R2 = 2 * E.r4(sh["m2"])
            assert E.h2_ok(c.Cin, c.Cout, sh["M"], c.N, R2) == (c.kernel == "syn"), c.name
            if c.kernel == "fma" or E.col_stage_ok(sh["M"], sh["m1"], E.r4(sh["m2"])) and sh["M"] <= 1024:
                got = lib.rpde_fno2d_lift_block_eval_ok(1, c.Cin, c.Cout, sh["M"], c.N, sh["m1"], sh["m2"])
                assert got == (c.kernel == "syn"), (c.name, got)
    # the switches
    for var, kernels in (("RPDE_CONV_PROJ", ("proj",)), ("RPDE_CONV_MLP", ("mlp",)), ("RPDE_CONV_SYN_H2", ("lift",)),
                         ("RPDE_LIFT_FUSED", ("lift",))):
        old = os.environ.get(var)
        os.environ[var] = "0"
        try:
            for c, sh in _resolved(256):
                q, args = E.ok_query(c, sh)
                assert getattr(lib, q)(*args) == (0 if c.kernel in kernels else 1), (var, c.name)
        finally:
            if old is None:
                os.environ.pop(var)
            else:
                os.environ[var] = old


# ---- the oracle ----------------------------------------------------------------------------------------------------------
def _dense(case, inp):
    """the case's float64 result from explicit DFT matrices"""
    t = E._to(inp, torch.float64)
    if case.kernel == "mlp":
        h = {"identity": lambda v: v, "gelu": torch.nn.functional.gelu, "relu": torch.relu}[case.act](t["x"])
    else:
        if "u" in t:
            x = (t["wl"][:, 0].view(1, -1, 1, 1) * t["u"] + t["wl"][:, 1].view(1, -1, 1, 1) * t["gx"].view(1, 1, -1, 1) +
                 t["wl"][:, 2].view(1, -1, 1, 1) * t["gy"].view(1, 1, 1, -1))
            if "bl" in t:
                x = x + t["bl"].view(1, -1, 1, 1)
        else:
            x = t["x"]
        B, Ci, M, N = x.shape
        m1, m2 = t["w1"].shape[2], t["w1"].shape[3]
        A = torch.from_numpy(D.analysis(N, m2, "backward"))
        xs = torch.complex(x @ A[0::2].T, x @ A[1::2].T)                              # [B,Ci,M,m2]
        weight = {}
        for r in range(m1):
            weight[r] = t["w1"][:, :, r]
        for r in range(m1):
            weight[M - m1 + r] = t["w2"][:, :, r]                                     # (overwrites on overlap: quirk Q6)
        rows = np.array(sorted(weight))
        CA = torch.from_numpy(D.complex_analysis(M, rows, "backward"))
        CS = torch.from_numpy(D.complex_synthesis(M, rows, "backward"))
        spec = torch.einsum("rm,bimk->birk", CA, xs)
        W = torch.stack([weight[int(r)] for r in rows], dim=2)                        # [Ci,Co,R,m2]
        z = torch.einsum("mr,bork->bomk", CS, torch.einsum("birk,iork->bork", spec, W))
        Sy = torch.from_numpy(D.synthesis(N, m2, "backward"))
        pre = z.real @ Sy[:, 0::2].T + z.imag @ Sy[:, 1::2].T
        pre = pre + torch.einsum("oi,bimn->bomn", t["wc"], x)
        if "bc" in t:
            pre = pre + t["bc"].view(1, -1, 1, 1)
        h = {"identity": lambda v: v, "gelu": torch.nn.functional.gelu, "relu": torch.relu}[case.act](pre)
        if case.kernel != "proj":
            return h
    hid = torch.einsum("hc,bc...->bh...", t["pw1"], h)
    if "pb1" in t:
        hid = hid + t["pb1"].view(1, -1, *([1] * (hid.dim() - 2)))
    out = torch.einsum("qh,bh...->bq...", t["pw2"], torch.nn.functional.gelu(hid))
    if "pb2" in t:
        out = out + t["pb2"].view(1, -1, *([1] * (out.dim() - 2)))
    return out


@pytest.mark.parametrize("name", ["p-straddle", "l-user-grid", "f-n4-co1", "s-1", "m-straddle"])
def test_oracle_equals_the_dense_matrix_statement(name):
    """a projection case (m2 = 5, Cq = 2), a lifted case on a user grid, N = 4 with its Nyquist column, M = m1 = 1 (weights2
    overwrites weights1: quirk Q6), and the MLP alone"""
    case = E.by_name(name)
    sh = E.resolve(case, 256)
    inp = E.make_inputs(case, sh)
    ref, dense = E.evaluate(case, inp), _dense(case, inp)
    assert ref.dtype == torch.float64 and ref.shape == dense.shape
    assert float((ref - dense).norm()) <= 1e-12 * float(ref.norm()), name


def test_the_block_expression_is_the_one_of_spectral_cf_ref():
    case = E.by_name("s-straddle")
    inp = E.make_inputs(case, E.resolve(case, 256))
    blk = dict(inp, g=torch.zeros(*inp["x"].shape[:1], case.Cout, *inp["x"].shape[2:]),
               wc=inp["wc"].view(case.Cout, case.Cin, 1, 1))
    for real in (torch.float64, torch.float32):
        want = S.run_oracle("block", blk, "identity", real)["out"]
        got = E.pre_activation(E._to(inp, real))
        assert got.dtype == real and torch.equal(got, want)


def test_inputs_are_what_the_cases_say():
    for c, sh in _resolved(64):
        if isinstance(c.rows, str) and c.rows in E.BOUNDARY:
            continue
        inp = E.make_inputs(c, sh)
        assert not set(c.null) & set(inp), c.name
        if c.kernel != "mlp":
            for w in ("w1", "w2"):                       # signed spectral weights
                assert float(inp[w].real.min()) < 0 < float(inp[w].real.max()) or inp[w].numel() < 4, c.name
                assert inp[w].dtype == torch.complex64
        x = inp["u" if c.kernel == "lift" else "x"]
        if c.content == "zero":
            assert not x[1].any() and x[0].any() and x[2].any()
            ref = E.evaluate(c, inp)
            const = E.zero_sample_planes(c, ref)      # every plane of the zero sample is one constant
            assert const.shape == (ref.shape[1],)
        if c.content == "scaled":
            rms = x.double().flatten(1).square().mean(dim=1).sqrt()
            assert 5e3 < float(rms[-1] / rms[0]) < 2e4      # four decades


FLOOR_NAMES = sorted(set(E.FAULT_CASES.values()) | {c.name for c in E.ALL_CASES if isinstance(c.rows, tuple)})


def test_the_float32_floor_is_inside_the_whole_tensor_bound():
    """the yardstick is not degenerate, and a float32 evaluation meets 2e-6 per line as well as over the tensor"""
    for name in FLOOR_NAMES:
        case = E.by_name(name)
        fl = E.reference(case, 64)[3]
        assert 0 < fl["rel"] <= E.TOL and 0 < fl["line"] <= E.TOL, (name, fl)


# ---- planted faults ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", PERSISTENT)
def test_planted_faults_are_caught_per_line_and_not_by_the_whole_tensor_norm(kernel):
    case = E.by_name(E.FAULT_CASES[kernel])
    sh, inp, ref, fl = E.reference(case, 256)
    n_lines = E.lines(case, ref).shape[0] * E.lines(case, ref).shape[1]
    bound = S.FLOOR_FACTOR * fl["line"]
    assert n_lines >= MIN_FAULT_LINES and 0 < fl["line"] <= E.TOL
    assert E.passes(case, sh, 256)[1:] == (2, 3)
    assert E.figures(case, ref, ref) == {"rel": 0.0, "line": 0.0}
    for kind in E.FAULTS:
        full = E.figures(case, E.plant(case, sh, 256, ref, kind), ref)
        print(f"[eval-cf faults] {case.name} {kind}: line {full['line']:.3g} = {full['line'] / bound:.3g} x bound, "
              f"whole tensor {full['rel']:.3g}")
        assert full["line"] >= E.FAULT_MARGIN * bound, (kind, full, bound)
        # one line among n: the whole-tensor figure is the line's error over sqrt(n) (the lines have about the RMS norm)
        assert full["rel"] <= 2.0 * full["line"] / math.sqrt(n_lines), (kind, full)
        assert full["rel"] > E.TOL                          # (full size cannot hide: see the docstring)
        s = 0.99 * E.TOL / full["rel"]
        small = E.figures(case, E.plant(case, sh, 256, ref, kind, size=s), ref)
        print(f"[eval-cf faults] {case.name} {kind} x {s:.3g}: whole tensor {small['rel']:.3g}, line {small['line'] / bound:.3g} x bound")
        assert small["rel"] <= E.TOL, (kind, small)
        assert small["line"] >= MARGIN_AT_TOL * bound, (kind, small, bound)
