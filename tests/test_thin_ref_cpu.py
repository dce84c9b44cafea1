"""What tests/test_gpu_thin_linear.py and tests/test_gpu_conv_small.py rest on, checked without a GPU (tests/thin_abi.py):
every case meets the edge it is listed for, the `exact` kind is exact in float32, the float32 CPU restatement of every
randn problem stays within half of each derived per-element bound, the checks see every planted fault, and the
workspace query covers the slabs the plan counts.

The one problem that lives on the device (Cin = 512 at 2^20 points: 2 GiB of input) is restated here on 2 x 4096 points,
the number its device reference is cross-checked on."""
import pytest
import torch

from tests import thin_abi as A


# ---------------------------------------------------------------------------------------------------------------------
# the edges
# ---------------------------------------------------------------------------------------------------------------------
def test_gelu_tol_is_the_pointwise_tests():
    from tests import test_gpu_pointwise as PW
    assert A.GELU_TOL == PW.GELU_TOL
    x = torch.linspace(-6, 6, 240001, dtype=torch.float64, requires_grad=True)
    d, = torch.autograd.grad(torch.nn.functional.gelu(x).sum(), x)
    assert float(d.abs().max()) <= A.DGELU_MAX


def _outer_trips(p0, p1, pps):
    """k_thin_outer's two loops for point lane 0, word for word (thin_linear.hip:109-140)"""
    p, full, rem = p0, 0, 0
    while p + (A.TL_UNROLL - 1) * pps < p1:
        full, p = full + 1, p + A.TL_UNROLL * pps
    while p < p1:
        rem, p = rem + 1, p + pps
    return full, rem


def test_thin_cases_use_the_stated_launches():
    for P, (shapes, expect) in A.LARGE_POINTS.items():
        for T, O in shapes:
            plan = A.thin_plan(P, T, O)
            want = dict(expect, **A.LARGE_EXTRA.get((P, T, O), {}))
            assert plan["thin_ok"] and {k: plan[k] for k in want} == want, (P, T, O, plan)
            assert _outer_trips(0, plan["ppb"], plan["pps"]) == (plan["full"], plan["rem"])
    # the second grid-stride trip of expand and of contract, the capped outer grid, its empty workgroups, the 8-deep
    # loop and its remainder in one workgroup -- with O <= 32 only at 2 100 001 points
    assert A.thin_plan(32769, 1, 64)["sweeps_contract"] > A.TL_GRID_CAP
    assert A.thin_plan(131072, 3, 64)["empty"] == 0 and A.thin_plan(131073, 3, 64)["empty"] == 7
    assert all(A.thin_plan(P, T, O)["full"] == 0 for P, (shapes, _) in A.LARGE_POINTS.items() if P < 2100001
               for T, O in shapes if O <= 32)
    assert A.thin_plan(70001, 3, 64)["ppb"] == 128 and A.thin_plan(70001, 3, 64)["rem"] == 0    # what the old test ran
    # the small set: a partial sweep, a second sweep, two workgroups of the outer kernel; one feature group at O = 4
    inst = set()
    for T, O in A.THIN_SHAPES:
        pts = A.small_points(T, O)
        pps = A.thin_plan(1, T, O)["pps"]
        assert pps == 1024 // O and {1, 15, 16, 17, 129} <= set(pts) and pps + 1 in pts and (pps == 1 or pps - 1 in pts)
        assert A.thin_plan(pps - 1, T, O)["sweeps_expand"] == 1 and A.thin_plan(pps + 1, T, O)["sweeps_expand"] == 2
        assert A.thin_plan(17, T, O)["sweeps_contract"] == 2 and A.thin_plan(129, T, O)["nb"] == 2
        assert all(A.is_thin(*A.shape_of(r, T, O)) for r in A.ROLES)
        inst.add((T, A.thin_plan(1, T, O)["NQ"]))
    assert len(inst) == 12 and {nq for _, nq in inst} == {1, 2, 4}              # every k_thin_contract<T, NQ>
    assert A.thin_plan(1, 2, 4)["pps"] == 256 and A.thin_plan(1, 2, 8)["pps"] == 128 and A.thin_plan(1, 2, 16)["pps"] == 64
    for T, O in A.REFUSED_SHAPES:
        assert not A.thin_plan(129, T, O)["thin_ok"] and not any(A.is_thin(*A.shape_of(r, T, O)) for r in A.ROLES)


def test_conv_cases_use_the_stated_launches():
    for case, expect in A.CONV_CASES:
        plan = A.conv_plan(*case)
        assert {k: plan[k] for k in expect} == expect, (case, plan)
    assert {A.conv_plan(*c)["CO"] for c, _ in A.CONV_CASES} == {4, 8, 16, 32}
    assert sum(A.conv_more_legs(c) for c, _ in A.CONV_CASES) == 6
    for case, mis in A.CONV_FALLBACKS:
        assert not A.conv_plan(*case, aligned=mis is None)["taken"], case
    assert A.conv_plan(1, 3, 5, (1 << 20) + 4)["taken"] and not A.conv_plan(1, 3, 5, (1 << 20) - 4)["taken"]
    assert not A.conv_plan(65536, 3, 5, 20)["taken"] and not A.conv_plan(1, 513, 17, 1 << 20)["taken"]
    assert A.conv_device((1, 512, 17, 1 << 20), "cuda:0") == "cuda:0"
    assert all(A.conv_device(c, "cuda:0") == "cpu" for c, _ in A.CONV_CASES if c[1] != 512)


# ---------------------------------------------------------------------------------------------------------------------
# the conditions on the problems
# ---------------------------------------------------------------------------------------------------------------------
def _linear_conditions(P, in_f, out_f):
    prob = A.linear_problem("exact", P, in_f, out_f)
    f32 = A.linear_f32(prob)
    for k in ("y", "y0", "dx", "dW", "db"):
        assert torch.equal(f32[k].double(), prob["ref"][k]), (P, in_f, out_f, k)
    prob = A.linear_problem("randn", P, in_f, out_f)
    f32 = A.linear_f32(prob)
    for bias, got in ((True, f32), (False, {"y": f32["y0"]})):          # (the GEMM legs' bounds are these and a margin)
        got = {k: got[k] for k in ("y", "dx", "dW", "db") if k in got}
        figs, miss = A.linear_misses(got, prob, bias=bias)
        assert not miss and all(f <= 0.5 for f, _ in figs.values()), (P, in_f, out_f, bias, figs)


@pytest.mark.parametrize("role", A.ROLES)
@pytest.mark.parametrize("T,O", A.THIN_SHAPES + A.REFUSED_SHAPES)
def test_small_linear_problems_are_exact_and_within_half_the_bounds(role, T, O):
    for P in A.small_points(T, O):
        _linear_conditions(P, *A.shape_of(role, T, O))


LARGE_CASES = [(P, T, O) for P, (shapes, _) in A.LARGE_POINTS.items() for T, O in shapes] + \
              [(8193, T, O) for T, O in A.REFUSED_SHAPES]


@pytest.mark.parametrize("role", A.ROLES)
@pytest.mark.parametrize("P,T,O", LARGE_CASES)
def test_large_linear_problems_are_exact_and_within_half_the_bounds(role, P, T, O):
    _linear_conditions(P, *A.shape_of(role, T, O))


def _cpu_case(case):
    """the case as this file restates it: the device-resident one on 2 x CROSS_POINTS points"""
    B, Cin, Cout, S = case
    return case if A.conv_device(case, "cuda:0") == "cpu" else (B, Cin, Cout, 2 * A.CROSS_POINTS)


@pytest.mark.parametrize("case", [c for c, _ in A.CONV_CASES] + sorted({c for c, _ in A.CONV_FALLBACKS}), ids=str)
def test_conv_problems_are_exact_and_within_half_the_bounds(case):
    more = A.conv_more_legs(case)
    legs = [(*l, True) for l in A.CONV_LEGS + (A.CONV_MORE_LEGS if more else [])]
    legs += [("identity", "identity", 0, False)] if more else []
    for kind in A.KINDS:
        prob = A.conv_problem(kind, _cpu_case(case))
        for act_in, act_out, acc, bias in legs:
            ref, bnd = A.conv_reference(prob, act_in, act_out, acc, bias)
            f32 = A.conv_f32(prob, act_in, act_out, acc, bias)
            if A.conv_is_exact(prob, act_in, act_out):
                assert torch.equal(f32.double(), ref), (case, act_in, act_out, acc, bias)
            else:
                f, i, missed = A.conv_misses(f32, ref, bnd, False)
                assert not missed and f <= 0.5, (case, kind, act_in, act_out, acc, bias, f, i)


# ---------------------------------------------------------------------------------------------------------------------
# planted faults
# ---------------------------------------------------------------------------------------------------------------------
NAN = float("nan")


def _correct(prob):
    if prob["kind"] == "exact":
        return {k: prob["ref"][k].float() for k in ("y", "dx", "dW", "db")}
    f32 = A.linear_f32(prob)
    return {k: f32[k].clone() for k in ("y", "dx", "dW", "db")}


def _caught(got, prob, name, where=None):
    """the check fails on `name` (and, on the randn kind, its worst element is one of `where`) and on nothing else"""
    figs, miss = A.linear_misses(got, prob)
    assert miss == [name], (prob["kind"], name, figs)
    if prob["kind"] == "randn" and where is not None:
        assert figs[name][1] in where, (name, figs[name], sorted(where)[:4])


def _live_point(prob):
    """a point with a non-zero x and a non-zero grad_out entry: leaving it out changes dW and db"""
    ok = (prob["x"] != 0).any(1) & (prob["g"] != 0).any(1)
    return int(torch.nonzero(ok)[-1])


@pytest.mark.parametrize("role", A.ROLES)
def test_planted_faults_in_the_weight_gradient_are_caught(role):
    P, T, O = 129, 3, 64
    in_f, out_f = A.shape_of(role, T, O)
    prob = A.linear_problem("exact", P, in_f, out_f)
    good = _correct(prob)
    assert A.linear_misses(good, prob)[1] == []
    p = _live_point(prob)
    one = torch.outer(prob["g"][p], prob["x"][p])
    for sign in (-1.0, 1.0):                                    # one point left out, one point counted twice
        _caught(dict(good, dW=good["dW"] + sign * one), prob, "dW")
        _caught(dict(good, db=good["db"] + sign * prob["g"][p]), prob, "db")
    ppb = A.thin_plan(P, T, O)["ppb"]                           # the second workgroup's slab added twice
    assert ppb == 65
    slab = prob["g"][ppb:].t() @ prob["x"][ppb:]
    assert bool((slab != 0).any())
    _caught(dict(good, dW=good["dW"] + slab), prob, "dW")


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("role", A.ROLES)
def test_planted_faults_in_the_forward_are_caught(role, kind):
    P, T, O = 129, 4, 256
    in_f, out_f = A.shape_of(role, T, O)
    prob = A.linear_problem(kind, P, in_f, out_f)
    good = _correct(prob)
    assert A.linear_misses(good, prob)[1] == []
    y = good["y"].clone()                                       # the last point's row left at its poison
    y[P - 1] = NAN
    _caught(dict(good, y=y), prob, "y", set(range((P - 1) * out_f, P * out_f)))
    if role == "lifting":                                       # one row of y with two 4-feature groups swapped
        row = 77
        y = good["y"].clone()
        y[row, 8:12], y[row, 132:136] = good["y"][row, 132:136], good["y"][row, 8:12]
        assert not torch.equal(good["y"][row, 8:12], good["y"][row, 132:136])
        _caught(dict(good, y=y), prob, "y", {row * out_f + c for c in (*range(8, 12), *range(132, 136))})
    else:                                                       # contract's y with one 64-feature quarter left out
        q = 2
        part = (prob["x"][:, 64 * q:64 * q + 64].double() @ prob["w"][:, 64 * q:64 * q + 64].double().t()).float()
        assert bool((part != 0).any())
        _caught(dict(good, y=good["y"] - part), prob, "y", set(range(P * out_f)))


@pytest.mark.parametrize("kind", A.KINDS)
def test_planted_faults_in_the_convolution_are_caught(kind):
    case = (3, 5, 5, 1024 + 344)
    B, Cin, Cout, S = case
    assert A.conv_plan(*case)["tail_points"] == 344 and A.conv_plan(*case)["padded"] == 3
    prob = A.conv_problem(kind, case)
    ref, bnd = A.conv_reference(prob, "identity", "identity", 0)
    exact = A.conv_is_exact(prob, "identity", "identity")
    good = ref.float() if exact else A.conv_f32(prob, "identity", "identity", 0, True)
    assert not A.conv_misses(good, ref, bnd, exact)[2]
    out = good.clone()                                          # the last S % 1024 points of one sample unwritten
    out[1, :, 1024:] = NAN
    f, i, missed = A.conv_misses(out, ref, bnd, exact)
    assert missed and (exact or (i // (Cout * S) == 1 and i % S >= 1024)), (f, i)
    out = good.clone()                                          # a padded channel (bias 0, weights 0: zeros) written
    out[2, 0] = 0.0                                             # where channel Cout of sample 1 would lie
    f, i, missed = A.conv_misses(out, ref, bnd, exact)
    assert missed and (exact or i // S == 2 * Cout), (f, i)


# ---------------------------------------------------------------------------------------------------------------------
# the workspace query (a host function: no device needed)
# ---------------------------------------------------------------------------------------------------------------------
def test_linear_workspace_covers_the_slabs():
    from rpde import _lib
    lib = _lib.load()
    for T, O in A.THIN_SHAPES:
        points = A.small_points(T, O) + [P for P, (shapes, _) in A.LARGE_POINTS.items() if (T, O) in shapes] + [131072, 1 << 22]
        for P in points:
            plan = A.thin_plan(P, T, O)
            assert plan["ws_floats"] == plan["nb"] * ((T + 1) * O + 4)
            for role in A.ROLES:
                in_f, out_f = A.shape_of(role, T, O)
                assert int(lib.rpde_linear_ws_bytes(P, in_f, out_f)) >= 4 * plan["ws_floats"], (P, T, O, role)
