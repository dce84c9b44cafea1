"""GPU: the kernels that only the evaluation forward of the channels-first FNO2d reaches -- k_conv_syn_h2<ACT, FULL, LIFT>
(csrc/conv_syn_h2.hip), k_conv_syn_proj_h2<MT, CO, ACT> (csrc/conv_proj_h2.hip), k_conv_mlp_h2<KS, MT, CO>
(csrc/conv_mlp.hip) and the synthesis tail k_conv1x1_small<CO, true> (csrc/conv_small.hip) -- per line and past one pass
per workgroup, on the case tables of tests/eval_cf_ref.py (whose pass arithmetic, coverage, oracle and planted faults
tests/test_eval_cf_ref_cpu.py checks without a device).

The five C entry points are called directly with ctypes in the guarded buffers of tests/ff_abi.py: every tensor, inputs
and weights included, sits between NaN guards, `out` and the workspace are filled with NaN before the call, the workspace
is exactly the queried byte count, and one byte less is refused with RPDE_ERR_WORKSPACE (include/rpde.h's code for a
short workspace) before anything is launched: `out` keeps its poison.

Per case, against float64: guards intact and `out` finite everywhere; whole-tensor relative L2 <= 2e-6 (the bound of the
older tests); the largest error of one line -- a (b, o, m) row of N points, for conv_mlp a tile of 16 points, normalised
as spectral_cf_ref.line_rel does, per sample in the sample-scaled cases -- over EVERY line <= FLOOR_FACTOR = 8 x the same
figure of the float32 CPU oracle; a sample that is exactly zero gives one bit-identical constant per (b, o) plane, within
2e-6 of the tensor's RMS of the float64 constant; two identical calls give identical bits.  Which kernel ran:
RPDE_CONV_SYN_H2=0 changes bits exactly in the syn cases (the h2 tail) and in none of the multiply-add cases, and its
leg meets the same bounds; RPDE_COL_FUSED=0 gives a leg within the same bounds; with RPDE_CONV_PROJ=0 / RPDE_CONV_MLP=0 /
RPDE_CONV_SYN_H2=0 the projection's, the MLP's and the lifted entry's *_ok queries answer 0.

FLOOR_FACTOR = 8 is the project's factor for these sums and stays.  Measured on an MI355X (256 CUs), line figure of the
device / of the float32 oracle per leg (instance: syn = k_conv_syn_h2<ACT, FULL, LIFT>, proj = k_conv_syn_proj_h2<MT, CO,
ACT>, mlp = k_conv_mlp_h2<KS, MT, CO>, fma = k_conv1x1_small<CO, true>; under RPDE_CONV_SYN_H2=0 every syn case runs fma):
    case           instance                      (workgroups, fewest, most passes)  default  SYN_H2=0  COL_FUSED=0   largest rel
    s-1            (syn, gelu, True, False)      (1, 1, 1)         1.27      1.34         0.90   1.74e-07
    s-U-1          (syn, relu, False, False)     (1, 1, 1)         1.42      1.75         1.19   1.70e-07
    s-U+1          (syn, identity, False, False) (2, 1, 1)         0.98      1.14         1.07   1.81e-07
    s-T-1          (syn, gelu, True, False)      (256, 1, 1)       1.05      1.32         2.04   3.69e-07
    s-T            (syn, relu, False, False)     (256, 1, 1)       0.95      1.08         1.72   3.21e-07
    s-T+1          (syn, identity, True, False)  (256, 1, 2)       0.61      0.65         1.11   3.11e-07
    s-3pass        (syn, gelu, True, False)      (256, 2, 3)       0.76      0.94         1.02   2.54e-07
    s-3pass-512    (syn, relu, True, False)      (256, 2, 3)       1.86      1.98         1.86   4.65e-07
    s-3pass-drain  (syn, gelu, False, False)     (256, 2, 3)       0.68      0.72         2.05   4.61e-07
    s-straddle     (syn, gelu, True, False)      (10, 1, 1)        1.08      1.43         1.12   2.12e-07
    s-scaled       (syn, gelu, True, False)      (5, 1, 1)         1.34      2.36         1.26   1.89e-07
    s-zero         (syn, gelu, False, False)     (8, 1, 1)         0.88      0.94         0.91   1.93e-07
    s-n64-r32      (syn, identity, False, False) (3, 1, 1)         1.03      1.34         0.99   1.98e-07
    s-nobias       (syn, relu, True, False)      (9, 1, 1)         1.13      1.13         0.98   1.89e-07
    l-1            (syn, gelu, True, True)       (1, 1, 1)         1.67         -            -   1.84e-07
    l-M9           (syn, gelu, False, True)      (2, 1, 1)         1.25         -            -   1.86e-07
    l-U-1          (syn, gelu, True, True)       (1, 1, 1)         1.32         -            -   1.88e-07
    l-T            (syn, relu, True, True)       (256, 1, 1)       2.18         -            -   1.86e-07
    l-T-1          (syn, gelu, True, True)       (255, 1, 1)       1.66         -            -   1.75e-07
    l-T+1          (syn, identity, True, True)   (256, 1, 2)       1.72         -            -   1.73e-07
    l-3pass        (syn, gelu, True, True)       (256, 2, 3)       0.71         -            -   1.78e-07
    l-M1024        (syn, identity, False, True)  (128, 1, 1)       1.78         -            -   1.59e-07
    l-user-grid    (syn, relu, False, True)      (6, 1, 1)         1.02         -            -   1.62e-07
    l-straddle     (syn, relu, True, True)       (10, 1, 1)        1.34         -            -   1.82e-07
    p-1            (proj, 2, 1, gelu)            (1, 1, 1)         0.98         -         0.94   3.92e-07
    p-U-1          (proj, 2, 4, relu)            (1, 1, 1)         0.98         -         0.93   2.60e-07
    p-U+1          (proj, 4, 1, identity)        (2, 1, 1)         0.77         -         0.87   1.78e-07
    p-T-1          (proj, 4, 4, gelu)            (256, 1, 1)       0.83         -         0.97   2.36e-07
    p-T            (proj, 8, 1, relu)            (256, 1, 1)       2.12         -         2.12   5.18e-07
    p-T+1          (proj, 8, 4, gelu)            (256, 1, 2)       0.69         -         1.24   4.05e-07
    p-3pass        (proj, 8, 1, gelu)            (256, 2, 3)       0.77         -         0.90   3.34e-07
    p-3pass-q4     (proj, 2, 4, identity)        (256, 2, 3)       0.79         -         1.02   2.48e-07
    p-straddle     (proj, 4, 4, gelu)            (5, 1, 1)         0.84         -         0.84   2.52e-07
    p-n512         (proj, 8, 1, gelu)            (3, 1, 1)         0.71         -         0.72   2.04e-07
    p-n1024        (proj, 8, 4, gelu)            (3, 1, 1)         1.51         -         1.48   4.66e-07
    p-scaled       (proj, 4, 1, gelu)            (5, 1, 1)         1.03         -         0.99   2.77e-07
    p-zero         (proj, 2, 4, relu)            (4, 1, 1)         1.18         -         1.16   1.88e-07
    p-nobias       (proj, 8, 4, identity)        (2, 1, 1)         0.93         -         0.82   2.54e-07
    m-1            (mlp, 1, 2, 1)                (1, 1, 1)         0.66         -            -   5.85e-08
    m-U-1          (mlp, 2, 2, 2)                (1, 1, 1)         0.71         -            -   1.39e-07
    m-U+1          (mlp, 1, 4, 4)                (2, 1, 1)         1.15         -            -   1.36e-07
    m-T-1          (mlp, 1, 4, 4)                (2048, 1, 1)      0.52         -            -   1.45e-07
    m-T            (mlp, 2, 4, 1)                (2048, 1, 1)      0.74         -            -   2.17e-07
    m-T+1          (mlp, 1, 8, 2)                (2048, 1, 2)      0.53         -            -   1.69e-07
    m-3pass        (mlp, 1, 8, 1)                (2048, 2, 3)      0.52         -            -   2.02e-07
    m-3pass-co4    (mlp, 1, 2, 4)                (2048, 2, 3)      0.87         -            -   1.41e-07
    m-straddle     (mlp, 2, 2, 4)                (4, 1, 1)         0.89         -            -   1.18e-07
    m-scaled       (mlp, 1, 8, 1)                (5, 1, 1)         0.70         -            -   8.51e-08
    m-zero         (mlp, 1, 4, 4)                (5, 1, 1)         0.63         -            -   1.56e-07
    m-nobias       (mlp, 2, 4, 2)                (4, 1, 1)         0.87         -            -   1.55e-07
    f-n4-co1       (fma, 4, True)                                  1.03      1.03         1.36   1.35e-07
    f-n4-co4       (fma, 4, True)                                  0.49      0.49         1.28   2.14e-07
    f-n32-co5      (fma, 8, True)                                  1.34      1.34         1.46   1.87e-07
    f-n32-co8      (fma, 8, True)                                  1.24      1.24         1.31   2.40e-07
    f-n1024-co9    (fma, 16, True)                                 1.17      1.17         1.20   1.42e-07
    f-n2048-co16   (fma, 16, True)                                 2.81      2.81         2.92   6.15e-07
    f-n1024-co17   (fma, 32, True)                                 1.05      1.05         0.91   1.85e-07
    f-n2048-co32   (fma, 32, True)                                 5.88      5.88         5.88   6.55e-07
    f-zero         (fma, 16, True)                                 1.13      1.13         1.26   1.45e-07
    f-scaled       (fma, 32, True)                                 3.42      3.42         3.42   4.24e-07
Largest: 5.88 (f-n2048-co32), 3.42 (f-scaled), 2.81 / 2.92 (f-n2048-co16); everything else is below 2.4, the h2 kernels
below 2.2 at every pass count.  The three large ones have the cause the sibling file names for its F1 / F2 / G: the floor
is an FFT, the layer's row analysis at N = 1024 / 2048 is an unsplit float32 sum of N terms in index order.  On the CPU,
that one step as a term-by-term float32 accumulation with everything else in float64 reads 5.76 (f-n2048-co32: one input
channel, so nothing else contributes to the floor), 3.54 (f-n2048-co16) and 2.02 (f-scaled) times the floor; summed eight
terms at a time it reads 1.26 / 1.16 / 0.81.  The synthesis tail under test adds nothing visible: the same tail on the h2
cases stays below 2.4.  No case had to be explained away and no kernel fault was found.
The 61 tests take 8 s on the MI355X, the slowest case (p-3pass: 42 MB in, three legs, two float64 passes) 0.73 s.
"""

import pytest
import torch

from tests import eval_cf_ref as E
from tests import spectral_cf_ref as S
from tests.ff_abi import Buffers, Env

pytestmark = pytest.mark.gpu

_ROWS = []          # (case, leg, instance, passes, rel, line, floor line)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n[eval-cf] case, leg, instance, (workgroups, fewest, most passes), whole-tensor rel, line figure / float32 floor")
    for name, leg, inst, geo, rel, line, fl in _ROWS:
        print(f"[eval-cf]   {name:<14} {leg:<18} {str(inst):<46} {str(geo):<14} {rel:.2e} {line / fl:5.2f}")
    worst = sorted(((line / fl, name, leg) for name, leg, _, _, _, line, fl in _ROWS), reverse=True)[:5]
    print("[eval-cf] worst five ratios: " + "; ".join(f"{v:.2f} ({n}, {l})" for v, n, l in worst))
    print("[eval-cf] instances run: " + ", ".join(sorted({str(i) for _, _, i, _, _, _, _ in _ROWS})))


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _call(dev, case, sh, inp, short_ws=False):
    """the case's entry point in guarded, poisoned buffers -> `out` on the CPU (short_ws: the status of a call whose
    workspace is one byte short, and whether `out` kept its poison)"""
    from rpde import _lib
    lib = _lib.load()
    bufs = Buffers(dev)
    g = {k: bufs.new(k, tuple(torch.view_as_real(v).shape) if v.is_complex() else tuple(v.shape),
                     torch.view_as_real(v) if v.is_complex() else v) for k, v in inp.items()}
    p = {k: (g[k].ptr if k in g else None) for k in ("x", "u", "gx", "gy", "wl", "bl", "w1", "w2", "wc", "bc", "pw1", "pb1", "pw2", "pb2")}
    B, M, N, m1, m2 = sh["B"], sh["M"], sh["N"], sh["m1"], sh["m2"]
    act, st = _lib.ACT[case.act], _lib.stream_ptr()
    k = case.kernel
    out = bufs.new("out", (B, case.Cout, sh["S"]) if k == "mlp" else (B, case.Cq if k == "proj" else case.Cout, M, N))
    if k == "mlp":
        assert not short_ws
        status = lib.rpde_conv_mlp_fwd(p["x"], p["pw1"], p["pb1"], p["pw2"], p["pb2"], out.ptr, B, case.Cin, case.Cmid, case.Cout,
                                       sh["S"], act, st)
    else:
        query = lib.rpde_fno2d_lift_block_eval_ws_bytes if k == "lift" else lib.rpde_fnoblock2d_eval_ws_bytes
        nws = int(query(B, case.Cin, case.Cout, M, N, m1, m2))
        assert nws > 0 and nws % 4 == 0
        ws = bufs.new_bytes("ws", nws)
        given = nws - 1 if short_ws else nws
        if k == "lift":
            status = lib.rpde_fno2d_lift_block_eval_fwd(p["u"], p["gx"], p["gy"], p["wl"], p["bl"], p["w1"], p["w2"], p["wc"], p["bc"],
                                                        out.ptr, B, case.Cin, case.Cout, M, N, m1, m2, act, ws.ptr, given, st)
        elif k == "proj":
            status = lib.rpde_fnoblock2d_proj_eval_fwd(p["x"], p["w1"], p["w2"], p["wc"], p["bc"], p["pw1"], p["pb1"], p["pw2"], p["pb2"],
                                                       out.ptr, B, case.Cin, case.Cout, M, N, m1, m2, act, case.Cmid, case.Cq,
                                                       ws.ptr, given, st)
        else:
            status = lib.rpde_fnoblock2d_eval_fwd(p["x"], p["w1"], p["w2"], p["wc"], p["bc"], out.ptr, B, case.Cin, case.Cout, M, N,
                                                  m1, m2, act, ws.ptr, given, st)
    torch.cuda.synchronize()
    if short_ws:
        bufs.check([], f"{case.name} short workspace")
        return status, out.non_finite() == out.n
    _lib.check(status, case.name)
    bufs.check(["out"], case.name)
    return out.t.cpu().clone()


def _judge(case, sh, cus, leg, got, ref, fl, bad):
    figs = E.figures(case, got, ref)
    geo = E.passes(case, sh, cus) if E.unit(case) else ""
    inst = E.instance(case, sh, leg != "RPDE_CONV_SYN_H2=0")
    if inst[0] == "k_conv1x1_small":
        geo = ""
    print(f"[eval-cf] {case.name} {leg}: {inst} passes {geo} rel {figs['rel']:.2e} (floor {fl['rel']:.2e}) "
          f"line {figs['line']:.2e} (floor {fl['line']:.2e}, ratio {figs['line'] / fl['line']:.2f})")
    _ROWS.append((case.name, leg, inst, geo, figs["rel"], figs["line"], fl["line"]))
    if not figs["rel"] <= E.TOL:
        bad.append((leg, "rel", figs["rel"], E.TOL))
    if not figs["line"] <= S.FLOOR_FACTOR * fl["line"]:
        bad.append((leg, "line", figs["line"], "floor", fl["line"], "ratio", figs["line"] / fl["line"]))
    if case.content == "zero":
        const = E.zero_sample_planes(case, ref)
        plane = got[1].reshape(got.shape[1], -1)
        if not bool((plane.view(torch.int32) == plane.view(torch.int32)[:, :1]).all()):
            bad.append((leg, "a plane of the zero sample is not one constant"))
        scale = float(ref.double().square().mean().sqrt())
        miss = float((plane[:, 0].double() - const).abs().max())
        if not miss <= E.TOL * scale:
            bad.append((leg, "the zero sample's constants", miss, E.TOL * scale))


@pytest.mark.parametrize("case", E.ALL_CASES, ids=lambda c: c.name)
def test_evaluation_kernel_against_float64_per_line(gpu_device, case):
    dev = gpu_device
    cus = _cus(dev)
    sh, inp, ref, fl = E.reference(case, cus)
    bad = []
    base = _call(dev, case, sh, inp)
    assert tuple(base.shape) == tuple(ref.shape)
    if not _bits_equal(base, _call(dev, case, sh, inp)):
        bad.append("two identical calls differ")
    _judge(case, sh, cus, "default", base, ref, fl, bad)
    if case.kernel != "mlp":
        status, untouched = _call(dev, case, sh, inp, short_ws=True)
        from rpde import _lib
        if status != _lib.ERR_WORKSPACE or not untouched:
            bad.append(("a workspace one byte short", status, "out untouched" if untouched else "out written"))
    if case.kernel in ("syn", "fma"):
        with Env({"RPDE_CONV_SYN_H2": "0"}):
            got = _call(dev, case, sh, inp)
        _judge(case, sh, cus, "RPDE_CONV_SYN_H2=0", got, ref, fl, bad)
        if _bits_equal(base, got) != (case.kernel == "fma"):
            bad.append("RPDE_CONV_SYN_H2=0: " + ("bit-identical to the default leg: the h2 tail did not run" if case.kernel == "syn"
                                                  else "differs from the default leg: the h2 tail ran where the table has none"))
    if case.kernel in ("syn", "fma", "proj"):
        with Env({"RPDE_COL_FUSED": "0"}):
            got = _call(dev, case, sh, inp)
        _judge(case, sh, cus, "RPDE_COL_FUSED=0", got, ref, fl, bad)
    assert not bad, bad


def test_switches_close_the_queries(gpu_device):
    from rpde import _lib
    lib = _lib.load()
    cus = _cus(gpu_device)
    for var, kernel in (("RPDE_CONV_PROJ", "proj"), ("RPDE_CONV_MLP", "mlp"), ("RPDE_CONV_SYN_H2", "lift")):
        for c in E.TABLES[kernel]:
            q, args = E.ok_query(c, E.resolve(c, cus))
            assert getattr(lib, q)(*args) == 1, (c.name, q)
            with Env({var: "0"}):
                assert getattr(lib, q)(*args) == 0, (var, c.name, q)
