"""GPU: the fused FeedForward (csrc/ff_fused.hip: k_ff3_fwd_h2, k_ff3_bwd_h2) and the streaming weight gradient
(csrc/wgrad_h2.hip: k_wgrad_h2 with and without the riding data gradient) at their tile and chunk edges, driven through
the C ABI by tests/ff_abi.py: guarded buffers, NaN-poisoned outputs and workspaces of exactly the queried size, a float64
oracle, and a float32 CPU evaluation of the same expression as the yardstick of every bound this file adds.  What these
tests rest on is checked without a GPU by tests/test_ff_edges_ref_cpu.py.

FeedForward, dim 64, factor 4, three layers.  A tile is 32 points (two blocks of 16); the kernels launch min(tiles, CUs)
workgroups, so with T = 32 * CUs: P = 32 is the smallest fused shape, 33 / 47 / 48 / 49 / 63 one tile plus one point, a
half tile and its neighbours, T exactly one tile per workgroup, T + 1 one workgroup with two tiles of which the last
holds one point, 2T - 15 two tiles everywhere and a partial last one.  P = 31 takes the per-GEMM path in the same harness.
From P = 8192 the three weight gradients come from k_wgrad_h2, the first layer's with the data gradient riding along
(wgrad_h2_dgrad), below it from the split-K GEMM with linear_dgrad_impl: T - 1 / T / T + 1 straddle that switch too on a
256-CU part.

Per case: guards intact, outputs finite, the project's global bounds (FF_FWD_TOL, FF_GRAD_TOL of
tests/test_gpu_dropout_parity.py), and per point for `out` and `dx` the row's L2 error over the RMS of the reference's
row norms, maximum over rows (and once more over the first row of the last tile and the last P % 32 rows alone), held to
ROW_MARGIN = 16 x the same figure of the float32 CPU evaluation: h2.h bounds a product's error by 3 * 2^-22 = 12 fp32
roundoffs, rounded up for the second split operand of the chain.  The inputs are plain randn without row scaling, which is
what this normalisation fits.  The planted fault -- the oracle with the last point left out of every reduction, what a
kernel that drops the last row or folds a padded one into db / dgamma would give -- must miss every dW, db, dgamma, dbeta
by 100 x FF_GRAD_TOL at P >= T - 1 and 1000 x at P < 64.  Evaluation (hs, ds NULL) and prepare / fwd_prepared give the
training forward's bits at dropout 0; two identical calls give identical bits at P = 33 and T + 1.

The streaming weight gradient alone, through rpde_linear_bwd: the three shapes wgrad_h2_ok accepts at P = 8191 (the GEMM
leg: RPDE_WGRAD_H2=0 changes no bit), 8192 (every chunk one step: prologue and epilogue of the pipeline coincide), 8193
(one two-step chunk, the last, with a one-point step), 8223, 8293, 12345 (one- and two-step chunks mixed), 16369; from
8192 on the two legs differ bitwise, so the test knows which kernel ran.  The last chunk owns ceil(steps / 256) steps, so a
one-step chunk that is also the partial step needs P < 8192, which wgrad_h2_ok refuses: that case cannot be reached.
Content cases at P = 8193 (shaping x) and 12345 (shaping grad_out): a zero prefix, one 64-channel block of exact zeros (its
rows of dW must be exactly 0.0), a one-step chunk closing on a row 2^20 above everything before it, and magnitudes
descending from 2^10 to 2^-20 (on the CPU the float32 matmul meets 2e-6 there, 3.9e-7: the 4 x rule of
ff_abi.wgrad_bound stays unused).  Per column and per row of dW, with channel magnitudes spread over 2^+-8: relative L2
<= 16 x the float32 CPU matmul's figure for the same column or row.  That is inside the documented range only: h2.h keeps
22 bits down to 2^-17 of a block's maximum; a channel more than 2^-17 below its 64-channel panel's maximum loses bits by
design, and the global 2e-6 is what wgrad_h2.hip promises there.

Largest figures seen on an MI355X (256 CUs, T = 8192); no bound had to be derived, every one stands at 16 x:
  per point, fused kernels: out 1.26 x the float32 figure (P = 33, dropout), dx 1.16 x (P = 32); the per-GEMM path at
  P = 31: out 1.20 x, dx 1.38 x.  Absolute: row figure of out <= 7.9e-7, of dx <= 1.13e-6; over the last tile's rows
  alone out <= 4.1e-7, dx <= 7.0e-7.  Global: out <= 3.7e-7 (bound 5e-6), gradients <= 1.41e-6 (bound 2e-5).
  planted fault: smallest miss 6.65e-3 at P = 16369 (2e-3 required), 6.8e-2 at P = 63 (2e-2 required).
  rpde_linear_fwd / _bwd: y <= 2.4e-7, dW <= 1.7e-7 streaming and 2.2e-7 on the GEMM leg, db <= 4.1e-7, dx <= 2.4e-7
  (bound 2e-6); per column of dW 2.48 x the float32 matmul's figure (64 x 256, P = 8193), per row 1.88 x (256 x 64,
  P = 8193).
The whole file takes about 6 s, the slowest case (P = 31, the first to touch the device) 0.7 s."""
import pytest
import torch

from tests import ff_abi as A

pytestmark = pytest.mark.gpu


def _report(name, **kv):
    print(f"\n[ff-edges] {name} " + " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()))


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _tile_points(dev):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert cus <= 1024, cus                               # the clamp in ff3_fused_bwd_launch
    return 32 * cus


def _check_training(name, mode, got, ref, f32, fault, spec, T, leg):
    """one training-mode result against the float64 oracle: global, per point, tail rows, planted fault"""
    P = spec.P
    # which mode ran: the forward saved h = gelu(u) of the first hidden layer, or u = dropout(z) itself to recompute from
    saved = A.rel(got["hs0"], ref["u0"] if mode == "recompute" else torch.nn.functional.gelu(ref["u0"]))
    assert saved < A.FF_FWD_TOL, (mode, "hs[0] is not what this mode saves", saved)
    names = ["out"] + (["dx"] if spec.grad_x else []) + [k for k in A.GRAD_NAMES if k in ref and
                                                         (spec.grad_biases or k not in ("db0", "db1", "db2"))]
    assert set(names) == {k for k in got if k not in ("is_fused", "hs0")}, (sorted(got), names)
    err = {k: A.rel(got[k], ref[k]) for k in names}
    tail = A.tail_rows(P)
    rows = {k: (A.row_fig(got[k], ref[k]), A.row_fig(got[k], ref[k], tail)) for k in ("out", "dx") if k in names}
    miss = A.fault_misses(got, fault)
    need = A.fault_factor(P, T)
    _report(name, is_fused=got["is_fused"], wgrad_leg=leg, fwd=err["out"], f32_fwd=f32["out"],
            grad=max(v for k, v in err.items() if k != "out"), f32_grad=max(f32[k] for k in names if k != "out"),
            **{f"row_{k}": v[0] for k, v in rows.items()}, **{f"tail_{k}": v[1] for k, v in rows.items()},
            **{f"f32_row_{k}": f32["row:" + k] for k in rows},
            **{f"ratio_{k}": max(v) / f32["row:" + k] for k, v in rows.items()},
            min_miss=min(miss.values()), required=(need or 0.0) * A.FF_GRAD_TOL)
    assert err["out"] < A.FF_FWD_TOL, err["out"]
    for k in names[1:]:
        assert err[k] < A.FF_GRAD_TOL, (k, err[k])
    for k, (every, last) in rows.items():
        bound = A.ROW_MARGIN * f32["row:" + k]
        assert every <= bound, (k, "a point's error", every, bound)
        assert last <= bound, (k, "a point of the last tile", last, bound, tail[:2])
    if need is not None:
        for k, m in miss.items():
            assert m >= need * A.FF_GRAD_TOL, ("the check cannot see a dropped last point", k, m)


FF_CASES = A.ff_cases()


@pytest.mark.parametrize("point,variant", FF_CASES, ids=[f"P={p}-{v}" for p, v in FF_CASES])
def test_fused_feedforward_at_tile_edges(gpu_device, point, variant):
    """k_ff3_fwd_h2<0|1|2>, k_ff3_bwd_h2<false|true>, the three weight gradients (split-K GEMM below 8192 points,
    k_wgrad_h2 plain / ACT / with the data gradient from there) and the fold of the per-workgroup sums, per contract"""
    T = _tile_points(gpu_device)
    P = A.resolve_points(point, T)
    spec = A.FFSpec(P=P, **A.FF_VARIANTS[variant])
    prob, ref, f32, fault = A.ff_oracle(spec.oracle_key())
    modes = A.ff_modes(point, variant)
    runs = {m: A.run_ff(gpu_device, prob, spec, m) for m in modes}
    for m, r in runs.items():
        assert r["is_fused"] == (0 if point == "31" else 1), (m, P)
    # the weight gradients' leg: k_wgrad_h2 (layer 0 with the data gradient) from 8192 points, the split-K GEMM and
    # linear_dgrad_impl below.  Where T straddles that switch the test finds out which ran: RPDE_WGRAD_H2=0 changes bits
    # on the streaming leg only
    leg = ("streaming" if P >= A.WG_MIN_P else "gemm") + " (by P)"
    if variant == "base" and point in ("T-1", "T", "T+1"):
        gemm = A.run_ff(gpu_device, prob, spec, "train", env={"RPDE_WGRAD_H2": "0"})
        differ = [k for k in ("dx", "dW0", "dW1", "dW2") if not _bits_equal(gemm[k], runs["train"][k])]
        assert differ == (["dx", "dW0", "dW1", "dW2"] if P >= A.WG_MIN_P else []), (P, differ)
        assert all(_bits_equal(gemm[k], runs["train"][k]) for k in ("out", "db0", "db1", "db2", "dgamma", "dbeta"))
        leg = "streaming" if differ else "gemm"
        _check_training(f"P={P} {variant} train RPDE_WGRAD_H2=0", "train", gemm, ref, f32, fault, spec, T, "gemm")
    for m in modes:
        if m in ("train", "recompute"):
            _check_training(f"P={P} {variant} {m}", m, runs[m], ref, f32, fault, spec, T, leg)
        else:
            # evaluation, in both forms, gives the training forward's bits (no dropout in these cases)
            assert spec.p == 0.0 and _bits_equal(runs[m]["out"], runs["train"]["out"]), (m, P)
            _report(f"P={P} {variant} {m}", is_fused=runs[m]["is_fused"], same_bits_as_training=True)
    if point in A.FF_FULL:
        # no atomics anywhere on this path: two identical calls, identical bits in every output
        for m in ("train", "recompute") if variant in ("base", "dropout") else ("train",):
            again = A.run_ff(gpu_device, prob, spec, m)
            for k, v in runs[m].items():
                if k != "is_fused":
                    assert _bits_equal(v, again[k]), (m, k, "not reproducible")


# ---------------------------------------------------------------------------------------------------------------------
# the streaming weight gradient alone
# ---------------------------------------------------------------------------------------------------------------------
WG_POINTS = [8191, 8192, 8193, 8192 + 31, 8192 + 32 * 3 + 5, 12345, 16369]
WG_CASES = [("plain", P, "every leg and chunk layout") for P in WG_POINTS] + [
    (k, P, why) for k, why in [
        ("zero_prefix", "running exponents start at their floor and first move mid-chunk"),
        ("zero_block", "a 64-channel block of exact zeros: its rows of dW are exactly 0.0"),
        ("huge_closing", "a one-step chunk closes on a row 2^20 larger: the rescale falls on the last step"),
        ("descending", "the running maximum never moves after the first step: a stale, large exponent"),
        ("channel_spread", "per column and per row of dW, channels spread over 2^+-8"),
    ] for P in (8193, 12345)]


@pytest.mark.parametrize("out_f,in_f", A.WGRAD_SHAPES, ids=[f"{o}x{i}" for o, i in A.WGRAD_SHAPES])
@pytest.mark.parametrize("kind,P,why", WG_CASES, ids=[f"{k}-P={P}" for k, P, _ in WG_CASES])
def test_streaming_weight_gradient_at_chunk_edges(gpu_device, kind, P, why, out_f, in_f):
    """rpde_linear_bwd: k_wgrad_h2 (from 8192 points) or the split-K GEMM, the column sums and the data gradient; and
    rpde_linear_fwd on the same operands"""
    prob = A.wgrad_problem(kind, P, out_f, in_f)
    ref, f32 = prob["ref"], prob["f32"]
    got = A.run_linear(gpu_device, prob)
    again = A.run_linear(gpu_device, prob)
    for k in got:
        assert _bits_equal(got[k], again[k]), (k, "not reproducible")
    err = {k: A.rel(got[k], ref[k]) for k in got}
    bound = {k: A.wgrad_bound(kind, f32[k]) for k in got}
    streaming = P >= A.WG_MIN_P
    leg = None
    if kind == "plain":
        gemm = A.run_linear(gpu_device, prob, env={"RPDE_WGRAD_H2": "0"})
        leg = "streaming" if not _bits_equal(gemm["dW"], got["dW"]) else "gemm"
        assert A.rel(gemm["dW"], ref["dW"]) < bound["dW"]
    _report(f"wgrad {kind} P={P} {out_f}x{in_f}", leg=leg or ("streaming" if streaming else "gemm") + " (by P)",
            **err, **{"f32_" + k: v for k, v in f32.items()}, bound=max(bound.values()),
            min_chunk=min(A.chunk_steps(P)), max_chunk=max(A.chunk_steps(P)))
    if leg is not None:
        assert leg == ("streaming" if streaming else "gemm"), (leg, P)
    for k in got:
        assert err[k] < bound[k], (k, err[k], bound[k], why)
    if kind == "zero_block":
        lo, hi = prob["info"]["zero_rows"]
        assert bool((got["dW"][lo:hi] == 0.0).all()) and bool((got["db"][lo:hi] == 0.0).all())
    if kind == "channel_spread":
        cols, rows = A.line_figs(got["dW"], ref["dW"], 0), A.line_figs(got["dW"], ref["dW"], 1)
        rc, rr = cols / prob["info"]["f32_cols"], rows / prob["info"]["f32_rows"]
        _report(f"wgrad {kind} P={P} {out_f}x{in_f} per line", col=float(cols.max()), f32_col=float(prob["info"]["f32_cols"].max()),
                ratio_col=float(rc.max()), row=float(rows.max()), f32_row=float(prob["info"]["f32_rows"].max()),
                ratio_row=float(rr.max()))
        assert float(rc.max()) <= A.ROW_MARGIN, ("a column of dW", int(rc.argmax()), float(rc.max()))
        assert float(rr.max()) <= A.ROW_MARGIN, ("a row of dW", int(rr.argmax()), float(rr.max()))
