"""What tests/test_gpu_ff_edges.py rests on, checked without a GPU on the oracle alone (tests/ff_abi.py), for every point
count, contract variant and content case of that file, at T = 8192 (256 compute units):

  * the float32 CPU evaluation of the FeedForward meets the project's global bounds with room to spare (<= 1/4 of each),
    so a per-row bound of 16 x its figure is a bound the kernels' fp32-class arithmetic can be held to;
  * the planted fault -- the last point left out of every reduction -- moves every dW, db, dgamma, dbeta by at least
    100 x FF_GRAD_TOL at P >= T - 1 and 1000 x at P < 64: a test that cannot see a dropped or a padded row fails;
  * the float32 matmul meets 2e-6 on every content case of the streaming weight gradient, or the case is one of
    ff_abi.FOUR_X_RULE, whose bound is then 4 x the float32 error;
  * the guard and poison helpers see a write one element before and one element after a view, and an element left
    unwritten."""
import pytest
import torch

from tests import ff_abi as A

T = 8192


def _report(name, **kv):
    print(f"\n[ff-edges-ref] {name} " + " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}"
                                                for k, v in kv.items()))


@pytest.mark.parametrize("point,variant", A.ff_cases(), ids=[f"P={p}-{v}" for p, v in A.ff_cases()])
def test_float32_margin_and_planted_fault(point, variant):
    P = A.resolve_points(point, T)
    spec = A.FFSpec(P=P, **A.FF_VARIANTS[variant])
    prob, ref, f32, fault = A.ff_oracle(spec.oracle_key())
    assert f32["out"] <= A.FF_FWD_TOL / 4, f32["out"]
    for k in ["dx"] + [n for n in A.GRAD_NAMES if n in ref]:
        assert f32[k] <= A.FF_GRAD_TOL / 4, (k, f32[k])
    assert ("dgamma" in ref) == spec.layer_norm
    miss = A.fault_misses(ref, fault)
    assert set(miss) == {n for n in A.GRAD_NAMES if n in ref}
    need = A.fault_factor(P, T)
    if need is not None:
        for k, m in miss.items():
            assert m >= need * A.FF_GRAD_TOL, (k, m)
    _report(f"P={P} {variant}", f32_out=f32["out"], f32_grad=max(f32[k] for k in miss), f32_row_out=f32["row:out"],
            f32_row_dx=f32["row:dx"], min_miss=min(miss.values()), required=(need or 0.0) * A.FF_GRAD_TOL)


def test_point_counts_cover_the_tile_and_chunk_edges():
    """the cases are the ones the kernels' launch geometry makes special"""
    Ps = {n: A.resolve_points(n, T) for n in A.FF_POINTS}
    assert Ps["T"] == 32 * 256 and Ps["2T-15"] == 16369 and Ps["T+1"] == 8193
    assert all(A.fault_factor(P, T) is not None for P in Ps.values() if P < 64 or P >= T - 1)
    for modes in (A.ff_modes(p, v) for p, v in A.ff_cases()):
        assert modes[0] == "train" and len(modes) >= 2
    seen = {m: [p for p, v in A.ff_cases() if m in A.ff_modes(p, v)] for m in A.FF_MODES}
    assert all(len(set(ps)) >= 4 for ps in seen.values()), seen
    # the streaming kernel's chunks: one step each at 8192, one two-step chunk (the last, with the partial step) at
    # 8193, a mix at 12345, two each at 16369.  The last chunk owns ceil(steps / 256) steps, so a one-step chunk is the
    # partial step only at P < 8192, which wgrad_h2_ok refuses: that case of the kernel cannot be reached.
    assert set(A.chunk_steps(8192)) == {1}
    assert A.chunk_steps(8193) == [1] * 255 + [2]
    assert set(A.chunk_steps(8192 + 31)) == {1, 2} and set(A.chunk_steps(12345)) == {1, 2}
    assert set(A.chunk_steps(16369)) == {2}
    for P in WG_POINTS:
        assert sum(A.chunk_steps(P)) == (P + 31) // 32 and min(A.chunk_steps(P)) >= 1
    for P in (8193, 12345):
        s = A.one_step_chunk(P)
        steps = (P + 31) // 32
        c = [c for c in range(256) if steps * c // 256 == s][0]
        assert A.chunk_steps(P)[c] == 1 and 32 * s + 31 < P


WG_POINTS = [8191, 8192, 8193, 8192 + 31, 8192 + 32 * 3 + 5, 12345, 16369]
WG_CONTENT = [(k, P) for k in A.WGRAD_KINDS if k != "plain" for P in (8193, 12345)]


@pytest.mark.parametrize("out_f,in_f", A.WGRAD_SHAPES)
@pytest.mark.parametrize("kind,P", [("plain", P) for P in WG_POINTS] + WG_CONTENT)
def test_float32_matmul_on_the_weight_gradient_cases(kind, P, out_f, in_f):
    prob = A.wgrad_problem(kind, P, out_f, in_f)
    f32 = prob["f32"]
    bounds = {k: A.wgrad_bound(kind, f32[k]) for k in f32}
    for k in f32:
        if kind in A.FOUR_X_RULE:
            assert bounds[k] == (A.WGRAD_TOL if f32[k] <= A.WGRAD_TOL else 4 * f32[k])
        else:
            assert f32[k] <= A.WGRAD_TOL and bounds[k] == A.WGRAD_TOL, (k, f32[k])
    if kind == "zero_block":
        lo, hi = prob["info"]["zero_rows"]
        assert float(prob["ref"]["dW"][lo:hi].abs().max()) == 0.0
    if kind == "channel_spread":
        # inside the documented range: every channel within 2^-17 of its 64-channel panel's maximum
        for t in (prob["x"], prob["g"]):
            m = t.abs().amax(0).reshape(-1, 64)
            assert float((m.amin(1) / m.amax(1)).min()) > 2.0 ** -17
        # the per-column / per-row bounds are multiples of these: none may vanish, all are fp32-class
        for figs in (prob["info"]["f32_cols"], prob["info"]["f32_rows"]):
            assert float(figs.min()) > 0.0 and float(figs.max()) < 1e-5, (float(figs.min()), float(figs.max()))
    _report(f"{kind} P={P} {out_f}x{in_f}", four_x=any(b != A.WGRAD_TOL for b in bounds.values()), **f32)


def test_backward_without_stored_derivatives_is_refused_only_off_the_fused_path():
    """rpde.h: ds NULL is the fused path's recompute mode.  The per-GEMM path needs the stored derivatives and says so
    before any device work (nothing is dereferenced or launched here); the fused shape with ds NULL is accepted, which
    only the GPU tests can show (`recompute` in tests/test_gpu_ff_edges.py passes NULL, not an array of NULLs)"""
    import ctypes as C
    from rpde import _lib
    lib = _lib.load()
    fake = 4096                                                       # an aligned non-null address, never read
    wa = (C.c_void_p * 3)(fake, fake, fake)
    hs = (C.c_void_p * 2)(fake, fake)
    PP = C.POINTER(C.c_void_p)

    def bwd(dim, hs_, ds_):
        fp = _lib.FFParams(3, dim, 4, 1, 1e-5, 0.0, 1, 0, C.cast(wa, PP), C.cast(wa, PP), fake, fake, None)
        return lib.rpde_feedforward_bwd(C.byref(fp), fake, hs_, ds_, fake, fake, None, None, None, None, None, 33, None, 0,
                                        None)
    assert lib.rpde_feedforward_is_fused(32, 4, 3, 33) == 0 and lib.rpde_feedforward_is_fused(64, 4, 3, 33) == 1
    assert bwd(32, C.cast(hs, PP), None) == _lib.ERR_ARG and b"saved hidden tensors missing" in lib.rpde_last_error()
    assert bwd(32, None, None) == _lib.ERR_ARG and b"saved hidden tensors missing" in lib.rpde_last_error()
    assert bwd(64, None, None) == _lib.ERR_ARG and b"saved hidden tensors missing" in lib.rpde_last_error()
    # the fused shape with hs and ds NULL gets past that check: the next verdict is the workspace's (none was given)
    assert bwd(64, C.cast(hs, PP), None) == _lib.ERR_WORKSPACE, lib.rpde_last_error()


def test_guards_and_poison_detect_a_stray_write_and_a_missing_one():
    g = A.Guarded("v", (5, 7), "cpu")
    assert g.raw.numel() == 2 * (A.GUARD_BYTES // 4) + 35 and A.GUARD_BYTES >= 32 * 256 * 4
    assert g.broken_guards() == [] and g.non_finite() == 35          # poisoned: every element a NaN
    g.t.zero_()
    assert g.broken_guards() == [] and g.non_finite() == 0
    flat = g.raw.view(torch.float32)
    n_guard = A.GUARD_BYTES // 4
    flat[n_guard - 1] = 0.0                                           # one element before the view
    bad = g.broken_guards()
    assert len(bad) == 1 and "before" in bad[0] and "element -1" in bad[0]
    g.raw[n_guard - 1] = A._GUARD_I32
    flat[n_guard + 35] = 1.0                                          # one element after it
    bad = g.broken_guards()
    assert len(bad) == 1 and "after" in bad[0] and "element 35" in bad[0]
    g.raw[n_guard + 35] = A._GUARD_I32
    assert g.broken_guards() == []
    g.poison()
    g.t[:4].zero_()                                                   # "did not store the last row"
    assert g.non_finite() == 7
    # the guard word is a NaN of its own: a read past the view is not a lucky zero, and it is not the poison
    assert bool(torch.isnan(flat[0])) and int(g.raw[0]) != -1
    bufs = A.Buffers("cpu")
    a = bufs.new("a", (3, 4))
    b = bufs.new("b", (3, 4), src=torch.ones(3, 4))
    ws = bufs.new_bytes("ws", 512)
    assert ws.nbytes == 512 and not b.non_finite() and ws.non_finite() == 128
    a.t.fill_(2.0)
    bufs.check(["a", "b"], "clean")
    with pytest.raises(AssertionError):
        bufs.check(["a", "ws"], "workspace still poisoned")
    a.raw[n_guard + 12] = 0
    with pytest.raises(AssertionError):
        bufs.check(["a"], "stray write")
    assert A.tail_rows(33) == [32] and A.tail_rows(64) == [32] and A.tail_rows(8223) == list(range(8192, 8223))
