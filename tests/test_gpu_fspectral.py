"""The channels-last FFNO spectral layers -- rpde.ops.fspectral2d / fspectral1d (csrc/fspectral.hip, fused_spectral.hip,
fused_mix.hip, mix1d.hip) -- against oracle.reference_path in float64 under autograd, forward and every gradient, on the
case tables of tests/fspectral_ref.py: one case per dispatch branch (see the comments there).

Legs.  A fused 2-D case runs the default leg, RPDE_FUSED_SPECTRAL=0, RPDE_FUSED_MIX=0, RPDE_ANA_SQ=0 on square grids and
RPDE_SYN3=0 on grids of 64-multiples, each against float64; the per-axis 2-D cases and the 1-D cases run the default leg
(RPDE_MIX1D is read once per process: the GEMM mix is reached through shapes).  The legs also show which branch ran: a
switched-off leg differs in bits from the default leg where the case is there for the fast path and is bit-identical where
it is not (fspectral_ref.legs); the default leg run twice is bit-identical.  The h2 tables of a plan do not depend on the
switches (core.hip build_plan builds them with the plan), so no leg can leave a crippled plan behind; the default leg
runs first all the same.

Bounds (fspectral_ref.check, the same function the CPU suite plants faults into).  Whole tensor: rel <= 2e-6 forward,
<= 5e-6 gradients.  The largest point error of out / dx per sample (point_rel) and the largest mode error of the weight
gradients (mode_rel) are held to FLOOR_FACTOR times the error of the same oracle run in float32 on the CPU with the same
inputs.  Modes >= keff of an axis must be exactly zero; everything must be finite.

FLOOR_FACTOR started at 4.  Measured on an MI355X, device / float32 floor (out.point_rel dx.point_rel worst mode_rel):
    case        default leg          largest over all legs, skip variants, gradient subsets and the prepared run
    F-nyq       0.87  0.84  0.86     0.93  0.94  1.15
    F-r8        0.98  0.97  0.94     1.18  1.25  0.95
    F-r40       0.99  1.00  0.89     1.12  1.15  0.90
    F-r48       0.94  1.03  0.97     1.07  1.16  0.97
    F-rect24    0.95  0.90  1.10     1.12  1.04  1.56
    F-rect16    0.97  0.99  1.25     1.25  1.24  1.25
    F-r32       0.92  0.88  1.02     1.09  1.08  1.52
    F-many      0.88  1.04  0.91     1.11  1.24  0.98
    F-small     0.85  0.88  0.79     1.04  1.08  0.82
    F-chunk     1.21  1.16  1.10     1.45  1.45  1.28
    F-ramp      1.10  1.12  1.35     1.17  1.24  1.35
    F-smooth    0.77  1.06  0.98     1.07  1.62  1.11
    F-lowpass   1.11  1.07    -      1.28  1.32    - 
    G-clamp     1.02  0.97  1.36     1.02  0.97  1.36
    G-odd       1.06  1.09  1.04     1.06  1.09  1.04
    G-mix1d     0.92  0.89  1.29     0.92  0.89  1.29
    G-gemm32    0.96  0.97  0.93     0.96  0.97  0.93
    G-c48       1.29  1.21  1.06     1.29  1.21  1.06
    G-tall      1.21  1.21  1.93     1.21  1.21  1.93
    G-lowpass   0.98  1.01    -      0.98  1.04    - 
    H-bwd       1.03  0.95  1.64     1.03  0.95  1.64
    H-fwd       1.21  1.32  1.29     1.21  1.32  1.29
    H-rows      1.16  1.28  1.36     1.16  1.28  1.36
    H-c48       1.19  1.18  1.24     1.19  1.18  1.24
    H-lowpass   1.28  1.25    -      1.28  1.25    - 
Largest: point_rel 1.62 (F-smooth, RPDE_FUSED_SPECTRAL=0, dx), mode_rel 1.93 (G-tall, dWx); twice either fits under 4, so
FLOOR_FACTOR = 4.

The first run of this suite measured mode_rel ratios of 4 to 16 on the default leg of every fused case whose samples differ
in magnitude (F-r32 16.1, F-nyq 15.1, F-r48 13.0, F-chunk 10.4, F-r8 and F-rect16 9.0, F-many 5.9, F-r40 5.3, F-small 3.9)
against 0.7 to 1.6 on the RPDE_FUSED_MIX=0 and RPDE_FUSED_SPECTRAL=0 legs and on the cases without a sample scale
(F-rect24, F-ramp, F-smooth).  Cause: k_mix_wgrad_h2 scaled each tensor by ONE power of two per axis, so a sample 2^20
below its neighbour in x (and as far above it in the cotangent) kept 2^-19 per element.  Fixed in csrc/fused_mix.hip (a pair
of scales per line with a constant product); the table above is measured with the fix.
"""
import os

import pytest
import torch

from tests import fspectral_ref as S

pytestmark = pytest.mark.gpu

_ROWS = []          # (case, leg, {statistic: device / floor})


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    print("\n[fspectral] device / float32 floor: case, leg, out.point_rel, dx.point_rel, worst mode_rel")
    for name, leg, r in _ROWS:
        modes = [v for k, v in r.items() if k.endswith("mode_rel")]
        print(f"[fspectral]   {name:<12} {leg:<30} {r.get('out.point_rel', float('nan')):5.2f} "
              f"{r.get('dx.point_rel', float('nan')):5.2f} {max(modes) if modes else float('nan'):5.2f}")
    worst = sorted(((v, name, leg, k) for name, leg, r in _ROWS for k, v in r.items()), reverse=True)[:5]
    print("[fspectral] worst five: " + "; ".join(f"{v:.2f} ({n}, {l}, {k})" for v, n, l, k in worst))


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _device(case, dev, with_skip, need_x=True, need_w=True):
    """the product path on the inputs of the oracle, loss <out, g> + <skip, g2> -> the oracle's result names, on the CPU"""
    from rpde import ops
    inp = S.inputs(case)
    t = {k: v.to(dev) for k, v in inp.items()}
    t["x"].requires_grad_(need_x)
    for k in S.GRADS:
        if k in t:
            t[k].requires_grad_(need_w)
    K = case.dims[-1]
    if case.kind == "2d":
        res = ops.fspectral2d(t["x"], t.get("wy"), t.get("wx"), K, mode=case.mode, with_skip=with_skip)
    else:
        res = ops.fspectral1d(t["x"], t.get("w"), K, mode=case.mode, norm=case.norm, with_skip=with_skip)
    out, skip = res if with_skip else (res, None)
    loss = (out * t["g"]).sum()
    if with_skip and need_x:
        loss = loss + (skip * t["g2"]).sum()
    loss.backward()
    got = {"out": out.detach()}
    if need_x:
        got["dx"] = t["x"].grad
    if need_w:
        got.update({S.GRADS[k]: t[k].grad for k in S.GRADS if k in t})
    assert all(v is not None for v in got.values()), [k for k, v in got.items() if v is None]
    return {k: v.cpu() for k, v in got.items()}


def _differs(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


def _judge(case, leg, got, with_skip, bad):
    ref, fl = S.oracle(case, with_skip), S.floor(case, with_skip)
    st = S.stats(case, got, ref)
    tag = f"{leg}{' +skip' if with_skip else ''}"
    for k, s in st.items():
        print(f"[fspectral] {case.name} {tag} {k}: " + " ".join(
            f"{n} {v:.2e} (floor {fl[k][n]:.2e})" if n != "stray" else f"stray {v:.1e}" for n, v in s.items() if n != "finite"))
    _ROWS.append((case.name, tag, S.ratios(st, fl)))
    bad.extend((tag,) + b for b in S.check(st, fl, case))


def _run_legs(dev, case):
    bad = []
    full = {"out", "dx"} | (set(S.keffs(case)) if case.mode == "full" else set())
    base = {}
    for skip in S.skips(case):
        base[skip] = _device(case, dev, skip)
        assert set(base[skip]) == full
        if _differs(base[skip], _device(case, dev, skip)):
            bad.append(("default", skip, "two identical calls differ"))
        _judge(case, "default", base[skip], skip, bad)
    for var, want in S.legs(case):
        diff = []
        for skip in S.skips(case):
            with _env(**{var: "0"}):
                got = _device(case, dev, skip)
            _judge(case, var + "=0", got, skip, bad)
            diff += _differs(base[skip], got)
        print(f"[fspectral] {case.name} {var}=0: differs from the default leg in {sorted(set(diff))}, expected {want}")
        if want == "differ" and not diff:
            bad.append((var + "=0", "bit-identical to the default leg: the fast path did not run"))
        if want == "same" and diff:
            bad.append((var + "=0", "differs from the default leg where the switch must not matter", diff))
    assert not bad, bad


@pytest.mark.parametrize("case", S.CASES_2D, ids=lambda c: c.name)
def test_fspectral2d_against_float64(gpu_device, case):
    _run_legs(gpu_device, case)


@pytest.mark.parametrize("case", S.CASES_1D, ids=lambda c: c.name)
def test_fspectral1d_against_float64(gpu_device, case):
    _run_legs(gpu_device, case)


@pytest.mark.parametrize("name", ["F-r40", "G-odd", "H-bwd"])
def test_gradient_subsets_against_float64(gpu_device, name):
    """the first layer of a model wants no dx, a frozen-weight fine-tune no weight gradient: fused2d_bwd takes hwg without
    hmix (gx == NULL) and hmix without hwg (gwy == gwx == NULL), axis_bwd its `if (gw)` / `if (gx)` guards.  Same bounds;
    the x-only backward carries the skip gradient"""
    case = S.by_name(name)
    bad = []
    got = _device(case, gpu_device, True, need_x=True, need_w=False)
    assert set(got) == {"out", "dx"}
    _judge(case, "x only", got, True, bad)
    skip = case.kind == "1d"
    got = _device(case, gpu_device, skip, need_x=False, need_w=True)
    assert set(got) == {"out"} | set(S.keffs(case))
    _judge(case, "weights only", got, skip, bad)
    assert not bad, bad


@pytest.mark.parametrize("name", ["F-r8", "F-r40", "G-odd"])
def test_prepared_evaluation_against_float64(gpu_device, name):
    """inside ops.frozen_weights() under no_grad the fused shapes run rpde_fspectral2d_prepare once and then
    rpde_fspectral2d_fwd_prepared: the forward bounds against float64, and the bits of the training-path forward.  G-odd has
    nothing to prepare (rpde_fspectral2d_prep_bytes == 0) and takes the ordinary path with the same result"""
    from rpde import ops
    from rpde._lib import load
    case = S.by_name(name)
    B, M, N, C, K = case.dims
    assert (load().rpde_fspectral2d_prep_bytes(M, N, C, K) > 0) == S.fused_ok(case)
    base = _device(case, gpu_device, False)["out"]
    t = {k: v.to(gpu_device) for k, v in S.inputs(case).items()}
    with torch.no_grad(), ops.frozen_weights():
        first = ops.fspectral2d(t["x"], t["wy"], t["wx"], K)
        entries = len(ops._FROZEN)
        second = ops.fspectral2d(t["x"], t["wy"], t["wx"], K)
        assert len(ops._FROZEN) == entries == (1 if S.fused_ok(case) else 0)
    bad = []
    _judge(case, "prepared", {"out": first.cpu()}, False, bad)
    assert not bad, bad
    assert torch.equal(first.cpu(), base) and torch.equal(second.cpu(), base)
