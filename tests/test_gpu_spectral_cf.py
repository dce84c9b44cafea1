"""The channels-first FNO operators -- rpde.ops.spectral1d / spectral2d, conv1x1 with its activation prologue, and the
FNOBlock pre-activation built from them -- against oracle.reference_path in float64 under autograd, forward and every
gradient, on the case tables of tests/spectral_cf_ref.py: one case per dispatch branch of csrc/cf_dft.hip (h2 streaming
kernel or GEMM, separately for analysis, synthesis and their adjoints), csrc/spectral_cf.hip (two-launch column stage or
the three steps; slab depth, workgroup size, staging chunks and ky0 passes of k_cmix) and the reduction splits of the
thin GEMMs and of rpde_conv1x1_bwd.

Every spectral case runs three legs, each against float64: the default, RPDE_FUSED_CF=0 and RPDE_COL_FUSED=0.  The legs
also show which branch ran: a switched-off leg differs in bits from the default leg where the case is there for the fast
path and is bit-identical where it is not (Case.cf / Case.col); the default leg run twice is bit-identical.  (A plan
built while RPDE_FUSED_CF is off never gets its h2 tables and stays cached for the process, so the default leg runs
first.)

Bounds.  Whole tensor: rel <= 2e-6 forward, <= 5e-6 gradients.  A whole-tensor norm cannot see one wrong line among
thousands or one wrong mode of a weight gradient (tests/test_spectral_cf_ref_cpu.py), so the largest line error of
out / dx (line_rel) and the largest mode error of the weight gradients (mode_rel) are held to FLOOR_FACTOR times the
error of the same oracle run in float32 on the CPU with the same inputs; a mode whose float64 gradient is exactly zero
(a weights1 slot that weights2 overwrites) must stay below 1e-6 of the RMS mode norm.

FLOOR_FACTOR started at 4.  Measured on an MI355X, device / float32 floor:
    case        default            RPDE_FUSED_CF=0    RPDE_COL_FUSED=0      (each: out.line_rel dx.line_rel worst mode_rel)
    A           0.98 1.31 1.44   1.32 1.66 1.97   1.04 1.31 1.50
    B           1.13 1.49 1.24   1.32 1.68 1.68   1.27 1.49 1.32
    C           1.13 1.28 1.80   1.13 1.28 1.80   1.17 1.28 1.85
    D           0.93 1.59 1.58   1.36 2.37 2.19   1.25 1.59 1.88
    D-gelu      3.08 1.42 3.63   2.60 2.09 3.54   3.23 1.42 4.29
    D-relu      2.31 1.62 4.61   2.25 2.36 4.65   2.60 1.62 5.46
    E           0.94 0.89 0.93   0.94 0.89 0.93   0.86 0.89 0.99
    F1          0.88 4.38 5.46   0.88 4.38 5.46   3.48 4.38 6.20
    F2          3.20 3.46 7.74   3.20 3.46 7.74   3.20 3.46 7.74
    G           0.91 1.19 1.54   4.33 4.03 6.88   1.07 1.19 1.88
    H           1.04 1.39 1.30   3.34 3.07 3.45   1.19 1.39 1.41
    I           1.17 1.81 3.25   1.17 1.81 3.25   1.32 1.81 2.92
    J           1.46 1.52 1.73   1.46 1.52 1.73   1.46 1.52 1.73
    K           1.18 1.54 1.51   1.18 1.54 1.51   1.31 1.54 1.73
    L           1.03 1.05 0.97   1.03 1.05 0.97   1.10 1.05 1.07
    C-gelu      1.44 1.45 2.42   1.44 1.45 2.42   1.70 1.45 2.90
    n1024       1.06 1.09 1.19   1.06 1.09 1.19   1.06 1.09 1.19
    n512        0.97 1.11 1.43   1.06 1.30 1.24   0.97 1.11 1.43
    n128        0.79 2.29 1.47   1.33 2.39 1.55   0.79 2.29 1.47
    n48         1.30 1.34 1.05   1.30 1.34 1.05   1.30 1.34 1.05
    n384-relu   1.71 1.63 1.10   1.71 1.63 1.10   1.71 1.63 1.10
    n16         1.06 0.98 0.97   1.06 0.98 0.97   1.06 0.98 0.97
    block A (gelu)  1.04 0.99 2.14      block D (gelu)  1.03 0.94 3.63
    conv1x1, 21 runs: out.line_rel and gx.line_rel between 0.68 and 1.11
Largest: line_rel 4.38 (F1, dx), mode_rel 7.74 (F2, dW2); twice either is past the cap of 8, so FLOOR_FACTOR = 8 for both.
Every ratio above 4 has one cause: the floor is an FFT, whose rounding error grows like sqrt(log n), the layer sums
dense float32 DFT rows, whose error grows like sqrt(n).
    F1, F2                 the column DFT over M = 1024 is a 2048-term float32 sum per mode
    G, RPDE_FUSED_CF=0     the unsplit GEMM over N = 1024 on 24 lines (the h2 kernel, which folds 128-point chunks, stays at
                           1.5 on the same grid, the 16-way split reduction of n1024 at 1.2)
    D-gelu, D-relu         act(x) has a mean of half its RMS, so the modes of row 0 / column 0 are small differences of
                           large partial sums; identity on the same grid (D) stays at 2.4
The same dense float32 products on the CPU stand in the same place against the FFT: worst mode of the retained spectra
5.1 (F2), 6.3 (D-relu), 5.2 (D-gelu), against 2.7 (D).
"""
import math
import os

import pytest
import torch

from tests import spectral_cf_ref as S

pytestmark = pytest.mark.gpu

_ROWS = []          # (case, leg, {statistic: device / floor})


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    print("\n[spectral_cf] device / float32 floor: case, leg, out.line_rel, dx.line_rel, worst mode_rel")
    for name, leg, r in _ROWS:
        modes = [v for k, v in r.items() if k.endswith("mode_rel")]
        print(f"[spectral_cf]   {name:<22} {leg:<17} {r.get('out.line_rel', float('nan')):5.2f} "
              f"{r.get('dx.line_rel', float('nan')):5.2f} {max(modes) if modes else float('nan'):5.2f}")
    worst = sorted(((v, name, leg, k) for name, leg, r in _ROWS for k, v in r.items()), reverse=True)[:3]
    print("[spectral_cf] worst three: " + "; ".join(f"{v:.2f} ({n}, {l}, {k})" for v, n, l, k in worst))


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


def _device(kind, inp, act, dev):
    """the product path on the inputs of the oracle -> the oracle's result names, on the CPU"""
    from rpde import ops
    t = {k: v.to(dev).requires_grad_(k != "g") for k, v in inp.items()}
    if kind == "2d":
        out, params = ops.spectral2d(t["x"], t["w1"], t["w2"], act), {"dW1": "w1", "dW2": "w2"}
    elif kind == "1d":
        out, params = ops.spectral1d(t["x"], t["w"], act), {"dW": "w"}
    elif kind == "conv":
        out = ops.conv1x1(t["x"], t["w"], t.get("b"), act, acc=t.get("acc"))
        params = {"gw": "w", **({"gb": "b"} if "b" in t else {}), **({"gacc": "acc"} if "acc" in t else {})}
    else:
        out = ops.conv1x1(t["x"], t["wc"], t["bc"], act, acc=ops.spectral2d(t["x"], t["w1"], t["w2"], act), acc_owned=True)
        params = {"dW1": "w1", "dW2": "w2", "gw": "wc", "gb": "bc"}
    out.backward(t["g"])
    res = {"out": out.detach(), "dx": t["x"].grad}
    res.update({k: t[v].grad for k, v in params.items()})
    return {k: v.cpu() for k, v in res.items()}


def _same(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


def _judge(name, leg, kind, got, ref, fl, bad):
    row = {}
    for k, s in S.stats(kind, got, ref).items():
        g = got[k]
        if tuple(g.shape) != tuple(ref[k].shape) or not bool(torch.isfinite(torch.view_as_real(g) if g.is_complex() else g).all()):
            bad.append((leg, k, "shape or not finite"))
            continue
        tol = S.FWD_TOL if k == "out" else S.GRAD_TOL
        line = f"[spectral_cf] {name} {leg} {k}:"
        if "rel" in s:
            line += f" rel {s['rel']:.2e} (floor {fl[k]['rel']:.2e})"
            if not s["rel"] <= tol:
                bad.append((leg, k, "rel", s["rel"], tol))
        for stat in ("line_rel", "mode_rel"):
            if stat not in s or (s[stat] == 0.0 and fl[k][stat] == 0.0):      # (no live mode: dW1 of case L)
                continue
            row[f"{k}.{stat}"] = s[stat] / fl[k][stat] if fl[k][stat] > 0 else math.inf
            line += f" {stat} {s[stat]:.2e} (floor {fl[k][stat]:.2e}, ratio {row[f'{k}.{stat}']:.2f})"
            if not s[stat] <= S.FLOOR_FACTOR * fl[k][stat]:
                bad.append((leg, k, stat, s[stat], "floor", fl[k][stat]))
        if s.get("zero"):
            line += f" {len(s['zero'])} zero modes, stray {s['stray']:.1e}"
            if not s["stray"] <= S.VANISH:
                bad.append((leg, k, "should vanish", s["stray"]))
        print(line)
    _ROWS.append((name, leg, row))


def _run_legs(dev, kind, case, inp):
    ref = S.run_oracle(kind, inp, case.act)
    fl = S.floor(kind, inp, case.act, ref)
    bad = []
    base = _device(kind, inp, case.act, dev)
    if _same(base, _device(kind, inp, case.act, dev)):
        bad.append("two identical calls differ")
    _judge(case.name, "default", kind, base, ref, fl, bad)
    for var, want in (("RPDE_FUSED_CF", case.cf), ("RPDE_COL_FUSED", case.col)):
        with _env(**{var: "0"}):
            got = _device(kind, inp, case.act, dev)
        _judge(case.name, var + "=0", kind, got, ref, fl, bad)
        diff = _same(base, got)
        if want == "differ" and not diff:
            bad.append((var + "=0", "bit-identical to the default leg: the fast path did not run"))
        if want == "same" and diff:
            bad.append((var + "=0", "differs from the default leg: a fast path ran where none is expected", diff))
    assert not bad, bad


@pytest.mark.parametrize("case", S.CASES_2D, ids=lambda c: c.name)
def test_spectral2d_against_float64(gpu_device, case):
    _run_legs(gpu_device, "2d", case, S.inputs_2d(case))


@pytest.mark.parametrize("case", S.CASES_1D, ids=lambda c: c.name)
def test_spectral1d_against_float64(gpu_device, case):
    _run_legs(gpu_device, "1d", case, S.inputs_1d(case))


@pytest.mark.parametrize("shape", S.CONV_SHAPES, ids=lambda s: "x".join(map(str, s[:3] + tuple(s[3]))))
def test_conv1x1_against_float64(gpu_device, shape):
    """out, gx, gw and gb for every activation prologue, with and without bias, and once accumulating into `acc`: the
    gradient of `acc` is the cotangent itself, bit for bit.  out and gx are held line by line like the spectral layers"""
    bad = []
    name = "conv " + "x".join(map(str, shape[:3] + tuple(shape[3])))
    runs = [(act, bias, False) for act in S.ACTS for bias in (True, False)] + [("gelu", True, True)]
    for act, bias, acc in runs:
        inp = S.inputs_conv(shape, bias, acc)
        ref = S.run_oracle("conv", inp, act)
        fl = S.floor("conv", inp, act, ref)
        got = _device("conv", inp, act, gpu_device)
        assert set(got) == {"out", "dx", "gw"} | ({"gb"} if bias else set()) | ({"gacc"} if acc else set())
        _judge(name, f"{act}{' bias' if bias else ''}{' acc' if acc else ''}", "conv", got, ref, fl, bad)
        if acc and not torch.equal(got["gacc"], inp["g"]):
            bad.append((act, "the gradient of acc is not the cotangent"))
    assert not bad, bad


@pytest.mark.parametrize("case", S.BLOCK_CASES, ids=lambda c: c.name)
def test_block_preactivation_against_float64(gpu_device, case):
    """SpectralConv2d(gelu(x)) + Conv1x1(gelu(x)) + b with the convolution accumulating in place into the spectral branch's
    output, as models/fno_blocks.py does: dx sums the dact epilogues of the two branches"""
    inp = S.inputs_block(case)
    ref = S.run_oracle("block", inp, "gelu")
    fl = S.floor("block", inp, "gelu", ref)
    bad = []
    _judge("block " + case.name, "gelu", "block", _device("block", inp, "gelu", gpu_device), ref, fl, bad)
    assert not bad, bad
