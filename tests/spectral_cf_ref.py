"""Case tables, inputs, float64 references, error statistics and the float32 floor for the channels-first FNO operators
(SpectralConv1d / SpectralConv2d, the 1x1 convolution with its activation prologue, the FNOBlock pre-activation).
Test infrastructure only: plain torch-CPU, the product tree does not import it.

Reference: oracle.reference_path.spectral_conv1d / spectral_conv2d in float64 / complex128 under autograd (pinned to the
reference by the layer fixtures, overwrite quirk Q6 and the ignored imaginary parts Q7 included), composed with act(x);
tests/test_spectral_cf_ref_cpu.py checks it against dense DFT matrices.  Inputs are drawn in float32 and widened, so the
device and the reference see identical values and the ReLU kinks fall in the same places.

Which kernel a shape takes (csrc/cf_dft.hip, csrc/spectral_cf.hip, csrc/feedforward.hip; kp = m2 rounded up to 4):
  transform along the contiguous axis   h2 streaming kernel when n % 128 == 0, 2 kp <= 32, the table fits 64 KB, there
                                        are at least 16 lines and no activation is folded in; synthesis also n <= 512
  column stage of the 2-D layer         two launches when kp in {4, 8, 12, 16} and 2 M kp 4 bytes <= 64 KB, else three steps
  k_cmix                                16 / 4 / 2 samples per slab by how many workgroups that leaves, 8 or 4 waves
"""
from __future__ import annotations

from collections import namedtuple

import torch

from oracle import reference_path as R

SEED = 23
FWD_TOL, GRAD_TOL = 2e-6, 5e-6          # whole-tensor float64 bounds of test_rectangular_grid_clamps_modes_per_axis
# line_rel / mode_rel: device <= FLOOR_FACTOR * the float32 oracle's own error.  Started at 4; the largest ratios measured on
# an MI355X are 4.38 (line_rel) and 7.74 (mode_rel), twice either is past the cap of 8 (tests/test_gpu_spectral_cf.py)
FLOOR_FACTOR = 8.0
VANISH = 1e-6                           # a gradient mode that is exactly zero in float64: device norm <= VANISH * RMS mode norm

# cf / col: what the RPDE_FUSED_CF=0 / RPDE_COL_FUSED=0 leg must be against the default leg: "differ" (the fast path
# ran), "same" (it did not), None (not asserted)
Case = namedtuple("Case", "name dims act cf col")

# (B, Ci, Co, M, N, m1, m2)
CASES_2D = [
    # h2 analysis + synthesis, one table tile, 126 / 210 lines (partial last tiles), kp = 8, odd M (tail loop and scalar
    # table loads of k_col_mix_synthesis), Ci != Co
    Case("A", (2, 3, 5, 21, 128, 3, 5), "identity", "differ", "differ"),
    # h2 with two table tiles (R = 32), kp = 16, m1 = M/2, batch 19: 4-sample slabs with a partial last one (mode 1),
    # uneven four-way batch split (mode 2)
    Case("B", (19, 4, 4, 16, 128, 8, 16), "identity", "differ", "differ"),
    # GEMM path, Q6 overlap (2 m1 > M), Nyquist column, odd M, B = 1
    Case("C", (1, 4, 4, 15, 24, 8, 13), "identity", "same", None),
    # kp = 12, the headline FNO grid family
    Case("D", (2, 8, 8, 64, 256, 6, 12), "identity", "differ", "differ"),
    # ... with an activation prologue: forward analysis by the GEMM, backward h2 adjoint analysis + epi_dact GEMM
    Case("D-gelu", (2, 8, 8, 64, 256, 6, 12), "gelu", "differ", "differ"),
    Case("D-relu", (2, 8, 8, 64, 256, 6, 12), "relu", "differ", "differ"),
    # 16-sample slabs with a one-sample last slab, two staging chunks, Nyquist; RPDE_COL_FUSED=0: mode 0 at depth 16
    Case("E", (17, 32, 32, 12, 20, 4, 11), "identity", "same", "differ"),
    # column stage at exactly 64 KB of LDS
    Case("F1", (1, 3, 3, 1024, 16, 2, 7), "identity", None, "differ"),
    # just past it: the three-step fallback
    Case("F2", (1, 3, 3, 1024, 16, 2, 9), "identity", None, "same"),
    # analysis h2, synthesis GEMM (n > 512)
    Case("G", (1, 3, 2, 8, 1024, 2, 7), "identity", "differ", None),
    # the same split by table bytes
    Case("H", (2, 2, 2, 8, 640, 3, 6), "identity", "differ", None),
    # 8 lines: GEMM on an eligible grid; kp = 4
    Case("I", (1, 1, 1, 8, 128, 2, 4), "identity", "same", None),
    # kp = 20: no column stage; second ky0 pass; Ci Co = 15 leaves dead waves
    Case("J", (2, 5, 3, 40, 64, 14, 18), "identity", "same", "same"),
    # 12 analysis waves with a second row-group pass; R kp = 512: two passes of the 320-thread mix
    Case("K", (2, 4, 4, 32, 48, 16, 16), "identity", None, "differ"),
    # m1 = M: every weights1 slot is overwritten, dW1 must vanish
    Case("L", (3, 2, 2, 6, 10, 6, 4), "identity", "same", None),
    # C with an activation prologue
    Case("C-gelu", (1, 4, 4, 15, 24, 8, 13), "gelu", "same", None),
]

# (B, Ci, Co, n, K); the column stage does not exist in one dimension
CASES_1D = [
    # 16-way split GEMM (128 KB table: no h2)
    Case("n1024", (3, 8, 6, 1024, 16), "identity", "same", "same"),
    # h2, both tables at exactly 64 KB, 20 lines
    Case("n512", (5, 4, 4, 512, 16), "identity", "differ", "same"),
    # kp = 4
    Case("n128", (2, 9, 5, 128, 3), "identity", "differ", "same"),
    # Nyquist, K > 16, 2-sample slabs with four-wave groups
    Case("n48", (70, 4, 4, 48, 25), "identity", None, "same"),
    # 3 lines
    Case("n384-relu", (1, 3, 3, 384, 10), "relu", None, "same"),
    # overlap-free small case shared with the dense-matrix check
    Case("n16", (2, 4, 5, 16, 9), "identity", None, "same"),
]

# (B, Ci, Co, spatial)
CONV_SHAPES = [
    (1, 17, 7, (21, 19)),       # S = 399: scalar k_rowsum; two-way reduction split
    (3, 32, 32, (64, 64)),      # eight-way split
    (70, 3, 5, (16,)),          # 1-D, no split
]
ACTS = ("identity", "gelu", "relu")

BLOCK_CASES = [c for c in CASES_2D if c.name in ("A", "D")]       # run with gelu


def by_name(table, name):
    return next(c for c in table if c.name == name)


def _gen(case_dims, salt):
    return torch.Generator().manual_seed(SEED + salt + sum((i + 1) * int(v) for i, v in enumerate(case_dims)))


def _crand(shape, g, scale):
    return torch.complex(torch.rand(*shape, generator=g), torch.rand(*shape, generator=g)) * scale


# ---- inputs (float32 / complex64, CPU) ------------------------------------------------------------------------------
def inputs_2d(case):
    """-> dict x [B,Ci,M,N], g [B,Co,M,N] (cotangent), w1, w2 [Ci,Co,m1,m2] complex64"""
    B, Ci, Co, M, N, m1, m2 = case.dims
    g = _gen(case.dims, 2000)
    return {"x": torch.randn(B, Ci, M, N, generator=g), "g": torch.randn(B, Co, M, N, generator=g),
            "w1": _crand((Ci, Co, m1, m2), g, 1.0 / (Ci * Co)), "w2": _crand((Ci, Co, m1, m2), g, 1.0 / (Ci * Co))}


def inputs_1d(case):
    B, Ci, Co, n, K = case.dims
    g = _gen(case.dims, 1000)
    return {"x": torch.randn(B, Ci, n, generator=g), "g": torch.randn(B, Co, n, generator=g),
            "w": _crand((Ci, Co, K), g, 1.0 / (Ci * Co))}


def inputs_conv(shape, bias=True, acc=False):
    B, Ci, Co, sp = shape
    g = _gen((B, Ci, Co) + tuple(sp), 3000)
    inp = {"x": torch.randn(B, Ci, *sp, generator=g), "g": torch.randn(B, Co, *sp, generator=g),
           "w": torch.randn(Co, Ci, *([1] * len(sp)), generator=g) / Ci, "b": torch.randn(Co, generator=g),
           "acc": torch.randn(B, Co, *sp, generator=g)}
    if not bias:
        inp.pop("b")
    if not acc:
        inp.pop("acc")
    return inp


def inputs_block(case):
    """the 2-D inputs plus the bypass convolution wc [Co,Ci,1,1], bc [Co]"""
    B, Ci, Co = case.dims[:3]
    inp = inputs_2d(case)
    g = _gen(case.dims, 4000)
    inp["wc"] = torch.randn(Co, Ci, 1, 1, generator=g) / Ci
    inp["bc"] = torch.randn(Co, generator=g)
    return inp


# ---- the oracle, in the dtype of its inputs ---------------------------------------------------------------------------
def _widen(inp, real):
    cplx = torch.complex128 if real == torch.float64 else torch.complex64
    return {k: v.detach().to(cplx if v.is_complex() else real, copy=True).requires_grad_(k != "g") for k, v in inp.items()}


def _conv(w, ax, b):
    o = torch.einsum("oi,bis->bos", w.reshape(w.shape[0], w.shape[1]), ax.flatten(2)).reshape(ax.shape[0], w.shape[0], *ax.shape[2:])
    return o if b is None else o + b.view(1, -1, *([1] * (ax.dim() - 2)))


def run_oracle(kind, inp, act, real=torch.float64):
    """kind: "2d" | "1d" | "conv" | "block".  -> dict of detached results: out, dx and the parameter gradients"""
    t = _widen(inp, real)
    ax = R._act(act)(t["x"])
    if kind == "2d":
        out, params = R.spectral_conv2d(ax, t["w1"], t["w2"]), {"dW1": "w1", "dW2": "w2"}
    elif kind == "1d":
        out, params = R.spectral_conv1d(ax, t["w"]), {"dW": "w"}
    elif kind == "conv":
        out, params = _conv(t["w"], ax, t.get("b")), {"gw": "w"}
        if "b" in t:
            params["gb"] = "b"
        if "acc" in t:
            out, params["gacc"] = out + t["acc"], "acc"
    elif kind == "block":
        out = R.spectral_conv2d(ax, t["w1"], t["w2"]) + _conv(t["wc"], ax, t["bc"])
        params = {"dW1": "w1", "dW2": "w2", "gw": "wc", "gb": "bc"}
    else:
        raise KeyError(kind)
    out.backward(t["g"])
    res = {"out": out.detach(), "dx": t["x"].grad}
    res.update({k: t[v].grad for k, v in params.items()})
    return res


# ---- statistics ------------------------------------------------------------------------------------------------------
def _d(t):
    t = t.detach().cpu()
    return t.to(torch.complex128) if t.is_complex() else t.double()


def rel(a, b):
    """whole-tensor relative L2 error of a against b"""
    a, b = _d(a), _d(b)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def line_rel(a, b):
    """largest L2 error of one line along the last axis over the root-mean-square line norm of b.  (The h2 kernels share
    one power-of-two scale across the 16 lines of a tile, so precision relative to one small line is not promised.)"""
    a, b = _d(a), _d(b)
    a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    rms = b.norm(dim=1).square().mean().sqrt().clamp_min(1e-300)
    return float((a - b).norm(dim=1).max() / rms)


def mode_norms(w):
    """w [Ci,Co,*modes] -> [*modes]: L2 norm over (i, o) of each mode"""
    w = _d(w)
    return w.abs().square().sum(dim=(0, 1)).sqrt()


def mode_scale(*refs):
    """RMS mode norm over the modes of the reference gradients that are not exactly zero (0.0 if there is none)"""
    n = torch.cat([mode_norms(r).flatten() for r in refs])
    n = n[n > 0]
    return float(n.square().mean().sqrt()) if n.numel() else 0.0


def mode_rel(a, b, scale=None):
    """a, b [Ci,Co,(m1,)m2] weight gradients.  -> (largest error of one mode over (i, o) / RMS mode norm, set of the modes
    whose reference gradient is exactly zero as index tuples, largest norm of a on those modes / RMS mode norm).
    scale: the RMS mode norm to use (mode_scale of both weights of a 2-D layer); default: that of b alone."""
    scale = mode_scale(b) if scale is None else scale
    err, ref, got = mode_norms(_d(a) - _d(b)), mode_norms(b), mode_norms(a)
    zero = ref == 0
    zset = {tuple(int(v) for v in idx) for idx in zero.nonzero()}
    live = err[~zero]
    worst = float(live.max()) / scale if live.numel() else 0.0
    stray = float(got[zero].max()) / scale if zset else 0.0
    return worst, zset, stray


def stats(kind, got, ref):
    """-> {name: {"rel":, "line_rel" | "mode_rel":, ("stray":, "zero":)}} for every result of the oracle"""
    out = {}
    wscale = mode_scale(*[ref[k] for k in ("dW1", "dW2", "dW") if k in ref]) if kind != "conv" else None
    for k, r in ref.items():
        s = {}
        if float(_d(r).abs().max()) > 0:
            s["rel"] = rel(got[k], r)
        if k in ("out", "dx"):
            s["line_rel"] = line_rel(got[k], r)
        elif k in ("dW1", "dW2", "dW"):
            s["mode_rel"], s["zero"], s["stray"] = mode_rel(got[k], r, wscale)
        out[k] = s
    return out


def floor(kind, inp, act, ref=None):
    """the same oracle in float32 on the CPU against float64: the yardstick of the line_rel / mode_rel bounds"""
    ref = run_oracle(kind, inp, act) if ref is None else ref
    return stats(kind, run_oracle(kind, inp, act, torch.float32), ref)
