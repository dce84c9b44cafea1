"""Case tables, inputs, float64 oracle, error statistics, the float32 floor and the checker for the channels-last FFNO
spectral layers (rpde.ops.fspectral2d / fspectral1d; csrc/fspectral.hip, fused_spectral.hip, fused_mix.hip, mix1d.hip).
Test infrastructure only: plain torch-CPU, the product tree does not import it.

Oracle: oracle.reference_path.fspectral2d_fourier / fspectral1d_fourier in float64 under autograd; the loss is
<out, g> + <skip, g2> when a run asks for the skip output, so its dx is the layer's dx plus g2.
tests/test_fspectral_ref_cpu.py checks the oracle against dense DFT matrices.  Inputs are drawn in float32 from a seeded
CPU generator and widened, so the device and the oracle see identical values.

Which kernels a 2-D shape takes (keff = min(K, n/2+1) per axis, kp = keff rounded up to 4, R = 2 kp):
  fused (fused2d_ok)     C = 64, M and N multiples of 32 and <= 256, keff_y == keff_x, R <= 48
    analysis             one pass k_dft_analysis_rr_h2 on square grids (RPDE_ANA_SQ=0: never), else the two-read
                         k_dft_analysis_h2, samples in chunks of 64 MB / sample_bytes; MT = ceil(R / 16)
    mode mix             h2 kernels of fused_mix.hip in "full" mode (RPDE_FUSED_MIX=0: pack + GEMM + fused2d_split, which
                         low-pass always takes on the raw spectra); weight gradient in mixw_slabs = clamp(rows/32/4, 1, 12) slabs
    synthesis            on 64-multiples with NF3 = 2 (R/32) + (3 (R%32)/8 + 3)/4 <= 3 the persistent kernels: synthesis4
                         (no skip gradient) or synthesis3 (with it), min(B, 8) groups; else the 16 x 16 tile synthesis2
                         (RPDE_SYN3=0: always)
  per axis               analysis GEMM | mix | synthesis GEMM; the mix is mix1d.hip when rows <= 64 and C in {32, 64, 128},
                         else pack + GEMM + split-K weight gradient; kp != keff takes a memset of the mixed spectrum
The h2 tables of a plan are built with the plan whatever the switches say (core.hip build_plan), so a plan first used
under a switch is complete; the default leg still runs first (tests/test_gpu_fspectral.py).
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import torch

from oracle import reference_path as R
from tests.spectral_cf_ref import FWD_TOL, GRAD_TOL, _d, rel  # noqa: F401  (re-exported)

SEED = 41
# point_rel / mode_rel: device <= FLOOR_FACTOR * the float32 oracle's own error on the same case.  Started at 4; the largest
# ratios measured on an MI355X are 1.62 (point_rel) and 1.93 (mode_rel), twice either fits under 4 (tests/test_gpu_fspectral.py)
FLOOR_FACTOR = 4.0
# per-case bounds in place of FLOOR_FACTOR, {(case name, result, statistic): factor}, each with its derivation
BOUNDS: dict = {}

# kind "2d": dims (B, M, N, C, K); skip: run the backward both without and with the skip gradient
# kind "1d": dims (B, n, C, K); always with the skip gradient
Case = namedtuple("Case", "name kind dims family mode skip norm", defaults=("gauss", "full", False, "ortho"))


def _c2(name, dims, family="gauss", mode="full", skip=False):
    return Case(name, "2d", dims, family, mode, skip, "ortho")


def _c1(name, dims, norm, mode):
    return Case(name, "1d", dims, "gauss", mode, True, norm)


CASES_2D = [
    # fused, Nyquist bin on both axes (keff = 17 = n/2+1: the ignored imaginary parts of DC and Nyquist in the forward, the
    # adjoint and dW[..., 0], dW[..., 16]); R = 40 (K32 = 1, TG = 1); one-pass analysis MT = 3; 16 x 16 synthesis; S = 1
    _c2("F-nyq", (2, 32, 32, 64, 17)),
    # R = 8, MT = 1; k_dft_synthesis4_h2 forward and no-skip adjoint, synthesis3 with the skip gradient; B < 8 groups
    _c2("F-r8", (3, 64, 64, 64, 4), skip=True),
    # B = 9: uneven groups of the persistent synthesis kernels; mixw_slabs S = 4; backward with one side wanted
    # (test_gradient_subsets: hmix without hwg and hwg without hmix in fused2d_bwd)
    _c2("F-r40", (9, 64, 64, 64, 20), skip=True),
    # NF3 = 4: synthesis2 on a grid of 64-multiples (RPDE_SYN3=0 changes nothing); K32 = 1, TG = 2
    _c2("F-r48", (2, 64, 64, 64, 24)),
    # two-read analysis (not square), R = 24, MT = 2; B = 1
    _c2("F-rect24", (1, 96, 32, 64, 12)),
    # rectangular 64-multiples on the persistent synthesis kernels, R = 16
    _c2("F-rect16", (3, 128, 64, 64, 8), skip=True),
    # K32 = 1, TG = 0; no Nyquist (16 < 17)
    _c2("F-r32", (2, 32, 64, 64, 16)),
    # mixw_slabs clamped at S = 12 (rows/32 = 50 >= 48) with uneven slabs; TG = 3 on synthesis4
    _c2("F-many", (25, 64, 64, 64, 12), skip=True),
    # more groups than a sample has tiles; slabs 20 / 4 = 5
    _c2("F-small", (20, 32, 32, 64, 8)),
    # largest grid (n = 32 ANA_MAXKS); under RPDE_ANA_SQ=0 the chunk of k_dft_analysis_h2 is 64 MB / 16 MB = 4 samples and
    # the fifth sits alone in the last, partial chunk ("skips the holes")
    _c2("F-chunk", (5, 256, 256, 64, 20)),
    # every later 32-point chunk of every line, along both axes, exceeds the running power-of-two scale of the line: the
    # accumulators of both analysis kernels (one-pass, and two-read under RPDE_ANA_SQ=0) are rescaled at every chunk
    _c2("F-ramp", (2, 128, 128, 64, 12), family="ramp", skip=True),
    # PDE-like field (power-law spectrum), trained-like weights (decay over the modes, outliers)
    _c2("F-smooth", (2, 64, 64, 64, 16), family="smooth"),
    # low-pass on the fused grid: analysis without line maxima, fused2d_split of the raw spectra, no h2 mix
    _c2("F-lowpass", (2, 64, 64, 64, 12), mode="low-pass", skip=True),
    # keff_y = 17 against keff_x = 20: per-axis path; dWy[..., 17:] == 0 while dWx[..., 17:] is live
    _c2("G-clamp", (2, 64, 32, 64, 20)),
    # M, N no multiples of 32; kp = 12 != keff = 9 (memset branch of axis_fwd / axis_bwd); gradient subsets (if (gw), if (gx))
    _c2("G-odd", (2, 48, 40, 64, 9), skip=True),
    # 64 rows per axis at C = 32: the 2-D layer on mix1d.hip
    _c2("G-mix1d", (2, 32, 32, 32, 8)),
    # 96 rows: pack + GEMM with the split weight gradient
    _c2("G-gemm32", (3, 32, 32, 32, 8)),
    # C = 48 (no mix1d at 20 / 24 rows); Nyquist along N (keff_y = 11 = N/2+1)
    _c2("G-c48", (1, 24, 20, 48, 11)),
    # M > 256 = 32 ANA_MAXKS falls off the fused path at C = 64
    _c2("G-tall", (1, 288, 64, 64, 12)),
    # per-axis low-pass
    _c2("G-lowpass", (2, 40, 24, 32, 5), mode="low-pass", skip=True),
]

CASES_1D = [
    # mix1d; kp = 12 != keff = 9; norm "backward"; gradient subsets
    _c1("H-bwd", (3, 64, 64, 9), "backward", "full"),
    # keff = 25 includes Nyquist; K > keff: dW[..., 25:] == 0; norm "forward"
    _c1("H-fwd", (2, 48, 32, 30), "forward", "full"),
    # more than 64 rows: pack + GEMM
    _c1("H-rows", (70, 96, 64, 12), "ortho", "full"),
    # width outside {32, 64, 128}
    _c1("H-c48", (5, 40, 48, 7), "ortho", "full"),
    # low-pass
    _c1("H-lowpass", (4, 128, 128, 16), "ortho", "low-pass"),
]


def by_name(name):
    return next(c for c in CASES_2D + CASES_1D if c.name == name)


def keffs(case):
    """retained modes per weight gradient: each axis is clamped by its own length"""
    if case.kind == "2d":
        B, M, N, C, K = case.dims
        return {"dWy": min(K, N // 2 + 1), "dWx": min(K, M // 2 + 1)}
    B, n, C, K = case.dims
    return {"dW": min(K, n // 2 + 1)}


def fused_ok(case):
    """fused2d_ok of csrc/fused_spectral.hip"""
    if case.kind != "2d":
        return False
    B, M, N, C, K = case.dims
    k = keffs(case)
    R = 2 * 4 * ((k["dWy"] + 3) // 4)
    return C == 64 and M % 32 == 0 and N % 32 == 0 and M <= 256 and N <= 256 and k["dWy"] == k["dWx"] and R <= 48


def skips(case):
    """the with_skip values a case runs with"""
    return (True,) if case.kind == "1d" else ((False, True) if case.skip else (False,))


def legs(case):
    """[(switch, want)]: what the leg with that switch set to 0 must be against the default leg: "differ" (the case is there
    for the fast path), "same" (the switch must not matter), None (not asserted).  G and H cases run the default leg only."""
    if not fused_ok(case):
        return []
    B, M, N, C, K = case.dims
    full = case.mode == "full"
    out = [("RPDE_FUSED_SPECTRAL", "differ"), ("RPDE_FUSED_MIX", "differ" if full else "same")]
    if M == N:
        # the one-pass kernel starts a line at the chunk of its own band and wraps round: another order of summation on
        # every grid of more than one chunk (on 32 points both kernels add the same one chunk)
        out.append(("RPDE_ANA_SQ", "differ" if M > 32 else None))
    if M % 64 == 0 and N % 64 == 0:
        # "same" with and without the persistent kernels (which run where NF3 = 2 (R/32) + (3 (R%32)/8 + 3)/4 <= 3): all
        # three synthesis kernels feed the same operand blocks and table fragments to the same MFMA chain per output point
        # and add the two axes in the same order, only the tiling differs -- the switch changes no bit
        out.append(("RPDE_SYN3", "same"))
    return out


# ---- inputs (float32, CPU) ----------------------------------------------------------------------------------------------
def _gen(case, salt):
    return torch.Generator().manual_seed(SEED + salt + sum((i + 1) * int(v) for i, v in enumerate(case.dims)))


def _smooth_field(shape, g):
    """[B, M, N, C] with the power-law spectrum |k|^-2.5 per channel, unit RMS per sample"""
    B, M, N, C = shape
    f = torch.fft.rfft2(torch.randn(B, C, M, N, generator=g))
    ky = torch.fft.fftfreq(M, 1.0 / M).view(M, 1)
    kx = torch.fft.rfftfreq(N, 1.0 / N).view(1, -1)
    amp = (ky.square() + kx.square()).sqrt().clamp_min(1.0).pow(-2.5)
    x = torch.fft.irfft2(f * amp, s=(M, N))
    x = x / x.square().mean(dim=(1, 2, 3), keepdim=True).sqrt()
    return x.permute(0, 2, 3, 1).contiguous()


def _weight(C, K, family, g):
    w = torch.randn(C, C, K, 2, generator=g) * 0.1
    if family == "smooth":
        w = w / (1.0 + torch.arange(K, dtype=torch.float32)).view(1, 1, K, 1)
        w = torch.where(torch.rand(C, C, K, 2, generator=g) < 0.01, w * 32.0, w)
    return w


@functools.lru_cache(maxsize=3)
def inputs(case):
    """-> dict of float32 CPU tensors: x, g (cotangent of out), g2 (cotangent of the skip output), and the weights wy, wx
    (2-D) or w (1-D) unless the case is low-pass.  Shared by every leg: do not write to them."""
    g = _gen(case, 1000 if case.kind == "1d" else 2000)
    B, C, K = case.dims[0], case.dims[-2], case.dims[-1]
    shape = tuple(case.dims[:-1])
    sample = [B] + [1] * (len(shape) - 1)
    if case.family == "gauss":
        s = torch.logspace(-3, 3, B).view(sample)
        x, gr = torch.randn(shape, generator=g) * s, torch.randn(shape, generator=g) / s
        g2 = torch.randn(shape, generator=g) / s
    elif case.family == "ramp":
        M, N = shape[1], shape[2]
        e = 3.0 * (torch.arange(M) // 32).view(1, M, 1, 1) + 3.0 * (torch.arange(N) // 32).view(1, 1, N, 1)
        ramp = torch.pow(2.0, e)
        x, gr = torch.randn(shape, generator=g) * ramp, torch.randn(shape, generator=g) * ramp
        g2 = torch.randn(shape, generator=g) * ramp
    elif case.family == "smooth":
        x, gr, g2 = _smooth_field(shape, g), torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    else:
        raise KeyError(case.family)
    inp = {"x": x.contiguous(), "g": gr.contiguous(), "g2": g2.contiguous()}
    if case.mode == "full":
        for k in (("wy", "wx") if case.kind == "2d" else ("w",)):
            inp[k] = _weight(C, K, case.family, g)
    return inp


# ---- the oracle, in the dtype asked for ----------------------------------------------------------------------------------
def layer(case, t):
    K = case.dims[-1]
    if case.kind == "2d":
        return R.fspectral2d_fourier(t["x"], t.get("wy"), t.get("wx"), K, case.mode)
    return R.fspectral1d_fourier(t["x"], t.get("w"), K, case.mode, case.norm)


GRADS = {"wy": "dWy", "wx": "dWx", "w": "dW"}


def run_oracle(case, real=torch.float64, fn=layer, inp=None):
    """-> dict of detached results without the skip gradient: out, dx and the weight gradients"""
    inp = inputs(case) if inp is None else inp
    t = {k: v.detach().to(real, copy=True).requires_grad_(k not in ("g", "g2")) for k, v in inp.items()}
    out = fn(case, t)
    out.backward(t["g"])
    res = {"out": out.detach(), "dx": t["x"].grad}
    res.update({GRADS[k]: t[k].grad for k in GRADS if k in t})
    return res


def add_skip(res, case, with_skip):
    """the results of the loss <out, g> + <skip, g2>"""
    if not with_skip:
        return res
    res = dict(res)
    res["dx"] = res["dx"] + inputs(case)["g2"].to(res["dx"].dtype)
    return res


@functools.lru_cache(maxsize=3)
def _oracle64(case):
    return run_oracle(case)


def oracle(case, with_skip=False):
    return add_skip(_oracle64(case), case, with_skip)


# ---- statistics ----------------------------------------------------------------------------------------------------------
def point_rel(a, b):
    """a, b [B, ..., C]: per sample, the largest L2 error over the C channels of one grid point over that sample's RMS point
    norm; the largest over the samples.  (The kernels promise one scale per line, so normalising per sample is honest;
    precision relative to one small point is not promised.)"""
    a, b = _d(a), _d(b)
    B, C = b.shape[0], b.shape[-1]
    err = (a - b).reshape(B, -1, C).norm(dim=2)
    rms = b.reshape(B, -1, C).norm(dim=2).square().mean(dim=1).sqrt().clamp_min(1e-300)
    return float((err.max(dim=1).values / rms).max())


def mode_norms(w):
    """w [C, C, K, 2] -> [K]: L2 norm of each mode over (i, o, re/im)"""
    return _d(w).square().sum(dim=(0, 1, 3)).sqrt()


def mode_scale(*refs):
    """RMS mode norm over the modes of the reference gradients that are not exactly zero"""
    if not refs:                                    # (low-pass: no weights)
        return 0.0
    n = torch.cat([mode_norms(r) for r in refs])
    n = n[n > 0]
    return float(n.square().mean().sqrt()) if n.numel() else 0.0


def mode_rel(a, b, scale):
    """largest error of one mode over the RMS mode norm `scale`"""
    return float(mode_norms(_d(a) - _d(b)).max()) / scale


def stats(case, got, ref):
    """-> {result: {"finite", "rel", "point_rel" | ("mode_rel", "stray")}} for every result in `got`.  stray: the largest
    magnitude the device left in a mode >= keff of that axis, where it writes zeros and the float64 gradient is exactly zero."""
    ke = keffs(case)
    wscale = mode_scale(*[ref[k] for k in ke if k in ref])
    out = {}
    for k, a in got.items():
        r = ref[k]
        s = {"finite": tuple(a.shape) == tuple(r.shape) and bool(torch.isfinite(a).all())}
        if s["finite"]:
            s["rel"] = rel(a, r)
            if k in ("out", "dx"):
                s["point_rel"] = point_rel(a, r)
            else:
                s["mode_rel"] = mode_rel(a, r, wscale)
                s["stray"] = float(a[:, :, ke[k]:].abs().max()) if a.shape[2] > ke[k] else 0.0
        out[k] = s
    return out


@functools.lru_cache(maxsize=3)
def oracle32(case):
    return run_oracle(case, torch.float32)


@functools.lru_cache(maxsize=None)
def floor(case, with_skip=False):
    """the same oracle in float32 on the CPU against float64: the yardstick of the point_rel / mode_rel bounds"""
    return stats(case, add_skip(oracle32(case), case, with_skip), oracle(case, with_skip))


def factor(case, k, stat):
    return BOUNDS.get((case.name, k, stat), FLOOR_FACTOR)


def check(st, fl, case):
    """the assertions of the GPU test on the statistics `st` of one run against the floor `fl` of the same case:
    -> list of failures, empty when the run passes"""
    bad = []
    for k, s in st.items():
        if not s["finite"]:
            bad.append((k, "wrong shape or not finite"))
            continue
        tol = FWD_TOL if k == "out" else GRAD_TOL
        if not s["rel"] <= tol:
            bad.append((k, "rel", s["rel"], tol))
        for stat in ("point_rel", "mode_rel"):
            if stat in s and not s[stat] <= factor(case, k, stat) * fl[k][stat]:
                bad.append((k, stat, s[stat], "floor", fl[k][stat], "ratio", s[stat] / max(fl[k][stat], 1e-300)))
        if s.get("stray", 0.0) != 0.0:
            bad.append((k, "modes >= keff are not exactly zero", s["stray"]))
    return bad


def ratios(st, fl):
    """{"out.point_rel": device / floor, ...}"""
    return {f"{k}.{stat}": s[stat] / fl[k][stat] if fl[k][stat] > 0 else math.inf
            for k, s in st.items() for stat in ("point_rel", "mode_rel") if stat in s}
