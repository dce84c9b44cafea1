"""A ctypes harness for the lifting / projection kernels at the model boundary, for tests that own every buffer:
tests/test_gpu_thin_linear.py and tests/test_gpu_conv_small.py on the GPU, tests/test_thin_ref_cpu.py for what those
tests rest on.  Nothing in this file needs a GPU to import.

Channels-last: csrc/thin_linear.hip (k_thin_expand, k_thin_contract, k_thin_outer, k_thin_fold) behind rpde_linear_fwd /
rpde_linear_bwd.  Channels-first: the plain instance k_conv1x1_small<CO, false> of csrc/conv_small.hip behind
rpde_conv1x1_fwd / rpde_conv1x1_act_fwd.  Buffers are ff_abi's: guarded by NaN words, outputs and workspace poisoned.

Plans.  thin_plan / conv_plan restate the launch constants of the two files; they show that a case meets the edge it is
listed for and never compute an expected value.

Problems.  Two kinds per case, float32 on the CPU, seeded from a CRC of the case.
  exact: every operand an integer of -3 .. 3, bias included.  Every product is an integer and, whatever the order of
         summation, every partial sum of an output element is bounded by the sum of its terms' magnitudes; the problem
         builder asserts that this sum stays below 2^24 for every element (9 P would not at P = 2 100 001, the actual
         sums -- about 2.9 P for a weight gradient -- do), so every partial sum is an exactly representable integer and
         a correct fp32 kernel equals the float64 result bit for bit.  One dropped, doubled or misplaced point changes an
         integer.
  randn: x and grad_out randn, w from torch.nn.Linear's initialisation times (1 + 0.3 randn).

Bounds on the randn kind, per element, derived and not measured: with u = 2^-24 and S_abs the sum of the magnitudes of
the element's terms (bias and accumulated input included), |got - ref| <= (n + c) u S_abs for n products: c = 2 for the
thin kernels (bias add and one more rounding), c = 3 for k_conv1x1_small (bias, accumulate, one more); a leg that runs
the GEMM path adds ff_abi.ROW_MARGIN to the count.  act_in = gelu adds GELU_TOL sum_i |W[o][i]|; act_out = gelu
multiplies by 1.13 >= max |gelu'| and adds GELU_TOL; relu is 1-Lipschitz and exact and changes nothing.  The weight and
bias gradients of the randn kind keep the whole-tensor 1e-5 of test_thin_linear_kernels: the exact kind pins their
structure."""
from __future__ import annotations

import functools
import zlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as Fn

from tests import ff_abi as F
from tests.ff_abi import Buffers, Env, Guarded, ROW_MARGIN, rel

UNIT = 2.0 ** -24
GELU_TOL = 1.5 * 4.2e-7                      # tests/test_gpu_pointwise.py (tests/test_thin_ref_cpu.py compares the two)
DGELU_MAX = 1.13                             # max |gelu'| = 1.1290 at x = 1.4142
WGRAD_TENSOR_TOL = 1e-5                      # tests/test_gpu_fused_paths.py::test_thin_linear_kernels, dw and db
EXACT_LIMIT = float(1 << 24)
KINDS = ("exact", "randn")


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------
# csrc/thin_linear.hip restated
# ---------------------------------------------------------------------------------------------------------------------
TL_THREADS = 256                             # thin_linear.hip:20
TL_GRID_CAP = 2048                           # :177-182 tl_grid
TL_OUTER_PTS, TL_OUTER_CAP = 128, 1024       # :226-231 tl_outer_blocks
TL_UNROLL = 8                                # :108 UN


def thin_ok(T: int, O: int) -> bool:
    """thin_linear.hip:171-174 thin_linear_ok, the switch aside"""
    return 1 <= T <= 4 and 4 <= O <= 256 and O % 4 == 0 and TL_THREADS % (O // 4) == 0


def is_thin(in_f: int, out_f: int) -> bool:
    """feedforward.hip:48-49, 73-74, 114-115: the thin kernels serve the layer when either side is the thin one"""
    return (in_f <= 4 and thin_ok(in_f, out_f)) or (out_f <= 4 and thin_ok(out_f, in_f))


def thin_plan(P: int, T: int, O: int) -> Dict[str, object]:
    """the launch of the three kernels for P points, T thin and O wide features"""
    plan: Dict[str, object] = {"thin_ok": thin_ok(T, O), "NQ": cdiv(O, 64)}       # :203 nq
    if not plan["thin_ok"]:
        return plan
    pps = TL_THREADS // (O // 4)                                                 # :27, :101, :187
    nb = max(1, min(cdiv(P, TL_OUTER_PTS), TL_OUTER_CAP))                        # :226-231
    ppb = cdiv(P, nb)                                                            # :276
    sizes = [max(0, min(P, (k + 1) * ppb) - k * ppb) for k in range(nb)]         # :102 p0, p1
    # k_thin_outer, point lane pl of a workgroup of n points: ceil((n - pl) / pps) points; :110 takes eight at a time
    # while eight remain, :130 the rest.  "ragged": the last remainder trip has live and idle point lanes.
    trips = []
    for n in sorted(set(sizes), reverse=True):
        own = cdiv(n, pps)                                                       # point lane 0
        trips.append(dict(points=n, full=own // TL_UNROLL, rem=own % TL_UNROLL, ragged=n % pps != 0,
                          count=sizes.count(n)))
    plan.update(pps=pps, grid_expand=max(1, min(cdiv(P, pps), TL_GRID_CAP)), sweeps_expand=cdiv(P, pps),
                grid_contract=max(1, min(cdiv(P, 16), TL_GRID_CAP)), sweeps_contract=cdiv(P, 16),     # :188, :202
                nb=nb, ppb=ppb, full=trips[0]["full"], rem=trips[0]["rem"], ragged=trips[0]["ragged"], trips=trips,
                empty=sizes.count(0), ws_floats=nb * ((T + 1) * O + 4))                                # :232
    return plan


# ---------------------------------------------------------------------------------------------------------------------
# csrc/conv_small.hip restated
# ---------------------------------------------------------------------------------------------------------------------
CONV_MIN_POINTS = 1 << 20                    # feedforward.hip:441


def conv_plan(B: int, Cin: int, Cout: int, S: int, aligned: bool = True) -> Dict[str, object]:
    """conv_small.hip:107-117 and feedforward.hip:441: whether k_conv1x1_small<CO, false> runs, and its launch"""
    CO = 4 if Cout <= 4 else 8 if Cout <= 8 else 16 if Cout <= 16 else 32        # :115
    taken = (1 <= Cout <= 32 and 1 <= Cin <= 512 and S % 4 == 0 and aligned and B <= 65535
             and B * S >= CONV_MIN_POINTS)
    quads = cdiv(S, 4)
    return dict(CO=CO, padded=CO - Cout if Cout <= 32 else 0, lds_bytes=4 * Cin * CO, blocks=cdiv(quads, 256),   # :116-117
                last_live=(quads - 1) % 256 + 1, tail_points=S % 1024, taken=taken)


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
THIN_T, THIN_O = (1, 2, 3, 4), (4, 8, 16, 32, 64, 128, 256)
THIN_SHAPES = [(T, O) for T in THIN_T for O in THIN_O]
REFUSED_SHAPES = [(3, 12), (3, 192), (5, 64), (3, 260)]          # what thin_linear_ok refuses: the GEMM path
ROLES = ("lifting", "projection")
MISALIGN = ("y", "x", "grad_out", "dx")
MISALIGN_POINTS = (129, 8193)


def small_points(T: int, O: int) -> List[int]:
    """1, 15, 16, 17 (contract's sweep of 16), pps - 1 and pps + 1 (expand's and outer's sweep), 129 (two workgroups of
    the outer kernel); the refused neighbours have no sweep and take 64 for it"""
    pps = TL_THREADS // (O // 4) if thin_ok(T, O) else 64
    return sorted({1, 15, 16, 17, pps - 1, pps + 1, 129} - {0})


# P -> (the shapes it runs for, the edge as thin_plan states it)
LARGE_POINTS = {
    8193: ([(T, 256) for T in THIN_T], dict(pps=4, sweeps_expand=2049, grid_expand=2048)),
    32769: ([(1, 64), (3, 64)], dict(pps=16, sweeps_expand=2049, grid_expand=2048, sweeps_contract=2049,
                                     grid_contract=2048)),
    131073: ([(T, O) for O in (64, 256) for T in THIN_T], dict(nb=1024, ppb=129, empty=7)),
    140001: ([(3, 64), (4, 256)], dict(nb=1024, ppb=137, empty=2)),
    524589: ([(2, 4)], dict(pps=256, sweeps_expand=2050, grid_expand=2048, full=0)),
    2100001: ([(4, 4)], dict(pps=256, ppb=2051, full=1, rem=1, ragged=True)),
}
# (P, T, O) -> more of the plan, where the table of the cases says more about one shape
LARGE_EXTRA = {(140001, 3, 64): dict(full=1, rem=1, ragged=True), (140001, 4, 256): dict(full=4, rem=3, ragged=True)}


def shape_of(role: str, T: int, O: int) -> Tuple[int, int]:
    """-> (in_f, out_f).  lifting: forward = expand, data gradient = contract, weight gradient = outer with G transposed
    and cs the bias gradient; projection: forward = contract, data gradient = expand through the strided weight view,
    weight gradient = outer with ts the bias gradient"""
    assert role in ROLES
    return (T, O) if role == "lifting" else (O, T)


# (B, Cin, Cout, S) -> what conv_plan must say
CONV_CASES = [
    ((1, 3, 1, (1 << 20) + 4), dict(CO=4, padded=3, last_live=1, taken=True)),
    ((1, 1, 4, (1 << 20) + 1020), dict(CO=4, padded=0, last_live=255, taken=True)),
    ((3, 5, 5, 349528), dict(CO=8, padded=3, tail_points=344, last_live=86, taken=True)),
    ((2, 20, 8, 524292), dict(CO=8, padded=0, last_live=1, taken=True)),
    ((1, 32, 9, (1 << 20) + 512), dict(CO=16, padded=7, last_live=128, taken=True)),
    ((1, 7, 16, 1 << 20), dict(CO=16, padded=0, tail_points=0, last_live=256, taken=True)),
    ((1, 16, 17, (1 << 20) + 4), dict(CO=32, padded=15, last_live=1, taken=True)),
    ((1, 512, 17, 1 << 20), dict(CO=32, padded=15, lds_bytes=64 * 1024, taken=True)),
    ((65535, 3, 5, 20), dict(CO=8, padded=3, blocks=1, last_live=5, taken=True)),
]
# (case, misaligned operand) -> the GEMM path must be right
CONV_FALLBACKS = [
    ((1, 3, 5, (1 << 20) + 2), None),          # S % 4 != 0
    ((1, 3, 33, 1 << 20), None),               # Cout > 32
    ((1, 3, 5, (1 << 20) + 4), "x"),
    ((1, 3, 5, (1 << 20) + 4), "out"),
]
CONV_LEGS = [("identity", "identity", 0)]
CONV_MORE_LEGS = [("gelu", "identity", 1), ("identity", "relu", 1)]     # padded channels and the 65535 case, + bias NULL
DEVICE_RESIDENT = 1 << 28                    # elements of x from which a problem lives on the device (Cin 512: 2 GiB)
CROSS_POINTS = 4096


def conv_more_legs(case) -> bool:
    B, Cin, Cout, S = case
    return conv_plan(*case)["padded"] > 0 or B == 65535


# ---------------------------------------------------------------------------------------------------------------------
# the linear problem
# ---------------------------------------------------------------------------------------------------------------------
def _ints(*shape, device="cpu", generator=None):
    return torch.randint(-3, 4, shape, device=device, generator=generator).float()


@functools.lru_cache(maxsize=2)
def linear_problem(kind: str, P: int, in_f: int, out_f: int):
    """x [P, in], grad_out [P, out], w [out, in], b [out] on the CPU in float32; float64 results `ref` (y with and
    without bias, dx, dW, db) and per-element term magnitudes `mag`"""
    assert kind in KINDS
    crc = zlib.crc32(repr(("thin", kind, P, in_f, out_f)).encode())
    with torch.random.fork_rng():
        torch.manual_seed(crc)
        if kind == "exact":
            x, g, w, b = _ints(P, in_f), _ints(P, out_f), _ints(out_f, in_f), _ints(out_f)
        else:
            x, g = torch.randn(P, in_f), torch.randn(P, out_f)
            lin = torch.nn.Linear(in_f, out_f)
            w = (lin.weight.detach() * (1 + 0.3 * torch.randn(out_f, in_f))).contiguous()
            b = lin.bias.detach().clone()
    xd, gd, wd, bd = x.double(), g.double(), w.double(), b.double()
    ref = {"y0": xd @ wd.t(), "dx": gd @ wd, "dW": gd.t() @ xd, "db": gd.sum(0)}
    ref["y"] = ref["y0"] + bd
    mag = {"y0": xd.abs() @ wd.abs().t(), "dx": gd.abs() @ wd.abs(), "dW": gd.abs().t() @ xd.abs(), "db": gd.abs().sum(0)}
    mag["y"] = mag["y0"] + bd.abs()
    if kind == "exact":
        worst = max(float(m.max()) for m in mag.values())
        assert worst < EXACT_LIMIT, (P, in_f, out_f, worst)
    return dict(kind=kind, P=P, in_f=in_f, out_f=out_f, x=x, g=g, w=w, b=b, ref=ref, mag=mag, on={})


FMA_CHAIN_MAX = 8


def chain32(terms: torch.Tensor) -> torch.Tensor:
    """the float32 sum of the last axis of `terms` (float64 holding exact values: float32 numbers and products of two),
    by fused multiply-adds in ascending order of magnitude.  The first term is rounded to float32, every later one
    enters as fmaf(a, b, s): the product is exact in float64, the sum is rounded there and then to float32.  For n terms
    of magnitudes t_1 <= .. <= t_n the error is at most u sum_k |s_k| <= u sum_j t_j (n - j + 1) <= u (n + 1) / 2 S_abs,
    the maximum at equal magnitudes: exactly half of the (products + 2) u S_abs and (Cin + 3) u S_abs of the kernels,
    whose terms are the products and the bias (and the accumulated input).  In the kernels' own order -- bias first --
    a bias that dominates is rounded once per product, up to (n - 1) u S_abs: that order was measured at 0.51 .. 0.56 of
    the bound for T = 3 and 4 at 8193 points and more, so the device may sit anywhere up to the bound itself"""
    order = torch.argsort(terms.abs(), dim=-1)
    t = torch.gather(terms, -1, order)
    s = t[..., 0].float()
    for k in range(1, t.shape[-1]):
        s = (s.double() + t[..., k]).float()
    return s


def _chain_rows(a: torch.Tensor, w: torch.Tensor, start: Optional[torch.Tensor]) -> torch.Tensor:
    """start[o] + sum_k a[p][k] w[o][k] by chain32, 4096 rows at a time"""
    out = torch.empty(a.shape[0], w.shape[0])
    wd = w.double()
    for p0 in range(0, a.shape[0], 4096):
        terms = a[p0:p0 + 4096, None, :].double() * wd[None]
        if start is not None:
            terms = torch.cat([terms, start.double()[None, :, None].expand(terms.shape[0], -1, 1)], dim=-1)
        out[p0:p0 + 4096] = chain32(terms)
    return out


def linear_f32(prob) -> Dict[str, torch.Tensor]:
    """the float32 CPU restatement: chain32 over at most FMA_CHAIN_MAX products, float32 matmuls beyond"""
    x, g, w, b = prob["x"], prob["g"], prob["w"], prob["b"]
    res = {"dW": g.t() @ x, "db": g.sum(0)}
    if prob["in_f"] <= FMA_CHAIN_MAX:
        res["y"], res["y0"] = _chain_rows(x, w, b), _chain_rows(x, w, None)
    else:
        res["y"], res["y0"] = x @ w.t() + b, x @ w.t()
    res["dx"] = _chain_rows(g, w.t(), None) if prob["out_f"] <= FMA_CHAIN_MAX else g @ w
    return res


def conv_f32(prob, act_in: str, act_out: str, accumulate: int, bias: bool) -> torch.Tensor:
    """the float32 CPU restatement of the convolution: chain32 over the products, the bias and the accumulated input for
    at most FMA_CHAIN_MAX input channels, a float32 einsum beyond"""
    # (the activation correctly rounded: a float32 erf good to one ulp is off by 4.8e-7 at |x| >= 4, most of GELU_TOL,
    #  which is a tolerance for the device's formula on |x| <= 9 and not for a library's last place)
    x = _ACT[act_in](prob["x"].double()).float()
    B, Cin, S = x.shape
    w = prob["w"]
    if Cin <= FMA_CHAIN_MAX:
        terms = [w.double().t()[None, :, :, None] * x.double()[:, :, None, :]]          # [B, Cin, Cout, S]
        if bias:
            terms.append(prob["b"].double()[None, None, :, None].expand(B, 1, -1, S))
        if accumulate:
            terms.append(prob["out0"].double()[:, None])
        out = chain32(torch.cat(terms, dim=1).movedim(1, -1))
    else:
        out = torch.einsum("oi,bis->bos", w, x)
        if bias:
            out = out + prob["b"][None, :, None]
        if accumulate:
            out = out + prob["out0"]
    return _ACT[act_out](out)


def _on(prob, dev):
    """float64 references and magnitudes on `dev`, moved once"""
    key = str(dev)
    if key not in prob["on"]:
        prob["on"][key] = ({k: v.to(dev) for k, v in prob["ref"].items()}, {k: v.to(dev) for k, v in prob["mag"].items()})
    return prob["on"][key]


def linear_counts(prob, gemm: bool) -> Dict[str, float]:
    """products + 2 of y (in_f) and dx (out_f): (T + 2) for expand, (O + 2) for contract, whichever the role makes them"""
    m = ROW_MARGIN if gemm else 0.0
    return {"y": prob["in_f"] + 2 + m, "dx": prob["out_f"] + 2 + m}


def linear_misses(got: Dict[str, torch.Tensor], prob, *, bias: bool = True, gemm: bool = False):
    """-> (figures, misses).  figures: per quantity the worst fraction of its bound (exact kind: the number of elements
    that differ) and where; misses: the quantities over their bound"""
    figs: Dict[str, Tuple[float, int]] = {}
    miss: List[str] = []
    count = linear_counts(prob, gemm)
    for k, t in got.items():
        dev = t.device
        ref, mag = _on(prob, dev)
        rk = "y0" if (k == "y" and not bias) else k
        r = ref[rk]
        assert t.shape == r.shape, (k, t.shape, r.shape)
        td = t.double()
        if prob["kind"] == "exact":
            ne = td != r
            n = int(ne.sum())
            figs[k] = (float(n), int(torch.nonzero(ne.flatten())[0]) if n else -1)
            bad = n > 0
        elif k in ("y", "dx"):
            frac = ((td - r).abs() / (count[k] * UNIT * mag[rk])).flatten()
            i = int(torch.argmax(torch.nan_to_num(frac, nan=float("inf"))))
            figs[k] = (float(frac[i]), i)
            bad = not figs[k][0] <= 1.0
        else:
            e = rel(t, r)
            figs[k] = (e / WGRAD_TENSOR_TOL, -1)
            bad = not e <= WGRAD_TENSOR_TOL
        if bad:
            miss.append(k)
    return figs, miss


def check_linear(got, prob, what, *, bias: bool = True, gemm: bool = False, worst: Optional[dict] = None,
                 misses: Optional[list] = None):
    """linear_misses, asserted -- or, given `misses`, collected there for one assertion after every leg has run;
    `worst` gathers the randn kind's largest fraction per quantity, with the leg and the element"""
    figs, miss = linear_misses(got, prob, bias=bias, gemm=gemm)
    if worst is not None and prob["kind"] == "randn":
        for k, (f, i) in figs.items():
            if f > worst.get(k, (-1.0,))[0]:
                worst[k] = (f, what, i)
    if misses is not None:
        misses += [(what, prob["kind"], k, figs[k]) for k in miss]
    else:
        assert not miss, (what, prob["kind"], {k: figs[k] for k in miss})
    return figs


# ---------------------------------------------------------------------------------------------------------------------
# buffers whose view is not 16-byte aligned
# ---------------------------------------------------------------------------------------------------------------------
class Shifted(Guarded):
    """a Guarded whose view starts 4 bytes into the space between the guards (one more guard word before it): the
    library's 16-byte alignment tests fail on it"""
    SHIFT = 1

    def __init__(self, name: str, shape, device, src: Optional[torch.Tensor] = None):
        self.name = name
        self.shape = tuple(int(s) for s in shape)
        self.n = int(np.prod(self.shape)) if self.shape else 1
        self.lo = F._G + self.SHIFT
        self.raw = torch.full((self.lo + self.n + F._G,), F._GUARD_I32, dtype=torch.int32, device=device)
        self.t = self.raw[self.lo:self.lo + self.n].view(torch.float32).view(self.shape)
        self.is_input = src is not None
        if src is not None:
            self.t.copy_(src.reshape(self.shape))
        else:
            self.poison()
        assert self.ptr % 16 == 4 * self.SHIFT

    @property
    def ptr(self) -> int:
        return self.raw.data_ptr() + 4 * self.lo

    def poison(self) -> None:
        self.raw[self.lo:self.lo + self.n].fill_(-1)

    def broken_guards(self) -> List[str]:
        bad = []
        for side, g, base in (("before", self.raw[:self.lo], -self.lo), ("after", self.raw[self.lo + self.n:], self.n)):
            diff = torch.nonzero(g != F._GUARD_I32).flatten()
            if diff.numel():
                bad.append(f"{self.name}: {diff.numel()} guard words {side} the view changed, first at element "
                           f"{base + int(diff[0])}")
        return bad


def _new(bufs: Buffers, name, shape, src=None, misalign=None) -> Guarded:
    g = (Shifted if name == misalign else Guarded)(name, shape, bufs.device, src)
    bufs.all[name] = g
    return g


def _unchanged(bufs: Buffers, srcs: Dict[str, torch.Tensor], what) -> None:
    for k, s in srcs.items():
        assert torch.equal(bufs.all[k].t.view(torch.int32), s.to(bufs.device).view(torch.int32).reshape(bufs.all[k].shape)), \
            (what, k, "input changed")


# ---------------------------------------------------------------------------------------------------------------------
# rpde_linear_fwd / rpde_linear_bwd
# ---------------------------------------------------------------------------------------------------------------------
def run_linear_thin(dev, prob, *, bias: bool = True, want: Sequence[str] = ("dx", "dW", "db"),
                    misalign: Optional[str] = None, env: Optional[Dict[str, str]] = None) -> Dict[str, torch.Tensor]:
    """forward and backward in guarded, poisoned buffers -> y and the outputs in `want`, on the device.  Outputs not in
    `want` are NULL; bias=False passes b = NULL to the forward; `misalign` names the one view of y / x / grad_out / dx
    that starts 4 bytes into its allocation; the workspace is exactly rpde_linear_ws_bytes, poisoned like the outputs"""
    from rpde import _lib
    lib = _lib.load()
    assert misalign in (None,) + MISALIGN and set(want) <= {"dx", "dW", "db"} and (misalign != "dx" or "dx" in want)
    P, out_f, in_f = prob["P"], prob["out_f"], prob["in_f"]
    what = f"linear {prob['kind']} P={P} in={in_f} out={out_f} bias={bias} want={tuple(want)} misalign={misalign} env={env}"
    bufs = Buffers(dev)
    srcs = {"x": prob["x"], "grad_out": prob["g"], "w": prob["w"], "b": prob["b"]}
    X, Gy = _new(bufs, "x", (P, in_f), prob["x"], misalign), _new(bufs, "grad_out", (P, out_f), prob["g"], misalign)
    W, B = _new(bufs, "w", (out_f, in_f), prob["w"]), _new(bufs, "b", (out_f,), prob["b"])
    y = _new(bufs, "y", (P, out_f), None, misalign)
    gx = _new(bufs, "dx", (P, in_f), None, misalign) if "dx" in want else None
    gw = _new(bufs, "dW", (out_f, in_f)) if "dW" in want else None
    gb = _new(bufs, "db", (out_f,)) if "db" in want else None
    st = _lib.stream_ptr()
    with Env(env):                                   # (the workspace query reads the switches too)
        nws = int(lib.rpde_linear_ws_bytes(P, in_f, out_f))
        ws = bufs.new_bytes("ws", nws)
        _lib.check(lib.rpde_linear_fwd(X.ptr, W.ptr, B.ptr if bias else None, y.ptr, P, in_f, out_f, st), "linear_fwd")
        _lib.check(lib.rpde_linear_bwd(X.ptr, W.ptr, Gy.ptr, F.ptr_or_none(gx), F.ptr_or_none(gw), F.ptr_or_none(gb), P, in_f,
                                       out_f, ws.ptr, nws, st), "linear_bwd")
        torch.cuda.synchronize()
    bufs.check(["y", *want], what)
    _unchanged(bufs, srcs, what)
    return {k: bufs.all[k].t for k in ("y", *want)}


# ---------------------------------------------------------------------------------------------------------------------
# the convolution problem, its float64 reference and rpde_conv1x1_fwd / rpde_conv1x1_act_fwd
# ---------------------------------------------------------------------------------------------------------------------
_ACT = {"identity": lambda v: v, "gelu": Fn.gelu, "relu": Fn.relu}
ACT_ID = {"identity": 0, "gelu": 1, "relu": 2}           # include/rpde.h RPDE_ACT_*


@functools.lru_cache(maxsize=1)
def conv_problem(kind: str, case: Tuple[int, int, int, int], device: str = "cpu"):
    """x [B, Cin, S], out0 [B, Cout, S] (what `out` holds before an accumulating call), w [Cout, Cin], b [Cout] in float32.
    w and b are drawn on the CPU; x and out0 on `device` (the CPU unless x has DEVICE_RESIDENT elements or more)"""
    assert kind in KINDS
    B, Cin, Cout, S = case
    crc = zlib.crc32(repr(("conv", kind, case)).encode())
    with torch.random.fork_rng():
        torch.manual_seed(crc)
        if kind == "exact":
            w, b = _ints(Cout, Cin), _ints(Cout)
        else:
            lin = torch.nn.Linear(Cin, Cout)
            w = (lin.weight.detach() * (1 + 0.3 * torch.randn(Cout, Cin))).contiguous()
            b = lin.bias.detach().clone()
    gen = torch.Generator(device=device)
    gen.manual_seed(crc)
    if kind == "exact":
        x, out0 = _ints(B, Cin, S, device=device, generator=gen), _ints(B, Cout, S, device=device, generator=gen)
    else:
        x = torch.randn(B, Cin, S, device=device, generator=gen)
        out0 = torch.randn(B, Cout, S, device=device, generator=gen)
    return dict(kind=kind, case=case, x=x, out0=out0, w=w, b=b)


def conv_device(case, dev) -> str:
    B, Cin, Cout, S = case
    return str(dev) if B * Cin * S >= DEVICE_RESIDENT else "cpu"


REF_ON_DEVICE = 1 << 26                      # multiply-adds from which the float64 reference is formed on the device


def conv_ref_device(case, dev) -> str:
    """where a GPU test forms the float64 reference: on the CPU while that takes a second or so for all the legs of a
    case, beyond that with torch float64 on the device, cross-checked against the CPU on 2 x CROSS_POINTS points"""
    B, Cin, Cout, S = case
    return str(dev) if B * Cin * Cout * S >= REF_ON_DEVICE else "cpu"


def conv_reference(prob, act_in: str, act_out: str, accumulate: int, bias: bool = True, gemm: bool = False,
                   points: Optional[slice] = None, device=None):
    """-> (ref, bound) in float64 [B, Cout, S'] on the problem's device (or `device`), formed in pieces of at most 2^24
    input elements; `points` restricts S.  The exact kind needs every element's term magnitudes below 2^24"""
    x, out0, w, b = prob["x"], prob["out0"], prob["w"], prob["b"]
    if points is not None:
        x, out0 = x[:, :, points], out0[:, :, points]
    dev = x.device if device is None else torch.device(device)
    B, Cin, S = x.shape
    Cout = w.shape[0]
    wd, bd = w.double().to(dev), (b.double() if bias else torch.zeros(Cout, dtype=torch.float64)).to(dev)
    ref = torch.empty(B, Cout, S, dtype=torch.float64, device=dev)
    bnd = torch.empty_like(ref)
    cs = min(S, max(1, (1 << 24) // Cin))
    bs = min(B, max(1, (1 << 24) // (Cin * cs)))
    count = Cin + 3 + (ROW_MARGIN if gemm else 0.0)
    worst = 0.0
    for b0 in range(0, B, bs):
        for s0 in range(0, S, cs):
            xa = _ACT[act_in](x[b0:b0 + bs, :, s0:s0 + cs].to(dev).double())
            pre = torch.einsum("oi,bis->bos", wd, xa) + bd[None, :, None]
            mag = torch.einsum("oi,bis->bos", wd.abs(), xa.abs()) + bd.abs()[None, :, None]
            if accumulate:
                o0 = out0[b0:b0 + bs, :, s0:s0 + cs].to(dev).double()
                pre, mag = pre + o0, mag + o0.abs()
            worst = max(worst, float(mag.max()))
            e = count * UNIT * mag
            if act_in == "gelu":
                e = e + GELU_TOL * wd.abs().sum(1)[None, :, None]
            if act_out == "gelu":
                e = DGELU_MAX * e + GELU_TOL
            ref[b0:b0 + bs, :, s0:s0 + cs] = _ACT[act_out](pre)
            bnd[b0:b0 + bs, :, s0:s0 + cs] = e
    if prob["kind"] == "exact":
        assert worst < EXACT_LIMIT, (prob["case"], worst)
    return ref, bnd


def conv_is_exact(prob, act_in: str, act_out: str) -> bool:
    """integers in, integers out: the result must equal float64 bit for bit"""
    return prob["kind"] == "exact" and act_in in ("identity", "relu") and act_out in ("identity", "relu")


def conv_misses(got: torch.Tensor, ref: torch.Tensor, bnd: torch.Tensor, exact: bool):
    """-> (figure, flat index, missed): the worst fraction of the bound (exact: the number of elements that differ)"""
    td = got.to(ref.device).double()
    assert td.shape == ref.shape, (td.shape, ref.shape)
    if exact:
        ne = (td != ref).flatten()
        n = int(ne.sum())
        return float(n), (int(torch.nonzero(ne)[0]) if n else -1), n > 0
    frac = ((td - ref).abs() / bnd).flatten()
    i = int(torch.argmax(torch.nan_to_num(frac, nan=float("inf"))))
    f = float(frac[i])
    return f, i, not f <= 1.0


def run_conv_small(dev, prob, *, act_in: str = "identity", act_out: str = "identity", accumulate: int = 0,
                   bias: bool = True, misalign: Optional[str] = None, env: Optional[Dict[str, str]] = None) -> torch.Tensor:
    """rpde_conv1x1_fwd (act_out identity) or rpde_conv1x1_act_fwd in guarded buffers -> out on the device.  `out` starts
    from the problem's out0 when accumulating and poisoned otherwise; `misalign` names x or out"""
    from rpde import _lib
    lib = _lib.load()
    assert misalign in (None, "x", "out")
    B, Cin, Cout, S = prob["case"]
    what = f"conv {prob['kind']} {prob['case']} {act_in}/{act_out} acc={accumulate} bias={bias} misalign={misalign} env={env}"
    bufs = Buffers(dev)
    X = _new(bufs, "x", (B, Cin, S), prob["x"], misalign)
    W, Bv = _new(bufs, "w", (Cout, Cin), prob["w"]), _new(bufs, "b", (Cout,), prob["b"])
    out = _new(bufs, "out", (B, Cout, S), prob["out0"] if accumulate else None, misalign)
    st = _lib.stream_ptr()
    with Env(env):
        if act_out == "identity":
            _lib.check(lib.rpde_conv1x1_fwd(X.ptr, W.ptr, Bv.ptr if bias else None, out.ptr, B, Cin, Cout, S, ACT_ID[act_in],
                                            int(accumulate), st), "conv1x1_fwd")
        else:
            _lib.check(lib.rpde_conv1x1_act_fwd(X.ptr, W.ptr, Bv.ptr if bias else None, out.ptr, B, Cin, Cout, S,
                                                ACT_ID[act_in], int(accumulate), ACT_ID[act_out], st), "conv1x1_act_fwd")
        torch.cuda.synchronize()
    bufs.check(["out"], what)
    _unchanged(bufs, {"w": prob["w"], "b": prob["b"]}, what)
    assert torch.equal(X.t.view(torch.int32), prob["x"].to(dev).view(torch.int32)), (what, "x changed")
    return out.t
