"""A ctypes harness for the FeedForward and linear entry points of the C ABI (include/rpde.h), for tests that own every
buffer: tests/test_gpu_ff_edges.py on the GPU and tests/test_ff_edges_ref_cpu.py for what those tests rest on.

Guarded buffers.  Every tensor the library writes, the workspace included, is a view into a larger allocation with
GUARD_BYTES (32 rows x 256 floats: a whole padded tile of the widest tensor) before and after it, filled with GUARD_WORD,
a NaN with a payload of its own.  After a call the guards must be bit-identical.  The tensors the library only reads sit
in such allocations too, so a read past a partial tile meets a NaN, not a lucky zero.  The workspace view is exactly the
byte count the *_ws_bytes query returned.

Poison.  Before a call every output and the whole workspace are filled with bytes 0xFF (a NaN); afterwards every output
element must be finite: "read a slab nobody wrote" and "did not store the last row" fail.

Oracle.  oracle.reference_path.feedforward in float64 with the restated masks of oracle.dropout_mask, post-activation and
residual applied as tests/test_gpu_dropout_parity.py does; and the same expression in float32 torch on the CPU, whose
error against float64 is what every per-row / per-column bound is a multiple of.  Nothing is calibrated on a kernel."""
from __future__ import annotations

import ctypes as C
import functools
import os
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

DIM, FACTOR, LAYERS, HID = 64, 4, 3, 256
FF_FWD_TOL, FF_GRAD_TOL = 5e-6, 2e-5          # tests/test_gpu_dropout_parity.py
WGRAD_TOL = 2e-6                              # tests/test_gpu_fused_paths.py::test_streaming_weight_gradient_kernel
ROW_MARGIN = 16.0                             # h2.h: <= 3 * 2^-22 = 12 fp32 roundoffs per product, rounded up
MISS = 100.0
WG_CHUNKS, WG_MIN_P = 256, 32 * 256           # csrc/wgrad_h2.hip: WG_BLOCKS chunks, streaming from P >= 8192

GUARD_BYTES = 32 * 256 * 4
GUARD_WORD = 0x7FE5C3A5                       # a quiet NaN with a payload: exponent all ones, mantissa 0x65C3A5
_GUARD_I32 = GUARD_WORD - (1 << 32) if GUARD_WORD >= (1 << 31) else GUARD_WORD
_G = GUARD_BYTES // 4
assert GUARD_BYTES % 256 == 0


# ---------------------------------------------------------------------------------------------------------------------
# guarded, poisoned buffers (CPU or GPU tensors alike)
# ---------------------------------------------------------------------------------------------------------------------
class Guarded:
    """guard | view | guard in one int32 allocation; `t` is the float32 view of `shape` (or of nbytes / 4 floats)"""

    def __init__(self, name: str, shape, device, src: Optional[torch.Tensor] = None):
        self.name = name
        self.shape = tuple(int(s) for s in shape)
        self.n = int(np.prod(self.shape)) if self.shape else 1
        self.raw = torch.full((2 * _G + self.n,), _GUARD_I32, dtype=torch.int32, device=device)
        self.t = self.raw[_G:_G + self.n].view(torch.float32).view(self.shape)
        self.is_input = src is not None
        if src is not None:
            self.t.copy_(src.reshape(self.shape))
        else:
            self.poison()

    @classmethod
    def of_bytes(cls, name: str, nbytes: int, device) -> "Guarded":
        assert nbytes % 4 == 0, nbytes
        return cls(name, (nbytes // 4,), device)

    @property
    def ptr(self) -> int:
        return self.raw.data_ptr() + 4 * _G

    @property
    def nbytes(self) -> int:
        return 4 * self.n

    def poison(self) -> None:
        self.raw[_G:_G + self.n].fill_(-1)               # bytes 0xFF: a NaN in every float

    def broken_guards(self) -> List[str]:
        """where the guards differ from the pattern: element offsets relative to the view (negative: before it)"""
        bad = []
        for side, g, base in (("before", self.raw[:_G], -_G), ("after", self.raw[_G + self.n:], self.n)):
            diff = torch.nonzero(g != _GUARD_I32).flatten()
            if diff.numel():
                bad.append(f"{self.name}: {diff.numel()} guard words {side} the view changed, first at element "
                           f"{base + int(diff[0])}")
        return bad

    def non_finite(self) -> int:
        return int((~torch.isfinite(self.t)).sum()) if self.n else 0


class Buffers:
    """the guarded allocations of one call sequence"""

    def __init__(self, device):
        self.device = device
        self.all: Dict[str, Guarded] = {}

    def new(self, name, shape, src=None) -> Guarded:
        g = Guarded(name, shape, self.device, src)
        self.all[name] = g
        return g

    def new_bytes(self, name, nbytes) -> Guarded:
        g = Guarded.of_bytes(name, nbytes, self.device)
        self.all[name] = g
        return g

    def check(self, finite: Sequence[str], what: str) -> None:
        """every guard intact (inputs' and workspaces' too) and every element of the named outputs finite"""
        bad: List[str] = []
        for g in self.all.values():
            bad += g.broken_guards()
        assert not bad, (what, bad)
        nf = {k: self.all[k].non_finite() for k in finite}
        assert not any(nf.values()), (what, "non-finite output elements (poison left or NaN computed)", nf)


class Env:
    """environment switches of the library (read at every call) for the length of a with block"""

    def __init__(self, kv: Optional[Dict[str, str]]):
        self.kv = dict(kv or {})

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def ptr_or_none(g: Optional[Guarded]):
    return g.ptr if g is not None else None


def ptr_list(gs: Optional[Sequence[Optional[Guarded]]]):
    """NULL for None, else a void*[] of the views' addresses (NULL entries for None)"""
    if gs is None:
        return None
    arr = (C.c_void_p * len(gs))()
    for i, g in enumerate(gs):
        arr[i] = g.ptr if g is not None else None
    return C.cast(arr, C.POINTER(C.c_void_p))


# ---------------------------------------------------------------------------------------------------------------------
# error figures
# ---------------------------------------------------------------------------------------------------------------------
def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def row_fig(a: torch.Tensor, ref: torch.Tensor, rows: Optional[Sequence[int]] = None) -> float:
    """a row's L2 error over the RMS of the reference's row norms, maximum over (the given) rows"""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    e = (a - ref).norm(dim=1)
    scale = float(ref.norm(dim=1).pow(2).mean().sqrt().clamp_min(1e-30))
    if rows is not None:
        e = e[torch.as_tensor(list(rows), dtype=torch.long)]
    return float(e.max()) / scale


def tail_rows(P: int) -> List[int]:
    """the first row of the last tile of 32 points and the last P % 32 rows"""
    first = 32 * ((P - 1) // 32)
    return sorted({first, *range(P - P % 32, P)})


def line_figs(a: torch.Tensor, ref: torch.Tensor, dim: int) -> torch.Tensor:
    """relative L2 error of every column (dim 0 reduced) or row (dim 1 reduced) of a matrix"""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return (a - ref).norm(dim=dim) / ref.norm(dim=dim).clamp_min(1e-300)


# ---------------------------------------------------------------------------------------------------------------------
# the FeedForward problem (dim 64, factor 4, three layers), its float64 oracle and its float32 calibration
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class FFSpec:
    P: int
    residual: bool = True
    layer_norm: bool = True
    post_act: str = "identity"
    p: float = 0.0
    epoch: int = 0
    grad_x: bool = True
    grad_biases: bool = True

    def oracle_key(self):
        return (self.P, self.residual, self.layer_norm, self.post_act, self.p, self.epoch)


GRAD_NAMES = ["dW0", "dW1", "dW2", "db0", "db1", "db2", "dgamma", "dbeta"]


def _post(name, t):
    return {"identity": lambda v: v, "gelu": F.gelu, "relu": F.relu}[name](t)


@functools.lru_cache(maxsize=4)
def ff_problem(P, residual, layer_norm, post_act, p, epoch):
    """weights (nn.Linear's default initialisation times 1 + 0.3 randn, contiguous; a LayerNorm with non-trivial affine
    parameters), plain randn inputs without row scaling, the seed and the restated masks: all on the CPU, float32"""
    from oracle import dropout_mask as D
    crc = zlib.crc32(repr((P, residual, layer_norm, post_act, p, epoch)).encode())
    with torch.random.fork_rng():
        torch.manual_seed(crc)
        sd = {}
        for i, (o, k) in enumerate([(HID, DIM), (HID, HID), (DIM, HID)]):
            lin = torch.nn.Linear(k, o)
            sd[f"layers.{i}.0.weight"] = (lin.weight.detach() * (1 + 0.3 * torch.randn(o, k))).contiguous()
            sd[f"layers.{i}.0.bias"] = lin.bias.detach().clone()
        if layer_norm:
            sd["layers.2.3.weight"] = 1 + 0.3 * torch.randn(DIM)
            sd["layers.2.3.bias"] = 0.3 * torch.randn(DIM)
        x = torch.randn(P, DIM)
        r = torch.randn(P, DIM) if residual else None
        probe = torch.randn(P, DIM)
    seed = 0xD1B54A32D192ED03 ^ crc
    masks = None
    if p > 0.0:
        masks = [D.layer_mask(seed, l, epoch, p, P, o) for l, o in enumerate([HID, HID, DIM])]
    return dict(sd=sd, x=x, r=r, probe=probe, seed=seed, masks=masks, P=P, layer_norm=layer_norm, post_act=post_act,
                p=p, epoch=epoch)


def ff_eval(prob, dtype, rows: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """out and every gradient of sum(out * probe) in `dtype` on the CPU, of the first `rows` points (default: all)"""
    from oracle import reference_path as R
    n = prob["P"] if rows is None else rows
    sd = {k: v.detach().to(dtype, copy=True).requires_grad_() for k, v in prob["sd"].items()}
    xd = prob["x"][:n].detach().to(dtype, copy=True).requires_grad_()
    masks = [m[:n] for m in prob["masks"]] if prob["masks"] is not None else None
    y = R.feedforward(xd, sd, "", LAYERS, prob["layer_norm"], masks=masks)
    y = _post(prob["post_act"], y)
    if prob["r"] is not None:
        y = y + prob["r"][:n].to(dtype)
    (y * prob["probe"][:n].to(dtype)).sum().backward()
    res = {"out": y.detach(), "dx": xd.grad}
    for l in range(LAYERS):
        res[f"dW{l}"] = sd[f"layers.{l}.0.weight"].grad
        res[f"db{l}"] = sd[f"layers.{l}.0.bias"].grad
    if prob["layer_norm"]:
        res["dgamma"], res["dbeta"] = sd["layers.2.3.weight"].grad, sd["layers.2.3.bias"].grad
    return res


@functools.lru_cache(maxsize=4)
def ff_oracle(key):
    """-> (problem, float64 reference, float32 figures, float64 reference with the last point left out of every reduction)
    f32 figures: global relative L2 per tensor, and 'row:out' / 'row:dx' (row_fig over all rows); the reference also
    holds 'u0' = dropout(z) of the first hidden layer, which tells the training modes apart"""
    prob = ff_problem(*key)
    ref = ff_eval(prob, torch.float64)
    f32 = ff_eval(prob, torch.float32)
    figs = {k: rel(f32[k], ref[k]) for k in ref}
    for k in ("out", "dx"):
        figs["row:" + k] = row_fig(f32[k], ref[k])
    fault = ff_eval(prob, torch.float64, rows=prob["P"] - 1)
    fault = {k: v for k, v in fault.items() if k in GRAD_NAMES}
    u = F.linear(prob["x"].double(), prob["sd"]["layers.0.0.weight"].double(), prob["sd"]["layers.0.0.bias"].double())
    ref["u0"] = u * prob["masks"][0] if prob["masks"] is not None else u
    return prob, ref, figs, fault


def fault_factor(P: int, T: int) -> Optional[float]:
    """the planted fault (last point left out) must miss by this multiple of FF_GRAD_TOL; None: not asserted at this P"""
    if P < 64:
        return 10.0 * MISS
    if P >= T - 1:
        return MISS
    return None


def fault_misses(got: Dict[str, torch.Tensor], fault: Dict[str, torch.Tensor]) -> Dict[str, float]:
    return {k: rel(got[k], fault[k]) for k in fault if k in got}


# ---------------------------------------------------------------------------------------------------------------------
# the cases: point counts relative to T = 32 * CUs (one tile of 32 points per workgroup), modes and contract variants
# ---------------------------------------------------------------------------------------------------------------------
FF_MODES = ("train", "recompute", "eval", "prepared")
# name -> (multiple of T, offset)
FF_POINTS = {"31": (0, 31), "32": (0, 32), "33": (0, 33), "47": (0, 47), "48": (0, 48), "49": (0, 49), "63": (0, 63),
             "64": (0, 64), "T-1": (1, -1), "T": (1, 0), "T+1": (1, 1), "T+31": (1, 31), "12345": (0, 12345),
             "2T-15": (2, -15)}
FF_FULL = ("33", "T+1")                        # the full cross product of modes, the variants, reproducibility
FF_VARIANTS = {
    "base": {},
    "no-residual": dict(residual=False),
    "no-layernorm": dict(layer_norm=False),
    "gelu": dict(post_act="gelu"),
    "relu": dict(post_act="relu"),
    "no-grad-x": dict(grad_x=False),
    "no-grad-biases": dict(grad_biases=False),
    "dropout": dict(p=0.25, epoch=(1 << 32) + 5),
    "all-at-once": dict(residual=False, layer_norm=False, post_act="gelu", grad_x=False, p=0.25, epoch=(1 << 32) + 5),
}


def resolve_points(name: str, T: int) -> int:
    m, o = FF_POINTS[name]
    return m * T + o


def ff_cases():
    """(point name, variant name): every point count with the base contract, every variant at the FF_FULL points"""
    return [(pn, "base") for pn in FF_POINTS] + [(pn, vn) for pn in FF_FULL for vn in FF_VARIANTS if vn != "base"]


def ff_modes(point: str, variant: str) -> Sequence[str]:
    """training first; the full cross product at the FF_FULL points, elsewhere one more mode, rotated over the point
    counts.  P = 31 is not fused: the GEMM path trains and evaluates with hs.  Dropout has no evaluation"""
    if point == "31":
        return ("train", "eval")
    if variant != "base":
        return ("train", "recompute")
    if point in FF_FULL:
        return FF_MODES
    others = [pn for pn in FF_POINTS if pn != "31" and pn not in FF_FULL]
    return ("train", FF_MODES[1 + others.index(point) % 3])


# ---------------------------------------------------------------------------------------------------------------------
# the FeedForward through the C ABI
# ---------------------------------------------------------------------------------------------------------------------


def run_ff(dev, prob, spec: FFSpec, mode: str, env: Optional[Dict[str, str]] = None) -> Dict[str, object]:
    with Env(env):                                   # (the workspace queries read the switches too)
        return _run_ff(dev, prob, spec, mode)


def _run_ff(dev, prob, spec: FFSpec, mode: str) -> Dict[str, object]:
    """forward (and, for train / recompute, backward) of `prob` in guarded, poisoned buffers.
    train: hs + ds;  recompute: hs only, ds NULL (k_ff3_bwd_h2<true>, the ACT instantiation of k_wgrad_h2);
    eval: hs, ds NULL -- only `out`;  prepared: rpde_feedforward_prepare + _fwd_prepared.
    A shape the library does not fuse takes the GEMM path: it needs hs (and ds to train), recompute / prepared are
    refused here.  -> CPU copies of every output, 'is_fused', and 'hs0' (what the forward saved for the first hidden
    layer: h = gelu(u) when training, u = dropout(z) in recompute mode)"""
    from rpde import _lib, ops
    lib = _lib.load()
    P, sd = prob["P"], prob["sd"]
    ln = prob["layer_norm"]
    fused = int(lib.rpde_feedforward_is_fused(DIM, FACTOR, LAYERS, P))
    assert mode in FF_MODES and (fused or mode in ("train", "eval")), (mode, fused)
    w = [sd[f"layers.{l}.0.weight"].to(dev).contiguous() for l in range(LAYERS)]
    b = [sd[f"layers.{l}.0.bias"].to(dev).contiguous() for l in range(LAYERS)]
    assert all(t.data_ptr() % 16 == 0 for t in w)
    gamma = sd["layers.2.3.weight"].to(dev) if ln else None
    beta = sd["layers.2.3.bias"].to(dev) if ln else None
    bufs = Buffers(dev)
    X = bufs.new("x", (P, DIM), prob["x"])
    Rs = bufs.new("residual", (P, DIM), prob["r"]) if prob["r"] is not None else None
    out = bufs.new("out", (P, DIM))
    training = mode in ("train", "recompute")
    keep_h = training or not fused
    z_last = bufs.new("z_last", (P, DIM)) if keep_h else None
    hs = [bufs.new(f"hs{l}", (P, HID)) for l in range(2)] if keep_h else None
    ds = [bufs.new(f"ds{l}", (P, HID)) for l in range(2)] if mode == "train" else None
    wa, ba = _lib.ptr_array(w), _lib.ptr_array(b)
    ep = ops.drop_epoch(dev) if prob["p"] > 0.0 else None
    fp = _lib.FFParams(LAYERS, DIM, FACTOR, int(ln), 1e-5, prob["p"], prob["seed"], _lib.ACT[prob["post_act"]],
                       C.cast(wa, C.POINTER(C.c_void_p)), C.cast(ba, C.POINTER(C.c_void_p)), _lib.ptr(gamma),
                       _lib.ptr(beta), ep.data_ptr() if ep is not None else None)
    nws_f = int(lib.rpde_feedforward_fwd_ws_bytes(DIM, FACTOR, LAYERS))
    ws_f = bufs.new_bytes("fwd_ws", nws_f)
    st = _lib.stream_ptr()
    res: Dict[str, object] = {"is_fused": fused}
    try:
        if ep is not None:
            ep.fill_(prob["epoch"])
        if mode == "prepared":
            _lib.check(lib.rpde_feedforward_prepare(C.byref(fp), ws_f.ptr, nws_f, st), "feedforward_prepare")
            _lib.check(lib.rpde_feedforward_fwd_prepared(C.byref(fp), X.ptr, ptr_or_none(Rs), out.ptr, P, ws_f.ptr, nws_f, st),
                       "feedforward_fwd_prepared")
        else:
            # (evaluation: the fused kernel does not write z_last; rpde.ops passes `out` there, and so does this)
            _lib.check(lib.rpde_feedforward_fwd(C.byref(fp), X.ptr, ptr_or_none(Rs), ptr_list(hs), ptr_list(ds),
                                                z_last.ptr if z_last is not None else out.ptr, out.ptr, P, ws_f.ptr, nws_f, st),
                       "feedforward_fwd")
        torch.cuda.synchronize()
        written = ["out"] + (["z_last", "hs0", "hs1"] if keep_h else []) + (["ds0", "ds1"] if ds else [])
        bufs.check(written, f"forward {mode} P={P}")
        res["out"] = out.t.cpu().clone()
        if not training:
            return res
        res["hs0"] = hs[0].t.cpu().clone()

        G = bufs.new("grad_out", (P, DIM), prob["probe"])
        gx = bufs.new("dx", (P, DIM)) if spec.grad_x else None
        gW = [bufs.new(f"dW{l}", tuple(w[l].shape)) for l in range(LAYERS)]
        gb = [bufs.new(f"db{l}", tuple(b[l].shape)) for l in range(LAYERS)] if spec.grad_biases else None
        gga = bufs.new("dgamma", (DIM,)) if ln else None
        gbe = bufs.new("dbeta", (DIM,)) if ln else None
        nws_b = int(lib.rpde_feedforward_ws_bytes(P, DIM, FACTOR, LAYERS))
        ws_b = bufs.new_bytes("bwd_ws", nws_b)
        saved = {k: bufs.all[k].t.clone() for k in written}
        _lib.check(lib.rpde_feedforward_bwd(C.byref(fp), X.ptr, ptr_list(hs), ptr_list(ds), z_last.ptr, G.ptr, ptr_or_none(gx),
                                            ptr_list(gW), ptr_list(gb), ptr_or_none(gga), ptr_or_none(gbe), P, ws_b.ptr,
                                            nws_b, st), "feedforward_bwd")
        torch.cuda.synchronize()
        outs = [k for k in ["dx"] + GRAD_NAMES if k in bufs.all]
        bufs.check(outs, f"backward {mode} P={P}")
        for k, v in saved.items():                       # the backward only reads what the forward saved
            assert torch.equal(bufs.all[k].t.view(torch.int32), v.view(torch.int32)), (k, "changed by the backward")
        for k in outs:
            res[k] = bufs.all[k].t.cpu().clone()
        return res
    finally:
        if ep is not None:
            ep.zero_()


# ---------------------------------------------------------------------------------------------------------------------
# the weight gradient alone: rpde_linear_bwd
# ---------------------------------------------------------------------------------------------------------------------
WGRAD_SHAPES = [(256, 256), (64, 256), (256, 64)]                 # (out, in): what wgrad_h2_ok accepts
WGRAD_KINDS = ("plain", "zero_prefix", "zero_block", "huge_closing", "descending", "channel_spread")
# kinds whose bound is 4 x the float32 matmul's own error where that error exceeds WGRAD_TOL (set from the CPU figures
# of tests/test_ff_edges_ref_cpu.py, never from a kernel)
FOUR_X_RULE = ("descending",)


def chunk_steps(P: int) -> List[int]:
    """steps of 32 points that each of the 256 chunks of k_wgrad_h2 owns: [steps c / 256, steps (c + 1) / 256)"""
    steps = (P + 31) // 32
    return [steps * (c + 1) // WG_CHUNKS - steps * c // WG_CHUNKS for c in range(WG_CHUNKS)]


def one_step_chunk(P: int) -> int:
    """the first step of a chunk of exactly one step, the one nearest the middle of the stream"""
    steps = (P + 31) // 32
    ones = [c for c, n in enumerate(chunk_steps(P)) if n == 1 and c > 0]
    assert ones, P
    c = min(ones, key=lambda c_: abs(c_ - WG_CHUNKS // 2))
    return steps * c // WG_CHUNKS


@functools.lru_cache(maxsize=2)
def wgrad_problem(kind: str, P: int, out_f: int, in_f: int):
    """x [P, in], grad_out [P, out], w [out, in], b [out] on the CPU in float32, with the float64 results and the float32 CPU
    matmuls' figures.  The structured kinds shape `x` at P = 8193 and `grad_out` at the other P, so that both operands'
    loader waves meet them."""
    assert kind in WGRAD_KINDS
    crc = zlib.crc32(repr((kind, P, out_f, in_f)).encode())
    with torch.random.fork_rng():
        torch.manual_seed(crc)
        x = torch.randn(P, in_f)
        g = torch.randn(P, out_f)
        lin = torch.nn.Linear(in_f, out_f)
        w = (lin.weight.detach() * (1 + 0.3 * torch.randn(out_f, in_f))).contiguous()
        b = lin.bias.detach().clone()
    one = x if P == 8193 else g
    info: Dict[str, object] = {}
    if kind == "zero_prefix":                 # running exponents start at their floor and first move mid-chunk
        x[:4096] = 0
        g[:4096] = 0
    elif kind == "zero_block":                # one 64-channel block of grad_out is zero for all points
        blk = 1 if out_f > 64 else 0
        g[:, 64 * blk:64 * blk + 64] = 0
        info["zero_rows"] = (64 * blk, 64 * blk + 64)
    elif kind == "huge_closing":              # a one-step chunk holds a row 2^20 above everything before it
        s = one_step_chunk(P)
        one[32 * s + 31] *= 2.0 ** 20
        info["row"] = 32 * s + 31
    elif kind == "descending":                # 2^10 down to 2^-20, one binary place per 256 points
        lvl = torch.clamp(torch.arange(P) // 256, max=30).double()
        one *= torch.pow(2.0, 10 - lvl).float()[:, None]
    elif kind == "channel_spread":            # channel magnitudes over 2^+-8, every value in every 64-channel panel
        x *= torch.pow(2.0, ((torch.arange(in_f) * 5) % 17 - 8).double()).float()[None, :]
        g *= torch.pow(2.0, ((torch.arange(out_f) * 7 + 3) % 17 - 8).double()).float()[None, :]
    ref = {"y": x.double() @ w.double().t() + b.double(), "dW": g.double().t() @ x.double(), "db": g.double().sum(0),
           "dx": g.double() @ w.double()}
    f32 = {"y": x @ w.t() + b, "dW": g.t() @ x, "db": g.sum(0), "dx": g @ w}
    figs = {k: rel(f32[k], ref[k]) for k in ref}
    if kind == "channel_spread":
        info["f32_cols"] = line_figs(f32["dW"], ref["dW"], 0)
        info["f32_rows"] = line_figs(f32["dW"], ref["dW"], 1)
    return dict(kind=kind, P=P, out_f=out_f, in_f=in_f, x=x, g=g, w=w, b=b, ref=ref, f32=figs, info=info)


def wgrad_bound(kind: str, f32_err: float) -> float:
    """WGRAD_TOL, or for a FOUR_X_RULE kind on which the float32 matmul itself misses it, 4 x that matmul's error"""
    if f32_err <= WGRAD_TOL or kind not in FOUR_X_RULE:
        return WGRAD_TOL
    return 4.0 * f32_err


def run_linear(dev, prob, env: Optional[Dict[str, str]] = None) -> Dict[str, torch.Tensor]:
    """rpde_linear_fwd and rpde_linear_bwd in guarded, poisoned buffers -> CPU copies of y, dW, db, dx"""
    from rpde import _lib
    lib = _lib.load()
    P, out_f, in_f = prob["P"], prob["out_f"], prob["in_f"]
    bufs = Buffers(dev)
    X = bufs.new("x", (P, in_f), prob["x"])
    Gy = bufs.new("grad_out", (P, out_f), prob["g"])
    W, B = prob["w"].to(dev), prob["b"].to(dev)
    y = bufs.new("y", (P, out_f))
    gx, gw, gb = bufs.new("dx", (P, in_f)), bufs.new("dW", (out_f, in_f)), bufs.new("db", (out_f,))
    with Env(env):                                   # (the workspace query reads the switches too)
        nws = int(lib.rpde_linear_ws_bytes(P, in_f, out_f))
        ws = bufs.new_bytes("ws", nws)
        _lib.check(lib.rpde_linear_fwd(X.ptr, W.data_ptr(), B.data_ptr(), y.ptr, P, in_f, out_f, _lib.stream_ptr()), "linear_fwd")
        _lib.check(lib.rpde_linear_bwd(X.ptr, W.data_ptr(), Gy.ptr, gx.ptr, gw.ptr, gb.ptr, P, in_f, out_f, ws.ptr, nws,
                                       _lib.stream_ptr()), "linear_bwd")
        torch.cuda.synchronize()
    bufs.check(["y", "dx", "dW", "db"], f"linear {prob['kind']} P={P} {out_f}x{in_f}")
    return {k: bufs.all[k].t.cpu().clone() for k in ("y", "dW", "db", "dx")}
