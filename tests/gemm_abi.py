"""A ctypes harness for rpde_gemm_f32 (include/rpde.h) that owns every buffer and drives the whole descriptor: padded
leading dimensions, two batch levels, interleaved and broadcast operands, misaligned bases, split-K slabs and every
epilogue field.  tests/test_gpu_gemm_descriptor.py runs it on the GPU, tests/test_gemm_abi_ref_cpu.py checks what those
tests rest on without one.  Nothing in this file needs a GPU.

Footprints.  For every operand the exact flat element offsets the descriptor addresses, computed from the strides and
leading dimensions alone (footprints()).  C's footprints of distinct (z, ks) must be disjoint and everything must fit
the allocation, or the case is refused.

Allocation.  Every operand lives in one ff_abi.Guarded allocation of base offset + footprint span floats.  An input
holds its values on the footprint and GUARD_WORD (a NaN) everywhere else, so a read of row padding or of a
neighbouring entry's gap shows as a NaN in the result.  An output is filled with GUARD_WORD, then its footprint gets
poison (bytes 0xFF) or the C0 values for accumulate in place.  After the call every word outside an output's
footprint must still be GUARD_WORD, every word inside finite, and every input bit-identical.

Oracle.  float64 on the CPU, gathering the operands from the flat buffers through those same footprints; the same
expression in float32 gives the condition on the inputs that tests/test_gemm_abi_ref_cpu.py asserts.  Two figures per
batch entry (split-K slabs summed in float64 first): relative L2, and the elementwise worst case in units of
2^-24 * (|alpha| |A| @ |B| + |bias| + |C0|), which any summation order keeps below K (the +16 of UNIT_MARGIN covers
the split-bf16 path's dropped third-order terms and the epilogue roundings).  With RPDE_EPI_MULAUX the magnitude of
the product part is multiplied by |aux|.  With an activation in prologue or epilogue only the relative L2 applies.

route() restates the host dispatch; it proves that the case table reaches every kernel variant and never computes an
expected value."""
from __future__ import annotations

import ctypes as C
import functools
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from tests import ff_abi as F
from tests.ff_abi import Guarded

GEMM_TOL, SPLIT_TOL, ACT_TOL = 2e-6, 4e-6, 1e-5      # tests/test_gpu_kernels.py
UNIT = 2.0 ** -24
UNIT_MARGIN = 16
MISS = 100.0
ACT_GELU, ACT_RELU, EPI_MULAUX = 1, 2, 100
OPERANDS = ("A", "B", "C", "aux", "bias", "acc_src", "aux_out", "colsum")
OUTPUTS = ("C", "aux_out", "colsum")


@dataclass(frozen=True)
class GemmCase:
    """one descriptor; None in a leading dimension or stride means the tight value (strides: with zdiv == 1 only)"""
    name: str
    family: str
    M: int
    N: int
    K: int
    a_k: int = 1
    b_k: int = 0
    lda: Optional[int] = None
    ldb: Optional[int] = None
    ldc: Optional[int] = None
    ldaux: Optional[int] = None
    batch: int = 1
    zdiv: int = 1
    sA1: Optional[int] = None
    sA2: int = 0
    sB1: Optional[int] = None
    sB2: int = 0
    sC1: Optional[int] = None
    sC2: int = 0
    ksplit: int = 1
    sCk: Optional[int] = None
    alpha: float = 1.0
    accumulate: bool = False
    bias_mode: int = 0
    act_a: int = 0
    act_b: int = 0
    epi_dact: int = 0
    write_act: int = 0
    aux_out: bool = False
    acc_src: bool = False
    colsum: bool = False
    a_split: bool = False
    b_split: bool = False
    off: Tuple[Tuple[str, int], ...] = ()         # (operand, base offset in floats, 0..3)
    data: Optional[str] = None                    # cases with the same key share their inputs (default: the name)

    # ---- resolved descriptor values ----------------------------------------------------------------------------------
    @property
    def has_aux(self) -> bool:
        return self.epi_dact != 0

    def ld(self, op: str) -> int:
        tight = {"A": self.K if self.a_k else self.M, "B": self.K if self.b_k else self.N, "C": self.N, "aux": self.N}[op]
        v = {"A": self.lda, "B": self.ldb, "C": self.ldc, "aux": self.ldaux}[op]
        return tight if v is None else v

    def strides(self, op: str) -> Tuple[int, int]:
        s1, s2 = {"A": (self.sA1, self.sA2), "B": (self.sB1, self.sB2), "C": (self.sC1, self.sC2)}[op]
        if s1 is None:
            assert self.zdiv == 1, (self.name, "two batch levels need explicit strides")
            slow = {"A": self.M if self.a_k else self.K, "B": self.N if self.b_k else self.K, "C": self.M}[op]
            s1 = slow * self.ld(op)
        return s1, s2

    @property
    def sck(self) -> int:
        if self.sCk is not None:
            return self.sCk
        s1, _ = self.strides("C")
        return self.batch * s1 if self.ksplit > 1 else 0

    def base_off(self, op: str) -> int:
        return dict(self.off).get(op, 0)

    @property
    def has_act(self) -> bool:
        return bool(self.act_a or self.act_b or self.write_act or self.epi_dact in (ACT_GELU, ACT_RELU))

    @property
    def tol(self) -> float:
        if self.has_act:
            return ACT_TOL
        if self.ksplit > 1 or (self.alpha != 1.0 and self.accumulate):
            return SPLIT_TOL
        return GEMM_TOL

    def present(self) -> List[str]:
        ops = ["A", "B", "C"]
        if self.has_aux:
            ops.append("aux")
        if self.bias_mode:
            ops.append("bias")
        for k in ("acc_src", "aux_out", "colsum"):
            if getattr(self, k):
                ops.append(k)
        return ops

    @property
    def two_level_or_interleaved(self) -> bool:
        if self.zdiv > 1:
            return True
        for op, slow in (("A", self.M if self.a_k else self.K), ("B", self.N if self.b_k else self.K), ("C", self.M)):
            s1, _ = self.strides(op)
            if self.batch > 1 and 0 < s1 < (slow - 1) * self.ld(op) + 1:
                return True
        return False


# ---------------------------------------------------------------------------------------------------------------------
# footprints: flat element offsets from strides and leading dimensions
# ---------------------------------------------------------------------------------------------------------------------
MISTAKES = ("swap_z", "sC2_for_sC1", "ldaux_for_ldc")


def _zoff(c: GemmCase, s1: int, s2: int, mistake: Optional[str]) -> np.ndarray:
    z = np.arange(c.batch, dtype=np.int64)
    z1, z2 = z // c.zdiv, z % c.zdiv
    if mistake == "swap_z":                          # A's and B's z read with the other level as the slow one
        n1 = max(1, c.batch // c.zdiv)
        z1, z2 = z % n1, z // n1
    return z1 * s1 + z2 * s2


def footprint(c: GemmCase, op: str, mistake: Optional[str] = None) -> np.ndarray:
    """offsets (relative to the operand's base pointer) in the operand's logical shape:
    A [batch, M, K], B [batch, K, N], C [batch, ksplit, M, N], aux / acc_src / aux_out [batch, M, N], bias [N] or [M],
    colsum [ceil(M / 128), N]"""
    i64 = np.int64
    if op == "A":
        s1, s2 = c.strides("A")
        m, k = np.arange(c.M, dtype=i64)[:, None], np.arange(c.K, dtype=i64)[None, :]
        inner = m * c.ld("A") + k if c.a_k else k * c.ld("A") + m
        return _zoff(c, s1, s2, mistake)[:, None, None] + inner[None]
    if op == "B":
        s1, s2 = c.strides("B")
        k, n = np.arange(c.K, dtype=i64)[:, None], np.arange(c.N, dtype=i64)[None, :]
        inner = n * c.ld("B") + k if c.b_k else k * c.ld("B") + n
        return _zoff(c, s1, s2, mistake)[:, None, None] + inner[None]
    if op in ("C", "aux", "acc_src", "aux_out"):
        s1, s2 = c.strides("C")
        if mistake == "sC2_for_sC1":
            s1 = s2
        ld = c.ld("aux") if op == "aux" else c.ld("C")
        if op == "aux" and mistake == "ldaux_for_ldc":
            ld = c.ld("C")
        m, n = np.arange(c.M, dtype=i64)[:, None], np.arange(c.N, dtype=i64)[None, :]
        per_z = _zoff(c, s1, s2, None)[:, None, None] + (m * ld + n)[None]      # (swap_z: the inputs' entries only)
        if op != "C":
            return per_z
        ks = np.arange(c.ksplit, dtype=i64) * c.sck
        return per_z[:, None] + ks[None, :, None, None]
    if op == "bias":
        return np.arange(c.N if c.bias_mode == 1 else c.M, dtype=i64)
    if op == "colsum":
        return np.arange(((c.M + 127) // 128) * c.N, dtype=i64).reshape(-1, c.N)
    raise KeyError(op)


@functools.lru_cache(maxsize=8)
def footprints(c: GemmCase) -> Dict[str, np.ndarray]:
    """the footprint of every operand the case has; refuses overlapping C entries and negative offsets"""
    fp = {op: footprint(c, op) for op in c.present()}
    for op, idx in fp.items():
        assert (idx.size or c.K == 0) and (not idx.size or int(idx.min()) >= 0), (c.name, op)
    for op in ("C", "aux_out"):
        if op in fp:
            flat = fp[op].ravel()
            assert np.unique(flat).size == flat.size, (c.name, op, "footprints of distinct (z, ks) overlap")
    return fp


def span(idx: np.ndarray) -> int:
    """floats from the base pointer to the last addressed element (K = 0: an operand nobody reads, four floats)"""
    return int(idx.max()) + 1 if idx.size else 4


# ---------------------------------------------------------------------------------------------------------------------
# inputs and the oracle
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def make_data(c: GemmCase) -> Dict[str, torch.Tensor]:
    """flat float32 CPU buffers of span floats for every input, plain randn; 'C0' (the old contents of C) for
    accumulate in place.  Only the values on the footprint are ever used."""
    fp = footprints(c)
    g = torch.Generator().manual_seed(zlib.crc32((c.data or c.name).encode()))
    data = {}
    for op in ("A", "B", "aux", "bias", "acc_src"):
        if op in fp:
            data[op] = torch.randn(span(fp[op]), generator=g)
    if c.accumulate and not c.acc_src:
        data["C0"] = torch.randn(span(fp["C"]), generator=g)
    return data


def _gelu(x):
    return torch.nn.functional.gelu(x)


def _dgelu(x):
    cdf = 0.5 * (1.0 + torch.erf(x * (0.5 ** 0.5)))
    pdf = torch.exp(-0.5 * x * x) * (1.0 / (2.0 * np.pi) ** 0.5)
    return cdf + x * pdf


def _act(kind, x):
    return {0: lambda v: v, ACT_GELU: _gelu, ACT_RELU: torch.relu}[kind](x)


def _dact(kind, x):
    return {ACT_GELU: _dgelu, ACT_RELU: lambda v: (v > 0).to(v.dtype)}[kind](x)


def _gather(flat: torch.Tensor, idx: np.ndarray, dtype) -> torch.Tensor:
    t = flat.to(dtype)
    i = torch.from_numpy(idx.ravel())
    if i.numel() and int(i.max()) >= t.numel():                        # (a mistaken footprint may leave the buffer)
        t = torch.cat([t, t.new_zeros(int(i.max()) + 1 - t.numel())])
    return t[i].reshape(idx.shape)


def evaluate(c: GemmCase, data: Dict[str, torch.Tensor], dtype=torch.float64, mistake: Optional[str] = None):
    """-> dict with 'C' [batch, M, N] (split-K: the sum of the slabs), 'mag' (the magnitude the elementwise bound is a
    multiple of; None with an activation), 'aux_out' where the case has it.  `mistake` plants one indexing error."""
    A = _gather(data["A"], footprint(c, "A", mistake), dtype)
    B = _gather(data["B"], footprint(c, "B", mistake), dtype)
    P = _act(c.act_a, A) @ _act(c.act_b, B)
    v = c.alpha * P
    mag = abs(c.alpha) * (A.abs() @ B.abs())
    if c.bias_mode:
        b = data["bias"].to(dtype)
        b = b[None, None, :] if c.bias_mode == 1 else b[None, :, None]
        v, mag = v + b, mag + b.abs()
    if c.has_aux:
        aux = _gather(data["aux"], footprint(c, "aux", mistake), dtype)
        if c.epi_dact == EPI_MULAUX:
            v, mag = v * aux, mag * aux.abs()
        else:
            v = v * _dact(c.epi_dact, aux)
    if c.accumulate:
        src = data["acc_src"] if c.acc_src else data["C0"]
        c0 = _gather(src, footprint(c, "acc_src", mistake), dtype)
        v, mag = v + c0, mag + c0.abs()
    out = {}
    if c.write_act:
        if c.aux_out:
            out["aux_out"] = _dact(c.write_act, v)
        v = _act(c.write_act, v)
    if mistake == "sC2_for_sC1":                         # the result lands where the mistaken C footprint says
        right = footprint(c, "C")[:, 0]
        wrong = footprint(c, "C", mistake)[:, 0]
        flat = v.new_zeros(max(span(right), span(wrong)))
        flat[torch.from_numpy(wrong.ravel())] = v.reshape(-1)
        v = flat[torch.from_numpy(right.ravel())].reshape(right.shape)
    out["C"] = v
    out["mag"] = None if c.has_act else mag
    return out


def colsum_ref(c: GemmCase, stored: torch.Tensor):
    """float64 column sums of the stored C [M, N] per 128-row tile, and the sums of |C| the bound is a multiple of"""
    tiles = (c.M + 127) // 128
    s = torch.stack([stored[128 * t:128 * t + 128].double().sum(0) for t in range(tiles)])
    a = torch.stack([stored[128 * t:128 * t + 128].double().abs().sum(0) for t in range(tiles)])
    return s, a


def figures(c: GemmCase, got: torch.Tensor, ref: torch.Tensor, mag: Optional[torch.Tensor]) -> Tuple[float, float]:
    """(worst relative L2 over the batch entries, worst elementwise error in units of 2^-24 * mag; 0 without mag)"""
    got, ref = got.double(), ref.double()
    d = got - ref
    rel = d.flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1).clamp_min(1e-300)
    units = 0.0
    if mag is not None:
        units = float((d.abs() / (UNIT * mag.double()).clamp_min(1e-300)).max())
    return float(rel.max()), units


def assert_figures(c: GemmCase, got: torch.Tensor, ref: torch.Tensor, mag, scale: float = 1.0, what: str = "C"):
    rel, units = figures(c, got, ref, mag)
    assert rel <= c.tol * scale, (c.name, what, "relative L2 of the worst batch entry", rel, c.tol * scale)
    assert units <= (c.K + UNIT_MARGIN) * scale, (c.name, what, "elementwise units of 2^-24", units, c.K + UNIT_MARGIN)
    return rel, units


# ---------------------------------------------------------------------------------------------------------------------
# the host dispatch, restated
# ---------------------------------------------------------------------------------------------------------------------
def route(c: GemmCase, split_mode: int = 2) -> Dict[str, object]:
    """Which kernel rpde_gemm_f32 launches for `c`, with every base 16-byte aligned but for c.off.  Restates
    csrc/gemm_f32.hip: kchunk (lines 22-24), pro (30), vec (34-38), tile choice and the small-problem fallback (40-53),
    tile counts, swz and the grid (54-62), cvec (65-74), the split-bf16 predicate and its images (83-101); and
    csrc/gemm_kernel.h launch_layout_impl (538-555): scalar 64x64, the PREAUX / single-stage / pipelined 128x128
    kernels, the pipelined 128x64, 64x128 and 64x64 tiles and the plain double-buffered 128x32 and 32x128 ones.
    Used to prove that the case table reaches every route, never to compute an expected value."""
    al = lambda op: c.base_off(op) % 4 == 0
    kchunk = (c.K + c.ksplit - 1) // c.ksplit
    kchunk = (kchunk + 31) // 32 * 32 or 32
    pro = 1 if c.act_a else (2 if c.act_b else 0)
    sA1, sA2 = c.strides("A")
    sB1, sB2 = c.strides("B")
    sC1, sC2 = c.strides("C")
    lda, ldb, ldc = c.ld("A"), c.ld("B"), c.ld("C")
    vec = (al("A") and al("B") and lda % 4 == 0 and ldb % 4 == 0 and all(s % 4 == 0 for s in (sA1, sA2, sB1, sB2))
           and (c.K if c.a_k else c.M) % 4 == 0 and (c.K if c.b_k else c.N) % 4 == 0)
    bm, bn = 64, 64
    if vec:
        tm = 32 if c.M <= 32 else (64 if c.M <= 64 else 128)
        tn = 32 if c.N <= 32 else (64 if c.N <= 64 else 128)
        if tm == 32:
            bm, bn = 32, 128
        elif tn == 32:
            bm, bn = 128, 32
        else:
            bm, bn = tm, tn
        if bm == 128 and bn == 128 and not c.colsum and \
                ((c.M + 127) // 128) * ((c.N + 127) // 128) * c.batch * c.ksplit < 384:
            bm, bn = 64, 64
    mtiles, ntiles = (c.M + bm - 1) // bm, (c.N + bn - 1) // bn
    swz = 1 if (ntiles > 1 and mtiles >= 64) else 0
    zt = c.batch * c.ksplit
    gy = min(zt, 32768)
    gz = (zt + gy - 1) // gy
    tiles = mtiles * ntiles
    if not swz and 1 < tiles <= 16 and gz == 1 and zt % 8 == 0:
        swz = 2
    gx = (mtiles + 7) // 8 * 8 * ntiles if swz == 1 else tiles
    cvec = (vec and al("C") and ldc % 4 == 0 and sC1 % 4 == 0 and sC2 % 4 == 0 and c.sck % 4 == 0 and c.N % 4 == 0
            and (not c.has_aux or (al("aux") and c.ld("aux") % 4 == 0)) and (c.bias_mode != 1 or al("bias")))
    if c.accumulate and c.acc_src:
        cvec = cvec and al("acc_src")
    if c.aux_out:
        cvec = cvec and al("aux_out")
    r = dict(vec=vec, cvec=cvec, tile=(bm, bn), swz=swz, grid=(gx, gy, gz), pro=pro, kchunk=kchunk,
             layout=("n" if c.a_k else "t") + ("t" if c.b_k else "n"), img=None)
    bimg = c.b_split and c.a_k and sB1 == 0 and sB2 == 0 and kchunk % 32 == 0 and c.K % 32 == 0
    aimg = (not bimg) and c.a_split and sA1 == 0 and sA2 == 0 and (c.K % 32 == 0 or (not c.b_k and c.ksplit == 1))
    k_ok = c.K >= 32 and c.K % 32 == 0
    if split_mode and vec and cvec and pro == 0 and (k_ok or (aimg and c.K >= 1)) and \
            ((((c.a_k or aimg) and (c.b_k or bimg)) or split_mode >= 2)) and bm in (64, 128) and bn in (64, 128):
        r.update(kernel="bf16x3", variant="x3", img="b" if bimg else ("a" if aimg else None))
        return r
    r["kernel"] = "native"
    if not vec:
        r["variant"] = "double"
    elif (bm, bn) == (128, 128):
        preaux = cvec and pro == 0 and not c.write_act and ((c.epi_dact == EPI_MULAUX) != bool(c.accumulate))
        r["variant"] = ("preaux" if preaux else "single") if kchunk <= 64 else "pipe"
    elif (bm, bn) in ((128, 64), (64, 128), (64, 64)):
        r["variant"] = "pipe"
    else:
        r["variant"] = "double"
    return r


# ---------------------------------------------------------------------------------------------------------------------
# guarded allocations and the call
# ---------------------------------------------------------------------------------------------------------------------
class Slot:
    """one operand: a Guarded allocation of base offset + span floats, GUARD_WORD everywhere but on the footprint"""

    def __init__(self, name: str, idx: np.ndarray, off: int, device, values: Optional[torch.Tensor], is_output: bool):
        self.name, self.off, self.is_output = name, off, is_output
        self.shape = idx.shape
        self.n = off + span(idx)
        assert 0 <= off < 4 and (not idx.size or (int(idx.min()) >= 0 and off + int(idx.max()) < self.n)), name
        self.g = Guarded(name, (self.n,), device)
        assert self.g.ptr % 16 == 0, name
        self.words = self.g.raw[F._G:F._G + self.n]                       # int32 view of the allocation
        self.words.fill_(F._GUARD_I32)
        self.idx = torch.from_numpy(idx.ravel()).to(device) + off
        if values is not None:
            self.g.t[self.idx] = values.to(device)[self.idx - off]
        else:
            self.words[self.idx] = -1                                     # bytes 0xFF
        self.inside = torch.zeros(self.n, dtype=torch.bool, device=device)
        self.inside[self.idx] = True
        self.before = self.g.raw.clone() if not is_output else None

    @property
    def ptr(self) -> int:
        return self.g.ptr + 4 * self.off

    def read(self) -> torch.Tensor:
        return self.g.t[self.idx].reshape(self.shape).cpu()

    def problems(self) -> List[str]:
        bad = list(self.g.broken_guards())
        if self.is_output:
            stray = torch.nonzero((self.words != F._GUARD_I32) & ~self.inside).flatten()
            if stray.numel():
                bad.append(f"{self.name}: {stray.numel()} words outside the footprint changed, first at element "
                           f"{int(stray[0]) - self.off} of the operand")
            left = torch.nonzero(~torch.isfinite(self.g.t[self.idx])).flatten()
            if left.numel():
                bad.append(f"{self.name}: {left.numel()} footprint elements not finite (poison left or NaN computed), "
                           f"first at footprint position {int(left[0])}")
        elif not torch.equal(self.g.raw, self.before):
            bad.append(f"{self.name}: an input changed")
        return bad


def allocate(c: GemmCase, data: Dict[str, torch.Tensor], device) -> Dict[str, Slot]:
    fp = footprints(c)
    slots = {}
    for op, idx in fp.items():
        values = data.get(op)
        if op == "C" and c.accumulate and not c.acc_src:
            values = data["C0"]
        slots[op] = Slot(op, idx, c.base_off(op), device, values, op in OUTPUTS)
    return slots


def check_slots(c: GemmCase, slots: Dict[str, Slot]) -> None:
    bad: List[str] = []
    for s in slots.values():
        bad += s.problems()
    assert not bad, (c.name, bad)


def descriptor(c: GemmCase, ptrs: Dict[str, Optional[int]]):
    from rpde import _lib
    d = _lib.GemmDesc()
    d.A, d.B, d.C = ptrs["A"], ptrs["B"], ptrs["C"]
    d.M, d.N, d.K, d.a_kmajor, d.b_kmajor = c.M, c.N, c.K, int(c.a_k), int(c.b_k)
    d.lda, d.ldb, d.ldc = c.ld("A"), c.ld("B"), c.ld("C")
    d.batch, d.zdiv = c.batch, c.zdiv
    (d.sA1, d.sA2), (d.sB1, d.sB2), (d.sC1, d.sC2) = c.strides("A"), c.strides("B"), c.strides("C")
    d.ksplit, d.sCk = c.ksplit, c.sck
    d.alpha, d.accumulate = c.alpha, int(c.accumulate)
    d.bias, d.bias_mode = ptrs.get("bias"), c.bias_mode
    d.act_a, d.act_b, d.epi_dact, d.write_act = c.act_a, c.act_b, c.epi_dact, c.write_act
    d.aux, d.ldaux = ptrs.get("aux"), c.ld("aux")
    for k in ("colsum", "aux_out", "acc_src", "a_split", "b_split"):
        setattr(d, k, ptrs.get(k))
    return d


def run_case(c: GemmCase, device) -> Dict[str, torch.Tensor]:
    """the case through rpde_gemm_f32 in guarded, poisoned buffers; guards, poison and inputs checked.
    -> CPU copies: 'C' [batch, ksplit, M, N], 'aux_out' [batch, M, N], 'colsum' [tiles, N]"""
    from rpde import _lib
    lib = _lib.load()
    data = make_data(c)
    slots = allocate(c, data, device)
    ptrs: Dict[str, Optional[int]] = {op: s.ptr for op, s in slots.items()}
    images = []
    for key, op, rows, kmajor in (("a_split", "A", c.M, c.a_k), ("b_split", "B", c.N, c.b_k)):
        if getattr(c, key):
            img = Guarded.of_bytes(key, int(lib.rpde_split_weights_bytes(rows, c.K)), device)
            _lib.check(lib.rpde_split_weights(slots[op].ptr, int(kmajor), c.ld(op), rows, c.K, img.ptr, _lib.stream_ptr()),
                       "split_weights")
            images.append(img)
            ptrs[key] = img.ptr
    d = descriptor(c, ptrs)
    _lib.check(lib.rpde_gemm_f32(C.byref(d), _lib.stream_ptr()), "gemm " + c.name)
    torch.cuda.synchronize()
    check_slots(c, slots)
    for img in images:
        assert not img.broken_guards(), (c.name, img.broken_guards())
    return {op: slots[op].read() for op in OUTPUTS if op in slots}


def check_result(c: GemmCase, got: Dict[str, torch.Tensor], split_mode: int = 2) -> Dict[str, float]:
    """both figures of C (and of aux_out), the slabs past K exactly zero, K = 0 exact, the column sums"""
    data = make_data(c)
    ref = evaluate(c, data)
    slabs = got["C"]
    if c.ksplit > 1:
        kchunk = route(c, split_mode)["kchunk"]
        for ks in range(c.ksplit):
            if ks * kchunk >= c.K:
                assert not slabs[:, ks].any(), (c.name, "slab past K is not exactly zero", ks)
    gotC = slabs.double().sum(1)
    rel, units = assert_figures(c, gotC, ref["C"], ref["mag"])
    figs = {"rel": rel, "units_over_K16": units / (c.K + UNIT_MARGIN)}
    if c.K == 0:
        exact = evaluate(c, data, torch.float32)["C"]
        assert torch.equal(gotC.float(), exact), (c.name, "K = 0 must store bias + accumulate exactly")
    if c.aux_out:
        r2, _ = assert_figures(c, got["aux_out"], ref["aux_out"], None, what="aux_out")
        figs["rel"] = max(rel, r2)
    if c.colsum:
        assert c.batch == 1
        s, a = colsum_ref(c, got["C"][0, 0])
        units_cs = float(((got["colsum"].double() - s).abs() / (UNIT * a).clamp_min(1e-300)).max())
        assert units_cs <= 128 + UNIT_MARGIN, (c.name, "column sums, units of 2^-24 * sum |C|", units_cs)
        figs["colsum_units_over_144"] = units_cs / (128 + UNIT_MARGIN)
    return figs


# ---------------------------------------------------------------------------------------------------------------------
# the case table of tests/test_gpu_gemm_descriptor.py
# ---------------------------------------------------------------------------------------------------------------------
LAYOUTS = [(1, 1), (1, 0), (0, 0), (0, 1)]
_LNAME = {(1, 1): "nt", (1, 0): "nn", (0, 0): "tn", (0, 1): "tt"}


def _padded(name, family, M, N, K, a_k, b_k, pad, **kw) -> GemmCase:
    """every leading dimension = extent + pad, ldaux = ldc + 4"""
    return GemmCase(name, family, M, N, K, a_k, b_k, lda=(K if a_k else M) + pad, ldb=(K if b_k else N) + pad,
                    ldc=N + pad, ldaux=N + pad + 4, **kw)


def _cases() -> List[GemmCase]:
    cs: List[GemmCase] = []
    # 1. padded leading dimensions: +4 stays on the vector route, +1 forces the scalar kernels
    for (a_k, b_k) in LAYOUTS:
        for (M, N, K) in [(72, 40, 64), (130, 68, 96), (33, 17, 5)]:
            for pad in (4, 1):
                n = f"pad{pad}-{_LNAME[a_k, b_k]}-{M}x{N}x{K}"
                cs.append(_padded(n, "padded", M, N, K, a_k, b_k, pad))
                cs.append(_padded(n + "-mulaux", "padded", M, N, K, a_k, b_k, pad, epi_dact=EPI_MULAUX))
    # 2. one operand 4 bytes off a 16-byte boundary (the aligned twin is the same case with off = ())
    p1 = dict(M=72, N=40, K=64, a_k=1, b_k=0, bias_mode=1, epi_dact=EPI_MULAUX, accumulate=True, acc_src=True)
    p2 = dict(M=72, N=40, K=64, a_k=1, b_k=0, bias_mode=1, write_act=ACT_GELU, aux_out=True)
    cs.append(GemmCase("mis-none", "misaligned", data="mis", **p1))
    for op in ("A", "B", "C", "aux", "bias", "acc_src"):
        cs.append(GemmCase(f"mis-{op}", "misaligned", off=((op, 1),), data="mis", **p1))
    cs.append(GemmCase("mis2-none", "misaligned", data="mis2", **p2))
    cs.append(GemmCase("mis2-aux_out", "misaligned", off=(("aux_out", 1),), data="mis2", **p2))
    # 3. two batch levels and shared operands.  Field [Bt, Mx, Ny, Cc] = [2, 6, 10, 8], lines along x
    Bt, Mx, Ny, Cc = 2, 6, 10, 8
    line = dict(batch=Bt * Ny, zdiv=Ny)
    cs.append(GemmCase("xlines-as-B", "batch-levels", 8, Cc, Mx, 0, 0, lda=8, ldb=Ny * Cc, sA1=0, sA2=0,
                       sB1=Mx * Ny * Cc, sB2=Cc, sC1=Ny * 8 * Cc, sC2=8 * Cc, **line))
    cs.append(GemmCase("xlines-as-C", "batch-levels", Mx, Cc, 8, 1, 0, ldc=Ny * Cc, sA1=0, sA2=0, sB1=Ny * 8 * Cc,
                       sB2=8 * Cc, sC1=Mx * Ny * Cc, sC2=Cc, **line))
    cs.append(GemmCase("xlines-as-C-mulaux", "batch-levels", Mx, Cc, 8, 1, 0, ldc=Ny * Cc, ldaux=Ny * Cc + 4, sA1=0,
                       sA2=0, sB1=Ny * 8 * Cc, sB2=8 * Cc, sC1=Mx * Ny * Cc, sC2=Cc, epi_dact=EPI_MULAUX, **line))
    bro = dict(M=72, N=40, K=64, a_k=1, b_k=0, batch=8, sA1=0, sA2=0, data="broadcast-A")
    cs.append(GemmCase("broadcast-A", "batch-levels", **bro))
    cs.append(GemmCase("broadcast-A-split", "batch-levels", a_split=True, **bro))
    cs.append(GemmCase("broadcast-A-split-ktail", "batch-levels", 72, 40, 44, 1, 0, batch=8, sA1=0, sA2=0, a_split=True))
    cs.append(GemmCase("broadcast-B-split", "batch-levels", 72, 40, 64, 1, 1, batch=8, sB1=0, sB2=0, b_split=True))
    Cm, kp = 18, 4                                      # the per-mode channel mix: entries inside each other's rows
    mix = dict(M=40, N=2 * Cm, K=2 * Cm, a_k=1, b_k=0, lda=2 * kp * Cm, ldc=2 * kp * Cm, batch=kp, sA1=2 * Cm,
               sC1=2 * Cm)
    cs.append(GemmCase("mode-mix", "batch-levels", ldaux=4 * kp * Cm, epi_dact=EPI_MULAUX, **mix))
    # (the same addresses without an epilogue, spelled with two batch levels)
    cs.append(GemmCase("mode-mix-two-level", "batch-levels", **dict(mix, zdiv=2, sA1=4 * Cm, sA2=2 * Cm, sC1=4 * Cm,
                                                                     sC2=2 * Cm, sB1=2 * 4 * Cm * Cm, sB2=4 * Cm * Cm)))
    keff = 4                                            # its weight gradient: x-major by x-major, slabs of all modes
    cs.append(GemmCase("mode-mix-wgrad", "batch-levels", 2 * Cm, 2 * Cm, 128, 0, 0, lda=2 * kp * Cm, ldb=2 * kp * Cm,
                       batch=keff, zdiv=2, sA1=4 * Cm, sA2=2 * Cm, sB1=4 * Cm, sB2=2 * Cm, sC1=8 * Cm * Cm,
                       sC2=4 * Cm * Cm, ksplit=4, sCk=keff * 4 * Cm * Cm))
    # 4. accumulate, in place and from acc_src
    for src in (False, True):
        s = "-src" if src else "-inplace"
        cs.append(GemmCase("acc-vec" + s, "accumulate", 72, 40, 40, 1, 0, batch=3, accumulate=True, acc_src=src, alpha=0.5))
        cs.append(GemmCase("acc-scalar" + s, "accumulate", 33, 17, 5, 1, 0, batch=3, accumulate=True, acc_src=src))
        cs.append(GemmCase("acc-x3" + s, "accumulate", 72, 40, 64, 1, 1, batch=3, accumulate=True, acc_src=src))
        for M in (256, 200):
            cs.append(GemmCase(f"acc-preaux-{M}" + s, "accumulate", M, 132, 64, 1, 0, batch=96, accumulate=True,
                               acc_src=src))
    for M in (256, 200):
        cs.append(GemmCase(f"mulaux-preaux-{M}", "accumulate", M, 132, 64, 1, 0, batch=96, epi_dact=EPI_MULAUX))
    # (K = 40 keeps the split-bf16 kernel away, so the default dispatch reaches PREAUX and the single-stage kernel too)
    cs.append(GemmCase("acc-preaux-200-k40", "accumulate", 200, 132, 40, 1, 0, batch=96, accumulate=True, ldc=136))
    cs.append(GemmCase("single-stage-200-k40", "accumulate", 200, 132, 40, 1, 0, batch=96, bias_mode=1))
    cs.append(GemmCase("pipe-128-200-k96", "accumulate", 200, 132, 96, 0, 1, batch=96, accumulate=True, acc_src=True))
    # 5. split-K into poisoned slabs
    cs.append(GemmCase("splitk-dead-vec", "split-k", 72, 40, 64, 1, 1, ksplit=8))
    cs.append(GemmCase("splitk-dead-scalar", "split-k", 33, 17, 64, 1, 1, ksplit=8))
    cs.append(GemmCase("splitk-tail-vec", "split-k", 72, 40, 4097, 0, 0, ksplit=16))
    cs.append(GemmCase("splitk-tail-scalar", "split-k", 64, 3, 4097, 0, 0, ksplit=16, batch=2))
    cs.append(GemmCase("splitk-gap", "split-k", 72, 40, 128, 1, 0, ksplit=4, batch=2, sCk=2 * 72 * 40 + 64))
    cs.append(GemmCase("splitk-swz2", "split-k", 132, 68, 128, 0, 0, ksplit=4, batch=2))
    cs.append(GemmCase("splitk-swz2-plus1", "split-k", 132, 68, 128, 0, 0, ksplit=4, batch=3))
    # 6. grid edges
    cs.append(GemmCase("grid-z2", "grid", 8, 8, 8, 1, 0, batch=32768 + 5))
    cs.append(GemmCase("grid-xcd-vec", "grid", 4228, 72, 32, 1, 1))
    cs.append(GemmCase("grid-xcd-scalar", "grid", 4293, 70, 8, 1, 0))
    # 7. batched epilogues: aux and aux_out follow C's batch offsets
    for tag, (M, N, K) in (("vec", (72, 40, 64)), ("scalar", (33, 17, 5))):
        b3 = dict(M=M, N=N, K=K, a_k=1, b_k=0, batch=3)
        cs.append(GemmCase(f"epi-{tag}-bias1", "epilogue", bias_mode=1, **b3))
        cs.append(GemmCase(f"epi-{tag}-bias2", "epilogue", bias_mode=2, alpha=-2.0, **b3))
        cs.append(GemmCase(f"epi-{tag}-dgelu", "epilogue", epi_dact=ACT_GELU, **b3))
        cs.append(GemmCase(f"epi-{tag}-drelu", "epilogue", epi_dact=ACT_RELU, bias_mode=2, **b3))
        cs.append(GemmCase(f"epi-{tag}-mulaux", "epilogue", epi_dact=EPI_MULAUX, ldaux=N + 4, **b3))
        cs.append(GemmCase(f"epi-{tag}-act-auxout", "epilogue", write_act=ACT_GELU, aux_out=True, bias_mode=1, **b3))
        cs.append(GemmCase(f"epi-{tag}-relu", "epilogue", write_act=ACT_RELU, **b3))
    cs.append(GemmCase("colsum-200x36", "epilogue", 200, 36, 64, 1, 1, colsum=True, bias_mode=1))
    cs.append(GemmCase("colsum-129x132", "epilogue", 129, 132, 64, 1, 1, colsum=True, bias_mode=1, write_act=ACT_GELU,
                       aux_out=True))
    cs.append(GemmCase("colsum-129x132-k40", "epilogue", 129, 132, 40, 1, 1, colsum=True))
    cs.append(GemmCase("pro-act-a", "epilogue", 72, 40, 64, 1, 1, act_a=ACT_GELU, lda=68))
    cs.append(GemmCase("pro-act-b", "epilogue", 72, 40, 64, 1, 0, act_b=ACT_RELU, ldb=44, batch=2))
    # 8. short reductions
    for K in (0, 1, 31, 32, 33):
        cs.append(GemmCase(f"shortk-vec-{K}", "short-k", 72, 40, K, 0, 0, bias_mode=1, accumulate=True))
        cs.append(GemmCase(f"shortk-scalar-{K}", "short-k", 33, 17, K, 0, 0, bias_mode=2, accumulate=True, acc_src=True))
    # the remaining vector tiles of the native kernels
    cs.append(GemmCase("tile-128x64", "padded", 132, 64, 96, 1, 1, ldc=68))
    cs.append(GemmCase("tile-64x128", "padded", 64, 132, 96, 1, 0, ldb=136))
    cs.append(GemmCase("tile-128x32", "padded", 132, 32, 64, 0, 1, lda=136))
    cs.append(GemmCase("tile-32x128", "padded", 32, 132, 64, 0, 0, ldb=136))
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    return cs


CASES: List[GemmCase] = _cases()
BY_NAME: Dict[str, GemmCase] = {c.name: c for c in CASES}
FAMILIES = sorted({c.family for c in CASES})


def aligned_twin(c: GemmCase) -> GemmCase:
    return BY_NAME["mis2-none" if c.name.startswith("mis2") else "mis-none"]


def applicable_mistakes(c: GemmCase) -> List[str]:
    m = []
    if c.zdiv > 1 and c.batch // c.zdiv > 1:
        m.append("swap_z")
    if c.zdiv > 1 and c.strides("C")[0] != c.strides("C")[1]:
        m.append("sC2_for_sC1")
    if c.has_aux and c.ld("aux") != c.ld("C"):
        m.append("ldaux_for_ldc")
    return m
