"""Case tables, launch geometry, inputs, float64 oracle, float32 floor and planted faults for the kernels that only the
evaluation forward of the channels-first FNO2d reaches:
    k_conv_syn_h2<ACT, FULL, LIFT>      csrc/conv_syn_h2.hip    rpde_fnoblock2d_eval_fwd, rpde_fno2d_lift_block_eval_fwd
    k_conv_syn_proj_h2<MT, CO, ACT>     csrc/conv_proj_h2.hip   rpde_fnoblock2d_proj_eval_fwd
    k_conv_mlp_h2<KS, MT, CO>           csrc/conv_mlp.hip       rpde_conv_mlp_fwd
    k_conv1x1_small<CO, true>           csrc/conv_small.hip     rpde_fnoblock2d_eval_fwd where the h2 tail is not eligible
Test infrastructure only: plain torch-CPU, the product tree does not import it.  tests/test_eval_cf_ref_cpu.py checks this
file without a device, tests/test_gpu_eval_cf.py runs the kernels on it.

Pass arithmetic (restated from the host code, checked against the library's *_ok queries on the CPU).  The three h2
kernels are persistent: a workgroup takes a UNIT of work per pass and strides by the grid,
    kernel   unit U                              grid                      one full pass T
    syn      512 / N rows (b, m)                 min(ceil(B M / U), CUs)   U CUs rows
    lift     the same kernel, LIFT = true
    proj     8 rows (one per wave)               min(ceil(B M / 8), CUs)   8 CUs rows
    mlp      4 tiles of 16 points (one a wave)   min(ceil(tiles / 4), 8 CUs)  32 CUs tiles
and each keeps something in flight from one pass into the next (LDS-DMA of the next row under a counted wait, the next
row's first 64 points, the next tile, a store deferred into the next group).  The multiply-add tail k_conv1x1_small
launches one workgroup per 1024 points and has no pass loop: its cases go by shape and padding only.

Row counts are symbolic (SYMS) and resolved from the device's CU count, as tests/ff_abi.py resolves T-1 / T / T+1:
1, U-1, U+1 (partial first pass, idle waves), T-1, T, T+1 (one workgroup with a second pass whose other waves idle) and
"3pass" = 2T + T/2 + 3 (workgroups with three passes beside workgroups with two: the steady state holds a previous
store and a next prefetch together).  split_rows turns a row count into (B, M) with B > 1 and M no multiple of U where
the count has such a divisor, so that a pass and a wave's consecutive rows straddle samples.

Operands.  x, u: randn; spectral weights complex randn of BOTH signs, scaled so that the spectral branch and the bypass
convolution contribute alike to a line; "scaled": sample b times 10^(-2 + 4 b / (B - 1)) (every operation here is per
sample: a scale that leaks between samples sharing a pass shows in the small samples' lines, which are normalised per
sample); "zero": sample 1 is exactly zero -- every (b, o) plane of it must be one bit-identical constant.

Oracle.  spectral_cf_ref.run_oracle("block", ..)'s expression (oracle.reference_path.spectral_conv2d + the 1x1
convolution) without its backward, the lifting cat(u, gx, gy) -> Conv1x1 in front for LIFT, the activation and the two
1x1 layers of the projection on top; `real` selects float64 (the reference) or float32 (the floor: the same expression
in float32 on the CPU, whose error against float64 every per-line bound is FLOOR_FACTOR times)."""
from __future__ import annotations

import functools
import math
import zlib
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import reference_path as R
from tests import spectral_cf_ref as S

TOL = 2e-6                      # the whole-tensor bound of the older tests of these kernels (tests/test_gpu_kernels.py)
FAULT_MARGIN = 100.0            # a planted fault must stand this many times above the per-line bound
CU_COUNTS = (64, 256, 304)      # the tables are checked for these; 256: MI355X
ACTS = S.ACTS
MAX_CASE_BYTES = 64 << 20


@dataclass(frozen=True)
class Case:
    kernel: str                 # "syn" | "lift" | "proj" | "mlp" | "fma"
    name: str
    rows: object                # a key of SYMS, or (B, M) -- mlp: M = tiles of 16 points per sample
    N: int = 16                 # points of a row (mlp: of a tile)
    Cin: int = 32
    Cout: int = 32              # the block's width (syn / lift / proj / fma); mlp: the output channels
    m1: int = 4
    m2: int = 12
    act: str = "gelu"           # act_out of the block; mlp: act_in
    Cmid: int = 0               # hidden width of the projection (proj, mlp)
    Cq: int = 0                 # its outputs (proj)
    content: str = "randn"      # "randn" | "scaled" | "zero"
    null: Tuple[str, ...] = ()  # biases passed as NULL
    grid: str = "unit"          # lift: linspace(0, 1) coordinates, or "user": any values


Shape = Dict[str, int]

SYMS = {"1": lambda T, U: 1, "U-1": lambda T, U: U - 1, "U+1": lambda T, U: U + 1, "T-1": lambda T, U: T - 1,
        "T": lambda T, U: T, "T+1": lambda T, U: T + 1, "3pass": lambda T, U: 2 * T + T // 2 + 3}
BOUNDARY = ("T-1", "T", "T+1", "3pass")


# ---------------------------------------------------------------------------------------------------------------------
# geometry: the host code of the four files, restated
# ---------------------------------------------------------------------------------------------------------------------
def r4(v: int) -> int:
    return (v + 3) // 4 * 4


def unit(case: Case) -> Optional[int]:
    """rows (mlp: tiles) a workgroup takes per pass; None: no pass loop"""
    return {"syn": 512 // case.N, "lift": 512 // case.N, "proj": 8, "mlp": 4, "fma": None}[case.kernel]


def clamp(case: Case, cus: int) -> int:
    return 8 * cus if case.kernel == "mlp" else cus


def full_pass(case: Case, cus: int) -> int:
    return unit(case) * clamp(case, cus)


def col_stage_ok(M: int, m1: int, kp: int) -> bool:
    return 4 <= kp <= 16 and kp % 4 == 0 and 2 * M * kp * 4 <= 65536 and m1 >= 1


def fma_lds(Cin, Cout, N, R2) -> int:
    CO = fma_co(Cout)
    rows = 1 if N >= 1024 else 1024 // N
    return 4 * (Cin * CO + rows * R2 * CO)


def fma_co(Cout: int) -> int:
    return 4 if Cout <= 4 else 8 if Cout <= 8 else 16 if Cout <= 16 else 32


def fma_ok(Cin, Cout, M, N, R2) -> bool:
    """conv1x1_syn_ok: what rpde_fnoblock2d_eval_ok answers (the h2 tail is chosen among these shapes)"""
    return (1 <= Cout <= 32 and 1 <= Cin <= 512 and (M * N) % 4 == 0 and N % 4 == 0 and (1024 % N == 0 or N % 1024 == 0)
            and fma_lds(Cin, Cout, N, R2) <= 65536)


def h2_ok(Cin, Cout, M, N, R2) -> bool:
    """conv_syn_h2_ok"""
    return N in (64, 128, 256, 512) and 1 <= M < (1 << 20) and Cin == 32 and 1 <= Cout <= 32 and 8 <= R2 <= 32 and R2 % 8 == 0


def proj_ok(Cin, Cout, M, N, m1, m2, Cmid, Cq) -> bool:
    R2 = 2 * r4(m2)
    return (m2 <= N // 2 + 1 and m1 <= M and Cin == 32 and 1 <= Cout <= 32 and 1 <= Cmid <= 128 and 1 <= Cq <= 4 and
            N % 64 == 0 and 64 <= N <= 1024 and 8 <= R2 <= 32 and R2 % 8 == 0 and M >= 1)


def lift_ok(C, Cout, M, N, m1, m2) -> bool:
    kp = r4(m2)
    return M <= 1024 and m2 <= N // 2 + 1 and m1 <= M and h2_ok(C, Cout, M, N, 2 * kp) and col_stage_ok(M, m1, kp)


def mlp_ok(Cin, Cmid, Cout, S_) -> bool:
    if not 1 <= Cout <= 4 or S_ % 16 or Cmid < 1:
        return False
    return (Cin == 32 and Cmid <= 128) or (Cin == 64 and Cmid <= 64)


def _mt(Cmid: int) -> int:
    mt = (Cmid + 15) // 16
    return 2 if mt <= 2 else 4 if mt <= 4 else 8


def proj_lds(N: int, Cmid: int) -> int:
    mt = _mt(Cmid)
    return (N // 16) * 2048 + mt * 2048 + 4 * 16 * mt * 5


def tail_of(case: Case, sh: Shape, h2_switch: bool = True) -> str:
    """which synthesis tail rpde_fnoblock2d_eval_fwd launches for a syn / fma case: "h2" | "fma" """
    R2 = 2 * r4(sh["m2"])
    assert fma_ok(case.Cin, case.Cout, sh["M"], case.N, R2), case
    return "h2" if h2_switch and h2_ok(case.Cin, case.Cout, sh["M"], case.N, R2) else "fma"


def instance(case: Case, sh: Shape, h2_switch: bool = True) -> Tuple:
    """the template instance the host code picks (h2_switch False: under RPDE_CONV_SYN_H2=0)"""
    k = case.kernel
    if k == "syn" and tail_of(case, sh, h2_switch) == "fma":
        k = "fma"
    if k in ("syn", "lift"):
        return ("k_conv_syn_h2", case.act, case.Cout == 32, k == "lift")
    if k == "proj":
        return ("k_conv_syn_proj_h2", _mt(case.Cmid), 1 if case.Cq == 1 else 4, case.act)
    if k == "mlp":
        mt = (case.Cmid + 15) // 16
        mt = (2 if mt <= 2 else 4 if mt <= 4 else 8) if case.Cin == 32 else (2 if mt <= 2 else 4)
        return ("k_conv_mlp_h2", case.Cin // 32, mt, 1 if case.Cout == 1 else 2 if case.Cout == 2 else 4)
    return ("k_conv1x1_small", fma_co(case.Cout), True)


def passes(case: Case, sh: Shape, cus: int) -> Tuple[int, int, int]:
    """-> (workgroups, fewest, most passes of a workgroup)"""
    U = unit(case)
    groups = -(-sh["rows"] // U)
    grid = min(groups, clamp(case, cus))
    return grid, groups // grid, -(-groups // grid)


def split_rows(rows: int, U: int, max_M: int) -> Tuple[int, int]:
    """(B, M) with B M = rows: the smallest B in 2..64 whose M fits and is no multiple of U, else any B that fits, else
    one sample"""
    fits = [b for b in range(2, 65) if rows % b == 0 and rows // b <= max_M]
    odd = [b for b in fits if (rows // b) % U]
    if odd or fits:
        b = (odd or fits)[0]
        return b, rows // b
    assert rows <= max_M, (rows, max_M)
    return 1, rows


def resolve(case: Case, cus: int) -> Shape:
    """the case's sizes on a device of `cus` compute units"""
    kp = r4(case.m2)
    max_M = min(1024, 8192 // kp) if case.kernel == "lift" else 1 << 19
    if isinstance(case.rows, str):
        U = unit(case)
        rows = SYMS[case.rows](full_pass(case, cus), U)
        assert rows >= 1, case
        B, M = split_rows(rows, U, max_M) if case.rows in BOUNDARY else (1, rows)
    else:
        B, M = case.rows
    sh = dict(B=B, M=M, rows=B * M, N=case.N, m1=min(case.m1, M), m2=case.m2, S=M * case.N)
    return sh


def tensor_bytes(case: Case, sh: Shape) -> int:
    """the largest device tensor of the case"""
    pts = sh["B"] * sh["S"]
    cin = 1 if case.kernel == "lift" else case.Cin
    cout = case.Cq if case.kernel == "proj" else case.Cout
    return 4 * pts * max(cin, cout)


# ---------------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------------
def _c(kernel, name, rows, **kw):
    return Case(kernel, name, rows, **kw)


# k_conv_syn_h2 through rpde_fnoblock2d_eval_fwd.  Cout = 32 is FULL (the counted wait), the others drain; R2 = 2 r4(m2)
# in {8, 16, 24, 32}.  (N = 64 with Cout > 16 stops at R2 = 24: rpde_fnoblock2d_eval_ok also wants the multiply-add
# tail's LDS to fit, and 16 rows x 32 entries x 32 channels do not.)
SYN_CASES = [
    _c("syn", "s-1", "1", N=64, Cout=32, m1=1, m2=3, act="gelu"),
    _c("syn", "s-U-1", "U-1", N=64, Cout=31, m1=2, m2=5, act="relu"),
    _c("syn", "s-U+1", "U+1", N=128, Cout=17, m1=2, m2=12, act="identity"),
    _c("syn", "s-T-1", "T-1", N=128, Cout=32, m1=4, m2=16, act="gelu"),
    _c("syn", "s-T", "T", N=256, Cout=16, m1=4, m2=12, act="relu"),
    _c("syn", "s-T+1", "T+1", N=512, Cout=32, m1=4, m2=12, act="identity"),
    _c("syn", "s-3pass", "3pass", N=64, Cout=32, m1=4, m2=12, act="gelu"),
    _c("syn", "s-3pass-512", "3pass", N=512, Cout=32, m1=4, m2=16, act="relu"),
    _c("syn", "s-3pass-drain", "3pass", N=256, Cout=1, m1=3, m2=3, act="gelu"),
    _c("syn", "s-straddle", (3, 13), N=128, Cout=32, m1=4, m2=12, act="gelu"),
    _c("syn", "s-scaled", (4, 10), N=64, Cout=32, m1=4, m2=12, act="gelu", content="scaled"),
    _c("syn", "s-zero", (3, 10), N=128, Cout=20, m1=3, m2=5, act="gelu", content="zero"),
    _c("syn", "s-n64-r32", (2, 9), N=64, Cout=16, m1=3, m2=16, act="identity"),
    _c("syn", "s-nobias", (2, 9), N=256, Cout=32, m1=3, m2=12, act="relu", null=("bc",)),
]

# ... with LIFT, through rpde_fno2d_lift_block_eval_fwd (C = 32; M <= 1024 and the column stage must fit: m2 <= 8 keeps
# every symbolic M below both limits up to 400 CUs).  The gx row is read four at a time from LDS: M a multiple of 4 and
# not, and M = 1024
LIFT_CASES = [
    _c("lift", "l-1", "1", N=64, Cout=32, m1=1, m2=3, act="gelu"),
    _c("lift", "l-M9", (1, 9), N=64, Cout=31, m1=2, m2=5, act="gelu", null=("bl",)),
    _c("lift", "l-U-1", "U-1", N=64, Cout=32, m1=2, m2=5, act="gelu"),
    _c("lift", "l-T", "T", N=128, Cout=32, m1=4, m2=5, act="relu"),
    _c("lift", "l-T-1", "T-1", N=512, Cout=32, m1=4, m2=8, act="gelu"),
    _c("lift", "l-T+1", "T+1", N=256, Cout=32, m1=4, m2=5, act="identity"),
    _c("lift", "l-3pass", "3pass", N=512, Cout=32, m1=4, m2=5, act="gelu"),
    _c("lift", "l-M1024", (1, 1024), N=64, Cout=17, m1=4, m2=3, act="identity"),
    _c("lift", "l-user-grid", (2, 12), N=128, Cout=20, m1=4, m2=12, act="relu", grid="user"),
    _c("lift", "l-straddle", (3, 13), N=128, Cout=32, m1=4, m2=16, act="relu"),
]

# k_conv_syn_proj_h2: every <MT, CO> (hidden 16, 24 | 48, 64 | 100, 128; Cq 1 | 2..4), every ACT, Cout in {32, 20, 16, 1},
# R2 in {8, 16, 24, 32}; the multi-pass cases at N = 64; N = 512 opts in to more than 64 KB of dynamic LDS, N = 1024 asks
# for 150 016 bytes
PROJ_CASES = [
    _c("proj", "p-1", "1", N=64, Cout=32, m1=1, m2=3, act="gelu", Cmid=16, Cq=1),
    _c("proj", "p-U-1", "U-1", N=64, Cout=20, m1=2, m2=5, act="relu", Cmid=24, Cq=2),
    _c("proj", "p-U+1", "U+1", N=128, Cout=16, m1=2, m2=12, act="identity", Cmid=48, Cq=1),
    _c("proj", "p-T-1", "T-1", N=64, Cout=32, m1=4, m2=12, act="gelu", Cmid=64, Cq=3),
    _c("proj", "p-T", "T", N=64, Cout=1, m1=4, m2=16, act="relu", Cmid=100, Cq=1),
    _c("proj", "p-T+1", "T+1", N=64, Cout=32, m1=4, m2=3, act="gelu", Cmid=128, Cq=4),
    _c("proj", "p-3pass", "3pass", N=64, Cout=32, m1=4, m2=12, act="gelu", Cmid=128, Cq=1),
    _c("proj", "p-3pass-q4", "3pass", N=64, Cout=20, m1=3, m2=5, act="identity", Cmid=16, Cq=4),
    _c("proj", "p-straddle", (3, 13), N=128, Cout=32, m1=4, m2=5, act="gelu", Cmid=48, Cq=2),
    _c("proj", "p-n512", (2, 9), N=512, Cout=32, m1=4, m2=12, act="gelu", Cmid=128, Cq=1),
    _c("proj", "p-n1024", (2, 12), N=1024, Cout=32, m1=4, m2=16, act="gelu", Cmid=128, Cq=4),
    _c("proj", "p-scaled", (4, 10), N=64, Cout=32, m1=4, m2=12, act="gelu", Cmid=64, Cq=1, content="scaled"),
    _c("proj", "p-zero", (3, 10), N=64, Cout=16, m1=3, m2=5, act="relu", Cmid=24, Cq=3, content="zero"),
    _c("proj", "p-nobias", (2, 5), N=192, Cout=32, m1=2, m2=9, act="identity", Cmid=100, Cq=2, null=("bc", "pb1", "pb2")),
]

# k_conv_mlp_h2: the five <KS, MT> (Cin 32: hidden <= 32 | <= 64 | <= 128; Cin 64: <= 32 | <= 64), Cout 1..4 (CO 1 | 2 | 4),
# the three act_in, b1 / b2 NULL.  rows = tiles of 16 points; M = tiles per sample
MLP_CASES = [
    _c("mlp", "m-1", "1", Cin=32, Cmid=16, Cout=1, act="identity"),
    _c("mlp", "m-U-1", (3, 1), Cin=64, Cmid=32, Cout=2, act="gelu"),
    _c("mlp", "m-U+1", "U+1", Cin=32, Cmid=40, Cout=3, act="relu"),
    _c("mlp", "m-T-1", "T-1", Cin=32, Cmid=64, Cout=4, act="identity"),
    _c("mlp", "m-T", "T", Cin=64, Cmid=64, Cout=1, act="gelu"),
    _c("mlp", "m-T+1", "T+1", Cin=32, Cmid=128, Cout=2, act="identity", null=("pb1",)),
    _c("mlp", "m-3pass", "3pass", Cin=32, Cmid=128, Cout=1, act="gelu"),
    _c("mlp", "m-3pass-co4", "3pass", Cin=32, Cmid=16, Cout=4, act="relu", null=("pb2",)),
    _c("mlp", "m-straddle", (5, 3), Cin=64, Cmid=17, Cout=3, act="identity"),
    _c("mlp", "m-scaled", (4, 5), Cin=32, Cmid=100, Cout=1, act="gelu", content="scaled"),
    _c("mlp", "m-zero", (3, 6), Cin=32, Cmid=48, Cout=4, act="identity", content="zero"),
    _c("mlp", "m-nobias", (2, 7), Cin=64, Cmid=33, Cout=2, act="relu", null=("pb1", "pb2")),
]

# the multiply-add tail by shape: N in {4, 32, 1024, 2048} (whole rows per 1024-point block, half a row per block), Cin in
# {1, 5, 32, 64}, Cout in {1, 4 | 5, 8 | 9, 16 | 17, 32}: the four CO instances with and without padding; and by
# RPDE_CONV_SYN_H2=0 on every syn case (the second leg of the GPU test)
FMA_CASES = [
    _c("fma", "f-n4-co1", (2, 6), N=4, Cin=1, Cout=1, m1=2, m2=3, act="gelu"),
    _c("fma", "f-n4-co4", (2, 300), N=4, Cin=5, Cout=4, m1=3, m2=2, act="relu"),
    _c("fma", "f-n32-co5", (2, 40), N=32, Cin=32, Cout=5, m1=4, m2=12, act="identity"),
    _c("fma", "f-n32-co8", (1, 33), N=32, Cin=64, Cout=8, m1=4, m2=16, act="gelu"),
    _c("fma", "f-n1024-co9", (2, 5), N=1024, Cin=5, Cout=9, m1=2, m2=5, act="relu"),
    _c("fma", "f-n2048-co16", (1, 3), N=2048, Cin=32, Cout=16, m1=1, m2=12, act="gelu"),
    _c("fma", "f-n1024-co17", (2, 4), N=1024, Cin=64, Cout=17, m1=2, m2=3, act="identity"),
    _c("fma", "f-n2048-co32", (3, 2), N=2048, Cin=1, Cout=32, m1=1, m2=16, act="gelu", null=("bc",)),
    _c("fma", "f-zero", (3, 6), N=32, Cin=5, Cout=9, m1=2, m2=5, act="gelu", content="zero"),
    _c("fma", "f-scaled", (4, 6), N=1024, Cin=32, Cout=32, m1=2, m2=12, act="gelu", content="scaled"),
]

TABLES = {"syn": SYN_CASES, "lift": LIFT_CASES, "proj": PROJ_CASES, "mlp": MLP_CASES, "fma": FMA_CASES}
ALL_CASES = [c for t in TABLES.values() for c in t]
# the case of each persistent kernel that the planted faults are applied to
FAULT_CASES = {"syn": "s-3pass", "lift": "l-3pass", "proj": "p-3pass-q4", "mlp": "m-3pass-co4"}

# the documented eligibility edges: (query, arguments) the library must refuse
REFUSED = [
    ("rpde_fnoblock2d_eval_ok", (32, 32, 32, 32, 12)),               # N = 32, width 32, 12 modes: 96 KB of LDS
    ("rpde_fnoblock2d_eval_ok", (32, 32, 8, 96, 12)),                # N = 96 neither divides 1024 nor is a multiple of it
    ("rpde_fnoblock2d_proj_eval_ok", (32, 32, 8, 64, 4, 12, 128, 5)),   # Cq = 5
    ("rpde_fnoblock2d_proj_eval_ok", (32, 32, 8, 64, 4, 12, 129, 1)),   # hidden 129
    ("rpde_conv_mlp_ok", (64, 65, 1, 64)),                           # Cin = 64 with hidden 65
    ("rpde_conv_mlp_ok", (32, 128, 5, 64)),                          # Cout = 5
    ("rpde_conv_mlp_ok", (32, 128, 1, 72)),                          # S % 16 != 0
    ("rpde_fno2d_lift_block_eval_ok", (1, 32, 32, 1025, 64, 4, 3)),  # M > 1024
    ("rpde_fno2d_lift_block_eval_ok", (1, 32, 32, 64, 1024, 4, 12)),  # N = 1024: no h2 tail
]


def by_name(name: str) -> Case:
    return next(c for c in ALL_CASES if c.name == name)


def ok_query(case: Case, sh: Shape) -> Tuple[str, Tuple[int, ...]]:
    """the library's host-only query that must accept the case, with its arguments"""
    k = case.kernel
    if k in ("syn", "fma"):
        return "rpde_fnoblock2d_eval_ok", (case.Cin, case.Cout, sh["M"], case.N, sh["m2"])
    if k == "lift":
        return "rpde_fno2d_lift_block_eval_ok", (1, case.Cin, case.Cout, sh["M"], case.N, sh["m1"], sh["m2"])
    if k == "proj":
        return "rpde_fnoblock2d_proj_eval_ok", (case.Cin, case.Cout, sh["M"], case.N, sh["m1"], sh["m2"], case.Cmid, case.Cq)
    return "rpde_conv_mlp_ok", (case.Cin, case.Cmid, case.Cout, sh["S"])


def ok_restated(case: Case, sh: Shape) -> bool:
    k, R2 = case.kernel, 2 * r4(sh["m2"])
    if k == "syn":
        return fma_ok(case.Cin, case.Cout, sh["M"], case.N, R2) and h2_ok(case.Cin, case.Cout, sh["M"], case.N, R2)
    if k == "fma":
        return fma_ok(case.Cin, case.Cout, sh["M"], case.N, R2) and not h2_ok(case.Cin, case.Cout, sh["M"], case.N, R2)
    if k == "lift":
        return lift_ok(case.Cin, case.Cout, sh["M"], case.N, sh["m1"], sh["m2"])
    if k == "proj":
        return proj_ok(case.Cin, case.Cout, sh["M"], case.N, sh["m1"], sh["m2"], case.Cmid, case.Cq)
    return mlp_ok(case.Cin, case.Cmid, case.Cout, sh["S"])


# ---------------------------------------------------------------------------------------------------------------------
# inputs (float32 / complex64, CPU)
# ---------------------------------------------------------------------------------------------------------------------
def _gen(case: Case, sh: Shape) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(repr((case.name, sorted(sh.items()))).encode()))


def _cweight(Ci, Co, m1, m2, M, N, g):
    """complex randn (both signs, unit variance) scaled so that the spectral branch has about unit variance per point"""
    s = 0.7 * math.sqrt(M * N / (4.0 * m1 * m2 * Ci))
    return torch.complex(torch.randn(Ci, Co, m1, m2, generator=g), torch.randn(Ci, Co, m1, m2, generator=g)) * s


def make_inputs(case: Case, sh: Shape) -> Dict[str, torch.Tensor]:
    g = _gen(case, sh)
    B, M, N, m1, m2 = sh["B"], sh["M"], sh["N"], sh["m1"], sh["m2"]
    inp: Dict[str, torch.Tensor] = {}
    if case.kernel == "mlp":
        inp["x"] = torch.randn(B, case.Cin, sh["S"], generator=g)
        inp["pw1"] = torch.randn(case.Cmid, case.Cin, generator=g) * (1.0 / math.sqrt(case.Cin))
        inp["pb1"] = torch.randn(case.Cmid, generator=g) * 0.3
        inp["pw2"] = torch.randn(case.Cout, case.Cmid, generator=g) * (1.0 / math.sqrt(case.Cmid))
        inp["pb2"] = torch.randn(case.Cout, generator=g) * 0.3
    else:
        if case.kernel == "lift":
            inp["u"] = torch.randn(B, 1, M, N, generator=g)
            if case.grid == "user":
                inp["gx"], inp["gy"] = torch.randn(M, generator=g), torch.randn(N, generator=g)
            else:
                inp["gx"], inp["gy"] = torch.linspace(0, 1, M), torch.linspace(0, 1, N)
            inp["wl"] = torch.randn(case.Cin, 3, generator=g) * 0.5
            inp["bl"] = torch.randn(case.Cin, generator=g) * 0.1
        else:
            inp["x"] = torch.randn(B, case.Cin, M, N, generator=g)
        inp["w1"] = _cweight(case.Cin, case.Cout, m1, m2, M, N, g)
        inp["w2"] = _cweight(case.Cin, case.Cout, m1, m2, M, N, g)
        inp["wc"] = torch.randn(case.Cout, case.Cin, generator=g) * (1.0 / math.sqrt(case.Cin))
        inp["bc"] = torch.randn(case.Cout, generator=g) * 0.3
        if case.kernel == "proj":
            inp["pw1"] = torch.randn(case.Cmid, case.Cout, generator=g) * (1.0 / math.sqrt(case.Cout))
            inp["pb1"] = torch.randn(case.Cmid, generator=g) * 0.3
            inp["pw2"] = torch.randn(case.Cq, case.Cmid, generator=g) * (1.0 / math.sqrt(case.Cmid))
            inp["pb2"] = torch.randn(case.Cq, generator=g) * 0.3
    field = inp["u" if case.kernel == "lift" else "x"]
    if case.content == "scaled":
        assert B >= 2 and case.kernel != "lift"
        field *= sample_scales(B).float().view(B, *([1] * (field.dim() - 1)))
    elif case.content == "zero":
        assert B >= 2 and case.kernel != "lift"
        field[1] = 0.0
    else:
        assert case.content == "randn"
    for k in case.null:
        assert k in ("bc", "bl", "pb1", "pb2"), (case.name, k)
        inp.pop(k)
    return inp


def sample_scales(B: int) -> torch.Tensor:
    """four decades over the samples"""
    return torch.pow(10.0, torch.linspace(-2.0, 2.0, B, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------------
# the oracle, in `real`
# ---------------------------------------------------------------------------------------------------------------------
def _to(inp, real):
    cplx = torch.complex128 if real == torch.float64 else torch.complex64
    return {k: v.to(cplx if v.is_complex() else real) for k, v in inp.items()}


def lifted(t) -> torch.Tensor:
    """cat(u, gx, gy) -> Conv1x1(wl, bl): reference models/fno.py:121-141"""
    u = t["u"]
    B, _, M, N = u.shape
    gx = t["gx"].view(1, 1, M, 1).expand(B, 1, M, N)
    gy = t["gy"].view(1, 1, 1, N).expand(B, 1, M, N)
    return S._conv(t["wl"], torch.cat([u, gx, gy], dim=1), t.get("bl"))


def pre_activation(t) -> torch.Tensor:
    """run_oracle("block", ..)'s forward expression with the identity in front"""
    x = lifted(t) if "u" in t else t["x"]
    return R.spectral_conv2d(x, t["w1"], t["w2"]) + S._conv(t["wc"], x, t.get("bc"))


def _mlp(t, h) -> torch.Tensor:
    return S._conv(t["pw2"], F.gelu(S._conv(t["pw1"], h, t.get("pb1"))), t.get("pb2"))


def evaluate(case: Case, inp, real=torch.float64) -> torch.Tensor:
    """what the case's entry point computes -> [B, Cout | Cq, M, N] (mlp: [B, Cout, S])"""
    with torch.no_grad():
        t = _to(inp, real)
        if case.kernel == "mlp":
            return _mlp(t, R._act(case.act)(t["x"]))
        h = R._act(case.act)(pre_activation(t))
        return _mlp(t, h) if case.kernel == "proj" else h


# ---------------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------------
def lines(case: Case, t: torch.Tensor) -> torch.Tensor:
    """[B, lines, points]: a line is one (b, o, m) row of N points; conv_mlp: one tile of 16 points"""
    n = 16 if case.kernel == "mlp" else t.shape[-1]
    return t.reshape(t.shape[0], -1, n)


def line_stat(case: Case, got: torch.Tensor, ref: torch.Tensor) -> float:
    """spectral_cf_ref.line_rel over every line; the sample-scaled case normalises per sample and takes the worst sample"""
    a, b = lines(case, got), lines(case, ref)
    if case.content == "scaled":
        return max(S.line_rel(a[i], b[i]) for i in range(a.shape[0]))
    return S.line_rel(a, b)


def figures(case: Case, got: torch.Tensor, ref: torch.Tensor) -> Dict[str, float]:
    return {"rel": S.rel(got, ref), "line": line_stat(case, got, ref)}


@functools.lru_cache(maxsize=3)
def reference(case: Case, cus: int):
    """-> (shape, inputs, float64 result, the float32 oracle's figures against it); shared by the legs of a case"""
    sh = resolve(case, cus)
    inp = make_inputs(case, sh)
    ref = evaluate(case, inp, torch.float64)
    return sh, inp, ref, figures(case, evaluate(case, inp, torch.float32), ref)


def zero_sample_planes(case: Case, ref: torch.Tensor) -> torch.Tensor:
    """content "zero": the constant of every plane (o) of sample 1, from the float64 result"""
    plane = ref[1].reshape(ref.shape[1], -1)
    assert bool((plane == plane[:, :1]).all()), case.name
    return plane[:, 0]


# ---------------------------------------------------------------------------------------------------------------------
# planted faults: what a broken pass loop would leave in `out`
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ("stale", "unwritten", "last", "segment")


def plant(case: Case, sh: Shape, cus: int, ref: torch.Tensor, kind: str, size: float = 1.0) -> torch.Tensor:
    """ref with one line (one tile for conv_mlp) wrong, as one of
      stale      the line one pass earlier in the same wave (a prefetch that was not replaced), in the third pass
      unwritten  a line of the second pass left as it was (zeros)
      last       the last line of the last pass dropped (zeros)
      segment    a 64-point segment of a line (a wave's share; N = 64 and conv_mlp: the whole line) swapped with the next
    size < 1 blends: ref + size (fault - ref), to find what the whole-tensor norm still sees"""
    T = full_pass(case, cus)
    row_pts = 16 if case.kernel == "mlp" else sh["N"]
    rows = sh["rows"]
    C = ref.shape[1]
    # [B, C, rows of the sample, points] -> a row (b, m) of channel o
    v = ref.clone().reshape(sh["B"], C, sh["M"], row_pts)
    bad = v.clone()
    o = C - 1

    def at(r):
        return r // sh["M"], o, r % sh["M"]

    if kind == "stale":
        r = 2 * T + 1
        assert r < rows
        bad[at(r)] = v[at(r - T)]
    elif kind == "unwritten":
        bad[at(T + 2)] = 0.0
    elif kind == "last":
        bad[at(rows - 1)] = 0.0
    elif kind == "segment":
        r = T + 5
        seg = min(64, row_pts)
        if row_pts >= 128:
            bad[at(r)][:seg], bad[at(r)][seg:2 * seg] = v[at(r)][seg:2 * seg].clone(), v[at(r)][:seg].clone()
        else:
            bad[at(r)], bad[at(r + 1)] = v[at(r + 1)].clone(), v[at(r)].clone()
    else:
        raise KeyError(kind)
    return (v + size * (bad - v)).reshape(ref.shape)
