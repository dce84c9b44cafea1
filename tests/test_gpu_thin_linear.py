"""csrc/thin_linear.hip through rpde_linear_fwd / rpde_linear_bwd, per point, in guarded and poisoned buffers
(tests/thin_abi.py; what these tests rest on is checked without a GPU in tests/test_thin_ref_cpu.py).

Every T of 1 .. 4 with every O of 4 .. 256 runs in both roles -- lifting (in = T, out = O): forward = k_thin_expand,
data gradient = k_thin_contract, weight gradient = k_thin_outer with G transposed and cs the bias gradient; projection
(in = O, out = T): forward = contract, data gradient = expand through the strided weight view, weight gradient = outer
with ts the bias gradient -- at 1, 15, 16, 17, pps - 1, pps + 1 and 129 points, and at the large point counts of
thin_abi.LARGE_POINTS for the shapes named there (a second grid-stride trip, the capped outer grid with empty
workgroups, the 8-deep loop with a ragged remainder).  The neighbours thin_linear_ok refuses, (3, 12), (3, 192), (5, 64)
and (3, 260), must be right on the GEMM path.

Legs per case: the default twice (bit-identical), RPDE_THIN_LINEAR=0, bias NULL, each single output with the others
NULL, and at 129 and 8193 points each of y / x / grad_out / dx starting 4 bytes into its allocation.  The workspace is
exactly rpde_linear_ws_bytes and poisoned; guards and poison are checked in every call.

The `exact` kind (integers -3 .. 3) must equal float64 bit for bit on every leg.  On the randn kind y and dx stay, per
element, within (products + 2) u S_abs (+ 16 u S_abs on a GEMM-path leg), dW and db within 1e-5 of the whole tensor.
From 8193 points dW of the default leg differs in bits from the switched-off leg for the thin shapes and is identical
for the refused ones: that shows which path ran.

Each test prints its worst figures (pytest -s).  Measured on an MI355X, the worst over all cases as a fraction of its
bound, thin kernels | GEMM-path legs (switched off, misaligned, refused shapes):
    y   0.561 (lifting T = 4, O = 256, P = 140001, bias NULL, element 33333883) | 0.154 (lifting (5, 64), P = 8193)
    dx  0.583 (projection T = 4, O = 256, P = 131073, element 14093947)         | 0.134 (projection (5, 64), P = 8193)
    dW  0.038 (lifting T = 2, O = 4, P = 255)                                   | 0.089 (lifting T = 4, O = 4, P = 2100001)
    db  0.207 (projection T = 1, O = 256, P = 131073)                           | 0.102 (projection T = 1, O = 16, P = 15)
and every `exact` problem bit-equal to float64 on every leg.  (y and dx of T = 3 and 4 sit above one half: the kernels
add the bias first, see thin_abi.chain32.)

What these tests found: projection T = 1, O = 256 at P = 131073, randn, RPDE_THIN_LINEAR=0 missed the 1e-5 of db.  db is
there a tensor of one element, the sum of 131073 randn values: -19.91 against sum |grad_out| = 104387.  k_colsum
(pointwise.hip) let one thread add the 256 row-lane partials of a column in turn, a running sum through 255 roundings per
workgroup: 2.75e-4 off, 1.383 of the bound (a float32 emulation of the kernel on the CPU gives the same bits).  The
partials now fold as a fixed tree (0.073 in the emulation), and the worst db of that case over all legs is the thin
kernels' 0.207.
"""
import pytest
import torch

from tests import thin_abi as A

pytestmark = pytest.mark.gpu

OFF = {"RPDE_THIN_LINEAR": "0"}
CASES = [(role, T, O, 0) for T, O in A.THIN_SHAPES + A.REFUSED_SHAPES for role in A.ROLES] + \
        [(role, T, O, P) for P, (shapes, _) in A.LARGE_POINTS.items() for T, O in shapes for role in A.ROLES] + \
        [(role, T, O, 8193) for T, O in A.REFUSED_SHAPES for role in A.ROLES]


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _legs(dev, prob, thin: bool, worst: dict, misses: list) -> None:
    P, kind = prob["P"], prob["kind"]
    tag = f"{kind} P={P}"
    first, again = A.run_linear_thin(dev, prob), A.run_linear_thin(dev, prob)
    for k in first:
        assert _same_bits(first[k], again[k]), (tag, k, "not reproducible")
    A.check_linear(first, prob, tag + " default", gemm=not thin, worst=worst, misses=misses)
    del again
    off = A.run_linear_thin(dev, prob, env=OFF)
    A.check_linear(off, prob, tag + " off", gemm=True, worst=worst, misses=misses)
    if kind == "randn" and P >= 8193:
        assert _same_bits(first["dW"], off["dW"]) == (not thin), (tag, "dW default / switched off", thin)
    del first, off
    A.check_linear(A.run_linear_thin(dev, prob, bias=False), prob, tag + " no bias", bias=False, gemm=not thin, worst=worst,
                   misses=misses)
    for w in ("dx", "dW", "db"):
        A.check_linear(A.run_linear_thin(dev, prob, want=(w,)), prob, f"{tag} want {w}", gemm=not thin, worst=worst, misses=misses)
    if P in A.MISALIGN_POINTS:
        for m in A.MISALIGN:
            A.check_linear(A.run_linear_thin(dev, prob, misalign=m), prob, f"{tag} misaligned {m}", gemm=True, worst=worst,
                           misses=misses)


@pytest.mark.parametrize("role,T,O,P", CASES, ids=lambda v: str(v))
def test_thin_linear_per_point(gpu_device, role, T, O, P):
    """one shape in one role at the small point counts (P = 0) or at one large one; every leg, both kinds"""
    in_f, out_f = A.shape_of(role, T, O)
    thin = A.is_thin(in_f, out_f)
    worst: dict = {}
    misses: list = []
    for n in ([P] if P else A.small_points(T, O)):
        for kind in A.KINDS:
            _legs(gpu_device, A.linear_problem(kind, n, in_f, out_f), thin, worst, misses)
    print(f"\n[thin_linear] {role} T={T} O={O} P={P or 'small'} thin={thin}: " +
          "; ".join(f"{k} {f:.3f} of its bound ({what}, element {i})" for k, (f, what, i) in sorted(worst.items())))
    assert not misses, misses
