"""The plain instance k_conv1x1_small<CO, false> of csrc/conv_small.hip through rpde_conv1x1_fwd / rpde_conv1x1_act_fwd,
per point, in guarded and poisoned buffers (tests/thin_abi.py; what these tests rest on is checked without a GPU in
tests/test_thin_ref_cpu.py).

thin_abi.CONV_CASES: every CO of 4, 8, 16, 32 full and with padded output channels, one and 255 live threads in the
last block, a tail of S % 1024 = 344 points with B on blockIdx.y, 64 KiB of dynamic LDS at Cin = 512, and
blockIdx.y = 65534 with five live threads per block.  thin_abi.CONV_FALLBACKS: S % 4 != 0, Cout = 33 and x or out
starting 4 bytes into its allocation must be right on the GEMM path.

Legs: (identity, identity, accumulate 0) on every case; on the cases with padded channels and the 65535 case also
(gelu, identity, 1) and (identity, relu, 1) and bias NULL; RPDE_CONV_SMALL=0 once per case.  With integers in and
integers out (identity / relu) the `exact` kind must equal float64 bit for bit; everything else stays, at every point,
within (Cin + 3) u S_abs (+ 16 u S_abs on the GEMM path, + GELU_TOL sum_i |W[o][i]| for gelu on the input).  On randn the
default and the switched-off leg differ in bits exactly where conv_plan says the kernel runs.  Guards stay intact, and
without accumulate no poison is left.

The float64 reference of (1, 512, 17, 2^20) -- 18 GFLOP, 2 GiB of input drawn on the device -- is formed with torch
float64 on the device and cross-checked against the CPU on the first and the last 4096 points; so are the references
of the other cases of 2^26 multiply-adds and more (thin_abi.conv_ref_device), whose legs together take the CPU several
seconds.  Their inputs are drawn on the CPU like everyone else's.

Each test prints its worst figure (pytest -s).  Measured on an MI355X, as a fraction of the bound: 0.552 at
(65535, 3, 5, 20), randn, (identity, relu, accumulate 1), element 4077428; 0.506 at (3, 5, 5, 349528) on the same leg;
0.40 and less on the cases of Cin >= 7, 0.040 at Cin = 512; 0.145 and less on the GEMM path of the neighbours.  Every
`exact` problem with identity / relu was bit-equal to float64 on both paths, and the device-formed references agreed
with the CPU's."""
import pytest
import torch

from tests import thin_abi as A

pytestmark = pytest.mark.gpu

OFF = {"RPDE_CONV_SMALL": "0"}


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _cross_check(prob, ref, bnd, leg) -> None:
    """a reference formed on the device against the CPU's on the first and the last CROSS_POINTS points: float64
    summation orders differ by some 2^-53 Cin S_abs, 2^-20 of the bound is far above that and far below a float32 error"""
    S = prob["case"][3]
    for pts in (slice(0, A.CROSS_POINTS), slice(S - A.CROSS_POINTS, S)):
        cref, cbnd = A.conv_reference(prob, *leg, points=pts, device="cpu")
        assert bool(((ref[:, :, pts].cpu() - cref).abs() <= 2.0 ** -20 * cbnd).all()), (prob["case"], leg, pts)
        assert bool(((bnd[:, :, pts].cpu() - cbnd).abs() <= 2.0 ** -20 * cbnd).all()), (prob["case"], leg, pts)


def _run_case(dev, case, gemm: bool, misalign=None):
    B, Cin, Cout, S = case
    more = A.conv_more_legs(case) and not gemm
    legs = [(*l, True) for l in A.CONV_LEGS + (A.CONV_MORE_LEGS if more else [])]
    legs += [("identity", "identity", 0, False)] if more else []
    worst = (-1.0, "")
    for kind in A.KINDS:
        where, ref_on = A.conv_device(case, dev), A.conv_ref_device(case, dev)
        prob = A.conv_problem(kind, case, where)
        for act_in, act_out, acc, bias in legs:
            what = f"{kind} {act_in}/{act_out} acc={acc} bias={bias}"
            ref, bnd = A.conv_reference(prob, act_in, act_out, acc, bias, gemm=gemm, device=ref_on)
            if ref_on != "cpu":
                _cross_check(prob, ref, bnd, (act_in, act_out, acc, bias, gemm))
            got = A.run_conv_small(dev, prob, act_in=act_in, act_out=act_out, accumulate=acc, bias=bias, misalign=misalign)
            exact = A.conv_is_exact(prob, act_in, act_out)
            f, i, missed = A.conv_misses(got, ref, bnd, exact)
            assert not missed, (case, what, f, i)
            if not exact and f > worst[0]:
                worst = (f, f"{what}, element {i}")
            if (act_in, act_out, acc, bias) != ("identity", "identity", 0, True):
                continue
            off = A.run_conv_small(dev, prob, env=OFF, misalign=misalign)
            scale = (Cin + 3 + A.ROW_MARGIN) / (Cin + 3 + (A.ROW_MARGIN if gemm else 0.0))
            f, i, missed = A.conv_misses(off, ref, bnd * scale, exact)
            assert not missed, (case, what, "switched off", f, i)
            if kind == "randn":
                taken = A.conv_plan(*case, aligned=misalign is None)["taken"]
                assert taken != gemm and _same_bits(got, off) == (not taken), (case, "default / switched off", taken)
            del off
        del prob
    print(f"\n[conv_small] {case} misalign={misalign}: {worst[0]:.3f} of its bound ({worst[1]})")


@pytest.mark.parametrize("case", [c for c, _ in A.CONV_CASES], ids=str)
def test_conv_small_per_point(gpu_device, case):
    _run_case(gpu_device, case, gemm=False)


@pytest.mark.parametrize("case,misalign", A.CONV_FALLBACKS, ids=str)
def test_conv_small_neighbours_take_the_gemm_path(gpu_device, case, misalign):
    _run_case(gpu_device, case, gemm=True, misalign=misalign)
