"""Shape tables, inputs, error measures and an independent float64 statement of the spectral resizers (test
infrastructure only; the product tree does not import it).

    1-D  out = x A(n_in, k)^T S(n_out, k)^T n_out / n_in,   k = min(n_in // 2 + 1, n_out // 2 + 1)
    2-D  the same along N; between the two N-axis transforms the complex DFT along M restricted to the rows
         [0, top) u [M - bot, M), re-embedded at [0, top) u [Mo - bot, Mo) of the target spectrum,
         top = min((M + 1) // 2, (Mo + 1) // 2), bot = min(M // 2, Mo // 2)

with A / S the truncated real-DFT matrices of oracle/dft_math.py ('backward' norm).  tests/test_resize_ref_cpu.py pins
oracle.reference_path.resize_1d / resize_2d (the torch.fft statement the GPU tests compare with) to these matrices.

Which kernel a shape takes (csrc/cf_dft.hip, cf_h2_eligible / cf_h2_syn_eligible; kp = k rounded up to 4, R = 2 kp):
the h2 analysis needs n_in % 128 == 0, R <= 32 and (n_in / 32) ceil(R / 16) 2 KB <= 64 KB, the h2 synthesis the same
at n_out and n_out <= 512; both only from 16 rows on.  Everything else is the generic GEMM path."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import dft_math as D

FWD_TOL = 1e-5            # the project's forward parity budget (tests/test_gpu_golden.py, BASELINE.json)
SEED = 17

# ---- 1-D: (n_in, n_out) ------------------------------------------------------------------------------------------
H2_ANALYSIS_1D = [(128, 16), (256, 7), (384, 26), (512, 30), (1024, 14)]     # 512->30 and 1024->14: table exactly 64 KB
OUTSIDE_ANALYSIS_1D = [(1024, 30), (640, 16), (1024, 32)]                    # table too big (twice), R = 40
H2_SYNTHESIS_1D = [(16, 128), (7, 256), (26, 384), (30, 512), (31, 128)]     # alpha = n_out / n_in != 1
OUTSIDE_SYNTHESIS_1D = [(14, 1024)]                                          # n_out > 512
GENERIC_1D = [(64, 96), (96, 64), (64, 64), (63, 63), (64, 33), (33, 64), (65, 31), (31, 65), (100, 36), (130, 129),
              (1023, 1024), (2, 7), (7, 2), (3, 2), (2, 3)]
H2_1D = H2_ANALYSIS_1D + H2_SYNTHESIS_1D
OUTSIDE_1D = OUTSIDE_ANALYSIS_1D + OUTSIDE_SYNTHESIS_1D
SHAPES_1D = H2_1D + OUTSIDE_1D + GENERIC_1D
# rows as [B, C]: 15 / 16 / 17 sit on either side of the `rows >= 16` switch, 100 is several tiles with a partial last one
ROWS_1D = {1: (1, 1), 15: (3, 5), 16: (2, 8), 17: (1, 17), 100: (4, 25)}

# ---- 2-D: ((M, N), (Mo, No)) -------------------------------------------------------------------------------------
H2_ANALYSIS_2D = [((128, 128), (16, 16)), ((256, 128), (24, 20)), ((96, 256), (40, 30))]
H2_SYNTHESIS_2D = [((16, 16), (128, 128)), ((24, 20), (256, 128)), ((20, 30), (33, 512))]
GENERIC_2D = [((64, 48), (48, 96)), ((48, 96), (64, 48)), ((32, 32), (32, 32)), ((31, 33), (31, 33)),
              ((40, 40), (25, 27)), ((25, 27), (40, 40)), ((33, 20), (20, 33)), ((2, 2), (5, 4)), ((5, 4), (2, 2)),
              ((3, 6), (2, 9)), ((130, 36), (129, 35))]
H2_2D = H2_ANALYSIS_2D + H2_SYNTHESIS_2D
SHAPES_2D = H2_2D + GENERIC_2D
ROWS_2D = {1: (1, 1), 3: (1, 3), 6: (2, 3)}

# ---- closed forms (an averaged norm cannot hide a boundary bin here) ----------------------------------------------
PHI = 0.7


def closed_form_up():
    """x[j] = cos(pi j) at 64 -> 96: the source Nyquist bin becomes an ordinary bin of weight 2.
    -> (x [64], expected [96]) float64"""
    j, t = np.arange(64), np.arange(96)
    return torch.from_numpy(np.cos(math.pi * j)), torch.from_numpy(2.0 * np.cos(2.0 * math.pi * 32 * t / 96))


def closed_form_down():
    """x[j] = cos(2 pi 32 j / 96 + phi) at 96 -> 64: bin 32 lands on the target's Nyquist bin, whose imaginary part is
    dropped and whose weight is 1.  -> (x [96], expected [64]) float64"""
    j, t = np.arange(96), np.arange(64)
    return (torch.from_numpy(np.cos(2.0 * math.pi * 32 * j / 96 + PHI)),
            torch.from_numpy(0.5 * math.cos(PHI) * np.cos(math.pi * t)))


def shape_id(s):
    if isinstance(s[0], tuple):
        return "x".join(map(str, s[0])) + "-" + "x".join(map(str, s[1]))
    return f"{s[0]}-{s[1]}"


# ---- inputs (fp32, CPU) --------------------------------------------------------------------------------------------
def make_input(shape, kind, spatial_dims):
    """kind 'randn', or 'scaled': row (1-D) / image (2-D) i times 2**((7 i) % 21 - 10) -- a 2^+-10 range inside one
    16-row tile, which shares ONE power-of-two scale in the h2 kernels"""
    g = torch.Generator().manual_seed(SEED + sum(shape) + 1000 * spatial_dims)
    x = torch.randn(*shape, generator=g, dtype=torch.float32)
    if kind == "scaled":
        lead = shape[:-spatial_dims]
        rows = int(np.prod(lead))
        e = (7 * torch.arange(rows)) % 21 - 10
        x = x * torch.pow(2.0, e.float()).view(*lead, *([1] * spatial_dims))
    elif kind != "randn":
        raise ValueError(kind)
    return x


# ---- error measures ------------------------------------------------------------------------------------------------
def rel(a, b):
    """whole-tensor relative L2 error of a against b"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def row_rel(a, b, spatial_dims=1):
    """largest relative L2 error of one row (1-D) / one image (2-D)"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    n = int(np.prod(b.shape[-spatial_dims:]))
    a, b = a.reshape(-1, n), b.reshape(-1, n)
    return float(((a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-300)).max())


# ---- the matrix statement ------------------------------------------------------------------------------------------
def _kept(n_in, n_out):
    return min(n_in // 2 + 1, n_out // 2 + 1)


def matrix_resize_1d(x, n_out):
    """x [..., n_in] -> float64 [..., n_out]"""
    x = x.double()
    n_in = x.shape[-1]
    k = _kept(n_in, n_out)
    A = torch.from_numpy(D.analysis(n_in, k, "backward"))             # [2k, n_in]
    S = torch.from_numpy(D.synthesis(n_out, k, "backward"))           # [n_out, 2k]
    return x @ A.T @ S.T * (n_out / n_in)


def kept_rows(M, Mo):
    """(rows_in, rows_out): the bins along M that survive and where they land along Mo"""
    top, bot = min((M + 1) // 2, (Mo + 1) // 2), min(M // 2, Mo // 2)
    rows_in = np.concatenate([np.arange(top), np.arange(M - bot, M)])
    rows_out = np.concatenate([np.arange(top), np.arange(Mo - bot, Mo)])
    return rows_in, rows_out


def matrix_resize_2d(x, out_size):
    """x [..., M, N] -> float64 [..., Mo, No]"""
    x = x.double()
    M, N = x.shape[-2], x.shape[-1]
    Mo, No = out_size
    k = _kept(N, No)
    A = torch.from_numpy(D.analysis(N, k, "backward"))
    S = torch.from_numpy(D.synthesis(No, k, "backward"))
    rows_in, rows_out = kept_rows(M, Mo)
    CA = torch.from_numpy(D.complex_analysis(M, rows_in, "backward"))       # [R, M]
    CS = torch.from_numpy(D.complex_synthesis(Mo, rows_out, "backward"))    # [Mo, R]
    s = x @ A.T                                                              # [..., M, 2k] (re, im) interleaved
    z = torch.complex(s[..., 0::2], s[..., 1::2])                            # [..., M, k]
    z = CS @ (CA @ z)                                                        # [..., Mo, k]
    t = torch.stack((z.real, z.imag), dim=-1).flatten(-2)                    # [..., Mo, 2k] interleaved again
    return t @ S.T * ((Mo / M) * (No / N))
