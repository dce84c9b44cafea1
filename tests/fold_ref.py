"""The summation order of the slab fold (csrc/pointwise.hip, slab_partial and k_fold_jobs), restated in numpy.

Every deterministic reduction of the library ends in  out[i] = sum_s slabs[s][i]  over S partial-sum slabs, and one
kernel computes all of them in one order.  Per output:

  wave ty of four takes the slabs ty, ty + 4, ty + 8, ...; call them t_0, t_1, ... (T of them).
  It keeps eight accumulators a[0..7], all zero at the start, and walks its slabs in three loops:
    while at least 32 are left:  a[j & 7] += t_j  for the next j = 0 .. 31   (32 loads in flight)
    while at least  8 are left:  a[j] += t_j      for the next j = 0 .. 7    ( 8 loads in flight)
    the rest, one by one:        a[0] += t
  then  w = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)),
  and the four waves meet as  (w0 + w1) + (w2 + w3).

Every add is a float32 add, rounded to nearest; numpy's float32 arithmetic does exactly that.  `fold_f32` is this order,
`fold_f32_no32` the same without the 32-deep loop (the order of the segment fold this kernel replaced: the 32-deep loop
feeds accumulator j & 7 with the same slabs in the same sequence as four rounds of the 8-deep one, so the two agree bit for
bit, which tests/test_fold_ref_cpu.py checks), `fold_serial` one running sum, and `fold_f64` the float64 sum the error
bounds are stated against."""
from __future__ import annotations

import numpy as np

WAVES = 4
# slab counts at the edges of the walker's three loops for each of the four waves
S_EDGES = [1, 2, 3, 4, 5, 28, 29, 32, 33, 60, 61, 124, 125, 128, 129, 132, 157, 253, 256, 257, 300]
# output counts at the edges of the 64-output workgroup
N_EDGES = [1, 63, 64, 65, 130]
EPS32 = 2.0 ** -24                     # one float32 roundoff (unit roundoff, round to nearest)


def _wave_partial(x: np.ndarray, ty: int, deep: bool) -> np.ndarray:
    """x [S, n] float32 -> wave ty's sum [n] float32"""
    assert x.dtype == np.float32 and x.ndim == 2
    S = x.shape[0]
    a = [np.zeros(x.shape[1], np.float32) for _ in range(8)]
    s = ty
    while deep and s + 124 < S:
        for j in range(32):
            a[j & 7] = a[j & 7] + x[s + 4 * j]
        s += 128
    while s + 28 < S:
        for j in range(8):
            a[j] = a[j] + x[s + 4 * j]
        s += 32
    while s < S:
        a[0] = a[0] + x[s]
        s += 4
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))


def _fold(x: np.ndarray, deep: bool) -> np.ndarray:
    w = [_wave_partial(x, ty, deep) for ty in range(WAVES)]
    out = (w[0] + w[1]) + (w[2] + w[3])
    assert out.dtype == np.float32
    return out


def fold_f32(x: np.ndarray) -> np.ndarray:
    """x [S, n] float32 -> [n] float32 in the kernel's order"""
    return _fold(x, True)


def fold_f32_no32(x: np.ndarray) -> np.ndarray:
    """the same without the 32-deep loop"""
    return _fold(x, False)


def fold_serial(x: np.ndarray) -> np.ndarray:
    """one running float32 sum over s = 0, 1, ..."""
    assert x.dtype == np.float32
    acc = np.zeros(x.shape[1], np.float32)
    for s in range(x.shape[0]):
        acc = acc + x[s]
    return acc


def fold_f64(x: np.ndarray) -> np.ndarray:
    return x.astype(np.float64).sum(axis=0)


def slabs(S: int, n: int, seed: int = 0) -> np.ndarray:
    """[S, n] float32, normal values spread over twelve binary orders of magnitude (so that the order of the adds shows
    in the last bits) and no zero among them (a sum of zeros could differ in sign alone)"""
    rng = np.random.default_rng([seed, S, n])
    x = rng.standard_normal((S, n)) * np.exp2(rng.integers(-6, 7, size=(S, n)))
    x = x.astype(np.float32)
    x[x == 0] = np.float32(1.0)
    return x
