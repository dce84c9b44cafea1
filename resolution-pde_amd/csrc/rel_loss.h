// What the relative losses share (rel_loss.hip): rel[b] = num[b] / (den[b] + REL_EPS) from two per-sample norms kept in
// stats[b] = (num, den), then mean / sum / the per-sample vector.  The relative L2 loss itself lives in rel_loss.hip; the
// mode-weighted loss (spectral_loss.hip) and the equation residuals (etd_residual.hip, ns_residual.hip) end in rel_final
// and form their backward coefficient with rel_coef; the two residuals also share their affine decode, their roots of
// unity and their block epilogue; band_energy.hip shares rel_diff and the slot count.
#pragma once
#include "rpde_internal.h"

namespace rpde {

constexpr float REL_EPS = 1e-8f;     // the one guard of the ratio's denominator

__device__ __forceinline__ float rel_ratio(float num, float den) { return num / (den + REL_EPS); }

// d (reduced loss) / d num[b] / num[b]: the factor in front of every relative loss's gradient, from the saved stats and
// the upstream gradient (grad_rel [B] for the per-sample vector, else the scalar grad_loss); 0 where num = 0
__device__ __forceinline__ float rel_coef(const float* __restrict__ stats, const float* __restrict__ grad_loss,
                                          const float* __restrict__ grad_rel, int b, int B, int size_average) {
  const float dn = stats[2 * b], yn = stats[2 * b + 1];
  const float gr = grad_rel ? grad_rel[b] : (size_average ? grad_loss[0] / B : grad_loss[0]);
  return dn > 0.f ? gr / (dn * (yn + REL_EPS)) : 0.f;
}

// float64 partial sums per (field, sample) or (sample, band) at most, and how many a sum of `terms` terms is split into
constexpr int REL_SLOTS = 32;
inline int rel_slots(long terms) { return (int)((terms + 2047) / 2048 < REL_SLOTS ? (terms + 2047) / 2048 : REL_SLOTS); }

// The tail of the float64 two-stage losses, one workgroup.  part[(f B + b) S + slot]: field 0 the numerator's energy,
// field 1 the denominator's.  stats[b] = (sqrt(inv E_0), sqrt(inv E_1)), rel[b] (may be null), loss = mean / sum (may be
// null).  Slots are added in order, no atomics: identical calls give identical bits
int rel_final(const double* part, float* rel, float* loss, float* stats, int B, int S, double inv, int size_average,
              hipStream_t st);

// The block epilogue of those two-field sums (grid (S, B, ...), a block of one wave or of four): the block's er and ex
// into its slot blockIdx.x of fields 0 and 1 of sample b.  Four waves add as (w0 + w1) + (w2 + w3), one wave's sum
// stands as it is; every thread of the block calls it.  `four` comes from the kernel: a constant where the block is
// always 256 threads, else read from blockDim where every thread runs (read inside the last thread's branch it is a
// memory load behind the barrier, at the tail of every block)
__device__ __forceinline__ void rel_block_slots(double er, double ex, double* __restrict__ part, int b, int B, bool four) {
  __shared__ double red[2][4];
  er = wave_sum(er);
  ex = wave_sum(ex);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = er; red[1][threadIdx.x >> 6] = ex; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[(long)b * gridDim.x + blockIdx.x] = four ? (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]) : red[0][0];
    part[((long)B + b) * gridDim.x + blockIdx.x] = four ? (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]) : red[1][0];
  }
}

// What the equation residuals (etd_residual.hip, ns_residual.hip) share beyond the tail.  The affine decode of the two
// fields, p~ = ap p + bp and x~ = ax x + bx, from the caller's four floats (null: the identity)
struct RelAffine { float ap, bp, ax, bx; };
inline RelAffine rel_affine(const float* affine) {
  return affine ? RelAffine{affine[0], affine[1], affine[2], affine[3]} : RelAffine{1.f, 0.f, 1.f, 0.f};
}

// tw[j] = (cos, -sin)(2 pi j / N), j < N, then the same for M: tw[N + j], j < M (M = 0: one axis) -- the float64 roots of
// unity of the residuals' analyses.  sincospi is exact at the multiples of a quarter turn, so Im of the mean and Nyquist
// bins is exactly zero
int rel_roots(double2* tw, int N, int M, hipStream_t st);

// d = x - y over `total` floats, in fp32 BEFORE any transform (freq_energy.hip has the reason: for a decent model the
// difference of two spectra loses the digits, the spectrum of the difference does not).  d: 16-byte aligned (the arena's
// pieces are)
int rel_diff(const float* x, const float* y, float* d, long total, hipStream_t st);

}  // namespace rpde
