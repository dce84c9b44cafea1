// What the relative losses share (rel_loss.hip): rel[b] = num[b] / (den[b] + REL_EPS) from two per-sample norms kept in
// stats[b] = (num, den), then mean / sum / the per-sample vector.  The relative L2 loss itself lives in rel_loss.hip; the
// mode-weighted loss (spectral_loss.hip) and the equation residual (etd_residual.hip) end in rel_final and form their
// backward coefficient with rel_coef; band_energy.hip shares rel_diff and the slot count.
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

// d = x - y over `total` floats, in fp32 BEFORE any transform (freq_energy.hip has the reason: for a decent model the
// difference of two spectra loses the digits, the spectrum of the difference does not).  d: 16-byte aligned (the arena's
// pieces are)
int rel_diff(const float* x, const float* y, float* d, long total, hipStream_t st);

}  // namespace rpde
