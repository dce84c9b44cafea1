// What the 1-D and 2-D CNO activation kernels (cno.hip, cno2d.hip) share: the banded table as the device sees it, the
// dot product over one of its rows, the range a run of rows reads, the host's bounds on those ranges from the filter's
// support, the argument checks of the entry points and the choice of a kernel's 16-byte variants.
#pragma once
#include "rpde_internal.h"

#include <cmath>
#include <type_traits>

namespace rpde {

// one band on the device: row i reads  weights[i * taps + t] * src[span[i].x + t],  t < span[i].y  (taps: row stride,
// a multiple of 4, zero padded)
struct CnoBand {
  const int2* span;
  const float* w;
  int taps;
};

// sum_t w[t] * src[t], t < cnt, in tap order; the weights come as 16-byte loads (rows are padded to whole float4s), the
// padding taps are never multiplied: what lies behind a staged segment is not ours to read into a sum
__device__ __forceinline__ float band_dot(const float* __restrict__ w, const float* src, int cnt) {
  float acc = 0.f;
  for (int t = 0; t < cnt; t += 4) {
    const float4 wv = *reinterpret_cast<const float4*>(w + t);
    acc = fmaf(wv.x, src[t], acc);
    if (t + 1 < cnt) acc = fmaf(wv.y, src[t + 1], acc);
    if (t + 2 < cnt) acc = fmaf(wv.z, src[t + 2], acc);
    if (t + 3 < cnt) acc = fmaf(wv.w, src[t + 3], acc);
  }
  return acc;
}

// [lo, hi) read by rows [r_lo, r_hi) of a band (starts and ends are monotone in the row), clipped to [0, n)
__device__ __forceinline__ void band_range(const CnoBand& b, int r_lo, int r_hi, int n, int& lo, int& hi) {
  if (r_hi <= r_lo) { lo = hi = 0; return; }
  const int2 first = b.span[r_lo], last = b.span[r_hi - 1];
  lo = min(max(first.x, 0), n);
  hi = min(max(last.x + last.y, lo), n);
}

// ---- host ---------------------------------------------------------------------------------------------------------
// Bounds from the filter of an na -> nb resampling (scale = na / nb, support = 2 max(scale, 1), centres scale (i + 1/2),
// indices truncated): the sources that L consecutive outputs read, and the outputs that read L consecutive sources
inline int cno_sources(int L, int na, int nb) {
  const double sc = (double)na / nb, sup = 2.0 * (sc >= 1.0 ? sc : 1.0);
  const double v = floor(sc * (L - 1) + 2.0 * sup) + 3.0;
  return v < na ? (int)v : na;
}
inline int cno_readers(int L, int na, int nb) {
  const double sc = (double)na / nb, sup = 2.0 * (sc >= 1.0 ? sc : 1.0);
  const double v = floor((L + 2.0 * sup) / sc) + 3.0;
  return v < nb ? (int)v : nb;
}

// the checks of one axis: n_in -> n_mid -> n_out (the 2-D entries run them once per axis)
inline int cno_check(const char* what, const void* x, const void* scale, const void* shift, int B, int C, int n_in,
                     int n_mid, int n_out, float slope) {
  RPDE_CHECK_ARG(x, "%s: null tensor", what);
  RPDE_CHECK_ARG(B > 0 && C > 0 && n_in > 0 && n_mid > 0 && n_out > 0, "%s: bad sizes B=%d C=%d n_in=%d n_mid=%d n_out=%d",
                 what, B, C, n_in, n_mid, n_out);
  RPDE_CHECK_ARG((scale == nullptr) == (shift == nullptr), "%s: scale and shift come together", what);
  RPDE_CHECK_ARG((long)B * C < (1L << 24) && n_in < (1 << 24) && n_mid < (1 << 24) && n_out < (1 << 24),
                 "%s: tensor too large (B*C, n_in, n_mid, n_out must stay below 2^24)", what);
  RPDE_CHECK_ARG(slope == slope, "%s: slope is NaN", what);
  return RPDE_OK;
}

// the checks of one table an entry point was handed, and the band the device sees
inline int cno_band(const char* what, const char* name, const int32_t* span, const float* w, int taps, CnoBand& band) {
  RPDE_CHECK_ARG(span && w, "%s: null %s table", what, name);
  RPDE_CHECK_ARG(taps >= 4 && taps % 4 == 0 && al16(w) && (reinterpret_cast<uintptr_t>(span) & 7) == 0,
                 "%s: %s table: taps %d must be a positive multiple of 4, weights 16-byte and spans 8-byte aligned", what,
                 name, taps);
  band = CnoBand{reinterpret_cast<const int2*>(span), w, taps};
  return RPDE_OK;
}

// launch(VX, VO) with the two run-time flags as compile-time constants (std::true_type / std::false_type): the
// activation kernels are templates on whether the n_in-long and the n_out-long tensors take 16-byte accesses
template <class Launch>
inline void cno_vec_dispatch(bool vx, bool vo, const Launch& launch) {
  if (vx && vo) launch(std::true_type{}, std::true_type{});
  else if (vx) launch(std::true_type{}, std::false_type{});
  else if (vo) launch(std::false_type{}, std::true_type{});
  else launch(std::false_type{}, std::false_type{});
}

}  // namespace rpde
