// What the Darcy generator (darcy.hip) and its equation residual (darcy_residual.hip) share: the grid limits, the
// per-sample partial sums, the finite-volume operator on one 16-byte group of a row and the separable product.
#pragma once
#include "halfspec.h"

namespace rpde {

constexpr int DARCY_MIN_S = 8, DARCY_MAX_S = 512;

inline bool darcy_dims_ok(int B, int s) {
  return B >= 1 && B <= 65535 && s >= DARCY_MIN_S && s <= DARCY_MAX_S && s % 4 == 0;
}
#define DARCY_CHECK_DIMS(what, B, s)                                                                                  \
  RPDE_CHECK_ARG(darcy_dims_ok(B, s), what ": bad B=%d s=%d (s a multiple of 4, %d .. %d, 1 <= B <= 65535)", B, s, \
                 DARCY_MIN_S, DARCY_MAX_S)

// the sum of n partials, lane-strided then across the wave: every wave of every block of the sample computes the same bits
__device__ __forceinline__ double darcy_fold(const double* __restrict__ part, int n) {
  double acc = 0.0;
  for (int i = threadIdx.x & 63; i < n; i += 64) acc += part[i];
  return wave_sum(acc);
}
// the block's sum to part[blockIdx.x] (256 threads, four waves added in order)
__device__ __forceinline__ void darcy_block_partial(float v, double* __restrict__ part) {
  __shared__ double sh[4];
  const double w = wave_sum((double)v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
__device__ __forceinline__ bool darcy_pos_finite(double v) { return v > 0.0 && v < INFINITY; }
__device__ __forceinline__ float darcy_hmean(float x, float y) { return (2.f * x * y) / (x + y); }

// how darcy_row4 reads its two fields: as they stand (the generator), or through an affine map applied to every value
// it loads, halo included (the residual's decode of an encoded coefficient and prediction)
struct DarcyPlain {
  __device__ __forceinline__ float a(float v) const { return v; }
  __device__ __forceinline__ float u(float v) const { return v; }
};
struct DarcyDecode {
  float ka, ba, ku, bu;
  __device__ __forceinline__ float a(float v) const { return fmaf(ka, v, ba); }
  __device__ __forceinline__ float u(float v) const { return fmaf(ku, v, bu); }
};

// (A u) of the four cells (i, j0 .. j0+3) of one sample, difference form
template <class Map = DarcyPlain>
__device__ __forceinline__ void darcy_row4(const float* __restrict__ a, const float* __restrict__ u, int s, int i, int j0,
                                           float s2, float (&out)[4], const Map map = Map()) {
  const long o = (long)i * s + j0;
  const bool hw = j0 > 0, he = j0 + 4 < s, hn = i > 0, hs = i + 1 < s;
  float ac[4], uc[4], an[4] = {0.f, 0.f, 0.f, 0.f}, un[4] = {0.f, 0.f, 0.f, 0.f}, as[4] = {0.f, 0.f, 0.f, 0.f},
                      us[4] = {0.f, 0.f, 0.f, 0.f};
  const auto lda = [&](const float* p, float (&v)[4]) {
    ld4(p, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = map.a(v[j]);
  };
  const auto ldu = [&](const float* p, float (&v)[4]) {
    ld4(p, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = map.u(v[j]);
  };
  lda(a + o, ac);
  ldu(u + o, uc);
  if (hn) { lda(a + o - s, an); ldu(u + o - s, un); }
  if (hs) { lda(a + o + s, as); ldu(u + o + s, us); }
  const float aw = hw ? map.a(a[o - 1]) : 0.f, uw = hw ? map.u(u[o - 1]) : 0.f;
  const float ae = he ? map.a(a[o + 4]) : 0.f, ue = he ? map.u(u[o + 4]) : 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool l = j > 0 || hw, r = j < 3 || he;
    const float al = j > 0 ? ac[j - 1] : aw, ul = j > 0 ? uc[j - 1] : uw;
    const float ar = j < 3 ? ac[j + 1] : ae, ur = j < 3 ? uc[j + 1] : ue;
    const float c = ac[j], two_c = 2.f * c, v = uc[j];
    const float wl = l ? darcy_hmean(c, al) : two_c, wr = r ? darcy_hmean(c, ar) : two_c;
    const float wn = hn ? darcy_hmean(c, an[j]) : two_c, ws = hs ? darcy_hmean(c, as[j]) : two_c;
    float acc = wl * (v - (l ? ul : 0.f));
    acc = fmaf(wr, v - (r ? ur : 0.f), acc);
    acc = fmaf(wn, v - (hn ? un[j] : 0.f), acc);
    acc = fmaf(ws, v - (hs ? us[j] : 0.f), acc);
    out[j] = s2 * acc;
  }
}

// out_b = op(L) in_b op(R)^T over B images [s, s]: cf_rowdft with the shared table for the left factor (into tmp), one GEMM
// over [B s, s] for the right one.  lt / rt: the table is stored transposed (op(X) = X^T)
inline int sep2d(const float* in, const float* L, bool lt, const float* R, bool rt, float* tmp, float* out, int B, int s,
                 hipStream_t st) {
  RPDE_TRY(cf_rowdft(L, s, lt, s, s, in, tmp, B, s, st));
  rpde_gemm_desc d = gemm_desc();
  d.A = tmp; d.a_kmajor = 1; d.lda = s;
  d.B = R; d.b_kmajor = rt ? 0 : 1; d.ldb = s;
  d.C = out; d.ldc = s;
  d.M = B * s; d.N = s; d.K = s;
  return launch_gemm(d, st);
}

}  // namespace rpde
