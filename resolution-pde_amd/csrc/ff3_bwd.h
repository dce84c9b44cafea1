// Device pieces of the fused FeedForward backward that the chain kernel (k_ff3_bwd_h2, ff_fused.hip) and the split pair
// (k_ffs_adjoint / k_ffs_layer1, ff_bwd_split.hip) share.  The two paths must give the same bits for dz3, du2, du1 and the
// five small gradients: what decides those bits stands here once.  How a kernel moves its data (asm or plain LDS
// accesses, registers or LDS-DMA, its waits) stays with the kernel.
//
// Roles, per tile of 32 points and workgroup of eight waves (w = wave, l = lane, g = l >> 4, li = l & 15): in the adjoint
// one POINT per 16-lane row (point 4 w + g of the tile), lane li on features 4 li .. 4 li + 3; in the transposed products
// wave w owns hidden rows 32 w .. 32 w + 31, accumulator tile (blk, t) = rows 16 (2 w + t) + 4 g .. + 3 of point 16 blk + li
#pragma once
#include "ff_fused.h"
#include "h2.h"
#include "pointwise.h"

namespace rpde {

// ---- the weight image of k_ff3_prep_bwd: this lane's 16 bytes of fragment f (0..3 W3^T, 4..19 W2^T), hi or lo piece ----
__device__ __forceinline__ const char* ff3_img_lane(const char* wimg, int w, int l) { return wimg + (long)w * FF3_WAVE_IMG + l * 16; }
__device__ __forceinline__ f16x8 ff3_img_frag(const char* lane_base, int f, int lo) {
  return *reinterpret_cast<const f16x8*>(lane_base + f * 2048 + lo * 1024);
}

// ---- prologue: gamma[64] | beta[64] (1 / 0 where the layer has none) and `nacc` zeroed sums in LDS ----
template <int THREADS>
__device__ __forceinline__ void ff3_bwd_stage_vec(float* vecw, const float* gamma, const float* beta, float* accw, int nacc, int tid) {
  for (int i = tid; i < 128; i += THREADS) vecw[i] = i < 64 ? (gamma ? gamma[i] : 1.f) : (beta ? beta[i - 64] : 0.f);
  for (int i = tid; i < nacc; i += THREADS) accw[i] = 0.f;
}

// ---- last-layer adjoint of one point on a 16-lane row: dropout, LayerNorm, post-activation ----
// A: the kernel's arguments (layer_norm, eps, post_act, drop2 resolved); g4 / z4: the row's grad_out and z3 (.x .. .w);
// pt3: the point, live3: whether it exists.  fetch(gmv, btv) brings gamma / beta of features feat .. feat + 3 into
// registers; it is called inside the LayerNorm branch, behind the statistics (the chain reads them by asm there: an
// ordinary read costs it a vmcnt(0)).  Out: dz[4] = this lane's dz3, dzb = a bound of the point's |dz3| (in every lane
// of the row), dgm / dbt = the point's terms of dgamma / dbeta (zero without LayerNorm).
template <class Args, class V4, class Fetch>
__device__ __forceinline__ void ff3_last_adjoint(const Args& A, const V4 g4, const V4 z4, long pt3, bool live3, int feat, Fetch&& fetch,
                                                 float (&dz)[4], float& dzb, float (&dgm)[4], float (&dbt)[4]) {
  float s4[4] = {1.f, 1.f, 1.f, 1.f};
  if (A.drop2.on()) drop_scale4(A.drop2, (uint64_t)(pt3 * 64 + feat), s4);
  const float tz[4] = {z4.x * s4[0], z4.y * s4[1], z4.z * s4[2], z4.w * s4[3]};
  float gy[4] = {g4.x, g4.y, g4.z, g4.w};
  if (!live3) { gy[0] = gy[1] = gy[2] = gy[3] = 0.f; }
#pragma unroll
  for (int k = 0; k < 4; ++k) dgm[k] = dbt[k] = 0.f;
  if (A.layer_norm) {
    const float mean = row_all16<false>((tz[0] + tz[1]) + (tz[2] + tz[3])) * (1.f / 64.f);
    const float m2 = row_all16<false>((tz[0] - mean) * (tz[0] - mean) + (tz[1] - mean) * (tz[1] - mean) +
                                      (tz[2] - mean) * (tz[2] - mean) + (tz[3] - mean) * (tz[3] - mean));
    const float rstd = rsqrtf(m2 * (1.f / 64.f) + A.eps);
    float gmv[4], btv[4];
    fetch(gmv, btv);
    float xh[4], dxh[4], s1 = 0.f, s2 = 0.f, am = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      xh[k] = (tz[k] - mean) * rstd;
      float dy = gy[k];
      if (A.post_act) dy *= dact_f(A.post_act, xh[k] * gmv[k] + btv[k]);
      dgm[k] = dy * xh[k];
      dbt[k] = dy;
      dxh[k] = dy * gmv[k];
      s1 += dxh[k];
      s2 += dxh[k] * xh[k];
      am = fmaxf(am, fabsf(dxh[k]));
    }
    const float S1 = row_all16<false>(s1) * (1.f / 64.f), S2 = row_all16<false>(s2) * (1.f / 64.f);
    const float AM = row_all16<true>(am);
#pragma unroll
    for (int k = 0; k < 4; ++k) dz[k] = rstd * (dxh[k] - S1 - xh[k] * S2) * s4[k];
    // bound of this POINT's |dz3|: |xhat| <= sqrt(63) < 8
    dzb = rstd * (AM + fabsf(S1) + 8.f * fabsf(S2)) * A.drop2.scale;
  } else {
    float am = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) { dz[k] = gy[k] * dact_f(A.post_act, tz[k]) * s4[k]; am = fmaxf(am, fabsf(dz[k])); }
    dzb = row_all16<true>(am);
  }
}

// ---- bias / gamma / beta gradients: the sums over the wave's four points (rows), in registers, the same in every row;
// the row with g == 0 adds them to the wave's [64] accumulators (per kernel), which ff3_part_out combines in fixed order
__device__ __forceinline__ void ff3_rows_sum(bool live3, bool layer_norm, const float (&dz)[4], float (&b)[4], float (&dgm)[4], float (&dbt)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    b[k] = live3 ? dz[k] : 0.f;
    b[k] += lane_xor16(b[k]); b[k] += lane_xor32(b[k]);
    if (layer_norm) {
      dgm[k] += lane_xor16(dgm[k]); dgm[k] += lane_xor32(dgm[k]);
      dbt[k] += lane_xor16(dbt[k]); dbt[k] += lane_xor32(dbt[k]);
    }
  }
}

// ---- dz3 of a tile as B fragments, 8 KB: [2 blk][2 ks][hi | lo][1 KB], one scale per point (its bound dzb) ----
// Features 4 li .. 4 li + 3 of point ptl are reduction slots 4 (li >> 2 & 1) .. + 3 of lane group li & 3 in the fragment
// (block ptl >> 4, half ks = li >> 3), point column ptl & 15.
// The 16-byte unit of fragment lane (c, p) = (li & 3, ptl & 15) sits at unit 16 c + (p ^ c ^ 4 ks) of its 1 KB piece:
// written plainly at 16 c + p, the sixteen lanes of a row -- same p, four c, two ks, 256 / 2048 bytes apart -- hit two
// banks (8-way conflicts: 29.4 M conflict cycles per launch in round 3's counters); permuted inside each 256-byte row they
// cover all 32.  The reader un-permutes its address; its own banking only sees a row's units in another order.
__device__ __forceinline__ void ff3_dz_split(const float (&dz)[4], float dzb, uint2& hi, uint2& lo) {
  float sdz, sdzi;
  h2_scale(dzb, 0, sdz, sdzi);
  h2_split4(dz[0] * sdz, dz[1] * sdz, dz[2] * sdz, dz[3] * sdz, hi, lo);
}
// writer: byte offset of the hi piece of (point ptl, lane li); the lo piece is 1 KB on
__device__ __forceinline__ int ff3_dz_off(int ptl, int li) {
  const int ksz = li >> 3, cz = li & 3;
  return (((ptl >> 4) * 2 + ksz) * 2) * 1024 + (cz * 16 + ((ptl & 15) ^ cz ^ (4 * ksz))) * 16 + ((li >> 2) & 1) * 8;
}
// reader: lane l's operands of the two k-steps of point block blk
__device__ __forceinline__ void ff3_dz_frags(const char* buf, int blk, int l, f16x8& zh0, f16x8& zl0, f16x8& zh1, f16x8& zl1) {
  const int zu = (l & 48) | ((l & 15) ^ (l >> 4));             // this lane's unit in the ks = 0 pieces; ks = 1: ^ 4
  const char* zb = buf + (blk * 2) * 2048;
  zh0 = *reinterpret_cast<const f16x8*>(zb + zu * 16); zl0 = *reinterpret_cast<const f16x8*>(zb + 1024 + zu * 16);
  zh1 = *reinterpret_cast<const f16x8*>(zb + 2048 + (zu ^ 4) * 16); zl1 = *reinterpret_cast<const f16x8*>(zb + 3072 + (zu ^ 4) * 16);
}

// ---- the bound chain: a point's scales follow from the bound bz of its |dz3| alone, recomputed at each use ----
// dz3 was scaled by bz's power of two: the factor that takes a (W3^T . dz3) accumulator back
__device__ __forceinline__ float ff3_inv_dz3(float bz, float winv3) {
  float a, ai;
  h2_scale(bz, 0, a, ai);
  return ai * winv3;
}
// |du2| <= c3t bz dmax (c3t: the largest column L1 norm of W3, dmax: bound of |gelu'| times the dropout scale): the scale
// du2 is staged under, and the factor that takes a (W2^T . du2) accumulator back
__device__ __forceinline__ void ff3_scale_du2(float bz, float c3t, float dmax, float winv2, float& s_du2, float& inv_b) {
  float ai;
  h2_scale(c3t * bz * dmax, 0, s_du2, ai);
  inv_b = ai * winv2;
}

// ---- one accumulator tile of du = (W^T . dz) * d: u[r] = acc[r] * inv * d[r], stored, and the bias sums bsum[r] += u[r] ----
// The two bias gradients round differently, and both kernels of each have to agree, so the rounding is stated and not
// left to the compiler's choice of contraction (which went one way in the chain and the other way in the split):
//   FMA = false (db2): the ROUNDED products are added;
//   FMA = true  (db1): the last multiplication is fused into the addition, bsum = fma(acc * inv, d, bsum).
// live: the point exists -- its four values go to dst (this lane's place in du) and into the sums.  (k_ffs_layer1 keeps
// the FMA form written out: called from there, this function costs it two registers and scratch.)
template <bool FMA>
__device__ __forceinline__ void ff3_du_tile(const f32x4v& acc, float inv, const float4& d4, bool live, float* dst, float (&u)[4], float* bsum) {
  const float d[4] = {d4.x, d4.y, d4.z, d4.w};
  float s[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { s[r] = acc[r] * inv; u[r] = s[r] * d[r]; }
  if (!FMA) {
#pragma unroll
    for (int r = 0; r < 4; ++r) pin(u[r]);
  }
  if (live) {
    *reinterpret_cast<float4*>(dst) = make_float4(u[0], u[1], u[2], u[3]);
#pragma unroll
    for (int r = 0; r < 4; ++r) bsum[r] = FMA ? __builtin_fmaf(s[r], d[r], bsum[r]) : bsum[r] + u[r];
  }
}
// the eight bias sums of a wave's tile, summed over the 16 points of a row of lanes (valid in lane 15 of each row), and
// the hidden row that sum i of lane group g belongs to; lane 15 adds them to the workgroup's [256] accumulator in the
// kernel (written there: as part of this function the addition costs k_ffs_adjoint an instruction per tile)
__device__ __forceinline__ void ff3_bias_rows(float (&bsum)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) bsum[i] = row_sum15(bsum[i]);
}
__device__ __forceinline__ int ff3_bias_row(int w, int g, int i) { return 16 * (2 * w + (i >> 2)) + 4 * g + (i & 3); }

// ---- per-workgroup sums out: entries FIRST .. LAST - 1 of this workgroup's FF3_PART (db1[256] db2[256] db3[64]
// dgamma[64] dbeta[64]).  acc: the plain sums, acc[0] being entry FIRST; acc_w8: db3 | dgamma | dbeta as [3][8 wave][64],
// the eight waves' sums combined in wave order ----
template <int FIRST, int LAST, int THREADS>
__device__ __forceinline__ void ff3_part_out(float* part, const float* acc, const float* acc_w8, int tid) {
  for (int i = FIRST + tid; i < LAST; i += THREADS) {
    float v;
    if (LAST <= 512 || i < 512) v = acc[i - FIRST];
    else {
      const float* a8 = acc_w8 + ((i - 512) >> 6) * 512 + ((i - 512) & 63);
      v = 0.f;
#pragma unroll
      for (int ww = 0; ww < 8; ++ww) v += a8[ww * 64];
    }
    part[i] = v;
  }
}

}  // namespace rpde
