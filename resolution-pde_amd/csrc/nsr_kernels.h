// What the equation residuals of the two Navier-Stokes generators share (ns_residual.hip: the vorticity equation;
// nsc_residual.hip: the active-scalar system): the separable float64 analysis of a batch of fields -- rows, then
// columns -- with its workspace piece, and the last kernel of the backward.  The kernels are those ns_residual.hip was
// written with, moved here as they stood.
#pragma once
#include "ns_kernels.h"
#include "rel_loss.h"

namespace rpde {

// grid (blocks over K, blocks of RY rows, B): R[b][y][k] = sum_j z[b][y][j] tw_N[j k mod N], RY rows y of z = x~ (p null)
// or of z = d = p~ - x~ decoded into LDS in float64 (d is never rounded to fp32); a thread owns one k for the RY rows, so a
// root of unity gathered once serves 2 RY multiply-adds.  TW: the N roots sit in LDS as well (N <= NSR_TW_MAX).
// Dynamic LDS: row[RY][N] doubles, then tw[N] double2
constexpr int NSR_TW_MAX = 1024;
template <int RY, bool TW>
__global__ __launch_bounds__(256) void k_nsr_rows(const float* __restrict__ x, const float* __restrict__ p,
                                                  const double2* __restrict__ twN, double2* __restrict__ R, HalfSpec g,
                                                  RelAffine a) {
  extern __shared__ double nsr_lds[];
  double* __restrict__ row = nsr_lds;
  const double2* __restrict__ tw = twN;
  const int b = blockIdx.z, y0 = blockIdx.y * RY, k = blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (TW) {
    double2* t = reinterpret_cast<double2*>(nsr_lds + (long)RY * g.N);
    for (int j = threadIdx.x; j < g.N; j += blockDim.x) t[j] = twN[j];
    tw = t;
  }
#pragma unroll
  for (int r = 0; r < RY; ++r) {
    const bool in = y0 + r < g.M;
    const long at = ((long)b * g.M + y0 + r) * g.N;
    for (int j = threadIdx.x; j < g.N; j += blockDim.x) {
      double v = 0.0;
      if (in) {
        const double xt = fma((double)a.ax, (double)x[at + j], (double)a.bx);
        v = p ? fma((double)a.ap, (double)p[at + j], (double)a.bp) - xt : xt;
      }
      row[r * g.N + j] = v;
    }
  }
  __syncthreads();
  if (k >= g.K) return;
  double sr[RY], si[RY];
#pragma unroll
  for (int r = 0; r < RY; ++r) { sr[r] = 0.0; si[r] = 0.0; }
  int idx = 0;                         // j k mod N
#pragma unroll 4
  for (int j = 0; j < g.N; ++j) {
    const double2 w = tw[idx];
    idx += k;
    if (idx >= g.N) idx -= g.N;
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      const double v = row[r * g.N + j];
      sr[r] = fma(v, w.x, sr[r]);
      si[r] = fma(v, w.y, si[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < RY; ++r)
    if (y0 + r < g.M) R[((long)b * g.M + y0 + r) * g.K + k] = make_double2(sr[r], si[r]);
}

// block (64 kx, 4 groups of NSR_KY rows ky), grid (blocks over kp, blocks over M, B):
// X[b][ky][kx] = sum_y R[b][y][kx] tw_M[y ky mod M], a thread owns one kx for NSR_KY rows ky so that one load of R serves
// 4 NSR_KY multiply-adds (8 where that leaves the card enough blocks, else 2); the M roots sit in LDS where M <=
// NSR_TW_MAX.  Into the float64 spectrum Xd and (unless null) its fp32 copy X32, both [B][M][re|im][kp] with the padded
// columns zero.  Every sum runs in index order whatever NSR_KY and RY: the bits do not depend on the choice
template <int NSR_KY>
__global__ __launch_bounds__(256) void k_nsr_cols(const double2* __restrict__ R, const double2* __restrict__ twG,
                                                  double* __restrict__ Xd, float* __restrict__ X32, HalfSpec g) {
  __shared__ double2 twl[NSR_TW_MAX];
  const double2* __restrict__ twM = twG;
  if (g.M <= NSR_TW_MAX) {
    for (int j = threadIdx.y * 64 + threadIdx.x; j < g.M; j += 256) twl[j] = twG[j];
    __syncthreads();
    twM = twl;
  }
  const int b = blockIdx.z, ky0 = (blockIdx.y * 4 + threadIdx.y) * NSR_KY, kx = blockIdx.x * 64 + threadIdx.x;
  if (ky0 >= g.M || kx >= g.kp) return;
  double sr[NSR_KY], si[NSR_KY];
  int idx[NSR_KY], step[NSR_KY];       // y ky mod M; a row past M steps by 0 and is not stored
#pragma unroll
  for (int i = 0; i < NSR_KY; ++i) { sr[i] = 0.0; si[i] = 0.0; idx[i] = 0; step[i] = ky0 + i < g.M ? ky0 + i : 0; }
  if (kx < g.K) {
    const double2* __restrict__ Rb = R + (long)b * g.M * g.K + kx;
#pragma unroll 2
    for (int y = 0; y < g.M; ++y) {
      const double2 r = Rb[(long)y * g.K];
#pragma unroll
      for (int i = 0; i < NSR_KY; ++i) {
        const double2 w = twM[idx[i]];
        idx[i] += step[i];
        if (idx[i] >= g.M) idx[i] -= g.M;
        sr[i] = fma(r.x, w.x, fma(-r.y, w.y, sr[i]));
        si[i] = fma(r.x, w.y, fma(r.y, w.x, si[i]));
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NSR_KY; ++i) {
    if (ky0 + i >= g.M) break;
    const long ore = ((long)b * g.M + ky0 + i) * 2 * g.kp + kx, oim = ore + g.kp;
    Xd[ore] = sr[i];         Xd[oim] = si[i];
    if (X32) { X32[ore] = (float)sr[i]; X32[oim] = (float)si[i]; }
  }
}

// grid (blocks, B): grad_p = a_p coef_b z, coef_b the family's rel_coef; n4 float4 groups per sample
static __global__ __launch_bounds__(256) void k_nsr_grad(const float* __restrict__ z, const float* __restrict__ stats,
                                                  const float* __restrict__ grad_loss, const float* __restrict__ grad_rel,
                                                  float* __restrict__ grad_p, int B, int n4, int size_average, float ap) {
  const int b = blockIdx.y;
  const float scale = ap * rel_coef(stats, grad_loss, grad_rel, b, B, size_average);
  const float* __restrict__ zb = z + (long)b * 4 * n4;
  float* __restrict__ gb = grad_p + (long)b * 4 * n4;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
    float v[4];
    ld4(zb + 4 * i, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] *= scale;
    st4(gb + 4 * i, v);
  }
}

// the float64 analysis: the roots of unity of both axes and the row spectra (double2 both)
struct NsrSpecWork {
  double2 *tw, *R;
  NsrSpecWork(Arena& ar, int B, int M, int N)
      : tw(reinterpret_cast<double2*>(ar.take((size_t)4 * (N + M)))),
        R(reinterpret_cast<double2*>(ar.take((size_t)4 * B * M * (N / 2 + 1)))) {}
};

// the float64 spectrum of x~ (p null) or of p~ - x~, rows then columns, after rel_roots(w.tw, N, M) on the same stream
static int nsr_spectrum(const float* x, const float* p, const NsrSpecWork& w, double* Xd, float* X32, const HalfSpec& g,
                        RelAffine a, hipStream_t st) {
  // the wider kernels where they still leave the card a few blocks per CU
  const int rb = g.K >= 256 ? 256 : (g.K + 63) / 64 * 64;
  const long xb = (g.K + rb - 1) / rb, cb = (g.kp + 63) / 64;
  const bool wide_rows = xb * ((g.M + 3) / 4) * g.images >= 512, wide_cols = cb * ((g.M + 31) / 32) * g.images >= 512;
  if (g.N > NSR_TW_MAX) {
    hipLaunchKernelGGL((k_nsr_rows<1, false>), dim3(xb, g.M, g.images), dim3(rb), (size_t)g.N * 8, st, x, p, w.tw, w.R, g, a);
  } else if (wide_rows) {
    hipLaunchKernelGGL((k_nsr_rows<4, true>), dim3(xb, (g.M + 3) / 4, g.images), dim3(rb), (size_t)g.N * (4 * 8 + 16), st, x, p, w.tw, w.R, g, a);
  } else {
    hipLaunchKernelGGL((k_nsr_rows<1, true>), dim3(xb, g.M, g.images), dim3(rb), (size_t)g.N * (8 + 16), st, x, p, w.tw, w.R, g, a);
  }
  RPDE_LAUNCH_CHECK();
  if (wide_cols) {
    hipLaunchKernelGGL(k_nsr_cols<8>, dim3(cb, (g.M + 31) / 32, g.images), dim3(64, 4), 0, st, w.R, w.tw + g.N, Xd, X32, g);
  } else {
    hipLaunchKernelGGL(k_nsr_cols<2>, dim3(cb, (g.M + 7) / 8, g.images), dim3(64, 4), 0, st, w.R, w.tw + g.N, Xd, X32, g);
  }
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

}  // namespace rpde
