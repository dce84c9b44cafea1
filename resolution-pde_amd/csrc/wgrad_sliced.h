// The deterministic weight and bias gradient of the small convolutions, written once: Conv(k = 3, padding = 1)
// (cno_layers.hip) and ConvTranspose(kernel_size = 2, stride = 2) (unet.hip), both ranks of each.  The two are
// transposes of each other.  Per point p = (b, y, x) one operand is narrow, one value per channel, and the other wide,
// Op::T values per channel (the taps), and the gradient is  gw[narrow][wide][t] = sum_p narrow[p] wide[p][t]:
//   Conv:           narrow = g[co], wide = the 3 KY shifted taps of x[ci],  gw [Cout][Cin][T]
//   ConvTranspose:  narrow = x[ci], wide = the 2 KY taps of g[co],          gw [Cin][Cout][T]
// and gb[co] is the sum of g, wherever it stands.  A workgroup owns a 4 x 4 tile of (ci, co) = (blockIdx.x, blockIdx.y)
// and one slice of the points: every thread walks the slice's points tid, tid + 256, ... with 16 T + 4 accumulators,
// then the workgroup adds them up in a fixed order (DPP sum inside a wave, the four waves in sequence).  With one slice
// the sums are the result; with more they are partial sums [slice][Cin Cout T + Cout], which one fold launch adds in a fixed
// order (pointwise.h).  No atomics.  DESIGN.md 10.19.
//
// An Op is constructed from (H, W, the slice's first point) and supplies
//   T, G_NARROW        the taps per channel pair; whether g is the narrow operand (then co = blockIdx.y is the narrow
//                      channel and the bias sums the narrow values, else ci = blockIdx.x and the bias sums the wide ones)
//   seek(i)            decode point i of the slice (an offset, known to be non-negative: index arithmetic on the
//                      absolute point would carry sign checks into every bounds test of the taps)
//   narrow(src, C, ch) the narrow operand's value of channel ch at the point (0 past the last channel)
//   wide(src, C, ch, v) v[t] = the wide operand's taps (0 past the last channel and outside the plane)
#pragma once
#include "pointwise.h"
#include "rpde_internal.h"
#include "wave.h"

#include <algorithm>

namespace rpde {

constexpr int WG_TILE = 4;
constexpr int WG_TARGET = 512;        // workgroups wanted: two per CU
constexpr int WG_MIN_POINTS = 256;    // a slice holds at least one point per thread

template <class Op>
__global__ void __launch_bounds__(256)
k_wgrad_sliced(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ gw, float* __restrict__ gb,
               long slice_stride, long NP, int Cin, int Cout, int H, int W, long points_per_slice) {
  constexpr int T = Op::T, N_GW = WG_TILE * WG_TILE * T;
  constexpr bool G_NARROW = Op::G_NARROW;
  __shared__ float red[4][N_GW + WG_TILE];
  const float* __restrict__ nsrc = G_NARROW ? g : x;
  const float* __restrict__ wsrc = G_NARROW ? x : g;
  const int Cn = G_NARROW ? Cout : Cin, Cw = G_NARROW ? Cin : Cout;
  const int co0 = blockIdx.y * WG_TILE;
  const int n0 = G_NARROW ? co0 : blockIdx.x * WG_TILE, w0 = G_NARROW ? blockIdx.x * WG_TILE : co0;
  const long p_lo = blockIdx.z * points_per_slice, p_hi = p_lo + points_per_slice < NP ? p_lo + points_per_slice : NP;
  float acc[WG_TILE][WG_TILE][T], bsum[WG_TILE];
#pragma unroll
  for (int i = 0; i < WG_TILE; ++i) {
    bsum[i] = 0.f;
#pragma unroll
    for (int j = 0; j < WG_TILE; ++j)
#pragma unroll
      for (int t = 0; t < T; ++t) acc[i][j][t] = 0.f;
  }
  Op op(H, W, p_lo);
  for (long at = threadIdx.x; at < p_hi - p_lo; at += 256) {
    op.seek(at);
    float nv[WG_TILE];
#pragma unroll
    for (int i = 0; i < WG_TILE; ++i) {
      nv[i] = op.narrow(nsrc, Cn, n0 + i);
      if (G_NARROW) bsum[i] += nv[i];
    }
#pragma unroll
    for (int j = 0; j < WG_TILE; ++j) {
      float wv[T];
      op.wide(wsrc, Cw, w0 + j, wv);
      if (!G_NARROW) {
#pragma unroll
        for (int t = 0; t < T; ++t) bsum[j] += wv[t];
      }
#pragma unroll
      for (int i = 0; i < WG_TILE; ++i)
#pragma unroll
        for (int t = 0; t < T; ++t) acc[i][j][t] = fmaf(nv[i], wv[t], acc[i][j][t]);
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < WG_TILE; ++i) {
#pragma unroll
    for (int j = 0; j < WG_TILE; ++j)
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const float v = wave_sum_dpp(acc[i][j][t]);
        if (lane == 0) red[wave][(i * WG_TILE + j) * T + t] = v;
      }
    const float v = wave_sum_dpp(bsum[i]);
    if (lane == 0) red[wave][N_GW + i] = v;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < N_GW + WG_TILE) {
    const float v = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    if (k < N_GW) {
      const int i = k / (WG_TILE * T), j = (k / T) % WG_TILE, t = k % T;
      if (n0 + i < Cn && w0 + j < Cw) gw[blockIdx.z * slice_stride + ((long)(n0 + i) * Cw + w0 + j) * T + t] = v;
    } else if (gb && blockIdx.x == 0 && co0 + (k - N_GW) < Cout) {
      gb[blockIdx.z * slice_stride + co0 + k - N_GW] = v;
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------
// Slices the points are split over, in whole units (an image row for the convolution, a point for the transposed one):
// the one place the *_slices queries and the launch take the count from
inline int wgrad_slices(int Cin, int Cout, long units, long points) {
  const long tiles = (long)((Cin + WG_TILE - 1) / WG_TILE) * ((Cout + WG_TILE - 1) / WG_TILE);
  const long n = std::min<long>(WG_TARGET / tiles, std::min<long>(units, points / WG_MIN_POINTS));
  return (int)std::max<long>(1, std::min<long>(n, 65535));
}

// gw, gb (or null) of B H W points in `units` units; `partial` [partial_slices][Cin Cout T + Cout] takes the partial
// sums of more than one slice
template <class Op>
int wgrad_sliced(const char* what, const float* x, const float* g, float* gw, float* gb, int B, int Cin, int Cout, int H,
                 int W, long units, float* partial, int partial_slices, hipStream_t st) {
  const long NP = (long)B * H * W;
  const int slices = wgrad_slices(Cin, Cout, units, NP);
  RPDE_CHECK_ARG(slices == 1 || (partial && partial_slices >= slices),
                 "%s: partial sums of %d slices needed, the buffer holds %d", what, slices, partial ? partial_slices : 0);
  const dim3 grid((unsigned)((Cin + WG_TILE - 1) / WG_TILE), (unsigned)((Cout + WG_TILE - 1) / WG_TILE), (unsigned)slices);
  RPDE_CHECK_ARG(grid.y <= 65535, "%s: too many output channels (%d)", what, Cout);
  const long per_slice = (units + slices - 1) / slices * (NP / units);
  const long n_gw = (long)Op::T * Cin * Cout, n_gb = Cout;
  // one slice: the sums are the result; more: partial sums, then their sum
  float* to_w = slices == 1 ? gw : partial;
  float* to_b = slices == 1 ? gb : partial + n_gw;
  const long stride = slices == 1 ? 0L : n_gw + n_gb;
  hipLaunchKernelGGL(k_wgrad_sliced<Op>, grid, dim3(256), 0, st, x, g, to_w, to_b, stride, NP, Cin, Cout, H, W, per_slice);
  RPDE_LAUNCH_CHECK();
  if (slices == 1) return RPDE_OK;
  FoldJobs folds;
  folds.add(partial, gw, n_gw, slices, n_gw + n_gb);
  if (gb) folds.add(partial + n_gw, gb, n_gb, slices, n_gw + n_gb);
  return fold_jobs(folds, st);
}

}  // namespace rpde
