// The CNO activation (reference models/CNO1d.py:30-45) as one kernel per direction: antialiased bicubic resampling to
// n_mid points, LeakyReLU, antialiased bicubic resampling to n_out points.  Both resamplings are fixed banded linear
// maps (rpde/cno.py builds their tables from torch's rule), so a workgroup stages a row segment with its halo in LDS,
// forms the mid signal there, and writes only the result: x is read once and out written once.
// Below it, the rest of a CNO block: Conv1d(k = 3) as three shifted GEMMs with its own weight-gradient kernel, and the
// two kernels of BatchNorm1d (per-channel moments, per-channel affine combine).  gfx950 (CDNA4, wave64) only.
#include "cno.h"
#include "wave.h"

#include <algorithm>

namespace rpde {

constexpr int CNO_THREADS = 256;
constexpr int CNO_TILE = 1024;        // points of the written tensor per workgroup, halved until the spans below fit
constexpr int CNO_MIN_TILE = 32;      // one 128-byte line
constexpr int CNO_IN_CAP = 1280;      // floats of LDS for the staged input segment(s)
constexpr int CNO_MID_CAP = 2304;     // ... for the mid signal
constexpr int CNO_G_CAP = 1280;       // ... for the staged upstream gradient (backward)
constexpr int CNO_PACK_WORK = 2048;   // mid points per workgroup up to which short rows are packed together

struct CnoShape {
  int rows, C, n_in, n_mid, n_out;
  int tile, ntiles, pack;             // points per tile, tiles per row, rows per workgroup
  int vec_x, vec_o;                   // 16-byte accesses to the n_in-long / n_out-long tensors
  float slope;
};

// rows [r0, r0 + nr) x points [lo, lo + len) of t [rows, n] -> dst [nr][len], scale[c] * v + shift[c] on the way when
// scale is given.  VEC: lo, len and n are multiples of 4 and t is 16-byte aligned
template <bool VEC>
__device__ __forceinline__ void cno_stage(float* dst, const float* __restrict__ t, int r0, int nr, int n, int lo, int len,
                                          const float* __restrict__ scale, const float* __restrict__ shift, int C) {
  if (VEC) {
    const int q = len >> 2;
    for (int idx = threadIdx.x; idx < nr * q; idx += CNO_THREADS) {
      const int r = idx / q, i = (idx - r * q) << 2;
      const long row = r0 + r;
      float4 v = *reinterpret_cast<const float4*>(t + row * n + lo + i);
      if (scale) {
        const float a = scale[row % C], b = shift[row % C];
        v.x = fmaf(a, v.x, b); v.y = fmaf(a, v.y, b); v.z = fmaf(a, v.z, b); v.w = fmaf(a, v.w, b);
      }
      *reinterpret_cast<float4*>(dst + r * len + i) = v;
    }
  } else {
    for (int idx = threadIdx.x; idx < nr * len; idx += CNO_THREADS) {
      const int r = idx / len, i = idx - r * len;
      const long row = r0 + r;
      float v = t[row * n + lo + i];
      if (scale) v = fmaf(scale[row % C], v, shift[row % C]);
      dst[idx] = v;
    }
  }
}

// dst[r0 + r][o0 + i] = sum over band row o0 + i of src[r][..], r < nr, i < len; src holds [nr][slen] from s_lo on
template <bool VEC>
__device__ __forceinline__ void cno_emit(float* __restrict__ dst, int r0, int nr, int n, int o0, int len, const CnoBand& b,
                                         const float* src, int slen, int s_lo) {
  if (VEC) {
    const int q = len >> 2;
    for (int idx = threadIdx.x; idx < nr * q; idx += CNO_THREADS) {
      const int r = idx / q, i = (idx - r * q) << 2;
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int o = o0 + i + k;
        const int2 sp = b.span[o];
        v[k] = band_dot(b.w + (long)o * b.taps, src + r * slen + (sp.x - s_lo), sp.y);
      }
      *reinterpret_cast<float4*>(dst + (long)(r0 + r) * n + o0 + i) = make_float4(v[0], v[1], v[2], v[3]);
    }
  } else {
    for (int idx = threadIdx.x; idx < nr * len; idx += CNO_THREADS) {
      const int r = idx / len, i = idx - r * len, o = o0 + i;
      const int2 sp = b.span[o];
      dst[(long)(r0 + r) * n + o] = band_dot(b.w + (long)o * b.taps, src + r * slen + (sp.x - s_lo), sp.y);
    }
  }
}

// the spans a workgroup stages never exceed what the host sized the tile for (cno_plan below bounds them from the
// filter's support); should a table not follow the rule, the spans are cut to the LDS they have instead of overrun
__device__ __forceinline__ int cno_cut(int len, int nr, int cap, bool vec) {
  const int most = cap / nr;
  len = min(len, most);
  return vec ? len & ~3 : len;
}

template <bool VX, bool VO>
__global__ void __launch_bounds__(CNO_THREADS)
k_cno_act_fwd(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
              float* __restrict__ out, CnoShape s, CnoBand U, CnoBand D) {
  __shared__ __attribute__((aligned(16))) float s_in[CNO_IN_CAP];
  __shared__ __attribute__((aligned(16))) float s_mid[CNO_MID_CAP];
  const int tile = blockIdx.x % s.ntiles, r0 = (blockIdx.x / s.ntiles) * s.pack;
  const int nr = min(s.pack, s.rows - r0);
  const int o0 = tile * s.tile, o1 = min(s.n_out, o0 + s.tile);
  int m_lo, m_hi, x_lo, x_hi;
  band_range(D, o0, o1, s.n_mid, m_lo, m_hi);
  band_range(U, m_lo, m_hi, s.n_in, x_lo, x_hi);
  if (VX) { x_lo &= ~3; x_hi = min(s.n_in, (x_hi + 3) & ~3); }
  const int sx = cno_cut(x_hi - x_lo, nr, CNO_IN_CAP, VX), sm = cno_cut(m_hi - m_lo, nr, CNO_MID_CAP, false);

  cno_stage<VX>(s_in, x, r0, nr, s.n_in, x_lo, sx, scale, shift, s.C);
  __syncthreads();
  for (int idx = threadIdx.x; idx < nr * sm; idx += CNO_THREADS) {
    const int r = idx / sm, m = m_lo + (idx - r * sm);
    const int2 sp = U.span[m];
    const float u = band_dot(U.w + (long)m * U.taps, s_in + r * sx + (sp.x - x_lo), sp.y);
    s_mid[idx] = u > 0.f ? u : s.slope * u;
  }
  __syncthreads();
  cno_emit<VO>(out, r0, nr, s.n_out, o0, o1 - o0, D, s_mid, sm, m_lo);
}

// gy = U^T (lrelu'(u) * D^T g) on the tile [i0, i1) of the input axis: the mid points that touch the tile (UT), their
// pre-activations u = U y recomputed from the staged x with its halo, and D^T g gathered (DT) from the staged g
template <bool VX, bool VO>
__global__ void __launch_bounds__(CNO_THREADS)
k_cno_act_bwd(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
              const float* __restrict__ g, float* __restrict__ gy, CnoShape s, CnoBand U, CnoBand UT, CnoBand DT) {
  __shared__ __attribute__((aligned(16))) float s_in[CNO_IN_CAP];
  __shared__ __attribute__((aligned(16))) float s_g[CNO_G_CAP];
  __shared__ __attribute__((aligned(16))) float s_mid[CNO_MID_CAP];
  const int tile = blockIdx.x % s.ntiles, r0 = (blockIdx.x / s.ntiles) * s.pack;
  const int nr = min(s.pack, s.rows - r0);
  const int i0 = tile * s.tile, i1 = min(s.n_in, i0 + s.tile);
  int m_lo, m_hi, x_lo, x_hi, g_lo, g_hi;
  band_range(UT, i0, i1, s.n_mid, m_lo, m_hi);
  band_range(U, m_lo, m_hi, s.n_in, x_lo, x_hi);
  band_range(DT, m_lo, m_hi, s.n_out, g_lo, g_hi);
  if (VX) { x_lo &= ~3; x_hi = min(s.n_in, (x_hi + 3) & ~3); }
  if (VO) { g_lo &= ~3; g_hi = min(s.n_out, (g_hi + 3) & ~3); }
  const int sx = cno_cut(x_hi - x_lo, nr, CNO_IN_CAP, VX), sg = cno_cut(g_hi - g_lo, nr, CNO_G_CAP, VO);
  const int sm = cno_cut(m_hi - m_lo, nr, CNO_MID_CAP, false);

  cno_stage<VX>(s_in, x, r0, nr, s.n_in, x_lo, sx, scale, shift, s.C);
  cno_stage<VO>(s_g, g, r0, nr, s.n_out, g_lo, sg, nullptr, nullptr, 1);
  __syncthreads();
  for (int idx = threadIdx.x; idx < nr * sm; idx += CNO_THREADS) {
    const int r = idx / sm, m = m_lo + (idx - r * sm);
    const int2 su = U.span[m], sd = DT.span[m];
    const float u = band_dot(U.w + (long)m * U.taps, s_in + r * sx + (su.x - x_lo), su.y);
    const float gm = band_dot(DT.w + (long)m * DT.taps, s_g + r * sg + (sd.x - g_lo), sd.y);
    s_mid[idx] = u > 0.f ? gm : s.slope * gm;
  }
  __syncthreads();
  cno_emit<VX>(gy, r0, nr, s.n_in, i0, i1 - i0, UT, s_mid, sm, m_lo);
}

// ---- host: tile and packing -------------------------------------------------------------------------------------
// fills tile / ntiles / pack of s for a kernel that writes the n_w-long axis; spans(T, sm, sx, sg) bounds what a tile
// of T written points stages (mid points, inputs, upstream gradients).  Rows that fit whole are packed, several to a
// workgroup; longer rows are tiled with the largest tile whose spans fit
template <class Spans>
static bool cno_plan(CnoShape& s, int n_w, const Spans& spans) {
  int sm, sx, sg;
  if (n_w <= CNO_TILE && s.n_mid <= CNO_MID_CAP && s.n_in <= CNO_IN_CAP && s.n_out <= CNO_G_CAP) {
    int pack = CNO_PACK_WORK / s.n_mid;
    pack = std::min(pack, std::min(CNO_MID_CAP / s.n_mid, std::min(CNO_IN_CAP / s.n_in, CNO_G_CAP / s.n_out)));
    pack = std::min(std::max(pack, 1), s.rows);
    s.tile = n_w; s.ntiles = 1; s.pack = pack;
    return true;
  }
  for (int T = CNO_TILE; T >= CNO_MIN_TILE; T >>= 1) {
    spans(T, sm, sx, sg);
    if (sm <= CNO_MID_CAP && sx + 8 <= CNO_IN_CAP && sg + 8 <= CNO_G_CAP) {
      s.tile = T; s.ntiles = (n_w + T - 1) / T; s.pack = 1;
      return true;
    }
  }
  return false;
}

// ---- Conv1d(k = 3, padding = 1): weight and bias gradient ---------------------------------------------------------
// gw[co][ci][t] = sum_{b,x} g[b][co][x] * x[b][ci][x + t - 1],  gb[co] = sum_{b,x} g[b][co][x].  One workgroup per
// 4 x 4 tile of (co, ci): every thread walks the (b, x) points tid, tid + 256, ... with 48 + 4 accumulators, then the
// workgroup adds them up in a fixed order (DPP sum inside a wave, the four waves in sequence): no atomics
constexpr int CNO_WG = 4;
__global__ void __launch_bounds__(256)
k_cno_conv_wgrad(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ gw, float* __restrict__ gb,
                 int B, int Cin, int Cout, int n) {
  __shared__ float red[4][CNO_WG * CNO_WG * 3 + CNO_WG];
  const int ci0 = blockIdx.x * CNO_WG, co0 = blockIdx.y * CNO_WG;
  float acc[CNO_WG][CNO_WG][3], accb[CNO_WG];
#pragma unroll
  for (int j = 0; j < CNO_WG; ++j) {
    accb[j] = 0.f;
#pragma unroll
    for (int i = 0; i < CNO_WG; ++i) acc[j][i][0] = acc[j][i][1] = acc[j][i][2] = 0.f;
  }
  const long total = (long)B * n;
  for (long p = threadIdx.x; p < total; p += 256) {
    const long b = p / n;
    const int xx = (int)(p - b * n);
    float gv[CNO_WG], xv[CNO_WG][3];
#pragma unroll
    for (int j = 0; j < CNO_WG; ++j) gv[j] = co0 + j < Cout ? g[(b * Cout + co0 + j) * n + xx] : 0.f;
#pragma unroll
    for (int i = 0; i < CNO_WG; ++i) {
      const bool live = ci0 + i < Cin;
      const float* row = x + (b * Cin + (live ? ci0 + i : 0)) * n;
      xv[i][0] = live && xx > 0 ? row[xx - 1] : 0.f;
      xv[i][1] = live ? row[xx] : 0.f;
      xv[i][2] = live && xx + 1 < n ? row[xx + 1] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < CNO_WG; ++j) {
      accb[j] += gv[j];
#pragma unroll
      for (int i = 0; i < CNO_WG; ++i)
#pragma unroll
        for (int t = 0; t < 3; ++t) acc[j][i][t] = fmaf(gv[j], xv[i][t], acc[j][i][t]);
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < CNO_WG; ++j) {
#pragma unroll
    for (int i = 0; i < CNO_WG; ++i)
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const float v = wave_sum_dpp(acc[j][i][t]);
        if (lane == 0) red[wave][(j * CNO_WG + i) * 3 + t] = v;
      }
    const float v = wave_sum_dpp(accb[j]);
    if (lane == 0) red[wave][CNO_WG * CNO_WG * 3 + j] = v;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < CNO_WG * CNO_WG * 3 + CNO_WG) {
    const float v = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    if (k < CNO_WG * CNO_WG * 3) {
      const int j = k / (CNO_WG * 3), i = (k / 3) % CNO_WG, t = k % 3;
      if (co0 + j < Cout && ci0 + i < Cin) gw[((long)(co0 + j) * Cin + ci0 + i) * 3 + t] = v;
    } else if (gb && blockIdx.x == 0 && co0 + (k - CNO_WG * CNO_WG * 3) < Cout) {
      gb[co0 + k - CNO_WG * CNO_WG * 3] = v;
    }
  }
}

// ---- BatchNorm1d pieces -------------------------------------------------------------------------------------------
// sums[c] = (sum a, sum b, sum a b, sum b^2) over (batch, x) of channel c of two [B, C, n] tensors, in double; one
// workgroup per channel, fixed order.  The forward takes mean and variance of z from (z, z), the backward sum gy and
// sum gy z from (gy, z)
__global__ void __launch_bounds__(256)
k_cno_moments(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ sums, int B, int C, int n) {
  __shared__ double red[4][4];
  const int c = blockIdx.x;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  const long total = (long)B * n;
  for (long p = threadIdx.x; p < total; p += 256) {
    const long bb = p / n;
    const long at = (bb * C + c) * n + (p - bb * n);
    const double va = a[at], vb = b[at];
    s[0] += va; s[1] += vb; s[2] += va * vb; s[3] += vb * vb;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double v = wave_sum(s[k]);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    sums[c * 4 + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// out = p0[c] a + p1[c] b + p2[c] (+ residual): a BatchNorm's apply step (p1 null: no b term), its backward
// dz = p0 gy + p1 z + p2, and the residual block's skip add.  The coefficients are doubles and so is the arithmetic,
// rounded once: with few values per channel the backward's three terms cancel to eps / (var + eps) of their size, and
// fp32 coefficients would leave nothing of the result; the kernel stays bound by its bytes
template <bool VEC>
__global__ void __launch_bounds__(256)
k_cno_affine(const float* __restrict__ a, const float* __restrict__ b, const double* __restrict__ p0,
             const double* __restrict__ p1, const double* __restrict__ p2, const float* __restrict__ res,
             float* __restrict__ out, long total, int C, int n) {
  constexpr int W = VEC ? 4 : 1;
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * W;
  if (i >= total) return;
  const int c = (int)((i / n) % C);
  const double k0 = p0[c], k1 = p1 ? p1[c] : 0.0, k2 = p2[c];
  alignas(16) float va[W], vb[W], vr[W], o[W];
  if (VEC) {
    *reinterpret_cast<float4*>(va) = *reinterpret_cast<const float4*>(a + i);
    if (p1) *reinterpret_cast<float4*>(vb) = *reinterpret_cast<const float4*>(b + i);
    if (res) *reinterpret_cast<float4*>(vr) = *reinterpret_cast<const float4*>(res + i);
  } else {
    va[0] = a[i];
    if (p1) vb[0] = b[i];
    if (res) vr[0] = res[i];
  }
#pragma unroll
  for (int k = 0; k < W; ++k) {
    double v = fma(k0, (double)va[k], k2);
    if (p1) v = fma(k1, (double)vb[k], v);
    if (res) v += (double)vr[k];
    o[k] = (float)v;
  }
  if (VEC) *reinterpret_cast<float4*>(out + i) = *reinterpret_cast<float4*>(o);
  else out[i] = o[0];
}

}  // namespace rpde

using namespace rpde;

extern "C" {

// the three taps of Conv1d(k = 3, padding = 1) as accumulating GEMMs on shifted views: the centre
// tap over the whole range (it carries the bias and initialises C), then tap 0 onto [1, n) and tap 2 onto [0, n - 1).
// transposed: the data gradient, the same three products with W_t^T and the shifts mirrored
static int cno_conv_taps(const float* src, const float* wt, const float* bias, float* dst, int B, int Csrc, int Cdst, int n,
                         bool transposed, hipStream_t st) {
  const int Cin = transposed ? Cdst : Csrc, Cout = transposed ? Csrc : Cdst;
  for (int pass = 0; pass < 3; ++pass) {
    const int t = pass == 0 ? 1 : (pass == 1 ? 0 : 2);          // tap of this pass
    if (t != 1 && n < 2) break;
    rpde_gemm_desc d = gemm_desc();
    d.A = wt + (long)t * Cout * Cin; d.a_kmajor = transposed ? 0 : 1; d.lda = Cin;
    d.b_kmajor = 0; d.ldb = n; d.ldc = n;
    d.M = Cdst; d.K = Csrc; d.N = t == 1 ? n : n - 1;
    d.batch = B; d.sB1 = (long)Csrc * n; d.sC1 = (long)Cdst * n;
    // forward: out[x] += W_t in[x + t - 1]; data gradient: gx[x] += W_t^T g[x - (t - 1)]
    const int read_first = (t == 1) ? 0 : ((t == 0) != transposed ? 0 : 1);
    const int write_first = (t == 1) ? 0 : 1 - read_first;
    d.B = src + read_first; d.C = dst + write_first;
    d.accumulate = pass > 0;
    if (pass == 0 && bias) { d.bias = bias; d.bias_mode = 2; }
    RPDE_TRY(launch_gemm(d, st));
  }
  return RPDE_OK;
}

int rpde_cno_conv1d_k3_fwd(const float* x, const float* wt, const float* bias, float* out, int B, int Cin, int Cout, int n,
                           void* stream) {
  RPDE_CHECK_ARG(x && wt && out, "cno_conv1d_k3_fwd: null tensor");
  RPDE_CHECK_ARG(B > 0 && Cin > 0 && Cout > 0 && n > 0, "cno_conv1d_k3_fwd: bad sizes B=%d Cin=%d Cout=%d n=%d", B, Cin, Cout, n);
  return cno_conv_taps(x, wt, bias, out, B, Cin, Cout, n, false, as_stream(stream));
}

int rpde_cno_conv1d_k3_bwd_data(const float* g, const float* wt, float* gx, int B, int Cin, int Cout, int n, void* stream) {
  RPDE_CHECK_ARG(g && wt && gx, "cno_conv1d_k3_bwd_data: null tensor");
  RPDE_CHECK_ARG(B > 0 && Cin > 0 && Cout > 0 && n > 0, "cno_conv1d_k3_bwd_data: bad sizes B=%d Cin=%d Cout=%d n=%d", B, Cin, Cout, n);
  return cno_conv_taps(g, wt, nullptr, gx, B, Cout, Cin, n, true, as_stream(stream));
}

int rpde_cno_conv1d_k3_bwd_weight(const float* x, const float* g, float* gw, float* gb, int B, int Cin, int Cout, int n,
                                  void* stream) {
  RPDE_CHECK_ARG(x && g && gw, "cno_conv1d_k3_bwd_weight: null tensor");
  RPDE_CHECK_ARG(B > 0 && Cin > 0 && Cout > 0 && n > 0, "cno_conv1d_k3_bwd_weight: bad sizes B=%d Cin=%d Cout=%d n=%d", B, Cin, Cout, n);
  const dim3 grid((unsigned)((Cin + CNO_WG - 1) / CNO_WG), (unsigned)((Cout + CNO_WG - 1) / CNO_WG));
  RPDE_CHECK_ARG(grid.y <= 65535, "cno_conv1d_k3_bwd_weight: too many output channels (%d)", Cout);
  hipLaunchKernelGGL(k_cno_conv_wgrad, grid, dim3(256), 0, as_stream(stream), x, g, gw, gb, B, Cin, Cout, n);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_cno_moments(const float* a, const float* b, double* sums, int B, int C, int n, void* stream) {
  RPDE_CHECK_ARG(a && b && sums, "cno_moments: null tensor");
  RPDE_CHECK_ARG(B > 0 && C > 0 && n > 0, "cno_moments: bad sizes B=%d C=%d n=%d", B, C, n);
  RPDE_CHECK_ARG((reinterpret_cast<uintptr_t>(sums) & 7) == 0, "cno_moments: sums must be 8-byte aligned");
  hipLaunchKernelGGL(k_cno_moments, dim3((unsigned)C), dim3(256), 0, as_stream(stream), a, b, sums, B, C, n);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_cno_affine(const float* a, const float* b, const double* p0, const double* p1, const double* p2, const float* residual,
                    float* out, int B, int C, int n, void* stream) {
  RPDE_CHECK_ARG(a && p0 && p2 && out, "cno_affine: null tensor");
  RPDE_CHECK_ARG((b == nullptr) == (p1 == nullptr), "cno_affine: b and p1 come together");
  RPDE_CHECK_ARG(B > 0 && C > 0 && n > 0, "cno_affine: bad sizes B=%d C=%d n=%d", B, C, n);
  const long total = (long)B * C * n;
  const bool vec = n % 4 == 0 && al16(a) && al16(out) && (!b || al16(b)) && (!residual || al16(residual));
  const long threads = vec ? total / 4 : total;
  RPDE_CHECK_ARG((threads + 255) / 256 < (1L << 31), "cno_affine: tensor too large for one launch");
  const dim3 grid((unsigned)((threads + 255) / 256));
  if (vec) hipLaunchKernelGGL((k_cno_affine<true>), grid, dim3(256), 0, as_stream(stream), a, b, p0, p1, p2, residual, out, total, C, n);
  else hipLaunchKernelGGL((k_cno_affine<false>), grid, dim3(256), 0, as_stream(stream), a, b, p0, p1, p2, residual, out, total, C, n);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_cno_act1d_fwd(const float* x, const float* scale, const float* shift, float* out, int B, int C, int n_in, int n_mid,
                       int n_out, float slope, const int32_t* u_span, const float* u_w, int u_taps, const int32_t* d_span,
                       const float* d_w, int d_taps, void* stream) {
  RPDE_TRY(cno_check("cno_act1d_fwd", x, scale, shift, B, C, n_in, n_mid, n_out, slope));
  RPDE_CHECK_ARG(out, "cno_act1d_fwd: null tensor");
  RPDE_TRY(cno_band("cno_act1d_fwd", "U", u_span, u_w, u_taps));
  RPDE_TRY(cno_band("cno_act1d_fwd", "D", d_span, d_w, d_taps));
  CnoShape s{B * C, C, n_in, n_mid, n_out, 0, 0, 0, 0, 0, slope};
  const bool fits = cno_plan(s, n_out, [&](int T, int& sm, int& sx, int& sg) {
    sm = cno_sources(T, n_mid, n_out); sx = cno_sources(sm, n_in, n_mid); sg = 0;
  });
  RPDE_CHECK_ARG(fits, "cno_act1d_fwd: %d -> %d -> %d: the sources of %d outputs do not fit a workgroup's staging area",
                 n_in, n_mid, n_out, CNO_MIN_TILE);
  s.vec_x = n_in % 4 == 0 && al16(x);
  s.vec_o = n_out % 4 == 0 && al16(out);
  const long groups = ((long)s.rows + s.pack - 1) / s.pack;
  RPDE_CHECK_ARG(groups * s.ntiles < (1L << 31), "cno_act1d_fwd: too many workgroups");
  const dim3 grid((unsigned)(groups * s.ntiles)), block(CNO_THREADS);
  const CnoBand U{reinterpret_cast<const int2*>(u_span), u_w, u_taps}, D{reinterpret_cast<const int2*>(d_span), d_w, d_taps};
  hipStream_t st = as_stream(stream);
  if (s.vec_x && s.vec_o) hipLaunchKernelGGL((k_cno_act_fwd<true, true>), grid, block, 0, st, x, scale, shift, out, s, U, D);
  else if (s.vec_x) hipLaunchKernelGGL((k_cno_act_fwd<true, false>), grid, block, 0, st, x, scale, shift, out, s, U, D);
  else if (s.vec_o) hipLaunchKernelGGL((k_cno_act_fwd<false, true>), grid, block, 0, st, x, scale, shift, out, s, U, D);
  else hipLaunchKernelGGL((k_cno_act_fwd<false, false>), grid, block, 0, st, x, scale, shift, out, s, U, D);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_cno_act1d_bwd(const float* x, const float* scale, const float* shift, const float* g, float* gy, int B, int C,
                       int n_in, int n_mid, int n_out, float slope, const int32_t* u_span, const float* u_w, int u_taps,
                       const int32_t* ut_span, const float* ut_w, int ut_taps, const int32_t* dt_span, const float* dt_w,
                       int dt_taps, void* stream) {
  RPDE_TRY(cno_check("cno_act1d_bwd", x, scale, shift, B, C, n_in, n_mid, n_out, slope));
  RPDE_CHECK_ARG(g && gy, "cno_act1d_bwd: null tensor");
  RPDE_TRY(cno_band("cno_act1d_bwd", "U", u_span, u_w, u_taps));
  RPDE_TRY(cno_band("cno_act1d_bwd", "U^T", ut_span, ut_w, ut_taps));
  RPDE_TRY(cno_band("cno_act1d_bwd", "D^T", dt_span, dt_w, dt_taps));
  CnoShape s{B * C, C, n_in, n_mid, n_out, 0, 0, 0, 0, 0, slope};
  const bool fits = cno_plan(s, n_in, [&](int T, int& sm, int& sx, int& sg) {
    sm = cno_readers(T, n_in, n_mid); sx = cno_sources(sm, n_in, n_mid); sg = cno_readers(sm, n_mid, n_out);
  });
  RPDE_CHECK_ARG(fits, "cno_act1d_bwd: %d -> %d -> %d: what %d inputs reach does not fit a workgroup's staging area",
                 n_in, n_mid, n_out, CNO_MIN_TILE);
  s.vec_x = n_in % 4 == 0 && al16(x) && al16(gy);
  s.vec_o = n_out % 4 == 0 && al16(g);
  const long groups = ((long)s.rows + s.pack - 1) / s.pack;
  RPDE_CHECK_ARG(groups * s.ntiles < (1L << 31), "cno_act1d_bwd: too many workgroups");
  const dim3 grid((unsigned)(groups * s.ntiles)), block(CNO_THREADS);
  const CnoBand U{reinterpret_cast<const int2*>(u_span), u_w, u_taps}, UT{reinterpret_cast<const int2*>(ut_span), ut_w, ut_taps},
      DT{reinterpret_cast<const int2*>(dt_span), dt_w, dt_taps};
  hipStream_t st = as_stream(stream);
  if (s.vec_x && s.vec_o) hipLaunchKernelGGL((k_cno_act_bwd<true, true>), grid, block, 0, st, x, scale, shift, g, gy, s, U, UT, DT);
  else if (s.vec_x) hipLaunchKernelGGL((k_cno_act_bwd<true, false>), grid, block, 0, st, x, scale, shift, g, gy, s, U, UT, DT);
  else if (s.vec_o) hipLaunchKernelGGL((k_cno_act_bwd<false, true>), grid, block, 0, st, x, scale, shift, g, gy, s, U, UT, DT);
  else hipLaunchKernelGGL((k_cno_act_bwd<false, false>), grid, block, 0, st, x, scale, shift, g, gy, s, U, UT, DT);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

}  // extern "C"
