// The CNO activation (reference models/CNO1d.py:30-45) as one kernel per direction: antialiased bicubic resampling to
// n_mid points, LeakyReLU, antialiased bicubic resampling to n_out points.  Both resamplings are fixed banded linear
// maps (rpde/cno.py builds their tables from torch's rule), so a workgroup stages a row segment with its halo in LDS,
// forms the mid signal there, and writes only the result: x is read once and out written once.
// The rest of a CNO block -- Conv(k = 3), BatchNorm -- is in cno_layers.hip.  gfx950 (CDNA4, wave64) only.
#include "cno.h"

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

}  // namespace rpde

using namespace rpde;

extern "C" {

int rpde_cno_act1d_fwd(const float* x, const float* scale, const float* shift, float* out, int B, int C, int n_in, int n_mid,
                       int n_out, float slope, const int32_t* u_span, const float* u_w, int u_taps, const int32_t* d_span,
                       const float* d_w, int d_taps, void* stream) {
  RPDE_TRY(cno_check("cno_act1d_fwd", x, scale, shift, B, C, n_in, n_mid, n_out, slope));
  RPDE_CHECK_ARG(out, "cno_act1d_fwd: null tensor");
  CnoBand U, D;
  RPDE_TRY(cno_band("cno_act1d_fwd", "U", u_span, u_w, u_taps, U));
  RPDE_TRY(cno_band("cno_act1d_fwd", "D", d_span, d_w, d_taps, D));
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
  hipStream_t st = as_stream(stream);
  cno_vec_dispatch(s.vec_x, s.vec_o, [&](auto VX, auto VO) {
    hipLaunchKernelGGL((k_cno_act_fwd<decltype(VX)::value, decltype(VO)::value>), grid, block, 0, st, x, scale, shift, out, s, U, D);
  });
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_cno_act1d_bwd(const float* x, const float* scale, const float* shift, const float* g, float* gy, int B, int C,
                       int n_in, int n_mid, int n_out, float slope, const int32_t* u_span, const float* u_w, int u_taps,
                       const int32_t* ut_span, const float* ut_w, int ut_taps, const int32_t* dt_span, const float* dt_w,
                       int dt_taps, void* stream) {
  RPDE_TRY(cno_check("cno_act1d_bwd", x, scale, shift, B, C, n_in, n_mid, n_out, slope));
  RPDE_CHECK_ARG(g && gy, "cno_act1d_bwd: null tensor");
  CnoBand U, UT, DT;
  RPDE_TRY(cno_band("cno_act1d_bwd", "U", u_span, u_w, u_taps, U));
  RPDE_TRY(cno_band("cno_act1d_bwd", "U^T", ut_span, ut_w, ut_taps, UT));
  RPDE_TRY(cno_band("cno_act1d_bwd", "D^T", dt_span, dt_w, dt_taps, DT));
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
  hipStream_t st = as_stream(stream);
  cno_vec_dispatch(s.vec_x, s.vec_o, [&](auto VX, auto VO) {
    hipLaunchKernelGGL((k_cno_act_bwd<decltype(VX)::value, decltype(VO)::value>), grid, block, 0, st, x, scale, shift, g, gy, s, U, UT, DT);
  });
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

}  // extern "C"
