// What a U-Net adds to the CNO layers (cno_layers.hip), both ranks: tanh behind a norm's per-channel affine with
// MaxPool(2) in the same pass and its one-pass backward, and ConvTranspose(kernel_size = 2, stride = 2) as one matrix
// product on the fp32-input MFMA with the taps interleaved in LDS, its transposed product and its deterministic weight
// gradient.  1-D is the 2-D entry on a plane of one row with one row of taps (KY = 1).  DESIGN.md 10.18.  gfx950 (CDNA4,
// wave64) only.
#include "cno.h"
#include "wgrad_sliced.h"

namespace rpde {

// ---- tanh(scale z + shift) and MaxPool over KY x 2 windows ----------------------------------------------------------
// A thread owns a patch of KY rows x CW columns of one plane: CW = 4 with 16-byte accesses (W % 4 == 0: two windows),
// CW = 2 otherwise (one window).  A trailing odd row or column gets a patch of its own that holds no whole window.
struct TpShape {
  int C, H, W;
  int HP, WG;        // patches per plane: rows of them, and per row
  int Ho, Wo;        // the pooled plane
  long items;
};

// the first maximum of v[0 .. N) in scan order; a NaN replaces whatever is held (torch's max_pool rule)
template <int N>
__device__ __forceinline__ int first_max(const float (&v)[N], float& best) {
  int at = 0;
  best = v[0];
#pragma unroll
  for (int k = 1; k < N; ++k)
    if (v[k] > best || isnan(v[k])) { best = v[k]; at = k; }
  return at;
}

template <int KY, bool VEC>
struct TpPatch {
  static constexpr int CW = VEC ? 4 : 2;
  int c, x0, y0;
  long base;         // of the patch's first element in a [B C, H, W] tensor
  long pool_at;      // of its first window in the pooled tensor
  bool whole_rows;   // all KY rows exist
  __device__ __forceinline__ bool locate(const TpShape& s) {
    const long it = (long)blockIdx.x * 256 + threadIdx.x;
    if (it >= s.items) return false;
    const int xg = (int)(it % s.WG);
    const long r = it / s.WG;
    const int yp = (int)(r % s.HP);
    const long bc = r / s.HP;
    c = (int)(bc % s.C);
    x0 = xg * CW; y0 = yp * KY;
    base = (bc * s.H + y0) * s.W + x0;
    pool_at = (bc * s.Ho + yp) * s.Wo + x0 / 2;
    whole_rows = y0 + KY <= s.H;
    return true;
  }
  // v[ty][tx] = src[patch]; elements outside the plane are left alone
  __device__ __forceinline__ void load(const float* __restrict__ src, const TpShape& s, float (&v)[KY][CW]) const {
#pragma unroll
    for (int ty = 0; ty < KY; ++ty) {
      if (y0 + ty >= s.H) continue;
      const float* row = src + base + (long)ty * s.W;
      if constexpr (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(row);
        v[ty][0] = q.x; v[ty][1] = q.y; v[ty][2] = q.z; v[ty][3] = q.w;
      } else {
        v[ty][0] = row[0];
        if (x0 + 1 < s.W) v[ty][1] = row[1];
      }
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ dst, const TpShape& s, const float (&v)[KY][CW]) const {
#pragma unroll
    for (int ty = 0; ty < KY; ++ty) {
      if (y0 + ty >= s.H) continue;
      float* row = dst + base + (long)ty * s.W;
      if constexpr (VEC) {
        *reinterpret_cast<float4*>(row) = make_float4(v[ty][0], v[ty][1], v[ty][2], v[ty][3]);
      } else {
        row[0] = v[ty][0];
        if (x0 + 1 < s.W) row[1] = v[ty][1];
      }
    }
  }
  // window j of the patch lies in the plane
  __device__ __forceinline__ bool window(const TpShape& s, int j) const { return whole_rows && x0 + 2 * j + 1 < s.W; }
};

template <int KY, bool VEC>
__global__ void __launch_bounds__(256)
k_unet_tanh_pool_fwd(const float* __restrict__ z, const float* __restrict__ scale, const float* __restrict__ shift,
                     float* __restrict__ act, float* __restrict__ pooled, TpShape s) {
  using P = TpPatch<KY, VEC>;
  constexpr int CW = P::CW;
  P p;
  if (!p.locate(s)) return;
  float v[KY][CW] = {};
  p.load(z, s, v);
  if (scale) {
    const float k0 = scale[p.c], k1 = shift[p.c];
#pragma unroll
    for (int ty = 0; ty < KY; ++ty)
#pragma unroll
      for (int tx = 0; tx < CW; ++tx) v[ty][tx] = fmaf(k0, v[ty][tx], k1);
  }
#pragma unroll
  for (int ty = 0; ty < KY; ++ty)
#pragma unroll
    for (int tx = 0; tx < CW; ++tx) v[ty][tx] = tanhf(v[ty][tx]);
  p.store(act, s, v);
  if (!pooled) return;
  float best[CW / 2];
#pragma unroll
  for (int j = 0; j < CW / 2; ++j) {
    float w[2 * KY];
#pragma unroll
    for (int ty = 0; ty < KY; ++ty) { w[2 * ty] = v[ty][2 * j]; w[2 * ty + 1] = v[ty][2 * j + 1]; }
    first_max(w, best[j]);
  }
  if constexpr (VEC) {
    if (p.whole_rows) *reinterpret_cast<float2*>(pooled + p.pool_at) = make_float2(best[0], best[1]);
  } else if (p.window(s, 0)) {
    pooled[p.pool_at] = best[0];
  }
}

// gy = (g_act + scatter(g_pool)) (1 - act^2): the window's gradient goes to the element first_max picks from act
template <int KY, bool VEC>
__global__ void __launch_bounds__(256)
k_unet_tanh_pool_bwd(const float* __restrict__ act, const float* __restrict__ g_act, const float* __restrict__ g_pool,
                     float* __restrict__ gy, TpShape s) {
  using P = TpPatch<KY, VEC>;
  constexpr int CW = P::CW;
  P p;
  if (!p.locate(s)) return;
  float a[KY][CW] = {}, g[KY][CW] = {};
  p.load(act, s, a);
  if (g_act) p.load(g_act, s, g);
  if (g_pool) {
#pragma unroll
    for (int j = 0; j < CW / 2; ++j) {
      if (!p.window(s, j)) continue;
      float w[2 * KY], best;
#pragma unroll
      for (int ty = 0; ty < KY; ++ty) { w[2 * ty] = a[ty][2 * j]; w[2 * ty + 1] = a[ty][2 * j + 1]; }
      const int at = first_max(w, best);
      const float gp = g_pool[p.pool_at + j];
#pragma unroll
      for (int ty = 0; ty < KY; ++ty)
#pragma unroll
        for (int tx = 0; tx < 2; ++tx)
          if (at == 2 * ty + tx) g[ty][2 * j + tx] += gp;
    }
  }
#pragma unroll
  for (int ty = 0; ty < KY; ++ty)
#pragma unroll
    for (int tx = 0; tx < CW; ++tx) g[ty][tx] *= fmaf(-a[ty][tx], a[ty][tx], 1.f);
  p.store(gy, s, g);
}

// ---- ConvTranspose(kernel_size = 2, stride = 2) ----------------------------------------------------------------------
// Stride equals kernel, so no two taps meet: with T = 2 KY taps, rows m = co T + 2 ty + tx (the weight [Cin][Cout][T] is
// [Cin][M] as it lies) and the points p = (b, y, x) of the input as columns,
//   forward:   out[m][p] = sum_ci w[ci][m] x[ci][p]          M = T Cout rows, K = Cin
//   backward:  gx[ci][p] = sum_m  w[ci][m] g[m][p]           M = Cin rows,    K = T Cout
// where row m of `out` / `g` at point p is element (b, co, KY y + ty, 2 x + tx) of the [B, Cout, KY H, 2 W] tensor.  A
// workgroup of four waves owns 64 rows x 64 points; K goes through LDS 16 at a time, every wave runs
// v_mfma_f32_16x16x4_f32 on its 16 points and four row tiles (an exact fmaf chain in k order).  The forward's epilogue
// reads the result tile back from LDS with (point, tx) as the fast index, so that a wave's stores are the contiguous
// elements 2 x + tx of an output row; the backward gathers them the same way on the load side.
constexpr int UC_TILE = 64, UC_K = 16;
constexpr int UC_LD = 80;            // row stride of the staged operands: the four k rows of a fragment read hit 64 banks

template <int KY, bool BWD>
__global__ void __launch_bounds__(256)
k_unet_upconv(const float* __restrict__ src, const float* __restrict__ w, const float* __restrict__ bias,
              float* __restrict__ dst, int B, int Cin, int Cout, int H, int W) {
  constexpr int T = 2 * KY;
  __shared__ float As[UC_K][UC_LD], Bs[UC_K][UC_LD];
  __shared__ float Cs[UC_TILE][UC_TILE + 1];
  const int MT = T * Cout;
  const int M = BWD ? Cin : MT, K = BWD ? MT : Cin;
  const long plane = (long)H * W, NP = (long)B * plane;
  const long big_plane = plane * T;                       // one channel of the [B, Cout, KY H, 2 W] tensor
  const int m0 = blockIdx.y * UC_TILE;
  const long p0 = (long)blockIdx.x * UC_TILE;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

  // the point this thread loads (and, in the forward, stores): the forward's loader walks (k, point), the gathering
  // sides walk (row pair, point, tx)
  const bool gather_load = BWD, gather_store = !BWD;
  const int pp_gather = (tid & 127) >> 1, tx_gather = tid & 1;
  const int pp_flat = tid & 63;
  // element (b, co = 0, KY y, 2 x) of the big tensor for point p, and element (b, c = 0, y, x) of the small one
  auto big_at = [&](long p, int C) {
    const long b = p / plane, q = p - b * plane;
    const long y = q / W, x = q - y * W;
    return b * C * big_plane + (long)KY * y * 2 * W + 2 * x;
  };
  auto small_at = [&](long p, int C) {
    const long b = p / plane;
    return b * C * plane + (p - b * plane);
  };
  const long p_load = p0 + (gather_load ? pp_gather : pp_flat);
  const bool p_load_ok = p_load < NP;
  const long load_at = !p_load_ok ? 0 : gather_load ? big_at(p_load, Cout) : small_at(p_load, Cin);

  f32x4v acc[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4v{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < K; k0 += UC_K) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + 256 * i;
      // A[m][k]: the forward reads w[k][m] along m, the backward w[m][k] along k
      const int kk = BWD ? e & 15 : e >> 6, mm = BWD ? e >> 4 : e & 63;
      const int m = m0 + mm, k = k0 + kk;
      float a = 0.f;
      if (m < M && k < K) a = BWD ? w[(long)m * MT + k] : w[(long)k * MT + m];
      As[kk][mm] = a;
      float b = 0.f;
      if (BWD) {
        const int pair = e >> 7, kb = 2 * pair + tx_gather, kg = k0 + kb;      // k = co T + 2 ty + tx
        if (p_load_ok && kg < K) {
          const int co = kg / T, ty = (kg % T) >> 1;
          b = src[load_at + co * big_plane + (long)ty * 2 * W + tx_gather];
        }
        Bs[kb][pp_gather] = b;
      } else {
        const int kb = e >> 6, kg = k0 + kb;
        if (p_load_ok && kg < K) b = src[load_at + kg * plane];
        Bs[kb][pp_flat] = b;
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < UC_K / 4; ++ks) {
      const int kr = ks * 4 + (lane >> 4);
      const float b = Bs[kr][wave * 16 + (lane & 15)];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(As[kr][mt * 16 + (lane & 15)], b, acc[mt], 0, 0, 0);
    }
    __syncthreads();
  }

  // accumulator tile: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) Cs[mt * 16 + (lane >> 4) * 4 + r][wave * 16 + (lane & 15)] = acc[mt][r];
  __syncthreads();

  if (gather_store) {
    const long p = p0 + pp_gather;
    if (p >= NP) return;
    const long store_at = big_at(p, Cout);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int pair = (tid >> 7) + 2 * i, ml = 2 * pair + tx_gather, m = m0 + ml;
      if (m >= M) continue;
      const int co = m / T, ty = (m % T) >> 1;
      const float v = Cs[ml][pp_gather] + (bias ? bias[co] : 0.f);
      dst[store_at + co * big_plane + (long)ty * 2 * W + tx_gather] = v;
    }
  } else {
    const long p = p0 + pp_flat;
    if (p >= NP) return;
    const long store_at = small_at(p, Cin);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int ml = (tid >> 6) + 4 * i, m = m0 + ml;
      if (m < M) dst[store_at + m * plane] = Cs[ml][pp_flat];
    }
  }
}

// gw[ci][co][t] = sum_p x[ci][p] g[co T + t][p],  gb[co] = sum_{p, t} g[co T + t][p], on the sliced scaffold of
// wgrad_sliced.h: x is the narrow operand, the 2 KY taps of g the wide one.  The slices are runs of points
template <int KY>
struct UpconvWgrad {
  static constexpr int T = 2 * KY;
  static constexpr bool G_NARROW = false;
  int W;
  long p_lo, plane, big_plane, b, q, y, xx;
  __device__ UpconvWgrad(int H, int W_, long p_lo_) : W(W_), p_lo(p_lo_), plane((long)H * W_), big_plane(plane * T) {}
  __device__ __forceinline__ void seek(long i) {
    const long p = p_lo + i;
    b = p / plane; q = p - b * plane;
    y = q / W; xx = q - y * W;
  }
  __device__ __forceinline__ float narrow(const float* __restrict__ x, int Cin, int ci) const {
    return ci < Cin ? x[(b * Cin + ci) * plane + q] : 0.f;
  }
  __device__ __forceinline__ void wide(const float* __restrict__ g, int Cout, int co, float (&gv)[T]) const {
    const bool live = co < Cout;
    const float* at = g + (b * Cout + (live ? co : 0)) * big_plane + (long)KY * y * 2 * W + 2 * xx;
#pragma unroll
    for (int t = 0; t < T; ++t) gv[t] = live ? at[(long)(t >> 1) * 2 * W + (t & 1)] : 0.f;
  }
};

constexpr int UNET_MAX = 1 << 24;

static int tp_shape(const char* what, int B, int C, int H, int W, int ky, bool pool, bool vec, TpShape& s) {
  RPDE_CHECK_ARG(ky == 1 || ky == 2, "%s: ky must be 1 (1-D) or 2 (2-D), got %d", what, ky);
  RPDE_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "%s: bad sizes B=%d C=%d H=%d W=%d", what, B, C, H, W);
  RPDE_CHECK_ARG(B < UNET_MAX && C < UNET_MAX && H < UNET_MAX && W < UNET_MAX, "%s: sizes must stay below 2^24", what);
  RPDE_CHECK_ARG(ky == 2 || H == 1, "%s: ky = 1 is the 1-D entry, a plane of one row (H = %d)", what, H);
  s.C = C; s.H = H; s.W = W;
  s.Ho = H / ky; s.Wo = W / 2;
  RPDE_CHECK_ARG(!pool || (s.Ho > 0 && s.Wo > 0), "%s: nothing left to pool from %d x %d with %d x 2 windows", what, H, W, ky);
  const int cw = vec ? 4 : 2;
  s.HP = (H + ky - 1) / ky; s.WG = (W + cw - 1) / cw;
  s.items = (long)B * C * s.HP * s.WG;
  RPDE_CHECK_ARG((s.items + 255) / 256 < (1L << 31), "%s: tensor too large for one launch", what);
  return RPDE_OK;
}

static int upconv_check(const char* what, const void* a, const void* b, const void* c, int B, int Cin, int Cout, int H, int W,
                        int ky) {
  RPDE_CHECK_ARG(a && b && c, "%s: null tensor", what);
  RPDE_CHECK_ARG(ky == 1 || ky == 2, "%s: ky must be 1 (1-D) or 2 (2-D), got %d", what, ky);
  RPDE_CHECK_ARG(B > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, "%s: bad sizes B=%d Cin=%d Cout=%d H=%d W=%d", what, B, Cin,
                 Cout, H, W);
  RPDE_CHECK_ARG(B < UNET_MAX && Cin < UNET_MAX && Cout < UNET_MAX && H < UNET_MAX && W < UNET_MAX,
                 "%s: sizes must stay below 2^24", what);
  RPDE_CHECK_ARG(ky == 2 || H == 1, "%s: ky = 1 is the 1-D entry, a plane of one row (H = %d)", what, H);
  RPDE_CHECK_ARG((long)B * H * W < (1L << 31), "%s: too many points (B H W must stay below 2^31)", what);
  return RPDE_OK;
}

template <bool BWD>
static int upconv_launch(const char* what, const float* src, const float* w, const float* bias, float* dst, int B, int Cin,
                         int Cout, int H, int W, int ky, hipStream_t st) {
  const long M = BWD ? Cin : 2L * ky * Cout, NP = (long)B * H * W;
  const dim3 grid((unsigned)((NP + UC_TILE - 1) / UC_TILE), (unsigned)((M + UC_TILE - 1) / UC_TILE));
  RPDE_CHECK_ARG(grid.y <= 65535, "%s: too many channels (%ld rows)", what, M);
  if (ky == 1) hipLaunchKernelGGL((k_unet_upconv<1, BWD>), grid, dim3(256), 0, st, src, w, bias, dst, B, Cin, Cout, H, W);
  else hipLaunchKernelGGL((k_unet_upconv<2, BWD>), grid, dim3(256), 0, st, src, w, bias, dst, B, Cin, Cout, H, W);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

}  // namespace rpde

using namespace rpde;

extern "C" {

int rpde_unet_tanh_pool_fwd(const float* z, const float* scale, const float* shift, float* act, float* pooled, int B, int C,
                            int H, int W, int ky, void* stream) {
  const char* what = "unet_tanh_pool_fwd";
  RPDE_CHECK_ARG(z && act, "%s: null tensor", what);
  RPDE_CHECK_ARG((scale == nullptr) == (shift == nullptr), "%s: scale and shift come together", what);
  const bool vec = W % 4 == 0 && al16(z) && al16(act) && (!pooled || al16(pooled));
  TpShape s;
  RPDE_TRY(tp_shape(what, B, C, H, W, ky, pooled != nullptr, vec, s));
  const dim3 grid((unsigned)((s.items + 255) / 256));
  cno_vec_dispatch(vec, ky == 2, [&](auto V, auto TWO) {
    hipLaunchKernelGGL((k_unet_tanh_pool_fwd<decltype(TWO)::value ? 2 : 1, decltype(V)::value>), grid, dim3(256), 0,
                       as_stream(stream), z, scale, shift, act, pooled, s);
  });
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_unet_tanh_pool_bwd(const float* act, const float* g_act, const float* g_pool, float* gy, int B, int C, int H, int W,
                            int ky, void* stream) {
  const char* what = "unet_tanh_pool_bwd";
  RPDE_CHECK_ARG(act && gy, "%s: null tensor", what);
  RPDE_CHECK_ARG(g_act || g_pool, "%s: no gradient given (g_act and g_pool are both null)", what);
  const bool vec = W % 4 == 0 && al16(act) && al16(gy) && (!g_act || al16(g_act));
  TpShape s;
  RPDE_TRY(tp_shape(what, B, C, H, W, ky, g_pool != nullptr, vec, s));
  const dim3 grid((unsigned)((s.items + 255) / 256));
  cno_vec_dispatch(vec, ky == 2, [&](auto V, auto TWO) {
    hipLaunchKernelGGL((k_unet_tanh_pool_bwd<decltype(TWO)::value ? 2 : 1, decltype(V)::value>), grid, dim3(256), 0,
                       as_stream(stream), act, g_act, g_pool, gy, s);
  });
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_unet_upconv_fwd(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int H, int W,
                         int ky, void* stream) {
  const char* what = "unet_upconv_fwd";
  RPDE_TRY(upconv_check(what, x, w, out, B, Cin, Cout, H, W, ky));
  return upconv_launch<false>(what, x, w, bias, out, B, Cin, Cout, H, W, ky, as_stream(stream));
}

int rpde_unet_upconv_bwd_data(const float* g, const float* w, float* gx, int B, int Cin, int Cout, int H, int W, int ky,
                              void* stream) {
  const char* what = "unet_upconv_bwd_data";
  RPDE_TRY(upconv_check(what, g, w, gx, B, Cin, Cout, H, W, ky));
  return upconv_launch<true>(what, g, w, nullptr, gx, B, Cin, Cout, H, W, ky, as_stream(stream));
}

int rpde_unet_upconv_bwd_weight_slices(int B, int Cin, int Cout, int H, int W) {
  if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return 0;
  return wgrad_slices(Cin, Cout, (long)B * H * W, (long)B * H * W);
}

int rpde_unet_upconv_bwd_weight(const float* x, const float* g, float* gw, float* gb, int B, int Cin, int Cout, int H, int W,
                                int ky, float* partial, int partial_slices, void* stream) {
  const char* what = "unet_upconv_bwd_weight";
  RPDE_TRY(upconv_check(what, x, g, gw, B, Cin, Cout, H, W, ky));
  const auto run = ky == 1 ? wgrad_sliced<UpconvWgrad<1>> : wgrad_sliced<UpconvWgrad<2>>;
  return run(what, x, g, gw, gb, B, Cin, Cout, H, W, (long)B * H * W, partial, partial_slices, as_stream(stream));
}

}  // extern "C"
