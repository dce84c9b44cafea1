// The first FFNO2D layer's spectral branch on the UNLIFTED input.
//
// Layer 0 is the only layer whose input is a pointwise linear map of a thin field, h0 = W_in u + b_in with u [B,M,N,Cin],
// Cin <= 4.  A pointwise channel map commutes with the DFT along space and the branch analysis -> mode mix -> synthesis
// is linear, so
//
//   synthesis(mix(analysis(W_in u + b_in))) = synthesis(mix'(analysis(u~)))
//   W'[k][j][o] = sum_i W~[i][j] Wmix[k][i][o]        W~ = [W_in | b_in],  u~ = [u | 1]   (CA = Cin + 1 channels)
//
// and the spectrum of the constant channel is sqrt(n) at k = 0 ('ortho' norm) and zero elsewhere: it is never computed
// or stored, the kernels put it in where they read S_u.
//
//   forward    k_lift_analysis   S_u[line][2kp][Cin] = Fa . u-line, both axes, exact fp32           (25 MB read at 256^2, B = 32)
//              k_lift_wprime     W' of both axes from W_in, b_in and the two mode-mix weights
//              k_lift_mix        Cin -> 64 per (line, mode) in fp32, written as the operand blocks + line scales that
//                                k_spec_split_h2 would write for that spectrum (fused_spectral.h, "operand blocks")
//              fused2d_synthesis unchanged
//   backward   fused2d_analysis of g (adjoint tables), unchanged
//              k_lift_tgrad      T[axis][k][j][o] = sum_lines conj(S_u~[line][k][j]) G[line][k][o]: partial sums over
//                                slabs of lines, folded in fixed order by reduce_slabs (no atomics: run-to-run identical)
//              k_lift_chain_w    gWmix[i][o][k] = sum_j W~[i][j] T[k][j][o]
//              k_lift_chain_in   gW~[i][j] = sum_{axis,k,o} Re(conj(Wmix[k][i][o]) T[k][j][o])   -> gW_in, gb_in
// No adjoint mix, no adjoint synthesis and no [P,64] input gradient: the branch's only consumers are weights.
// Only S_u is saved: lines x 2kp x Cin floats per axis.
#include "fused_spectral.h"
#include "h2.h"
#include "lifted_spectral.h"
#include "pointwise.h"
#include "workspace.h"

namespace rpde {

constexpr int LIFT_LT = 32;           // lines per workgroup of the analysis (one 128-byte-or-longer run per point along x)
constexpr int LIFT_ML = 16;           // lines per workgroup of the mix (W' stays in registers over them)

struct LiftGeom {
  int B, M, N, keff, kp, R;
  long lines[2];                      // y: one line per (b, m), n = N points;  x: one per (b, n), n = M points
  int n[2];
};

static LiftGeom lift_geom(int B, int M, int N, int K) {
  LiftGeom g;
  g.B = B; g.M = M; g.N = N;
  const int ky = K < N / 2 + 1 ? K : N / 2 + 1;
  g.keff = ky; g.kp = r4(ky); g.R = 2 * g.kp;      // fused2d_ok: the same count on both axes
  g.lines[0] = (long)B * M; g.lines[1] = (long)B * N;
  g.n[0] = N; g.n[1] = M;
  return g;
}

// ------------------------------------------------------------------------------------------------------------
// analysis of the thin field: S[line][r][c] = sum_y Fa[r][y] u[line][y][c], 32 points at a time through LDS (the next
// 32 are fetched into registers meanwhile); thread (line = tid / 8, rg = tid % 8) owns the rows rg + 8 i of its line
// and reads four points of the line and of each of its table rows per 16-byte LDS read
// ------------------------------------------------------------------------------------------------------------
template <int CIN>
__global__ __launch_bounds__(256) void k_lift_analysis(const float* __restrict__ u, const float* __restrict__ fa_y,
                                                       const float* __restrict__ fa_x, int ldn_y, int ldn_x,
                                                       float* __restrict__ s_y, float* __restrict__ s_x, int B, int M, int N, int R,
                                                       int nblk_y) {
  constexpr int LS = 32 * CIN + 4;                       // line stride in LDS: 16-byte aligned, the 8 lines of a wave on
  constexpr int TS = 36;                                 // different banks; likewise the table rows
  constexpr int NU = 32 * 32 * CIN / 256, NT = 6;        // floats per thread and chunk: field, table (R <= 48)
  __shared__ __attribute__((aligned(16))) float tab[48 * TS];                 // [r][yy]
  __shared__ __attribute__((aligned(16))) float tile[LIFT_LT * LS];           // [line][yy][c]
  const int tid = threadIdx.x;
  const int a = blockIdx.x >= nblk_y ? 1 : 0;
  const long l0 = (long)(a ? blockIdx.x - nblk_y : blockIdx.x) * LIFT_LT;
  const int n = a ? M : N;
  const float* __restrict__ fa = a ? fa_x : fa_y;
  const int ldn = a ? ldn_x : ldn_y;
  const int line = tid >> 3, rg = tid & 7, NI = R / 8;
  float acc[6][CIN];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int c = 0; c < CIN; ++c) acc[i][c] = 0.f;
  // y: lines (b, m0 .. m0 + 31), N * CIN floats apart;  x: lines (b, n0 .. n0 + 31), points N * CIN floats apart
  const long b = a ? l0 / N : l0 / M;
  const long r0 = a ? l0 % N : l0 % M;
  float ru[NU], rt[NT];
  auto fetch = [&](int y0) {
#pragma unroll
    for (int v = 0; v < NU; ++v) {
      const int e = tid + 256 * v, o = e / (32 * CIN), rem = e % (32 * CIN);
      ru[v] = !a ? u[((b * M + r0 + o) * N + y0) * CIN + rem]                  // o: line, rem: (yy, c)
                 : u[((b * M + y0 + o) * N + r0) * CIN + rem];                 // o: yy, rem: (line, c)
    }
#pragma unroll
    for (int v = 0; v < NT; ++v) {
      const int e = tid + 256 * v;
      rt[v] = e < 32 * R ? fa[(long)(e >> 5) * ldn + y0 + (e & 31)] : 0.f;
    }
  };
  fetch(0);
  for (int y0 = 0; y0 < n; y0 += 32) {
    __syncthreads();
#pragma unroll
    for (int v = 0; v < NU; ++v) {
      const int e = tid + 256 * v, o = e / (32 * CIN), rem = e % (32 * CIN);
      if (!a) tile[o * LS + rem] = ru[v];
      else tile[(rem / CIN) * LS + o * CIN + rem % CIN] = ru[v];
    }
#pragma unroll
    for (int v = 0; v < NT; ++v) {
      const int e = tid + 256 * v;
      if (e < 32 * R) tab[(e >> 5) * TS + (e & 31)] = rt[v];
    }
    __syncthreads();
    if (y0 + 32 < n) fetch(y0 + 32);
#pragma unroll 2
    for (int q = 0; q < 8; ++q) {
      float uv[4 * CIN];
#pragma unroll
      for (int c = 0; c < CIN; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(tile + line * LS + q * 4 * CIN + 4 * c);
        uv[4 * c] = v.x; uv[4 * c + 1] = v.y; uv[4 * c + 2] = v.z; uv[4 * c + 3] = v.w;
      }
#pragma unroll
      for (int i = 0; i < 6; ++i)
        if (i < NI) {
          const float4 t = *reinterpret_cast<const float4*>(tab + (rg + 8 * i) * TS + 4 * q);
          const float tv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
          for (int yy = 0; yy < 4; ++yy)
#pragma unroll
            for (int c = 0; c < CIN; ++c) acc[i][c] = fmaf(tv[yy], uv[yy * CIN + c], acc[i][c]);
        }
    }
  }
  float* __restrict__ s = (a ? s_x : s_y) + (l0 + line) * (long)R * CIN;
#pragma unroll
  for (int i = 0; i < 6; ++i)
    if (i < NI) {
#pragma unroll
      for (int c = 0; c < CIN; ++c) s[(rg + 8 * i) * CIN + c] = acc[i][c];
    }
}

// ------------------------------------------------------------------------------------------------------------
// W'[axis][k][j][o] (complex) = sum_i W~[i][j] Wmix_axis[i][o][k];  zero for the padding modes k >= keff
// wave q sums the 16 input channels 16 q .., the four partial sums are added in one fixed order
// ------------------------------------------------------------------------------------------------------------
template <int CIN>
__global__ __launch_bounds__(256) void k_lift_wprime(const float* __restrict__ w_in, const float* __restrict__ b_in,
                                                     const float* __restrict__ w_y, const float* __restrict__ w_x, int K, int keff,
                                                     int kp, float* __restrict__ wp) {
  constexpr int CA = CIN + 1;
  __shared__ float red[4][2 * CA][64];
  const int k = blockIdx.x, a = blockIdx.y, o = threadIdx.x & 63, q = threadIdx.x >> 6;
  const float* __restrict__ w = a ? w_x : w_y;
  float re[CA], im[CA];
#pragma unroll
  for (int j = 0; j < CA; ++j) re[j] = im[j] = 0.f;
  if (k < keff) {
#pragma unroll 16
    for (int i = 16 * q; i < 16 * q + 16; ++i) {
      const float2 v = *reinterpret_cast<const float2*>(w + ((long)(i * 64 + o) * K + k) * 2);
#pragma unroll
      for (int j = 0; j < CA; ++j) {
        const float t = j < CIN ? w_in[i * CIN + j] : (b_in ? b_in[i] : 0.f);
        re[j] = fmaf(t, v.x, re[j]);
        im[j] = fmaf(t, v.y, im[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < CA; ++j) { red[q][2 * j][o] = re[j]; red[q][2 * j + 1][o] = im[j]; }
  __syncthreads();
  if (q == 0) {
#pragma unroll
    for (int j = 0; j < CA; ++j)
      *reinterpret_cast<float2*>(wp + ((((long)a * kp + k) * CA + j) * 64 + o) * 2) =
          make_float2((red[0][2 * j][o] + red[1][2 * j][o]) + (red[2][2 * j][o] + red[3][2 * j][o]),
                      (red[0][2 * j + 1][o] + red[1][2 * j + 1][o]) + (red[2][2 * j + 1][o] + red[3][2 * j + 1][o]));
  }
}

// ------------------------------------------------------------------------------------------------------------
// thin mix: mixed[line][2k + part][o] = sum_j S_u~[line][k][j] W'[k][j][o], formed in registers in the lane layout of
// k_spec_split_h2 (thread (cb, g, li): channel 16 cb + li, rows 32 s + 8 g + j) and written as that kernel writes it:
// line scale from the line's own maximum, K32 hi + K32 lo fragments + packed tail per 16-channel block
// ------------------------------------------------------------------------------------------------------------
struct LiftMixP {
  const float* s[2]; char* img[2]; float* inv[2];
  const float* wp;
  long nblk_y;
  float sqn[2];
  int kp, R;
};

template <int K32, int TG, int CIN>
__global__ __launch_bounds__(256) void k_lift_mix(const LiftMixP P) {
  constexpr int NF = K32 + (TG ? 1 : 0);
  constexpr int CA = CIN + 1;
  typedef H2Block<K32, TG> L;
  __shared__ float sl[LIFT_ML * 48 * CIN];
  __shared__ float wmax[2][4];
  const int tid = threadIdx.x, l = tid & 63, cb = tid >> 6, g = l >> 4, li = l & 15;
  const int a = (long)blockIdx.x >= P.nblk_y ? 1 : 0;
  const long line0 = ((long)blockIdx.x - (a ? P.nblk_y : 0)) * LIFT_ML;
  const int R = P.R, o = 16 * cb + li;
  const float sqn = P.sqn[a];
  // this thread's W': modes 16 s + 4 g + jj (rows 32 s + 8 g + 2 jj, + 1)
  float2 wq[NF][4][CA];
#pragma unroll
  for (int s = 0; s < NF; ++s)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int k = 16 * s + 4 * g + jj;
#pragma unroll
      for (int j = 0; j < CA; ++j)
        wq[s][jj][j] = k < P.kp ? *reinterpret_cast<const float2*>(P.wp + ((((long)a * P.kp + k) * CA + j) * 64 + o) * 2)
                                : make_float2(0.f, 0.f);
    }
  {
    const float* __restrict__ src = P.s[a] + line0 * (long)R * CIN;
    for (int e = tid; e < LIFT_ML * R * CIN; e += 256) sl[e] = src[e];
  }
  __syncthreads();
  for (int t = 0; t < LIFT_ML; ++t) {
    const long line = line0 + t;
    const float* __restrict__ sp = sl + t * R * CIN;
    float v[NF][8];
    float m = 0.f;
#pragma unroll
    for (int s = 0; s < NF; ++s)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int k = 16 * s + 4 * g + jj;
        float re = 0.f, im = 0.f;
        if (k < P.kp) {
#pragma unroll
          for (int j = 0; j < CIN; ++j) {
            const float sr = sp[(2 * k) * CIN + j], si = sp[(2 * k + 1) * CIN + j];
            const float2 w = wq[s][jj][j];
            re = fmaf(sr, w.x, re); re = fmaf(-si, w.y, re);
            im = fmaf(sr, w.y, im); im = fmaf(si, w.x, im);
          }
          if (k == 0) { re = fmaf(sqn, wq[s][jj][CIN].x, re); im = fmaf(sqn, wq[s][jj][CIN].y, im); }
        }
        v[s][2 * jj] = re; v[s][2 * jj + 1] = im;
        m = fmaxf(m, fmaxf(fabsf(re), fabsf(im)));
      }
    m = wave_max(m);
    if (l == 0) wmax[t & 1][cb] = m;
    __syncthreads();                                     // (wmax is double buffered: one barrier per line)
    m = fmaxf(fmaxf(wmax[t & 1][0], wmax[t & 1][1]), fmaxf(wmax[t & 1][2], wmax[t & 1][3]));
    float scale, inv;
    h2_scale(m, H2_TABLE_EXP, scale, inv);
    if (tid == 0) P.inv[a][line] = inv;
    char* blk = P.img[a] + (line * 4 + cb) * (long)L::BYTES;
#pragma unroll
    for (int s = 0; s < NF; ++s) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[s][j] *= scale;
      uint4 hi, lo;
      h2_split8(v[s], hi, lo);
      if (s < K32) {
        *reinterpret_cast<uint4*>(blk + L::hi(s) + l * 16) = hi;
        *reinterpret_cast<uint4*>(blk + L::lo(s) + l * 16) = lo;
      } else if (g < TG) {
        L::template store_tail<false>(blk, g, li, hi, lo);
      }
    }
    if (TG > 0 && g == 0) L::zero_unused(blk, li);
  }
}

// ------------------------------------------------------------------------------------------------------------
// T partials: wave kg of a 512-thread workgroup owns the modes kg + 8 i, lane o the output channel; the S_u values are
// the same for the whole wave.  part[slab][axis][k][j < CA][o][re|im]; the constant channel j = Cin only at k = 0
// ------------------------------------------------------------------------------------------------------------
template <int CIN>
__global__ __launch_bounds__(512) void k_lift_tgrad(const float* __restrict__ g_y, const float* __restrict__ g_x,
                                                    const float* __restrict__ s_y, const float* __restrict__ s_x, long lines_y,
                                                    long lines_x, int kp, float sqn_y, float sqn_x, int S, float* __restrict__ part) {
  constexpr int CA = CIN + 1;
  const int o = threadIdx.x & 63, kg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int slab = blockIdx.x, a = blockIdx.y, R = 2 * kp;
  const long lines = a ? lines_x : lines_y;
  const float* __restrict__ G = a ? g_x : g_y;
  const float* __restrict__ Su = a ? s_x : s_y;
  const long lps = (lines + S - 1) / S, t0 = slab * lps, t1 = min(t0 + lps, lines);
  float tre[3][CA], tim[3][CA];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < CA; ++j) tre[i][j] = tim[i][j] = 0.f;
  // two lines per pass: twelve loads of the g-spectra in flight per thread
  for (long t = t0; t < t1; t += 2) {
    const bool two = t + 1 < t1;
    float gre[2][3], gim[2][3];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float* __restrict__ gl = G + (t + h) * (long)R * 64 + o;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int k = kg + 8 * i;
        const bool on = k < kp && (h == 0 || two);
        gre[h][i] = on ? gl[(2 * k) * 64] : 0.f;
        gim[h][i] = on ? gl[(2 * k + 1) * 64] : 0.f;
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (h == 1 && !two) break;
      const float* __restrict__ sp = Su + (t + h) * (long)R * CIN;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int k = kg + 8 * i;
        if (k < kp) {
#pragma unroll
          for (int j = 0; j < CIN; ++j) {
            const float sr = sp[(2 * k) * CIN + j], si = sp[(2 * k + 1) * CIN + j];
            tre[i][j] = fmaf(sr, gre[h][i], tre[i][j]); tre[i][j] = fmaf(si, gim[h][i], tre[i][j]);
            tim[i][j] = fmaf(sr, gim[h][i], tim[i][j]); tim[i][j] = fmaf(-si, gre[h][i], tim[i][j]);
          }
          tre[i][CIN] += gre[h][i]; tim[i][CIN] += gim[h][i];
        }
      }
    }
  }
  const float sqn = a ? sqn_x : sqn_y;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int k = kg + 8 * i;
    if (k < kp) {
      float* __restrict__ dst = part + ((((long)slab * 2 + a) * kp + k) * CA) * 128 + o * 2;
#pragma unroll
      for (int j = 0; j < CA; ++j) {
        const float f = j < CIN ? 1.f : (k == 0 ? sqn : 0.f);
        *reinterpret_cast<float2*>(dst + j * 128) = make_float2(tre[i][j] * f, tim[i][j] * f);
      }
    }
  }
}

// gw[i][o][k][2] = sum_j W~[i][j] T[axis][k][j][o];  zero for k >= keff
template <int CIN>
__global__ __launch_bounds__(256) void k_lift_chain_w(const float* __restrict__ T, const float* __restrict__ w_in,
                                                      const float* __restrict__ b_in, float* __restrict__ gw_y,
                                                      float* __restrict__ gw_x, int K, int keff, int kp) {
  constexpr int CA = CIN + 1;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;        // (i * 64 + o) * K + k
  const int a = blockIdx.y;
  float* __restrict__ gw = a ? gw_x : gw_y;
  if (idx >= 4096L * K || !gw) return;
  const int k = (int)(idx % K), o = (int)((idx / K) & 63), i = (int)(idx / K / 64);
  float2 acc = make_float2(0.f, 0.f);
  if (k < keff) {
#pragma unroll
    for (int j = 0; j < CA; ++j) {
      const float t = j < CIN ? w_in[i * CIN + j] : (b_in ? b_in[i] : 0.f);
      const float2 v = *reinterpret_cast<const float2*>(T + ((((long)a * kp + k) * CA + j) * 64 + o) * 2);
      acc.x = fmaf(t, v.x, acc.x); acc.y = fmaf(t, v.y, acc.y);
    }
  }
  *reinterpret_cast<float2*>(gw + idx * 2) = acc;
}

// gW~[i][j] = sum_{axis, k < keff, o} (Wr T_re + Wi T_im): one workgroup per i, a fixed tree over its 256 partial sums
template <int CIN>
__global__ __launch_bounds__(256) void k_lift_chain_in(const float* __restrict__ T, const float* __restrict__ w_y,
                                                       const float* __restrict__ w_x, float* __restrict__ gw_in,
                                                       float* __restrict__ gb_in, int K, int keff, int kp) {
  constexpr int CA = CIN + 1;
  __shared__ float red[CA][256];
  const int i = blockIdx.x, tid = threadIdx.x;
  float acc[CA];
#pragma unroll
  for (int j = 0; j < CA; ++j) acc[j] = 0.f;
  for (int e = tid; e < 2 * keff * 64; e += 256) {
    const int o = e & 63, k = (e >> 6) % keff, a = (e >> 6) / keff;
    const float2 w = *reinterpret_cast<const float2*>((a ? w_x : w_y) + ((long)(i * 64 + o) * K + k) * 2);
#pragma unroll
    for (int j = 0; j < CA; ++j) {
      const float2 v = *reinterpret_cast<const float2*>(T + ((((long)a * kp + k) * CA + j) * 64 + o) * 2);
      acc[j] = fmaf(w.x, v.x, acc[j]); acc[j] = fmaf(w.y, v.y, acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < CA; ++j) red[j][tid] = acc[j];
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int j = 0; j < CA; ++j) red[j][tid] += red[j][tid + h];
    }
    __syncthreads();
  }
  if (tid < CIN && gw_in) gw_in[i * CIN + tid] = red[tid][0];
  if (tid == CIN && gb_in) gb_in[i] = red[CIN][0];
}

// ------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------
// slabs of lines of the T kernel: a function of the shape alone (the fold order must not depend on the device)
static int lift_slabs(const LiftGeom& g) {
  const long fewest = g.lines[0] < g.lines[1] ? g.lines[0] : g.lines[1];
  long S = fewest / 8;
  if (S > 256) S = 256;
  if (S < 1) S = 1;
  return (int)S;
}
static size_t lift_t_floats(const LiftGeom& g, int Cin) { return (size_t)2 * g.kp * (Cin + 1) * 128; }
static size_t lift_spec_floats(const LiftGeom& g, int Cin, int axis) { return (size_t)g.lines[axis] * g.R * Cin; }

// forward: W', both axes' operand blocks and line scales
struct LiftFwdWork {
  float* wp; void *imgy, *imgx; float *invy, *invx;
  LiftFwdWork(Arena& ar, const LiftGeom& g, int Cin)
      : wp(ar.take(lift_t_floats(g, Cin))), imgy(ar.take(fused2d_img_bytes(g.lines[0], g.R) / 4)),
        imgx(ar.take(fused2d_img_bytes(g.lines[1], g.R) / 4)), invy(ar.take(g.lines[0])), invx(ar.take(g.lines[1])) {}
};
// backward: the g-spectra, the slab partials of T, T
struct LiftBwdWork {
  int S; float *gsy, *gsx, *part, *T;
  LiftBwdWork(Arena& ar, const LiftGeom& g, int Cin)
      : S(lift_slabs(g)), gsy(ar.take((size_t)g.lines[0] * g.R * 64)), gsx(ar.take((size_t)g.lines[1] * g.R * 64)),
        part(ar.take((size_t)S * lift_t_floats(g, Cin))), T(ar.take(lift_t_floats(g, Cin))) {}
};

#define RPDE_LIFT_CIN(Cin, CALL)                  \
  do {                                            \
    switch (Cin) {                                \
      case 1: { constexpr int CIN = 1; CALL; } break; \
      case 2: { constexpr int CIN = 2; CALL; } break; \
      case 3: { constexpr int CIN = 3; CALL; } break; \
      default: { constexpr int CIN = 4; CALL; } break; \
    }                                             \
  } while (0)

static int lift_plans(const LiftGeom& g, const rpde_plan** py, const rpde_plan** px, hipStream_t st) {
  RPDE_TRY(get_plan(py, g.n[0], g.keff, RPDE_NORM_ORTHO, 0, PLAN_REAL, st));
  return get_plan(px, g.n[1], g.keff, RPDE_NORM_ORTHO, 0, PLAN_REAL, st);
}

// the larger of the two layouts at the widest input: a piece of rpde_fspectral2d_ws_bytes (fspectral.hip), the one
// workspace query of the 2-D layer
size_t lifted2d_ws_bytes(int B, int M, int N, int K) {
  const LiftGeom g = lift_geom(B, M, N, K);
  return ws_max(ws_measure<LiftFwdWork>(g, LIFT_MAXC), ws_measure<LiftBwdWork>(g, LIFT_MAXC));
}

}  // namespace rpde

using namespace rpde;

extern "C" {

// RPDE_LIFTED_SPECTRAL=0: layer 0 keeps the 64-channel path (A/B, tests)
int rpde_lifted_fspectral2d_ok(int M, int N, int C, int Cin, int K) {
  if (switch_off("RPDE_LIFTED_SPECTRAL") || M <= 0 || N <= 0 || K <= 0 || Cin < 1 || Cin > LIFT_MAXC) return 0;
  const int ky = K < N / 2 + 1 ? K : N / 2 + 1, kx = K < M / 2 + 1 ? K : M / 2 + 1;
  return fused2d_ok(M, N, C, ky, kx) ? 1 : 0;
}

// floats of the saved spectra: the y lines' [B*M][2kp][Cin], then the x lines' [B*N][2kp][Cin]
size_t rpde_lifted_fspectral2d_spec_elems(int B, int M, int N, int Cin, int K) {
  const LiftGeom g = lift_geom(B, M, N, K);
  return lift_spec_floats(g, Cin, 0) + lift_spec_floats(g, Cin, 1);
}

int rpde_lifted_fspectral2d_fwd(const float* u, const float* w_in, const float* b_in, const float* w_y, const float* w_x,
                                float* out, float* spec_u, int B, int M, int N, int C, int Cin, int K, void* ws,
                                size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(u && w_in && w_y && w_x && out && spec_u && B > 0, "lifted_fspectral2d_fwd: bad arguments");
  RPDE_CHECK_ARG(rpde_lifted_fspectral2d_ok(M, N, C, Cin, K), "lifted_fspectral2d_fwd: shape not on the lifted path");
  const LiftGeom g = lift_geom(B, M, N, K);
  RPDE_CARVE("lifted_fspectral2d_fwd", LiftFwdWork, wk, ws, ws_bytes, g, Cin);
  hipStream_t st = as_stream(stream);
  const rpde_plan *py, *px;
  RPDE_TRY(lift_plans(g, &py, &px, st));
  float* s_y = spec_u;
  float* s_x = spec_u + lift_spec_floats(g, Cin, 0);
  const int nby = (int)(g.lines[0] / LIFT_LT), nbx = (int)(g.lines[1] / LIFT_LT);
  RPDE_LIFT_CIN(Cin, hipLaunchKernelGGL(k_lift_analysis<CIN>, dim3(nby + nbx), dim3(256), 0, st, u, py->fa, px->fa, py->ldn,
                                        px->ldn, s_y, s_x, B, M, N, g.R, nby));
  RPDE_LAUNCH_CHECK();
  RPDE_LIFT_CIN(Cin, hipLaunchKernelGGL(k_lift_wprime<CIN>, dim3(g.kp, 2), dim3(256), 0, st, w_in, b_in, w_y, w_x, K, g.keff, g.kp,
                                        wk.wp));
  RPDE_LAUNCH_CHECK();
  LiftMixP P;
  P.s[0] = s_y; P.s[1] = s_x; P.img[0] = (char*)wk.imgy; P.img[1] = (char*)wk.imgx; P.inv[0] = wk.invy; P.inv[1] = wk.invx;
  P.wp = wk.wp; P.nblk_y = g.lines[0] / LIFT_ML; P.sqn[0] = sqrtf((float)g.n[0]); P.sqn[1] = sqrtf((float)g.n[1]);
  P.kp = g.kp; P.R = g.R;
  const dim3 mgrid((unsigned)(g.lines[0] / LIFT_ML + g.lines[1] / LIFT_ML));
  RPDE_LIFT_CIN(Cin, h2_dispatch(g.R, [&](auto k32, auto tg) {
                  hipLaunchKernelGGL((k_lift_mix<k32(), tg(), CIN>), mgrid, dim3(256), 0, st, P);
                }));
  RPDE_LAUNCH_CHECK();
  return fused2d_synthesis(wk.imgy, wk.imgx, wk.invy, wk.invx, py, px, 0, out, nullptr, B, M, N, st);
}

int rpde_lifted_fspectral2d_bwd(const float* grad_out, const float* spec_u, const float* w_in, const float* b_in,
                                const float* w_y, const float* w_x, float* grad_w_in, float* grad_b_in, float* grad_wy,
                                float* grad_wx, int B, int M, int N, int C, int Cin, int K, void* ws, size_t ws_bytes,
                                void* stream) {
  RPDE_CHECK_ARG(grad_out && spec_u && w_in && w_y && w_x && B > 0, "lifted_fspectral2d_bwd: bad arguments");
  RPDE_CHECK_ARG(rpde_lifted_fspectral2d_ok(M, N, C, Cin, K), "lifted_fspectral2d_bwd: shape not on the lifted path");
  const LiftGeom g = lift_geom(B, M, N, K);
  RPDE_CARVE("lifted_fspectral2d_bwd", LiftBwdWork, wk, ws, ws_bytes, g, Cin);
  hipStream_t st = as_stream(stream);
  const rpde_plan *py, *px;
  RPDE_TRY(lift_plans(g, &py, &px, st));
  const float* s_y = spec_u;
  const float* s_x = spec_u + lift_spec_floats(g, Cin, 0);
  RPDE_TRY(fused2d_analysis(grad_out, wk.gsy, wk.gsx, nullptr, nullptr, py, px, 1, B, M, N, st));
  RPDE_LIFT_CIN(Cin, hipLaunchKernelGGL(k_lift_tgrad<CIN>, dim3(wk.S, 2), dim3(512), 0, st, wk.gsy, wk.gsx, s_y, s_x, g.lines[0],
                                        g.lines[1], g.kp, sqrtf((float)g.n[0]), sqrtf((float)g.n[1]), wk.S, wk.part));
  RPDE_LAUNCH_CHECK();
  const long n_out = (long)lift_t_floats(g, Cin);
  RPDE_TRY(reduce_slabs(wk.part, wk.T, n_out, wk.S, n_out, 1.f, 0, st));      // T[e] = sum_slab part[slab][e]
  if (grad_wy || grad_wx) {
    RPDE_LIFT_CIN(Cin, hipLaunchKernelGGL(k_lift_chain_w<CIN>, dim3((unsigned)((4096L * K + 255) / 256), 2), dim3(256), 0, st, wk.T,
                                          w_in, b_in, grad_wy, grad_wx, K, g.keff, g.kp));
    RPDE_LAUNCH_CHECK();
  }
  if (grad_w_in || grad_b_in) {
    RPDE_LIFT_CIN(Cin, hipLaunchKernelGGL(k_lift_chain_in<CIN>, dim3(64), dim3(256), 0, st, wk.T, w_y, w_x, grad_w_in, grad_b_in, K,
                                          g.keff, g.kp));
    RPDE_LAUNCH_CHECK();
  }
  return RPDE_OK;
}

}  // extern "C"
