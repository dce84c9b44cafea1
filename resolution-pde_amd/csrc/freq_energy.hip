// Error and solution energy per Fourier mode (1-D) or per radial frequency bin (2-D): the numbers behind the reference's
// utils/frequency_error.py (decompose_error_by_frequency_1d / _2d), which takes one inverse FFT of the whole batch and
// one host synchronisation per mode or per bin.  By Parseval the norm of a band-limited reconstruction is the weighted
// energy of its retained modes, so all of it is ONE forward transform, a square and a small reduction:
//
//   1-D  E[k] = w_k / n      sum_rows |Z[row, k]|^2                      Z = rfft(z),   w = 1 at DC / Nyquist, else 2
//   2-D  E[i] = 1 / (H W)    sum_{(ky,kx) in bin i} w_kx sum_img |Z[img, ky, kx]|^2     Z = rfft2(z)
//
// for z = prediction - target (formed in fp32 BEFORE the transform: exact by Sterbenz for a decent model, where
// subtracting two spectra loses the digits) and z = target.  The transform is the DFT as a matrix product in h2
// arithmetic (h2.h), full spectrum, tables from the plan cache (plan.h) as f16 hi/lo fragments (cf_dft.h).
//
// One kernel, k_fe, does every product.  The TABLE is the A operand (16 outputs r per tile, streamed from L2 as ready
// fragments: at full spectrum it does not fit LDS) and the FIELD is the B operand: a workgroup stages 16 rows x 256
// points of both fields in LDS (difference, one power-of-two scale per field and block, f16 split), its four waves take
// NTW output tiles each.  So lane (g, li) of an accumulator holds outputs r = 16 nt + 4 g + j of field row li:
//   energy epilogue:  square, add up over the workgroup's row tiles in registers, one 16-lane DPP sum at the end, and
//                     lane 15 writes the workgroup's partial -- no atomics; k_fe_fold* add the partials up in a fixed
//                     order in float64 and add them into the caller's accumulator: identical calls give identical bits;
//   spectrum epilogue (2-D row stage): (re, im) pairs of column kx go to ws[kx][image][2 h + ri], 128 contiguous bytes
//                     per 16 lanes, which is the row layout the column stage (complex plan keeping every row) reads.
// The 2-D evaluator walks the batch in chunks of images whose half-spectra stay in L2 / MALL: the workspace does not
// grow with the batch, prediction and target are read once.
#include "freq_energy.h"
#include "cf_dft.h"
#include "h2.h"
#include "plan.h"
#include "pointwise.h"

#include <map>
#include <mutex>

namespace rpde {

constexpr int FE_KC = 8;             // reduction steps (of 32 points) per staged block: 256 points
constexpr int FE_SLOTS_1D = 64;      // partial sums per output, 1-D (workgroups along the rows)
constexpr int FE_SLOTS_2D = 8;       // ... per column kx, 2-D
constexpr int FE_MAX_N = 4096;       // per axis: the full-spectrum tables are quadratic in it (64 MiB each at 4096)

struct FeP {
  const float* a; const float* b;    // two fields, rows [groups * rpg][K]
  const char* timg;                  // table fragments [KS][NT][hi|lo][1 KB]
  float* out0; float* out1;          // spectrum epilogue: the two spectra; energy epilogue: out0 = partials
  int K, KS, NT;
  int rpg, tiles, S;                 // rows per group, 16-row tiles per group, workgroups per group (gridDim.x)
  int H, KW, bcc;                    // spectrum epilogue: row = image * H + h, KW columns kept, bcc images in the chunk
  int vec;                           // rows are 16-byte aligned and K % 4 == 0
};

__device__ __forceinline__ float4 fe_load4(const float* __restrict__ p, int k0, int K, bool rok, int vec) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!rok) return v;
  if (vec) {
    if (k0 < K) v = *reinterpret_cast<const float4*>(p + k0);
  } else {
    if (k0 < K) v.x = p[k0];
    if (k0 + 1 < K) v.y = p[k0 + 1];
    if (k0 + 2 < K) v.z = p[k0 + 2];
    if (k0 + 3 < K) v.w = p[k0 + 3];
  }
  return v;
}
__device__ __forceinline__ float fe_absmax4(float m, float4 v) {
  return fmaxf(fmaxf(fmaxf(m, fabsf(v.x)), fmaxf(fabsf(v.y), fabsf(v.z))), fabsf(v.w));
}

template <bool DIFF, bool SPEC, int NTW>
__global__ __launch_bounds__(256) void k_fe(const FeP P) {
  __shared__ __attribute__((aligned(16))) char smem[2 * FE_KC * 2048];       // [field][ks][hi|lo][1 KB]
  __shared__ float smax[2][4];
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, g = l >> 4, li = l & 15;
  const int nt0 = ((int)blockIdx.y * 4 + w) * NTW;
  const long grow0 = (long)blockIdx.z * P.rpg;
  const int nchunk = (P.KS + FE_KC - 1) / FE_KC;
  float e[NTW][2][4];
#pragma unroll
  for (int i = 0; i < NTW; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) e[i][0][j] = e[i][1][j] = 0.f;

  for (int tile = blockIdx.x; tile < P.tiles; tile += P.S) {
    const int r = tile * 16 + li;
    const bool rok = r < P.rpg;
    const float* __restrict__ pa = P.a + (grow0 + (rok ? r : 0)) * P.K;
    const float* __restrict__ pb = P.b + (grow0 + (rok ? r : 0)) * P.K;
    f32x4v tot[NTW][2];
#pragma unroll
    for (int i = 0; i < NTW; ++i) tot[i][0] = tot[i][1] = (f32x4v){0.f, 0.f, 0.f, 0.f};
    // wave w stages the half-steps q = w + 4 i of a block: step q >> 1, points 16 (q & 1) + 4 g .. + 3 of it (frag_perm)
    float4 na[4], nb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = w + 4 * i, k0 = (q >> 1) * 32 + 16 * (q & 1) + 4 * g;
      na[i] = fe_load4(pa, k0, P.K, rok, P.vec);
      nb[i] = fe_load4(pb, k0, P.K, rok, P.vec);
    }
    for (int c = 0; c < nchunk; ++c) {
      float4 ca[4], cb[4];
      float m0 = 0.f, m1 = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ca[i] = na[i]; cb[i] = nb[i];
        if (DIFF) { ca[i].x -= cb[i].x; ca[i].y -= cb[i].y; ca[i].z -= cb[i].z; ca[i].w -= cb[i].w; }
        m0 = fe_absmax4(m0, ca[i]);
        m1 = fe_absmax4(m1, cb[i]);
      }
      if (c + 1 < nchunk) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int q = w + 4 * i, k0 = ((c + 1) * FE_KC + (q >> 1)) * 32 + 16 * (q & 1) + 4 * g;
          na[i] = fe_load4(pa, k0, P.K, rok, P.vec);
          nb[i] = fe_load4(pb, k0, P.K, rok, P.vec);
        }
      }
      m0 = wave_max(m0);
      m1 = wave_max(m1);
      __syncthreads();                       // the previous block's products have read smem and smax
      if (l == 0) { smax[0][w] = m0; smax[1][w] = m1; }
      __syncthreads();
      m0 = fmaxf(fmaxf(smax[0][0], smax[0][1]), fmaxf(smax[0][2], smax[0][3]));
      m1 = fmaxf(fmaxf(smax[1][0], smax[1][1]), fmaxf(smax[1][2], smax[1][3]));
      float sc0, inv0, sc1, inv1;
      h2_scale(m0, H2_TABLE_EXP, sc0, inv0);
      h2_scale(m1, H2_TABLE_EXP, sc1, inv1);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int q = w + 4 * i;
        uint2 hi, lo;
        char* d = smem + (q >> 1) * 2048 + l * 16 + (q & 1) * 8;
        h2_split4(ca[i].x * sc0, ca[i].y * sc0, ca[i].z * sc0, ca[i].w * sc0, hi, lo);
        *reinterpret_cast<uint2*>(d) = hi;
        *reinterpret_cast<uint2*>(d + 1024) = lo;
        h2_split4(cb[i].x * sc1, cb[i].y * sc1, cb[i].z * sc1, cb[i].w * sc1, hi, lo);
        *reinterpret_cast<uint2*>(d + FE_KC * 2048) = hi;
        *reinterpret_cast<uint2*>(d + FE_KC * 2048 + 1024) = lo;
      }
      __syncthreads();
      f32x4v acc[NTW][2];
#pragma unroll
      for (int i = 0; i < NTW; ++i) acc[i][0] = acc[i][1] = (f32x4v){0.f, 0.f, 0.f, 0.f};
      const int ksn = min(FE_KC, P.KS - c * FE_KC);
      for (int ks = 0; ks < ksn; ++ks) {
        const char* f = smem + ks * 2048 + l * 16;
        const f16x8 f0h = *reinterpret_cast<const f16x8*>(f), f0l = *reinterpret_cast<const f16x8*>(f + 1024);
        const f16x8 f1h = *reinterpret_cast<const f16x8*>(f + FE_KC * 2048);
        const f16x8 f1l = *reinterpret_cast<const f16x8*>(f + FE_KC * 2048 + 1024);
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
          if (nt0 + i < P.NT) {
            const char* t = P.timg + ((long)(c * FE_KC + ks) * P.NT + nt0 + i) * 2048 + l * 16;
            const f16x8 th = *reinterpret_cast<const f16x8*>(t), tl = *reinterpret_cast<const f16x8*>(t + 1024);
            acc[i][0] = h2_mfma32(th, tl, f0h, f0l, acc[i][0]);
            acc[i][1] = h2_mfma32(th, tl, f1h, f1l, acc[i][1]);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < NTW; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          tot[i][0][j] = fmaf(acc[i][0][j], inv0, tot[i][0][j]);
          tot[i][1][j] = fmaf(acc[i][1][j], inv1, tot[i][1][j]);
        }
    }
    if (SPEC) {
      if (rok) {
        const int img = r / P.H, h = r - img * P.H;
#pragma unroll
        for (int i = 0; i < NTW; ++i)
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) {
            const int kx = 8 * (nt0 + i) + 2 * g + jj;
            if (nt0 + i < P.NT && kx < P.KW) {
              const long o = ((long)kx * P.bcc + img) * (2L * P.H) + 2 * h;
              *reinterpret_cast<float2*>(P.out0 + o) = make_float2(tot[i][0][2 * jj], tot[i][0][2 * jj + 1]);
              *reinterpret_cast<float2*>(P.out1 + o) = make_float2(tot[i][1][2 * jj], tot[i][1][2 * jj + 1]);
            }
          }
      }
    } else {
#pragma unroll
      for (int i = 0; i < NTW; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          e[i][0][j] = fmaf(tot[i][0][j], tot[i][0][j], e[i][0][j]);
          e[i][1][j] = fmaf(tot[i][1][j], tot[i][1][j], e[i][1][j]);
        }
    }
  }
  if (!SPEC) {
    const int npad = P.NT * 16;
    float* part = P.out0 + ((long)blockIdx.z * P.S + blockIdx.x) * 2 * npad;
#pragma unroll
    for (int i = 0; i < NTW; ++i)
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float s = e[i][f][j];                     // sum over the 16 rows of the tile: lane 15 of each row of lanes
          s = dpp_add_step<0x111, 0xf>(s);
          s = dpp_add_step<0x112, 0xf>(s);
          s = dpp_add_step<0x114, 0xf>(s);
          s = dpp_add_step<0x118, 0xf>(s);
          v[j] = s;
        }
        if (li == 15 && nt0 + i < P.NT)
          *reinterpret_cast<float4*>(part + f * npad + 16 * (nt0 + i) + 4 * g) = make_float4(v[0], v[1], v[2], v[3]);
      }
  }
}

// acc[f][k] += w_k / n * sum_s (part[s][f][2k] + part[s][f][2k+1]), in float64 and in the order of s
__global__ __launch_bounds__(256) void k_fe_fold1d(const float* __restrict__ part, int S, int npad, int modes, int n,
                                                   double* __restrict__ acc) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * modes) return;
  const int f = idx / modes, k = idx - f * modes;
  double s = 0.0;
  for (int q = 0; q < S; ++q) {
    const float* p = part + ((long)q * 2 + f) * npad + 2 * k;
    s += (double)p[0] + (double)p[1];
  }
  const double wk = (k == 0 || (n % 2 == 0 && k == n / 2)) ? 1.0 : 2.0;
  acc[idx] += s * wk / (double)n;
}

// one workgroup per (bin, field): thread t walks the entries t, t + 256, .. of the [H, KW] bin table, takes those of its
// bin from the partials [kx][s][f][2 ky + ri], and the 256 sums meet in a fixed tree
__global__ __launch_bounds__(256) void k_fe_fold2d(const float* __restrict__ part, const int* __restrict__ bins, int S,
                                                   int npad, int H, int KW, int W, int n_bins, double* __restrict__ acc) {
  __shared__ double red[256];
  const int bin = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
  double s = 0.0;
  for (int en = t; en < H * KW; en += 256) {
    if (bins[en] != bin) continue;
    const int ky = en / KW, kx = en - ky * KW;
    double v = 0.0;
    for (int q = 0; q < S; ++q) {
      const float* p = part + (((long)kx * S + q) * 2 + f) * npad + 2 * ky;
      v += (double)p[0] + (double)p[1];
    }
    s += ((kx == 0 || (W % 2 == 0 && kx == W / 2)) ? 1.0 : 2.0) * v;
  }
  red[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) acc[f * n_bins + bin] += red[0] / ((double)H * (double)W);
}

// ---- host side --------------------------------------------------------------
static std::mutex g_fe_mu;
static std::map<const void*, char*> g_fe_img;      // table of a cached plan -> its fragments; never freed, like the plans

// fragments of src[r*rs + y] (r < R, y < n), built once per table on the calling stream (one synchronisation, as
// get_plan does for the tables themselves)
static int fe_fragments(const char** out, const float* src, long rs, int R, int n, hipStream_t st) {
  std::lock_guard<std::mutex> lk(g_fe_mu);
  auto it = g_fe_img.find(src);
  if (it != g_fe_img.end()) { *out = it->second; return RPDE_OK; }
  char* img = nullptr;
  RPDE_HIP(hipMalloc(&img, cf_table_bytes(R, n)));
  RPDE_TRY(cf_table_fragments(src, rs, 1L, R, n, img, st));
  RPDE_HIP(hipStreamSynchronize(st));
  g_fe_img[src] = img;
  *out = img;
  return RPDE_OK;
}

// output tiles per wave.  Few workgroups (a Burgers batch is four row tiles): one, so that the tiles spread over the
// chip.  Otherwise four or five, whichever needs fewer workgroups along the outputs -- every one of them stages the row
// tile again, and the power-of-two grids have one tile more than a multiple of 16 (NT = 17 at W = 256, 65 at n = 1024,
// from the Nyquist mode): five per wave serve those from ONE staging (four of them at n = 1024 instead of five).
template <bool DIFF, bool SPEC>
static int fe_launch(const FeP& P, int groups, hipStream_t st) {
  const int ng4 = (P.NT + 15) / 16, ng5 = (P.NT + 19) / 20;
  const int ng = ng5 < ng4 ? ng5 : ng4;
  int cus;
  (void)cu_count(&cus);
  if ((long)P.S * ng * groups < cus)
    hipLaunchKernelGGL((k_fe<DIFF, SPEC, 1>), dim3(P.S, (P.NT + 3) / 4, groups), dim3(256), 0, st, P);
  else if (ng5 < ng4) hipLaunchKernelGGL((k_fe<DIFF, SPEC, 5>), dim3(P.S, ng5, groups), dim3(256), 0, st, P);
  else hipLaunchKernelGGL((k_fe<DIFF, SPEC, 4>), dim3(P.S, ng4, groups), dim3(256), 0, st, P);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int fe_chunk_images(long images, int H, int W) {
  const size_t per = (size_t)2 * (W / 2 + 1) * 2 * H * sizeof(float);
  long c = (long)(FE_SPEC_BYTES / per);
  if (c >= 16) c = c / 16 * 16;
  if (c < 1) c = 1;
  return (int)(images < c ? images : c);
}

}  // namespace rpde

using namespace rpde;

extern "C" {

// the slots' partial energies of both fields
struct Fe1dWork {
  float* part;
  Fe1dWork(Arena& ar, int64_t rows, int num_modes) {
    const long tiles = (rows + 15) / 16;
    const int S = (int)(tiles < FE_SLOTS_1D ? tiles : FE_SLOTS_1D), NT = (2 * r4(num_modes) + 15) / 16;
    part = ar.take((size_t)S * 2 * NT * 16);
  }
};

size_t rpde_freq_energy1d_ws_bytes(int64_t rows, int n, int num_modes) {
  if (rows < 1 || n < 2 || n > FE_MAX_N || num_modes < 1) return 0;
  return ws_measure<Fe1dWork>(rows, num_modes);
}

int rpde_freq_energy1d(const float* pred, const float* target, double* acc, int64_t rows, int n, int num_modes,
                       void* ws, size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(pred && target && acc, "freq_energy1d: null pointer");
  RPDE_CHECK_ARG(rows >= 1 && rows < (1L << 31) && n >= 2 && n <= FE_MAX_N && num_modes >= 1,
                 "freq_energy1d: bad rows=%ld n=%d (2 .. %d) num_modes=%d", (long)rows, n, FE_MAX_N, num_modes);
  if (num_modes > n / 2 + 1) { set_error("freq_energy1d: num_modes %d exceed n/2+1 = %d", num_modes, n / 2 + 1); return RPDE_ERR_MODES; }
  RPDE_CARVE("freq_energy1d", Fe1dWork, w, ws, ws_bytes, rows, num_modes);
  RPDE_CHECK_ARG(al16(ws), "freq_energy1d: the workspace must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const rpde_plan* pl;
  RPDE_TRY(get_plan(&pl, n, num_modes, RPDE_NORM_BACKWARD, 0, PLAN_REAL, st));
  FeP P;
  memset(&P, 0, sizeof(P));
  RPDE_TRY(fe_fragments(&P.timg, pl->fa, pl->ldn, 2 * pl->kp, n, st));
  P.a = pred; P.b = target; P.out0 = w.part;
  P.K = n; P.KS = (n + 31) / 32; P.NT = (2 * pl->kp + 15) / 16;
  P.rpg = (int)rows; P.tiles = (int)((rows + 15) / 16); P.S = P.tiles < FE_SLOTS_1D ? P.tiles : FE_SLOTS_1D;
  P.vec = n % 4 == 0 && al16(pred) && al16(target);
  RPDE_TRY((fe_launch<true, false>(P, 1, st)));
  hipLaunchKernelGGL(k_fe_fold1d, dim3((2 * num_modes + 255) / 256), dim3(256), 0, st, P.out0, P.S, P.NT * 16, num_modes, n, acc);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

// a chunk's half-spectra of both fields and the slots' partial energies
struct Fe2dWork {
  float *s0, *s1, *part;
  Fe2dWork(Arena& ar, int64_t images, int H, int W) {
    const int cs = fe_chunk_images(images, H, W), KW = W / 2 + 1;
    const int tiles = (cs + 15) / 16, S = tiles < FE_SLOTS_2D ? tiles : FE_SLOTS_2D, NT = (2 * H + 15) / 16;
    s0 = ar.take((size_t)KW * cs * 2 * H);
    s1 = ar.take((size_t)KW * cs * 2 * H);
    part = ar.take((size_t)KW * S * 2 * NT * 16);
  }
};

size_t rpde_freq_energy2d_ws_bytes(int64_t images, int H, int W) {
  if (images < 1 || H < 2 || W < 2 || H > FE_MAX_N || W > FE_MAX_N) return 0;
  return ws_measure<Fe2dWork>(images, H, W);
}

int rpde_freq_energy2d(const float* pred, const float* target, const int32_t* bins, double* acc, int64_t images, int H,
                       int W, int n_bins, void* ws, size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(pred && target && bins && acc, "freq_energy2d: null pointer");
  RPDE_CHECK_ARG(images >= 1 && H >= 2 && W >= 2 && H <= FE_MAX_N && W <= FE_MAX_N && n_bins >= 1 && n_bins <= 65535 &&
                     images * H < (1L << 31),
                 "freq_energy2d: bad images=%ld H=%d W=%d (2 .. %d) n_bins=%d", (long)images, H, W, FE_MAX_N, n_bins);
  RPDE_CARVE("freq_energy2d", Fe2dWork, w, ws, ws_bytes, images, H, W);
  RPDE_CHECK_ARG(al16(ws), "freq_energy2d: the workspace must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const int KW = W / 2 + 1, cs = fe_chunk_images(images, H, W);
  const rpde_plan *pw, *ph;
  RPDE_TRY(get_plan(&pw, W, KW, RPDE_NORM_BACKWARD, 0, PLAN_REAL, st));
  RPDE_TRY(get_plan(&ph, H, H, RPDE_NORM_BACKWARD, 0, PLAN_CPLX, st, 0));
  const char *tw, *th;
  RPDE_TRY(fe_fragments(&tw, pw->fa, pw->ldn, 2 * pw->kp, W, st));
  RPDE_TRY(fe_fragments(&th, ph->fa, ph->ldn, 2 * H, 2 * H, st));
  const int NT2 = (2 * H + 15) / 16;
  for (int64_t i0 = 0; i0 < images; i0 += cs) {
    const int c = (int)(images - i0 < cs ? images - i0 : cs);
    // rows along W: [c * H, W] -> both half-spectra, [kx][image][2 h + ri]
    FeP P;
    memset(&P, 0, sizeof(P));
    P.a = pred + i0 * H * W; P.b = target + i0 * H * W; P.timg = tw; P.out0 = w.s0; P.out1 = w.s1;
    P.K = W; P.KS = (W + 31) / 32; P.NT = (2 * pw->kp + 15) / 16;
    P.rpg = c * H; P.tiles = (c * H + 15) / 16; P.S = P.tiles;
    P.H = H; P.KW = KW; P.bcc = c;
    P.vec = W % 4 == 0 && al16(pred) && al16(target);
    RPDE_TRY((fe_launch<true, true>(P, 1, st)));
    // columns along H: group kx holds c rows of 2 H interleaved (re, im) -> |Z|^2 summed over the images
    FeP Q;
    memset(&Q, 0, sizeof(Q));
    Q.a = w.s0; Q.b = w.s1; Q.timg = th; Q.out0 = w.part;
    Q.K = 2 * H; Q.KS = (2 * H + 31) / 32; Q.NT = NT2;
    Q.rpg = c; Q.tiles = (c + 15) / 16; Q.S = Q.tiles < FE_SLOTS_2D ? Q.tiles : FE_SLOTS_2D;
    Q.vec = (2 * H) % 4 == 0;
    RPDE_TRY((fe_launch<false, false>(Q, KW, st)));
    hipLaunchKernelGGL(k_fe_fold2d, dim3(n_bins, 2), dim3(256), 0, st, w.part, bins, Q.S, NT2 * 16, H, KW, W, n_bins, acc);
    RPDE_LAUNCH_CHECK();
  }
  return RPDE_OK;
}

}  // extern "C"
