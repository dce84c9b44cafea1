// HBM-bound pointwise / reduction kernels around the GEMMs.
// All are coalesced (16 B per lane where the layout allows), wave64 shuffles
// for row reductions, deterministic two-stage sums (per-block partial slabs,
// then reduce_slabs) -- no float atomics, so results are run-to-run identical.
#include "rpde_internal.h"
#include "pointwise.h"

#include <type_traits>

namespace rpde {

// ---------------------------------------------------------------------------
// out[i] (+)= scale * sum_s slabs[s*stride + i]
// ---------------------------------------------------------------------------
// 64 consecutive outputs per block; the 4 waves split the slabs, LDS combines them
__device__ __forceinline__ float slab_partial(const float* __restrict__ slabs, long i, int S, long stride, int ty) {
  float acc;
  {
    // with few outputs and many slabs this loop is pure load latency (2 blocks, 256 slabs: 13 us with eight loads in
    // flight per lane): 32 in flight while there are that many, then 8, then the rest -- the summation order is fixed by
    // S alone, so results stay reproducible
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int s = ty;
    for (; s + 124 < S; s += 128) {
      float v[32];
#pragma unroll
      for (int j = 0; j < 32; ++j) v[j] = slabs[(long)(s + 4 * j) * stride + i];
#pragma unroll
      for (int j = 0; j < 32; ++j) a[j & 7] += v[j];
    }
    for (; s + 28 < S; s += 32) {
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] += slabs[(long)(s + 4 * j) * stride + i];
    }
    for (; s < S; s += 4) a[0] += slabs[(long)s * stride + i];
    acc = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  }
  return acc;
}

// The one fold kernel: several independent folds, one launch; block -> job by the jobs' first-block numbers.
// dst[i] = scale * sum (+ dst[i] when accumulate); a launch of several jobs passes 1.f, 0 (the product is exact)
__global__ __launch_bounds__(256) void k_fold_jobs(const FoldJobs J, float scale, int accumulate) {
  __shared__ float red[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  int jn = 0;
#pragma unroll
  for (int q = 1; q < FoldJobs::MAX; ++q)
    if (q < J.n && (int)blockIdx.x >= J.j[q].blk0) jn = q;
  const float* src = J.j[0].src; float* dst = J.j[0].dst; long stride = J.j[0].stride, len = J.j[0].len; int S = J.j[0].S, b0 = 0;
#pragma unroll
  for (int q = 1; q < FoldJobs::MAX; ++q)          // (selects instead of a dynamically indexed kernel argument)
    if (q == jn) { src = J.j[q].src; dst = J.j[q].dst; stride = J.j[q].stride; len = J.j[q].len; S = J.j[q].S; b0 = J.j[q].blk0; }
  const long i = (long)((int)blockIdx.x - b0) * 64 + tx;
  float acc = i < len ? slab_partial(src, i, S, stride, ty) : 0.f;
  red[ty][tx] = acc;
  __syncthreads();
  if (ty == 0 && i < len) {
    acc = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
    acc *= scale;
    if (accumulate) acc += dst[i];
    dst[i] = acc;
  }
}

int fold_jobs(FoldJobs& jobs, hipStream_t st, float scale, int accumulate) {
  int blocks = 0;
  for (int q = 0; q < jobs.n; ++q) { jobs.j[q].blk0 = blocks; blocks += (int)((jobs.j[q].len + 63) / 64); }
  if (blocks == 0) return RPDE_OK;
  hipLaunchKernelGGL(k_fold_jobs, dim3((unsigned)blocks), dim3(256), 0, st, jobs, scale, accumulate);
  RPDE_LAUNCH_CHECK();
  jobs.n = 0;
  return RPDE_OK;
}

int reduce_slabs(const float* slabs, float* out, long n, int S, long stride, float scale, int accumulate, hipStream_t st) {
  FoldJobs one;
  one.add(slabs, out, n, S, stride);
  return fold_jobs(one, st, scale, accumulate);
}

// many slabs, few outputs (per-tile column sums): first fold S slabs into REDUCE_CHUNKS
// partial rows (tmp [REDUCE_CHUNKS][n]) with one block per (64 outputs, chunk), then fold those
__global__ __launch_bounds__(256) void k_reduce_slabs_chunk(const float* __restrict__ slabs, float* __restrict__ tmp, long n,
                                                            int S, long stride, int per_chunk) {
  __shared__ float red[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * 64 + tx;
  const int s0 = blockIdx.y * per_chunk, s1 = min(S, s0 + per_chunk);      // (a chunk past the last slab: s1 < s0, sum 0)
  float acc = i < n ? slab_partial(slabs + (long)s0 * stride, i, s1 - s0, stride, ty) : 0.f;
  red[ty][tx] = acc;
  __syncthreads();
  if (ty == 0 && i < n) tmp[(long)blockIdx.y * n + i] = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
}

int reduce_slabs_2pass(const float* slabs, float* out, long n, int S, long stride, float* tmp, hipStream_t st) {
  if (S <= 4 * REDUCE_CHUNKS) return reduce_slabs(slabs, out, n, S, stride, 1.f, 0, st);
  const int per = (S + REDUCE_CHUNKS - 1) / REDUCE_CHUNKS;
  hipLaunchKernelGGL(k_reduce_slabs_chunk, dim3((unsigned)((n + 63) / 64), REDUCE_CHUNKS), dim3(256), 0, st, slabs, tmp, n, S, stride, per);
  RPDE_LAUNCH_CHECK();
  return reduce_slabs(tmp, out, n, REDUCE_CHUNKS, n, 1.f, 0, st);
}

// ---------------------------------------------------------------------------
// column sums of x [P, N] (row stride ld): slab[block][n] partials
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_colsum(const float* __restrict__ x, float* __restrict__ slab, long P, int N, long ld,
                                                long rows_per_block) {
  __shared__ float red[256];
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = min(P, r0 + rows_per_block);
  const int t = threadIdx.x;
  if (N <= 256 && 256 % N == 0) {
    const int tr = t / N, c = t % N, step = 256 / N;
    float acc = 0.f;
    for (long r = r0 + tr; r < r1; r += step) acc += x[r * ld + c];
    red[t] = acc;
    __syncthreads();
    // the step row-lanes of a column fold as a fixed tree (step is a power of two): one thread adding them in turn
    // carried a running sum through up to 255 roundings, which for N = 1 was most of the error of the whole column sum
    for (int w = step >> 1; w >= 1; w >>= 1) {
      if (tr < w) red[t] += red[t + w * N];
      __syncthreads();
    }
    if (tr == 0) slab[(long)blockIdx.x * N + c] = red[t];
  } else {
    for (int c = t; c < N; c += 256) {
      float acc = 0.f;
      for (long r = r0; r < r1; ++r) acc += x[r * ld + c];
      slab[(long)blockIdx.x * N + c] = acc;
    }
  }
}

// the slab-producing kernels run between 1 and 1024 workgroups: one slab each
static long slab_blocks(long nb) { return nb < 1 ? 1 : nb > 1024 ? 1024 : nb; }

size_t colsum_ws_floats(long P, int N) { return (size_t)slab_blocks((P + 255) / 256) * N; }

int colsum(const float* x, float* out, long P, int N, long ld, float* ws, int accumulate, hipStream_t st) {
  const long nb = slab_blocks((P + 255) / 256);
  const long rpb = (P + nb - 1) / nb;
  hipLaunchKernelGGL(k_colsum, dim3((unsigned)nb), dim3(256), 0, st, x, ws, P, N, ld, rpb);
  RPDE_LAUNCH_CHECK();
  return reduce_slabs(ws, out, N, (int)nb, N, 1.f, accumulate, st);
}

// ---------------------------------------------------------------------------
// FeedForward tail: out = residual + post_act( LN( dropout(z) ) )
// One row of C floats is owned by G = C/4 lanes (float4 each); a wave holds
// 64/G rows.  C must be a multiple of 4 with C/4 in {1,2,4,...,64}; other
// widths take the one-wave-per-row path below.
// ---------------------------------------------------------------------------
static bool tail_vec_ok(int C) {
  const int G = C / 4;
  return (C % 4 == 0) && (G == 1 || G == 2 || G == 4 || G == 8 || G == 16 || G == 32 || G == 64);
}
// f(G as a constant) for the G = C / 4 of a width that tail_vec_ok accepts
template <class F>
static void tail_dispatch(int G, F&& f) {
  switch (G) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    default: f(std::integral_constant<int, 64>{}); break;
  }
}

template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int G>
__global__ __launch_bounds__(256) void k_ff_tail_fwd(const float* __restrict__ z, const float* __restrict__ res,
                                                     float* __restrict__ out, long P, int layer_norm, float eps,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     DropCfg drop, int post_act) {
  drop = drop_resolve(drop);
  constexpr int C = 4 * G;
  const int lane_in_row = threadIdx.x % G;
  const long rows_per_block = 256 / G;
  for (long row = (long)blockIdx.x * rows_per_block + threadIdx.x / G; row < P; row += (long)gridDim.x * rows_per_block) {
    const long off = row * C + lane_in_row * 4;
    float4 v = *reinterpret_cast<const float4*>(z + off);
    if (drop.on()) {
      float s[4];
      drop_scale4(drop, (uint64_t)off, s);
      v.x *= s[0]; v.y *= s[1]; v.z *= s[2]; v.w *= s[3];
    }
    if (layer_norm) {
      const float mean = group_sum<G>(v.x + v.y + v.z + v.w) * (1.f / C);
      const float dx = v.x - mean, dy = v.y - mean, dz = v.z - mean, dw = v.w - mean;
      const float var = group_sum<G>(dx * dx + dy * dy + dz * dz + dw * dw) * (1.f / C);
      const float rstd = rsqrtf(var + eps);
      const float4 gm = *reinterpret_cast<const float4*>(gamma + lane_in_row * 4);
      const float4 bt = *reinterpret_cast<const float4*>(beta + lane_in_row * 4);
      v.x = dx * rstd * gm.x + bt.x;
      v.y = dy * rstd * gm.y + bt.y;
      v.z = dz * rstd * gm.z + bt.z;
      v.w = dw * rstd * gm.w + bt.w;
    }
    if (post_act) {
      v.x = act_f(post_act, v.x); v.y = act_f(post_act, v.y);
      v.z = act_f(post_act, v.z); v.w = act_f(post_act, v.w);
    }
    if (res) {
      const float4 r = *reinterpret_cast<const float4*>(res + off);
      v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
    }
    *reinterpret_cast<float4*>(out + off) = v;
  }
}

// generic width: one wave per row, up to 8 elements per lane (C <= 512)
__global__ __launch_bounds__(256) void k_ff_tail_fwd_any(const float* __restrict__ z, const float* __restrict__ res,
                                                         float* __restrict__ out, long P, int C, int layer_norm, float eps,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         DropCfg drop, int post_act) {
  drop = drop_resolve(drop);
  const int lane = threadIdx.x & 63;
  for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < P; row += (long)gridDim.x * 4) {
    float v[8];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = lane + 64 * j;
      v[j] = 0.f;
      if (c < C) {
        const long off = row * C + c;
        v[j] = z[off];
        if (drop.on()) v[j] *= drop_scale1(drop, (uint64_t)off);
        sum += v[j];
      }
    }
    float mean = 0.f, rstd = 1.f;
    if (layer_norm) {
      mean = wave_sum(sum) / C;
      float sq = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) if (lane + 64 * j < C) sq += (v[j] - mean) * (v[j] - mean);
      rstd = rsqrtf(wave_sum(sq) / C + eps);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = lane + 64 * j;
      if (c < C) {
        float y = v[j];
        if (layer_norm) y = (y - mean) * rstd * gamma[c] + beta[c];
        y = act_f(post_act, y);
        const long off = row * C + c;
        if (res) y += res[off];
        out[off] = y;
      }
    }
  }
}

int ff_tail_fwd(const float* z, const float* res, float* out, long P, int C, int layer_norm, float eps,
                const float* gamma, const float* beta, DropCfg drop, int post_act, hipStream_t st) {
  RPDE_CHECK_ARG(!layer_norm || (gamma && beta), "ff_tail: layer_norm needs gamma/beta");
  const int G = C / 4;
  if (!tail_vec_ok(C)) {
    RPDE_CHECK_ARG(C <= 512, "ff_tail: width %d > 512 unsupported", C);
    long nb = (P + 3) / 4; if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_ff_tail_fwd_any, dim3((unsigned)nb), dim3(256), 0, st, z, res, out, P, C, layer_norm, eps, gamma, beta, drop, post_act);
    RPDE_LAUNCH_CHECK();
    return RPDE_OK;
  }
  const long rpb = 256 / G;
  long nb = (P + rpb - 1) / rpb; if (nb > 8192) nb = 8192;
  tail_dispatch(G, [&](auto g_) {
    hipLaunchKernelGGL((k_ff_tail_fwd<g_()>), dim3((unsigned)nb), dim3(256), 0, st, z, res, out, P, layer_norm, eps, gamma, beta, drop, post_act);
  });
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

// ---------------------------------------------------------------------------
// backward of the tail.  g = d(out).  Produces dz (through post_act', LN and
// the dropout mask) and per-block partial sums for d(gamma), d(beta):
// slab[block][0:C] = sum dy*xhat, slab[block][C:2C] = sum dy.
// One wave per row (any C <= 512): simple and HBM bound.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ff_tail_bwd(const float* __restrict__ z, const float* __restrict__ g,
                                                     float* __restrict__ dz, float* __restrict__ slab, long P, int C,
                                                     int layer_norm, float eps, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, DropCfg drop, int post_act) {
  drop = drop_resolve(drop);
  __shared__ float red[4][2][512];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float dg[8], db[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { dg[j] = 0.f; db[j] = 0.f; }
  for (long row = (long)blockIdx.x * 4 + w; row < P; row += (long)gridDim.x * 4) {
    float t[8], s[8], gy[8];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = lane + 64 * j;
      t[j] = 0.f; s[j] = 1.f; gy[j] = 0.f;
      if (c < C) {
        const long off = row * C + c;
        if (drop.on()) s[j] = drop_scale1(drop, (uint64_t)off);
        t[j] = z[off] * s[j];
        gy[j] = g[off];
        sum += t[j];
      }
    }
    if (!layer_norm) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = lane + 64 * j;
        if (c < C) dz[row * C + c] = gy[j] * dact_f(post_act, t[j]) * s[j];
      }
      continue;
    }
    const float mean = wave_sum(sum) / C;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) if (lane + 64 * j < C) sq += (t[j] - mean) * (t[j] - mean);
    const float rstd = rsqrtf(wave_sum(sq) / C + eps);
    float xh[8], dxh[8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = lane + 64 * j;
      xh[j] = 0.f; dxh[j] = 0.f;
      if (c < C) {
        xh[j] = (t[j] - mean) * rstd;
        const float gm = gamma[c];
        float dy = gy[j];
        if (post_act) dy *= dact_f(post_act, xh[j] * gm + beta[c]);
        dg[j] += dy * xh[j];
        db[j] += dy;
        dxh[j] = dy * gm;
        s1 += dxh[j];
        s2 += dxh[j] * xh[j];
      }
    }
    s1 = wave_sum(s1) / C;
    s2 = wave_sum(s2) / C;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = lane + 64 * j;
      if (c < C) dz[row * C + c] = rstd * (dxh[j] - s1 - xh[j] * s2) * s[j];
    }
  }
  if (!layer_norm) return;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[w][0][lane + 64 * j] = dg[j];
    red[w][1][lane + 64 * j] = db[j];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    slab[(long)blockIdx.x * 2 * C + c] = red[0][0][c] + red[1][0][c] + red[2][0][c] + red[3][0][c];
    slab[(long)blockIdx.x * 2 * C + C + c] = red[0][1][c] + red[1][1][c] + red[2][1][c] + red[3][1][c];
  }
}

// vector form: a row of C = 4G floats is owned by G lanes (float4 each); every
// thread keeps the same 4 columns for all its rows, so d(gamma), d(beta) and the
// bias gradient sum(dz) accumulate in registers and meet once in LDS.
// slab[block][3][C] = (sum dy*xhat, sum dy, sum dz)
template <int G>
__global__ __launch_bounds__(256) void k_ff_tail_bwd_vec(const float* __restrict__ z, const float* __restrict__ g,
                                                         float* __restrict__ dz, float* __restrict__ slab, long P,
                                                         int layer_norm, float eps, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, DropCfg drop, int post_act) {
  drop = drop_resolve(drop);
  constexpr int C = 4 * G;
  constexpr int RPB = 256 / G;
  __shared__ float red[3][RPB][C];
  const int lir = threadIdx.x % G, rib = threadIdx.x / G;
  float4 gm = make_float4(1.f, 1.f, 1.f, 1.f), bt = make_float4(0.f, 0.f, 0.f, 0.f);
  if (layer_norm) {
    gm = *reinterpret_cast<const float4*>(gamma + lir * 4);
    bt = *reinterpret_cast<const float4*>(beta + lir * 4);
  }
  float dg[4] = {0.f, 0.f, 0.f, 0.f}, db[4] = {0.f, 0.f, 0.f, 0.f}, ds[4] = {0.f, 0.f, 0.f, 0.f};
  const float gmv[4] = {gm.x, gm.y, gm.z, gm.w}, btv[4] = {bt.x, bt.y, bt.z, bt.w};
  for (long row = (long)blockIdx.x * RPB + rib; row < P; row += (long)gridDim.x * RPB) {
    const long off = row * C + lir * 4;
    const float4 z4 = *reinterpret_cast<const float4*>(z + off);
    const float4 g4 = *reinterpret_cast<const float4*>(g + off);
    float s[4] = {1.f, 1.f, 1.f, 1.f};
    if (drop.on()) drop_scale4(drop, (uint64_t)off, s);
    const float t[4] = {z4.x * s[0], z4.y * s[1], z4.z * s[2], z4.w * s[3]};
    const float gy[4] = {g4.x, g4.y, g4.z, g4.w};
    float o[4];
    if (layer_norm) {
      const float mean = group_sum<G>(t[0] + t[1] + t[2] + t[3]) * (1.f / C);
      float d[4], sq = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) { d[k] = t[k] - mean; sq += d[k] * d[k]; }
      const float rstd = rsqrtf(group_sum<G>(sq) * (1.f / C) + eps);
      float xh[4], dxh[4], s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        xh[k] = d[k] * rstd;
        float dy = gy[k];
        if (post_act) dy *= dact_f(post_act, xh[k] * gmv[k] + btv[k]);
        dg[k] += dy * xh[k];
        db[k] += dy;
        dxh[k] = dy * gmv[k];
        s1 += dxh[k];
        s2 += dxh[k] * xh[k];
      }
      s1 = group_sum<G>(s1) * (1.f / C);
      s2 = group_sum<G>(s2) * (1.f / C);
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = rstd * (dxh[k] - s1 - xh[k] * s2) * s[k];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = gy[k] * dact_f(post_act, t[k]) * s[k];
    }
    *reinterpret_cast<float4*>(dz + off) = make_float4(o[0], o[1], o[2], o[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) ds[k] += o[k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    red[0][rib][lir * 4 + k] = dg[k];
    red[1][rib][lir * 4 + k] = db[k];
    red[2][rib][lir * 4 + k] = ds[k];
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 3 * C; idx += 256) {
    const int w = idx / C, c = idx % C;
    float a = 0.f;
#pragma unroll 4
    for (int r = 0; r < RPB; ++r) a += red[w][r][c];
    slab[(long)blockIdx.x * 3 * C + idx] = a;
  }
}

static long tail_bwd_blocks(long P) { return slab_blocks((P + 3) / 4); }
size_t ff_tail_bwd_ws_floats(long P, int C) { return (size_t)tail_bwd_blocks(P) * 3 * C; }

// grad_bias (optional) receives colsum(dz) when the vector kernel runs; returns whether it did
int ff_tail_bwd(const float* z, const float* g, float* dz, long P, int C, int layer_norm, float eps, const float* gamma,
                const float* beta, DropCfg drop, int post_act, float* grad_gamma, float* grad_beta, float* grad_bias,
                int* bias_done, float* ws, hipStream_t st, FoldJobs* defer) {
  *bias_done = 0;
  // the per-block partial sums are folded here, or (defer) by the caller's one fold launch -- same sums
  auto fold = [&](const float* src, float* dst, int S, long stride) -> int {
    if (defer && defer->add(src, dst, C, S, stride)) return RPDE_OK;
    return reduce_slabs(src, dst, C, S, stride, 1.f, 0, st);
  };
  if (tail_vec_ok(C)) {
    const int G = C / 4;
    const long rpb = 256 / G;
    const long nb = slab_blocks((P + rpb - 1) / rpb);
    tail_dispatch(G, [&](auto g_) {
      hipLaunchKernelGGL((k_ff_tail_bwd_vec<g_()>), dim3((unsigned)nb), dim3(256), 0, st, z, g, dz, ws, P, layer_norm, eps, gamma, beta, drop, post_act);
    });
    RPDE_LAUNCH_CHECK();
    if (layer_norm) {
      if (grad_gamma) RPDE_TRY(fold(ws, grad_gamma, (int)nb, 3L * C));
      if (grad_beta) RPDE_TRY(fold(ws + C, grad_beta, (int)nb, 3L * C));
    }
    if (grad_bias) { RPDE_TRY(fold(ws + 2 * C, grad_bias, (int)nb, 3L * C)); *bias_done = 1; }
    return RPDE_OK;
  }
  RPDE_CHECK_ARG(C <= 512, "ff_tail_bwd: width %d > 512 unsupported", C);
  const long nb = tail_bwd_blocks(P);
  hipLaunchKernelGGL(k_ff_tail_bwd, dim3((unsigned)nb), dim3(256), 0, st, z, g, dz, ws, P, C, layer_norm, eps, gamma, beta, drop, post_act);
  RPDE_LAUNCH_CHECK();
  if (layer_norm) {
    if (grad_gamma) RPDE_TRY(fold(ws, grad_gamma, (int)nb, 2L * C));
    if (grad_beta) RPDE_TRY(fold(ws + C, grad_beta, (int)nb, 2L * C));
  }
  return RPDE_OK;
}

// ---------------------------------------------------------------------------
// per-mode complex weights [Ci,Co,K,2] <-> real block matrices [k][2Ci][2Co]
//   (re,i)->(re,o): Wr   (im,i)->(re,o): -Wi   (re,i)->(im,o): Wi   (im,i)->(im,o): Wr
// ---------------------------------------------------------------------------
__global__ void k_pack_mix(const float* __restrict__ w, float* __restrict__ blk, int Ci, int Co, int K, int keff) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = 4L * Ci * Co;
  if (idx >= per * keff) return;
  const int k = (int)(idx / per);
  const long r = idx % per;
  const int row = (int)(r / (2 * Co)), col = (int)(r % (2 * Co));
  const int ri_in = row / Ci, i = row % Ci, ri_out = col / Co, o = col % Co;
  const float* p = w + (((long)i * Co + o) * K + k) * 2;
  float v;
  if (ri_in == ri_out) v = p[0];
  else v = ri_in ? -p[1] : p[1];
  blk[idx] = v;
}

int pack_mix_weights(const float* w, float* blk, int Ci, int Co, int K, int keff, hipStream_t st) {
  const long tot = 4L * Ci * Co * keff;
  hipLaunchKernelGGL(k_pack_mix, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, w, blk, Ci, Co, K, keff);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

// gw[i,o,k,:] = fold( sum_s slab[s][k][2Ci][2Co] ), zero for k >= keff
__global__ void k_unpack_mix_grad(const float* __restrict__ slabs, float* __restrict__ gw, int Ci, int Co, int K, int keff,
                                  int S, long sstride) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)Ci * Co * K) return;
  const int k = (int)(idx % K);
  const long io = idx / K;
  const int o = (int)(io % Co), i = (int)(io / Co);
  float gr = 0.f, gi = 0.f;
  if (k < keff) {
    const long per = 4L * Ci * Co, ld = 2L * Co;
    for (int s = 0; s < S; ++s) {
      const float* b = slabs + (long)s * sstride + (long)k * per;
      gr += b[(long)i * ld + o] + b[(long)(Ci + i) * ld + Co + o];
      gi += b[(long)i * ld + Co + o] - b[(long)(Ci + i) * ld + o];
    }
  }
  gw[idx * 2] = gr;
  gw[idx * 2 + 1] = gi;
}

int unpack_mix_grad(const float* slabs, float* gw, int Ci, int Co, int K, int keff, int S, long sstride, hipStream_t st) {
  const long tot = (long)Ci * Co * K;
  hipLaunchKernelGGL(k_unpack_mix_grad, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, slabs, gw, Ci, Co, K, keff, S, sstride);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

// ---------------------------------------------------------------------------
// weight normalisation of WNLinear (models/custom_layer.py:70-108; torch.nn.utils.weight_norm, dim 0):
//   w[o,:] = v[o,:] * (g[o] / |v[o,:]|)
//   gg[o]  = <gw[o,:], v[o,:]> / |v[o,:]|
//   gv[o,:] = (g[o] / |v[o,:]|) * (gw[o,:] - v[o,:] * <gw[o,:], v[o,:]> / |v[o,:]|^2)
// one wave per row (the reference's graph is a dozen ATen kernels on [128,1] / [1,128] tensors per step)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_weight_norm_fwd(const float* __restrict__ v, const float* __restrict__ g,
                                                         float* __restrict__ w, int out_f, int in_f) {
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (o >= out_f) return;
  const float* vr = v + (long)o * in_f;
  float ss = 0.f;
  for (int i = lane; i < in_f; i += 64) ss = fmaf(vr[i], vr[i], ss);
  const float scale = g[o] / sqrtf(wave_sum(ss));
  for (int i = lane; i < in_f; i += 64) w[(long)o * in_f + i] = vr[i] * scale;
}

__global__ __launch_bounds__(256) void k_weight_norm_bwd(const float* __restrict__ v, const float* __restrict__ g,
                                                         const float* __restrict__ gw, float* __restrict__ gv,
                                                         float* __restrict__ gg, int out_f, int in_f) {
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (o >= out_f) return;
  const float* vr = v + (long)o * in_f;
  const float* gr = gw + (long)o * in_f;
  float ss = 0.f, dot = 0.f;
  for (int i = lane; i < in_f; i += 64) { ss = fmaf(vr[i], vr[i], ss); dot = fmaf(gr[i], vr[i], dot); }
  ss = wave_sum(ss);
  dot = wave_sum(dot);
  const float nrm = sqrtf(ss), scale = g[o] / nrm, back = dot / ss;
  if (gg && lane == 0) gg[o] = dot / nrm;
  if (gv)
    for (int i = lane; i < in_f; i += 64) gv[(long)o * in_f + i] = scale * (gr[i] - vr[i] * back);
}

}  // namespace rpde

using namespace rpde;

extern "C" {

int rpde_weight_norm_fwd(const float* v, const float* g, float* w, int out_f, int in_f, void* stream) {
  RPDE_CHECK_ARG(v && g && w && out_f > 0 && in_f > 0, "weight_norm_fwd: bad arguments");
  hipLaunchKernelGGL(k_weight_norm_fwd, dim3((out_f + 3) / 4), dim3(256), 0, as_stream(stream), v, g, w, out_f, in_f);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_weight_norm_bwd(const float* v, const float* g, const float* grad_w, float* grad_v, float* grad_g, int out_f, int in_f,
                         void* stream) {
  RPDE_CHECK_ARG(v && g && grad_w && (grad_v || grad_g) && out_f > 0 && in_f > 0, "weight_norm_bwd: bad arguments");
  hipLaunchKernelGGL(k_weight_norm_bwd, dim3((out_f + 3) / 4), dim3(256), 0, as_stream(stream), v, g, grad_w, grad_v, grad_g, out_f, in_f);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// layout helpers at the model boundary
// ---------------------------------------------------------------------------
namespace rpde {

// out (channels-last [B,S,Ct] or channels-first [B,Ct,S]) = cat(x [B,Cin,S], grid coords)
__global__ void k_concat_grid(const float* __restrict__ x, float* __restrict__ out, int B, int Cin, int M, int N, int G,
                              double lo, double hi, int channels_last, const float* __restrict__ gx,
                              const float* __restrict__ gy) {
  const long S = (long)M * N;
  const int Ct = Cin + G;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * S * Ct) return;
  int c; long s; int b;
  if (channels_last) { c = (int)(idx % Ct); s = (idx / Ct) % S; b = (int)(idx / (Ct * S)); }
  else { s = idx % S; c = (int)((idx / S) % Ct); b = (int)(idx / (S * Ct)); }
  float v;
  if (c < Cin) {
    v = x[((long)b * Cin + c) * S + s];
  } else {
    const int axis = c - Cin;                 // 0: first spatial dim, 1: second
    const int len = (G == 2 && axis == 1) ? N : M;
    const int pos = (G == 2) ? (axis == 0 ? (int)(s / N) : (int)(s % N)) : (int)s;
    const float* tab = axis == 0 ? gx : gy;
    if (tab) v = tab[pos];
    else {
      // numpy.linspace(lo, hi, len) in double, then cast (quirk Q10): pos * step is rounded BEFORE lo is added, as numpy
      // does it -- a contracted fma differs in the last fp32 place at some positions when lo != 0
      // (tests/test_gpu_pointwise.py, lo = -1, hi = 2.5).  hipcc contracts by default, through __dmul_rn / __dadd_rn
      // too; the pragma is what keeps v_mul_f64 and v_add_f64 apart
#pragma clang fp contract(off)
      const double step = len > 1 ? (hi - lo) / (double)(len - 1) : 0.0;
      const double scaled = (double)pos * step;
      v = (pos == len - 1 && len > 1) ? (float)hi : (float)(scaled + lo);
    }
  }
  out[idx] = v;
}

// tiled transpose [B,S,C] <-> [B,C,S]
__global__ __launch_bounds__(256) void k_transpose(const float* __restrict__ in, float* __restrict__ out, long R, long Cc) {
  // in [B][R][Cc] -> out [B][Cc][R]
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const long r0 = (long)blockIdx.y * 32, c0 = (long)blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  const float* ib = in + (long)b * R * Cc;
  float* ob = out + (long)b * R * Cc;
  for (int j = ty; j < 32; j += 8) {
    const long r = r0 + j, c = c0 + tx;
    if (r < R && c < Cc) tile[j][tx] = ib[r * Cc + c];
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const long c = c0 + j, r = r0 + tx;
    if (r < R && c < Cc) ob[c * R + r] = tile[tx][j];
  }
}

__global__ void k_act_fwd(const float* __restrict__ x, float* __restrict__ out, long n, int act) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = act_f(act, x[i]);
}
__global__ void k_act_bwd(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ dx, long n, int act) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dx[i] = g[i] * dact_f(act, x[i]);
}

}  // namespace rpde

extern "C" {

int rpde_concat_grid(const float* x, float* out, int B, int Cin, int M, int N, int grid_dims, double lo, double hi,
                     int channels_last, const float* gridx, const float* gridy, void* stream) {
  RPDE_CHECK_ARG(x && out && B > 0 && Cin > 0 && M > 0 && N > 0, "concat_grid: bad arguments");
  RPDE_CHECK_ARG(grid_dims >= 0 && grid_dims <= 2, "concat_grid: grid_dims %d", grid_dims);
  const long tot = (long)B * M * N * (Cin + grid_dims);
  hipLaunchKernelGGL(k_concat_grid, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, as_stream(stream), x, out, B, Cin, M, N, grid_dims, lo, hi, channels_last, gridx, gridy);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_transpose_cs(const float* in, float* out, int B, int64_t S, int C, int to_channels_first, void* stream) {
  RPDE_CHECK_ARG(in && out && B > 0 && S > 0 && C > 0, "transpose_cs: bad arguments");
  const long R = to_channels_first ? S : C, Cc = to_channels_first ? C : S;
  dim3 grid((unsigned)((Cc + 31) / 32), (unsigned)((R + 31) / 32), B);
  RPDE_CHECK_ARG(grid.y <= 65535 && B <= 65535, "transpose_cs: tensor too large for one launch");
  hipLaunchKernelGGL(k_transpose, grid, dim3(256), 0, as_stream(stream), in, out, R, Cc);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_act_fwd(const float* x, float* out, int64_t n, int act, void* stream) {
  RPDE_CHECK_ARG(x && out && n >= 0, "act_fwd: bad arguments");
  if (n == 0) return RPDE_OK;
  hipLaunchKernelGGL(k_act_fwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), x, out, (long)n, act);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_act_bwd(const float* x, const float* g, float* dx, int64_t n, int act, void* stream) {
  RPDE_CHECK_ARG(x && g && dx && n >= 0, "act_bwd: bad arguments");
  if (n == 0) return RPDE_OK;
  hipLaunchKernelGGL(k_act_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), x, g, dx, (long)n, act);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

}  // extern "C"
