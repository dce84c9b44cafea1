// The relative-loss family's shared code (rel_loss.h) and the relative L2 loss itself (utils/loss.py RelativeL2Loss;
// reference: utils/loss.py:17-59): per-sample |x - y|_2 / (|y|_2 + REL_EPS), then mean / sum / the per-sample vector.
// Every sum is two-stage and in fixed order, no atomics: identical calls give identical bits.
#include "rel_loss.h"

namespace rpde {

// ---------------------------------------------------------------------------
// shared by the mode-weighted loss, the band energies and the equation residual
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rel_diff(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ d,
                                                  long n, int vec) {
  const long i0 = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
  if (vec) {
    for (long i = i0; i < n / 4; i += step) {
      const float4 a = reinterpret_cast<const float4*>(x)[i], b = reinterpret_cast<const float4*>(y)[i];
      reinterpret_cast<float4*>(d)[i] = make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
    }
  } else {
    for (long i = i0; i < n; i += step) d[i] = x[i] - y[i];
  }
}

int rel_diff(const float* x, const float* y, float* d, long total, hipStream_t st) {
  const int vec = total % 4 == 0 && al16(x) && al16(y) && al16(d);
  long nb = ((vec ? total / 4 : total) + 255) / 256;
  nb = nb > 2048 ? 2048 : nb < 1 ? 1 : nb;
  hipLaunchKernelGGL(k_rel_diff, dim3((unsigned)nb), dim3(256), 0, st, x, y, d, total, vec);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

// one workgroup; the order of every sum is fixed: slots j = 0 .. S-1 of a sample, samples strided by 256, the halving tree
__global__ __launch_bounds__(256) void k_rel_final(const double* __restrict__ part, float* __restrict__ rel, float* __restrict__ loss,
                                                   float* __restrict__ stats, int B, int S, double inv, int size_average) {
  __shared__ double red[256];
  double acc = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) {
    double e0 = 0.0, e1 = 0.0;
    for (int j = 0; j < S; ++j) { e0 += part[(long)b * S + j]; e1 += part[((long)B + b) * S + j]; }
    const float dn = (float)sqrt(e0 * inv), yn = (float)sqrt(e1 * inv);
    const float r = rel_ratio(dn, yn);
    stats[2 * b] = dn; stats[2 * b + 1] = yn;
    if (rel) rel[b] = r;
    acc += (double)r;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0 && loss) *loss = (float)(size_average ? red[0] / B : red[0]);
}

int rel_final(const double* part, float* rel, float* loss, float* stats, int B, int S, double inv, int size_average,
              hipStream_t st) {
  hipLaunchKernelGGL(k_rel_final, dim3(1), dim3(256), 0, st, part, rel, loss, stats, B, S, inv, size_average);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

__global__ __launch_bounds__(256) void k_rel_roots(double2* __restrict__ tw, int N, int M) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= N + M) return;
  const int n = j < N ? N : M, i = j < N ? j : j - N;
  double s, c;
  sincospi(2.0 * (double)i / (double)n, &s, &c);
  tw[j] = make_double2(c, -s);
}

int rel_roots(double2* tw, int N, int M, hipStream_t st) {
  hipLaunchKernelGGL(k_rel_roots, dim3((N + M + 255) / 256), dim3(256), 0, st, tw, N, M);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

// ---------------------------------------------------------------------------
// relative L2 loss
// ---------------------------------------------------------------------------
constexpr int L2_BLOCKS = 64;   // partial blocks per sample

__global__ __launch_bounds__(256) void k_rel_l2_partial(const float* __restrict__ x, const float* __restrict__ y,
                                                        float* __restrict__ part, long per) {
  __shared__ float red[2][4];
  const int b = blockIdx.y;
  const float* xb = x + (long)b * per;
  const float* yb = y + (long)b * per;
  float sd = 0.f, sy = 0.f;
  const bool vec = (per % 4 == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0) && ((reinterpret_cast<uintptr_t>(y) & 15) == 0);
  if (vec) {
    const long nv = per / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
      const float4 a = reinterpret_cast<const float4*>(xb)[i];
      const float4 c = reinterpret_cast<const float4*>(yb)[i];
      const float d0 = a.x - c.x, d1 = a.y - c.y, d2 = a.z - c.z, d3 = a.w - c.w;
      sd += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
      sy += c.x * c.x + c.y * c.y + c.z * c.z + c.w * c.w;
    }
  } else {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
      const float d = xb[i] - yb[i];
      sd += d * d;
      sy += yb[i] * yb[i];
    }
  }
  sd = wave_sum(sd);
  sy = wave_sum(sy);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][w] = sd; red[1][w] = sy; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[((long)b * gridDim.x + blockIdx.x) * 2] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    part[((long)b * gridDim.x + blockIdx.x) * 2 + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

// one block: stats[b] = (|x-y|, |y|), rel[b], loss = mean/sum.  Not folded into k_rel_final: its partials, its sums over
// the blocks and over the samples and its mean are float, interleaved (sd, sy) pairs, and the training benchmark's
// headline loss is this kernel's output -- float64 sums there would move its bits
__global__ void k_rel_l2_final(const float* __restrict__ part, int nblk, float* __restrict__ rel, float* __restrict__ loss,
                               float* __restrict__ stats, int B, int size_average) {
  __shared__ float red[256];
  float acc = 0.f;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    float sd = 0.f, sy = 0.f;
    for (int j = 0; j < nblk; ++j) { sd += part[((long)b * nblk + j) * 2]; sy += part[((long)b * nblk + j) * 2 + 1]; }
    const float dn = sqrtf(sd), yn = sqrtf(sy);
    const float r = rel_ratio(dn, yn);
    stats[2 * b] = dn; stats[2 * b + 1] = yn;
    if (rel) rel[b] = r;
    acc += r;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = blockDim.x / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0 && loss) *loss = size_average ? red[0] / B : red[0];
}

__global__ __launch_bounds__(256) void k_rel_l2_bwd(const float* __restrict__ x, const float* __restrict__ y,
                                                    const float* __restrict__ stats, const float* __restrict__ grad_loss,
                                                    const float* __restrict__ grad_rel, float* __restrict__ gx, int B, long per,
                                                    int size_average) {
  const int b = blockIdx.y;
  const float coef = rel_coef(stats, grad_loss, grad_rel, b, B, size_average);
  const float* xb = x + (long)b * per;
  const float* yb = y + (long)b * per;
  float* gb = gx + (long)b * per;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) gb[i] = coef * (xb[i] - yb[i]);
}

}  // namespace rpde

using namespace rpde;

extern "C" {

int rpde_rel_l2_fwd(const float* x, const float* y, float* rel, float* loss, float* stats, int B, int64_t per,
                    int size_average, void* stream) {
  RPDE_CHECK_ARG(x && y && stats && B > 0 && per > 0, "rel_l2_fwd: bad arguments");
  hipStream_t st = as_stream(stream);
  // partial sums live behind the stats the caller keeps: stats has 2*B floats,
  // the partials need 2*B*L2_BLOCKS more -> caller allocates stats with
  // rpde_rel_l2_stats_elems(B) floats.
  float* part = stats + 2L * B;
  hipLaunchKernelGGL(k_rel_l2_partial, dim3(L2_BLOCKS, B), dim3(256), 0, st, x, y, part, (long)per);
  RPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_rel_l2_final, dim3(1), dim3(256), 0, st, part, L2_BLOCKS, rel, loss, stats, B, size_average);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int64_t rpde_rel_l2_stats_elems(int B) { return 2L * B * (1 + L2_BLOCKS); }

int rpde_rel_l2_bwd(const float* x, const float* y, const float* stats, const float* grad_loss, const float* grad_rel,
                    float* grad_x, int B, int64_t per, int size_average, void* stream) {
  RPDE_CHECK_ARG(x && y && stats && grad_x && (grad_loss || grad_rel), "rel_l2_bwd: bad arguments");
  long nb = (per + 1023) / 1024; if (nb > 256) nb = 256; if (nb < 1) nb = 1;
  hipLaunchKernelGGL(k_rel_l2_bwd, dim3((unsigned)nb, B), dim3(256), 0, as_stream(stream), x, y, stats, grad_loss, grad_rel, grad_x, B, (long)per, size_average);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

}  // extern "C"
