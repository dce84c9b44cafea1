// Gradient-norm clipping and non-finite step skipping for the flat AdamW step, without a host read.
//   1. k_grad_sumsq_partial: sum of g^2 over the flat gradient buffer, squares and sums in float64 (fp32 squares
//      overflow from |g| ~ 1.8e19 and vanish below ~ 1e-23), one double per workgroup;
//   2. k_grad_norm_final: one workgroup adds the partials in fixed order, forms the norm and
//      torch.nn.utils.clip_grad_norm_'s scale = min(1, max_norm / (norm + 1e-6)), and writes the record clip_dev;
//   3. k_adamw_clip / k_adamw_tick_clip: the update of adamw.hip (the same adamw_one / adamw_tick) on clip_dev[1] * g,
//      and nothing at all when clip_dev[2] says that this step is skipped.
// No atomics: the grid depends on the length alone and every sum has a fixed order, so identical calls give identical
// bits.  clip_dev, 8 floats: [0] norm  [1] scale  [2] skipped (1.0 / 0.0)  [3] steps seen  [4] steps clipped
// [5] steps skipped  [6] largest finite norm  [7] sum of the finite norms.  The counters [3..5] are fp32: exact up to
// 2^24 steps between two resets (the training loop resets them every epoch).
#include "adamw.h"

namespace rpde {

constexpr int GN_MAX_BLOCKS = 1024;       // 4 workgroups per CU of an MI355X; also the length of the final sum

static int grad_norm_grid(long n4) {
  long g = (n4 + 255) / 256;
  if (g > GN_MAX_BLOCKS) g = GN_MAX_BLOCKS;
  if (g < 1) g = 1;
  return (int)g;
}

// scale * g as a rounded product of its own: without the contract flag the compiler may not fuse it into adamw_one's
// g - m, so the moments see one value of scale * g, and with scale 1 that value IS g
__device__ __forceinline__ float scaled(float g, float sc) {
#pragma clang fp contract(off)
  return g * sc;
}

__device__ __forceinline__ bool nonfinite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(256) void k_grad_sumsq_partial(const float* __restrict__ g, long n4, double* __restrict__ part) {
  __shared__ double red[4];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 a = reinterpret_cast<const float4*>(g)[i];
    const double x = (double)a.x, y = (double)a.y, z = (double)a.z, w = (double)a.w;
    s0 = fma(x, x, s0); s1 = fma(y, y, s1); s2 = fma(z, z, s2); s3 = fma(w, w, s3);
  }
  const double s = wave_sum((s0 + s1) + (s2 + s3));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void k_grad_norm_final(const double* __restrict__ part, int nblk, float max_norm,
                                                         int skip_nonfinite, float* __restrict__ clip) {
  __shared__ double red[256];
  double acc = 0.0;
  for (int j = threadIdx.x; j < nblk; j += 256) acc += part[j];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const float norm = (float)sqrt(red[0]);                    // the one rounding to fp32
  const bool measure_only = !(max_norm > 0.f) || nonfinite_f(max_norm);
  float scale = 1.f;
  if (!measure_only) {
    const float q = max_norm / (norm + 1e-6f);               // torch's constant; inf norm -> 0, NaN norm -> NaN
    scale = q > 1.f ? 1.f : q;                               // a NaN q fails the comparison and stays (torch.clamp)
  }
  const bool bad = nonfinite_f(norm);
  const bool skip = bad && skip_nonfinite != 0;
  clip[0] = norm;
  clip[1] = scale;
  clip[2] = skip ? 1.f : 0.f;
  clip[3] += 1.f;
  if (!skip && scale < 1.f) clip[4] += 1.f;
  if (skip) clip[5] += 1.f;
  if (!bad) {
    if (norm > clip[6]) clip[6] = norm;
    clip[7] += norm;
  }
}

template <bool DEV>
__global__ __launch_bounds__(256) void k_adamw_clip(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, long n4, AdamwScalars s,
                                                    const float* __restrict__ dev, const float* __restrict__ clip) {
  if (clip[2] != 0.f) return;                                // a skipped step touches nothing
  const float sc = clip[1];
  if (DEV) { s.step_size = dev[1]; s.bc2_sqrt = dev[2]; s.omlw = dev[5]; }
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    float4 pp = reinterpret_cast<float4*>(p)[i], mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    // with scale 1 the update equals the plain kernel's bit for bit
    adamw_one(pp.x, scaled(gg.x, sc), mm.x, vv.x, s); adamw_one(pp.y, scaled(gg.y, sc), mm.y, vv.y, s);
    adamw_one(pp.z, scaled(gg.z, sc), mm.z, vv.z, s); adamw_one(pp.w, scaled(gg.w, sc), mm.w, vv.w, s);
    reinterpret_cast<float4*>(p)[i] = pp; reinterpret_cast<float4*>(m)[i] = mm; reinterpret_cast<float4*>(v)[i] = vv;
  }
}

// the tick of adamw.hip; a skipped step leaves the counter and the words derived from it where they are
__global__ void k_adamw_tick_clip(float* dev, float b1, float b2, const float* __restrict__ clip) {
  if (clip[2] != 0.f) return;
  adamw_tick(dev, b1, b2);
}

static bool flat_ok(const void* p, const void* g, const void* m, const void* v, int64_t n) {
  return p && g && m && v && n > 0 && n % 4 == 0;
}
static bool flat_al16(const void* p, const void* g, const void* m, const void* v) { return al16(p) && al16(g) && al16(m) && al16(v); }

}  // namespace rpde

using namespace rpde;

extern "C" {

size_t rpde_grad_norm_ws_bytes(int64_t n) {
  if (n <= 0 || n % 4 != 0) return 0;
  return sizeof(double) * (size_t)grad_norm_grid((long)(n / 4));
}

int rpde_grad_norm(const float* g, int64_t n, float max_norm, int skip_nonfinite, float* clip_dev, void* ws, size_t ws_bytes,
                   void* stream) {
  RPDE_CHECK_ARG(g && clip_dev && ws && n > 0 && n % 4 == 0, "grad_norm: null buffer or length %ld not a multiple of 4", (long)n);
  RPDE_CHECK_ARG(max_norm == max_norm, "grad_norm: max_norm is NaN");
  RPDE_CHECK_ARG(al16(g) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0, "grad_norm: g must be 16-byte, ws 8-byte aligned");
  if (ws_bytes < rpde_grad_norm_ws_bytes(n)) {
    set_error("grad_norm: workspace of %zu bytes, %zu needed", ws_bytes, rpde_grad_norm_ws_bytes(n));
    return RPDE_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const int grid = grad_norm_grid((long)(n / 4));
  double* part = static_cast<double*>(ws);
  hipLaunchKernelGGL(k_grad_sumsq_partial, dim3(grid), dim3(256), 0, st, g, (long)(n / 4), part);
  RPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_grad_norm_final, dim3(1), dim3(256), 0, st, part, grid, max_norm, skip_nonfinite, clip_dev);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_adamw_step_clip(float* p, const float* g, float* m, float* v, int64_t n, float one_minus_lr_wd, float one_minus_b1,
                         float b2, float one_minus_b2, float step_size, float bc2_sqrt, float eps, const float* clip_dev,
                         void* stream) {
  RPDE_CHECK_ARG(flat_ok(p, g, m, v, n) && clip_dev, "adamw_step_clip: null buffer or length %ld not a multiple of 4", (long)n);
  RPDE_CHECK_ARG(flat_al16(p, g, m, v), "adamw_step_clip: buffers must be 16-byte aligned");
  const AdamwScalars s{one_minus_lr_wd, one_minus_b1, b2, one_minus_b2, step_size, bc2_sqrt, eps};
  hipLaunchKernelGGL(k_adamw_clip<false>, dim3(adamw_grid(n / 4)), dim3(256), 0, as_stream(stream), p, g, m, v, (long)(n / 4), s,
                     nullptr, clip_dev);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_adamw_step_dev_clip(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps,
                             float weight_decay, float* step_dev, const float* clip_dev, void* stream) {
  RPDE_CHECK_ARG(flat_ok(p, g, m, v, n) && step_dev && clip_dev, "adamw_step_dev_clip: bad arguments");
  RPDE_CHECK_ARG(flat_al16(p, g, m, v), "adamw_step_dev_clip: buffers must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  // lr / weight decay as in rpde_adamw_step_dev: an eager call stores its arguments (a skipped step too: they are
  // the host's values, not a result of the step), a call that is being captured leaves the device words alone
  if (!capturing(st)) RPDE_TRY(rpde_adamw_set_hyper_dev(step_dev, lr, weight_decay, stream));
  hipLaunchKernelGGL(k_adamw_tick_clip, dim3(1), dim3(1), 0, st, step_dev, b1, b2, clip_dev);
  RPDE_LAUNCH_CHECK();
  const AdamwScalars s{1.f, 1.f - b1, b2, 1.f - b2, 0.f, 1.f, eps};
  hipLaunchKernelGGL(k_adamw_clip<true>, dim3(adamw_grid(n / 4)), dim3(256), 0, st, p, g, m, v, (long)(n / 4), s, step_dev, clip_dev);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_adamw_apply_dev_clip(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps,
                              float weight_decay, const float* step_dev, const float* clip_dev, void* stream) {
  RPDE_CHECK_ARG(flat_ok(p, g, m, v, n) && step_dev && clip_dev, "adamw_apply_dev_clip: bad arguments");
  RPDE_CHECK_ARG(flat_al16(p, g, m, v), "adamw_apply_dev_clip: buffers must be 16-byte aligned");
  (void)lr; (void)weight_decay;           // (the step's values are on the device since rpde_adamw_step_dev_clip)
  const AdamwScalars s{1.f, 1.f - b1, b2, 1.f - b2, 0.f, 1.f, eps};
  hipLaunchKernelGGL(k_adamw_clip<true>, dim3(adamw_grid(n / 4)), dim3(256), 0, as_stream(stream), p, g, m, v, (long)(n / 4), s,
                     step_dev, clip_dev);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

}  // extern "C"
