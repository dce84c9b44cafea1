// Mode-weighted relative L2 loss (utils/loss.py SpectralRelativeL2Loss; no counterpart in the reference)
//   E(z)[b] = sum_c sum_k  omega_k c_kx / (M N) |Z[b,c,k]|^2,   Z = rfft / rfft2 of z, unnormalised,
//   rel[b]  = sqrt(E(x - y)[b]) / (sqrt(E(y)[b]) + 1e-8),        c_kx = 1 at kx = 0 and (even N) kx = N/2, else 2
// on the full-spectrum real 2-D DFT of cf_dft.h (cf_rfft2_plans): analysis along N, for M > 1 the complex column DFT
// keeping every row in fft order.  A spectrum is the half spectrum of halfspec.h over B*C images (the plan's table rows
// past N/2 are zero).  The small kernels around the transforms:
//   k_wl2_diff     d = x - y in fp32 BEFORE the transform (freq_energy.hip has the reason: for a decent model the
//                  difference of two spectra loses the digits, the spectrum of the difference does not)
//   k_wl2_energy   omega_k c_kx |Z|^2 summed per (field, sample, slot) in float64; k_wl2_final adds the slots in fixed
//                  order -- the k_rel_l2_partial / k_rel_l2_final pattern, no atomics: identical calls, identical bits
//   k_wl2_weight   backward: coef_b omega_k D, coef_b = g_b / (sqrt(E_d) (sqrt(E_y) + 1e-8)) formed from the saved
//                  stats and the upstream gradient on the device (0 where E_d = 0, as k_rel_l2_bwd), then the inverse
//                  transform: d rel[b] / d x = coef_b irfft(omega . rfft(x - y))
#include "halfspec.h"
#include "wave.h"

namespace rpde {

constexpr int WL2_SLOTS = 32;        // partial sums per (field, sample) at most

__global__ __launch_bounds__(256) void k_wl2_diff(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ d,
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

struct Wl2Geom : HalfSpec { int B, C, S; };     // B C images; S partial sums per (field, sample)

__device__ __forceinline__ float wl2_mult(int kx, int N) { return (kx == 0 || (N % 2 == 0 && kx == N / 2)) ? 1.f : 2.f; }

// grid (S, B, 2): field 0 = spectrum of x - y, field 1 = spectrum of y; part[(f B + b) S + slot]
__global__ __launch_bounds__(256) void k_wl2_energy(const float* __restrict__ sd, const float* __restrict__ sy,
                                                    const float* __restrict__ omega, double* __restrict__ part, Wl2Geom g) {
  __shared__ double red[4];
  const int b = blockIdx.y, f = blockIdx.z;
  const long per = (long)g.C * g.M * 2 * g.kp;
  const float* __restrict__ sp = (f ? sy : sd) + (long)b * per;
  double acc = 0.0;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < per; e += (long)gridDim.x * 256) {
    const int kx = (int)(e % g.kp);
    if (kx >= g.K) continue;
    const int ky = (int)((e / (2L * g.kp)) % g.M);
    const float v = sp[e];
    acc += (double)(omega[(long)ky * g.K + kx] * wl2_mult(kx, g.N)) * ((double)v * (double)v);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[((long)f * g.B + b) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one workgroup: stats[b] = (sqrt E_d, sqrt E_y), rel[b], loss = mean / sum
__global__ __launch_bounds__(256) void k_wl2_final(const double* __restrict__ part, float* __restrict__ rel, float* __restrict__ loss,
                                                   float* __restrict__ stats, Wl2Geom g, int size_average) {
  __shared__ double red[256];
  const double inv = 1.0 / ((double)g.M * (double)g.N);
  double acc = 0.0;
  for (int b = threadIdx.x; b < g.B; b += 256) {
    double ed = 0.0, ey = 0.0;
    for (int j = 0; j < g.S; ++j) { ed += part[(long)b * g.S + j]; ey += part[((long)g.B + b) * g.S + j]; }
    const float dn = (float)sqrt(ed * inv), yn = (float)sqrt(ey * inv);
    const float r = dn / (yn + 1e-8f);
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
  if (threadIdx.x == 0 && loss) *loss = (float)(size_average ? red[0] / g.B : red[0]);
}

// grid (blocks, B): w[b] = coef_b omega D[b]; the padded columns (kx >= K) are written as zeros
__global__ __launch_bounds__(256) void k_wl2_weight(const float* __restrict__ sd, const float* __restrict__ omega,
                                                    const float* __restrict__ stats, const float* __restrict__ grad_loss,
                                                    const float* __restrict__ grad_rel, float* __restrict__ w, Wl2Geom g,
                                                    int size_average) {
  const int b = blockIdx.y;
  const float dn = stats[2 * b], yn = stats[2 * b + 1];
  const float gr = grad_rel ? grad_rel[b] : (size_average ? grad_loss[0] / g.B : grad_loss[0]);
  const float coef = dn > 0.f ? gr / (dn * (yn + 1e-8f)) : 0.f;
  const long per = (long)g.C * g.M * 2 * g.kp;
  const float* __restrict__ sp = sd + (long)b * per;
  float* __restrict__ wp = w + (long)b * per;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < per; e += (long)gridDim.x * 256) {
    const int kx = (int)(e % g.kp);
    const int ky = (int)((e / (2L * g.kp)) % g.M);
    wp[e] = kx < g.K ? (coef * omega[(long)ky * g.K + kx]) * sp[e] : 0.f;
  }
}

static bool wl2_dims_ok(int B, int C, int M, int N) {
  return B > 0 && C > 0 && M >= 1 && N >= 2 && M <= HS_MAX_N && N <= HS_MAX_N && (long)B * C * M < (1L << 31);
}
static Wl2Geom wl2_geom(int B, int C, int M, int N) {
  Wl2Geom g{hs_geom(B * C, M, N), B, C, 1};
  const long per = (long)C * hs_per(g);
  g.S = (int)((per + 2047) / 2048 < WL2_SLOTS ? (per + 2047) / 2048 : WL2_SLOTS);
  return g;
}

}  // namespace rpde

using namespace rpde;

extern "C" {

size_t rpde_wrel_l2_spec_elems(int B, int C, int M, int N) {
  return wl2_dims_ok(B, C, M, N) ? hs_elems(hs_geom(B * C, M, N)) : 0;
}

size_t rpde_wrel_l2_ws_bytes(int B, int C, int M, int N) {
  if (!wl2_dims_ok(B, C, M, N)) return 0;
  const size_t spec = rpde_wrel_l2_spec_elems(B, C, M, N);
  // forward: the difference, the target's spectrum, the row spectra, the partial sums (doubles); the backward needs less
  return arena_bytes((size_t)B * C * M * N) + 2 * arena_bytes(spec) + arena_bytes((size_t)2 * 2 * B * WL2_SLOTS);
}

int rpde_wrel_l2_fwd(const float* x, const float* y, const float* omega, float* rel, float* loss, float* stats, float* spec_d,
                     int B, int C, int M, int N, int size_average, void* ws, size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(x && y && omega && stats && spec_d && ws, "wrel_l2_fwd: null pointer");
  RPDE_CHECK_ARG(wl2_dims_ok(B, C, M, N), "wrel_l2_fwd: bad B=%d C=%d M=%d N=%d (axes 2 .. %d; M = 1: one-dimensional)", B, C, M, N,
                 HS_MAX_N);
  const Wl2Geom g = wl2_geom(B, C, M, N);
  const size_t spec = hs_elems(g);
  Arena ar(ws, ws_bytes);
  float* d = ar.take((size_t)g.images * M * N);
  float* sy = ar.take(spec);
  float* s1 = ar.take(spec);
  double* part = reinterpret_cast<double*>(ar.take((size_t)2 * 2 * B * WL2_SLOTS));
  if (!ar.ok()) { set_error("wrel_l2_fwd: workspace too small"); return RPDE_ERR_WORKSPACE; }
  hipStream_t st = as_stream(stream);
  const long total = (long)g.images * M * N;
  const int vec = total % 4 == 0 && al16(x) && al16(y) && al16(d);
  long nb = ((vec ? total / 4 : total) + 255) / 256;
  if (nb > 2048) nb = 2048;
  hipLaunchKernelGGL(k_wl2_diff, dim3((unsigned)nb), dim3(256), 0, st, x, y, d, total, vec);
  RPDE_LAUNCH_CHECK();
  RPDE_TRY(hs_rfft(g, d, s1, spec_d, st));
  RPDE_TRY(hs_rfft(g, y, s1, sy, st));
  hipLaunchKernelGGL(k_wl2_energy, dim3(g.S, B, 2), dim3(256), 0, st, spec_d, sy, omega, part, g);
  RPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_wl2_final, dim3(1), dim3(256), 0, st, part, rel, loss, stats, g, size_average);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_wrel_l2_bwd(const float* spec_d, const float* omega, const float* stats, const float* grad_loss, const float* grad_rel,
                     float* grad_x, int B, int C, int M, int N, int size_average, void* ws, size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(spec_d && omega && stats && grad_x && ws && (grad_loss || grad_rel), "wrel_l2_bwd: null pointer");
  RPDE_CHECK_ARG(wl2_dims_ok(B, C, M, N), "wrel_l2_bwd: bad B=%d C=%d M=%d N=%d (axes 2 .. %d; M = 1: one-dimensional)", B, C, M, N,
                 HS_MAX_N);
  const Wl2Geom g = wl2_geom(B, C, M, N);
  const size_t spec = hs_elems(g);
  Arena ar(ws, ws_bytes);
  float* w = ar.take(spec);
  float* t1 = ar.take(spec);
  if (!ar.ok()) { set_error("wrel_l2_bwd: workspace too small"); return RPDE_ERR_WORKSPACE; }
  hipStream_t st = as_stream(stream);
  const long per = (long)C * hs_per(g);
  long nb = (per + 1023) / 1024;
  if (nb > 256) nb = 256;
  hipLaunchKernelGGL(k_wl2_weight, dim3((unsigned)nb, B), dim3(256), 0, st, spec_d, omega, stats, grad_loss, grad_rel, w, g,
                     size_average);
  RPDE_LAUNCH_CHECK();
  return hs_irfft(g, w, t1, grad_x, st);
}

}  // extern "C"
