// Mode-weighted relative L2 loss (utils/loss.py SpectralRelativeL2Loss; no counterpart in the reference)
//   E(z)[b] = sum_c sum_k  omega_k c_kx / (M N) |Z[b,c,k]|^2,   Z = rfft / rfft2 of z, unnormalised,
//   rel[b]  = sqrt(E(x - y)[b]) / (sqrt(E(y)[b]) + REL_EPS),     c_kx = 1 at kx = 0 and (even N) kx = N/2, else 2
// on the full-spectrum real 2-D DFT of cf_dft.h (cf_rfft2_plans): analysis along N, for M > 1 the complex column DFT
// keeping every row in fft order.  A spectrum is the half spectrum of halfspec.h over B*C images (the plan's table rows
// past N/2 are zero).  The difference (rel_diff), the tail (rel_final) and the backward coefficient (rel_coef) are the
// family's, rel_loss.h; what is this loss's own:
//   k_wl2_energy   omega_k c_kx |Z|^2 summed per (field, sample, slot) in float64, for rel_final
//   k_wl2_weight   backward: coef_b omega_k D (padded columns zero), then the inverse transform:
//                  d rel[b] / d x = coef_b irfft(omega . rfft(x - y))
#include "halfspec.h"
#include "rel_loss.h"
#include "wave.h"

namespace rpde {

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

// grid (blocks, B): w[b] = coef_b omega D[b]; the padded columns (kx >= K) are written as zeros
__global__ __launch_bounds__(256) void k_wl2_weight(const float* __restrict__ sd, const float* __restrict__ omega,
                                                    const float* __restrict__ stats, const float* __restrict__ grad_loss,
                                                    const float* __restrict__ grad_rel, float* __restrict__ w, Wl2Geom g,
                                                    int size_average) {
  const int b = blockIdx.y;
  const float coef = rel_coef(stats, grad_loss, grad_rel, b, g.B, size_average);
  const long per = (long)g.C * g.M * 2 * g.kp;
  const float* __restrict__ sp = sd + (long)b * per;
  float* __restrict__ wp = w + (long)b * per;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < per; e += (long)gridDim.x * 256) {
    const int kx = (int)(e % g.kp);
    const int ky = (int)((e / (2L * g.kp)) % g.M);
    wp[e] = kx < g.K ? (coef * omega[(long)ky * g.K + kx]) * sp[e] : 0.f;
  }
}

static Wl2Geom wl2_geom(int B, int C, int M, int N) {
  Wl2Geom g{hs_geom(B * C, M, N), B, C, 1};
  g.S = rel_slots((long)C * hs_per(g));
  return g;
}

}  // namespace rpde

using namespace rpde;

extern "C" {

size_t rpde_wrel_l2_spec_elems(int B, int C, int M, int N) {
  return hs_loss_dims_ok(B, C, M, N) ? hs_elems(hs_geom(B * C, M, N)) : 0;
}

// forward: the difference, the target's spectrum, the row spectra, the partial sums (doubles)
struct Wl2FwdWork {
  float *d, *sy, *s1; double* part;
  Wl2FwdWork(Arena& ar, const HalfSpec& g, int B)
      : d(ar.take((size_t)g.images * g.M * g.N)), sy(ar.take(hs_elems(g))), s1(ar.take(hs_elems(g))),
        part(reinterpret_cast<double*>(ar.take((size_t)2 * 2 * B * REL_SLOTS))) {}
};
// backward: the weighted spectrum and the row spectra
struct Wl2BwdWork {
  float *w, *t1;
  Wl2BwdWork(Arena& ar, const HalfSpec& g) : w(ar.take(hs_elems(g))), t1(ar.take(hs_elems(g))) {}
};

size_t rpde_wrel_l2_ws_bytes(int B, int C, int M, int N) {
  if (!hs_loss_dims_ok(B, C, M, N)) return 0;
  const HalfSpec g = hs_geom(B * C, M, N);
  return ws_max(ws_measure<Wl2FwdWork>(g, B), ws_measure<Wl2BwdWork>(g));
}

int rpde_wrel_l2_fwd(const float* x, const float* y, const float* omega, float* rel, float* loss, float* stats, float* spec_d,
                     int B, int C, int M, int N, int size_average, void* ws, size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(x && y && omega && stats && spec_d && ws, "wrel_l2_fwd: null pointer");
  RPDE_CHECK_ARG(hs_loss_dims_ok(B, C, M, N), "wrel_l2_fwd: bad B=%d C=%d M=%d N=%d (axes 2 .. %d; M = 1: one-dimensional)", B, C,
                 M, N, HS_MAX_N);
  const Wl2Geom g = wl2_geom(B, C, M, N);
  RPDE_CARVE("wrel_l2_fwd", Wl2FwdWork, w, ws, ws_bytes, g, B);
  hipStream_t st = as_stream(stream);
  RPDE_TRY(rel_diff(x, y, w.d, (long)g.images * M * N, st));
  RPDE_TRY(hs_rfft(g, w.d, w.s1, spec_d, st));
  RPDE_TRY(hs_rfft(g, y, w.s1, w.sy, st));
  hipLaunchKernelGGL(k_wl2_energy, dim3(g.S, B, 2), dim3(256), 0, st, spec_d, w.sy, omega, w.part, g);
  RPDE_LAUNCH_CHECK();
  return rel_final(w.part, rel, loss, stats, B, g.S, 1.0 / ((double)M * (double)N), size_average, st);
}

int rpde_wrel_l2_bwd(const float* spec_d, const float* omega, const float* stats, const float* grad_loss, const float* grad_rel,
                     float* grad_x, int B, int C, int M, int N, int size_average, void* ws, size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(spec_d && omega && stats && grad_x && ws && (grad_loss || grad_rel), "wrel_l2_bwd: null pointer");
  RPDE_CHECK_ARG(hs_loss_dims_ok(B, C, M, N), "wrel_l2_bwd: bad B=%d C=%d M=%d N=%d (axes 2 .. %d; M = 1: one-dimensional)", B, C,
                 M, N, HS_MAX_N);
  const Wl2Geom g = wl2_geom(B, C, M, N);
  RPDE_CARVE("wrel_l2_bwd", Wl2BwdWork, w, ws, ws_bytes, g);
  hipStream_t st = as_stream(stream);
  const long per = (long)C * hs_per(g);
  long nb = (per + 1023) / 1024;
  if (nb > 256) nb = 256;
  hipLaunchKernelGGL(k_wl2_weight, dim3((unsigned)nb, B), dim3(256), 0, st, spec_d, omega, stats, grad_loss, grad_rel, w.w, g,
                     size_average);
  RPDE_LAUNCH_CHECK();
  return hs_irfft(g, w.w, w.t1, grad_x, st);
}

}  // extern "C"
