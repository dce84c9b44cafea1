// The streaming kernels of the Navier-Stokes vorticity step that the generator (ns_solver.hip) and the vorticity
// equation residual (ns_residual.hip) share: the update and fan-out of the derivative spectra, the advection product and
// the scaling of spectra by a table.  A thread owns one 16-byte group of kx for both re and im.
#pragma once
#include "halfspec.h"

namespace rpde {

constexpr float NS_TWO_PI = 6.28318530717958647692f;

// the step's tables; the plain step has, and so passes, only the first three
template <bool SCALAR> struct NsTables { const float *cw, *cf, *il; };
template <> struct NsTables<true> { const float *cw, *cf, *il, *dw, *df; float beta; };

// MODE 0: fan-out only (the first step of a call: the state is read, not written)
//      1: update, then fan-out of the new state
//      2: update only (the last step of a call)
// grid (blocks, B), g.images = B.  F is [1 | 2][B] spectra (F_w, F_c), D is [4 | 6][B]: q^ = 2 pi i k2 psi,
// v^ = -2 pi i k1 psi, w_1^ = 2 pi i k1 W, w_2^ = 2 pi i k2 W, c_1^ = 2 pi i k1 C, c_2^ = 2 pi i k2 C, psi = W inv_lap.
// g_h has gstride floats between samples (0: one forcing for the batch).  Padded columns (kx > N/2) are written as
// zeros in the state and in D: the synthesis reads them.
template <int MODE, bool SCALAR>
__global__ __launch_bounds__(256) void k_ns_update_fanout(float* __restrict__ S, const float* __restrict__ F,
                                                          const float* __restrict__ gh, long gstride, NsTables<SCALAR> t,
                                                          float* __restrict__ D, HalfSpec g) {
  const int b = blockIdx.y;
  const int c4n = g.kp / 4, per4 = g.M * c4n;
  const long per = (long)g.M * 2 * g.kp, half = (long)g.images * per;
  float* __restrict__ Wb = S + (long)b * per;
  float* __restrict__ Cb = Wb + half;                   // the scalar's spectra and products: SCALAR only
  const float* __restrict__ Fw = F + (long)b * per;
  const float* __restrict__ Fc = Fw + half;
  const float* __restrict__ gb = gh + (long)b * gstride;
  float* __restrict__ Db = D + (long)b * per;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < per4; v += gridDim.x * 256) {
    const int ky = v / c4n, kx0 = (v - ky * c4n) * 4;
    const long ore = (long)ky * 2 * g.kp + kx0, oim = ore + g.kp, ot = (long)ky * g.kp + kx0;
    const float k1 = NS_TWO_PI * (float)(ky < g.M / 2 ? ky : ky - g.M);
    float wr[4], wi[4], cr[4], ci[4];
    ld4(Wb + ore, wr); ld4(Wb + oim, wi);
    if constexpr (SCALAR) { ld4(Cb + ore, cr); ld4(Cb + oim, ci); }
    if (MODE != 0) {
      float fr[4], fi[4], gr[4], gi[4], a[4], c[4];
      ld4(Fw + ore, fr); ld4(Fw + oim, fi);
      ld4(gb + ore, gr); ld4(gb + oim, gi);
      ld4(t.cw + ot, a); ld4(t.cf + ot, c);
      if constexpr (SCALAR) {
        float er[4], ei[4], p[4], q[4];
        ld4(Fc + ore, er); ld4(Fc + oim, ei);
        ld4(t.dw + ot, p); ld4(t.df + ot, q);
        const float bk = t.beta * k1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool live = kx0 + j < g.K;
          // F_w - beta 2 pi i k1 C = (F_re + bk C_im) + i (F_im - bk C_re), C of the old time level
          fr[j] = fmaf(bk, ci[j], fr[j]);
          fi[j] = fmaf(-bk, cr[j], fi[j]);
          cr[j] = live ? fmaf(p[j], cr[j], -(q[j] * er[j])) : 0.f;
          ci[j] = live ? fmaf(p[j], ci[j], -(q[j] * ei[j])) : 0.f;
        }
        st4(Cb + ore, cr); st4(Cb + oim, ci);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool live = kx0 + j < g.K;
        wr[j] = live ? fmaf(a[j], wr[j], fmaf(-c[j], fr[j], gr[j])) : 0.f;
        wi[j] = live ? fmaf(a[j], wi[j], fmaf(-c[j], fi[j], gi[j])) : 0.f;
      }
      st4(Wb + ore, wr); st4(Wb + oim, wi);
    }
    if (MODE != 2) {
      float li[4], qr[4], qi[4], vr[4], vi[4], xr[4], xi[4], yr[4], yi[4];
      ld4(t.il + ot, li);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool live = kx0 + j < g.K;
        const float k2 = NS_TWO_PI * (float)(kx0 + j);
        const float pr = wr[j] * li[j], pi = wi[j] * li[j];
        qr[j] = live ? -k2 * pi : 0.f;     qi[j] = live ? k2 * pr : 0.f;
        vr[j] = live ? k1 * pi : 0.f;      vi[j] = live ? -k1 * pr : 0.f;
        xr[j] = live ? -k1 * wi[j] : 0.f;  xi[j] = live ? k1 * wr[j] : 0.f;
        yr[j] = live ? -k2 * wi[j] : 0.f;  yi[j] = live ? k2 * wr[j] : 0.f;
      }
      st4(Db + ore, qr);            st4(Db + oim, qi);
      st4(Db + half + ore, vr);     st4(Db + half + oim, vi);
      st4(Db + 2 * half + ore, xr); st4(Db + 2 * half + oim, xi);
      st4(Db + 3 * half + ore, yr); st4(Db + 3 * half + oim, yi);
      if constexpr (SCALAR) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool live = kx0 + j < g.K;
          const float k2 = NS_TWO_PI * (float)(kx0 + j);
          xr[j] = live ? -k1 * ci[j] : 0.f;  xi[j] = live ? k1 * cr[j] : 0.f;
          yr[j] = live ? -k2 * ci[j] : 0.f;  yi[j] = live ? k2 * cr[j] : 0.f;
        }
        st4(Db + 4 * half + ore, xr); st4(Db + 4 * half + oim, xi);
        st4(Db + 5 * half + ore, yr); st4(Db + 5 * half + oim, yi);
      }
    }
  }
}

// P [4 | 6][B M N] = (q, v, w_1, w_2, c_1, c_2) -> out [1 | 2][B M N] = (q w_1 + v w_2, q c_1 + v c_2); n4 float4 groups
// per field (M, N even and the workspace pieces 256-byte aligned: always whole, aligned groups)
template <bool SCALAR>
__global__ __launch_bounds__(256) void k_ns_advect(const float* __restrict__ P, float* __restrict__ out, long n4) {
  const float4* __restrict__ q = reinterpret_cast<const float4*>(P);
  const float4 *__restrict__ v = q + n4, *__restrict__ w1 = q + 2 * n4, *__restrict__ w2 = q + 3 * n4;
  const float4 *__restrict__ c1 = q + 4 * n4, *__restrict__ c2 = q + 5 * n4;
  float4* __restrict__ o = reinterpret_cast<float4*>(out);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 a = q[i], b = v[i], c = w1[i], d = w2[i];
    o[i] = make_float4(fmaf(a.x, c.x, b.x * d.x), fmaf(a.y, c.y, b.y * d.y), fmaf(a.z, c.z, b.z * d.z), fmaf(a.w, c.w, b.w * d.w));
    if constexpr (SCALAR) {
      const float4 e = c1[i], f = c2[i];
      o[n4 + i] = make_float4(fmaf(a.x, e.x, b.x * f.x), fmaf(a.y, e.y, b.y * f.y), fmaf(a.z, e.z, b.z * f.z), fmaf(a.w, e.w, b.w * f.w));
    }
  }
}

// out = table . spec over `images` spectra, table [M][kp] (g_h = dt / (1 + a) f_h, once per solve); grid (blocks, images)
static __global__ __launch_bounds__(256) void k_ns_scale(const float* __restrict__ spec, const float* __restrict__ table,
                                                  float* __restrict__ out, HalfSpec g) {
  const int c4n = g.kp / 4, per4 = g.M * 2 * c4n;
  const long per = (long)g.M * 2 * g.kp;
  const float* __restrict__ sb = spec + (long)blockIdx.y * per;
  float* __restrict__ ob = out + (long)blockIdx.y * per;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < per4; v += gridDim.x * 256) {
    const int row = v / c4n, kx0 = (v - row * c4n) * 4;          // row = 2 ky + (re | im)
    float s[4], t[4];
    ld4(sb + (long)row * g.kp + kx0, s);
    ld4(table + (long)(row >> 1) * g.kp + kx0, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = kx0 + j < g.K ? s[j] * t[j] : 0.f;
    st4(ob + (long)row * g.kp + kx0, s);
  }
}

}  // namespace rpde
