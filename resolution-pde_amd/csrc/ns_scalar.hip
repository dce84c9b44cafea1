// Active-scalar Navier-Stokes generator on the unit periodic square: the vorticity step of ns_solver.hip with a scalar c
// that the flow advects and that drives the flow back through buoyancy along axis 2 (Boussinesq: the curl of the force
// is beta dc/dx1).  Pseudo-spectral, Crank-Nicolson on both diffusions, explicit advection, buoyancy and forcing, 2/3
// de-aliasing.  gfx950, wave64.
//
// The state is two half spectra per sample, S = [W_0 .. W_{B-1}, C_0 .. C_{B-1}], each [M][re|im][kp] (halfspec.h).  One
// step is six launches on the caller's stream, no host synchronisation:
//   rowdft + synthesis    one batched inverse 2-D transform of the 6B derivative spectra (q^, v^, w_1^, w_2^, c_1^, c_2^)
//   k_nsc_advect          the two products q w_1 + v w_2 and q c_1 + v c_2
//   analysis + rowdft     one forward 2-D transform of the 2B products
//   k_nsc_update_fanout   W <- c_w W - c_f (F_w - beta 2 pi i k1 C) + g_h with the OLD C, C <- d_w C - d_f F_c, and from
//                         the NEW W and C the six derivative spectra of the next step
// with the tables formed by the caller in float64 and rounded to fp32 once (rpde.ops.nsc2d_tables).  The transforms are
// hs_rfft / hs_irfft; g_h comes from rpde_ns2d_scale.  Everything here streams: a thread owns one 16-byte group of kx
// for both re and im, so a wave covers whole 128-byte lines of every array it reads or writes.  No atomics anywhere:
// identical calls give identical bits.
#include "halfspec.h"

namespace rpde {

constexpr float NSC_TWO_PI = 6.28318530717958647692f;

// B within gridDim.y and the 6B derivative images within the limits of a generator grid
inline bool nsc_dims_ok(int B, int M, int N) { return B > 0 && B <= 65535 / 6 && hs_dims2_ok(6 * B, M, N); }

#define NSC_CHECK_DIMS(what, B, M, N)                                                                                   \
  RPDE_CHECK_ARG(nsc_dims_ok(B, M, N), what ": bad B=%d M=%d N=%d (even axes %d .. %d, 24 B max(M, N) < 2^31, 6 B <= 65535)", \
                 B, M, N, HS_MIN_N, HS_MAX_N)

// MODE 0: fan-out only (the first step of a call: S is read, not written)
//      1: update, then fan-out of the new W and C
//      2: update only (the last step of a call)
// grid (blocks, B), g.images = B.  F is [2][B] spectra (F_w, F_c), D is [6][B]: q^ = 2 pi i k2 psi, v^ = -2 pi i k1 psi,
// w_1^ = 2 pi i k1 W, w_2^ = 2 pi i k2 W, c_1^ = 2 pi i k1 C, c_2^ = 2 pi i k2 C, psi = W inv_lap.  g_h has gstride floats
// between samples (0: one forcing for the batch).  Padded columns (kx > N/2) are written as zeros in S and in D: the
// synthesis reads them.
template <int MODE>
__global__ __launch_bounds__(256) void k_nsc_update_fanout(float* __restrict__ S, const float* __restrict__ F,
                                                           const float* __restrict__ gh, long gstride,
                                                           const float* __restrict__ cw, const float* __restrict__ cf,
                                                           const float* __restrict__ dw, const float* __restrict__ df,
                                                           const float* __restrict__ il, float beta,
                                                           float* __restrict__ D, HalfSpec g) {
  const int b = blockIdx.y;
  const int c4n = g.kp / 4, per4 = g.M * c4n;
  const long per = (long)g.M * 2 * g.kp, half = (long)g.images * per;
  float* __restrict__ Wb = S + (long)b * per;
  float* __restrict__ Cb = Wb + half;
  const float* __restrict__ Fw = F + (long)b * per;
  const float* __restrict__ Fc = Fw + half;
  const float* __restrict__ gb = gh + (long)b * gstride;
  float* __restrict__ Db = D + (long)b * per;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < per4; v += gridDim.x * 256) {
    const int ky = v / c4n, kx0 = (v - ky * c4n) * 4;
    const long ore = (long)ky * 2 * g.kp + kx0, oim = ore + g.kp, ot = (long)ky * g.kp + kx0;
    const float k1 = NSC_TWO_PI * (float)(ky < g.M / 2 ? ky : ky - g.M);
    float wr[4], wi[4], cr[4], ci[4];
    ld4(Wb + ore, wr); ld4(Wb + oim, wi);
    ld4(Cb + ore, cr); ld4(Cb + oim, ci);
    if (MODE != 0) {
      float fr[4], fi[4], er[4], ei[4], gr[4], gi[4], a[4], c[4], p[4], q[4];
      ld4(Fw + ore, fr); ld4(Fw + oim, fi);
      ld4(Fc + ore, er); ld4(Fc + oim, ei);
      ld4(gb + ore, gr); ld4(gb + oim, gi);
      ld4(cw + ot, a);   ld4(cf + ot, c);
      ld4(dw + ot, p);   ld4(df + ot, q);
      const float bk = beta * k1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool live = kx0 + j < g.K;
        // F_w - beta 2 pi i k1 C = (F_re + bk C_im) + i (F_im - bk C_re), C of the old time level
        const float tr = fmaf(bk, ci[j], fr[j]), ti = fmaf(-bk, cr[j], fi[j]);
        wr[j] = live ? fmaf(a[j], wr[j], fmaf(-c[j], tr, gr[j])) : 0.f;
        wi[j] = live ? fmaf(a[j], wi[j], fmaf(-c[j], ti, gi[j])) : 0.f;
        cr[j] = live ? fmaf(p[j], cr[j], -(q[j] * er[j])) : 0.f;
        ci[j] = live ? fmaf(p[j], ci[j], -(q[j] * ei[j])) : 0.f;
      }
      st4(Wb + ore, wr); st4(Wb + oim, wi);
      st4(Cb + ore, cr); st4(Cb + oim, ci);
    }
    if (MODE != 2) {
      float li[4], qr[4], qi[4], vr[4], vi[4], xr[4], xi[4], yr[4], yi[4];
      ld4(il + ot, li);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool live = kx0 + j < g.K;
        const float k2 = NSC_TWO_PI * (float)(kx0 + j);
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
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool live = kx0 + j < g.K;
        const float k2 = NSC_TWO_PI * (float)(kx0 + j);
        xr[j] = live ? -k1 * ci[j] : 0.f;  xi[j] = live ? k1 * cr[j] : 0.f;
        yr[j] = live ? -k2 * ci[j] : 0.f;  yi[j] = live ? k2 * cr[j] : 0.f;
      }
      st4(Db + 4 * half + ore, xr); st4(Db + 4 * half + oim, xi);
      st4(Db + 5 * half + ore, yr); st4(Db + 5 * half + oim, yi);
    }
  }
}

// S -> D [B][3] spectra (C, q^, v^), sample-major: their inverse transform is out [B, 3, M, N] = (c, q, v) as it stands.
// grid (blocks, B), g.images = B; padded columns zero
__global__ __launch_bounds__(256) void k_nsc_fields_fanout(const float* __restrict__ S, const float* __restrict__ il,
                                                           float* __restrict__ D, HalfSpec g) {
  const int b = blockIdx.y;
  const int c4n = g.kp / 4, per4 = g.M * c4n;
  const long per = (long)g.M * 2 * g.kp, half = (long)g.images * per;
  const float* __restrict__ Wb = S + (long)b * per;
  const float* __restrict__ Cb = Wb + half;
  float* __restrict__ Db = D + (long)b * 3 * per;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < per4; v += gridDim.x * 256) {
    const int ky = v / c4n, kx0 = (v - ky * c4n) * 4;
    const long ore = (long)ky * 2 * g.kp + kx0, oim = ore + g.kp, ot = (long)ky * g.kp + kx0;
    const float k1 = NSC_TWO_PI * (float)(ky < g.M / 2 ? ky : ky - g.M);
    float wr[4], wi[4], cr[4], ci[4], li[4], qr[4], qi[4], vr[4], vi[4];
    ld4(Wb + ore, wr); ld4(Wb + oim, wi);
    ld4(Cb + ore, cr); ld4(Cb + oim, ci);
    ld4(il + ot, li);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool live = kx0 + j < g.K;
      const float k2 = NSC_TWO_PI * (float)(kx0 + j);
      const float pr = wr[j] * li[j], pi = wi[j] * li[j];
      cr[j] = live ? cr[j] : 0.f;      ci[j] = live ? ci[j] : 0.f;
      qr[j] = live ? -k2 * pi : 0.f;   qi[j] = live ? k2 * pr : 0.f;
      vr[j] = live ? k1 * pi : 0.f;    vi[j] = live ? -k1 * pr : 0.f;
    }
    st4(Db + ore, cr);           st4(Db + oim, ci);
    st4(Db + per + ore, qr);     st4(Db + per + oim, qi);
    st4(Db + 2 * per + ore, vr); st4(Db + 2 * per + oim, vi);
  }
}

// P [6][B M N] = (q, v, w_1, w_2, c_1, c_2) -> out [2][B M N] = (q w_1 + v w_2, q c_1 + v c_2); n4 float4 groups per field
// (M, N even and the workspace pieces 256-byte aligned: always whole, aligned groups)
__global__ __launch_bounds__(256) void k_nsc_advect(const float* __restrict__ P, float* __restrict__ out, long n4) {
  const float4* __restrict__ q = reinterpret_cast<const float4*>(P);
  const float4 *__restrict__ v = q + n4, *__restrict__ w1 = q + 2 * n4, *__restrict__ w2 = q + 3 * n4;
  const float4 *__restrict__ c1 = q + 4 * n4, *__restrict__ c2 = q + 5 * n4;
  float4* __restrict__ o = reinterpret_cast<float4*>(out);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 a = q[i], b = v[i], c = w1[i], d = w2[i], e = c1[i], f = c2[i];
    o[i] = make_float4(fmaf(a.x, c.x, b.x * d.x), fmaf(a.y, c.y, b.y * d.y), fmaf(a.z, c.z, b.z * d.z), fmaf(a.w, c.w, b.w * d.w));
    o[n4 + i] = make_float4(fmaf(a.x, e.x, b.x * f.x), fmaf(a.y, e.y, b.y * f.y), fmaf(a.z, e.z, b.z * f.z), fmaf(a.w, e.w, b.w * f.w));
  }
}

}  // namespace rpde

using namespace rpde;

extern "C" {

size_t rpde_nsc2d_ws_bytes(int B, int M, int N) {
  if (!nsc_dims_ok(B, M, N)) return 0;
  const size_t spec = hs_elems(hs_geom(B, M, N)), phys = (size_t)B * M * N;
  // rpde_nsc2d_steps: derivative spectra and their column stage (6B each), the six fields, their two products, the
  // products' row spectra and spectra; rpde_nsc2d_fields needs the first two pieces, 3B of each
  return 2 * arena_bytes(6 * spec) + arena_bytes(6 * phys) + arena_bytes(2 * phys) + 2 * arena_bytes(2 * spec);
}

int rpde_nsc2d_steps(float* S, const float* g_h, int g_batched, const float* c_w, const float* c_f, const float* d_w,
                     const float* d_f, const float* inv_lap, float beta, int B, int M, int N, int nsteps, void* ws,
                     size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(S && g_h && c_w && c_f && d_w && d_f && inv_lap && ws, "nsc2d_steps: null pointer");
  NSC_CHECK_DIMS("nsc2d_steps", B, M, N);
  HS_CHECK_WS("nsc2d_steps", ws);
  RPDE_CHECK_ARG(nsteps >= 0, "nsc2d_steps: nsteps %d < 0", nsteps);
  RPDE_CHECK_ARG(al16(S) && al16(g_h) && al16(c_w) && al16(c_f) && al16(d_w) && al16(d_f) && al16(inv_lap),
                 "nsc2d_steps: state, forcing and tables must be 16-byte aligned");
  const HalfSpec g = hs_geom(B, M, N), g2 = hs_geom(2 * B, M, N), g6 = hs_geom(6 * B, M, N);
  const size_t spec = hs_elems(g), phys = (size_t)B * M * N;
  Arena ar(ws, ws_bytes);
  float* D = ar.take(6 * spec);
  float* T1 = ar.take(6 * spec);
  float* P = ar.take(6 * phys);
  float* Fp = ar.take(2 * phys);
  float* S1 = ar.take(2 * spec);
  float* F = ar.take(2 * spec);
  if (!ar.ok()) { set_error("nsc2d_steps: workspace too small"); return RPDE_ERR_WORKSPACE; }
  if (nsteps == 0) return RPDE_OK;
  hipStream_t st = as_stream(stream);
  const dim3 ug = hs_grid((long)M * (g.kp / 4), B);
  const long gstride = g_batched ? (long)hs_per(g) : 0;
  const long n4 = (long)phys / 4;
  hipLaunchKernelGGL(k_nsc_update_fanout<0>, ug, dim3(256), 0, st, S, F, g_h, gstride, c_w, c_f, d_w, d_f, inv_lap, beta, D, g);
  RPDE_LAUNCH_CHECK();
  for (int j = 0; j < nsteps; ++j) {
    RPDE_TRY(hs_irfft(g6, D, T1, P, st));
    hipLaunchKernelGGL(k_nsc_advect, dim3(hs_blocks(n4, 2048)), dim3(256), 0, st, P, Fp, n4);
    RPDE_LAUNCH_CHECK();
    RPDE_TRY(hs_rfft(g2, Fp, S1, F, st));
    if (j + 1 < nsteps)
      hipLaunchKernelGGL(k_nsc_update_fanout<1>, ug, dim3(256), 0, st, S, F, g_h, gstride, c_w, c_f, d_w, d_f, inv_lap, beta, D, g);
    else
      hipLaunchKernelGGL(k_nsc_update_fanout<2>, ug, dim3(256), 0, st, S, F, g_h, gstride, c_w, c_f, d_w, d_f, inv_lap, beta, D, g);
    RPDE_LAUNCH_CHECK();
  }
  return RPDE_OK;
}

int rpde_nsc2d_fields(const float* S, const float* inv_lap, float* out, int B, int M, int N, void* ws, size_t ws_bytes,
                      void* stream) {
  RPDE_CHECK_ARG(S && inv_lap && out && ws, "nsc2d_fields: null pointer");
  NSC_CHECK_DIMS("nsc2d_fields", B, M, N);
  HS_CHECK_WS("nsc2d_fields", ws);
  RPDE_CHECK_ARG(al16(S) && al16(inv_lap) && al16(out), "nsc2d_fields: state, table and output must be 16-byte aligned");
  const HalfSpec g = hs_geom(B, M, N), g3 = hs_geom(3 * B, M, N);
  const size_t spec = hs_elems(g);
  Arena ar(ws, ws_bytes);
  float* D = ar.take(3 * spec);
  float* T1 = ar.take(3 * spec);
  if (!ar.ok()) { set_error("nsc2d_fields: workspace too small"); return RPDE_ERR_WORKSPACE; }
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_nsc_fields_fanout, hs_grid((long)M * (g.kp / 4), B), dim3(256), 0, st, S, inv_lap, D, g);
  RPDE_LAUNCH_CHECK();
  return hs_irfft(g3, D, T1, out, st);
}

}  // extern "C"
