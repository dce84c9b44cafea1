// Navier-Stokes vorticity generator on the unit periodic square (reference: data_generation/ns_2d.py): pseudo-spectral,
// Crank-Nicolson on the diffusion, explicit advection and forcing, 2/3 de-aliasing.  gfx950, wave64.
//
// The state is the half spectrum W = rfft2(w), [B][M][re|im][kp] (halfspec.h).  One step is six launches on the
// caller's stream, no host synchronisation:
//   rowdft + synthesis   one batched inverse 2-D transform of the 4B derivative spectra (q^, v^, w_x^, w_y^)
//   k_ns_advect          F_phys = q w_x + v w_y
//   analysis + rowdft    one forward 2-D transform of the B products
//   k_ns_update_fanout   W <- c_w W - c_f F + g_h, and from the NEW W the four derivative spectra of the next step
// with the coefficient tables formed by the caller in float64 and rounded to fp32 once:
//   a = dt visc lap / 2,  c_w = (1 - a) / (1 + a),  c_f = dt dealias / (1 + a),  g_h = dt / (1 + a) f_h,  inv_lap = 1 / lap.
// The transforms are the full-spectrum real 2-D DFT of cf_dft.h (hs_rfft / hs_irfft, GEMM form); the rfft2 / irfft2
// entries and the random field that seeds the solver are in halfspec.hip.  Everything else here streams: a thread owns
// one 16-byte group of kx for both re and im, so a wave covers whole 128-byte lines of every array it reads or writes.
// No atomics anywhere: identical calls give identical bits.
#include "halfspec.h"

namespace rpde {

constexpr float NS_TWO_PI = 6.28318530717958647692f;

// MODE 0: fan-out only (the first step of a call: W is read, not written)
//      1: update, then fan-out of the new W
//      2: update only (the last step of a call)
// grid (blocks, B).  D is [4][B] spectra: q^ = 2 pi i k2 psi, v^ = -2 pi i k1 psi, w_x^ = 2 pi i k1 W, w_y^ = 2 pi i k2 W,
// psi = W inv_lap.  g_h has gstride floats between samples (0: one forcing for the batch).  Padded columns
// (kx > N/2) are written as zeros in W and in D: the synthesis reads them.
template <int MODE>
__global__ __launch_bounds__(256) void k_ns_update_fanout(float* __restrict__ W, const float* __restrict__ F,
                                                          const float* __restrict__ gh, long gstride,
                                                          const float* __restrict__ cw, const float* __restrict__ cf,
                                                          const float* __restrict__ il, float* __restrict__ D, HalfSpec g) {
  const int b = blockIdx.y;
  const int c4n = g.kp / 4, per4 = g.M * c4n;
  const long per = (long)g.M * 2 * g.kp, dstride = (long)g.images * per;
  float* __restrict__ Wb = W + (long)b * per;
  const float* __restrict__ Fb = F + (long)b * per;
  const float* __restrict__ gb = gh + (long)b * gstride;
  float* __restrict__ Db = D + (long)b * per;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < per4; v += gridDim.x * 256) {
    const int ky = v / c4n, kx0 = (v - ky * c4n) * 4;
    const long ore = (long)ky * 2 * g.kp + kx0, oim = ore + g.kp, ot = (long)ky * g.kp + kx0;
    float wr[4], wi[4];
    ld4(Wb + ore, wr);
    ld4(Wb + oim, wi);
    if (MODE != 0) {
      float fr[4], fi[4], gr[4], gi[4], a[4], c[4];
      ld4(Fb + ore, fr); ld4(Fb + oim, fi);
      ld4(gb + ore, gr); ld4(gb + oim, gi);
      ld4(cw + ot, a);   ld4(cf + ot, c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool live = kx0 + j < g.K;
        wr[j] = live ? fmaf(a[j], wr[j], fmaf(-c[j], fr[j], gr[j])) : 0.f;
        wi[j] = live ? fmaf(a[j], wi[j], fmaf(-c[j], fi[j], gi[j])) : 0.f;
      }
      st4(Wb + ore, wr);
      st4(Wb + oim, wi);
    }
    if (MODE != 2) {
      float li[4], qr[4], qi[4], vr[4], vi[4], xr[4], xi[4], yr[4], yi[4];
      ld4(il + ot, li);
      const float k1 = NS_TWO_PI * (float)(ky < g.M / 2 ? ky : ky - g.M);
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
      st4(Db + ore, qr);               st4(Db + oim, qi);
      st4(Db + dstride + ore, vr);     st4(Db + dstride + oim, vi);
      st4(Db + 2 * dstride + ore, xr); st4(Db + 2 * dstride + oim, xi);
      st4(Db + 3 * dstride + ore, yr); st4(Db + 3 * dstride + oim, yi);
    }
  }
}

// P [4][B M N] = (q, v, w_x, w_y) -> out = q w_x + v w_y; n4 float4 groups per field (M, N even and the workspace pieces
// 256-byte aligned: always whole, aligned groups)
__global__ __launch_bounds__(256) void k_ns_advect(const float* __restrict__ P, float* __restrict__ out, long n4) {
  const float4* __restrict__ q = reinterpret_cast<const float4*>(P);
  const float4 *__restrict__ v = q + n4, *__restrict__ wx = q + 2 * n4, *__restrict__ wy = q + 3 * n4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 a = q[i], b = v[i], c = wx[i], d = wy[i];
    reinterpret_cast<float4*>(out)[i] =
        make_float4(fmaf(a.x, c.x, b.x * d.x), fmaf(a.y, c.y, b.y * d.y), fmaf(a.z, c.z, b.z * d.z), fmaf(a.w, c.w, b.w * d.w));
  }
}

// out = table . spec over `images` spectra, table [M][kp] (g_h = dt / (1 + a) f_h, once per solve); grid (blocks, images)
__global__ __launch_bounds__(256) void k_ns_scale(const float* __restrict__ spec, const float* __restrict__ table,
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

using namespace rpde;

extern "C" {

size_t rpde_ns2d_spec_elems(int B, int M, int N) { return hs_dims2_ok(B, M, N) ? hs_elems(hs_geom(B, M, N)) : 0; }

size_t rpde_ns2d_ws_bytes(int B, int M, int N) {
  if (!hs_dims2_ok(B, M, N)) return 0;
  const size_t spec = hs_elems(hs_geom(B, M, N)), phys = (size_t)B * M * N;
  // rpde_ns2d_steps: derivative spectra and their column stage (4B each), the four fields, their product, the
  // product's row spectra and spectrum; the transforms alone need one spectrum
  return 2 * arena_bytes(4 * spec) + arena_bytes(4 * phys) + arena_bytes(phys) + 2 * arena_bytes(spec);
}

int rpde_ns2d_scale(const float* spec, const float* table, float* out, int B, int M, int N, void* stream) {
  RPDE_CHECK_ARG(spec && table && out, "ns2d_scale: null pointer");
  HS_CHECK_DIMS_2D("ns2d_scale", B, M, N);
  RPDE_CHECK_ARG(al16(spec) && al16(table) && al16(out), "ns2d_scale: pointers must be 16-byte aligned");
  const HalfSpec g = hs_geom(B, M, N);
  hipLaunchKernelGGL(k_ns_scale, hs_grid((long)M * 2 * (g.kp / 4), B), dim3(256), 0, as_stream(stream), spec, table, out, g);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_ns2d_steps(float* W, const float* g_h, int g_batched, const float* c_w, const float* c_f, const float* inv_lap,
                    int B, int M, int N, int nsteps, void* ws, size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(W && g_h && c_w && c_f && inv_lap && ws, "ns2d_steps: null pointer");
  HS_CHECK_DIMS_2D("ns2d_steps", B, M, N);
  HS_CHECK_WS("ns2d_steps", ws);
  RPDE_CHECK_ARG(nsteps >= 0, "ns2d_steps: nsteps %d < 0", nsteps);
  RPDE_CHECK_ARG(al16(W) && al16(g_h) && al16(c_w) && al16(c_f) && al16(inv_lap),
                 "ns2d_steps: state, forcing and tables must be 16-byte aligned");
  const HalfSpec g = hs_geom(B, M, N), g4 = hs_geom(4 * B, M, N);      // the state; the four derivative fields
  const size_t spec = hs_elems(g), phys = (size_t)B * M * N;
  Arena ar(ws, ws_bytes);
  float* D = ar.take(4 * spec);
  float* T1 = ar.take(4 * spec);
  float* P = ar.take(4 * phys);
  float* Fp = ar.take(phys);
  float* S1 = ar.take(spec);
  float* F = ar.take(spec);
  if (!ar.ok()) { set_error("ns2d_steps: workspace too small"); return RPDE_ERR_WORKSPACE; }
  if (nsteps == 0) return RPDE_OK;
  hipStream_t st = as_stream(stream);
  const dim3 ug = hs_grid((long)M * (g.kp / 4), B);
  const long gstride = g_batched ? (long)hs_per(g) : 0;
  const long n4 = (long)phys / 4;
  hipLaunchKernelGGL(k_ns_update_fanout<0>, ug, dim3(256), 0, st, W, F, g_h, gstride, c_w, c_f, inv_lap, D, g);
  RPDE_LAUNCH_CHECK();
  for (int j = 0; j < nsteps; ++j) {
    RPDE_TRY(hs_irfft(g4, D, T1, P, st));
    hipLaunchKernelGGL(k_ns_advect, dim3(hs_blocks(n4, 2048)), dim3(256), 0, st, P, Fp, n4);
    RPDE_LAUNCH_CHECK();
    RPDE_TRY(hs_rfft(g, Fp, S1, F, st));
    if (j + 1 < nsteps) hipLaunchKernelGGL(k_ns_update_fanout<1>, ug, dim3(256), 0, st, W, F, g_h, gstride, c_w, c_f, inv_lap, D, g);
    else hipLaunchKernelGGL(k_ns_update_fanout<2>, ug, dim3(256), 0, st, W, F, g_h, gstride, c_w, c_f, inv_lap, D, g);
    RPDE_LAUNCH_CHECK();
  }
  return RPDE_OK;
}

}  // extern "C"
