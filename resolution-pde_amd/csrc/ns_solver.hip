// Navier-Stokes vorticity generator on the unit periodic square (reference: data_generation/ns_2d.py), plain or with an
// active scalar c that the flow advects and that drives the flow back through buoyancy along axis 2 (Boussinesq: the
// curl of the force is beta dc/dx1; data_generation/active_scalar_2d.py).  Pseudo-spectral, Crank-Nicolson on the
// diffusions, explicit advection, buoyancy and forcing, 2/3 de-aliasing.  gfx950, wave64.
//
// The state is the half spectrum W = rfft2(w), [B][M][re|im][kp] (halfspec.h); with the scalar, two per sample:
// S = [W_0 .. W_{B-1}, C_0 .. C_{B-1}].  One step is six launches on the caller's stream, no host synchronisation:
//   rowdft + synthesis   one batched inverse 2-D transform of the derivative spectra, 4B (q^, v^, w_1^, w_2^) or with
//                        the scalar 6B (.. c_1^, c_2^)
//   k_ns_advect          F_phys = q w_1 + v w_2, and with the scalar q c_1 + v c_2
//   analysis + rowdft    one forward 2-D transform of the B (2B) products
//   k_ns_update_fanout   W <- c_w W - c_f F + g_h, and from the NEW W the derivative spectra of the next step.  With the
//                        scalar: W <- c_w W - c_f (F_w - beta 2 pi i k1 C) + g_h with the OLD C, C <- d_w C - d_f F_c,
//                        and the fan-out from the new W and C
// One code path serves both (SCALAR of the kernels and of ns_steps): the scalar's parts are additions to the plain step.
// The coefficient tables are formed by the caller in float64 and rounded to fp32 once (rpde.ops.ns2d_tables, nsc2d_tables):
//   a = dt visc lap / 2,  c_w = (1 - a) / (1 + a),  c_f = dt dealias / (1 + a),  g_h = dt / (1 + a) f_h,  inv_lap = 1 / lap,
//   d_w and d_f as c_w and c_f with the scalar's diffusivity.
// The transforms are the full-spectrum real 2-D DFT of cf_dft.h (hs_rfft / hs_irfft, GEMM form); the rfft2 / irfft2
// entries and the random field that seeds the solver are in halfspec.hip.  Everything else here streams: a thread owns
// one 16-byte group of kx for both re and im, so a wave covers whole 128-byte lines of every array it reads or writes.
// No atomics anywhere: identical calls give identical bits.
#include "ns_kernels.h"

namespace rpde {

// k_ns_update_fanout, k_ns_advect and k_ns_scale are in ns_kernels.h: the vorticity residual runs them too

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
    const float k1 = NS_TWO_PI * (float)(ky < g.M / 2 ? ky : ky - g.M);
    float wr[4], wi[4], cr[4], ci[4], li[4], qr[4], qi[4], vr[4], vi[4];
    ld4(Wb + ore, wr); ld4(Wb + oim, wi);
    ld4(Cb + ore, cr); ld4(Cb + oim, ci);
    ld4(il + ot, li);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool live = kx0 + j < g.K;
      const float k2 = NS_TWO_PI * (float)(kx0 + j);
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


// Per sample, the derivative spectra of a step and its products.  The plain step's 4B derivative spectra are what the
// limits of a generator grid already count; the 6B of the scalar step are held to them as a batch of their own
// (hs_dims_ok's fan)
constexpr int ns_derivs(bool scalar) { return scalar ? 6 : 4; }
constexpr int ns_products(bool scalar) { return scalar ? 2 : 1; }
inline bool ns_dims_ok(bool scalar, int B, int M, int N) { return hs_dims2_ok(B, M, N, scalar ? ns_derivs(true) : 1); }

// The workspace of a step: the derivative spectra and their column stage, the fields, their products, the products' row
// spectra and spectra.  The transforms alone need one spectrum
struct NsWork {
  float *D, *T1, *P, *Fp, *S1, *F;
  NsWork(Arena& ar, size_t nd, size_t np, size_t spec, size_t phys)
      : D(ar.take(nd * spec)), T1(ar.take(nd * spec)), P(ar.take(nd * phys)), Fp(ar.take(np * phys)), S1(ar.take(np * spec)),
        F(ar.take(np * spec)) {}
};
// rpde_nsc2d_fields: three derivative spectra per sample and their column stage
struct NscFieldsWork {
  float *D, *T1;
  NscFieldsWork(Arena& ar, size_t spec) : D(ar.take(3 * spec)), T1(ar.take(3 * spec)) {}
};

static size_t ns_ws_bytes(bool scalar, int B, int M, int N) {
  if (!ns_dims_ok(scalar, B, M, N)) return 0;
  const size_t spec = hs_elems(hs_geom(B, M, N)), steps = ws_measure<NsWork>((size_t)ns_derivs(scalar), (size_t)ns_products(scalar), spec, (size_t)B * M * N);
  return scalar ? ws_max(steps, ws_measure<NscFieldsWork>(spec)) : steps;
}

// rpde_ns2d_steps and rpde_nsc2d_steps: the checks, the workspace, the first fan-out and nsteps times six launches
template <bool SCALAR>
static int ns_steps(float* S, const float* g_h, int g_batched, const NsTables<SCALAR>& t, int B, int M, int N, int nsteps,
                    void* ws, size_t ws_bytes, void* stream) {
  const char* what = SCALAR ? "nsc2d_steps" : "ns2d_steps";
  bool tables = t.cw && t.cf && t.il, aligned = al16(S) && al16(g_h) && al16(t.cw) && al16(t.cf) && al16(t.il);
  if constexpr (SCALAR) {
    tables = tables && t.dw && t.df;
    aligned = aligned && al16(t.dw) && al16(t.df);
  }
  RPDE_CHECK_ARG(S && g_h && tables && ws, "%s: null pointer", what);
  if (SCALAR) HS_CHECK_DIMS_2D_FAN(what, B, M, N, ns_derivs(true));
  else HS_CHECK_DIMS_2D("ns2d_steps", B, M, N);
  HS_CHECK_WS(what, ws);
  RPDE_CHECK_ARG(nsteps >= 0, "%s: nsteps %d < 0", what, nsteps);
  RPDE_CHECK_ARG(aligned, "%s: state, forcing and tables must be 16-byte aligned", what);
  // the state; the products; the derivative fields
  const HalfSpec g = hs_geom(B, M, N), gp = hs_geom(ns_products(SCALAR) * B, M, N), gd = hs_geom(ns_derivs(SCALAR) * B, M, N);
  const size_t phys = (size_t)B * M * N;
  RPDE_CARVE(what, NsWork, w, ws, ws_bytes, ns_derivs(SCALAR), ns_products(SCALAR), hs_elems(g), phys);
  if (nsteps == 0) return RPDE_OK;
  hipStream_t st = as_stream(stream);
  const dim3 ug = hs_grid((long)M * (g.kp / 4), B);
  const long gstride = g_batched ? (long)hs_per(g) : 0;
  const long n4 = (long)phys / 4;
  hipLaunchKernelGGL((k_ns_update_fanout<0, SCALAR>), ug, dim3(256), 0, st, S, w.F, g_h, gstride, t, w.D, g);
  RPDE_LAUNCH_CHECK();
  for (int j = 0; j < nsteps; ++j) {
    RPDE_TRY(hs_irfft(gd, w.D, w.T1, w.P, st));
    hipLaunchKernelGGL(k_ns_advect<SCALAR>, dim3(hs_blocks(n4, 2048)), dim3(256), 0, st, w.P, w.Fp, n4);
    RPDE_LAUNCH_CHECK();
    RPDE_TRY(hs_rfft(gp, w.Fp, w.S1, w.F, st));
    if (j + 1 < nsteps) hipLaunchKernelGGL((k_ns_update_fanout<1, SCALAR>), ug, dim3(256), 0, st, S, w.F, g_h, gstride, t, w.D, g);
    else hipLaunchKernelGGL((k_ns_update_fanout<2, SCALAR>), ug, dim3(256), 0, st, S, w.F, g_h, gstride, t, w.D, g);
    RPDE_LAUNCH_CHECK();
  }
  return RPDE_OK;
}

}  // namespace rpde

using namespace rpde;

extern "C" {

size_t rpde_ns2d_spec_elems(int B, int M, int N) { return hs_dims2_ok(B, M, N) ? hs_elems(hs_geom(B, M, N)) : 0; }

size_t rpde_ns2d_ws_bytes(int B, int M, int N) { return ns_ws_bytes(false, B, M, N); }

size_t rpde_nsc2d_ws_bytes(int B, int M, int N) { return ns_ws_bytes(true, B, M, N); }

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
  return ns_steps<false>(W, g_h, g_batched, NsTables<false>{c_w, c_f, inv_lap}, B, M, N, nsteps, ws, ws_bytes, stream);
}

int rpde_nsc2d_steps(float* S, const float* g_h, int g_batched, const float* c_w, const float* c_f, const float* d_w,
                     const float* d_f, const float* inv_lap, float beta, int B, int M, int N, int nsteps, void* ws,
                     size_t ws_bytes, void* stream) {
  return ns_steps<true>(S, g_h, g_batched, NsTables<true>{c_w, c_f, inv_lap, d_w, d_f, beta}, B, M, N, nsteps, ws, ws_bytes,
                        stream);
}

int rpde_nsc2d_fields(const float* S, const float* inv_lap, float* out, int B, int M, int N, void* ws, size_t ws_bytes,
                      void* stream) {
  RPDE_CHECK_ARG(S && inv_lap && out && ws, "nsc2d_fields: null pointer");
  HS_CHECK_DIMS_2D_FAN("nsc2d_fields", B, M, N, ns_derivs(true));
  HS_CHECK_WS("nsc2d_fields", ws);
  RPDE_CHECK_ARG(al16(S) && al16(inv_lap) && al16(out), "nsc2d_fields: state, table and output must be 16-byte aligned");
  const HalfSpec g = hs_geom(B, M, N), g3 = hs_geom(3 * B, M, N);
  RPDE_CARVE("nsc2d_fields", NscFieldsWork, w, ws, ws_bytes, hs_elems(g));
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_nsc_fields_fanout, hs_grid((long)M * (g.kp / 4), B), dim3(256), 0, st, S, inv_lap, w.D, g);
  RPDE_LAUNCH_CHECK();
  return hs_irfft(g3, w.D, w.T1, out, st);
}

}  // extern "C"
