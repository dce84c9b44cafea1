// Equation-residual loss of the 2-D vorticity equation w_t = -visc lap w - A(w) + f on the unit periodic square
// (utils/loss.py VorticityResidualLoss; no counterpart in the reference): does the one-step map x = w(t) -> p ~ w(t + D)
// satisfy the equation of the generator (ns_solver.hip)?  The conventions are the generator's: W = rfft2(w) unnormalised,
// k1 signed along ky, k2 = kx, lap = 4 pi^2 (k1^2 + k2^2), psi = W / lap (lap[0,0] -> 1), and its discrete advection
//   A(w) = dealias rfft2(q w_x + v w_y),  q = irfft2(2 pi i k2 psi), v = irfft2(-2 pi i k1 psi), w_x = irfft2(2 pi i k1 W), w_y = irfft2(2 pi i k2 W).
// The exponential trapezoidal rule (ETD2, as etd_residual.hip) with z = -D visc lap, all real here:
//   r^ = d^ - (E - 1) x^ - (m0 + m1) f^ + m0 A(x) + m1 A(p),   d = p - x formed in physical space (in float64),
//   E = e^z, m0 = D (phi1 - phi2), m1 = D phi2;  rel[b] = sqrt(E_r[b]) / (sqrt(E_x[b]) + REL_EPS),
//   E(z)[b] = sum c |z^|^2 / (M N),  c = 1 on the columns kx = 0 and N/2, else 2.
// The caller forms the tables in float64 and rounds them once (rpde.ops.ns2d_residual_tables): em1 = E - 1,
// m0 dealias, m1 dealias, 1 / lap, each [M][kp], and the forcing term (m0 + m1) f^ as one spectrum (or none).
// An affine decode (a_p p + b_p, a_x x + b_x) is folded into the first pass.
// Forward, on the caller's stream:
//   rel_roots, then k_nsr_rows and k_nsr_cols twice:     x^ and d^ as separable float64 analyses (rows, then columns).
//                         r^ is a remainder of 1e-3 |x| and less, and (E - 1) x^ carries an fp32 transform's absolute
//                         error in x^ straight into it; d is formed in float64 in LDS and never rounded (DESIGN.md
//                         10.12 has the figures with d^ on the layer's transform).  Both stay in float64 for the
//                         residual; an fp32 copy of x^ feeds the fan-out
//   k_nsr_pred            P^ = X^ + D^, rounded once, into the fan-out's state and into the saved spectra
//   k_ns_update_fanout    the generator's fan-out, once, on the state [X^ | P^]: eight derivative spectra per sample
//   hs_irfft, k_ns_advect, hs_rfft   8 B fields, the two products q w_x + v w_y, their 2 B spectra
//   k_nsr_residual        r^ (rounded once, padded columns zero), c |r^|^2 and c |x^|^2 per (sample, slot) in float64
//   rel_final             (rel_loss.h) adds the slots in fixed order.  The slots depend on the grid alone
// Backward, the exact adjoint of the discrete operator.  With g = irfft2(m1 dealias r^) and the four fields of p~
// rebuilt from the saved P^ (one fan-out; their spectra ride in the same inverse transform as g's):
//   G^ = r^ + conj(2 pi i k2 / lap) rfft2(g w_x) + conj(-2 pi i k1 / lap) rfft2(g w_y) + conj(2 pi i k1) rfft2(g q)
//           + conj(2 pi i k2) rfft2(g v),     grad_p = a_p coef_b irfft2(G^)
// No atomics anywhere: identical calls give identical bits, and a sample's value does not depend on its batch.
#include "nsr_kernels.h"

namespace rpde {

// k_nsr_rows, k_nsr_cols, nsr_spectrum and k_nsr_grad are in nsr_kernels.h: the active-scalar residual runs them too

// P^ = X^ + D^ in float64, rounded once, over n4 groups of four of B spectra (padded columns: zero plus zero), written
// twice: into the fan-out's state and into the spectra kept for backward
__global__ __launch_bounds__(256) void k_nsr_pred(const double* __restrict__ Xd, const double* __restrict__ Dd,
                                                  float* __restrict__ P, float* __restrict__ keep, long n4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    float pv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) pv[j] = (float)(Xd[4 * i + j] + Dd[4 * i + j]);
    st4(P + 4 * i, pv); st4(keep + 4 * i, pv);
  }
}

// grid (slots, B), g.images = B; a thread owns one 16-byte group of kx for both planes.  F [2][B] spectra: rfft2 of the
// advection products of x~ and of p~, before de-aliasing (m0 and m1 carry it); fs: the forcing term (m0 + m1) f^, one
// spectrum, or null.  r^ in float64, rounded once into spec_r, padded columns zero.
// part[(f B + b) S + slot], field 0 = c |r^|^2, field 1 = c |x^|^2
__global__ __launch_bounds__(256) void k_nsr_residual(const double* __restrict__ Dd, const double* __restrict__ Xd,
                                                      const float* __restrict__ F, const float* __restrict__ em1,
                                                      const float* __restrict__ m0, const float* __restrict__ m1,
                                                      const float* __restrict__ fs, float* __restrict__ spec_r,
                                                      double* __restrict__ part, HalfSpec g) {
  const int b = blockIdx.y;
  const int c4n = g.kp / 4, per4 = g.M * c4n;
  const long per = (long)g.M * 2 * g.kp, base = (long)b * per, half = (long)g.images * per;
  double er = 0.0, ex = 0.0;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < per4; v += gridDim.x * 256) {
    const int ky = v / c4n, kx0 = (v - ky * c4n) * 4;
    const long ore = (long)ky * 2 * g.kp + kx0, oim = ore + g.kp, ot = (long)ky * g.kp + kx0;
    float ar[4], ai[4], br[4], bi[4], e[4], c0[4], c1[4], fr[4] = {0.f, 0.f, 0.f, 0.f}, fi[4] = {0.f, 0.f, 0.f, 0.f};
    float rr[4], ri[4];
    ld4(F + base + ore, ar);        ld4(F + base + oim, ai);
    ld4(F + half + base + ore, br); ld4(F + half + base + oim, bi);
    ld4(em1 + ot, e); ld4(m0 + ot, c0); ld4(m1 + ot, c1);
    if (fs) { ld4(fs + ore, fr); ld4(fs + oim, fi); }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kx = kx0 + j;
      const bool live = kx < g.K;
      const double xr = Xd[base + ore + j], xi = Xd[base + oim + j];
      const double tr = Dd[base + ore + j] - (double)e[j] * xr - (double)fr[j] + (double)c0[j] * (double)ar[j] + (double)c1[j] * (double)br[j];
      const double ti = Dd[base + oim + j] - (double)e[j] * xi - (double)fi[j] + (double)c0[j] * (double)ai[j] + (double)c1[j] * (double)bi[j];
      const double c = (kx == 0 || kx == g.N / 2) ? 1.0 : 2.0;
      if (live) {
        er += c * (tr * tr + ti * ti);
        ex += c * (xr * xr + xi * xi);
      }
      rr[j] = live ? (float)tr : 0.f;
      ri[j] = live ? (float)ti : 0.f;
    }
    st4(spec_r + base + ore, rr); st4(spec_r + base + oim, ri);
  }
  rel_block_slots(er, ex, part, b, g.images, true);
}

// P [5][B M N] = (g, q, v, w_x, w_y) -> out [4][B M N] = (g w_x, g w_y, g q, g v); n4 float4 groups per field
__global__ __launch_bounds__(256) void k_nsr_products(const float* __restrict__ P, float* __restrict__ out, long n4) {
  const float4* __restrict__ gg = reinterpret_cast<const float4*>(P);
  const float4 *__restrict__ q = gg + n4, *__restrict__ v = gg + 2 * n4, *__restrict__ w1 = gg + 3 * n4, *__restrict__ w2 = gg + 4 * n4;
  float4* __restrict__ o = reinterpret_cast<float4*>(out);
  const auto mul = [](const float4& a, const float4& b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); };
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 a = gg[i];
    o[i] = mul(a, w1[i]);
    o[n4 + i] = mul(a, w2[i]);
    o[2 * n4 + i] = mul(a, q[i]);
    o[3 * n4 + i] = mul(a, v[i]);
  }
}

// grid (blocks, B), g.images = B.  H [4][B] spectra of (g w_x, g w_y, g q, g v):
// G^ = r^ - i c_q H_0 + i c_v H_1 - i c_x H_2 - i c_y H_3,  c_q = 2 pi k2 / lap, c_v = 2 pi k1 / lap, c_x = 2 pi k1,
// c_y = 2 pi k2 -- the conjugates of the fan-out's multipliers; padded columns zero
__global__ __launch_bounds__(256) void k_nsr_combine(const float* __restrict__ spec_r, const float* __restrict__ H,
                                                     const float* __restrict__ il, float* __restrict__ G, HalfSpec g) {
  const int b = blockIdx.y;
  const int c4n = g.kp / 4, per4 = g.M * c4n;
  const long per = (long)g.M * 2 * g.kp, base = (long)b * per, half = (long)g.images * per;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < per4; v += gridDim.x * 256) {
    const int ky = v / c4n, kx0 = (v - ky * c4n) * 4;
    const long ore = (long)ky * 2 * g.kp + kx0, oim = ore + g.kp, ot = (long)ky * g.kp + kx0;
    const float k1 = NS_TWO_PI * (float)(ky < g.M / 2 ? ky : ky - g.M);
    float rr[4], ri[4], li[4], h[4][2][4];
    ld4(spec_r + base + ore, rr); ld4(spec_r + base + oim, ri);
    ld4(il + ot, li);
#pragma unroll
    for (int f = 0; f < 4; ++f) { ld4(H + f * half + base + ore, h[f][0]); ld4(H + f * half + base + oim, h[f][1]); }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool live = kx0 + j < g.K;
      const float k2 = NS_TWO_PI * (float)(kx0 + j);
      const float cq = k2 * li[j], cv = k1 * li[j];
      // (a + i b)(-i c) = c b - i c a;  (a + i b)(i c) = -c b + i c a
      const float re = rr[j] + cq * h[0][1][j] - cv * h[1][1][j] + k1 * h[2][1][j] + k2 * h[3][1][j];
      const float im = ri[j] - cq * h[0][0][j] + cv * h[1][0][j] - k1 * h[2][0][j] - k2 * h[3][0][j];
      rr[j] = live ? re : 0.f;
      ri[j] = live ? im : 0.f;
    }
    st4(G + base + ore, rr); st4(G + base + oim, ri);
  }
}

// Per sample the forward fans out eight derivative spectra: held to the half-spectrum layer's limits as a batch of 8 B
constexpr int NSR_FAN = 8;
static bool nsr_dims_ok(int B, int M, int N) { return hs_dims2_ok(B, M, N, NSR_FAN); }

// forward: the analysis, x^ and d^ in float64, the state [X^ | P^], the eight derivative spectra and the transforms'
// row stage (it serves every transform of the call), the fields, the products and their spectra, the partial sums
struct NsrFwdWork {
  NsrSpecWork a;
  double *Xd, *Dd; float *S, *D, *T1, *P, *Fp, *F; double* part;
  NsrFwdWork(Arena& ar, int B, int M, int N, size_t spec, size_t phys)
      : a(ar, B, M, N), Xd(reinterpret_cast<double*>(ar.take(2 * spec))), Dd(reinterpret_cast<double*>(ar.take(2 * spec))), S(ar.take(2 * spec)),
        D(ar.take(NSR_FAN * spec)), T1(ar.take(NSR_FAN * spec)), P(ar.take(NSR_FAN * phys)), Fp(ar.take(2 * phys)),
        F(ar.take(2 * spec)), part(reinterpret_cast<double*>(ar.take((size_t)2 * 2 * B * REL_SLOTS))) {}
};
// backward: [g^ | the four derivative spectra of p~], the row stage, their fields, the four products and their spectra,
// G^ and its field
struct NsrBwdWork {
  float *D, *T1, *P, *Q, *H, *G, *z;
  NsrBwdWork(Arena& ar, size_t spec, size_t phys)
      : D(ar.take(5 * spec)), T1(ar.take(5 * spec)), P(ar.take(5 * phys)), Q(ar.take(4 * phys)), H(ar.take(4 * spec)),
        G(ar.take(spec)), z(ar.take(phys)) {}
};

}  // namespace rpde

using namespace rpde;

extern "C" {

size_t rpde_ns2d_residual_spec_elems(int B, int M, int N) { return nsr_dims_ok(B, M, N) ? 2 * hs_elems(hs_geom(B, M, N)) : 0; }

size_t rpde_ns2d_residual_ws_bytes(int B, int M, int N) {
  if (!nsr_dims_ok(B, M, N)) return 0;
  const size_t spec = hs_elems(hs_geom(B, M, N)), phys = (size_t)B * M * N;
  return ws_max(ws_measure<NsrFwdWork>(B, M, N, spec, phys), ws_measure<NsrBwdWork>(spec, phys));
}

int rpde_ns2d_residual_spectrum(const float* x, const float* affine, double* spec64, float* spec32, int B, int M, int N,
                                void* ws, size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(x && spec64 && spec32 && ws, "ns2d_residual_spectrum: null pointer");
  HS_CHECK_DIMS_2D_FAN("ns2d_residual_spectrum", B, M, N, NSR_FAN);
  HS_CHECK_WS("ns2d_residual_spectrum", ws);
  RPDE_CHECK_ARG(al16(spec64) && al16(spec32), "ns2d_residual_spectrum: the spectra must be 16-byte aligned");
  RPDE_CARVE("ns2d_residual_spectrum", NsrSpecWork, w, ws, ws_bytes, B, M, N);
  const RelAffine a{1.f, 0.f, affine ? affine[0] : 1.f, affine ? affine[1] : 0.f};
  RPDE_TRY(rel_roots(w.tw, N, M, as_stream(stream)));
  return nsr_spectrum(x, nullptr, w, spec64, spec32, hs_geom(B, M, N), a, as_stream(stream));
}

int rpde_ns2d_residual_fwd(const float* p, const float* x, const float* em1, const float* m0, const float* m1,
                           const float* inv_lap, const float* forcing_spec, const float* affine, float* rel, float* loss,
                           float* stats, float* spec, int B, int M, int N, int size_average, void* ws, size_t ws_bytes,
                           void* stream) {
  RPDE_CHECK_ARG(p && x && em1 && m0 && m1 && inv_lap && stats && spec && ws, "ns2d_residual_fwd: null pointer");
  HS_CHECK_DIMS_2D_FAN("ns2d_residual_fwd", B, M, N, NSR_FAN);
  HS_CHECK_WS("ns2d_residual_fwd", ws);
  RPDE_CHECK_ARG(al16(p) && al16(x) && al16(em1) && al16(m0) && al16(m1) && al16(inv_lap) && al16(forcing_spec) && al16(spec),
                 "ns2d_residual_fwd: fields, tables and spec must be 16-byte aligned");
  const HalfSpec g = hs_geom(B, M, N), g2 = hs_geom(2 * B, M, N), g8 = hs_geom(NSR_FAN * B, M, N);
  const size_t nspec = hs_elems(g), phys = (size_t)B * M * N;
  RPDE_CARVE("ns2d_residual_fwd", NsrFwdWork, w, ws, ws_bytes, B, M, N, nspec, phys);
  hipStream_t st = as_stream(stream);
  const RelAffine a = rel_affine(affine);
  float* spec_p = spec + nspec;                                   // spec = [r^ | P^]
  RPDE_TRY(rel_roots(w.a.tw, N, M, st));
  RPDE_TRY(nsr_spectrum(x, nullptr, w.a, w.Xd, w.S, g, a, st));
  RPDE_TRY(nsr_spectrum(x, p, w.a, w.Dd, nullptr, g, a, st));
  hipLaunchKernelGGL(k_nsr_pred, dim3(hs_blocks((long)nspec / 4, 2048)), dim3(256), 0, st, w.Xd, w.Dd, w.S + nspec, spec_p,
                     (long)nspec / 4);
  RPDE_LAUNCH_CHECK();
  const long groups = (long)M * (g.kp / 4);
  // the generator's fan-out of a state it only reads (MODE 0): its products, forcing and step tables are not touched
  hipLaunchKernelGGL((k_ns_update_fanout<0, false>), hs_grid(groups, 2 * B), dim3(256), 0, st, w.S, w.F, w.F, 0L,
                     NsTables<false>{nullptr, nullptr, inv_lap}, w.D, g2);
  RPDE_LAUNCH_CHECK();
  RPDE_TRY(hs_irfft(g8, w.D, w.T1, w.P, st));
  const long n4 = 2 * (long)phys / 4;
  hipLaunchKernelGGL(k_ns_advect<false>, dim3(hs_blocks(n4, 2048)), dim3(256), 0, st, w.P, w.Fp, n4);
  RPDE_LAUNCH_CHECK();
  RPDE_TRY(hs_rfft(g2, w.Fp, w.T1, w.F, st));
  const int slots = rel_slots((long)M * g.kp);
  hipLaunchKernelGGL(k_nsr_residual, dim3(slots, B), dim3(256), 0, st, w.Dd, w.Xd, w.F, em1, m0, m1, forcing_spec, spec, w.part, g);
  RPDE_LAUNCH_CHECK();
  return rel_final(w.part, rel, loss, stats, B, slots, 1.0 / ((double)M * (double)N), size_average, st);
}

int rpde_ns2d_residual_bwd(const float* spec, const float* m1, const float* inv_lap, const float* affine, const float* stats,
                           const float* grad_loss, const float* grad_rel, float* grad_p, int B, int M, int N,
                           int size_average, void* ws, size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(spec && m1 && inv_lap && stats && grad_p && ws && (grad_loss || grad_rel), "ns2d_residual_bwd: null pointer");
  HS_CHECK_DIMS_2D_FAN("ns2d_residual_bwd", B, M, N, NSR_FAN);
  HS_CHECK_WS("ns2d_residual_bwd", ws);
  RPDE_CHECK_ARG(al16(spec) && al16(m1) && al16(inv_lap) && al16(grad_p),
                 "ns2d_residual_bwd: tables, spec and grad_p must be 16-byte aligned");
  const HalfSpec g = hs_geom(B, M, N), g4 = hs_geom(4 * B, M, N), g5 = hs_geom(5 * B, M, N);
  const size_t nspec = hs_elems(g), phys = (size_t)B * M * N;
  RPDE_CARVE("ns2d_residual_bwd", NsrBwdWork, w, ws, ws_bytes, nspec, phys);
  hipStream_t st = as_stream(stream);
  const long groups = (long)M * (g.kp / 4);
  // D = [g^ = m1 dealias r^ | q^, v^, w_x^, w_y^ of the saved P^]
  hipLaunchKernelGGL(k_ns_scale, hs_grid(2 * groups, B), dim3(256), 0, st, spec, m1, w.D, g);
  RPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_ns_update_fanout<0, false>), hs_grid(groups, B), dim3(256), 0, st, const_cast<float*>(spec + nspec), w.H,
                     w.H, 0L, NsTables<false>{nullptr, nullptr, inv_lap}, w.D + nspec, g);
  RPDE_LAUNCH_CHECK();
  RPDE_TRY(hs_irfft(g5, w.D, w.T1, w.P, st));
  hipLaunchKernelGGL(k_nsr_products, dim3(hs_blocks((long)phys / 4, 2048)), dim3(256), 0, st, w.P, w.Q, (long)phys / 4);
  RPDE_LAUNCH_CHECK();
  RPDE_TRY(hs_rfft(g4, w.Q, w.T1, w.H, st));
  hipLaunchKernelGGL(k_nsr_combine, hs_grid(groups, B), dim3(256), 0, st, spec, w.H, inv_lap, w.G, g);
  RPDE_LAUNCH_CHECK();
  RPDE_TRY(hs_irfft(g, w.G, w.T1, w.z, st));
  const int n4 = M * N / 4;
  hipLaunchKernelGGL(k_nsr_grad, hs_grid(n4, B), dim3(256), 0, st, w.z, stats, grad_loss, grad_rel, grad_p, B, n4, size_average,
                     rel_affine(affine).ap);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

}  // extern "C"
