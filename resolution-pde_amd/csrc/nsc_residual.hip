// Equation-residual loss of the active-scalar Navier-Stokes system on the unit periodic square (utils/loss.py
// ActiveScalarResidualLoss; no counterpart in the reference): does the one-step map x = (c, q, v)(t) -> p ~ (c, q, v)(t + D)
// satisfy the equation of the generator (ns_solver.hip, SCALAR)?  The data are not the evolved variable: the equation
// evolves (w, c) with w = curl u, so the loss also says what a predicted velocity owes to incompressibility and to its
// mean.  Conventions as ns_residual.hip; with the channel spectra x^ and d^ (d = p~ - x~ formed in physical space):
//   X_c = x^_c,  X_w = 2 pi i k1 x^_v - 2 pi i k2 x^_q   (likewise D_c, D_w;  P = X + D)
//   N_w(W, C) = dealias (rfft2(q w_1 + v w_2) - beta 2 pi i k1 C),  N_c(W, C) = dealias rfft2(q c_1 + v c_2): the
//               generator's F_w and F_c, q and v from psi = W / lap (only the solenoidal part of a velocity advects)
//   r^_w = D_w - (E_nu - 1) X_w + m0_nu N_w(X) + m1_nu N_w(P) - (m0_nu + m1_nu) f^          z = -D visc lap
//   r^_c = D_c - (E_kappa - 1) X_c + m0_kappa N_c(X) + m1_kappa N_c(P)                      z = -D kappa lap
//   delta^ = 2 pi i k1 P_q + 2 pi i k2 P_v,   mu = (d^_q[0,0], d^_v[0,0])     divergence and change of the mean velocity
//   E_ru = sum_{k != 0} c (|r^_w|^2 + |delta^|^2) / lap / (M N) + |mu|^2 / (M N),   E_rc = sum c |r^_c|^2 / (M N)
//   rel[b] = sqrt(lambda E_rc + E_ru) / (sqrt(lambda E(x^_c) + E(x^_q) + E(x^_v)) + REL_EPS)
// -- the residual of the vorticity measured as a velocity (energy |r^|^2 / lap), in the norm of the data's channels.
// The tables are ns_residual.hip's, once per diffusivity (rpde.ops.nsc2d_residual_tables); m0 and m1 carry the mask.
// Forward, on the caller's stream:
//   rel_roots, then nsr_spectrum twice    x^ of the 3 B images of x~ and d^ of the 3 B images of d, in float64
//                                         (nsr_kernels.h; DESIGN.md 10.12 has why the fp32 transform is not enough)
//   k_nscr_state          X_w, X_c, P_w, P_c from the float64 channel spectra (the curl is a multiplier), rounded once,
//                         into the fan-out's state [X_w | P_w | X_c | P_c] and into the saved spectra
//   k_ns_update_fanout<0, true>   the generator's fan-out over 2 B states: six derivative spectra per state
//   hs_irfft, k_ns_advect<true>, hs_rfft  12 B fields, the products q w_1 + v w_2 and q c_1 + v c_2, their 4 B spectra
//   k_nscr_residual       r^_w, r^_c, delta^, mu in float64 (the buoyancy terms from the float64 X_c, P_c), the partial
//                         sums per (sample, slot), and what the backward needs, rounded once, padded columns zero
//   rel_final             (rel_loss.h) adds the slots in fixed order
// Backward, the exact adjoint of the discrete operator.  With rho_w = r^_w / lap (0 at the mean mode), rho_c = lambda r^_c,
// rho_d = delta^ / lap, g_w = irfft2(m1_nu rho_w), g_c = irfft2(m1_kappa rho_c) and the six fields of p~ rebuilt from the
// saved P_w, P_c (one fan-out; their spectra ride in the same inverse transform as g's, 8 B images):
//   G_w = rho_w + conj(2 pi i k2 / lap) rfft2(g_w w_1 + g_c c_1) + conj(-2 pi i k1 / lap) rfft2(g_w w_2 + g_c c_2)
//               + conj(2 pi i k1) rfft2(g_w q) + conj(2 pi i k2) rfft2(g_w v)
//   G_c = rho_c + conj(2 pi i k1) rfft2(g_c q) + conj(2 pi i k2) rfft2(g_c v) + conj(-beta 2 pi i k1) m1_nu rho_w
//   grad p_c = irfft2(G_c),  grad p_q = irfft2(conj(-2 pi i k2) G_w + conj(2 pi i k1) rho_d + [k = 0] mu_q),
//   grad p_v = irfft2(conj(2 pi i k1) G_w + conj(2 pi i k2) rho_d + [k = 0] mu_v),    all times a_p coef_b
// (one forward transform of 6 B products, one inverse of 3 B).
// No atomics anywhere: identical calls give identical bits, and a sample's value does not depend on its batch.
#include "nsr_kernels.h"

namespace rpde {

constexpr double NSCR_TWO_PI = 6.283185307179586476925286766559;

// grid (blocks, B), g.images = B.  Xd, Dd: float64 spectra of the 3 B images (c, q, v per sample) of x~ and of d.
// S [4][B] fp32 spectra = [X_w | P_w | X_c | P_c]: two states (W's, then C's) of 2 B samples for the generator's fan-out;
// keep [2][B] = [P_w | P_c] (may be null).  Padded columns zero
__global__ __launch_bounds__(256) void k_nscr_state(const double* __restrict__ Xd, const double* __restrict__ Dd,
                                                    float* __restrict__ S, float* __restrict__ keep, HalfSpec g) {
  const int b = blockIdx.y;
  const int c4n = g.kp / 4, per4 = g.M * c4n;
  const long per = (long)g.M * 2 * g.kp, half = (long)g.images * per, base = (long)b * per;
  const double* __restrict__ Xb = Xd + 3 * base;
  const double* __restrict__ Db = Dd + 3 * base;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < per4; v += gridDim.x * 256) {
    const int ky = v / c4n, kx0 = (v - ky * c4n) * 4;
    const long ore = (long)ky * 2 * g.kp + kx0, oim = ore + g.kp;
    const double k1 = NSCR_TWO_PI * (double)(ky < g.M / 2 ? ky : ky - g.M);
    float xwr[4], xwi[4], pwr[4], pwi[4], xcr[4], xci[4], pcr[4], pci[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool live = kx0 + j < g.K;
      const double k2 = NSCR_TWO_PI * (double)(kx0 + j);
      const double cr = Xb[ore + j], ci = Xb[oim + j], qr = Xb[per + ore + j], qi = Xb[per + oim + j];
      const double vr = Xb[2 * per + ore + j], vi = Xb[2 * per + oim + j];
      const double dcr = Db[ore + j], dci = Db[oim + j], dqr = Db[per + ore + j], dqi = Db[per + oim + j];
      const double dvr = Db[2 * per + ore + j], dvi = Db[2 * per + oim + j];
      // i (k1 V - k2 Q) = -(k1 V_im - k2 Q_im) + i (k1 V_re - k2 Q_re)
      const double wr = -(k1 * vi - k2 * qi), wi = k1 * vr - k2 * qr;
      const double ewr = -(k1 * dvi - k2 * dqi), ewi = k1 * dvr - k2 * dqr;
      xwr[j] = live ? (float)wr : 0.f;          xwi[j] = live ? (float)wi : 0.f;
      pwr[j] = live ? (float)(wr + ewr) : 0.f;  pwi[j] = live ? (float)(wi + ewi) : 0.f;
      xcr[j] = live ? (float)cr : 0.f;          xci[j] = live ? (float)ci : 0.f;
      pcr[j] = live ? (float)(cr + dcr) : 0.f;  pci[j] = live ? (float)(ci + dci) : 0.f;
    }
    st4(S + base + ore, xwr);            st4(S + base + oim, xwi);
    st4(S + half + base + ore, pwr);     st4(S + half + base + oim, pwi);
    st4(S + 2 * half + base + ore, xcr); st4(S + 2 * half + base + oim, xci);
    st4(S + 3 * half + base + ore, pcr); st4(S + 3 * half + base + oim, pci);
    if (keep) {
      st4(keep + base + ore, pwr);        st4(keep + base + oim, pwi);
      st4(keep + half + base + ore, pcr); st4(keep + half + base + oim, pci);
    }
  }
}

// the six tables of the residual, [M][kp] each: E - 1, m0 dealias, m1 dealias per diffusivity
struct NscrTables { const float *en, *m0n, *m1n, *ek, *m0k, *m1k; };

// grid (slots, B), g.images = B; a thread owns one 16-byte group of kx for all planes.  F [4][B] spectra: rfft2 of the
// products (q w_1 + v w_2)(X), (..)(P), (q c_1 + v c_2)(X), (..)(P), before de-aliasing (m0 and m1 carry it); fs: the
// forcing term (m0_nu + m1_nu) f^, one spectrum, or null.  Everything in float64 from the float64 channel spectra.
// spec [3][B] = [rho_w = r^_w / lap | rho_c = lambda r^_c | rho_d = delta^ / lap], each rounded once, padded columns
// zero; rho_w and rho_d are zero at the mean mode, and the mean mode of rho_d holds mu = (mu_q, mu_v) as (re, im).
// part[(f B + b) S + slot], field 0 = lambda E_rc + E_ru, field 1 = lambda E_xc + E_xu (before the 1 / (M N))
__global__ __launch_bounds__(256) void k_nscr_residual(const double* __restrict__ Xd, const double* __restrict__ Dd,
                                                       const float* __restrict__ F, NscrTables t, const float* __restrict__ fs,
                                                       float beta, float lambda, float* __restrict__ spec,
                                                       double* __restrict__ part, HalfSpec g) {
  const int b = blockIdx.y;
  const int c4n = g.kp / 4, per4 = g.M * c4n;
  const long per = (long)g.M * 2 * g.kp, half = (long)g.images * per, base = (long)b * per;
  const double* __restrict__ Xb = Xd + 3 * base;
  const double* __restrict__ Db = Dd + 3 * base;
  const double lam = (double)lambda, bt = (double)beta;
  double er = 0.0, ex = 0.0;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < per4; v += gridDim.x * 256) {
    const int ky = v / c4n, kx0 = (v - ky * c4n) * 4;
    const long ore = (long)ky * 2 * g.kp + kx0, oim = ore + g.kp, ot = (long)ky * g.kp + kx0;
    const double k1 = NSCR_TWO_PI * (double)(ky < g.M / 2 ? ky : ky - g.M);
    float a[4][2][4], en[4], m0n[4], m1n[4], ek[4], m0k[4], m1k[4], fr[4] = {0.f, 0.f, 0.f, 0.f}, fi[4] = {0.f, 0.f, 0.f, 0.f};
    float rwr[4], rwi[4], rcr[4], rci[4], rdr[4], rdi[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) { ld4(F + f * half + base + ore, a[f][0]); ld4(F + f * half + base + oim, a[f][1]); }
    ld4(t.en + ot, en); ld4(t.m0n + ot, m0n); ld4(t.m1n + ot, m1n);
    ld4(t.ek + ot, ek); ld4(t.m0k + ot, m0k); ld4(t.m1k + ot, m1k);
    if (fs) { ld4(fs + ore, fr); ld4(fs + oim, fi); }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kx = kx0 + j;
      const bool live = kx < g.K, mean = ky == 0 && kx == 0;
      const double k2 = NSCR_TWO_PI * (double)kx;
      const double il = mean ? 0.0 : 1.0 / (k1 * k1 + k2 * k2);
      const double cr = Xb[ore + j], ci = Xb[oim + j], qr = Xb[per + ore + j], qi = Xb[per + oim + j];
      const double vr = Xb[2 * per + ore + j], vi = Xb[2 * per + oim + j];
      const double dcr = Db[ore + j], dci = Db[oim + j], dqr = Db[per + ore + j], dqi = Db[per + oim + j];
      const double dvr = Db[2 * per + ore + j], dvi = Db[2 * per + oim + j];
      const double xwr = -(k1 * vi - k2 * qi), xwi = k1 * vr - k2 * qr;
      const double dwr = -(k1 * dvi - k2 * dqi), dwi = k1 * dvr - k2 * dqr;
      const double pcr = cr + dcr, pci = ci + dci;
      // -beta 2 pi i k1 C = beta k1 C_im - i beta k1 C_re
      const double nxr = (double)a[0][0][j] + bt * k1 * ci, nxi = (double)a[0][1][j] - bt * k1 * cr;
      const double npr = (double)a[1][0][j] + bt * k1 * pci, npi = (double)a[1][1][j] - bt * k1 * pcr;
      const double wr = dwr - (double)en[j] * xwr - (double)fr[j] + (double)m0n[j] * nxr + (double)m1n[j] * npr;
      const double wi = dwi - (double)en[j] * xwi - (double)fi[j] + (double)m0n[j] * nxi + (double)m1n[j] * npi;
      const double sr = dcr - (double)ek[j] * cr + (double)m0k[j] * (double)a[2][0][j] + (double)m1k[j] * (double)a[3][0][j];
      const double si = dci - (double)ek[j] * ci + (double)m0k[j] * (double)a[2][1][j] + (double)m1k[j] * (double)a[3][1][j];
      // i (k1 P_q + k2 P_v)
      const double pqr = qr + dqr, pqi = qi + dqi, pvr = vr + dvr, pvi = vi + dvi;
      const double er_ = -(k1 * pqi + k2 * pvi), ei_ = k1 * pqr + k2 * pvr;
      const double c = (kx == 0 || kx == g.N / 2) ? 1.0 : 2.0;
      if (live) {
        er += c * ((wr * wr + wi * wi + er_ * er_ + ei_ * ei_) * il + lam * (sr * sr + si * si));
        if (mean) er += dqr * dqr + dvr * dvr;
        ex += c * (qr * qr + qi * qi + vr * vr + vi * vi + lam * (cr * cr + ci * ci));
      }
      rwr[j] = live ? (float)(wr * il) : 0.f;  rwi[j] = live ? (float)(wi * il) : 0.f;
      rcr[j] = live ? (float)(lam * sr) : 0.f; rci[j] = live ? (float)(lam * si) : 0.f;
      rdr[j] = live ? (float)(er_ * il) : 0.f; rdi[j] = live ? (float)(ei_ * il) : 0.f;
      if (mean) { rdr[j] = (float)dqr; rdi[j] = (float)dvr; }
    }
    st4(spec + base + ore, rwr);            st4(spec + base + oim, rwi);
    st4(spec + half + base + ore, rcr);     st4(spec + half + base + oim, rci);
    st4(spec + 2 * half + base + ore, rdr); st4(spec + 2 * half + base + oim, rdi);
  }
  rel_block_slots(er, ex, part, b, g.images, true);
}

// P [8][B M N] = (g_w, g_c, q, v, w_1, w_2, c_1, c_2) -> out [6][B M N] = (g_w w_1 + g_c c_1, g_w w_2 + g_c c_2, g_w q,
// g_w v, g_c q, g_c v); n4 float4 groups per field
__global__ __launch_bounds__(256) void k_nscr_products(const float* __restrict__ P, float* __restrict__ out, long n4) {
  const float4* __restrict__ p = reinterpret_cast<const float4*>(P);
  float4* __restrict__ o = reinterpret_cast<float4*>(out);
  const auto mul = [](const float4& a, const float4& b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); };
  const auto dot = [](const float4& a, const float4& b, const float4& c, const float4& d) {
    return make_float4(fmaf(a.x, b.x, c.x * d.x), fmaf(a.y, b.y, c.y * d.y), fmaf(a.z, b.z, c.z * d.z), fmaf(a.w, b.w, c.w * d.w));
  };
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 gw = p[i], gc = p[n4 + i], q = p[2 * n4 + i], v = p[3 * n4 + i];
    o[i] = dot(gw, p[4 * n4 + i], gc, p[6 * n4 + i]);
    o[n4 + i] = dot(gw, p[5 * n4 + i], gc, p[7 * n4 + i]);
    o[2 * n4 + i] = mul(gw, q);
    o[3 * n4 + i] = mul(gw, v);
    o[4 * n4 + i] = mul(gc, q);
    o[5 * n4 + i] = mul(gc, v);
  }
}

// grid (blocks, B), g.images = B.  spec [3][B] as k_nscr_residual left it, H [6][B] spectra of k_nscr_products' fields:
//   G_w = rho_w - i c_q H_0 + i c_v H_1 - i c_x H_2 - i c_y H_3,   G_c = rho_c - i c_x H_4 - i c_y H_5 + i beta c_x m1_nu rho_w,
//   c_q = 2 pi k2 / lap, c_v = 2 pi k1 / lap, c_x = 2 pi k1, c_y = 2 pi k2 -- the conjugates of the fan-out's multipliers;
// G [B][3] spectra, sample-major, whose inverse transform is the gradient [B, 3, M, N] = (c, q, v) as it stands:
//   G_c,   i c_y G_w - i c_x rho_d + [k = 0] mu_q,   -i c_x G_w - i c_y rho_d + [k = 0] mu_v;   padded columns zero
__global__ __launch_bounds__(256) void k_nscr_combine(const float* __restrict__ spec, const float* __restrict__ H,
                                                      const float* __restrict__ m1n, const float* __restrict__ il, float beta,
                                                      float* __restrict__ G, HalfSpec g) {
  const int b = blockIdx.y;
  const int c4n = g.kp / 4, per4 = g.M * c4n;
  const long per = (long)g.M * 2 * g.kp, base = (long)b * per, half = (long)g.images * per;
  float* __restrict__ Gb = G + 3 * base;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < per4; v += gridDim.x * 256) {
    const int ky = v / c4n, kx0 = (v - ky * c4n) * 4;
    const long ore = (long)ky * 2 * g.kp + kx0, oim = ore + g.kp, ot = (long)ky * g.kp + kx0;
    const float k1 = NS_TWO_PI * (float)(ky < g.M / 2 ? ky : ky - g.M);
    float wr[4], wi[4], cr[4], ci[4], dr[4], di[4], li[4], m1[4], h[6][2][4];
    float qr[4], qi[4], vr[4], vi[4];
    ld4(spec + base + ore, wr);            ld4(spec + base + oim, wi);
    ld4(spec + half + base + ore, cr);     ld4(spec + half + base + oim, ci);
    ld4(spec + 2 * half + base + ore, dr); ld4(spec + 2 * half + base + oim, di);
    ld4(il + ot, li); ld4(m1n + ot, m1);
#pragma unroll
    for (int f = 0; f < 6; ++f) { ld4(H + f * half + base + ore, h[f][0]); ld4(H + f * half + base + oim, h[f][1]); }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool live = kx0 + j < g.K, mean = ky == 0 && kx0 + j == 0;
      const float k2 = NS_TWO_PI * (float)(kx0 + j);
      const float cq = k2 * li[j], cv = k1 * li[j], bk = beta * k1;
      // (a + i b)(-i c) = c b - i c a;  (a + i b)(i c) = -c b + i c a
      const float gwr = wr[j] + cq * h[0][1][j] - cv * h[1][1][j] + k1 * h[2][1][j] + k2 * h[3][1][j];
      const float gwi = wi[j] - cq * h[0][0][j] + cv * h[1][0][j] - k1 * h[2][0][j] - k2 * h[3][0][j];
      const float sr = m1[j] * wr[j], si = m1[j] * wi[j];        // m1_nu rho_w: the spectrum of g_w
      const float gcr = cr[j] + k1 * h[4][1][j] + k2 * h[5][1][j] - bk * si;
      const float gci = ci[j] - k1 * h[4][0][j] - k2 * h[5][0][j] + bk * sr;
      // the mean mode of rho_d holds mu; there k1 = k2 = 0 and every other term vanishes
      const float er = mean ? 0.f : dr[j], ei = mean ? 0.f : di[j];
      const float oqr = -k2 * gwi + k1 * ei + (mean ? dr[j] : 0.f), oqi = k2 * gwr - k1 * er;
      const float ovr = k1 * gwi + k2 * ei + (mean ? di[j] : 0.f), ovi = -k1 * gwr - k2 * er;
      cr[j] = live ? gcr : 0.f;  ci[j] = live ? gci : 0.f;
      qr[j] = live ? oqr : 0.f;  qi[j] = live ? oqi : 0.f;
      vr[j] = live ? ovr : 0.f;  vi[j] = live ? ovi : 0.f;
    }
    st4(Gb + ore, cr);           st4(Gb + oim, ci);
    st4(Gb + per + ore, qr);     st4(Gb + per + oim, qi);
    st4(Gb + 2 * per + ore, vr); st4(Gb + 2 * per + oim, vi);
  }
}

// Per sample the forward fans out twelve derivative spectra (six per state, two states): held to the half-spectrum
// layer's limits as a batch of 12 B
constexpr int NSCR_FAN = 12;
static bool nscr_dims_ok(int B, int M, int N) { return hs_dims2_ok(B, M, N, NSCR_FAN); }

// the state alone: the analysis of 3 B images and the float64 channel spectra of x~ and of d
struct NscrStateWork {
  NsrSpecWork a;
  double *Xd, *Dd;
  NscrStateWork(Arena& ar, int B, int M, int N, size_t spec)
      : a(ar, 3 * B, M, N), Xd(reinterpret_cast<double*>(ar.take(6 * spec))), Dd(reinterpret_cast<double*>(ar.take(6 * spec))) {}
};
// forward: the state's pieces, the state [X_w | P_w | X_c | P_c], the twelve derivative spectra and the transforms' row
// stage (it serves every transform of the call), the fields, the four products and their spectra, the partial sums
struct NscrFwdWork {
  NscrStateWork s;
  float *S, *D, *T1, *P, *Fp, *F; double* part;
  NscrFwdWork(Arena& ar, int B, int M, int N, size_t spec, size_t phys)
      : s(ar, B, M, N, spec), S(ar.take(4 * spec)), D(ar.take(NSCR_FAN * spec)), T1(ar.take(NSCR_FAN * spec)),
        P(ar.take(NSCR_FAN * phys)), Fp(ar.take(4 * phys)), F(ar.take(4 * spec)),
        part(reinterpret_cast<double*>(ar.take((size_t)2 * 2 * B * REL_SLOTS))) {}
};
// backward: [g_w^ | g_c^ | the six derivative spectra of p~], the row stage, their fields, the six products and their
// spectra, the three gradient spectra and their fields
struct NscrBwdWork {
  float *D, *T1, *P, *Q, *H, *G, *z;
  NscrBwdWork(Arena& ar, size_t spec, size_t phys)
      : D(ar.take(8 * spec)), T1(ar.take(8 * spec)), P(ar.take(8 * phys)), Q(ar.take(6 * phys)), H(ar.take(6 * spec)),
        G(ar.take(3 * spec)), z(ar.take(3 * phys)) {}
};

// The decode maps are the last thing an entry checks, behind the verdict on its workspace: reading them is the first
// use of the caller's four floats
static bool nscr_affine_ok(const RelAffine& a) {
  const auto ok = [](float v) { return v == v && fabsf(v) < INFINITY; };
  return ok(a.ap) && ok(a.bp) && ok(a.ax) && ok(a.bx);
}
#define NSCR_CHECK_AFFINE(what, a) RPDE_CHECK_ARG(nscr_affine_ok(a), what ": the affine map (a_p, b_p, a_x, b_x) must be finite")

// rel_roots, the two analyses and k_nscr_state
static int nscr_state(const float* p, const float* x, const NscrStateWork& w, float* S, float* keep, int B, int M, int N,
                      RelAffine a, hipStream_t st) {
  const HalfSpec g = hs_geom(B, M, N), g3 = hs_geom(3 * B, M, N);
  RPDE_TRY(rel_roots(w.a.tw, N, M, st));
  RPDE_TRY(nsr_spectrum(x, nullptr, w.a, w.Xd, nullptr, g3, a, st));
  RPDE_TRY(nsr_spectrum(x, p, w.a, w.Dd, nullptr, g3, a, st));
  hipLaunchKernelGGL(k_nscr_state, hs_grid((long)M * (g.kp / 4), B), dim3(256), 0, st, w.Xd, w.Dd, S, keep, g);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

}  // namespace rpde

using namespace rpde;

extern "C" {

size_t rpde_nsc2d_residual_spec_elems(int B, int M, int N) { return nscr_dims_ok(B, M, N) ? 5 * hs_elems(hs_geom(B, M, N)) : 0; }

size_t rpde_nsc2d_residual_arena_bytes(int B, int M, int N) {
  if (!nscr_dims_ok(B, M, N)) return 0;
  const size_t spec = hs_elems(hs_geom(B, M, N)), phys = (size_t)B * M * N;
  return ws_max(ws_max(ws_measure<NscrFwdWork>(B, M, N, spec, phys), ws_measure<NscrBwdWork>(spec, phys)),
                ws_measure<NscrStateWork>(B, M, N, spec));
}

int rpde_nsc2d_residual_state(const float* p, const float* x, const float* affine, float* state, int B, int M, int N,
                              void* ws, size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(p && x && state && ws, "nsc2d_residual_state: null pointer");
  HS_CHECK_DIMS_2D_FAN("nsc2d_residual_state", B, M, N, NSCR_FAN);
  HS_CHECK_WS("nsc2d_residual_state", ws);
  RPDE_CHECK_ARG(al16(p) && al16(x) && al16(state), "nsc2d_residual_state: fields and state must be 16-byte aligned");
  RPDE_CARVE("nsc2d_residual_state", NscrStateWork, w, ws, ws_bytes, B, M, N, hs_elems(hs_geom(B, M, N)));
  const RelAffine a = rel_affine(affine);
  NSCR_CHECK_AFFINE("nsc2d_residual_state", a);
  return nscr_state(p, x, w, state, nullptr, B, M, N, a, as_stream(stream));
}

int rpde_nsc2d_residual_fwd(const float* p, const float* x, const float* em1_nu, const float* m0_nu, const float* em1_kappa,
                            const float* m0_kappa, const float* forcing_spec, float scalar_weight, const float* m1_nu,
                            const float* m1_kappa, const float* inv_lap, float beta, const float* affine, float* rel,
                            float* loss, float* stats, float* spec, int B, int M, int N, int size_average, void* ws,
                            size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(p && x && em1_nu && m0_nu && em1_kappa && m0_kappa && m1_nu && m1_kappa && inv_lap && stats && spec && ws,
                 "nsc2d_residual_fwd: null pointer");
  HS_CHECK_DIMS_2D_FAN("nsc2d_residual_fwd", B, M, N, NSCR_FAN);
  HS_CHECK_WS("nsc2d_residual_fwd", ws);
  RPDE_CHECK_ARG(scalar_weight >= 0.f && scalar_weight < INFINITY && beta == beta && fabsf(beta) < INFINITY,
                 "nsc2d_residual_fwd: scalar_weight %g must be finite and >= 0, beta %g finite", (double)scalar_weight, (double)beta);
  RPDE_CHECK_ARG(al16(p) && al16(x) && al16(em1_nu) && al16(m0_nu) && al16(em1_kappa) && al16(m0_kappa) && al16(m1_nu) &&
                     al16(m1_kappa) && al16(inv_lap) && al16(forcing_spec) && al16(spec),
                 "nsc2d_residual_fwd: fields, tables and spec must be 16-byte aligned");
  const HalfSpec g = hs_geom(B, M, N), g2 = hs_geom(2 * B, M, N), g4 = hs_geom(4 * B, M, N), g12 = hs_geom(NSCR_FAN * B, M, N);
  const size_t nspec = hs_elems(g), phys = (size_t)B * M * N;
  RPDE_CARVE("nsc2d_residual_fwd", NscrFwdWork, w, ws, ws_bytes, B, M, N, nspec, phys);
  const RelAffine a = rel_affine(affine);
  NSCR_CHECK_AFFINE("nsc2d_residual_fwd", a);
  hipStream_t st = as_stream(stream);
  // spec = [rho_w | rho_c | rho_d | P_w | P_c]
  RPDE_TRY(nscr_state(p, x, w.s, w.S, spec + 3 * nspec, B, M, N, a, st));
  const long groups = (long)M * (g.kp / 4);
  // the generator's fan-out of a state it only reads (MODE 0): its products, forcing and step tables are not touched
  hipLaunchKernelGGL((k_ns_update_fanout<0, true>), hs_grid(groups, 2 * B), dim3(256), 0, st, w.S, w.F, w.F, 0L,
                     NsTables<true>{nullptr, nullptr, inv_lap, nullptr, nullptr, 0.f}, w.D, g2);
  RPDE_LAUNCH_CHECK();
  RPDE_TRY(hs_irfft(g12, w.D, w.T1, w.P, st));
  const long n4 = 2 * (long)phys / 4;
  hipLaunchKernelGGL(k_ns_advect<true>, dim3(hs_blocks(n4, 2048)), dim3(256), 0, st, w.P, w.Fp, n4);
  RPDE_LAUNCH_CHECK();
  RPDE_TRY(hs_rfft(g4, w.Fp, w.T1, w.F, st));
  const int slots = rel_slots((long)M * g.kp);
  hipLaunchKernelGGL(k_nscr_residual, dim3(slots, B), dim3(256), 0, st, w.s.Xd, w.s.Dd, w.F,
                     NscrTables{em1_nu, m0_nu, m1_nu, em1_kappa, m0_kappa, m1_kappa}, forcing_spec, beta, scalar_weight, spec,
                     w.part, g);
  RPDE_LAUNCH_CHECK();
  return rel_final(w.part, rel, loss, stats, B, slots, 1.0 / ((double)M * (double)N), size_average, st);
}

int rpde_nsc2d_residual_bwd(const float* spec, const float* m1_nu, const float* m1_kappa, const float* inv_lap, float beta,
                            const float* affine, const float* stats, const float* grad_loss, const float* grad_rel,
                            float* grad_p, int B, int M, int N, int size_average, void* ws, size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(spec && m1_nu && m1_kappa && inv_lap && stats && grad_p && ws && (grad_loss || grad_rel),
                 "nsc2d_residual_bwd: null pointer");
  HS_CHECK_DIMS_2D_FAN("nsc2d_residual_bwd", B, M, N, NSCR_FAN);
  HS_CHECK_WS("nsc2d_residual_bwd", ws);
  RPDE_CHECK_ARG(al16(spec) && al16(m1_nu) && al16(m1_kappa) && al16(inv_lap) && al16(grad_p),
                 "nsc2d_residual_bwd: tables, spec and grad_p must be 16-byte aligned");
  const HalfSpec g = hs_geom(B, M, N), g3 = hs_geom(3 * B, M, N), g6 = hs_geom(6 * B, M, N), g8 = hs_geom(8 * B, M, N);
  const size_t nspec = hs_elems(g), phys = (size_t)B * M * N;
  RPDE_CARVE("nsc2d_residual_bwd", NscrBwdWork, w, ws, ws_bytes, nspec, phys);
  const RelAffine a = rel_affine(affine);
  NSCR_CHECK_AFFINE("nsc2d_residual_bwd", a);
  hipStream_t st = as_stream(stream);
  const long groups = (long)M * (g.kp / 4);
  // D = [g_w^ = m1_nu rho_w | g_c^ = m1_kappa rho_c | q^, v^, w_1^, w_2^, c_1^, c_2^ of the saved (P_w, P_c)]
  hipLaunchKernelGGL(k_ns_scale, hs_grid(2 * groups, B), dim3(256), 0, st, spec, m1_nu, w.D, g);
  RPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ns_scale, hs_grid(2 * groups, B), dim3(256), 0, st, spec + nspec, m1_kappa, w.D + nspec, g);
  RPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_ns_update_fanout<0, true>), hs_grid(groups, B), dim3(256), 0, st, const_cast<float*>(spec + 3 * nspec),
                     w.H, w.H, 0L, NsTables<true>{nullptr, nullptr, inv_lap, nullptr, nullptr, 0.f}, w.D + 2 * nspec, g);
  RPDE_LAUNCH_CHECK();
  RPDE_TRY(hs_irfft(g8, w.D, w.T1, w.P, st));
  hipLaunchKernelGGL(k_nscr_products, dim3(hs_blocks((long)phys / 4, 2048)), dim3(256), 0, st, w.P, w.Q, (long)phys / 4);
  RPDE_LAUNCH_CHECK();
  RPDE_TRY(hs_rfft(g6, w.Q, w.T1, w.H, st));
  hipLaunchKernelGGL(k_nscr_combine, hs_grid(groups, B), dim3(256), 0, st, spec, w.H, m1_nu, inv_lap, beta, w.G, g);
  RPDE_LAUNCH_CHECK();
  RPDE_TRY(hs_irfft(g3, w.G, w.T1, w.z, st));
  const int n4 = 3 * (M * N / 4);                                 // M and N even: whole groups of four per channel
  hipLaunchKernelGGL(k_nsr_grad, hs_grid(n4, B), dim3(256), 0, st, w.z, stats, grad_loss, grad_rel, grad_p, B, n4, size_average,
                     a.ap);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

}  // extern "C"
