// Equation-residual loss of the 1-D ETD family u_t = L u - (c/2) (u^2)_x (utils/loss.py EquationResidualLoss; no
// counterpart in the reference): does the one-step map x = u(t) -> p ~ u(t + D) satisfy the equation?  With the exponential
// trapezoidal rule (ETD2: the linear part exact, Nhat(w) = i g rfft(w^2) interpolated linearly between the two ends)
//   r^_n   = p^_n - E_n x^_n - m0_n rfft(x^2)_n - m1_n rfft(p^2)_n,      E = e^z, m0 = D (phi1 - phi2) i g, m1 = D phi2 i g
//   rel[b] = sqrt(E_r[b]) / (sqrt(E_x[b]) + REL_EPS),   E(z)[b] = sum_n c_n |z^_n|^2 / N,   c_n = 1 at n = 0, N/2, else 2
// on the half-spectrum layer of halfspec.h at M = 1.  The three tables are complex, [re|im][kp], formed by the caller in
// float64 and rounded once (include/rpde.h has the formulas): no division and no transcendental here but the final
// sqrt and the per-sample coefficient.  An affine decode (a_p p + b_p, a_x x + b_x) is folded into the first pass.
// Forward, three launches on the caller's stream:
//   rel_roots       (rel_loss.h) the N float64 roots of unity, into the workspace
//   k_res_spectrum  decode, square, the four spectra of [x~ | p~ | x~^2 | p~^2] and r^ in one pass, all in float64: for a
//                   good model r^ is a small remainder (1e-3 of p^ and less) of terms of the size of the field, and the
//                   fp32 transforms of halfspec.h leave an error of that size in it (see the kernel).  r^ is rounded once
//                   and stored for backward (padded columns zero); c_n |r^_n|^2 and c_n |x^_n|^2 per (field, sample,
//                   slot) in float64
//   rel_final       (rel_loss.h) adds the slots in fixed order: stats, rel, loss.  The slots of a sample depend on N
//                   alone, so its value does not depend on the batch around it
// Backward:  d rel[b] / d p = a_p coef_b (irfft(r^) - 2 p~ irfft(conj(m1) r^))
//   k_res_fan       [r^ | conj(m1) r^], 2 B spectra
//   synthesis       of the 2 B images
//   k_res_grad      p~ recomputed from p; coef_b is rel_coef of rel_loss.h
// The backward's spectral kernel streams as k_etd_stage_cx does: a thread owns one 16-byte group of k for both planes,
// whole float4 loads and stores, grid (blocks, images).  Its transform is that of halfspec.h: the gradient is no
// remainder, and holds its bound with it.
#include "etd_cx.h"
#include "halfspec.h"
#include "rel_loss.h"

namespace rpde {

constexpr int RES_BLOCK = 256;       // threads of a block of k_res_spectrum where an image has more than 64 columns
constexpr int RES_SLOTS = (HS_MAX_N / 2 + 4 + RES_BLOCK - 1) / RES_BLOCK;   // partial sums per (field, sample) at most

struct ResGeom : HalfSpec { int B; };

// grid (S, B), S = the blocks over the kp columns of an image; a thread owns one k; tw: the N roots of rel_roots.  The spectra of x~, p~, x~^2 and p~^2
// as float64 sums over the N points (the fields and their squares are formed in registers, the squares exact in
// float64), then r^ = p^ - E x^ - m0 rfft(x~^2) - m1 rfft(p~^2) in float64, rounded once into spec_r (padded columns zero).
// Why not the matrix-product transform of halfspec.h: its error in x^ is absolute, about 2e-7 |x| at every mode, and for
// a good model r^ is a remainder of 1e-3 |x| and less; E x^ carries that error into every mode whose E is far from 1,
// 5e-5 of rel where the float32 restatement has 4e-6.
// part[(f B + b) S + slot], field 0 = c_n |r^_n|^2, field 1 = c_n |x^_n|^2
__global__ __launch_bounds__(RES_BLOCK) void k_res_spectrum(const float* __restrict__ p, const float* __restrict__ x,
                                                            const double2* __restrict__ tw, const float* __restrict__ E,
                                                            const float* __restrict__ m0, const float* __restrict__ m1,
                                                            float* __restrict__ spec_r, double* __restrict__ part, ResGeom g,
                                                            RelAffine a) {
  const int b = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
  const float* __restrict__ xb = x + (long)b * g.N;
  const float* __restrict__ pb = p + (long)b * g.N;
  double er = 0.0, ex = 0.0;
  if (k < g.K) {
    double xr = 0.0, xi = 0.0, pr = 0.0, pi = 0.0, ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0;
    int idx = 0;                       // j k mod N
    // an image has few waves (a column a thread): eight roots in flight hide the gather's latency
#pragma unroll 8
    for (int j = 0; j < g.N; ++j) {
      const double xt = (double)fmaf(a.ax, xb[j], a.bx), pt = (double)fmaf(a.ap, pb[j], a.bp);
      const double2 w = tw[idx];
      idx += k;
      if (idx >= g.N) idx -= g.N;
      const double x2 = xt * xt, p2 = pt * pt;
      xr = fma(xt, w.x, xr); xi = fma(xt, w.y, xi);
      pr = fma(pt, w.x, pr); pi = fma(pt, w.y, pi);
      ar = fma(x2, w.x, ar); ai = fma(x2, w.y, ai);
      br = fma(p2, w.x, br); bi = fma(p2, w.y, bi);
    }
    const double e_r = E[k], e_i = E[g.kp + k], m0r = m0[k], m0i = m0[g.kp + k], m1r = m1[k], m1i = m1[g.kp + k];
    const double rr = pr - (e_r * xr - e_i * xi) - (m0r * ar - m0i * ai) - (m1r * br - m1i * bi);
    const double ri = pi - (e_r * xi + e_i * xr) - (m0r * ai + m0i * ar) - (m1r * bi + m1i * br);
    const double c = (k == 0 || k == g.N / 2) ? 1.0 : 2.0;
    er = c * (rr * rr + ri * ri);
    ex = c * (xr * xr + xi * xi);
    spec_r[(long)b * 2 * g.kp + k] = (float)rr;
    spec_r[(long)b * 2 * g.kp + g.kp + k] = (float)ri;
  } else if (k < g.kp) {
    spec_r[(long)b * 2 * g.kp + k] = 0.f;
    spec_r[(long)b * 2 * g.kp + g.kp + k] = 0.f;
  }
  rel_block_slots(er, ex, part, b, g.B, blockDim.x == RES_BLOCK);
}

// grid (blocks, B): out [2 B] spectra, out[b] = r^[b], out[B + b] = conj(m1) r^[b].  The padded columns of spec_r and of
// m1 are zero, and so are those of both outputs
__global__ __launch_bounds__(256) void k_res_fan(const float* __restrict__ spec_r, const float* __restrict__ m1,
                                                 float* __restrict__ out, ResGeom g) {
  const long per = 2L * g.kp, base = (long)blockIdx.y * per, second = (long)g.B * per;
  const int c4n = g.kp / 4;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < c4n; q += gridDim.x * blockDim.x) {
    const int k0 = q * 4, k1 = k0 + g.kp;
    float rr[4], ri[4], mr[4], mi[4], sr[4], si[4];
    ld4(spec_r + base + k0, rr); ld4(spec_r + base + k1, ri);
    ld4(m1 + k0, mr);            ld4(m1 + k1, mi);
#pragma unroll
    for (int j = 0; j < 4; ++j) etd_cmul(mr[j], -mi[j], rr[j], ri[j], sr[j], si[j]);
    st4(out + base + k0, rr);          st4(out + base + k1, ri);
    st4(out + second + base + k0, sr); st4(out + second + base + k1, si);
  }
}

// grid (blocks, B).  rs [2][B][N]: r = irfft(r^), s = irfft(conj(m1) r^).  grad_p = a_p coef_b (r - 2 p~ s)
__global__ __launch_bounds__(256) void k_res_grad(const float* __restrict__ p, const float* __restrict__ rs,
                                                  const float* __restrict__ stats, const float* __restrict__ grad_loss,
                                                  const float* __restrict__ grad_rel, float* __restrict__ grad_p, int B, int N,
                                                  int vec, int size_average, RelAffine a) {
  const int b = blockIdx.y;
  const float scale = a.ap * rel_coef(stats, grad_loss, grad_rel, b, B, size_average);
  const long row = (long)b * N;
  const float* __restrict__ pb = p + row;
  const float* __restrict__ rb = rs + row;
  const float* __restrict__ sb = rs + (long)B * N + row;
  float* __restrict__ gb = grad_p + row;
  const int i0 = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
  if (vec) {
    for (int i = i0; i < N / 4; i += step) {
      float pv[4], rv[4], sv[4], gv[4];
      ld4(pb + 4 * i, pv); ld4(rb + 4 * i, rv); ld4(sb + 4 * i, sv);
#pragma unroll
      for (int j = 0; j < 4; ++j) gv[j] = scale * fmaf(-2.f * fmaf(a.ap, pv[j], a.bp), sv[j], rv[j]);
      st4(gb + 4 * i, gv);
    }
  } else {
    for (int i = i0; i < N; i += step) gb[i] = scale * fmaf(-2.f * fmaf(a.ap, pb[i], a.bp), sb[i], rb[i]);
  }
}

// the batch limit of four fields of B images as one batch of the half-spectrum layer
constexpr int RES_MAX_B = 65535 / 4;
static bool res_dims_ok(int B, int N) { return B > 0 && B <= RES_MAX_B && hs_dims_ok(4 * B, 1, N); }

#define RES_CHECK_DIMS(what, B, N)                                                                                        \
  RPDE_CHECK_ARG(res_dims_ok(B, N), what ": bad B=%d N=%d (N even, %d .. %d, 1 <= B <= %d: four fields of B images)", B, N, \
                 HS_MIN_N, HS_MAX_N, RES_MAX_B)

}  // namespace rpde

using namespace rpde;

extern "C" {

size_t rpde_etd_residual_spec_elems(int B, int N) { return res_dims_ok(B, N) ? hs_elems(hs_geom(B, 1, N)) : 0; }

// forward: the roots of unity and the partial sums (doubles both)
struct ResFwdWork {
  double2* tw; double* part;
  ResFwdWork(Arena& ar, int B, int N)
      : tw(reinterpret_cast<double2*>(ar.take((size_t)4 * N))), part(reinterpret_cast<double*>(ar.take((size_t)2 * 2 * B * RES_SLOTS))) {}
};
// backward: two spectra and two fields
struct ResBwdWork {
  float *s2, *rs;
  ResBwdWork(Arena& ar, int B, int N) : s2(ar.take(hs_elems(hs_geom(2 * B, 1, N)))), rs(ar.take((size_t)2 * B * N)) {}
};

size_t rpde_etd_residual_ws_bytes(int B, int N) {
  return res_dims_ok(B, N) ? ws_max(ws_measure<ResFwdWork>(B, N), ws_measure<ResBwdWork>(B, N)) : 0;
}

int rpde_etd_residual_fwd(const float* p, const float* x, const float* E, const float* m0, const float* m1,
                          const float* affine, float* rel, float* loss, float* stats, float* spec_r, int B, int N,
                          int size_average, void* ws, size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(p && x && E && m0 && m1 && stats && spec_r && ws, "etd_residual_fwd: null pointer");
  RES_CHECK_DIMS("etd_residual_fwd", B, N);
  HS_CHECK_WS("etd_residual_fwd", ws);
  RPDE_CHECK_ARG(al16(E) && al16(m0) && al16(m1) && al16(spec_r), "etd_residual_fwd: tables and spec_r must be 16-byte aligned");
  const ResGeom g{hs_geom(B, 1, N), B};
  RPDE_CARVE("etd_residual_fwd", ResFwdWork, w, ws, ws_bytes, B, N);
  // a wave per image of at most 64 columns (N <= 120), RES_BLOCK threads otherwise; the blocks of an image are its slots
  const dim3 sb(g.kp <= 64 ? 64 : RES_BLOCK), sg((g.kp + sb.x - 1) / sb.x, B);
  hipStream_t st = as_stream(stream);
  RPDE_TRY(rel_roots(w.tw, N, 0, st));
  hipLaunchKernelGGL(k_res_spectrum, sg, sb, 0, st, p, x, w.tw, E, m0, m1, spec_r, w.part, g, rel_affine(affine));
  RPDE_LAUNCH_CHECK();
  return rel_final(w.part, rel, loss, stats, B, (int)sg.x, 1.0 / (double)N, size_average, st);
}

int rpde_etd_residual_bwd(const float* p, const float* spec_r, const float* m1, const float* affine, const float* stats,
                          const float* grad_loss, const float* grad_rel, float* grad_p, int B, int N, int size_average,
                          void* ws, size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(p && spec_r && m1 && stats && grad_p && ws && (grad_loss || grad_rel), "etd_residual_bwd: null pointer");
  RES_CHECK_DIMS("etd_residual_bwd", B, N);
  HS_CHECK_WS("etd_residual_bwd", ws);
  RPDE_CHECK_ARG(al16(m1) && al16(spec_r), "etd_residual_bwd: tables and spec_r must be 16-byte aligned");
  const ResGeom g{hs_geom(B, 1, N), B};
  const HalfSpec g2 = hs_geom(2 * B, 1, N);
  RPDE_CARVE("etd_residual_bwd", ResBwdWork, w, ws, ws_bytes, B, N);
  hipStream_t st = as_stream(stream);
  const dim3 sb(hs_block(g.kp / 4)), sg = hs_grid(g.kp / 4, B, sb.x);
  hipLaunchKernelGGL(k_res_fan, sg, sb, 0, st, spec_r, m1, w.s2, g);
  RPDE_LAUNCH_CHECK();
  RPDE_TRY(hs_irfft(g2, w.s2, nullptr, w.rs, st));
  const int vec = N % 4 == 0 && al16(p) && al16(grad_p);
  hipLaunchKernelGGL(k_res_grad, hs_grid(vec ? N / 4 : N, B), dim3(256), 0, st, p, w.rs, stats, grad_loss, grad_rel, grad_p, B, N,
                     vec, size_average, rel_affine(affine));
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

}  // extern "C"
