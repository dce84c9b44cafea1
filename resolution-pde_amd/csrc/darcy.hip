// Darcy flow generator on the unit square (reference: dataloaders/darcy_loader.py and the piececonst_* files it reads):
// -div(a grad u) = f, u = 0 on the boundary, finite volumes on s x s cell centres, solved per sample by conjugate
// gradients preconditioned with the constant-coefficient Dirichlet Laplacian.  gfx950, wave64.
//
// Discrete operator (include/rpde.h has the formulas): a face between cells c and n weighs w = 2 a_c a_n / (a_c + a_n),
// a boundary face 2 a_c with u = 0 behind it, (A u)_c = s^2 sum_faces w (u_c - u_n) -- always in this difference form.
// The weights are formed from `a` inside the apply kernel: one array and its halo per iteration instead of two face
// arrays, and w(c, n) == w(n, c) bit for bit.  The preconditioner is P^-1 r = S^T (inv_lambda . (S r S^T)) S with the
// orthogonal DST-II table S: two sep2d products (out_b = L in_b R^T, a cf_rowdft for the left factor and one GEMM over
// [B s, s] for the right one) around one streaming scale.
//
// One iteration is nine launches on the caller's stream, no host synchronisation, no device-to-host read:
//   k_darcy_apply<1>     Ap = A p, per-block partials of p.Ap                   reads a, p (+ halo), writes Ap
//   k_darcy_update       alpha = rz / pAp; u += alpha p, r -= alpha Ap; partials of |r|^2     reads u, ul, r, p, Ap, writes u, ul, r
//   rowdft, gemm         rh = S r S^T                                            reads r, writes T; reads T, writes rh
//   k_darcy_scale        rh *= inv_lambda                                        reads rh, table, writes rh
//   rowdft, gemm         z = S^T rh S                                            reads rh, writes T; reads T, writes z
//   k_darcy_dot          partials of r.z                                         reads r, z
//   k_darcy_direction    freeze test, beta = rz_new / rz_old, p = z + beta p     reads z, p, writes p
// Every streaming kernel: a thread owns one 16-byte group of a row, grid (blocks, B), every block of a sample re-reduces
// that sample's partials in a fixed order (doubles, one per block), so a sample never sees another sample's scalars and
// there are no atomics: identical calls give identical bits.  The per-sample state (rz, |f|^2, active, frozen_at) lives in
// two device records written by thread 0 of block 0 with ordinary stores; a kernel reads one record and writes the other.
// A sample freezes -- alpha = beta = 0, u fixed, its blocks return at once -- when |r| <= tol |f| or pAp or rz is not a
// positive finite number.  After the loop one more apply forms f - A u and its norm: the true residual.
// u is carried as an unevaluated sum u + ul (two-float arithmetic in the update kernel): a dozen plain fp32 updates would
// each round u at its full size, and that high-frequency noise times s^2 is what the true residual then shows (at
// s = 32: 2e-5 plain against 6e-6 for the correctly rounded exact solution).  u is always the rounded value of the pair.
#include "darcy.h"

namespace rpde {

struct DarcyState { double rz, ff; int active, frozen_at; };

// MODE 0: out = A u                                   (rpde_darcy2d_apply)
//      1: out = A u and partials of u . out, frozen samples skipped     (u is the direction p)
//      2: partials of |f - A u|^2, nothing stored     (the true residual after the loop)
// grid (blocks, B); f has fstride floats between samples (0: one right-hand side for the batch)
template <int MODE>
__global__ __launch_bounds__(256) void k_darcy_apply(const float* __restrict__ a, const float* __restrict__ u,
                                                     float* __restrict__ out, const float* __restrict__ f, long fstride,
                                                     double* __restrict__ part, const DarcyState* __restrict__ st, int s) {
  const int b = blockIdx.y;
  if (MODE == 1 && !st[b].active) return;
  const int c4n = s / 4, per4 = s * c4n;
  const long per = (long)s * s;
  const float* __restrict__ ab = a + (long)b * per;
  const float* __restrict__ ub = u + (long)b * per;
  const float s2 = (float)s * (float)s;
  float acc = 0.f;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < per4; v += gridDim.x * 256) {
    const int i = v / c4n, j0 = (v - i * c4n) * 4;
    const long o = (long)i * s + j0;
    float au[4];
    darcy_row4(ab, ub, s, i, j0, s2, au);
    if (MODE != 2) st4(out + (long)b * per + o, au);
    if (MODE == 1) {
      float p[4];
      ld4(ub + o, p);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = fmaf(p[j], au[j], acc);
    }
    if (MODE == 2) {
      float fv[4];
      ld4(f + (long)b * fstride + o, fv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = fv[j] - au[j];
        acc = fmaf(d, d, acc);
      }
    }
  }
  if (MODE != 0) darcy_block_partial(acc, part + (long)b * gridDim.x);
}

// u = ul = 0, r = f, partials of |f|^2
__global__ __launch_bounds__(256) void k_darcy_init(const float* __restrict__ f, long fstride, float* __restrict__ u,
                                                    float* __restrict__ ul, float* __restrict__ r, double* __restrict__ part,
                                                    int s) {
  const int b = blockIdx.y, per4 = s * (s / 4);
  const long base = (long)b * s * s;
  const float zero[4] = {0.f, 0.f, 0.f, 0.f};
  float acc = 0.f;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < per4; v += gridDim.x * 256) {
    float fv[4];
    ld4(f + (long)b * fstride + 4L * v, fv);
    st4(u + base + 4L * v, zero);
    st4(ul + base + 4L * v, zero);
    st4(r + base + 4L * v, fv);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = fmaf(fv[j], fv[j], acc);
  }
  darcy_block_partial(acc, part + (long)b * gridDim.x);
}

// alpha = rz / pAp from the sample's partials; u += alpha p, r -= alpha Ap, partials of |r|^2.  A sample whose pAp is not
// a positive finite number freezes here, before the update of iteration `iter`.  u + ul is the iterate, advanced by the
// exact product alpha p in two-float arithmetic, so u is the pair's rounded value after every update.
__global__ __launch_bounds__(256) void k_darcy_update(float* __restrict__ u, float* __restrict__ ul, float* __restrict__ r,
                                                      const float* __restrict__ p,
                                                      const float* __restrict__ Ap, const double* __restrict__ pap_part,
                                                      double* __restrict__ rr_part, const DarcyState* __restrict__ sin,
                                                      DarcyState* __restrict__ sout, int iter, int s) {
  const int b = blockIdx.y;
  DarcyState S = sin[b];
  const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
  if (!S.active) {
    if (writer) sout[b] = S;
    return;
  }
  const double pap = darcy_fold(pap_part + (long)b * gridDim.x, gridDim.x);
  if (!darcy_pos_finite(pap)) {
    S.active = 0;
    S.frozen_at = iter;
    if (writer) sout[b] = S;
    return;
  }
  const float alpha = (float)(S.rz / pap);
  const int per4 = s * (s / 4);
  const long base = (long)b * s * s;
  float acc = 0.f;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < per4; v += gridDim.x * 256) {
    const long o = base + 4L * v;
    float uv[4], lv[4], rv[4], pv[4], av[4];
    ld4(u + o, uv); ld4(ul + o, lv); ld4(r + o, rv); ld4(p + o, pv); ld4(Ap + o, av);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma clang fp contract(off)      // the two-sums need the rounded product and sums as written, not fused ones
      // alpha p = ph + pl exactly (the fma gives the product's rounding error); (t, e) = two-sum(u, ph)
      const float ph = alpha * pv[j], pl = fmaf(alpha, pv[j], -ph);
      const float t = uv[j] + ph, bb = t - uv[j], e = (uv[j] - (t - bb)) + (ph - bb);
      // the low parts are a few ulps of u at most: adding them rounds at eps^2; then renormalise with a second two-sum
      const float l = e + (pl + lv[j]), un = t + l, cc = un - t;
      lv[j] = (t - (un - cc)) + (l - cc);
      uv[j] = un;
      rv[j] = fmaf(-alpha, av[j], rv[j]);
      acc = fmaf(rv[j], rv[j], acc);
    }
    st4(u + o, uv);
    st4(ul + o, lv);
    st4(r + o, rv);
  }
  darcy_block_partial(acc, rr_part + (long)b * gridDim.x);
  if (writer) sout[b] = S;
}

// x *= table over B images of n4 groups, table [s][s] shared by the batch
__global__ __launch_bounds__(256) void k_darcy_scale(float* __restrict__ x, const float* __restrict__ table, int per4) {
  float* __restrict__ xb = x + (long)blockIdx.y * per4 * 4;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < per4; v += gridDim.x * 256) {
    float xv[4], t[4];
    ld4(xb + 4L * v, xv);
    ld4(table + 4L * v, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) xv[j] *= t[j];
    st4(xb + 4L * v, xv);
  }
}

// partials of r . z; st null (the start of a solve): every sample
__global__ __launch_bounds__(256) void k_darcy_dot(const float* __restrict__ r, const float* __restrict__ z,
                                                   double* __restrict__ part, const DarcyState* __restrict__ st, int s) {
  const int b = blockIdx.y;
  if (st && !st[b].active) return;
  const int per4 = s * (s / 4);
  const long base = (long)b * s * s;
  float acc = 0.f;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < per4; v += gridDim.x * 256) {
    float rv[4], zv[4];
    ld4(r + base + 4L * v, rv);
    ld4(z + base + 4L * v, zv);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = fmaf(rv[j], zv[j], acc);
  }
  darcy_block_partial(acc, part + (long)b * gridDim.x);
}

// INIT: the state's first record from the partials of |f|^2 (in rr_part) and of r.z; p = z.
// else: the freeze test of iteration `iter` (|r|^2 <= tol^2 |f|^2, or rz not positive finite), beta = rz_new / rz_old,
//       p = z + beta p.
template <bool INIT>
__global__ __launch_bounds__(256) void k_darcy_direction(float* __restrict__ p, const float* __restrict__ z,
                                                         const double* __restrict__ rr_part, const double* __restrict__ rz_part,
                                                         const DarcyState* __restrict__ sin, DarcyState* __restrict__ sout,
                                                         int iter, double tol2, int s) {
  const int b = blockIdx.y;
  const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
  DarcyState S;
  if (INIT) {
    S.rz = 0.0; S.ff = 0.0; S.active = 1; S.frozen_at = 0;
  } else {
    S = sin[b];
    if (!S.active) {
      if (writer) sout[b] = S;
      return;
    }
  }
  const double rr = darcy_fold(rr_part + (long)b * gridDim.x, gridDim.x);
  const double rz = darcy_fold(rz_part + (long)b * gridDim.x, gridDim.x);
  if (INIT) S.ff = rr;
  if (!(rr > tol2 * S.ff) || !darcy_pos_finite(rz)) {
    S.active = 0;
    S.frozen_at = INIT ? 0 : iter + 1;
    if (writer) sout[b] = S;
    return;
  }
  const float beta = INIT ? 0.f : (float)(rz / S.rz);
  S.rz = rz;
  const int per4 = s * (s / 4);
  const long base = (long)b * s * s;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < per4; v += gridDim.x * 256) {
    const long o = base + 4L * v;
    float zv[4];
    ld4(z + o, zv);
    if (!INIT) {
      float pv[4];
      ld4(p + o, pv);
#pragma unroll
      for (int j = 0; j < 4; ++j) zv[j] = fmaf(beta, pv[j], zv[j]);
    }
    st4(p + o, zv);
  }
  if (writer) sout[b] = S;
}

// rel[b] = |f - A u| / |f| from the residual's partials (0 for f = 0), frozen_at[b] (`iterations`: never froze);
// grid (B), one wave
__global__ __launch_bounds__(64) void k_darcy_finish(const double* __restrict__ part, int nblk, const DarcyState* __restrict__ st,
                                                     float* __restrict__ rel, int* __restrict__ frozen_at, int iterations) {
  const int b = blockIdx.x;
  const double rr = darcy_fold(part + (long)b * nblk, nblk);
  const DarcyState S = st[b];
  if (threadIdx.x == 0) {
    rel[b] = S.ff > 0.0 ? (float)sqrt(rr / S.ff) : (rr == 0.0 ? 0.f : INFINITY);
    frozen_at[b] = S.active ? iterations : S.frozen_at;
  }
}

}  // namespace rpde

using namespace rpde;

extern "C" {

// rpde_darcy2d_solve: r, p, Ap, z, the low part of u, the transform's intermediate and the spectrum; three sets of
// per-block partials (doubles); two state records.  rpde_sep2d needs one field, which fits the first
struct DarcyWork {
  float *r, *p, *Ap, *z, *ul, *tmp, *rh; double *pap, *rr, *rz; DarcyState *s0, *s1;
  DarcyWork(Arena& ar, int B, int s) {
    const size_t phys = (size_t)B * s * s, nblk = hs_grid((long)s * (s / 4), B).x;
    const auto state = [&] { return reinterpret_cast<DarcyState*>(ar.take((size_t)B * sizeof(DarcyState) / sizeof(float))); };
    const auto partials = [&] { return reinterpret_cast<double*>(ar.take(2 * B * nblk)); };
    r = ar.take(phys); p = ar.take(phys); Ap = ar.take(phys); z = ar.take(phys);
    ul = ar.take(phys); tmp = ar.take(phys); rh = ar.take(phys);
    pap = partials(); rr = partials(); rz = partials();
    s0 = state(); s1 = state();
  }
};

size_t rpde_darcy2d_ws_bytes(int B, int s) { return darcy_dims_ok(B, s) ? ws_measure<DarcyWork>(B, s) : 0; }

int rpde_darcy2d_apply(const float* a, const float* u, float* Au, int B, int s, void* stream) {
  RPDE_CHECK_ARG(a && u && Au, "darcy2d_apply: null pointer");
  DARCY_CHECK_DIMS("darcy2d_apply", B, s);
  RPDE_CHECK_ARG(al16(a) && al16(u) && al16(Au), "darcy2d_apply: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(k_darcy_apply<0>, hs_grid((long)s * (s / 4), B), dim3(256), 0, as_stream(stream), a, u, Au,
                     (const float*)nullptr, 0L, (double*)nullptr, (const DarcyState*)nullptr, s);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_sep2d(const float* in, const float* L, const float* R, float* out, int B, int s, void* ws, size_t ws_bytes,
               void* stream) {
  RPDE_CHECK_ARG(in && L && R && out && ws, "sep2d: null pointer");
  DARCY_CHECK_DIMS("sep2d", B, s);
  HS_CHECK_WS("sep2d", ws);
  RPDE_CHECK_ARG(al16(in) && al16(L) && al16(R) && al16(out), "sep2d: pointers must be 16-byte aligned");
  Arena ar(ws, ws_bytes);
  float* tmp = ar.take((size_t)B * s * s);
  RPDE_CLAIM_WS("sep2d", ar, ws_bytes);
  return sep2d(in, L, false, R, false, tmp, out, B, s, as_stream(stream));
}

int rpde_darcy2d_solve(const float* a, const float* f, int f_batched, const float* S, const float* inv_lambda, float* u,
                       float* rel_residual, int* frozen_at, int B, int s, int iterations, float tol, void* ws,
                       size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(a && f && S && inv_lambda && u && rel_residual && frozen_at && ws, "darcy2d_solve: null pointer");
  DARCY_CHECK_DIMS("darcy2d_solve", B, s);
  HS_CHECK_WS("darcy2d_solve", ws);
  RPDE_CHECK_ARG(iterations >= 0, "darcy2d_solve: iterations %d < 0", iterations);
  RPDE_CHECK_ARG(tol >= 0.f && tol < INFINITY, "darcy2d_solve: tol must be finite and >= 0");
  RPDE_CHECK_ARG(al16(a) && al16(f) && al16(S) && al16(inv_lambda) && al16(u),
                 "darcy2d_solve: fields and tables must be 16-byte aligned");
  const dim3 grid = hs_grid((long)s * (s / 4), B);
  const size_t nblk = grid.x;
  RPDE_CARVE("darcy2d_solve", DarcyWork, w, ws, ws_bytes, B, s);
  float *r = w.r, *p = w.p, *Ap = w.Ap, *z = w.z, *ul = w.ul, *tmp = w.tmp, *rh = w.rh;
  double *pap = w.pap, *rr = w.rr, *rz = w.rz;
  DarcyState *s0 = w.s0, *s1 = w.s1;
  hipStream_t st = as_stream(stream);
  const dim3 blk(256);
  const long fstride = f_batched ? (long)s * s : 0;
  const int per4 = s * (s / 4);
  const double tol2 = (double)tol * (double)tol;
  // z = P^-1 r
  auto precondition = [&]() -> int {
    RPDE_TRY(sep2d(r, S, false, S, false, tmp, rh, B, s, st));
    hipLaunchKernelGGL(k_darcy_scale, grid, blk, 0, st, rh, inv_lambda, per4);
    RPDE_LAUNCH_CHECK();
    return sep2d(rh, S, true, S, true, tmp, z, B, s, st);
  };
  hipLaunchKernelGGL(k_darcy_init, grid, blk, 0, st, f, fstride, u, ul, r, rr, s);
  RPDE_LAUNCH_CHECK();
  RPDE_TRY(precondition());
  hipLaunchKernelGGL(k_darcy_dot, grid, blk, 0, st, r, z, rz, (const DarcyState*)nullptr, s);
  RPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_darcy_direction<true>, grid, blk, 0, st, p, z, rr, rz, (const DarcyState*)nullptr, s0, 0, tol2, s);
  RPDE_LAUNCH_CHECK();
  for (int k = 0; k < iterations; ++k) {
    hipLaunchKernelGGL(k_darcy_apply<1>, grid, blk, 0, st, a, p, Ap, (const float*)nullptr, 0L, pap, s0, s);
    RPDE_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_darcy_update, grid, blk, 0, st, u, ul, r, p, Ap, pap, rr, s0, s1, k, s);
    RPDE_LAUNCH_CHECK();
    RPDE_TRY(precondition());
    hipLaunchKernelGGL(k_darcy_dot, grid, blk, 0, st, r, z, rz, s1, s);
    RPDE_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_darcy_direction<false>, grid, blk, 0, st, p, z, rr, rz, s1, s0, k, tol2, s);
    RPDE_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_darcy_apply<2>, grid, blk, 0, st, a, u, (float*)nullptr, f, fstride, pap, (const DarcyState*)nullptr, s);
  RPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_darcy_finish, dim3(B), dim3(64), 0, st, pap, (int)nblk, s0, rel_residual, frozen_at, iterations);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

}  // extern "C"
