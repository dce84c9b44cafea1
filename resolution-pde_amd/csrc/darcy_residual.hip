// Equation-residual loss of the Darcy generator (utils/loss.py DarcyResidualLoss; no counterpart in the reference): does
// the map a -> p ~ u satisfy -div(a grad u) = f, u = 0 on the boundary, in the generator's own discretisation (darcy.hip)?
// The equation is steady and the network's input is the operator's coefficient.  With the decoded fields
// a~ = a_x a + b_x, u~ = a_p p + b_p and r_b = f - A(a~_b) u~_b, A the operator of darcy_row4 bit for bit:
//   dual norm:  E_b = sum_k inv_lambda_k (S r_b S^T)_k^2 = r_b . P^-1 r_b,  P = A(1) the solver's preconditioner
//   L2:         E_b = |r_b|^2
//   rel[b] = sqrt(E_b) / (D + REL_EPS),  D the same norm of f, formed by the caller in float64
// Every face weight lies in [a_min, a_max], so a_min P <= A(a) <= a_max P and r . P^-1 r is the energy-norm error of the
// prediction to within the contrast, at every grid size; the L2 form grows with s^2.
// Forward, on the caller's stream:
//   k_darcyres_apply       r = f - A(a~) u~, decoded on load, halo included.  L2: into spec, with the partials of |r|^2
//   rowdft, gemm           dual norm: rh = S r S^T into spec                                  (sep2d)
//   k_darcyres_energy      dual norm: spec = inv_lambda . rh, partials of inv_lambda rh^2
//   rel_final              (rel_loss.h) adds the slots in fixed order: stats[b] = (sqrt(E_b), D), rel, loss
// Backward (A is self-adjoint: one more application of the same operator):
//   rowdft, gemm           dual norm: z = S^T spec S                                          (sep2d; L2: z = spec = r)
//   k_darcyres_grad        grad_p = -a_p coef_b A(a~) z, coef_b the family's rel_coef
// A thread owns one 16-byte group of a row, grid (blocks, B), per-block double partials in slots that depend on the grid
// alone: no atomics, identical calls give identical bits, and a batch equals its B = 1 calls bit for bit.
// A decoded coefficient that is not positive makes the loss non-finite: the caller's contract, as in the solver.
#include "darcy.h"
#include "rel_loss.h"

namespace rpde {

// grid (blocks, B).  r = f - A(a~) u~ for one right-hand side f [s][s]; L2: the block's partial of |r|^2 into field 0
// of its slot and the denominator's energy d2 into field 1 (slot 0 carries it, the others zero)
template <bool L2>
__global__ __launch_bounds__(256) void k_darcyres_apply(const float* __restrict__ a, const float* __restrict__ p,
                                                        const float* __restrict__ f, float* __restrict__ r,
                                                        double* __restrict__ part, double d2, DarcyDecode map, int s) {
  const int b = blockIdx.y, c4n = s / 4, per4 = s * c4n;
  const long per = (long)s * s;
  const float* __restrict__ ab = a + (long)b * per;
  const float* __restrict__ pb = p + (long)b * per;
  const float s2 = (float)s * (float)s;
  double acc = 0.0;                  // the squares are exact in float64: the sum adds nothing to the error of r itself
  for (int v = blockIdx.x * 256 + threadIdx.x; v < per4; v += gridDim.x * 256) {
    const int i = v / c4n, j0 = (v - i * c4n) * 4;
    const long o = (long)i * s + j0;
    float au[4], fv[4];
    darcy_row4(ab, pb, s, i, j0, s2, au, map);
    ld4(f + o, fv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma clang fp contract(off)      // f minus the rounded A u, never fused with the row's last product: r is f minus the
      fv[j] = fv[j] - au[j];        // apply entry's output bit for bit
      if (L2) acc = fma((double)fv[j], (double)fv[j], acc);
    }
    st4(r + (long)b * per + o, fv);
  }
  if (L2) rel_block_slots(acc, blockIdx.x == 0 && threadIdx.x == 0 ? d2 : 0.0, part, b, gridDim.y, true);
}

// grid (blocks, B).  spec = inv_lambda . rh in place, the block's partial of sum inv_lambda rh^2 (non-negative terms)
// into field 0 of its slot, d2 into field 1 as above
__global__ __launch_bounds__(256) void k_darcyres_energy(float* __restrict__ spec, const float* __restrict__ inv_lambda,
                                                         double* __restrict__ part, double d2, int per4) {
  const int b = blockIdx.y;
  float* __restrict__ sb = spec + (long)b * per4 * 4;
  double acc = 0.0;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < per4; v += gridDim.x * 256) {
    float rh[4], il[4];
    ld4(sb + 4L * v, rh);
    ld4(inv_lambda + 4L * v, il);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float t = il[j] * rh[j];
      acc = fma((double)t, (double)rh[j], acc);
      rh[j] = t;
    }
    st4(sb + 4L * v, rh);
  }
  rel_block_slots(acc, blockIdx.x == 0 && threadIdx.x == 0 ? d2 : 0.0, part, b, gridDim.y, true);
}

// grid (blocks, B).  grad_p = -a_p coef_b A(a~) z: the coefficient decoded on load, z as it stands
__global__ __launch_bounds__(256) void k_darcyres_grad(const float* __restrict__ a, const float* __restrict__ z,
                                                       const float* __restrict__ stats, const float* __restrict__ grad_loss,
                                                       const float* __restrict__ grad_rel, float* __restrict__ grad_p,
                                                       int size_average, float ap, DarcyDecode map, int s) {
  const int b = blockIdx.y, c4n = s / 4, per4 = s * c4n;
  const long per = (long)s * s;
  const float scale = -ap * rel_coef(stats, grad_loss, grad_rel, b, gridDim.y, size_average);
  const float s2 = (float)s * (float)s;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < per4; v += gridDim.x * 256) {
    const int i = v / c4n, j0 = (v - i * c4n) * 4;
    float az[4];
    darcy_row4(a + (long)b * per, z + (long)b * per, s, i, j0, s2, az, map);
#pragma unroll
    for (int j = 0; j < 4; ++j) az[j] *= scale;
    st4(grad_p + (long)b * per + (long)i * s + j0, az);
  }
}

// forward: the partial sums of both fields; dual norm: the residual and the transform's intermediate as well.
// backward: nothing for L2; dual norm: the transform's intermediate and z.  Both fit the solve's seven fields and three
// sets of partials, so rpde_darcy2d_ws_bytes sizes them
struct DarcyResFwdWork {
  double* part; float *r, *tmp;
  DarcyResFwdWork(Arena& ar, int B, int s, bool dual)
      : part(reinterpret_cast<double*>(ar.take((size_t)2 * 2 * B * hs_grid((long)s * (s / 4), B).x))),
        r(dual ? ar.take((size_t)B * s * s) : nullptr), tmp(dual ? ar.take((size_t)B * s * s) : nullptr) {}
};
struct DarcyResBwdWork {
  float *tmp, *z;
  DarcyResBwdWork(Arena& ar, int B, int s, bool dual)
      : tmp(dual ? ar.take((size_t)B * s * s) : nullptr), z(dual ? ar.take((size_t)B * s * s) : nullptr) {}
};

}  // namespace rpde

using namespace rpde;

extern "C" {

size_t rpde_darcy2d_residual_spec_elems(int B, int s) { return darcy_dims_ok(B, s) ? (size_t)B * s * s : 0; }

int rpde_darcy2d_residual_fwd(const float* p, const float* a, const float* f, const float* S, const float* inv_lambda,
                              double D, const float* affine, float* rel, float* loss, float* stats, float* spec, int B,
                              int s, int size_average, void* ws, size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(p && a && f && stats && spec && ws, "darcy2d_residual_fwd: null pointer");
  RPDE_CHECK_ARG(!S == !inv_lambda, "darcy2d_residual_fwd: S and inv_lambda go together (both null: the L2 norm)");
  DARCY_CHECK_DIMS("darcy2d_residual_fwd", B, s);
  HS_CHECK_WS("darcy2d_residual_fwd", ws);
  RPDE_CHECK_ARG(D > 0.0 && D < INFINITY, "darcy2d_residual_fwd: the norm D of the right-hand side must be positive and finite");
  RPDE_CHECK_ARG(al16(p) && al16(a) && al16(f) && al16(S) && al16(inv_lambda) && al16(spec),
                 "darcy2d_residual_fwd: fields, tables and spec must be 16-byte aligned");
  const bool dual = S != nullptr;
  RPDE_CARVE("darcy2d_residual_fwd", DarcyResFwdWork, w, ws, ws_bytes, B, s, dual);
  hipStream_t st = as_stream(stream);
  const RelAffine af = rel_affine(affine);
  const DarcyDecode map{af.ax, af.bx, af.ap, af.bp};
  const int per4 = s * (s / 4);
  const dim3 grid = hs_grid(per4, B);
  if (dual) {
    hipLaunchKernelGGL(k_darcyres_apply<false>, grid, dim3(256), 0, st, a, p, f, w.r, w.part, D * D, map, s);
    RPDE_LAUNCH_CHECK();
    RPDE_TRY(sep2d(w.r, S, false, S, false, w.tmp, spec, B, s, st));
    hipLaunchKernelGGL(k_darcyres_energy, grid, dim3(256), 0, st, spec, inv_lambda, w.part, D * D, per4);
  } else {
    hipLaunchKernelGGL(k_darcyres_apply<true>, grid, dim3(256), 0, st, a, p, f, spec, w.part, D * D, map, s);
  }
  RPDE_LAUNCH_CHECK();
  return rel_final(w.part, rel, loss, stats, B, (int)grid.x, 1.0, size_average, st);
}

int rpde_darcy2d_residual_bwd(const float* a, const float* spec, const float* S, const float* affine, const float* stats,
                              const float* grad_loss, const float* grad_rel, float* grad_p, int B, int s, int size_average,
                              void* ws, size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(a && spec && stats && grad_p && ws && (grad_loss || grad_rel), "darcy2d_residual_bwd: null pointer");
  DARCY_CHECK_DIMS("darcy2d_residual_bwd", B, s);
  HS_CHECK_WS("darcy2d_residual_bwd", ws);
  RPDE_CHECK_ARG(al16(a) && al16(spec) && al16(S) && al16(grad_p),
                 "darcy2d_residual_bwd: fields, tables and spec must be 16-byte aligned");
  const bool dual = S != nullptr;
  RPDE_CARVE("darcy2d_residual_bwd", DarcyResBwdWork, w, ws, ws_bytes, B, s, dual);
  hipStream_t st = as_stream(stream);
  const RelAffine af = rel_affine(affine);
  const DarcyDecode map{af.ax, af.bx, 1.f, 0.f};
  if (dual) RPDE_TRY(sep2d(spec, S, true, S, true, w.tmp, w.z, B, s, st));
  hipLaunchKernelGGL(k_darcyres_grad, hs_grid((long)s * (s / 4), B), dim3(256), 0, st, a, dual ? w.z : spec, stats, grad_loss,
                     grad_rel, grad_p, size_average, af.ap, map, s);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

}  // extern "C"
