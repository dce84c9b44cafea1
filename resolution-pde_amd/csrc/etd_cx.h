// Complex products on the plane layout of a half spectrum, in fused multiply-adds: what the complex-symbol stage kernels
// (etd1d.hip) and the equation-residual loss (etd_residual.hip) share.
#pragma once
#include <hip/hip_runtime.h>

namespace rpde {

// p = c x
__device__ __forceinline__ void etd_cmul(float cr, float ci, float xr, float xi, float& pr, float& pi) {
  pr = fmaf(-ci, xi, cr * xr);
  pi = fmaf(ci, xr, cr * xi);
}
// p += c x
__device__ __forceinline__ void etd_cfma(float cr, float ci, float xr, float xi, float& pr, float& pi) {
  pr = fmaf(-ci, xi, fmaf(cr, xr, pr));
  pi = fmaf(ci, xr, fmaf(cr, xi, pi));
}

}  // namespace rpde
