// Navier-Stokes vorticity generator (ns_solver.hip): geometry, limits, and the full-spectrum 2-D transforms it shares
// with the mode-weighted loss (spectral_cf.hip).
#pragma once
#include "rpde_internal.h"
#include "plan.h"

namespace rpde {

constexpr int NS_MIN_N = 4;          // per axis, even
constexpr int NS_MAX_N = 4096;       // the full-spectrum tables are quadratic in it (WL2_MAX_N)

// A half spectrum is [images][M][re|im][kp]: rows ky in fft order (signed k1 = ky < M/2 ? ky : ky - M, so the Nyquist
// row counts as -M/2), kx = 0 .. N/2 along the contiguous axis, kp = N/2+1 rounded up to 4, padded columns zero.
struct NsGeom { int B, M, N, K, kp; };

// The plans of the resizers at equal sizes: real planar analysis / synthesis along N, complex column DFT keeping every
// row along M, both RPDE_NORM_BACKWARD, so forward is unnormalised and inverse carries 1 / (M N) in its tables.
// The first use of a grid builds the tables: it allocates and synchronises the stream once (plan.h).
int wl2_plans(const rpde_plan** pn, const rpde_plan** pm, int M, int N, hipStream_t st);
// z [rows, M, N] -> spec [rows][2M][kp]; s1: scratch of the spectrum's size
int wl2_forward_dft(const rpde_plan* pn, const rpde_plan* pm, const float* z, float* s1, float* spec, long rows, int M,
                    int N, hipStream_t st);
// spec [rows][2M][kp] -> z [rows, M, N] as torch.fft.irfft2: Im of the self-conjugate bins of the last axis is ignored
// (their synthesis table entries are sin(0) = 0); t1: scratch of the spectrum's size
int wl2_inverse_dft(const rpde_plan* pn, const rpde_plan* pm, const float* spec, float* t1, float* z, long rows, int M, int N,
                    hipStream_t st);

}  // namespace rpde
