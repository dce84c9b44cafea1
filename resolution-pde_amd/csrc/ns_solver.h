// Navier-Stokes vorticity generator (ns_solver.hip): geometry and limits.
#pragma once
#include "rpde_internal.h"

namespace rpde {

constexpr int NS_MIN_N = 4;          // per axis, even
constexpr int NS_MAX_N = 4096;       // the full-spectrum tables are quadratic in it (WL2_MAX_N of spectral_loss.hip)

// A half spectrum is [images][M][re|im][kp]: rows ky in fft order (signed k1 = ky < M/2 ? ky : ky - M, so the Nyquist
// row counts as -M/2), kx = 0 .. N/2 along the contiguous axis, kp = N/2+1 rounded up to 4, padded columns zero.
struct NsGeom { int B, M, N, K, kp; };

}  // namespace rpde
