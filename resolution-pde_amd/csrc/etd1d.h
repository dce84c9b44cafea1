// 1-D exponential-time-differencing generator (etd1d.hip): geometry and limits.
#pragma once
#include "ns_solver.h"

namespace rpde {

constexpr int ETD_MIN_N = NS_MIN_N;  // even; the full-spectrum tables are those of the NS generator
constexpr int ETD_MAX_N = NS_MAX_N;

// A half spectrum is [images][re|im][kp]: k = 0 .. N/2 along the contiguous axis, K = N/2+1 of them, kp = K rounded up
// to 4, padded columns zero -- the one-row case of NsGeom's layout.
struct EtdGeom { int B, N, K, kp; };

}  // namespace rpde
