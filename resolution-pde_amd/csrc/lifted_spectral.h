// FFNO2D's first spectral layer on the unlifted input (lifted_spectral.hip): what fspectral.hip needs of it.
#pragma once
#include <cstddef>

namespace rpde {

constexpr int LIFT_MAXC = 4;          // thin input channels the kernels are instantiated for
// workspace of rpde_lifted_fspectral2d_fwd / _bwd for any Cin <= LIFT_MAXC (shapes of the fused 2-D path)
size_t lifted2d_ws_bytes(int B, int M, int N, int K);

}  // namespace rpde
