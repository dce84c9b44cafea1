// Split backward of the fused three-layer FeedForward (ff_bwd_split.hip): the chain of ff_fused.hip cut at du2, the
// second product fused with the first layer's weight and data gradient, so that du1 never goes to HBM.
#pragma once
#include "rpde_internal.h"
#include "pointwise.h"

namespace rpde {

// stash mode with both first-layer gradients wanted, at a size the streaming first-layer kernel takes;
// RPDE_FF_BWD_SPLIT=0 turns the path off (k_ff3_bwd_h2 and k_wgrad_h2 with the data gradient take over)
bool ff_bwd_split_ok(long P, int hid, int dim);

// ds: the saved derivative factors d1, d2.  Writes dz3 [P,64] and du2 [P,256] (operands of the two upper weight
// gradients), gx [P,64], the first layer's weight-gradient slabs (folded into gw1 by `folds`, or here when that is full)
// and part [grid][FF3_PART]; dzb: P floats of scratch (the per-point bound of |dz3| that scales du2)
int ff_bwd_split_launch(const rpde_ff_params* p, const float* const* ds, const float* z_last, const float* grad_out,
                        const float* x, float* dz3, float* du2, float* dzb, float* gx, float* slabs, float* gw1, float* part,
                        int* grid_out, long P, void* fimg, hipStream_t st, FoldJobs* folds);

}  // namespace rpde
