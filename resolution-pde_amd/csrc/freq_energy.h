// Per-frequency energy of (prediction - target) and of the target (freq_energy.hip)
#pragma once
#include "rpde_internal.h"

namespace rpde {
// samples of a [images, H, W] batch that one pass of the 2-D evaluator takes through its workspace: the two
// half-spectra of a chunk (2 * 2H * (W/2+1) floats per image) stay under FE_SPEC_BYTES, a whole number of 16-row
// tiles when it is more than one
constexpr size_t FE_SPEC_BYTES = 16u << 20;
int fe_chunk_images(long images, int H, int W);
}  // namespace rpde
