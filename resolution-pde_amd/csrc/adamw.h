// The AdamW update of one element and the step state's arithmetic, shared by the translation units that build
// kernels around them: adamw.hip (the plain step) and adamw_clip.hip (the step behind a gradient-norm record).
#pragma once
#include "rpde_internal.h"

namespace rpde {

struct AdamwScalars { float omlw, omb1, b2, omb2, step_size, bc2_sqrt, eps; };

__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, const AdamwScalars& s) {
  p *= s.omlw;
  m = fmaf(g - m, s.omb1, m);
  v = fmaf(s.omb2 * g, g, v * s.b2);
  const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
  p = fmaf(-s.step_size, m / denom, p);
}

// device-side step state (hipGraph-capturable steps): dev[0] = step (incremented here), dev[1] = lr / (1 - b1^t),
// dev[2] = sqrt(1 - b2^t), dev[3] = lr, dev[4] = weight decay, dev[5] = 1 - lr * wd.  lr and wd live on the device so
// that a captured step follows a learning-rate schedule: a replay repeats its launch ARGUMENTS, but reads these words
__device__ __forceinline__ void adamw_tick(float* dev, float b1, float b2) {
  const double t = (double)dev[0] + 1.0, lr = (double)dev[3];
  dev[0] = (float)t;
  dev[1] = (float)(lr / (1.0 - pow((double)b1, t)));
  dev[2] = (float)sqrt(1.0 - pow((double)b2, t));
  dev[5] = (float)(1.0 - lr * (double)dev[4]);
}

inline bool capturing(hipStream_t st) {
  hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &status) != hipSuccess) { (void)hipGetLastError(); return false; }
  return status != hipStreamCaptureStatusNone;
}

inline int adamw_grid(long n4) {
  long g = (n4 + 255) / 256;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace rpde
