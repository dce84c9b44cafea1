// Counter-based dropout masks: the one definition every mask producer uses (the GEMM prologues and epilogue, the
// FeedForward tail kernels, the fused FeedForward kernels) and that a plain C++ compiler can also build, so that the
// masks can be restated off the device (oracle/dropout_mask.py, tests/test_oracle_dropout_cpu.py).
//
// element id = point * ld + feature, so the forward staging, the backward epilogue and the weight-gradient staging
// regenerate the same mask without storing it.  Groups of four consecutive ids share one base word; each 32-bit
// avalanche hash (two multiplies) yields two 16-bit uniforms.  An element is dropped when its uniform is below
// thresh = round(p * 65536) clamped to [1, 65535]; a kept element is multiplied by 1 / (1 - thresh / 65536).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RPDE_HD __host__ __device__
#define RPDE_HD_INLINE __host__ __device__ __forceinline__
#else
#define RPDE_HD
#define RPDE_HD_INLINE inline
#endif

namespace rpde {

RPDE_HD_INLINE uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

struct DropCfg {
  uint64_t seed;
  uint32_t thresh;   // drop when 16-bit uniform < thresh
  float scale;       // 1/(1-thresh/65536)
  // optional device counter mixed into the seed by the KERNEL (drop_resolve): a captured hipGraph replays its launch
  // arguments, so a seed drawn on the host would freeze the masks -- the training step advances this counter on the
  // device instead (rpde.ops.drop_epoch, rpde/graph.py); forward and backward of one step see the same value
  const uint64_t* epoch;
  RPDE_HD bool on() const { return thresh != 0; }
};

inline DropCfg make_drop(float p, uint64_t seed, const uint64_t* epoch = nullptr) {
  DropCfg d;
  d.seed = seed;
  d.epoch = epoch;
  if (p <= 0.f) { d.thresh = 0; d.scale = 1.f; d.epoch = nullptr; return d; }
  double t = (double)p * 65536.0;
  d.thresh = (uint32_t)(t + 0.5);
  if (d.thresh > 65535u) d.thresh = 65535u;
  if (d.thresh == 0) d.thresh = 1;
  d.scale = (float)(1.0 / (1.0 - (double)d.thresh / 65536.0));
  return d;
}

// the seed of layer l of a FeedForward whose call drew `seed` (splitmix64 finaliser of seed + (l + 1) * golden ratio)
RPDE_HD_INLINE uint64_t layer_seed(uint64_t seed, int l) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(l + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// once per kernel, before the first mask: the configuration with the device counter folded into the seed
RPDE_HD_INLINE DropCfg drop_resolve(DropCfg d) {
  if (d.epoch) {
    d.seed ^= (*d.epoch) * 0x9E3779B97F4A7C15ull;
    d.epoch = nullptr;
  }
  return d;
}
RPDE_HD_INLINE uint32_t drop_base(const DropCfg& d, uint64_t group) {
  const uint32_t lo = (uint32_t)group, hi = (uint32_t)(group >> 32);
  return (lo ^ (uint32_t)d.seed) + (hi * 0x9E3779B9u ^ (uint32_t)(d.seed >> 32));
}
RPDE_HD_INLINE float drop_scale1(const DropCfg& d, uint64_t id) {
  const uint32_t base = drop_base(d, id >> 2);
  const uint32_t h = mix32((id & 2) ? (base ^ 0x68E31DA4u) : base);
  const uint32_t u = (id & 1) ? (h >> 16) : (h & 0xFFFFu);
  return u < d.thresh ? 0.f : d.scale;
}
// id must be a multiple of 4
RPDE_HD_INLINE void drop_scale4(const DropCfg& d, uint64_t id, float s[4]) {
  const uint32_t base = drop_base(d, id >> 2);
  const uint32_t h0 = mix32(base), h1 = mix32(base ^ 0x68E31DA4u);
  s[0] = (h0 & 0xFFFFu) < d.thresh ? 0.f : d.scale;
  s[1] = (h0 >> 16) < d.thresh ? 0.f : d.scale;
  s[2] = (h1 & 0xFFFFu) < d.thresh ? 0.f : d.scale;
  s[3] = (h1 >> 16) < d.thresh ? 0.f : d.scale;
}

}  // namespace rpde
