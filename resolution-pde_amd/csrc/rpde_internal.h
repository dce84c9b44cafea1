// Internal helpers shared by the HIP translation units of librpde_hip.so.
// gfx950 (CDNA4, wave64) only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <string>

#include "rpde.h"
// counter-based dropout: mix32, DropCfg, make_drop, layer_seed, drop_resolve, drop_scale1/4 (namespace rpde)
#include "drop_hash.h"

namespace rpde {

void set_error(const char* fmt, ...);

#define RPDE_CHECK_ARG(cond, ...)                       \
  do {                                                  \
    if (!(cond)) {                                      \
      ::rpde::set_error(__VA_ARGS__);                   \
      return RPDE_ERR_ARG;                              \
    }                                                   \
  } while (0)

#define RPDE_HIP(call)                                                              \
  do {                                                                              \
    hipError_t e_ = (call);                                                         \
    if (e_ != hipSuccess) {                                                         \
      ::rpde::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),      \
                        __FILE__, __LINE__);                                        \
      return RPDE_ERR_HIP;                                                          \
    }                                                                               \
  } while (0)

#define RPDE_LAUNCH_CHECK() RPDE_HIP(hipGetLastError())

#define RPDE_TRY(call)               \
  do {                               \
    int s_ = (call);                 \
    if (s_ != RPDE_OK) return s_;    \
  } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// ---- host helpers ----------------------------------------------------------
// 16-byte aligned: what the 16-byte loads and stores of the vectorised kernels need
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// v rounded up to a multiple of 4 (mode counts and leading dimensions are padded to whole float4s)
inline int r4(int v) { return (v + 3) / 4 * 4; }
// compute units of the current device, for the grids of the persistent kernels; 256 (an MI355X) is left in *cus when
// the query fails, for the callers that go on regardless
inline hipError_t cu_count(int* cus) {
  int dev = 0;
  *cus = 256;
  const hipError_t e = hipGetDevice(&dev);
  return e != hipSuccess ? e : hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev);
}
// whether the environment switch `name` (RPDE_X, default on) is set to 0.  Reads the environment at every call:
// tests and A/B runs flip switches inside one process
inline bool switch_off(const char* name) {
  const char* e = getenv(name);
  return e && e[0] == '0';
}

// ---- device math -----------------------------------------------------------
// Phi(x) and the normal density phi(x) from ONE exponential and one reciprocal (Abramowitz & Stegun 26.2.17, the
// normal-distribution form of 7.1.26):  1 - Phi(|x|) = phi(x) (b1 s + ... + b5 s^5),  s = 1 / (1 + 0.2316419 |x|).
// About 14 VALU instructions for Phi, 3 more for GELU and GELU' together, instead of the device library's erff
// (~100).  Measured in fp32 against scipy over [-9, 9]: |Phi error| <= 3.0e-7, |gelu error| <= 4.2e-7,
// |gelu' error| <= 3.1e-7 (parity budget of the hot path: 1e-5).  On the MI355X itself, against float64 on 4e6 points of
// [-14, 14] (tests/test_gpu_pointwise.py, which pins 1.5 x these bounds): max |gelu error| 4.21e-7 at x = 3.07496,
// max |gelu' error| 2.76e-7 at x = 0.25471; beyond |x| = 9 gelu is exactly x or below 1e-12, gelu' 1 or 0.
// gk = exp(-x^2/2) / sqrt(2 pi) = the normal density (the 1/sqrt(2 pi) rides in the exponent: exp2(-x^2 c + log2 k)),
// and the polynomial coefficients carry sqrt(2 pi) / 2 so that half = (p s) gk = 0.5 erfc(|x| / sqrt 2)
__device__ __forceinline__ void phi_parts(float x, float& cdf, float& gk) {
  const float s = __builtin_amdgcn_rcpf(fmaf(0.2316418882f, fabsf(x), 1.0f));
  gk = __builtin_amdgcn_exp2f(fmaf(x * x, -0.72134752044f, -1.32574806473f));
  float p = fmaf(1.330274429f, s, -1.821255978f);
  p = fmaf(p, s, 1.781477937f);
  p = fmaf(p, s, -0.356563782f);
  p = fmaf(p, s, 0.319381530f);
  const float half = (p * s) * gk;
  cdf = x < 0.f ? half : 1.0f - half;
}
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float norm_cdf_f(float x) {
  float c, g;
  phi_parts(x, c, g);
  return c;
}
__device__ __forceinline__ float gelu_f(float u) { return u * norm_cdf_f(u); }
__device__ __forceinline__ float dgelu_f(float u) {
  float c, gk;
  phi_parts(u, c, gk);
  return fmaf(u, gk, c);
}
// h = act(u), d = act'(u) in one evaluation
__device__ __forceinline__ void act_both(int act, float u, float& h, float& d) {
  if (act == RPDE_ACT_GELU) {
    float c, gk;
    phi_parts(u, c, gk);
    h = u * c;
    d = fmaf(u, gk, c);
  } else if (act == RPDE_ACT_RELU) {
    h = u > 0.f ? u : 0.f;
    d = u > 0.f ? 1.f : 0.f;
  } else {
    h = u;
    d = 1.f;
  }
}
__device__ __forceinline__ float act_f(int act, float u) {
  if (act == RPDE_ACT_GELU) return gelu_f(u);
  if (act == RPDE_ACT_RELU) return u > 0.f ? u : 0.f;
  return u;
}
__device__ __forceinline__ float dact_f(int act, float u) {
  if (act == RPDE_ACT_GELU) return dgelu_f(u);
  if (act == RPDE_ACT_RELU) return u > 0.f ? 1.f : 0.f;
  return 1.f;
}

// ---- wave / block reductions -----------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

int launch_gemm(const rpde_gemm_desc& d, hipStream_t stream);
// pre-split operands of the split-bf16 GEMM (gemm_bf16x3.hip)
int split_npad(int N);
size_t split_bytes(int N, int K);
int split_weights(const float* w, int kmajor, long ld, int N, int K, void* out, hipStream_t st);
struct SplitJobs {
  static constexpr int MAX = 4;
  int n = 0;
  struct Job { const float* w; char* out; long ld; int kmajor, N, K, blk0; } j[MAX];
  void add(const float* w, int kmajor, long ld, int N, int K, void* out) {
    j[n].w = w; j[n].out = static_cast<char*>(out); j[n].ld = ld; j[n].kmajor = kmajor; j[n].N = N; j[n].K = K; j[n].blk0 = 0;
    ++n;
  }
};
int split_weights_multi(SplitJobs& J, hipStream_t st);

inline rpde_gemm_desc gemm_desc() {
  rpde_gemm_desc d;
  memset(&d, 0, sizeof(d));
  d.batch = 1; d.zdiv = 1; d.ksplit = 1; d.alpha = 1.f;
  d.a_kmajor = 1; d.b_kmajor = 1;
  return d;
}

}  // namespace rpde
