// fp32 products on the f16 matrix pipe by two-piece splitting ("h2" arithmetic), shared by the fused kernels.
//
//   a * 2^ea = ah + al + O(2^-22 |a 2^ea|),   ah = f16(a 2^ea),  al = f16(a 2^ea - ah)         (11 + 11 significant bits)
//   a b = 2^-(ea+eb) (ah bh + ah bl + al bh) + O(2^-22 |a b|)        -- three v_mfma_f32_16x16x32_f16, fp32 accumulate
//
// f16 has a 5-bit exponent, so every operand block carries a power-of-two scale chosen from the block's own maximum
// (|max| -> [2^14, 2^15)): multiplying by it is exact, the low piece keeps 2^-24 absolute resolution in scaled units
// (2^-39 of the block maximum), and the product of the scales is undone on the fp32 accumulator.  Per product the
// error is <= 3 * 2^-22 (representation of a, of b, and the dropped al*bl), rms ~1.5e-7: fp32-GEMM class accuracy
// with half the matrix instructions of the three-piece bf16 split (gemm_bf16x3.hip), which stays the generic path.
#pragma once
#include "rpde_internal.h"
#include "wave.h"

namespace rpde {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4v __attribute__((ext_vector_type(4)));

constexpr int H2_TABLE_EXP = 12;     // DFT tables (|entry| <= 2/sqrt(n) <= 1) are stored times 2^12

// power-of-two scale for a block whose largest magnitude is m (any finite float, 0 allowed):
// scale = 2^(141 - E) puts m into [2^14, 2^15); inv = 2^(E - 141 - extra) undoes it together with `extra` more
// binary places (the table scale).  E is clamped so that both stay normal numbers.
__device__ __forceinline__ void h2_scale(float m, int extra, float& scale, float& inv) {
  int E = (int)(__float_as_uint(m) >> 23) & 0xff;
  E = max(E, 15 + extra);
  scale = __uint_as_float((unsigned)(268 - E) << 23);
  inv = __uint_as_float((unsigned)(E - 14 - extra) << 23);
}

// four scaled floats -> hi / lo f16 pieces (round to nearest both times)
__device__ __forceinline__ void h2_split4(float a, float b, float c, float d, uint2& hi, uint2& lo) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  union { f16x4 v; uint2 u; } h, l;
  h.v = __builtin_convertvector((f4){a, b, c, d}, f16x4);
  const f4 hf = __builtin_convertvector(h.v, f4);
  l.v = __builtin_convertvector((f4){a - hf.x, b - hf.y, c - hf.z, d - hf.w}, f16x4);
  hi = h.u; lo = l.u;
}

// eight scaled floats of a lane (the eight reduction slots it supplies to a 32-deep MFMA) -> the 16-byte hi and lo
// pieces of one fragment
__device__ __forceinline__ void h2_split8(const float (&v)[8], uint4& hi, uint4& lo) {
  uint2 h0, l0, h1, l1;
  h2_split4(v[0], v[1], v[2], v[3], h0, l0);
  h2_split4(v[4], v[5], v[6], v[7], h1, l1);
  hi = make_uint4(h0.x, h0.y, h1.x, h1.y);
  lo = make_uint4(l0.x, l0.y, l1.x, l1.y);
}
// ... stored as one fragment in memory or LDS: lane l's hi piece at dst (= fragment base + 16 l), its lo piece 1 KB on
__device__ __forceinline__ void h2_put_frag(char* dst, const float (&v)[8]) {
  uint4 hi, lo;
  h2_split8(v, hi, lo);
  *reinterpret_cast<uint4*>(dst) = hi;
  *reinterpret_cast<uint4*>(dst + 1024) = lo;
}
// ... as a pair of MFMA operands in registers
__device__ __forceinline__ void h2_frag(const float (&v)[8], f16x8& hi, f16x8& lo) {
  union { f16x8 v; struct { uint2 a, b; } u; } H, L;
  h2_split4(v[0], v[1], v[2], v[3], H.u.a, L.u.a);
  h2_split4(v[4], v[5], v[6], v[7], H.u.b, L.u.b);
  hi = H.v; lo = L.v;
}

// three-term product of split operands, small terms first
__device__ __forceinline__ f32x4v h2_mfma32(f16x8 ah, f16x8 al, f16x8 bh, f16x8 bl, f32x4v c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, c, 0, 0, 0);
}
// (There is deliberately no 16-deep variant on v_mfma_f32_16x16x16_f16.  Round 2 saw wrong accumulators when the fused
//  synthesis kernel closed a 32-deep chain with a 16-deep tail; round 4 reduced it to two instructions
//  (profiles/ubench/mfma_mix.hip, output + disassembly in profiles/r04_mfma_mix.txt): ROCm 7.2 emits
//  `v_mfma_f32_16x16x32_f16 v[0:3], ..` and the dependent `v_mfma_f32_16x16x16_f16 v[0:3], .., v[0:3]` back to back and
//  half of the result is wrong; with s_nop padding between them, or in the order 16-deep -> 32-deep, it is exact.  The
//  shorter instruction reads its SrcC before the longer one has written all of it, and neither the hardware nor the
//  compiler's hazard recognizer waits for this opcode pair.  Same-shape chains are handled.  Short reduction tails are
//  therefore packed into 32-deep fragments -- fused_spectral.h, H2Block -- which also costs no padding.)

}  // namespace rpde
