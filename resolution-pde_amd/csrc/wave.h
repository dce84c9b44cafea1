// Lane-, wave- and LDS-level device primitives shared by the HIP kernels: cross-lane moves and reductions on the VALU
// (DPP, permlane swaps), the layout helpers of the f16 staging tiles and MFMA fragments, the LDS-only barrier, and the
// LDS / global accesses that are issued as inline asm so that the compiler does not wait for them (DESIGN.md section 3.1;
// the counted vmcnt waits that go with them are in cw.h).  gfx950 (CDNA4, wave64) only.
#pragma once
#include <hip/hip_runtime.h>

namespace rpde {

typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef unsigned u32x2v __attribute__((ext_vector_type(2)));

// ---- reductions over the wave --------------------------------------------------------------------------------
// maximum over the wave of non-negative values, returned in every lane.  Six DPP steps on the VALU (row shifts, then
// the two row broadcasts) and one v_readlane -- __shfl_xor would make six dependent round trips through the LDS crossbar
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_max_step(float v) {
  const int t = __builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xf, false);
  return fmaxf(v, __int_as_float(t));
}
__device__ __forceinline__ float wave_max(float v) {
  v = dpp_max_step<0x111, 0xf>(v);     // row_shr:1
  v = dpp_max_step<0x112, 0xf>(v);     // row_shr:2
  v = dpp_max_step<0x114, 0xf>(v);     // row_shr:4
  v = dpp_max_step<0x118, 0xf>(v);     // row_shr:8   -> lane 15 of each row of 16 holds the row maximum
  v = dpp_max_step<0x142, 0xa>(v);     // row_bcast:15 into rows 1 and 3
  v = dpp_max_step<0x143, 0xc>(v);     // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave maximum
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// sum over the wave, returned in every lane: the same six DPP steps with additions (out-of-row sources read as zero)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add_step(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, true));
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v = dpp_add_step<0x111, 0xf>(v);
  v = dpp_add_step<0x112, 0xf>(v);
  v = dpp_add_step<0x114, 0xf>(v);
  v = dpp_add_step<0x118, 0xf>(v);     // lane 15 of each row: the row's sum
  v = dpp_add_step<0x142, 0xa>(v);     // row_bcast:15 into rows 1 and 3: lane 31 = rows 0+1, lane 63 = rows 2+3 (so far)
  v = dpp_add_step<0x143, 0xc>(v);     // row_bcast:31 into rows 2 and 3: lane 63 = everything
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// ---- reductions over a row of 16 lanes -------------------------------------------------------------------------
// sum over the 16 lanes of a row, valid in lane 15 of the row (the four row shifts of wave_sum_dpp)
__device__ __forceinline__ float row_sum15(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, true));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xf, 0xf, true));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x114, 0xf, 0xf, true));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x118, 0xf, 0xf, true));
  return v;
}

// sum / maximum over the 16 lanes of a row, in every lane (quad butterflies, then the two mirrors)
template <bool MAX>
__device__ __forceinline__ float row_all16(float v) {
#define RPDE_ROW_STEP(CTRL)                                                                               \
  {                                                                                                       \
    const float o_ = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true)); \
    v = MAX ? fmaxf(v, o_) : v + o_;                                                                      \
  }
  RPDE_ROW_STEP(0xB1)      // quad_perm [1,0,3,2]
  RPDE_ROW_STEP(0x4E)      // quad_perm [2,3,0,1]
  RPDE_ROW_STEP(0x141)     // row_half_mirror
  RPDE_ROW_STEP(0x140)     // row_mirror
#undef RPDE_ROW_STEP
  return v;
}

// ---- moves between lanes ---------------------------------------------------------------------------------------
// the value held by lane l ^ 16 / l ^ 32, by gfx950's v_permlane16_swap / v_permlane32_swap (vector ALU: no trip through
// the LDS crossbar as __shfl_xor takes).  swap(v, v) returns {v with its odd rows (upper half) replaced by the even rows
// (lower half), v with its even rows (lower half) replaced by the odd rows (upper half)}: each lane picks the copy in
// which its own position was overwritten by its partner.
__device__ __forceinline__ float lane_xor16(float v) {
  const u32x2v r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float((threadIdx.x & 16) ? r.x : r.y);
}
__device__ __forceinline__ float lane_xor32(float v) {
  const u32x2v r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float((threadIdx.x & 32) ? r.x : r.y);
}

// a and b hold one value per lane; afterwards a's upper half (lane-rows 2, 3) and b's lower half (rows 0, 1) have changed
// places / a's odd lane-rows and b's even lane-rows have changed places
__device__ __forceinline__ void swap_halves(float& a, float& b) {
  const u32x2v r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r.x); b = __uint_as_float(r.y);
}
__device__ __forceinline__ void swap_rows(float& a, float& b) {
  const u32x2v r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r.x); b = __uint_as_float(r.y);
}

// 4 x 4 transpose inside every quad of lanes: afterwards register c of lane p (p = lane & 3) holds what register p of
// lane c held.  Two butterfly stages on DPP quad permutes (lane ^ 1, then lane ^ 2).
template <int CTRL>
__device__ __forceinline__ float quad_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ void quad_transpose(float& v0, float& v1, float& v2, float& v3) {
  const bool b0 = threadIdx.x & 1, b1 = threadIdx.x & 2;
  { const float a = quad_dpp<0xB1>(v0), c = quad_dpp<0xB1>(v1); v1 = b0 ? v1 : a; v0 = b0 ? c : v0; }   // quad_perm [1,0,3,2]
  { const float a = quad_dpp<0xB1>(v2), c = quad_dpp<0xB1>(v3); v3 = b0 ? v3 : a; v2 = b0 ? c : v2; }
  { const float a = quad_dpp<0x4E>(v0), c = quad_dpp<0x4E>(v2); v2 = b1 ? v2 : a; v0 = b1 ? c : v0; }   // quad_perm [2,3,0,1]
  { const float a = quad_dpp<0x4E>(v1), c = quad_dpp<0x4E>(v3); v3 = b1 ? v3 : a; v1 = b1 ? c : v1; }
}

// makes the compiler produce x here, in program order relative to the other volatile asm statements (barriers, waits):
// without it the VALU work between the two phases of the 64 x 64 synthesis kernels (scaling, turn, the y phase's
// multiply-adds) is sunk to the end of the kernel and both phases' 128 accumulators are alive at once (80 spilled
// registers)
__device__ __forceinline__ void pin(float& x) { asm volatile("" : "+v"(x)); }

// ---- layouts ---------------------------------------------------------------------------------------------------
// byte offset of the 8-byte chunk c8 (columns 4 c8 .. 4 c8 + 3) of row k inside one staged piece ([32 rows][64 columns]
// f16, 128-byte rows; rows = points or lines, columns = channels): chunks are XOR-swizzled so that the transposing
// reads (ds_read_b64_tr_b16), which fetch rows 8g+q / 8g+4+q per 16-lane group, spread over all 64 banks
__device__ __forceinline__ int stage_off(int k, int c8) {
  return k * 128 + ((c8 ^ ((((k >> 1) & 1) << 2) | (((k >> 3) & 1) << 3))) << 3);
}
// the transposing reads' side of it: at(piece, tile) is where lane (g, li) reads its share of the 16-column tile `tile`
// (0..3) of the staged piece at `piece` (a pointer or an LDS address) -- row 8 g + q (q = li >> 2) and, 512 bytes on, row
// 8 g + 4 + q, 8-byte chunk li & 3 of the tile; `sw` is the chunk-group XOR of those rows (the same for both)
struct StageTr {
  int sw, row;
  __device__ __forceinline__ StageTr(int g, int li)
      : sw(((li >> 3) & 1) | ((g & 1) << 1)), row((8 * g + (li >> 2)) * 128 + (li & 3) * 8) {}
  template <class P>
  __device__ __forceinline__ P at(P piece, int tile) const { return piece + row + ((tile ^ sw) << 5); }
};

// reduction slot j (0..7) of lane group g -> index inside a 32-deep reduction step, for operands built from two
// accumulator tiles (a 16 x 16 accumulator holds rows 4g..4g+3 in lane group g) or loaded as two 16-byte runs per lane;
// whatever sits on the other side of the product is built in the same order
__device__ __forceinline__ int frag_perm(int g, int j) { return 16 * (j >> 2) + 4 * g + (j & 3); }

// ---- LDS ordering ----------------------------------------------------------------------------------------------
// LDS accesses of one wave to its private staging area: the hardware executes a wave's DS instructions in order;
// this only keeps the compiler from reordering a lane's read above another lane's write
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// workgroup barrier that orders LDS traffic only: __syncthreads() would also wait for every outstanding global load
// (prefetches a step ahead) and store (what a training forward writes), several times per tile
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- LDS accesses and global loads the compiler does not see as such -------------------------------------------
// gfx950 has ONE in-order counter (vmcnt) for loads, stores and LDS-DMA.  With an LDS-DMA in flight the compiler puts
// s_waitcnt vmcnt(0) in front of every ordinary ds_read / ds_write (it cannot tell that the DMA's landing area and the
// area accessed are disjoint; the transposing-read builtin carries no memory operand at all) -- stores included, and
// again after every store in between -- and an ordinary load that is one tile in flight is answered with vmcnt(0) at
// its use, i.e. with a wait for the DMA issued just before.  Issued as asm, none of that happens, and the kernel keeps
// the counters itself:
//   * a wave's DS instructions execute in order, so its later reads see its asm writes without a wait;
//   * the results of asm reads pass through lds_wait as tied operands (what orders their uses behind the wait), ONE
//     statement per wait;
//   * the results of asm global loads are covered by a counted wait of the kernel (cw.h), and the in-flight registers
//     are followed through the ISA by tests/test_isa_pending_loads_cpu.py.
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(unsigned long)(const __attribute__((address_space(3))) char*)p;
}
__device__ __forceinline__ void lds_write_b128(unsigned addr, f32x4v v) {
  asm volatile("ds_write_b128 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_write_b64(unsigned addr, uint2 v) {
  asm volatile("ds_write_b64 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_write_b32(unsigned addr, float v) {
  asm volatile("ds_write_b32 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ f32x4v lds_read_b128(unsigned addr) {
  f32x4v r;
  asm volatile("ds_read_b128 %0, %1" : "=v"(r) : "v"(addr) : "memory");
  return r;
}
template <int OFF>
__device__ __forceinline__ u32x2v lds_read_tr16(unsigned addr) {
  u32x2v r;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
  return r;
}
template <class T>
__device__ __forceinline__ void lds_wait(T& a, T& b) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b)::"memory");
}
template <class T>
__device__ __forceinline__ void lds_wait(T& a, T& b, T& c, T& d) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)::"memory");
}
template <class T>
__device__ __forceinline__ void lds_wait(T (&v)[8]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7])::"memory");
}
__device__ __forceinline__ f32x4v global_load_b128(const float* p) {
  f32x4v v;
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
  return v;
}

}  // namespace rpde
