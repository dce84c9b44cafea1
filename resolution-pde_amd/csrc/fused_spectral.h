// Fused FSpectralConv2d kernels (fused_spectral.hip): entry points used by fspectral.hip and core.hip.
#pragma once
#include <type_traits>

#include "rpde_internal.h"
#include "plan.h"

namespace rpde {

// true when the fused path covers the problem (C = 64, grid sides multiples of 32 up to 256, <= 24 padded modes,
// same mode count on both axes); everything else keeps the GEMM-per-step path of fspectral.hip
bool fused2d_ok(int M, int N, int C, int keff_y, int keff_x);
int h2_build_tables(rpde_plan* p, hipStream_t st);

// ---- operand blocks of the synthesis MFMAs ----
// One operand (a 16-row tile of a table, or 16 channels of a spectrum line) over R = 32 K32 + 8 TG reduction rows is
// stored as K32 "hi" fragments, K32 "lo" fragments (1 KB each: lane l holds rows 32 s + 8 (l >> 4) + j) and NP packed
// tail fragments.  The tail has only TG < 4 real lane groups per 32-deep fragment, so the three h2 terms
// (lo*hi, hi*lo, hi*hi) of each real group are laid side by side along the reduction axis: slot t*TG + q holds, on the
// table side, piece (lo, hi, hi)[t] of group q and on the spectrum side piece (hi, lo, hi)[t]; slot -> fragment
// slot / 4, lane group slot % 4.  One MFMA on a packed fragment then yields all three terms: R = 40 costs 4 MFMAs and
// 3 loads per line instead of 6 and 4.  (A 16-deep MFMA for the tail is not an option: a v_mfma_f32_16x16x16_f16 directly
// behind the v_mfma_f32_16x16x32_f16 it accumulates onto reads a partly written accumulator on gfx950 with ROCm 7.2 --
// h2.h, profiles/r04_mfma_mix.txt.)
__host__ __device__ constexpr int h2_np(int TG) { return (3 * TG + 3) / 4; }
__host__ __device__ constexpr int h2_block_bytes(int K32, int TG) { return (2 * K32 + h2_np(TG)) * 1024; }

// byte offsets inside one block, and its writers.  Every kernel that writes or reads a block goes through this struct:
// the table builder and the three spectrum writers (k_spec_split_h2, k_mix_h2, k_lift_mix), the register and LDS readers
// of the synthesis kernels (Frag).
template <int K32, int TG>
struct H2Block {
  static constexpr int NP = h2_np(TG), NF = 2 * K32 + NP, BYTES = NF * 1024;
  // fragment s of the hi / lo plane, packed tail fragment q; a lane's 16-byte piece sits 16 * lane further on
  __host__ __device__ static constexpr int hi(int s) { return s * 1024; }
  __host__ __device__ static constexpr int lo(int s) { return (K32 + s) * 1024; }
  __host__ __device__ static constexpr int pk(int q) { return (2 * K32 + q) * 1024; }
  // 16-byte piece of column c (a table row / a channel, < 16) in tail slot `slot`
  __device__ static __forceinline__ uint4* tail(char* blk, int slot, int c) {
    return reinterpret_cast<uint4*>(blk + pk(slot / 4) + ((slot & 3) * 16 + c) * 16);
  }
  // the three pieces of tail group q (rows 32 K32 + 8 q ..): (lo, hi, hi) on the table side, (hi, lo, hi) on the
  // spectrum side
  template <bool TABLE>
  __device__ static __forceinline__ void store_tail(char* blk, int q, int c, uint4 hi4, uint4 lo4) {
#pragma unroll
    for (int t = 0; t < 3; ++t) *tail(blk, t * TG + q, c) = t == (TABLE ? 0 : 1) ? lo4 : hi4;
  }
  // slots of the packed fragments that no group uses: zero (the persistent synthesis kernels feed whole fragments to
  // the MFMAs); one call per column c
  __device__ static __forceinline__ void zero_unused(char* blk, int c) {
#pragma unroll
    for (int slot = 3 * TG; slot < 4 * NP; ++slot) *tail(blk, slot, c) = make_uint4(0, 0, 0, 0);
  }
};

// R = 8 .. 48 in steps of 8 -> f(K32, TG) with (K32, TG) = (0,1) (0,2) (0,3) (1,0) (1,1) (1,2) as integral constants.
// UP_TO_40: the caller's kernels exist only up to R = 40 (the persistent synthesis kernels: three fragments per block
// at most) and it has checked that; (1,2) is then not instantiated
template <bool UP_TO_40 = false, class F>
inline void h2_dispatch(int R, F&& f) {
  using std::integral_constant;
  typedef integral_constant<int, 0> I0;
  typedef integral_constant<int, 1> I1;
  switch (R / 8) {
    case 1: f(I0{}, I1{}); break;
    case 2: f(I0{}, integral_constant<int, 2>{}); break;
    case 3: f(I0{}, integral_constant<int, 3>{}); break;
    case 4: f(I1{}, I0{}); break;
    case 5: f(I1{}, I1{}); break;
    default:
      if constexpr (UP_TO_40) f(I1{}, I1{});
      else f(I1{}, integral_constant<int, 2>{});
      break;
  }
}

// B-fragment image of `lines` spectra of R rows x 64 channels
size_t fused2d_img_bytes(long lines, int R);
// spec_y[(b,m)][R][64], spec_x[(b,n)][R][64] = table . lines of x;  adjoint: tables Fs^T instead of Fa
// amax_y / amax_x (may be null): max |spectrum| of every line, for the mode-mix kernel's scaling (fused_mix.hip)
int fused2d_analysis(const float* x, float* spec_y, float* spec_x, float* amax_y, float* amax_x, const rpde_plan* py,
                     const rpde_plan* px, int adjoint, int B, int M, int N, hipStream_t st);
int fused2d_split(const float* spec, void* img, float* inv, long lines, int R, hipStream_t st);
// out = table_y . img_y[row] + table_x . img_x[col] (+ skip);  adjoint: tables Fa^T instead of Fs
int fused2d_synthesis(const void* imgy, const void* imgx, const float* invy, const float* invx, const rpde_plan* py,
                      const rpde_plan* px, int adjoint, float* out, const float* skip, int B, int M, int N, hipStream_t st);

// ---- mode mix in h2 arithmetic (fused_mix.hip) ----
constexpr int MIX_W_BYTES_PER_MODE = 4 * 2 * 2 * 2 * 1024;      // [cb 4][Wr|Wi][ks 2][hi|lo] fragments of 1 KB
size_t mix_wimg_bytes(int kp);
// weights of both axes -> fragment image + wc[2][kp][2] = {1 / scale, norm}; conj_t: W^H (the adjoint's operand)
int mix_prep(const float* w_y, const float* w_x, int K, int keff, int kp, int conj_t, void* wimg, float* wc, hipStream_t st);
// weight gradients of the mix, both axes: two launches (slabs of lines, then a fixed-order fold); amax_*: line maxima of the
// saved spectra / of the gradient spectra; slabs: mix_wgrad_slab_floats(kp, S) floats of workspace
size_t mix_wgrad_slab_floats(int kp, int S);
int mix_wgrad_h2(const float* spec_y, const float* spec_x, const float* gspec_y, const float* gspec_x, const float* amax_sy,
                 const float* amax_sx, const float* amax_gy, const float* amax_gx, float* gw_y, float* gw_x, long lines_y,
                 long lines_x, int K, int keff, int kp, float* slabs, int S, hipStream_t st);
int mix_h2(const float* spec_y, const float* spec_x, const float* amax_y, const float* amax_x, void* img_y, void* img_x,
           float* inv_y, float* inv_x, long lines_y, long lines_x, int kp, const void* wimg, const float* wc, hipStream_t st);

}  // namespace rpde
