// Device pieces of the streaming weight gradient gW += A^T . B over panels of 32 points, shared by k_wgrad_h2
// (wgrad_h2.hip) and the first-layer consumer inside k_ffs_layer1 (ff_bwd_split.hip).
//
// A panel is [hi | lo][32 points][64 channels] f16 in the stage_off layout (wave.h), scaled by the power of two of a
// RUNNING exponent: the largest biased exponent its writer has seen so far (start 15, capped at 254).  Accumulators are
// expressed in the exponents of the panels they were fed from; when one moves, the accumulators are rescaled once, and
// the slab write-out undoes the two exponents.  Which wave loads, converts or consumes what, and when, stays with the
// kernel.
#pragma once
#include "h2.h"

namespace rpde {

constexpr int WG_PANEL = 8192;                 // bytes per panel: [hi | lo][32 points][64 channels] f16

// ---- running exponent -> scale: m = the new values' maximum; the running maximum goes to [2^14, 2^15) ----
__device__ __forceinline__ float panel_run_scale(int& e_run, float m) {
  e_run = max(e_run, (int)(__float_as_uint(m) >> 23) & 0xff);
  e_run = min(e_run, 254);
  return __uint_as_float((unsigned)(268 - e_run) << 23);
}

// ---- panel writer: channels 4 c8 .. 4 c8 + 3 of point `row`, scaled and split ----
__device__ __forceinline__ void panel_put4(char* panel, int row, int c8, float a, float b, float c, float d, float scale) {
  uint2 hi, lo;
  h2_split4(a * scale, b * scale, c * scale, d * scale, hi, lo);
  const int off = stage_off(row, c8);
  *reinterpret_cast<uint2*>(panel + off) = hi;
  *reinterpret_cast<uint2*>(panel + 4096 + off) = lo;
}

// ---- transposing fragment reader: 16-channel tile `tile` of a panel as an MFMA operand whose k is the point ----
__device__ __forceinline__ void panel_frag_tr(const char* panel, const StageTr& lane, int tile, f16x8& hi, f16x8& lo) {
  typedef s16x4v __attribute__((address_space(3))) * lds_tr;
  const char* t = lane.at(panel, tile);
  union { struct { s16x4v a, b; } h; f16x8 v; } uh, ul;
  uh.h.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr)(t));
  uh.h.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr)(t + 512));
  ul.h.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr)(t + 4096));
  ul.h.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr)(t + 4096 + 512));
  hi = uh.v; lo = ul.v;
}

// ---- accumulator rescale when a running maximum moved ----
// ea_used / eb_used: the exponents the accumulators fed from an A panel (and the B panel) are expressed in; ea / eb: the
// exponents of the panels about to be consumed (wave-uniform).  ea_used becomes ea; where the sum moved (rare: a new
// running maximum) the result is true and the accumulators are to be multiplied by f = 2^(old - new) (0 below the normal
// range).  The caller sets eb_used = eb behind its last A panel.
__device__ __forceinline__ bool panel_exp_moved(int& ea_used, int eb_used, int ea, int eb, float& f) {
  const bool moved = ea + eb != ea_used + eb_used;
  const int d = (ea_used + eb_used) - (ea + eb);                       // <= 0
  f = d > -126 ? __uint_as_float((unsigned)(127 + d) << 23) : 0.f;
  ea_used = ea;
  return moved;
}

// ---- what undoes the scale of a panel written under running exponent e_used (the data gradient's partial products;
// the slab write-out multiplies by the same two factors, written out in both kernels) ----
__device__ __forceinline__ float panel_exp_factor(int e_used) { return __uint_as_float((unsigned)(e_used - 14) << 23); }

// ---- W -> B fragments in LDS for the data gradient gx = gy . W, under ONE power-of-two scale; returns its inverse ----
// w: [32 KS][ldw] (rows = the layer's output channels = k, columns 0..63 = input channels = n); wfrag: [KS k-step]
// [4 n-tile][hi | lo][64 lanes][16 B]; wmax: THREADS / 64 floats of LDS.  Called by all THREADS threads (it holds a
// __syncthreads()); the fragments are visible behind the caller's next barrier.
template <int KS, int THREADS>
__device__ __forceinline__ float panel_stage_w(const float* __restrict__ w, int ldw, char* wfrag, float* wmax, int tid) {
  constexpr int NF = KS * 4 * 64 / THREADS;                   // (k-step, n-tile, lane) triples per thread
  float wv[NF][8];
  float m = 0.f;
#pragma unroll
  for (int r = 0; r < NF; ++r) {
    const int c = tid + r * THREADS, fl = c & 63, nt = (c >> 6) & 3, ks = c >> 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      wv[r][j] = w[(long)(32 * ks + 8 * (fl >> 4) + j) * ldw + 16 * nt + (fl & 15)];
      m = fmaxf(m, fabsf(wv[r][j]));
    }
  }
  m = wave_max(m);
  if ((tid & 63) == 0) wmax[tid >> 6] = m;
  __syncthreads();
  m = 0.f;
#pragma unroll
  for (int i = 0; i < THREADS / 64; ++i) m = fmaxf(m, wmax[i]);
  float w_scale, w_inv;
  h2_scale(m, 0, w_scale, w_inv);
#pragma unroll
  for (int r = 0; r < NF; ++r) {
    const int c = tid + r * THREADS, fl = c & 63, nt = (c >> 6) & 3, ks = c >> 8;
    const float sv[8] = {wv[r][0] * w_scale, wv[r][1] * w_scale, wv[r][2] * w_scale, wv[r][3] * w_scale,
                         wv[r][4] * w_scale, wv[r][5] * w_scale, wv[r][6] * w_scale, wv[r][7] * w_scale};
    h2_put_frag(wfrag + (ks * 4 + nt) * 2048 + fl * 16, sv);
  }
  return w_inv;
}

}  // namespace rpde
