// Backward of the fused FeedForward 64 -> 256 -> 256 -> 64 with the data-gradient chain of ff_fused.hip cut at du2:
//
//   k_ffs_adjoint   g, z3, d2  ->  dz3, du2 = (W3^T dz3) * d2            (and db2, db3, dgamma, dbeta)
//   k_ffs_layer1    du2, d1, x ->  gx = du1 . W1,  gW1 = du1^T . x        (and db1),  du1 = (W2^T du2) * d1
//
// du1 (1 KB per point) is formed and consumed inside one workgroup and never goes to HBM: k_ff3_bwd_h2 wrote it and
// k_wgrad_h2<.., DG> read it back.  The two upper weight gradients run on dz3 and du2 as before.
//
// Both kernels keep the chain's form -- transposed products, wave w owns hidden rows 32w .. 32w+31 of W3^T / W2^T as
// register fragments (the image of k_ff3_prep_bwd), one scale per point derived from the bound of its |dz3| -- and its
// tile order (tile = workgroup, workgroup + grid, ..), and they sum the small gradients in the chain's order, so dz3,
// du2, du1 and the five small gradients have the chain's bits: both call the functions of ff3_bwd.h for them.  Everything
// else is the plain style of wgrad_h2.hip: loads through registers one tile ahead, waits left to the compiler,
// lds_barrier().
//
// k_ffs_layer1 then hands du1 to the first layer's weight-gradient consumer through LDS, on the pieces of wgrad_panel.h
// that k_wgrad_h2 is built from: each wave writes its 32 channels of the tile as half a [hi | lo][32 points][64 channels]
// panel under a running exponent of its own, x is staged the same way under one running exponent the eight waves agree
// on, and the consumer has the wave tiling of k_wgrad_h2<4, 1, 4, 2, 4, 2, false, true>: gW1 += du1^T . x by transposing
// reads, gx = du1 . W1 against ready-made W1 fragments in LDS.
#include "ff_bwd_split.h"
#include "ff3_bwd.h"
#include "h2.h"
#include "pointwise.h"
#include "wgrad_h2.h"
#include "wgrad_panel.h"

namespace rpde {

constexpr int FS_WAVES = 8;
constexpr int FS_MAX_GRID = 256;               // the slab region of the first layer (wgrad_h2_slab_floats) holds 256
struct FsA {
  const float* g; const float* z3; const float* d2;
  float* dz3; float* du2; float* dzb;
  const char* wimg; const float* consts;
  const float* gamma; const float* beta;
  float* part;
  long P; int layer_norm; float eps; int post_act;
  DropCfg drop2;
  int ntiles;
};

constexpr int FA_DZBUF = 0;                        // [2 parity][2 blk][2 ks][hi|lo][1 KB]: dz3 as B fragments   = 16 KB
constexpr int FA_VEC = FA_DZBUF + 16384;           // gamma[64] beta[64]
constexpr int FA_ACC = FA_VEC + 512;               // db2[256] | db3, dgamma, dbeta: [3][8 wave][64]             =  7 KB
constexpr int FA_INFO = FA_ACC + 7168;             // [2 parity][32 points] bound of |dz3|
constexpr int FA_LDS = FA_INFO + 256;

__global__ __launch_bounds__(64 * FS_WAVES, 2) void k_ffs_adjoint(const FsA A0) {
  __shared__ __attribute__((aligned(16))) char smem[FA_LDS];
  FsA A = A0;
  A.drop2 = drop_resolve(A0.drop2);
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, g = l >> 4, li = l & 15;
  f16x8 w3h[2][2], w3l[2][2];
  {
    const char* base = ff3_img_lane(A.wimg, w, l);
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      w3h[f >> 1][f & 1] = ff3_img_frag(base, f, 0);
      w3l[f >> 1][f & 1] = ff3_img_frag(base, f, 1);
    }
    ff3_bwd_stage_vec<64 * FS_WAVES>(reinterpret_cast<float*>(smem + FA_VEC), A.gamma, A.beta, reinterpret_cast<float*>(smem + FA_ACC), 1792, tid);
  }
  const float* const vec = reinterpret_cast<const float*>(smem + FA_VEC);
  float* const acc_db2 = reinterpret_cast<float*>(smem + FA_ACC);
  float* const acc_db3 = acc_db2 + 256;        // [8 wave][64]
  float* const acc_dg = acc_db2 + 768;         // [8 wave][64]
  float* const acc_dbt = acc_db2 + 1280;       // [8 wave][64]
  float* const info = reinterpret_cast<float*>(smem + FA_INFO);
  const float winv3 = A.consts[2];
  // the last-layer adjoint works on one POINT per 16-lane row (point 4 w + q3 of the tile), lane li on features 4 li ..
  const int q3 = l >> 4, feat = 4 * li;

  float4 g4n = make_float4(0.f, 0.f, 0.f, 0.f), z4n = g4n, d2n[4];
  auto issue = [&](int tile) {
    const long p = min((long)tile * 32 + 4 * w + q3, A.P - 1);
    g4n = *reinterpret_cast<const float4*>(A.g + p * 64 + feat);
    z4n = *reinterpret_cast<const float4*>(A.z3 + p * 64 + feat);
    // d2 of the wave's hidden rows, in accumulator layout: point 16 blk + li, rows 16 (2 w + t) + 4 g ..
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
      for (int t = 0; t < 2; ++t)
        d2n[blk * 2 + t] = *reinterpret_cast<const float4*>(A.d2 + min((long)tile * 32 + 16 * blk + li, A.P - 1) * 256 + 16 * (2 * w + t) + 4 * g);
  };
#pragma unroll
  for (int i = 0; i < 4; ++i) d2n[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  if ((int)blockIdx.x < A.ntiles) issue(blockIdx.x);
  lds_barrier();                               // vectors and zeroed accumulators are in LDS

  int par = 0;
  for (int tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x, par ^= 1) {
    const int next_tile = tile + gridDim.x;
    const long p0 = (long)tile * 32;
    const int ptl = 4 * w + q3;
    const long pt3 = p0 + ptl;
    const bool live3 = pt3 < A.P;
    const long off3 = min(pt3, A.P - 1) * 64 + feat;
    const float4 g4 = g4n, z4 = z4n;
    float4 dq[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) dq[i] = d2n[i];
    if (next_tile < A.ntiles) issue(next_tile);

    // ---- last-layer adjoint: dropout, LayerNorm, post-activation ----
    float dz[4], dzb, dgm[4], dbt[4];
    ff3_last_adjoint(A, g4, z4, pt3, live3, feat, [&](float (&gmv)[4], float (&btv)[4]) {
      const float4 gm = *reinterpret_cast<const float4*>(vec + feat);
      const float4 bt = *reinterpret_cast<const float4*>(vec + 64 + feat);
      gmv[0] = gm.x; gmv[1] = gm.y; gmv[2] = gm.z; gmv[3] = gm.w;
      btv[0] = bt.x; btv[1] = bt.y; btv[2] = bt.z; btv[3] = bt.w;
    }, dz, dzb, dgm, dbt);
    if (live3) *reinterpret_cast<float4*>(A.dz3 + off3) = make_float4(dz[0], dz[1], dz[2], dz[3]);
    // bias / gamma / beta gradients: sum over the wave's four points, one writer per (wave, feature)
    {
      float b[4];
      ff3_rows_sum(live3, A.layer_norm, dz, b, dgm, dbt);
      if (q3 == 0) {
        float4* a3 = reinterpret_cast<float4*>(acc_db3 + w * 64 + feat);
        float4 v3 = *a3;
        v3.x += b[0]; v3.y += b[1]; v3.z += b[2]; v3.w += b[3];
        *a3 = v3;
        if (A.layer_norm) {
          float4* ag = reinterpret_cast<float4*>(acc_dg + w * 64 + feat);
          float4* ab = reinterpret_cast<float4*>(acc_dbt + w * 64 + feat);
          float4 vg = *ag, vb = *ab;
          vg.x += dgm[0]; vg.y += dgm[1]; vg.z += dgm[2]; vg.w += dgm[3];
          vb.x += dbt[0]; vb.y += dbt[1]; vb.z += dbt[2]; vb.w += dbt[3];
          *ag = vg;
          *ab = vb;
        }
      }
    }
    // dz3 -> B fragments, one scale per point (its bound), in the layout of ff3_dz_off
    {
      uint2 hi, lo;
      ff3_dz_split(dz, dzb, hi, lo);
      char* dst = smem + FA_DZBUF + par * 8192 + ff3_dz_off(ptl, li);
      *reinterpret_cast<uint2*>(dst) = hi;
      *reinterpret_cast<uint2*>(dst + 1024) = lo;
      if (li == 0) {
        info[par * 32 + ptl] = dzb;
        if (live3) A.dzb[pt3] = dzb;             // k_ffs_layer1 scales du2 by the bound derived from it
      }
    }
    // (the fragments and bounds are double-buffered by tile parity: a wave writes those of tile i + 2 only behind the
    //  barrier of tile i + 1, which every wave reaches after its reads of tile i -- one barrier per tile)
    lds_barrier();

    // ---- du2 = (W3^T dz3) * d2: this wave's 32 hidden rows ----
    float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      f16x8 zh0, zl0, zh1, zl1;
      ff3_dz_frags(smem + FA_DZBUF + par * 8192, blk, l, zh0, zl0, zh1, zl1);
      const long pt = p0 + 16 * blk + li;
      const float inv_a = ff3_inv_dz3(info[par * 32 + blk * 16 + li], winv3);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x4v acc = {0.f, 0.f, 0.f, 0.f};
        acc = h2_mfma32(w3h[t][0], w3l[t][0], zh0, zl0, acc);
        acc = h2_mfma32(w3h[t][1], w3l[t][1], zh1, zl1, acc);
        const int hid = 16 * (2 * w + t) + 4 * g;
        float u[4];
        ff3_du_tile<false>(acc, inv_a, dq[blk * 2 + t], pt < A.P, A.du2 + pt * 256 + hid, u, bsum + 4 * t);
      }
    }
    ff3_bias_rows(bsum);
    if (li == 15)
#pragma unroll
      for (int i = 0; i < 8; ++i) acc_db2[ff3_bias_row(w, g, i)] += bsum[i];
  }
  // ---- per-workgroup sums out: db2 | db3 | dgamma | dbeta of FF3_PART (db1 comes from k_ffs_layer1) ----
  lds_barrier();
  ff3_part_out<256, FF3_PART, 64 * FS_WAVES>(A.part + (long)blockIdx.x * FF3_PART, acc_db2, acc_db3, tid);
}

// ====================================================================================================================
struct FsB {
  const float* du2; const float* d1; const float* x; const float* dzb; const float* w1;
  float* gx; float* slabs; float* part;
  const char* wimg; const float* consts;
  long P; float dmax; int ntiles;
};

constexpr int FL_PANEL = WG_PANEL;                 // [hi | lo][32 points][64 channels] f16
constexpr int FL_DUBUF = 0;                        // [2 blk][8 kappa][hi|lo][1 KB]: du2 as B fragments           = 32 KB
constexpr int FL_PAN = FL_DUBUF + 32768;           // four du1 panels                                              = 32 KB
constexpr int FL_X = FL_PAN + 4 * FL_PANEL;        // the x panel                                                  =  8 KB
constexpr int FL_W1 = FL_X + FL_PANEL;             // [8 k-step][4 n-tile][hi | lo][64 lanes][16 B]: W1            = 64 KB
constexpr int FL_W2L = FL_W1 + 65536;             // [8 wave][2 t][64 lanes][16 B]: the lo pieces of W2^T's last k-step  = 16 KB
constexpr int FL_LDS = FL_W2L + 16384;
#ifdef RPDE_STAMPS
// debug build: lane 0 of waves 0, 3 and 6 of workgroup 100 records s_memtime around the phases of tiles 5 .. 12
__device__ unsigned long long g_flstamps[3 * 64];
#define FLSTAMP(i) do { if (stamp_on && stamp_t >= 0 && stamp_t < 8) g_flstamps[stamp_w * 64 + stamp_t * 8 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define FLSTAMP(i) do { } while (0)
#endif
constexpr int FL_PARKED = 7;                       // .. fragments (t, kappa = 7): read back at their uses, 8 VGPRs fewer

__global__ __launch_bounds__(64 * FS_WAVES, 2) void k_ffs_layer1(const FsB A) {
  __shared__ __attribute__((aligned(16))) char smem[FL_LDS];
  __shared__ int einfo[FS_WAVES];                 // running exponent of each wave's half panel of du1
  __shared__ float xmax[FS_WAVES];
  __shared__ float wmax[FS_WAVES];
  __shared__ float acc_db1[256];
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, g = l >> 4, li = l & 15;
  // ---- W2^T rows 32w .. 32w+31 -> registers; W1 -> LDS as B fragments (k = hidden channel, n = input channel) ----
  // (two of the sixteen lo fragments wait in this wave's own 2 KB of LDS: the same values, read where they are used)
  f16x8 w2h[2][8], w2l[2][FL_PARKED];
  char* const parked = smem + FL_W2L + w * 2048 + l * 16;
  {
    const char* base = ff3_img_lane(A.wimg, w, l);
#pragma unroll
    for (int f = 0; f < 16; ++f) {
      w2h[f >> 3][f & 7] = ff3_img_frag(base, 4 + f, 0);
      const f16x8 lo = ff3_img_frag(base, 4 + f, 1);
      if ((f & 7) < FL_PARKED) w2l[f >> 3][f & 7] = lo;
      else *reinterpret_cast<f16x8*>(parked + (f >> 3) * 1024) = lo;
    }
  }
  if (tid < 256) acc_db1[tid] = 0.f;
  char* const wfrag = smem + FL_W1;
  const float w_inv = panel_stage_w<8, 64 * FS_WAVES>(A.w1, 64, wfrag, wmax, tid);
  const float winv2 = A.consts[1], c3t = A.consts[3];

  // ---- this thread's loads of a tile: du2 and d1 in accumulator layout (point 16 blk + li, rows 16 (2 w + t) + 4 g ..),
  // the bounds of its two points, and one float4 of the x panel (row tid / 16, channels 4 (tid & 15) ..) ----
  const int xrow = tid >> 4, xc = tid & 15;
  float4 du2r[4], d1r[4], xr;
  float bzr[2];
  // (addresses as a per-tile uniform base plus a 32-bit lane offset: a 64-bit pointer per load spilled.  Every load is
  //  issued in every pass and by every lane -- behind the last tile the last tile's again, rows past P the last point's,
  //  neither used -- so that the number of loads in flight at each use is the same on every path through the loop and
  //  the compiler's vmcnt waits are the exact ones: with the loads under `has_next` it waited for x with vmcnt(0), that
  //  is for the next tile's du2 and d1 too)
  const unsigned cb = 32 * w + 4 * g;
  const int last_tile = A.ntiles - 1;
  auto load_du2 = [&](int tile) {
    const long t0 = (long)min(tile, last_tile) * 32;
    const int rmax = (int)min(31L, A.P - 1 - t0);           // rows past P read the last point's (and are not used)
    const float* __restrict__ src = A.du2 + t0 * 256;
    const float* __restrict__ bz = A.dzb + t0;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const unsigned r = (unsigned)min(16 * blk + li, rmax);
      bzr[blk] = bz[r];
#pragma unroll
      for (int t = 0; t < 2; ++t) du2r[blk * 2 + t] = *reinterpret_cast<const float4*>(src + (r * 256u + cb + 16u * t));
    }
  };
  auto load_d1 = [&](int tile) {
    const long t0 = (long)min(tile, last_tile) * 32;
    const int rmax = (int)min(31L, A.P - 1 - t0);
    const float* __restrict__ src = A.d1 + t0 * 256;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const unsigned r = (unsigned)min(16 * blk + li, rmax);
#pragma unroll
      for (int t = 0; t < 2; ++t) d1r[blk * 2 + t] = *reinterpret_cast<const float4*>(src + (r * 256u + cb + 16u * t));
    }
  };
  auto load_x = [&](int tile) {
    const long t0 = (long)min(tile, last_tile) * 32;
    const int rmax = (int)min(31L, A.P - 1 - t0);
    const float* __restrict__ src = A.x + t0 * 64;
    xr = *reinterpret_cast<const float4*>(src + (unsigned)(min(xrow, rmax) * 64 + 4 * xc));
  };
  auto x_of = [&](int tile) {                    // .. where it is used: rows past P are zero
    return (long)tile * 32 + xrow < A.P ? xr : make_float4(0.f, 0.f, 0.f, 0.f);
  };

  // ---- consumer role (the wave tiling of k_wgrad_h2<4, 1, 4, 2, 4, 2, false, true>, on the pieces of wgrad_panel.h):
  // du1 panel wm against x channels 32 wn .. ----
  const int wm = w >> 1, wn = w & 1;
  f32x4v gw[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) gw[i][j] = (f32x4v){0.f, 0.f, 0.f, 0.f};
  int ea_used[2] = {15, 15}, eb_used = 15;     // exponents the accumulators are expressed in
  int e_run = 15, e_x = 15;                    // running exponents: this wave's du1 channels; x (the same in every wave)
  const int dg_mt = w & 1, dg_nt = w >> 1;     // this wave's tile of gx: points 16 dg_mt .., input channels 16 dg_nt ..

  // ---- staging of a tile, from the registers its loads filled: du2 -> B fragments, slice kappa = w, one scale per point
  // (the bound the chain derives from that of dz3), the registers free for the tile after; and the wave's maximum of x ----
  float inv_b[2];
  auto stage_du2 = [&]() {
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      float s_du2;
      ff3_scale_du2(bzr[blk], c3t, A.dmax, winv2, s_du2, inv_b[blk]);
      const float4 a = du2r[blk * 2], b = du2r[blk * 2 + 1];
      const float hv[8] = {a.x * s_du2, a.y * s_du2, a.z * s_du2, a.w * s_du2, b.x * s_du2, b.y * s_du2, b.z * s_du2, b.w * s_du2};
      h2_put_frag(smem + FL_DUBUF + ((blk * 8 + w) * 2) * 1024 + l * 16, hv);
    }
  };
  auto stage_xmax = [&](int tile) {
    const float4 xv = x_of(tile);
    float m = fmaxf(fmaxf(fabsf(xv.x), fabsf(xv.y)), fmaxf(fabsf(xv.z), fabsf(xv.w)));
    m = wave_max(m);
    if (l == 0) xmax[w] = m;
  };

  load_du2(blockIdx.x); load_d1(blockIdx.x); load_x(blockIdx.x);      // (the grid is at most the number of tiles)
  lds_barrier();                               // W1 fragments and the zeroed sums are in LDS
  stage_du2(); stage_xmax(blockIdx.x);
  load_du2(blockIdx.x + gridDim.x);
  // (the second-dispatched half of the workgroup loses the issue arbitration against its SIMD partners in every phase:
  //  one static priority step for it, 1589 -> 1575 us)
  if (__builtin_amdgcn_readfirstlane(w) >= 4) __builtin_amdgcn_s_setprio(1);
#ifdef RPDE_STAMPS
  const bool stamp_on = blockIdx.x == 100 && l == 0 && (w == 0 || w == 3 || w == 6);
  const int stamp_w = w == 0 ? 0 : (w == 3 ? 1 : 2);
  int stamp_t = -4;                      // skip the first four tiles (cold caches)
#endif
  for (int tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
    const int next_tile = tile + gridDim.x;
    const long p0 = (long)tile * 32;
    FLSTAMP(0);
    lds_barrier();                                                                    // 1: du2 slices and x maxima in LDS
    FLSTAMP(1);

    // ---- du1 = (W2^T du2) * d1: this wave's 32 hidden rows of both point blocks ----
    float u[4][4];                               // [blk * 2 + t][r]: point 16 blk + li, row 16 (2 w + t) + 4 g + r
    float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    {
      f32x4v acc[2][2];
#pragma unroll
      for (int blk = 0; blk < 2; ++blk) {
        acc[blk][0] = (f32x4v){0.f, 0.f, 0.f, 0.f}; acc[blk][1] = (f32x4v){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kap = 0; kap < 8; ++kap) {
          const char* hb = smem + FL_DUBUF + ((blk * 8 + kap) * 2) * 1024 + l * 16;
          const f16x8 bh = *reinterpret_cast<const f16x8*>(hb), bl = *reinterpret_cast<const f16x8*>(hb + 1024);
          if (kap < FL_PARKED) {
            acc[blk][0] = h2_mfma32(w2h[0][kap], w2l[0][kap], bh, bl, acc[blk][0]);
            acc[blk][1] = h2_mfma32(w2h[1][kap], w2l[1][kap], bh, bl, acc[blk][1]);
          } else {
            const f16x8 l0 = *reinterpret_cast<const f16x8*>(parked), l1 = *reinterpret_cast<const f16x8*>(parked + 1024);
            acc[blk][0] = h2_mfma32(w2h[0][kap], l0, bh, bl, acc[blk][0]);
            acc[blk][1] = h2_mfma32(w2h[1][kap], l1, bh, bl, acc[blk][1]);
          }
        }
      }
#pragma unroll
      for (int blk = 0; blk < 2; ++blk) {
        const bool live = p0 + 16 * blk + li < A.P;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          // (ff3_du_tile<true> written out, plus the zeroing: through the call the kernel takes 256 registers and scratch)
          const float4 d4 = d1r[blk * 2 + t];
          const float d[4] = {d4.x, d4.y, d4.z, d4.w};
          float* v = u[blk * 2 + t];
          float s[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) { s[r] = acc[blk][t][r] * inv_b[blk]; v[r] = s[r] * d[r]; }
          if (live) {
#pragma unroll
            for (int r = 0; r < 4; ++r) bsum[4 * t + r] = __builtin_fmaf(s[r], d[r], bsum[4 * t + r]);
          } else {                                // a point past the end: its column of the products is not a gradient
            v[0] = v[1] = v[2] = v[3] = 0.f;
          }
        }
      }
    }
    // (d1's registers are free from here, but the next tile's loads start only behind the consumer: in flight across it
    //  they are the 16 registers its gx products need to read a half panel ahead -- 1572 -> 1532 us with both)
    FLSTAMP(2);
    ff3_bias_rows(bsum);
    if (li == 15)
#pragma unroll
      for (int i = 0; i < 8; ++i) acc_db1[ff3_bias_row(w, g, i)] += bsum[i];
    // ---- du1 -> this wave's half of panel w / 2 (channels 32 (w & 1) .. of it) under the wave's running exponent ----
    {
      float m = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) m = fmaxf(fmaxf(m, fmaxf(fabsf(u[i][0]), fabsf(u[i][1]))), fmaxf(fabsf(u[i][2]), fabsf(u[i][3])));
      const float scale = panel_run_scale(e_run, wave_max(m));
      char* const dst = smem + FL_PAN + (w >> 1) * FL_PANEL;
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const float* v = u[blk * 2 + t];
          panel_put4(dst, 16 * blk + li, (w & 1) * 8 + 4 * t + g, v[0], v[1], v[2], v[3], scale);
        }
      if (l == 0) einfo[w] = e_run;
    }
    // ---- x -> its panel under the running exponent of the whole panel ----
    {
      float m = 0.f;
#pragma unroll
      for (int i = 0; i < FS_WAVES; ++i) m = fmaxf(m, xmax[i]);
      const float scale = panel_run_scale(e_x, m);
      const float4 xv = x_of(tile);
      panel_put4(smem + FL_X, xrow, xc, xv.x, xv.y, xv.z, xv.w, scale);
    }
    load_x(next_tile);
    FLSTAMP(3);
    lds_barrier();                                                                    // 2: du1 and x panels in LDS
    FLSTAMP(4);
    // ---- the NEXT tile's du2 slices, ahead of this tile's consumer, and the loads of the tile after it ----
    // No new barrier: the du2 slices were last read by the products above, which every wave has finished (lds_barrier
    // waits for its LDS reads) before any wave passes barrier 2, and they are read again only behind the next barrier 1;
    // the x maxima (written at the end of the pass) were last read by the x panel write above, in front of barrier 2
    // too.  What the consumer below reads -- the panels, einfo -- is written again only behind the next barrier 1, which
    // no wave passes before all have left the consumer.
    // (Built and measured, same machine, us per launch in the step, the parent's order 1659: the du2 loads at the end of
    //  the pass with the staging there 1717; that with waves 4-7 / waves 0-3 staging in front of the consumer as in
    //  k_wgrad_h2, 1699 / 1702; all eight waves staging here with the loads right behind, 1596 -- kept.  The staging is
    //  about 110 vector instructions of a pass's 530: what a pair can overlap between two barriers is a few hundred
    //  cycles of 12 K, less than the later issue of the loads costs)

    stage_du2();
    load_du2(next_tile + gridDim.x);
    FLSTAMP(5);

    // (the consumer's LDS addresses are formed here, per tile, from a lane index the compiler cannot see through: hoisted
    //  out of the loop they stayed in registers beside W2^T and the accumulators, and seven of them spilled)
    int lc = l;
    asm volatile("" : "+v"(lc));
    const int gc = lc >> 4, lic = lc & 15;
    // ---- gW1 += du1^T . x ----
    {
      const StageTr tr(gc, lic);
      const int eb = __builtin_amdgcn_readfirstlane(e_x);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        float f;
        if (panel_exp_moved(ea_used[k], eb_used, __builtin_amdgcn_readfirstlane(einfo[2 * wm + k]), eb, f)) {
#pragma unroll
          for (int j = 0; j < 2; ++j) { gw[2 * k][j] *= f; gw[2 * k + 1][j] *= f; }
        }
      }
      eb_used = eb;
      f16x8 bh[2], bl[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) panel_frag_tr(smem + FL_X, tr, 2 * wn + j, bh[j], bl[j]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f16x8 ah, al;
        panel_frag_tr(smem + FL_PAN + wm * FL_PANEL, tr, i, ah, al);
#pragma unroll
        for (int j = 0; j < 2; ++j) gw[i][j] = h2_mfma32(ah, al, bh[j], bl[j], gw[i][j]);
      }
    }
    FLSTAMP(6);
    // ---- gx = du1 . W1: one half panel (32 hidden channels, one exponent) at a time ----
    {
      f32x4v tot = (f32x4v){0.f, 0.f, 0.f, 0.f};
      const int row = 16 * dg_mt + lic;                     // A fragment: lane = point, 8 consecutive channels
      f16x8 ah[2], al[2], bh[2], bl[2];
      auto frags = [&](int hp) {
        const char* pa_ = smem + FL_PAN + (hp >> 1) * FL_PANEL + stage_off(row, 2 * (4 * (hp & 1) + gc));
        ah[hp & 1] = *reinterpret_cast<const f16x8*>(pa_); al[hp & 1] = *reinterpret_cast<const f16x8*>(pa_ + 4096);
        const char* wb = wfrag + (hp * 4 + dg_nt) * 2048 + lc * 16;
        bh[hp & 1] = *reinterpret_cast<const f16x8*>(wb); bl[hp & 1] = *reinterpret_cast<const f16x8*>(wb + 1024);
      };
      frags(0);
      // (each half panel's fragments are read under the products of the one before: read, wait, three dependent
      //  products, scale, eight times in a row, was a fifth of a pass for 24 products -- profiles/ffs_layer1_stamps.py)
#pragma unroll
      for (int hp = 0; hp < 8; ++hp) {
        if (hp + 1 < 8) frags(hp + 1);
        const f32x4v part = h2_mfma32(ah[hp & 1], al[hp & 1], bh[hp & 1], bl[hp & 1], (f32x4v){0.f, 0.f, 0.f, 0.f});
        const int ek = __builtin_amdgcn_readfirstlane(einfo[hp]);
        const float fk = panel_exp_factor(ek) * w_inv;
        tot += part * fk;
      }
      // lane (g, li) holds points 4 g + r of channel li: a 4 x 4 transpose inside every quad gives one 16-byte store
      float t0 = tot[0], t1 = tot[1], t2 = tot[2], t3 = tot[3];
      quad_transpose(t0, t1, t2, t3);
      const int rq = 16 * dg_mt + 4 * gc + (lic & 3);
      if (p0 + rq < A.P) *reinterpret_cast<float4*>(A.gx + p0 * 64 + (unsigned)(rq * 64 + 16 * dg_nt + 4 * (lic >> 2))) = make_float4(t0, t1, t2, t3);
    }
    FLSTAMP(7);
    load_d1(next_tile);
    stage_xmax(next_tile);
#ifdef RPDE_STAMPS
    ++stamp_t;
#endif
  }

  // ---- this workgroup's slab [256][64] of gW1 and its db1 ----
  // (written out as in k_wgrad_h2, see there; the factors are panel_exp_factor's)
  const float fb = __uint_as_float((unsigned)(eb_used - 14) << 23);
  float* __restrict__ out = A.slabs + (long)blockIdx.x * 256 * 64;
  const unsigned o0 = (unsigned)((wm * 64 + 4 * g) * 64 + wn * 32 + li);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float fa = __uint_as_float((unsigned)(ea_used[i >> 1] - 14) << 23);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[o0 + (unsigned)((16 * i + r) * 64 + 16 * j)] = gw[i][j][r] * fa * fb;
  }
  lds_barrier();
  ff3_part_out<0, 256, 64 * FS_WAVES>(A.part + (long)blockIdx.x * FF3_PART, acc_db1, nullptr, tid);
}

// --------------------------------------------------------------------------------------------------------------------
bool ff_bwd_split_ok(long P, int hid, int dim) { return !switch_off("RPDE_FF_BWD_SPLIT") && wgrad_h2_dgrad_ok(P, hid, dim); }

int ff_bwd_split_launch(const rpde_ff_params* p, const float* const* ds, const float* z_last, const float* grad_out,
                        const float* x, float* dz3, float* du2, float* dzb, float* gx, float* slabs, float* gw1, float* part,
                        int* grid_out, long P, void* fimg, hipStream_t st, FoldJobs* folds) {
  RPDE_CHECK_ARG(ff_bwd_split_ok(P, p->dim * p->factor, p->dim) && ds && ds[0] && ds[1] && gx && gw1 && slabs,
                 "ff_bwd_split: unsupported call");
  const char* img;
  const float* consts;
  RPDE_TRY(ff3_fused_bwd_prepare(p, fimg, &img, &consts, st));
  const int ntiles = (int)((P + 31) / 32);
  int cus;
  RPDE_HIP(cu_count(&cus));
  int grid = cus < FS_MAX_GRID ? cus : FS_MAX_GRID;
  if (ntiles < grid) grid = ntiles;
  const DropCfg drop2 = make_drop(p->dropout_p, layer_seed(p->seed, 2), p->seed_epoch);   // the forward's mask of layer 3

  FsA a;
  memset(&a, 0, sizeof(a));
  a.g = grad_out; a.z3 = z_last; a.d2 = ds[1];
  a.dz3 = dz3; a.du2 = du2; a.dzb = dzb;
  a.wimg = img; a.consts = consts; a.gamma = p->ln_gamma; a.beta = p->ln_beta; a.part = part;
  a.P = P; a.layer_norm = p->layer_norm; a.eps = p->ln_eps; a.post_act = p->post_act;
  a.drop2 = drop2; a.ntiles = ntiles;
  hipLaunchKernelGGL(k_ffs_adjoint, dim3(grid), dim3(64 * FS_WAVES), 0, st, a);
  RPDE_LAUNCH_CHECK();

  FsB b;
  memset(&b, 0, sizeof(b));
  b.du2 = du2; b.d1 = ds[0]; b.x = x; b.dzb = dzb; b.w1 = p->weights[0];
  b.gx = gx; b.slabs = slabs; b.part = part;
  b.wimg = img; b.consts = consts;
  b.P = P; b.dmax = 1.13f * drop2.scale;     // |gelu'| <= 1.129, times the dropout scale folded into d (as the chain)
  b.ntiles = ntiles;
  hipLaunchKernelGGL(k_ffs_layer1, dim3(grid), dim3(64 * FS_WAVES), 0, st, b);
  RPDE_LAUNCH_CHECK();
  *grid_out = grid;
  const int hid = p->dim * p->factor;
  if (folds && folds->add(slabs, gw1, hid * p->dim, grid, (long)hid * p->dim)) return RPDE_OK;
  return reduce_slabs(slabs, gw1, (long)hid * p->dim, grid, (long)hid * p->dim, 1.f, 0, st);
}

}  // namespace rpde

#ifdef RPDE_STAMPS
extern "C" int rpde_debug_ffl_stamps(unsigned long long* host_out) {
  RPDE_HIP(hipDeviceSynchronize());
  RPDE_HIP(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(rpde::g_flstamps), sizeof(unsigned long long) * 3 * 64));
  return RPDE_OK;
}
#endif
