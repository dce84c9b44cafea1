// Fused kernels of FSpectralConv2d.forward_fourier and its adjoint for channels-last fields with C = 64
// channels (reference: models/spectral_convolution.py:256-318), in h2 arithmetic (h2.h).
//
//   analysis   one launch, both axes: every WAVE owns whole lines (one (b,m) row along y, one (b,n) column
//              along x), streams them in 32-point chunks HBM -> registers -> (scale, split into two f16 pieces) ->
//              its private 8 KB of LDS -> transposing reads -> MFMA against the DFT table (resident in LDS as ready
//              fragments), and writes the line's [2K, C] spectrum.  No workgroup barrier after the table is loaded.
//              Blocks are ordered sample-chunk by sample-chunk, y lines then x lines, so that the second read of a
//              sample is served by the Infinity Cache rather than HBM.
//   split      the (mixed) spectra, ~15 % of the field, are re-laid once as MFMA B fragments: [line][16 channels]
//              [hi|lo] 1 KB pieces that a wave loads with one coalesced 16-byte-per-lane read, plus one scale per line.
//   synthesis  ONE pass writes out = Fs_y . At_y[row] + Fs_x . At_x[col] (+ skip gradient): a wave owns a
//              16 x 16 x 16-channel tile, forms the x-axis part column by column (MFMA rows = m), turns it
//              through its private 16 KB of LDS into the layout of the y-axis part (MFMA rows = n), adds and stores.
//              The field is written once and never read back (the round-1 path wrote it twice and re-read it once).
#include "fused_spectral.h"
#include "cw.h"
#include "h2.h"

namespace rpde {

// RPDE_STAMPS (debug build, rpde/build.py --stamps): lane 0 of waves from the middle of a launch records s_memtime at
// phase boundaries into a buffer of its own; rpde_debug_fused_stamps() copies it out (profiles/fused_stamps.py)
#ifdef RPDE_STAMPS
__device__ unsigned long long g_fstamps[2][64 * 32];
#define FSTAMP(k, i) do { if (stamp_on) g_fstamps[k][stamp_slot * 32 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define FSTAMP(k, i) do { } while (0)
#endif

// ------------------------------------------------------------------------------------------------------------
// table fragments (built once per plan)
// ------------------------------------------------------------------------------------------------------------
// analysis operand of T[r][y] = src[r*rs + y*cs] (r < R, y < n): fragment (s, mt, piece) holds for lane l the
// eight entries T[16 mt + (l & 15)][32 s + 8 (l >> 4) + j] * 2^12
// perm: slot j of lane group g holds reduction index 32 s + 4 j + g instead of 32 s + 8 g + j (the points a lane of
// k_dft_analysis_rr_h2 loads)
__global__ __launch_bounds__(64) void k_h2_table_ana(const float* __restrict__ src, long rs, long cs, int R, int n, int MT,
                                                     char* __restrict__ out, int perm) {
  const int f = blockIdx.x, l = threadIdx.x;
  const int s = f / MT, mt = f % MT;
  const int r = 16 * mt + (l & 15), g = l >> 4;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int y = 32 * s + (perm ? 4 * j + g : 8 * g + j);
    v[j] = (r < R && y < n) ? src[r * rs + y * cs] * (float)(1 << H2_TABLE_EXP) : 0.f;
  }
  uint4 hi, lo;
  h2_split8(v, hi, lo);
  char* p = out + (long)f * 2048 + l * 16;
  *reinterpret_cast<uint4*>(p) = hi;
  *reinterpret_cast<uint4*>(p + 1024) = lo;
}

// synthesis operand of S[y][r] = src[y*rs + r*cs] (y < n, r < R), times 2^12: one operand block (fused_spectral.h) per
// 16-row tile
template <int K32, int TG>
__global__ __launch_bounds__(64) void k_h2_table_syn(const float* __restrict__ src, long rs, long cs, int n, int R,
                                                     char* __restrict__ out) {
  typedef H2Block<K32, TG> L;
  const int yt = blockIdx.x, l = threadIdx.x, g = l >> 4, li = l & 15;
  const int y = 16 * yt + li;
  char* blk = out + (long)yt * L::BYTES;
#pragma unroll
  for (int s = 0; s <= K32; ++s) {
    if (s == K32 && g >= TG) break;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r = 32 * s + 8 * g + j;
      v[j] = (y < n && r < R) ? src[y * rs + r * cs] * (float)(1 << H2_TABLE_EXP) : 0.f;
    }
    uint4 hi, lo;
    h2_split8(v, hi, lo);
    if (s < K32) {
      *reinterpret_cast<uint4*>(blk + L::hi(s) + l * 16) = hi;
      *reinterpret_cast<uint4*>(blk + L::lo(s) + l * 16) = lo;
    } else {
      L::template store_tail<true>(blk, g, li, hi, lo);
    }
  }
  if (TG > 0 && g == 0) L::zero_unused(blk, li);
}

size_t h2_ana_bytes(int n, int R) { return (size_t)(n / 32) * ((R + 15) / 16) * 2048; }
size_t h2_syn_bytes(int n, int R) { return (size_t)((n + 15) / 16) * h2_block_bytes(R / 32, (R % 32) / 8); }

int h2_build_tables(rpde_plan* p, hipStream_t st) {
  const int R = 2 * p->kp, n = p->n;
  const int MT = (R + 15) / 16;
  for (int i = 0; i < 2; ++i) {
    RPDE_HIP(hipMalloc(&p->h2_ana[i], h2_ana_bytes(n, R)));
    RPDE_HIP(hipMalloc(&p->h2_ana_p[i], h2_ana_bytes(n, R)));
    RPDE_HIP(hipMalloc(&p->h2_syn[i], h2_syn_bytes(n, R)));
  }
  const dim3 ga((n / 32) * MT), gs((n + 15) / 16);
  // [0]: forward operands (Fa analysis, Fs synthesis); [1]: adjoint operands (Fs^T analysis, Fa^T synthesis)
  hipLaunchKernelGGL(k_h2_table_ana, ga, dim3(64), 0, st, p->fa, (long)p->ldn, 1L, R, n, MT, (char*)p->h2_ana[0], 0);
  hipLaunchKernelGGL(k_h2_table_ana, ga, dim3(64), 0, st, p->fs, 1L, (long)R, R, n, MT, (char*)p->h2_ana[1], 0);
  hipLaunchKernelGGL(k_h2_table_ana, ga, dim3(64), 0, st, p->fa, (long)p->ldn, 1L, R, n, MT, (char*)p->h2_ana_p[0], 1);
  hipLaunchKernelGGL(k_h2_table_ana, ga, dim3(64), 0, st, p->fs, 1L, (long)R, R, n, MT, (char*)p->h2_ana_p[1], 1);
  h2_dispatch(R, [&](auto k32, auto tg) {
    hipLaunchKernelGGL((k_h2_table_syn<k32(), tg()>), gs, dim3(64), 0, st, p->fs, (long)R, 1L, n, R, (char*)p->h2_syn[0]);
    hipLaunchKernelGGL((k_h2_table_syn<k32(), tg()>), gs, dim3(64), 0, st, p->fa, 1L, (long)p->ldn, n, R, (char*)p->h2_syn[1]);
  });
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

// ------------------------------------------------------------------------------------------------------------
// analysis
// ------------------------------------------------------------------------------------------------------------
constexpr int ANA_WAVES = 8;          // lines in flight per workgroup: one round
constexpr int ANA_MAXKS = 8;          // n <= 256

struct AnaAxis {
  const char* timg;   // analysis-type table fragments
  float* spec;        // [lines][R][64]
  float* amax;        // [lines] max |spectrum| (null: not wanted)
  int n, ks;          // axis length, n / 32
  int lps, rps;       // lines per sample, rounds (of ANA_WAVES lines) per sample
  int zdiv;           // line z -> field offset (z / zdiv) * s1 + (z % zdiv) * s2
  long s1, s2, ldk;   // ldk: stride between consecutive points of a line
};
struct AnaP {
  const float* x;
  AnaAxis ax[2];
  int naxes, B, chunk, R;
  int items;          // rounds in the launch, ordered chunk of samples by chunk: all y rounds, then all x rounds
};

template <int MT>
__global__ __launch_bounds__(64 * ANA_WAVES, 2) void k_dft_analysis_h2(const AnaP P) {
  __shared__ __attribute__((aligned(16))) char smem[ANA_MAXKS * MT * 2048 + ANA_WAVES * 8192];
  const int tid = threadIdx.x, l = tid & 63, wave = tid >> 6;
  char* const stage = smem + ANA_MAXKS * MT * 2048 + wave * 8192;
  const int g = l >> 4, li = l & 15;
  const StageTr tr(g, li);                      // transposing-read address of this lane inside a piece (wave.h)
  typedef s16x4v __attribute__((address_space(3))) * lds_tr;

  // persistent workgroups: round w, w + gridDim.x, ...; every wave walks the same rounds and owns line `wave` of each
  // (the host guarantees whole rounds: lines per sample % 8 == 0).  The 32-point chunks of all its lines form one
  // stream, read two chunks ahead into two register sets, so that 16 KB per wave (128 KB per CU) are in flight.
  const int per_chunk = P.chunk * (P.ax[0].rps + (P.naxes > 1 ? P.ax[1].rps : 0));
  struct Pos { int w, a, s; long z; };              // a < 0: past the end
  auto first_valid = [&](int w) {
    Pos p; p.a = -1; p.s = 0; p.z = -1;
    for (; w < P.items; w += gridDim.x) {          // skips the holes of the last, partial chunk of samples
      const int ck = w / per_chunk;
      int r = w - ck * per_chunk;
      const int nb = min(P.chunk, P.B - ck * P.chunk);
      int aa = 0;
      if (r >= nb * P.ax[0].rps) { r -= nb * P.ax[0].rps; aa = 1; }
      if (aa >= P.naxes || r >= nb * P.ax[aa].rps) continue;
      p.a = aa;
      p.z = (long)(ck * P.chunk + r / P.ax[aa].rps) * P.ax[aa].lps + (r % P.ax[aa].rps) * ANA_WAVES + wave;
      break;
    }
    p.w = w;
    return p;
  };
  auto next = [&](Pos p) {
    if (p.a < 0) return p;
    if (p.s + 1 < P.ax[p.a].ks) { ++p.s; return p; }
    return first_valid(p.w + gridDim.x);
  };
  auto issue = [&](float4 (&buf)[8], const Pos& p) {
    if (p.a < 0) return;
    const AnaAxis& A = P.ax[p.a];
    const float* __restrict__ q0 = P.x + (p.z / A.zdiv) * A.s1 + (p.z % A.zdiv) * A.s2 + (long)(32 * p.s + g) * A.ldk + li * 4;
    const long st4 = 4 * A.ldk;
#pragma unroll
    for (int i = 0; i < 8; ++i) buf[i] = *reinterpret_cast<const float4*>(q0 + i * st4);
  };
  int cur_axis = -1;
  int line_E = 0;              // exponent field the current line is scaled by (0: nothing seen yet)
  f32x4v tot[MT][4];
#ifdef RPDE_STAMPS
  const bool stamp_blk = blockIdx.x >= 96 && blockIdx.x < 160;
  const int stamp_slot = (int)blockIdx.x - 96;
  int stamp_n = 0;
#endif
  // one chunk: buf holds chunk p; once it is in LDS the registers are refilled with chunk pn
  auto process = [&](float4 (&buf)[8], const Pos& p, const Pos& pn) {
    const AnaAxis& A = P.ax[p.a];
    if (p.s == 0) {
      if (p.a != cur_axis) {
        // ---- table fragments -> LDS (the only workgroup-wide step; every wave starts a line of this round here) ----
        __syncthreads();
        const uint4* src = reinterpret_cast<const uint4*>(A.timg);
        uint4* dst = reinterpret_cast<uint4*>(smem);
        const int nvec = A.ks * MT * 128;
        for (int i = tid; i < nvec; i += 64 * ANA_WAVES) dst[i] = src[i];
        __syncthreads();
        cur_axis = p.a;
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) tot[mt][nt] = (f32x4v){0.f, 0.f, 0.f, 0.f};
      line_E = 0;
    }
#ifdef RPDE_STAMPS
    const bool stamp_on = stamp_blk && tid == 0 && stamp_n < 6;
#endif
    FSTAMP(0, stamp_n * 5 + 0);
    // chunk maximum -> the line's running power-of-two scale.  The accumulators stay in scaled units for the whole
    // line (the MFMAs accumulate in place; no per-chunk rescaling on the VALU): the scale exponent only ever grows,
    // and when a chunk exceeds it the accumulators are multiplied by the (exact) ratio once.
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(m) : "v"(buf[i].x), "v"(buf[i].y));
      asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(m) : "v"(buf[i].z), "v"(buf[i].w));
    }
    m = wave_max(m);
    {
      const int E = max((int)(__float_as_uint(m) >> 23) & 0xff, 15 + H2_TABLE_EXP);
      if (E > line_E) {                                  // wave-uniform
        if (line_E > 0) {
          const float f = __uint_as_float((unsigned)(127 + line_E - E) << 23);      // 2^(old - new) <= 1/2, >= 2^-126
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
              for (int j = 0; j < 4; ++j) tot[mt][nt][j] *= (E - line_E < 126 ? f : 0.f);
        }
        line_E = E;
      }
    }
    const float scale = __uint_as_float((unsigned)(268 - line_E) << 23);
    FSTAMP(0, stamp_n * 5 + 1);
    // split into two f16 pieces, keep the memory order [point][channel] in LDS
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      uint2 hi, lo;
      h2_split4(buf[i].x * scale, buf[i].y * scale, buf[i].z * scale, buf[i].w * scale, hi, lo);
      const int off = stage_off(4 * i + g, li);
      *reinterpret_cast<uint2*>(stage + off) = hi;
      *reinterpret_cast<uint2*>(stage + 4096 + off) = lo;
    }
    issue(buf, pn);
    wave_lds_fence();
    FSTAMP(0, stamp_n * 5 + 2);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const char* t = tr.at(stage, nt);
      union { struct { s16x4v a, b; } h; f16x8 v; } bh, bl;
      bh.h.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr)(t));
      bh.h.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr)(t + 512));
      bl.h.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr)(t + 4096));
      bl.h.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr)(t + 4096 + 512));
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        // table fragments straight from LDS each time (the LDS pipe is nearly idle; keeping all of them in
        // registers would cost 16 VGPRs that the second load buffer needs)
        const char* ta = smem + (p.s * MT + mt) * 2048 + l * 16;
        const f16x8 ah = *reinterpret_cast<const f16x8*>(ta), al = *reinterpret_cast<const f16x8*>(ta + 1024);
        tot[mt][nt] = h2_mfma32(ah, al, bh.v, bl.v, tot[mt][nt]);
      }
    }
    wave_lds_fence();
    FSTAMP(0, stamp_n * 5 + 3);
#ifdef RPDE_STAMPS
    ++stamp_n;
#endif
    if (p.s == A.ks - 1) {
      // spectrum of the line: row 16 mt + 4 g + j, channel 16 nt + li
      float* __restrict__ sp = A.spec + p.z * (long)P.R * 64;
      const float inv = __uint_as_float((unsigned)(line_E - 14 - H2_TABLE_EXP) << 23);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = 16 * mt + 4 * g + j;
          if (row < P.R) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) sp[row * 64 + 16 * nt + li] = tot[mt][nt][j] * inv;
          }
        }
      if (A.amax) {
        // (rows beyond R belong to zero table rows: they do not disturb the maximum)
        float am = 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) {
            asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(am) : "v"(tot[mt][nt][0]), "v"(tot[mt][nt][1]));
            asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(am) : "v"(tot[mt][nt][2]), "v"(tot[mt][nt][3]));
          }
        am = wave_max(am);
        if (l == 0) A.amax[p.z] = am * inv;
      }
    }
  };
  float4 ba[8], bb[8];
  Pos pa = first_valid(blockIdx.x), pb = next(pa);
  issue(ba, pa);
  issue(bb, pb);
  while (pa.a >= 0) {
    const Pos pc = next(pb);
    process(ba, pa, pc);
    if (pb.a < 0) break;
    const Pos pd = next(pc);
    process(bb, pb, pd);
    pa = pc; pb = pd;
  }
}

// ------------------------------------------------------------------------------------------------------------
// analysis of square grids, both axes out of ONE pass over HBM: the round-robin schedule (round 4)
// ------------------------------------------------------------------------------------------------------------
// k_dft_analysis_h2 reads the field twice -- once per axis -- and the second read comes from the Infinity Cache at
// best, which streams no faster than HBM (profiles/r03_mall_bandwidth.txt: 6.1 vs 5.4 TB/s).  An L2 does (12 TB/s),
// but it holds 4 MB per XCD, so the two reads of a piece of the field must come close together in time and place.
// The retired row-block kernel (round 3) walked a sample 32-row block by block and read the field
// once, but a row's eight 32-point chunks sat in eight waves and their partial spectra were summed through 96 KB of LDS
// behind two barriers per step -- in-kernel stamps put 5.8 K of a step's 12.3 K cycles there, against 4.3 K for the
// chunks themselves.  The sum exists because in a 32-row block every wave has one chunk of a column (32 rows) but only
// an eighth of a row.  It goes away if a wave meets its WHOLE row over the rounds of a sample the way it already meets
// its whole column: cut the sample into nb x nb tiles of 32 x 32 points (nb = n / 32) and let wave gw of a group own
// row gw AND column gw.  In round t the wave in band i = gw / 32 adds
//   * to its row accumulators    the 32 points of its row    that lie in tile (i, i + t),      and
//   * to its column accumulators the 32 points of its column that lie in tile (i - t, i)       (indices mod nb).
// Tile (a, b) is then read in round b - a by the waves of band a (as rows) and by the waves of band b (as columns): both
// in the SAME round -- a tournament schedule -- so the second read finds the tile in the L2 of the XCD that the group's
// workgroups share (placement is a speed matter only), exactly the 2 MB per round that the row-block walk kept there.
// After nb rounds every wave holds one finished row spectrum and one finished column spectrum.  No landing zone, no
// partial sums, no barrier after the table is in LDS; the table (48 KB) is all the LDS the kernel uses; every wave has a
// row and a column on every grid (a group is exactly n waves = n / 8 workgroups), so the idle-wave cases of the
// row-block kernel (and the memory fault they once caused) do not exist here.
// Loads: inline asm one round ahead, waits counted by hand (left to the compiler, every use of a prefetched chunk also
// waits for everything issued behind it: DESIGN.md section 3.1); behind a chunk there are always the 8 loads of the
// other axis's chunk, so a fixed vmcnt(8) covers it (the 20-odd spectrum stores of a sample's last round only make that
// wait longer).
// Measured (profiles/r04_analysis_variants.txt; 256^2, B = 32, same box within a pair; FETCH = 2 x FETCH_SIZE):
//   the retired row-block kernel ..................................... 208 us, 551 MB fetched
//   this kernel, every wave free-running ............................. 213 us, 847 MB  (waves of a workgroup drift apart:
//                                                                              the second reader of a tile comes too late)
//   + odd bands take their row chunk first ........................... 226 us, 838 MB
//   + ONE s_barrier per round (no LDS traffic) ....................... 196 us, 565 MB  <- shipped
// In-kernel stamps of the shipped form (profiles/fused_stamps.py): of a round's ~13 K cycles the two chunks take 2 x 1.6 K;
// ISSUING a chunk's eight loads takes 1.5-4 K -- the CU's vector-memory pipeline accepts a 1 KB wave-load every ~100
// cycles once its queues are full, i.e. ~10 bytes per cycle and CU (the HBM-bound streaming rate of
// MI355X_MICROARCH.md's cycle table) -- and the barrier absorbs the skew that leaves.  Every byte of the field passes
// that pipeline TWICE (once per axis; the second time from L2 at about twice the rate): 2.1 MB / 10 + 2.1 MB / 23 +
// 0.66 MB / 10 bytes per cycle = 0.37 M cycles = 185 us at 2 GHz.  The kernel is at the rate of the bytes its CUs load,
// not of the bytes HBM delivers; only loading each byte once per CU would change that.
struct AnaRrP {
  const float* x; const char* timg;
  float* spec_y; float* spec_x; float* amax_y; float* amax_x;
  int B, n, nb, R, ng;
};

template <int MT>
__global__ __launch_bounds__(64 * ANA_WAVES, 2) void k_dft_analysis_rr_h2(const AnaRrP P) {
  __shared__ __attribute__((aligned(16))) char smem[ANA_MAXKS * MT * 2048];
  const int tid = threadIdx.x, l = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = l >> 4, li = l & 15;
  const int n = P.n, nb = P.nb;
  const int xg = blockIdx.x % P.ng, jw = blockIdx.x / P.ng, gw = jw * ANA_WAVES + wave;     // gw < n: this wave's row and column
  const int band = gw >> 5;
  const int nsamp = (P.B - xg + P.ng - 1) / P.ng;
  const long units = (long)nsamp * nb;               // (sample, round) pairs of this group, in order
  if (units <= 0) return;                            // (more groups than samples)
  {
    const uint4* src = reinterpret_cast<const uint4*>(P.timg);
    uint4* dst = reinterpret_cast<uint4*>(smem);
    for (int i = tid; i < nb * MT * 128; i += 64 * ANA_WAVES) dst[i] = src[i];
    __syncthreads();
  }
  const long rowf = (long)n * 64;                    // floats per row of the field
  // Which chunk a wave takes first.  Tile (a, a + t) is read by band a as a ROW chunk and by band a + t as a COLUMN chunk;
  // the second read finds the tile in L2 more surely when both are requested in the same half of the round than half a
  // round apart (with "column first" everywhere 58 % of the second reads missed: 847 MB fetched for a 537 MB field).
  // Odd bands therefore take their row chunk first, even bands their column chunk: every tile of an odd round (a and
  // a + t of different parity) is then requested by both its readers in the same half.  The order is fixed per wave --
  // the two accumulator sets are bound to "first" and "second", so nothing in the loop depends on it but addresses.
  const bool row_first = band & 1;
  // chunk `half` (0: first, 1: second) of round u into buf: a row chunk (points of band (band + t) mod nb, lane (g, li)
  // takes points 4 i + g, channels 4 li ..) or a column chunk (rows of band (band - t) mod nb).  Past the end: a clamped
  // re-read, so that every round issues the same 16 loads.  Returns the table chunk that goes with it.
  auto chunk_of = [&](long u, int half, const float*& q0, long& st) {
    u = u < units ? u : units - 1;
    const int sb = (int)(u / nb), t = (int)(u - (long)sb * nb);
    const bool is_row = row_first == (half == 0);
    int ra = band - t; ra += ra < 0 ? nb : 0;
    int cb = band + t; cb -= cb >= nb ? nb : 0;
    const long base = (long)(xg + P.ng * sb) * n;
    q0 = is_row ? P.x + ((base + gw) * n + 32 * cb + g) * 64 + li * 4 : P.x + ((base + 32 * ra + g) * n + gw) * 64 + li * 4;
    st = is_row ? 256 : 4 * rowf;
    return is_row ? cb : ra;
  };
  auto issue = [&](f32x4v (&buf)[8], long u, int half) {
    const float* q0; long st;
    chunk_of(u, half, q0, st);
#pragma unroll
    for (int i = 0; i < 8; ++i) buf[i] = global_load_b128(q0 + i * st);
  };
  // the chunk in buf has landed once at most 8 later vector-memory instructions are outstanding: the other axis's chunk
  // (tests/test_isa_pending_loads_cpu.py follows the `landed` comment, which names the registers)
  auto landed = [&](f32x4v (&buf)[8]) {
    asm volatile("s_waitcnt vmcnt(8)\n\ts_nop 0 ; landed %0 %1 %2 %3 %4 %5 %6 %7"
                 : "+v"(buf[0]), "+v"(buf[1]), "+v"(buf[2]), "+v"(buf[3]), "+v"(buf[4]), "+v"(buf[5]), "+v"(buf[6]), "+v"(buf[7])
                 :
                 : "memory");
  };
  // one 32-point chunk into accumulators that stay in scaled units for the whole line (k_dft_analysis_h2's running
  // power-of-two scale).  No staging: the eight points a lane loaded for channel 4 li + e (buf[0..7], component e) ARE
  // the eight reduction slots of its lane group in a B fragment whose column li stands for channel 4 li + e -- the table
  // image carries the matching permutation of the reduction index (h2_ana_p)
  auto process = [&](f32x4v (&buf)[8], int s, f32x4v (&tot)[MT][4], int& line_E) {
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      m = fmaxf(m, fmaxf(fmaxf(fabsf(buf[i].x), fabsf(buf[i].y)), fmaxf(fabsf(buf[i].z), fabsf(buf[i].w))));
    m = wave_max(m);
    {
      const int E = max((int)(__float_as_uint(m) >> 23) & 0xff, 15 + H2_TABLE_EXP);
      if (E > line_E) {
        if (line_E > 0) {
          const float f = __uint_as_float((unsigned)(127 + line_E - E) << 23);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
              for (int j = 0; j < 4; ++j) tot[mt][nt][j] *= (E - line_E < 126 ? f : 0.f);
        }
        line_E = E;
      }
    }
    const float scale = __uint_as_float((unsigned)(268 - line_E) << 23);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      union { f16x8 v; struct { uint2 a, b; } u; } H, L;
      h2_split4(buf[0][e] * scale, buf[1][e] * scale, buf[2][e] * scale, buf[3][e] * scale, H.u.a, L.u.a);
      h2_split4(buf[4][e] * scale, buf[5][e] * scale, buf[6][e] * scale, buf[7][e] * scale, H.u.b, L.u.b);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const char* ta = smem + (s * MT + mt) * 2048 + l * 16;
        const f16x8 ah = *reinterpret_cast<const f16x8*>(ta), al = *reinterpret_cast<const f16x8*>(ta + 1024);
        tot[mt][e] = h2_mfma32(ah, al, H.v, L.v, tot[mt][e]);
      }
    }
  };
  // a finished line: row 16 mt + 4 g + j of the spectrum, channels 4 li .. 4 li + 3 (accumulator column li of tot[mt][e] is
  // channel 4 li + e), 256 contiguous bytes per 16 lanes; and the line's maximum for the mode mix
  auto finish = [&](f32x4v (&tot)[MT][4], int line_E, float* __restrict__ spec, float* __restrict__ amax, long z) {
    float* __restrict__ sp = spec + z * (long)P.R * 64;
    const float inv = __uint_as_float((unsigned)(line_E - 14 - H2_TABLE_EXP) << 23);
    float am = 0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = 16 * mt + 4 * g + j;
        if (row < P.R)
          *reinterpret_cast<float4*>(sp + row * 64 + 4 * li) =
              make_float4(tot[mt][0][j] * inv, tot[mt][1][j] * inv, tot[mt][2][j] * inv, tot[mt][3][j] * inv);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) am = fmaxf(am, fabsf(tot[mt][nt][j]));
      }
    am = wave_max(am);
    if (l == 0 && amax) amax[z] = am * inv;
  };

  f32x4v tota[MT][4], totb[MT][4];                         // the line of the first / the second chunk
  int Ea = 0, Eb = 0;
  f32x4v ba[8], bb[8];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // (the table copy above: from here on the queue is counted by hand)
  issue(ba, 0, 0);
  issue(bb, 0, 1);
  for (long u = 0; u < units; ++u) {
    const int sb = (int)(u / nb), t = (int)(u - (long)sb * nb);
    const long z = (long)(xg + P.ng * sb) * n + gw;         // this wave's line of the sample, as a row and as a column
    if (t == 0) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) tota[mt][nt] = totb[mt][nt] = (f32x4v){0.f, 0.f, 0.f, 0.f};
      Ea = Eb = 0;
    }
    const float* q_; long st_;
    const int sa = chunk_of(u, 0, q_, st_), sbk = chunk_of(u, 1, q_, st_);
#ifdef RPDE_STAMPS
    // rounds 9 .. 12 (second sample) of wave 3 of workgroups 96 .. 159: 7 stamps each
    const bool stamp_on = l == 0 && wave == 3 && blockIdx.x >= 96 && blockIdx.x < 160 && u >= 9 && u < 13;
    const int stamp_slot = (int)blockIdx.x - 96, sq0 = (int)(u - 9) * 7;
#endif
    FSTAMP(0, sq0 + 0);
    asm volatile("s_barrier" ::: "memory");      // (keeps the eight waves of a workgroup in one round)
    FSTAMP(0, sq0 + 1);
    landed(ba);
    FSTAMP(0, sq0 + 2);
    process(ba, sa, tota, Ea);
    FSTAMP(0, sq0 + 3);
    issue(ba, u + 1, 0);
    landed(bb);
    FSTAMP(0, sq0 + 4);
    process(bb, sbk, totb, Eb);
    FSTAMP(0, sq0 + 5);
    issue(bb, u + 1, 1);
    FSTAMP(0, sq0 + 6);
    if (t == nb - 1) {
      finish(tota, Ea, row_first ? P.spec_y : P.spec_x, row_first ? P.amax_y : P.amax_x, z);
      finish(totb, Eb, row_first ? P.spec_x : P.spec_y, row_first ? P.amax_x : P.amax_y, z);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // (the re-reads past the end)
}

// ------------------------------------------------------------------------------------------------------------
// split: fp32 spectra [line][R][64] -> operand blocks [line][16-channel block] (layout above) + 1/scale per line
// ------------------------------------------------------------------------------------------------------------
template <int K32, int TG>
__global__ __launch_bounds__(256) void k_spec_split_h2(const float* __restrict__ spec, char* __restrict__ img,
                                                       float* __restrict__ inv_out, int R) {
  typedef H2Block<K32, TG> L;
  constexpr int NF = K32 + (TG ? 1 : 0);
  __shared__ float wmax[4];
  const long line = blockIdx.x;
  const int tid = threadIdx.x, l = tid & 63, cb = tid >> 6, g = l >> 4, li = l & 15;
  const float* __restrict__ src = spec + line * (long)R * 64 + 16 * cb + li;
  float v[NF][8];
  float m = 0.f;
#pragma unroll
  for (int s = 0; s < NF; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 32 * s + 8 * g + j;
      v[s][j] = k < R ? src[k * 64] : 0.f;
      m = fmaxf(m, fabsf(v[s][j]));
    }
  m = wave_max(m);
  if (l == 0) wmax[cb] = m;
  __syncthreads();
  m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  float scale, inv;
  h2_scale(m, H2_TABLE_EXP, scale, inv);
  if (tid == 0) inv_out[line] = inv;
  char* blk = img + (line * 4 + cb) * (long)L::BYTES;
#pragma unroll
  for (int s = 0; s < NF; ++s) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[s][j] *= scale;
    uint4 hi, lo;
    h2_split8(v[s], hi, lo);
    if (s < K32) {
      *reinterpret_cast<uint4*>(blk + L::hi(s) + l * 16) = hi;
      *reinterpret_cast<uint4*>(blk + L::lo(s) + l * 16) = lo;
    } else if (g < TG) {
      L::template store_tail<false>(blk, g, li, hi, lo);
    }
  }
  if (TG > 0 && g == 0) L::zero_unused(blk, li);
}

// ------------------------------------------------------------------------------------------------------------
// synthesis of both axes
// ------------------------------------------------------------------------------------------------------------
struct SynP {
  const char* imgy; const char* imgx;     // B fragments of the y lines (b,m) and the x lines (b,n)
  const float* invy; const float* invx;   // 1 / (line scale * table scale)
  const char* taby; const char* tabx;     // synthesis-type table fragments: rows n (y axis, length N), rows m (x axis, length M)
  float* out; const float* skip;          // [B,M,N,64]; optional tensor added to the result
  int B, M, N;
  int sy, sx;                              // super-tile of sy x sx tiles (divide M/16, N/16): what one XCD has in flight
};

// one operand block in registers
template <int K32, int TG>
struct Frag {
  typedef H2Block<K32, TG> L;
  static constexpr int NP = L::NP;
  f16x8 h[K32 > 0 ? K32 : 1], lo[K32 > 0 ? K32 : 1], pk[NP > 0 ? NP : 1];
  __device__ __forceinline__ void load(const char* __restrict__ p, int l) {
#pragma unroll
    for (int s = 0; s < K32; ++s) {
      h[s] = *reinterpret_cast<const f16x8*>(p + L::hi(s) + l * 16);
      lo[s] = *reinterpret_cast<const f16x8*>(p + L::lo(s) + l * 16);
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      constexpr int full = 3 * TG / 4;               // packed fragments with all four lane groups in use
      const int slots = q < full ? 4 : 3 * TG - 4 * full;
      const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      pk[q] = z;
      if ((l >> 4) < slots) pk[q] = *reinterpret_cast<const f16x8*>(p + L::pk(q) + l * 16);
    }
  }
};

// float index of element (m, n, c) of a wave's 16 x 16 x 16 turning buffer: the n slot is XOR-ed so that both the
// writes (lanes differ in c and m>>2) and the reads (lanes differ in c and n>>2) touch 32 different banks
__device__ __forceinline__ int turn_idx(int m, int n, int c) {
  return m * 256 + ((n ^ ((m >> 2) & 1) ^ ((n >> 2) & 1)) << 4) + c;
}

template <int K32, int TG>
__global__ __launch_bounds__(256, 2) void k_dft_synthesis2_h2(const SynP P) {
  constexpr int BB = h2_block_bytes(K32, TG);
  constexpr long LB = 4L * BB;                 // bytes per line: 4 channel blocks
  __shared__ __attribute__((aligned(16))) float turn[4 * 4096];
  const int tid = threadIdx.x, l = tid & 63, cb = tid >> 6, g = l >> 4, li = l & 15;
  // tile: groups of 8 samples, one per XCD (blocks b, b+8, .. share an L2)
  const int tn = P.N >> 4, tps = (P.M >> 4) * tn;
  const long group = 8L * tps;
  const int blk = (int)(blockIdx.x / group);
  const int r0 = (int)(blockIdx.x - blk * group);
  const int nb = min(8, P.B - 8 * blk);
  const int b = 8 * blk + r0 % nb, t = r0 / nb;
  if (t >= tps) return;
  // tiles of a sample go super-tile by super-tile (8 x 8 tiles = the 64 workgroups an XCD runs at once): the lines a
  // super-tile needs, (sy + sx) * 16, fit in the XCD's L2 and each is fetched from beyond it once per super-tile
  const int per_st = P.sy * P.sx, st = t / per_st, wi = t - st * per_st;
  const int stn = tn / P.sx;
  const int m0 = ((st / stn) * P.sy + wi / P.sx) << 4, n0 = ((st % stn) * P.sx + wi % P.sx) << 4;
  float* const buf = turn + cb * 4096;
#ifdef RPDE_STAMPS
  const long stamp_first = ((long)gridDim.x / 2) & ~63L;
  const bool stamp_on = l == 0 && cb == 0 && blockIdx.x >= stamp_first && blockIdx.x < stamp_first + 64;
  const int stamp_slot = (int)(blockIdx.x - stamp_first);
#endif
  FSTAMP(1, 0);

  typedef Frag<K32, TG> F;
  F tx, ty;
  tx.load(P.tabx + (long)(m0 >> 4) * BB, l);        // rows m0.. of the x-axis table
  ty.load(P.taby + (long)(n0 >> 4) * BB, l);        // rows n0.. of the y-axis table

  // 32 lines: 0..15 are the columns n0 + i of the x-axis part ([16 m][16 c] tiles, written to the turning buffer),
  // 16..31 the rows m0 + i of the y-axis part ([16 n][16 c] tiles, added to the turned x part in the buffer).
  const long zx = (long)b * P.N + n0, zy = (long)b * P.M + m0;
  const char* __restrict__ srcx = P.imgx + zx * LB + cb * BB;
  const char* __restrict__ srcy = P.imgy + zy * LB + cb * BB;
  // the 32 line scales in one vector load each (a scalar load per line would put its latency on every step)
  const float invx_l = P.invx[zx + li], invy_l = P.invy[zy + li];
  // lines go through in groups of four whose MFMA chains are interleaved; the next group's fragments are in flight
  // (three groups in flight -- 12 lines, 238 VGPRs -- measured the same 338 us inside the training step: the kernel
  //  is bound by the bandwidth between the L2 / Infinity Cache and the CUs, not by the latency of these loads)
  F f[8];
  auto line_src = [&](int i) { return i < 16 ? srcx + i * LB : srcy + (i - 16) * LB; };
#pragma unroll
  for (int u = 0; u < 4; ++u) f[u].load(line_src(u), l);
#pragma unroll
  for (int gi = 0; gi < 8; ++gi) {
    if (gi + 1 < 8) {
#pragma unroll
      for (int u = 0; u < 4; ++u) f[((gi + 1) * 4 + u) & 7].load(line_src((gi + 1) * 4 + u), l);
    }
    const F& tab = gi < 4 ? tx : ty;
    f32x4v c[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) c[u] = (f32x4v){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < F::NP; ++q)
#pragma unroll
      for (int u = 0; u < 4; ++u) c[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(tab.pk[q], f[(gi * 4 + u) & 7].pk[q], c[u], 0, 0, 0);
#pragma unroll
    for (int s = K32 - 1; s >= 0; --s) {
#pragma unroll
      for (int u = 0; u < 4; ++u) c[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(tab.lo[s], f[(gi * 4 + u) & 7].h[s], c[u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < 4; ++u) c[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(tab.h[s], f[(gi * 4 + u) & 7].lo[s], c[u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < 4; ++u) c[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(tab.h[s], f[(gi * 4 + u) & 7].h[s], c[u], 0, 0, 0);
    }
    FSTAMP(1, 1 + 2 * gi);
    if (gi == 4) wave_lds_fence();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = gi * 4 + u;
      if (gi < 4) {
        const float sc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(invx_l), i));
#pragma unroll
        for (int j = 0; j < 4; ++j) buf[turn_idx(4 * g + j, i, li)] = c[u][j] * sc;
      } else {
        const int r = i - 16;
        const float sc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(invy_l), r));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int ix = turn_idx(r, 4 * g + j, li);
          buf[ix] = fmaf(c[u][j], sc, buf[ix]);
        }
      }
    }
    FSTAMP(1, 2 + 2 * gi);
  }
  wave_lds_fence();
  FSTAMP(1, 17);
  // the finished [16 m][16 n][16 c] tile leaves as 16-byte pieces: lane -> point n = l >> 2, channels 4 (l & 3) ..
  {
    const int n = l >> 2, c4 = (l & 3) << 2;
    const long o = (zy * P.N + n0 + n) * 64 + 16 * cb + c4;
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      float4 v = *reinterpret_cast<const float4*>(buf + turn_idx(m, n, c4));
      const long oo = o + (long)m * P.N * 64;
      if (P.skip) {
        const float4 k = *reinterpret_cast<const float4*>(P.skip + oo);
        v.x += k.x; v.y += k.y; v.z += k.z; v.w += k.w;
      }
      *reinterpret_cast<float4*>(P.out + oo) = v;
    }
  }
  FSTAMP(1, 18);
}

// ------------------------------------------------------------------------------------------------------------
// synthesis of both axes, persistent 64-row tiles (rounds 3 and 4): one scaffold, two tile shapes
// ------------------------------------------------------------------------------------------------------------
// k_dft_synthesis2_h2 gives every wave a 16 x 16 x 16-channel tile and lets it fetch its 32 spectrum lines itself:
// 5.5 bytes loaded from L2 per byte stored (3.2 GB per forward at 256^2, B = 32), and that -- not HBM -- bounded it
// (317 us).  The two kernels below give an 8-wave workgroup a tile of 64 rows, so a line's fragments are fetched from
// L2 once per FOUR 16-point tiles.  What they share (SynTile, SynWalk, SynLane):
//   * the lines of the tile stream through a 3-slot LDS ring in stages of 16 fragments, by LDS-DMA (global_load_lds:
//     1 KB fragment pieces land lane-linear, exactly as the MFMA wants them; no registers held), two stages ahead; one
//     s_barrier per stage.  The table blocks and the line scales travel the same way (a 12 KB corner of LDS that holds
//     the x-axis table during the x phase and the y-axis table after it): no ordinary global load for an operand
//     anywhere, so the compiler never drains the DMA queue for one.  The waits are counted (cw.h).
//   * wave (mt, p) owns 128 accumulator registers.  Stages 0-3 form the x-axis part column by column (accumulator rows
//     = m), the later stages the y-axis part row by row (accumulator rows = n).  Between them the x part is turned into
//     the y layout INSIDE the register file: both layouts keep the channel on lane & 15, so the turn is sixteen 4 x 4
//     transposes between the register index and the lane-row index -- two v_permlane32_swap + two v_permlane16_swap
//     each.  No LDS turning buffer (k_dft_synthesis2_h2 spends ~200 LDS instructions and 2.1 M bank-conflict cycles
//     per launch there).
//   * persistent: one workgroup per CU walks over its share of the items, and the ring never runs dry -- the first two
//     stages (and the tables) of the NEXT tile are requested during the last stages of the current one.  In-kernel
//     stamps of the first, one-tile-per-workgroup version: 33 % of a workgroup's life was the cold start of its DMA
//     queue, 29 % the burst of stores at its end.
//   * every line carries its own power-of-two scale (undone on the accumulators).
// What differs is the tile (a geometry trait each: item_at, issue_piece, issue_table, issue_inv), the y phase, the way
// out, and the style of the stage loop:
//   k_dft_synthesis3_h2  64 x 64 points x 16 channels, 8 stages, 1.5 bytes of fragments per byte stored.  Wave (mt, p)
//     owns the 16-row block mt and the two 16-column blocks p, p + 2.  It serves the adjoint with a skip gradient: loads
//     of the skip gradient + stores in four batches after the last stage, 16 bytes per lane (a 4 x 4 transpose inside
//     each quad of lanes gives every lane four consecutive channels of one point).  (The retired forward instances
//     spread the stores over the eight stages instead; the measurements below are theirs.)  What bounds it (measured
//     with the parts switched off one at a time, 256^2, B = 32): DMA skeleton alone 76 us, + MFMAs 25 us, + stores
//     130 us; HBM traffic 0.30 GB read + 0.54 GB written in 215-230 us.  Burst or spread, in step or staggered across
//     XCDs, 4-byte or 16-byte stores: the store time adds to the rest (a CU's memory pipeline takes a 16-segment store
//     instruction in ~60-90 cycles and DMA pieces through the same queue).
//   k_dft_synthesis4_h2  64 x 32 points x 32 channels, 12 stages; forward and adjoint without a skip gradient.
//     Kernel 3 owns 16 channels of its points, so every store instruction writes sixteen 64-byte segments -- half cache
//     lines -- and a CU's memory pipeline takes such an instruction at a quarter of the rate of one that writes eight
//     whole 128-byte lines (profiles/ubench/storepat.hip: 37 vs 135 GB/s per CU); with the stores in, that kernel ran
//     225 us against 100 us without them.  Here a workgroup owns a PAIR of channel blocks (32 channels = one 128-byte
//     line per point) -- the same 128 accumulator registers per lane -- at the price of 2.25 instead of 1.5 bytes of
//     fragments fetched from L2 per byte stored (the fragments of a channel pair of a sample, 3.1 MB at 256^2, still
//     fit the XCD's L2 while all its tiles use them).  Wave (mt, p) owns rows 16 mt .., columns 16 p .. of the tile for
//     BOTH channel blocks a = 0, 1: acc[a][i][jj].  x stages 0-3 (channel block s >> 1, columns 8 (s & 1) .. + 7 of
//     both column blocks), y stages 4-11 (rows 2 (s - 4), + 1 of the four row blocks, both channel blocks).
//     12 = 0 mod 3: the ring position is the same for every tile.  A row is final after its y stage and leaves right
//     there: four store instructions per wave and y stage, each eight points x 128 bytes.  The 4 x 4 quad transpose that
//     gives a lane four consecutive channels of one point takes its four inputs from BOTH channel blocks -- (a, column)
//     = (0, 0), (0, 1), (1, 0), (1, 1) -- so the lanes of a quad end up with the two 64-byte halves of two points'
//     lines: no exchange beyond the transpose itself.
//     Tried on top and dropped (same-box, 256^2, B = 32; profiles/r04_synthesis_variants.txt): requesting ALL pieces of
//     stage s + 2 right behind the barrier and issuing the stores of a stage's rows one stage later, behind the next
//     requests, so that a store has three stages instead of two to be acknowledged before a wait on younger pieces
//     covers it (the counter is in order) and no request queues behind a burst of stores: 225-230 us against 219 us.
//     Neither the store segment (this kernel against kernel 3: 219 vs 224-235 us), nor the fragment volume (2.25 vs 1.5
//     bytes per byte stored), nor the store window moves the time; the same store pattern alone streams at 6.2 TB/s =
//     87 us (profiles/ubench/storepat.hip, pattern C / D).  What is left is that ONE workgroup per CU runs all its
//     waves through the same phase at the same time -- wait for pieces | fragments + matrix work | transposes + stores
//     -- so the three add up instead of overlapping.
// Both kernels are sensitive to how they compile; the shared pieces are the ones that leave every instance's instruction
// stream as it was (profiles/isa_streams.py, profiles/synthesis_fold_ab.txt).
constexpr int SYN3_WAVES = 8;

// one item: one tile of one channel block (kernel 3) / channel pair (kernel 4) of one sample
struct SynItem {
  const char* gx; const char* gy;       // fragment pieces of the tile's first column / first row (first channel block)
  const char* tx; const char* ty;       // table blocks of the tile's first 16 rows / first 16 columns
  const float* ivx; const float* ivy;   // line scales of the tile's columns / rows
  long o;                               // float offset of the tile's first point, first channel of the item
};

// a lane's place in the workgroup
struct SynLane {
  int l, w, g, li, mt, p;
  unsigned lane16;
  __device__ static __forceinline__ SynLane here() {
    const int tid = threadIdx.x, l = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    return {l, w, l >> 4, l & 15, w & 3, w >> 2, (unsigned)(l * 16)};
  }
};

// this workgroup's items.  Blocks b, b + ng, .. share an XCD (an L2): group xg = blockIdx % ng takes the samples
// xg, xg + ng, ..; its nj workgroups take the items (wps per sample) round-robin from jw, so the ~32 in flight are
// neighbours that share spectrum lines.  (Placement is a speed matter only.)
struct SynWalk {
  int ng, xg, jw, nj;
  long nitems;
  __device__ __forceinline__ SynWalk(const SynP& P, int wps)
      : ng(P.sy), xg(blockIdx.x % ng), jw(blockIdx.x / ng), nj(gridDim.x / ng), nitems((long)((P.B - xg + ng - 1) / ng) * wps) {}
};

template <int K32, int TG>
struct SynTile {
  typedef H2Block<K32, TG> L;
  typedef Frag<K32, TG> F;
  static constexpr int NP = L::NP, NF = L::NF, BB = L::BYTES;
  static constexpr long LB = 4L * BB;             // bytes per line: 4 channel blocks
  static constexpr int SLOT = 16 * BB;            // one stage: 16 fragments
  static_assert(NF <= 3, "ring of three 16-fragment slots + the table corner must fit 160 KB");
  static constexpr int TAB = 3 * SLOT, INV = TAB + 4 * BB, LDS_BYTES = INV + 512;

  // operands of the LDS-DMA builtin
  typedef __attribute__((address_space(3))) void* lds_ptr;
  typedef const __attribute__((address_space(1))) void* glb_ptr;
  // one operand block from LDS (base = block + 16 * lane)
  __device__ static __forceinline__ void lds_frag(F& f, const char* base) {
#pragma unroll
    for (int s2 = 0; s2 < K32; ++s2) {
      f.h[s2] = *reinterpret_cast<const f16x8*>(base + L::hi(s2));
      f.lo[s2] = *reinterpret_cast<const f16x8*>(base + L::lo(s2));
    }
#pragma unroll
    for (int qq = 0; qq < NP; ++qq) f.pk[qq] = *reinterpret_cast<const f16x8*>(base + L::pk(qq));
  }
  // the three h2 terms of table block x line block, small terms first
  __device__ static __forceinline__ f32x4v chain(const F& tab, const F& f) {
    f32x4v c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int qq = 0; qq < NP; ++qq) c = __builtin_amdgcn_mfma_f32_16x16x32_f16(tab.pk[qq], f.pk[qq], c, 0, 0, 0);
#pragma unroll
    for (int s2 = K32 - 1; s2 >= 0; --s2) {
      c = __builtin_amdgcn_mfma_f32_16x16x32_f16(tab.lo[s2], f.h[s2], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_f16(tab.h[s2], f.lo[s2], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_f16(tab.h[s2], f.h[s2], c, 0, 0, 0);
    }
    return c;
  }
  // x stage s < 4: the eight columns 8 (s & 1) .. of the wave's column block in slot (= ring slot + 16 * lane), into
  // acc[s >> 1][8 (s & 1) ..][jj] (rows m = 4g + jj); request(c8) between the chains.  Line fragments are read one line ahead of
  // their MFMAs, no further (the compiler barrier keeps the LDS reads of later lines from being hoisted on top of 128
  // live accumulators)
  template <class Req>
  __device__ static __forceinline__ void x_stage(const SynLane& ln, int s, const char* slot, const F& tx, F (&fq)[2],
                                                 float (&acc)[2][16][4], Req&& request) {
    const int a = s >> 1, h = s & 1;
    lds_frag(fq[0], slot + (ln.p * 8) * BB);
#pragma unroll
    for (int c8 = 0; c8 < 8; ++c8) {
      if (c8 + 1 < 8) lds_frag(fq[(c8 + 1) & 1], slot + (ln.p * 8 + c8 + 1) * BB);
      asm volatile("" ::: "memory");
      const f32x4v c = chain(tx, fq[c8 & 1]);
      request(c8);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) acc[a][8 * h + c8][jj] = c[jj];
    }
  }
  // x part of one 16 x 16 block -> true units (column i times lane i of invx), then turned into the y layout: physical
  // register [4 (r >> 2) + j][r & 3] then holds row r, column 4g + j
  __device__ static __forceinline__ void turn(float (&acc)[16][4], const float& invx) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float sc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(invx), i));
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) acc[i][jj] *= sc;
    }
#pragma unroll
    for (int jy = 0; jy < 4; ++jy)
#pragma unroll
      for (int jr = 0; jr < 4; ++jr) {
        swap_halves(acc[jy][jr], acc[8 + jy][jr]);
        swap_halves(acc[4 + jy][jr], acc[12 + jy][jr]);
        swap_rows(acc[jy][jr], acc[4 + jy][jr]);
        swap_rows(acc[8 + jy][jr], acc[12 + jy][jr]);
      }
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) pin(acc[i][jj]);
  }
};

// ---- kernel 3's tile: 64 x 64 points x 16 channels, (M / 64) (N / 64) 4 items per sample ----
template <int K32, int TG>
struct Syn3Geom {
  typedef SynTile<K32, TG> T;
  // piece i (of 2 NF) of this wave for stage s of a tile: stage s < 4: columns 8 (s & 1) .. + 7 of the column blocks
  // (s >> 1) * 2 + {0, 1}; stage s >= 4: rows 4 (s - 4) .. + 3 of the four row blocks
  __device__ static __forceinline__ void issue_piece(char* smem, const SynLane& ln, const SynItem& it, int s, int i, int slot) {
    constexpr int NF = T::NF;
    const int idx = ln.w + 8 * i, ell = idx / NF, f = idx - ell * NF;     // (ell * NF + f == idx: pieces land in order)
    const char* src;
    if (s < 4) src = it.gx + (long)(16 * ((ell >> 3) + 2 * (s >> 1)) + 8 * (s & 1) + (ell & 7)) * T::LB + f * 1024;
    else src = it.gy + (long)(16 * (ell >> 2) + 4 * (s - 4) + (ell & 3)) * T::LB + f * 1024;
    __builtin_amdgcn_global_load_lds((typename T::glb_ptr)(src + ln.lane16), (typename T::lds_ptr)(smem + slot * T::SLOT + idx * 1024), 16, 0, 0);
  }
  // the four 16-row blocks of a table (x axis: rows m0 .. m0 + 63; y axis: the column blocks p + 2a at [p * 2 + a])
  __device__ static __forceinline__ void issue_table(char* smem, const SynLane& ln, const char* tab, bool yaxis) {
    constexpr int NF = T::NF;
#pragma unroll
    for (int i = 0; i < (4 * NF + 7) / 8; ++i) {
      const int idx = ln.w + 8 * i;
      if (idx < 4 * NF) {
        const int blk = idx / NF, f = idx - blk * NF;
        const int src_blk = yaxis ? (blk >> 1) + 2 * (blk & 1) : blk;
        __builtin_amdgcn_global_load_lds((typename T::glb_ptr)(tab + (long)src_blk * T::BB + f * 1024 + ln.lane16), (typename T::lds_ptr)(smem + T::TAB + idx * 1024), 16, 0, 0);
      }
    }
  }
  __device__ static __forceinline__ void issue_inv(char* smem, const SynLane& ln, const SynItem& it) {          // 64 + 64 floats, one 4-byte DMA each
    if (ln.w == 6) __builtin_amdgcn_global_load_lds((typename T::glb_ptr)(it.ivx + ln.l), (typename T::lds_ptr)(smem + T::INV), 4, 0, 0);
    if (ln.w == 7) __builtin_amdgcn_global_load_lds((typename T::glb_ptr)(it.ivy + ln.l), (typename T::lds_ptr)(smem + T::INV + 256), 4, 0, 0);
  }
};

template <int K32, int TG>
__global__ __launch_bounds__(64 * SYN3_WAVES, 2) void k_dft_synthesis3_h2(const SynP P) {
  typedef SynTile<K32, TG> T;
  typedef Syn3Geom<K32, TG> G;
  typedef typename T::F F;
  constexpr int NF = T::NF, BB = T::BB, SLOT = T::SLOT, TAB = T::TAB, INV = T::INV;
  __shared__ __attribute__((aligned(16))) char smem[T::LDS_BYTES];
  // (decomposed here, not by SynLane::here(): through it the instances with two fragment pieces spill one scalar less)
  const int tid = threadIdx.x, l = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), g = l >> 4, li = l & 15;
  const int mt = w & 3, p = w >> 2;
  const SynLane ln = {l, w, g, li, mt, p, (unsigned)(l * 16)};
  // (item_at stays here: as a member of Syn3Geom, like Syn4Geom's, the items-per-sample product compiles differently)
  const int tn = P.N >> 6, wps = (P.M >> 6) * tn * 4;
  const SynWalk wk(P, wps);
  auto item_at = [&](long q) {
    SynItem it;
    const int sb = (int)(q / wps), t = (int)(q - (long)sb * wps);
    // channel blocks in pairs: first every tile of the sample for blocks 0 and 1, then for 2 and 3.  The ~32 workgroups
    // of a group then work on ONE pair at a time -- the pair's fragments of a 256^2 sample (3.2 MB) stay in the 4 MB L2
    // while all sixteen tiles use them (with the four blocks of a tile side by side only half of a sample's tiles ran
    // together and the other half fetched the lines again: 319 MB for 201 MB of operands) -- and the two blocks of a
    // pair still complete each other's 128-byte lines in L2.
    const int half = wps >> 1, hb = t / half, r = t - hb * half;
    const int b = wk.xg + wk.ng * sb, cb = 2 * hb + (r & 1), tile = r >> 1;
    const int m0 = (tile / tn) << 6, n0 = (tile % tn) << 6;
    it.gx = P.imgx + ((long)b * P.N + n0) * T::LB + cb * BB;
    it.gy = P.imgy + ((long)b * P.M + m0) * T::LB + cb * BB;
    it.tx = P.tabx + (long)(m0 >> 4) * BB;
    it.ty = P.taby + (long)(n0 >> 4) * BB;
    it.ivx = P.invx + (long)b * P.N + n0;
    it.ivy = P.invy + (long)b * P.M + m0;
    it.o = (((long)b * P.M + m0) * P.N + n0) * 64 + 16 * cb;
    return it;
  };
  long q = wk.jw;
  if (q >= wk.nitems) return;
  SynItem cur = item_at(q);
  auto issue_piece = [&](const SynItem& it, int s, int i, int slot) { G::issue_piece(smem, ln, it, s, i, slot); };
  // ---- prologue: tables / scales of the first tile, then its first two stages (in place in both kernels: as a shared
  // function it changes every instance's schedule) ----
  G::issue_table(smem, ln, cur.tx, false);
  G::issue_inv(smem, ln, cur);
#pragma unroll
  for (int i = 0; i < 2 * NF; ++i) issue_piece(cur, 0, i, 0);
  cw_mark<3>();                 // (tags 3 / 4: the first tile's stages 0 / 1, waited for under `first` -- a path-insensitive
#pragma unroll                  //  check cannot know that `first` and "came from the prologue" are the same thing)
  for (int i = 0; i < 2 * NF; ++i) issue_piece(cur, 1, i, 1);
  cw_mark<4>();
  int ring = 0;                 // slot of the current tile's stage 0
  bool first = true;
  const int qd = li >> 2, pl = li & 3;
  // acc[a][i][jj]: x phase -- column i of column block a, rows m = 4g + jj; after the turn, physical register
  // [a][4 (r >> 2) + j][r & 3] holds row r, column 4g + j
  float acc[2][16][4];

  while (true) {
    const long qn = q + wk.nj;
    const bool has_next = qn < wk.nitems;
    SynItem nxt = cur;
    if (has_next) nxt = item_at(qn);
    F tx, ty[2];
    F fq[2];
    float invx_l[2], invy_l;
    // output: after the quad transpose lane (g, 4 qd + pl) holds channels 4 qd .. + 3 of the point (row r, column
    // 16 (p + 2a) + 4g + pl)
    const long o = cur.o + ((long)(16 * mt) * P.N + 16 * p + 4 * g + pl) * 64 + 4 * qd;
    auto tile_out = [&](int r, int a) {
      float4 v = make_float4(acc[a][4 * (r >> 2) + 0][r & 3], acc[a][4 * (r >> 2) + 1][r & 3], acc[a][4 * (r >> 2) + 2][r & 3],
                             acc[a][4 * (r >> 2) + 3][r & 3]);
      quad_transpose(v.x, v.y, v.z, v.w);
      return v;
    };
#ifdef RPDE_STAMPS
    const bool stamp_on = l == 0 && w == 5 && blockIdx.x >= 96 && blockIdx.x < 160 && q == wk.jw + 2 * (long)wk.nj;
    const int stamp_slot = (int)blockIdx.x - 96;
#endif
    FSTAMP(1, 0);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      // ---- this wave's pieces of stage s have landed.  vmcnt(N): everything but the N youngest operations of this wave
      // is done; younger than the pieces of stage s are the pieces of stage s + 1 (2 NF); a wait that also covers table /
      // scale pieces issued in between only over-waits
      // (cw.h: the requests of stage s are marked with the tag s % 3 behind their last piece, and the ISA test checks
      //  these counts on the compiled code)
      const int T3 = s % 3;
      // (every stage requests its pieces, the last tile's stages 6 / 7 a harmless re-read: no count depends on has_next.
      //  The arms below that wait alike are kept apart on purpose: merged, they compile to other register assignments.)
      if (!first && s < 2) cw_wait_t<63>(T3);                      // (behind the 64 loads / stores of the epilogue)
      else if (first && s < 2) { if (s == 0) cw_wait<3, 2 * NF>(); else cw_wait<4, 2 * NF>(); }
      else if (first && s < 5) cw_wait_t<2 * NF>(T3);
      else if (s == 0 || s == 1 || s == 6) cw_wait_t<2 * NF>(T3);
      else if (s <= 5) cw_wait_t<2 * NF>(T3);
      else cw_wait_t<2 * NF>(T3);
      FSTAMP(1, 1 + 3 * s);
      lds_barrier();                                               // everyone's have; everyone is done with stage s - 1
      FSTAMP(1, 2 + 3 * s);
      const int slot_s = (ring + s) % 3, slot_n = (ring + s + 2) % 3;
      // what this stage requests (spread between its MFMA chains): stage s + 2 of this tile, or stage s - 6 of the next
      auto request = [&](int i) {
        if (i >= 2 * NF) return;
        if (s + 2 < 8) issue_piece(cur, s + 2, i, slot_n);
        else issue_piece(nxt, s - 6, i, slot_n);               // (last tile: nxt = cur, a re-read nobody uses)
      };
      // tables: the y-axis blocks replace the x-axis blocks once every wave has its x block in registers (stage 0); the
      // next tile's x blocks and scales replace them once every wave has its y blocks (stage 4)
      if (s == 1) G::issue_table(smem, ln, cur.ty, true);
      if (s == 5 && has_next) { G::issue_table(smem, ln, nxt.tx, false); G::issue_inv(smem, ln, nxt); }
      const char* slot = smem + slot_s * SLOT + l * 16;
      if (s < 4) {
        if (s == 0) {
          T::lds_frag(tx, smem + TAB + mt * BB + l * 16);
          invx_l[0] = *reinterpret_cast<const float*>(smem + INV + (16 * p + li) * 4);
          invx_l[1] = *reinterpret_cast<const float*>(smem + INV + (16 * (p + 2) + li) * 4);
          invy_l = *reinterpret_cast<const float*>(smem + INV + 256 + (16 * mt + li) * 4);
        }
        const int a = s >> 1, h = s & 1;
        T::lds_frag(fq[0], slot + (p * 8) * BB);
#pragma unroll
        for (int c8 = 0; c8 < 8; ++c8) {
          if (c8 + 1 < 8) T::lds_frag(fq[(c8 + 1) & 1], slot + (p * 8 + c8 + 1) * BB);
          asm volatile("" ::: "memory");
          const f32x4v c = T::chain(tx, fq[c8 & 1]);
          request(c8);
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) acc[a][8 * h + c8][jj] = c[jj];
        }
        cw_mark_t((s + 2) % 3);                        // the pieces of stage s + 2 are all requested
        if (s == 3) {
          // ---- SynTile::turn written out: through the function all five instances are scheduled differently ----
#pragma unroll
          for (int a2 = 0; a2 < 2; ++a2) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const float sc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(invx_l[a2]), i));
#pragma unroll
              for (int jj = 0; jj < 4; ++jj) acc[a2][i][jj] *= sc;
            }
#pragma unroll
            for (int jy = 0; jy < 4; ++jy)
#pragma unroll
              for (int jr = 0; jr < 4; ++jr) {
                swap_halves(acc[a2][jy][jr], acc[a2][8 + jy][jr]);
                swap_halves(acc[a2][4 + jy][jr], acc[a2][12 + jy][jr]);
                swap_rows(acc[a2][jy][jr], acc[a2][4 + jy][jr]);
                swap_rows(acc[a2][8 + jy][jr], acc[a2][12 + jy][jr]);
              }
#pragma unroll
            for (int i = 0; i < 16; ++i)
#pragma unroll
              for (int jj = 0; jj < 4; ++jj) pin(acc[a2][i][jj]);
          }
        }
      } else {
        const int sy = s - 4;
        if (sy == 0) {
          T::lds_frag(ty[0], smem + TAB + ((p * 2 + 0) * NF) * 1024 + l * 16);
          T::lds_frag(ty[1], smem + TAB + ((p * 2 + 1) * NF) * 1024 + l * 16);
        }
        T::lds_frag(fq[0], slot + (mt * 4) * BB);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int r = 4 * sy + rr;
          if (rr + 1 < 4) T::lds_frag(fq[(rr + 1) & 1], slot + (mt * 4 + rr + 1) * BB);
          asm volatile("" ::: "memory");
          const float sc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(invy_l), r));
#pragma unroll
          for (int a = 0; a < 2; ++a) {
            const f32x4v c = T::chain(ty[a], fq[rr & 1]);
            request(2 * rr + a);                                  // (2 NF <= 6 pieces: all out before the stage's stores)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              acc[a][4 * (r >> 2) + j][r & 3] = fmaf(c[j], sc, acc[a][4 * (r >> 2) + j][r & 3]);
              pin(acc[a][4 * (r >> 2) + j][r & 3]);
            }
          }
        }
        cw_mark_t(s + 2 < 8 ? (s + 2) % 3 : (s - 6) % 3);      // the pieces of stage s + 2 (of the next tile: s - 6)
      }
      FSTAMP(1, 3 + 3 * s);
    }
    {
      // the tensor added to the result (the gradient that arrives through the skip connection) is fetched in four
      // batches of 8 float4, each batch a step ahead of the additions and stores it feeds: loads and stores share
      // one in-order counter, so load - add - store per element would wait for every store before the next load
      float4 sk[2][8];
      auto fetch = [&](float4 (&d)[8], int k) {
#pragma unroll
        for (int e = 0; e < 8; ++e) d[e] = *reinterpret_cast<const float4*>(P.skip + o + ((long)(4 * k + (e >> 1)) * P.N + 32 * (e & 1)) * 64);
      };
      fetch(sk[0], 0);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k + 1 < 4) fetch(sk[(k + 1) & 1], k + 1);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int r = 4 * k + (e >> 1), a = e & 1;
          float4 v = tile_out(r, a);
          const float4 q4 = sk[k & 1][e];
          v.x += q4.x; v.y += q4.y; v.z += q4.z; v.w += q4.w;
          *reinterpret_cast<float4*>(P.out + o + ((long)r * P.N + 32 * a) * 64) = v;
        }
      }
    }
    FSTAMP(1, 26);
    if (!has_next) {
      wait_vmcnt<0>();          // (the re-reads of the last two stages must have landed before the LDS is given back)
      break;
    }
    cur = nxt;
    q = qn;
    ring = (ring + 8) % 3;
    first = false;
  }
}

// ---- kernel 4's tile: 64 x 32 points x 32 channels, (M / 64) (N / 32) 2 items per sample: within a sample all tiles of
// channel pair 0, then all of pair 1 (a pair's fragments stay in the group's L2 meanwhile) ----
template <int K32, int TG>
struct Syn4Geom {
  typedef SynTile<K32, TG> T;
  int tn, tiles, wps;
  __device__ __forceinline__ Syn4Geom(const SynP& P) : tn(P.N >> 5), tiles((P.M >> 6) * tn), wps(tiles * 2) {}
  __device__ __forceinline__ SynItem item_at(const SynP& P, const SynWalk& wk, long q) const {
    SynItem it;
    const int sb = (int)(q / wps), t = (int)(q - (long)sb * wps);
    const int hb = t / tiles, tile = t - hb * tiles;
    const int b = wk.xg + wk.ng * sb;
    const int m0 = (tile / tn) << 6, n0 = (tile % tn) << 5;
    it.gx = P.imgx + ((long)b * P.N + n0) * T::LB + (2 * hb) * T::BB;
    it.gy = P.imgy + ((long)b * P.M + m0) * T::LB + (2 * hb) * T::BB;
    it.tx = P.tabx + (long)(m0 >> 4) * T::BB;
    it.ty = P.taby + (long)(n0 >> 4) * T::BB;
    it.ivx = P.invx + (long)b * P.N + n0;
    it.ivy = P.invy + (long)b * P.M + m0;
    it.o = (((long)b * P.M + m0) * P.N + n0) * 64 + 32 * hb;
    return it;
  }
  // piece i (of 2 NF) of this wave for stage s of a tile
  __device__ static __forceinline__ void issue_piece(char* smem, const SynLane& ln, const SynItem& it, int s, int i, int slot) {
    constexpr int NF = T::NF;
    const int idx = ln.w + 8 * i, ell = idx / NF, f = idx - ell * NF;     // fragment ell of the stage, piece f of it
    const char* src;
    if (s < 4) src = it.gx + (long)(16 * (ell >> 3) + 8 * (s & 1) + (ell & 7)) * T::LB + (s >> 1) * T::BB + f * 1024;
    else src = it.gy + (long)(16 * (ell >> 2) + 2 * (s - 4) + ((ell >> 1) & 1)) * T::LB + (ell & 1) * T::BB + f * 1024;
    __builtin_amdgcn_global_load_lds((typename T::glb_ptr)(src + ln.lane16), (typename T::lds_ptr)(smem + slot * T::SLOT + idx * 1024), 16, 0, 0);
  }
  // consecutive 16-row blocks of a table (x axis: the tile's four row blocks; y axis: its two column blocks)
  __device__ static __forceinline__ void issue_table(char* smem, const SynLane& ln, const char* tab, bool yaxis) {
    constexpr int NF = T::NF;
    const int nblk = yaxis ? 2 : 4;
#pragma unroll
    for (int i = 0; i < (4 * NF + 7) / 8; ++i) {
      const int idx = ln.w + 8 * i;
      if (idx < nblk * NF) __builtin_amdgcn_global_load_lds((typename T::glb_ptr)(tab + (long)idx * 1024 + ln.lane16), (typename T::lds_ptr)(smem + T::TAB + idx * 1024), 16, 0, 0);
    }
  }
  __device__ static __forceinline__ void issue_inv(char* smem, const SynLane& ln, const SynItem& it) {          // 32 + 64 floats, one 4-byte DMA each
    if (ln.w == 6 && ln.l < 32) __builtin_amdgcn_global_load_lds((typename T::glb_ptr)(it.ivx + ln.l), (typename T::lds_ptr)(smem + T::INV), 4, 0, 0);
    if (ln.w == 7) __builtin_amdgcn_global_load_lds((typename T::glb_ptr)(it.ivy + ln.l), (typename T::lds_ptr)(smem + T::INV + 256), 4, 0, 0);
  }
};

template <int S> struct StageC { static constexpr int value = S; };

template <int K32, int TG>
__global__ __launch_bounds__(64 * SYN3_WAVES, 2) void k_dft_synthesis4_h2(const SynP P) {
  typedef SynTile<K32, TG> T;
  typedef Syn4Geom<K32, TG> G;
  typedef typename T::F F;
  constexpr int NF = T::NF, BB = T::BB, SLOT = T::SLOT, TAB = T::TAB, INV = T::INV;
  constexpr int NS = 12;                        // stages per tile
  __shared__ __attribute__((aligned(16))) char smem[T::LDS_BYTES];
  const SynLane ln = SynLane::here();
  const int l = ln.l, g = ln.g, li = ln.li, mt = ln.mt, p = ln.p;
  const G geo(P);
  const SynWalk wk(P, geo.wps);
  long q = wk.jw;
  if (q >= wk.nitems) return;
  SynItem cur = geo.item_at(P, wk, q);
  const int w = ln.w;
  const unsigned lane16 = l * 16;
  typedef typename T::glb_ptr glb_ptr; typedef typename T::lds_ptr lds_ptr;
  constexpr long LB = T::LB;
  auto issue_piece = [&](const SynItem& it, int s, int i, int slot) { G::issue_piece(smem, ln, it, s, i, slot); };
  // ---- prologue: tables / scales of the first tile, then its first two stages (in place in both kernels: as a shared
  // function it changes every instance's schedule) ----
  G::issue_table(smem, ln, cur.tx, false);
  G::issue_inv(smem, ln, cur);
#pragma unroll
  for (int i = 0; i < 2 * NF; ++i) issue_piece(cur, 0, i, 0);
  cw_mark<3>();                 // (tags 3 / 4: the first tile's stages 0 / 1, waited for under `first` -- a path-insensitive
#pragma unroll                  //  check cannot know that `first` and "came from the prologue" are the same thing)
  for (int i = 0; i < 2 * NF; ++i) issue_piece(cur, 1, i, 1);
  cw_mark<4>();
  bool first = true;
  const int qd = li >> 2, pl = li & 3;
  // acc[a][i][jj]: x phase -- channel block a, column i of the wave's column block, rows m = 4g + jj; after the turn,
  // physical register [a][4 (r >> 2) + j][r & 3] holds row r, column 4g + j
  float acc[2][16][4];

  while (true) {
    const long qn = q + wk.nj;
    const bool has_next = qn < wk.nitems;
    SynItem nxt = cur;
    if (has_next) nxt = geo.item_at(P, wk, qn);
    F tx, ty;
    F fq[2];
    float invx_l, invy_l;
    // a lane's share of a store instruction: the two points (row r, column 16 p + 4 g + 2 h + (pl & 1)), h = 0, 1; of each
    // the 16 bytes of channels 16 (pl >> 1) + 4 qd .. + 3 of the pair
    const long o = cur.o + ((long)(16 * mt) * P.N + 16 * p + 4 * g + (pl & 1)) * 64 + 16 * (pl >> 1) + 4 * qd;
    auto store_row = [&](long ob, int r) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float4 v = make_float4(acc[0][4 * (r >> 2) + 2 * h][r & 3], acc[0][4 * (r >> 2) + 2 * h + 1][r & 3],
                               acc[1][4 * (r >> 2) + 2 * h][r & 3], acc[1][4 * (r >> 2) + 2 * h + 1][r & 3]);
        quad_transpose(v.x, v.y, v.z, v.w);
        *reinterpret_cast<float4*>(P.out + ob + ((long)r * P.N + 2 * h) * 64) = v;
      }
    };
    // (one call per stage with the stage number as a type: left as a loop of twelve the optimizer gives up unrolling the
    //  instances with three fragment pieces, and the accumulators -- indexed by the stage -- go to scratch memory)
    auto stage = [&](auto stage_c) {
      constexpr int s = decltype(stage_c)::value;
      // ---- this wave's pieces of stage s have landed: all but the N youngest operations of the wave are done; younger
      // than the pieces of stage s are the stores of stage s - 2 (4 if it was a y stage), the pieces of stage s + 1
      // (2 NF) and the stores of stage s - 1; table / scale pieces issued in between only make the wait longer
      // (cw.h: tag = ring slot; tests/test_isa_counted_waits_cpu.py checks these counts on the compiled code)
      constexpr int T3 = s % 3;
      // (every stage requests its 2 NF pieces, the last tile's stages 10 / 11 a harmless re-read: the counts do not
      //  depend on has_next)
      if (s == 0) { if (first) cw_wait<3, 2 * NF>(); else cw_wait<T3, 2 * NF + 8>(); }
      else if (s == 1) { if (first) cw_wait<4, 2 * NF>(); else cw_wait<T3, 2 * NF + 4>(); }
      else if (s <= 4) cw_wait<T3, 2 * NF>();
      else if (s == 5) cw_wait<T3, 2 * NF + 4>();
      else cw_wait<T3, 2 * NF + 8>();
      lds_barrier();                                               // everyone's have; everyone is done with stage s - 1
      const int slot_s = s % 3, slot_n = (s + 2) % 3;
      auto request = [&](int i) {
        if (i >= 2 * NF) return;
        if (s + 2 < NS) issue_piece(cur, s + 2, i, slot_n);
        else issue_piece(nxt, s + 2 - NS, i, slot_n);   // (last tile: nxt = cur, a re-read nobody uses)
      };
      // tables: the y-axis blocks replace the x-axis blocks once every wave has its x block in registers (stage 0); the
      // next tile's x blocks and scales replace them once every wave has its y block (stage 4)
      if (s == 1) G::issue_table(smem, ln, cur.ty, true);
      if (s == 5 && has_next) { G::issue_table(smem, ln, nxt.tx, false); G::issue_inv(smem, ln, nxt); }
      const char* slot = smem + slot_s * SLOT + l * 16;
      if (s < 4) {
        if (s == 0) {
          T::lds_frag(tx, smem + TAB + mt * BB + l * 16);
          invx_l = *reinterpret_cast<const float*>(smem + INV + (16 * p + li) * 4);
          invy_l = *reinterpret_cast<const float*>(smem + INV + 256 + (16 * mt + li) * 4);
        }
        T::x_stage(ln, s, slot, tx, fq, acc, request);
        cw_mark<(s + 2) % 3>();                        // the pieces of stage s + 2 are all requested
        if (s == 3) {
#pragma unroll
          for (int a2 = 0; a2 < 2; ++a2) T::turn(acc[a2], invx_l);
        }
      } else {
        const int sy = s - 4;
        if (sy == 0) T::lds_frag(ty, smem + TAB + p * BB + l * 16);
        T::lds_frag(fq[0], slot + (mt * 4) * BB);
#pragma unroll
        for (int e = 0; e < 4; ++e) {                   // fragment mt * 4 + e: row 2 sy + (e >> 1), channel block e & 1
          const int r = 2 * sy + (e >> 1), a = e & 1;
          if (e + 1 < 4) T::lds_frag(fq[(e + 1) & 1], slot + (mt * 4 + e + 1) * BB);
          asm volatile("" ::: "memory");
          const float sc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(invy_l), r));
          const f32x4v c = T::chain(ty, fq[e & 1]);
          request(2 * e);
          request(2 * e + 1);                           // (2 NF <= 6 pieces: all out before the stage's stores)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc[a][4 * (r >> 2) + j][r & 3] = fmaf(c[j], sc, acc[a][4 * (r >> 2) + j][r & 3]);
            pin(acc[a][4 * (r >> 2) + j][r & 3]);
          }
        }
        cw_mark<(s + 2) % 3>();                        // the pieces of stage s + 2 (of the next tile: s + 2 - 12)
        store_row(o, 2 * sy);
        store_row(o, 2 * sy + 1);
      }
    };
    stage(StageC<0>{}); stage(StageC<1>{}); stage(StageC<2>{}); stage(StageC<3>{});
    stage(StageC<4>{}); stage(StageC<5>{}); stage(StageC<6>{}); stage(StageC<7>{});
    stage(StageC<8>{}); stage(StageC<9>{}); stage(StageC<10>{}); stage(StageC<11>{});
    if (!has_next) {
      wait_vmcnt<0>();          // (the re-reads of the last two stages must have landed before the LDS is given back)
      break;
    }
    cur = nxt;
    q = qn;
    first = false;
  }
}

// ------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------
bool fused2d_ok(int M, int N, int C, int keff_y, int keff_x) {
  const int Ry = 2 * r4(keff_y), Rx = 2 * r4(keff_x);
  if (switch_off("RPDE_FUSED_SPECTRAL")) return false;
  // keff_y == keff_x, not only equal padded counts: the h2 mode mix (k_mix_prep, k_mix_wgrad_fold) zeroes the weights and
  // gradients of modes >= keff with ONE keff for both axes, while the reference clamps each axis by its own length
  // (spectral_convolution.py:269-300) -- e.g. a [64, 32] grid with 20 modes keeps 17 along y and 20 along x
  return C == 64 && M % 32 == 0 && N % 32 == 0 && M <= 32 * ANA_MAXKS && N <= 32 * ANA_MAXKS && keff_y == keff_x && Ry == Rx &&
         Ry <= 48;
}

size_t fused2d_img_bytes(long lines, int R) { return (size_t)lines * 4 * h2_block_bytes(R / 32, (R % 32) / 8); }

// RPDE_ANA_SQ=0: keep the two-read analysis kernel for every shape (A/B, tests).  Default: the one-pass kernel on every
// square grid (its round-3 predecessor, with a workgroup's rows matched to the grid, was level with the two-read kernel
// at 64^2 and 128^2 for B = 32 and ahead at B = 8: 2.03 vs 2.25 ms per training step at 64^2).
static bool ana_sq_ok(int M, int N, int cus) {
  if (switch_off("RPDE_ANA_SQ")) return false;
  return M == N && cus >= 256;
}

int fused2d_analysis(const float* x, float* spec_y, float* spec_x, float* amax_y, float* amax_x, const rpde_plan* py,
                     const rpde_plan* px, int adjoint, int B, int M, int N, hipStream_t st) {
  {
    int cus;
    RPDE_HIP(cu_count(&cus));
    if (ana_sq_ok(M, N, cus) && py->h2_ana[adjoint] == px->h2_ana[adjoint]) {
      // the round-robin schedule: a group = N waves = N / 8 workgroups; as many groups as fit (never more than samples)
      AnaRrP Q;
      Q.x = x; Q.timg = (const char*)py->h2_ana_p[adjoint]; Q.spec_y = spec_y; Q.spec_x = spec_x; Q.amax_y = amax_y; Q.amax_x = amax_x;
      Q.B = B; Q.n = N; Q.nb = N / 32; Q.R = 2 * py->kp;
      const int wpg = N / ANA_WAVES;
      int ng = cus / wpg;
      if (ng < 1) ng = 1;
      Q.ng = B < ng ? B : ng;
      const dim3 grid(wpg * Q.ng), blk(64 * ANA_WAVES);
      const int MTq = (Q.R + 15) / 16;
      if (MTq == 1) hipLaunchKernelGGL(k_dft_analysis_rr_h2<1>, grid, blk, 0, st, Q);
      else if (MTq == 2) hipLaunchKernelGGL(k_dft_analysis_rr_h2<2>, grid, blk, 0, st, Q);
      else hipLaunchKernelGGL(k_dft_analysis_rr_h2<3>, grid, blk, 0, st, Q);
      RPDE_LAUNCH_CHECK();
      return RPDE_OK;
    }
  }
  AnaP P;
  memset(&P, 0, sizeof(P));
  P.x = x; P.naxes = 2; P.B = B; P.R = 2 * py->kp;
  // chunk of samples whose field (read twice) stays inside the 256 MB Infinity Cache beside everything else that
  // streams through it (measured at B = 32, 256^2: no chunking 0.73 ms per forward, 160 MB 0.69, 40-80 MB 0.66)
  const long sample_bytes = (long)M * N * 64 * 4;
  long ch = (64L << 20) / sample_bytes;
  P.chunk = (int)(ch < 1 ? 1 : (ch > B ? B : ch));
  AnaAxis& ay = P.ax[0];
  ay.timg = (const char*)py->h2_ana[adjoint]; ay.spec = spec_y; ay.amax = amax_y; ay.n = N; ay.ks = N / 32; ay.lps = M;
  ay.rps = (M + ANA_WAVES - 1) / ANA_WAVES; ay.zdiv = 1; ay.s1 = (long)N * 64; ay.s2 = 0; ay.ldk = 64;
  AnaAxis& ax = P.ax[1];
  ax.timg = (const char*)px->h2_ana[adjoint]; ax.spec = spec_x; ax.amax = amax_x; ax.n = M; ax.ks = M / 32; ax.lps = N;
  ax.rps = (N + ANA_WAVES - 1) / ANA_WAVES; ax.zdiv = N; ax.s1 = (long)M * N * 64; ax.s2 = 64; ax.ldk = (long)N * 64;
  P.items = ((B + P.chunk - 1) / P.chunk) * P.chunk * (ay.rps + ax.rps);
  // one persistent workgroup per CU (the table + 8 staging areas take 80-112 KB of LDS)
  int cus;
  RPDE_HIP(cu_count(&cus));
  const int grid = P.items < cus ? P.items : cus;
  const int MT = (P.R + 15) / 16;
  if (MT == 1) hipLaunchKernelGGL(k_dft_analysis_h2<1>, dim3(grid), dim3(64 * ANA_WAVES), 0, st, P);
  else if (MT == 2) hipLaunchKernelGGL(k_dft_analysis_h2<2>, dim3(grid), dim3(64 * ANA_WAVES), 0, st, P);
  else hipLaunchKernelGGL(k_dft_analysis_h2<3>, dim3(grid), dim3(64 * ANA_WAVES), 0, st, P);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int fused2d_split(const float* spec, void* img, float* inv, long lines, int R, hipStream_t st) {
  const dim3 grid((unsigned)lines), blk(256);
  h2_dispatch(R, [&](auto k32, auto tg) {
    hipLaunchKernelGGL((k_spec_split_h2<k32(), tg()>), grid, blk, 0, st, spec, (char*)img, inv, R);
  });
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

// RPDE_SYN3=0: keep the 16 x 16 tile kernel for every shape (A/B, tests)
static bool syn3_ok(int M, int N) {
  if (switch_off("RPDE_SYN3")) return false;
  return M % 64 == 0 && N % 64 == 0;
}

int fused2d_synthesis(const void* imgy, const void* imgx, const float* invy, const float* invx, const rpde_plan* py,
                      const rpde_plan* px, int adjoint, float* out, const float* skip, int B, int M, int N, hipStream_t st) {
  SynP P;
  P.imgy = (const char*)imgy; P.imgx = (const char*)imgx; P.invy = invy; P.invx = invx;
  P.taby = (const char*)py->h2_syn[adjoint]; P.tabx = (const char*)px->h2_syn[adjoint];
  P.out = out; P.skip = skip; P.B = B; P.M = M; P.N = N;
  const int R = 2 * py->kp;
  if (syn3_ok(M, N) && 2 * (R / 32) + h2_np((R % 32) / 8) <= 3) {
    // the persistent kernels (three fragments per block at most, R <= 40): one workgroup per CU, in 8 groups (one per
    // XCD; fewer when the batch is smaller); never more per group than the busiest group has items.  Without a skip
    // gradient 64 x 32 x 32-channel tiles, whole 128-byte lines per store: (M / 64) (N / 32) 2 items per sample; with
    // it 64 x 64 x 16-channel tiles, (M / 64) (N / 64) 4 items per sample
    int cus;
    RPDE_HIP(cu_count(&cus));
    const int ng = B < 8 ? B : 8;
    P.sy = ng;
    P.sx = 1;
    const long wps = skip ? (long)(M / 64) * (N / 64) * 4 : (long)(M / 64) * (N / 32) * 2;
    long per_group = cus / ng;
    const long most = (long)((B + ng - 1) / ng) * wps;
    if (per_group > most) per_group = most;
    if (per_group < 1) per_group = 1;
    const dim3 grid((unsigned)(ng * per_group)), blk(64 * SYN3_WAVES);
    h2_dispatch</* UP_TO_40 = */ true>(R, [&](auto k32, auto tg) {
      if (skip) hipLaunchKernelGGL((k_dft_synthesis3_h2<k32(), tg()>), grid, blk, 0, st, P);
      else hipLaunchKernelGGL((k_dft_synthesis4_h2<k32(), tg()>), grid, blk, 0, st, P);
    });
    RPDE_LAUNCH_CHECK();
    return RPDE_OK;
  }
  // (super-tile side, measured at B = 32, 256^2, forward + backward: 2 -> 1.52 ms, 4 -> 1.44, 8 -> 1.45, 16 -> 1.53)
  auto side = [](int tiles) { int s = tiles < 8 ? tiles : 8; while (tiles % s) --s; return s; };
  P.sy = side(M / 16); P.sx = side(N / 16);
  const long tps = (long)(M / 16) * (N / 16);
  const dim3 grid((unsigned)(((B + 7) / 8) * 8 * tps)), blk(256);
  h2_dispatch(R, [&](auto k32, auto tg) { hipLaunchKernelGGL((k_dft_synthesis2_h2<k32(), tg()>), grid, blk, 0, st, P); });
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

}  // namespace rpde

#ifdef RPDE_STAMPS
extern "C" int rpde_debug_fused_stamps(unsigned long long* host_out) {
  RPDE_HIP(hipDeviceSynchronize());
  RPDE_HIP(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(rpde::g_fstamps), sizeof(unsigned long long) * 2 * 64 * 32));
  return RPDE_OK;
}
#endif
