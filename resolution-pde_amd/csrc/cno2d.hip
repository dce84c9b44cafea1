// The CNO activation in 2-D (reference models/CNO2d.py:31-46) as one kernel per direction: antialiased bicubic
// resampling of a plane to h_mid x w_mid, LeakyReLU, antialiased bicubic resampling to h_out x w_out.  The 2-D
// resampling is the tensor product of the 1-D banded maps of rpde/cno.py, so a workgroup stages a rectangular tile of
// the plane with its halo in LDS and runs four separable passes LDS to LDS; the four-times-larger mid plane never
// reaches memory.  The rest of a CNO block -- Conv(k = 3), BatchNorm -- is in cno_layers.hip.
// gfx950 (CDNA4, wave64) only.
#include "cno.h"

#include <algorithm>

namespace rpde {

constexpr int C2_THREADS = 256;
constexpr int C2_TILE = 32;           // rows and columns of the written plane per workgroup (one 128-byte line wide),
                                      // each halved as far as it takes for the spans below to fit their LDS
constexpr int C2_MIN_TW = 4;          // narrowest tile: one 16-byte store
// LDS of the forward: R0 holds the staged input tile, then the mid tile; R1 the two half-resampled intermediates
constexpr int C2F_R0 = 6400, C2F_R1 = 3840;          // floats: 40 KiB per workgroup, four workgroups per CU
// LDS of the backward: R0 holds the staged x and g tiles, then the mid tile; R1 their half-resampled forms, then the
// half-gathered gradient
constexpr int C2B_R0 = 6400, C2B_R1 = 6912;          // 52 KiB per workgroup, three per CU
constexpr int C2_PACK_WORK = 4096;    // mid points per workgroup up to which whole planes are packed together
constexpr int C2_ALIGN_SLACK = 6;     // columns a staged tile may grow by when its ends are moved to 16-byte bounds

struct Cno2Shape {
  int planes, C;
  int h_in, w_in, h_mid, w_mid, h_out, w_out;
  int th, tw, nty, ntx, pack;         // tile of the written plane, tiles per plane, planes per workgroup
  float slope;
};

struct C2Run { int lo, n; };          // [lo, lo + n) along one axis

__device__ __forceinline__ C2Run c2_range(const CnoBand& b, C2Run rows, int n_src) {
  int lo, hi;
  band_range(b, rows.lo, rows.lo + rows.n, n_src, lo, hi);
  return C2Run{lo, hi - lo};
}
__device__ __forceinline__ C2Run c2_align4(C2Run r, int n) {
  const int lo = r.lo & ~3, hi = min(n, (r.lo + r.n + 3) & ~3);
  return C2Run{lo, hi - lo};
}

// every tile in LDS has its rows a whole number of float4s apart, so that the passes along y move four columns at once
__host__ __device__ __forceinline__ int c2_r4(int v) { return (v + 3) & ~3; }

// The spans a workgroup stages never exceed what the host sized the tile for (c2_fits_* below bound them from the
// filter's support); should a table not follow the rule, the tile is cut to the LDS it has instead of overrunning it:
// np planes of rows x cols floats, rows c2_r4(cols) apart, in cap
__device__ __forceinline__ void c2_cut(int& rows, int& cols, int np, int cap, bool vec) {
  const int most = cap / np;
  if (c2_r4(cols) > most) cols = most & ~3;
  if (vec) cols &= ~3;
  const int stride = c2_r4(cols);
  rows = stride > 0 ? min(rows, cap / (np * stride)) : 0;
}

// the taps of band row `row` that lie inside a source run of slen points starting at s_lo: first point (relative) and
// count; a row that leaves the run (never, for tables that follow the rule) reads nothing of what it does not own
__device__ __forceinline__ int2 c2_taps(const CnoBand& b, int row, int s_lo, int slen) {
  const int2 sp = b.span[row];
  const int off = sp.x - s_lo;
  return make_int2(off, off < 0 ? 0 : min(sp.y, slen - off));
}

// planes [p0, p0 + np) x rows ry x columns rx of t [planes, H, W] -> dst [np][ry.n][c2_r4(rx.n)], scale[c] * v +
// shift[c] on the way when scale is given.  VEC: rx.lo, rx.n and W are multiples of 4 and t is 16-byte aligned
template <bool VEC>
__device__ __forceinline__ void c2_stage(float* dst, const float* __restrict__ t, int p0, int np, int H, int W, C2Run ry,
                                         C2Run rx, const float* __restrict__ scale, const float* __restrict__ shift, int C) {
  const int q = VEC ? rx.n >> 2 : rx.n, ds = c2_r4(rx.n);
  const int per = ry.n * q;
  for (int idx = threadIdx.x; idx < np * per; idx += C2_THREADS) {
    const int p = idx / per, rem = idx - p * per;
    const int r = rem / q, i = rem - r * q;
    const long plane = p0 + p;
    const float* src = t + (plane * H + ry.lo + r) * W + rx.lo;
    float a = 1.f, b = 0.f;
    if (scale) { a = scale[plane % C]; b = shift[plane % C]; }
    if (VEC) {
      float4 v = *reinterpret_cast<const float4*>(src + 4 * i);
      if (scale) { v.x = fmaf(a, v.x, b); v.y = fmaf(a, v.y, b); v.z = fmaf(a, v.z, b); v.w = fmaf(a, v.w, b); }
      *reinterpret_cast<float4*>(dst + (p * ry.n + r) * ds + 4 * i) = v;
    } else {
      float v = src[i];
      if (scale) v = fmaf(a, v, b);
      dst[(p * ry.n + r) * ds + i] = v;
    }
  }
}

// the map along x: dst [rows][c2_r4(cols.n)], dst[r][j] = sum over band row cols.lo + j of src[r][..]; src holds
// [rows][c2_r4(sw)], sw columns from s_lo on.  A thread forms one column of four rows: the span, the weights and the
// index arithmetic are paid once for four sums, each in tap order as band_dot forms it
__device__ __forceinline__ void c2_pass_x(float* dst, const float* src, int rows, C2Run cols, const CnoBand& b, int sw,
                                          int s_lo) {
  const int ss = c2_r4(sw), ds = c2_r4(cols.n);
  const int groups = (rows + 3) >> 2;
  for (int idx = threadIdx.x; idx < groups * cols.n; idx += C2_THREADS) {
    const int rg = idx / cols.n, j = idx - rg * cols.n;
    const int2 tp = c2_taps(b, cols.lo + j, s_lo, sw);
    const float* __restrict__ w = b.w + (long)(cols.lo + j) * b.taps;
    const int r0 = 4 * rg, last = rows - 1;
    // (rows past the end repeat the last one: read, never written)
    const float* s0 = src + r0 * ss + tp.x;
    const float* s1 = src + min(r0 + 1, last) * ss + tp.x;
    const float* s2 = src + min(r0 + 2, last) * ss + tp.x;
    const float* s3 = src + min(r0 + 3, last) * ss + tp.x;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int t = 0; t < tp.y; t += 4) {
      const float4 wv = *reinterpret_cast<const float4*>(w + t);
      a0 = fmaf(wv.x, s0[t], a0); a1 = fmaf(wv.x, s1[t], a1); a2 = fmaf(wv.x, s2[t], a2); a3 = fmaf(wv.x, s3[t], a3);
      if (t + 1 < tp.y) {
        a0 = fmaf(wv.y, s0[t + 1], a0); a1 = fmaf(wv.y, s1[t + 1], a1); a2 = fmaf(wv.y, s2[t + 1], a2); a3 = fmaf(wv.y, s3[t + 1], a3);
      }
      if (t + 2 < tp.y) {
        a0 = fmaf(wv.z, s0[t + 2], a0); a1 = fmaf(wv.z, s1[t + 2], a1); a2 = fmaf(wv.z, s2[t + 2], a2); a3 = fmaf(wv.z, s3[t + 2], a3);
      }
      if (t + 3 < tp.y) {
        a0 = fmaf(wv.w, s0[t + 3], a0); a1 = fmaf(wv.w, s1[t + 3], a1); a2 = fmaf(wv.w, s2[t + 3], a2); a3 = fmaf(wv.w, s3[t + 3], a3);
      }
    }
    float* d = dst + r0 * ds + j;
    d[0] = a0;
    if (r0 + 1 < rows) d[ds] = a1;
    if (r0 + 2 < rows) d[2 * ds] = a2;
    if (r0 + 3 < rows) d[3 * ds] = a3;
  }
}

// sum_t w[t] * src[t * stride + k], t < cnt, in tap order, for four adjacent columns k: band_dot down four columns,
// one 16-byte LDS read per tap (src 16-byte aligned, stride a multiple of 4)
__device__ __forceinline__ float4 c2_dot_y4(const float* __restrict__ w, const float* src, int cnt, int stride) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int t = 0; t < cnt; ++t) {
    const float4 v = *reinterpret_cast<const float4*>(src + t * stride);
    const float wt = w[t];
    acc.x = fmaf(wt, v.x, acc.x); acc.y = fmaf(wt, v.y, acc.y); acc.z = fmaf(wt, v.z, acc.z); acc.w = fmaf(wt, v.w, acc.w);
  }
  return acc;
}

// the written tile: out[p0 + p][rows.lo + i][cols.lo + c] = sum over band row rows.lo + i of src[p][..][c]; src holds
// [np][sh][c2_r4(cols.n)] from row s_lo on.  Four columns per thread; VEC: they leave as one 16-byte store
template <bool VEC>
__device__ __forceinline__ void c2_emit_y(float* __restrict__ out, int p0, int np, int H, int W, C2Run rows, C2Run cols,
                                          const CnoBand& b, const float* src, int sh, int s_lo) {
  const int ss = c2_r4(cols.n), q = ss >> 2;
  const int per = rows.n * q;
  for (int idx = threadIdx.x; idx < np * per; idx += C2_THREADS) {
    const int p = idx / per, rem = idx - p * per;
    const int i = rem / q, c = 4 * (rem - i * q);
    const int2 tp = c2_taps(b, rows.lo + i, s_lo, sh);
    const float4 v = c2_dot_y4(b.w + (long)(rows.lo + i) * b.taps, src + (p * sh + tp.x) * ss + c, tp.y, ss);
    float* dst = out + ((long)(p0 + p) * H + rows.lo + i) * W + cols.lo + c;
    if (VEC) {
      *reinterpret_cast<float4*>(dst) = v;
    } else {
      dst[0] = v.x;
      if (c + 1 < cols.n) dst[1] = v.y;
      if (c + 2 < cols.n) dst[2] = v.z;
      if (c + 3 < cols.n) dst[3] = v.w;
    }
  }
}

// which tile and planes a workgroup owns: tiles of a plane are neighbours in the grid, x fastest
__device__ __forceinline__ void c2_whoami(const Cno2Shape& s, int H, int W, int& p0, int& np, C2Run& ty, C2Run& tx) {
  int b = blockIdx.x;
  const int ix = b % s.ntx; b /= s.ntx;
  const int iy = b % s.nty; b /= s.nty;
  p0 = b * s.pack;
  np = min(s.pack, s.planes - p0);
  ty = C2Run{iy * s.th, min(s.th, H - iy * s.th)};
  tx = C2Run{ix * s.tw, min(s.tw, W - ix * s.tw)};
}

__device__ __forceinline__ float c2_lrelu(float u, float slope) { return u > 0.f ? u : slope * u; }
__device__ __forceinline__ float c2_dlrelu(float u, float g, float slope) { return u > 0.f ? g : slope * g; }

// out = D_y lrelu(U_y y U_x^T) D_x^T on a tile of the output plane, y = scale x + shift
template <bool VX, bool VO>
__global__ void __launch_bounds__(C2_THREADS)
k_cno2d_act_fwd(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                float* __restrict__ out, Cno2Shape s, CnoBand Uy, CnoBand Ux, CnoBand Dy, CnoBand Dx) {
  __shared__ __attribute__((aligned(16))) float r0[C2F_R0];
  __shared__ __attribute__((aligned(16))) float r1[C2F_R1];
  int p0, np;
  C2Run oy, ox;
  c2_whoami(s, s.h_out, s.w_out, p0, np, oy, ox);
  C2Run my = c2_range(Dy, oy, s.h_mid), mx = c2_range(Dx, ox, s.w_mid);
  C2Run iy = c2_range(Uy, my, s.h_in), ix = c2_range(Ux, mx, s.w_in);
  if (VX) ix = c2_align4(ix, s.w_in);
  c2_cut(iy.n, ix.n, np, C2F_R0, VX);          // the staged input
  c2_cut(iy.n, mx.n, np, C2F_R1, false);       // resampled along x
  c2_cut(my.n, mx.n, np, C2F_R0, false);       // the mid tile
  c2_cut(my.n, ox.n, np, C2F_R1, VO);          // resampled down along x

  c2_stage<VX>(r0, x, p0, np, s.h_in, s.w_in, iy, ix, scale, shift, s.C);
  __syncthreads();
  c2_pass_x(r1, r0, np * iy.n, mx, Ux, ix.n, ix.lo);
  __syncthreads();
  const int ms = c2_r4(mx.n), q = ms >> 2, per = my.n * q;
  for (int idx = threadIdx.x; idx < np * per; idx += C2_THREADS) {
    const int p = idx / per, rem = idx - p * per;
    const int i = rem / q, c = 4 * (rem - i * q);
    const int2 tp = c2_taps(Uy, my.lo + i, iy.lo, iy.n);
    float4 u = c2_dot_y4(Uy.w + (long)(my.lo + i) * Uy.taps, r1 + (p * iy.n + tp.x) * ms + c, tp.y, ms);
    u.x = c2_lrelu(u.x, s.slope); u.y = c2_lrelu(u.y, s.slope); u.z = c2_lrelu(u.z, s.slope); u.w = c2_lrelu(u.w, s.slope);
    *reinterpret_cast<float4*>(r0 + (p * my.n + i) * ms + c) = u;      // (columns past mx.n: padding, never read)
  }
  __syncthreads();
  c2_pass_x(r1, r0, np * my.n, ox, Dx, mx.n, mx.lo);
  __syncthreads();
  c2_emit_y<VO>(out, p0, np, s.h_out, s.w_out, oy, ox, Dy, r1, my.n, my.lo);
}

// gy = U_y^T (lrelu'(u) * (D_y^T g D_x)) U_x on a tile of the input plane: the mid points that touch the tile (the
// transposed bands of U), their pre-activations u recomputed from the staged x with its halo, and D_y^T g D_x gathered
// through the transposed bands of D from the staged g
template <bool VX, bool VO>
__global__ void __launch_bounds__(C2_THREADS)
k_cno2d_act_bwd(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                const float* __restrict__ g, float* __restrict__ gy, Cno2Shape s, CnoBand Uy, CnoBand Ux, CnoBand UyT,
                CnoBand UxT, CnoBand DyT, CnoBand DxT) {
  __shared__ __attribute__((aligned(16))) float r0[C2B_R0];
  __shared__ __attribute__((aligned(16))) float r1[C2B_R1];
  int p0, np;
  C2Run ty, tx;
  c2_whoami(s, s.h_in, s.w_in, p0, np, ty, tx);
  C2Run my = c2_range(UyT, ty, s.h_mid), mx = c2_range(UxT, tx, s.w_mid);
  C2Run xy = c2_range(Uy, my, s.h_in), xx = c2_range(Ux, mx, s.w_in);
  C2Run gr = c2_range(DyT, my, s.h_out), gc = c2_range(DxT, mx, s.w_out);
  if (VX) xx = c2_align4(xx, s.w_in);
  if (VO) gc = c2_align4(gc, s.w_out);
  c2_cut(xy.n, xx.n, np, C2B_R0, VX);
  const int g_at = np * xy.n * c2_r4(xx.n);              // the staged g follows the staged x
  c2_cut(gr.n, gc.n, np, C2B_R0 - g_at, VO);
  c2_cut(xy.n, mx.n, np, C2B_R1, false);
  const int b_at = np * xy.n * c2_r4(mx.n);
  c2_cut(gr.n, mx.n, np, C2B_R1 - b_at, false);
  c2_cut(my.n, mx.n, np, C2B_R0, false);
  c2_cut(my.n, tx.n, np, C2B_R1, VX);
  // (a later cut only shrinks what an earlier one placed: every buffer is addressed with the final sizes below)
  const int ms = c2_r4(mx.n);
  float* s_x = r0;
  float* s_g = r0 + g_at;
  float* s_a = r1;                                       // U_x applied to x: [np][xy.n][ms]
  float* s_b = r1 + np * xy.n * ms;                      // D_x^T applied to g: [np][gr.n][ms]

  c2_stage<VX>(s_x, x, p0, np, s.h_in, s.w_in, xy, xx, scale, shift, s.C);
  c2_stage<VO>(s_g, g, p0, np, s.h_out, s.w_out, gr, gc, nullptr, nullptr, 1);
  __syncthreads();
  c2_pass_x(s_a, s_x, np * xy.n, mx, Ux, xx.n, xx.lo);
  c2_pass_x(s_b, s_g, np * gr.n, mx, DxT, gc.n, gc.lo);
  __syncthreads();
  const int q = ms >> 2, per = my.n * q;
  for (int idx = threadIdx.x; idx < np * per; idx += C2_THREADS) {
    const int p = idx / per, rem = idx - p * per;
    const int i = rem / q, c = 4 * (rem - i * q);
    const int2 tu = c2_taps(Uy, my.lo + i, xy.lo, xy.n), td = c2_taps(DyT, my.lo + i, gr.lo, gr.n);
    const float4 u = c2_dot_y4(Uy.w + (long)(my.lo + i) * Uy.taps, s_a + (p * xy.n + tu.x) * ms + c, tu.y, ms);
    float4 gm = c2_dot_y4(DyT.w + (long)(my.lo + i) * DyT.taps, s_b + (p * gr.n + td.x) * ms + c, td.y, ms);
    gm.x = c2_dlrelu(u.x, gm.x, s.slope); gm.y = c2_dlrelu(u.y, gm.y, s.slope);
    gm.z = c2_dlrelu(u.z, gm.z, s.slope); gm.w = c2_dlrelu(u.w, gm.w, s.slope);
    *reinterpret_cast<float4*>(r0 + (p * my.n + i) * ms + c) = gm;
  }
  __syncthreads();
  c2_pass_x(r1, r0, np * my.n, tx, UxT, mx.n, mx.lo);
  __syncthreads();
  c2_emit_y<VX>(gy, p0, np, s.h_in, s.w_in, ty, tx, UyT, r1, my.n, my.lo);
}

// ---- host: tile and packing -------------------------------------------------------------------------------------
// cno_sources / cno_readers with the equal-size map taken as what it is, the identity (their bound adds its support)
static int c2_src(int L, int na, int nb) { return na == nb ? std::min(L, na) : cno_sources(L, na, nb); }
static int c2_rdr(int L, int na, int nb) { return na == nb ? std::min(L, nb) : cno_readers(L, na, nb); }

// the LDS a th x tw tile of the written plane needs, per plane: forward (tile of the output) and backward (tile of the
// input); whole: the tile is the plane, every span is the plane's own size
static bool c2_fits_fwd(const Cno2Shape& s, int th, int tw, bool whole, int np) {
  const long my = whole ? s.h_mid : c2_src(th, s.h_mid, s.h_out), mx = whole ? s.w_mid : c2_src(tw, s.w_mid, s.w_out);
  const long iy = whole ? s.h_in : c2_src((int)my, s.h_in, s.h_mid);
  const long ix = whole ? s.w_in : std::min(c2_src((int)mx, s.w_in, s.w_mid) + C2_ALIGN_SLACK, s.w_in);
  const long mxs = c2_r4((int)mx);
  return np * iy * c2_r4((int)ix) <= C2F_R0 && np * my * mxs <= C2F_R0 && np * iy * mxs <= C2F_R1 &&
         np * my * c2_r4(tw) <= C2F_R1;
}
static bool c2_fits_bwd(const Cno2Shape& s, int th, int tw, bool whole, int np) {
  const long my = whole ? s.h_mid : c2_rdr(th, s.h_in, s.h_mid), mx = whole ? s.w_mid : c2_rdr(tw, s.w_in, s.w_mid);
  const long xy = whole ? s.h_in : c2_src((int)my, s.h_in, s.h_mid);
  const long xx = whole ? s.w_in : std::min(c2_src((int)mx, s.w_in, s.w_mid) + C2_ALIGN_SLACK, s.w_in);
  const long gr = whole ? s.h_out : c2_rdr((int)my, s.h_mid, s.h_out);
  const long gc = whole ? s.w_out : std::min(c2_rdr((int)mx, s.w_mid, s.w_out) + C2_ALIGN_SLACK, s.w_out);
  const long mxs = c2_r4((int)mx);
  return np * xy * c2_r4((int)xx) + np * gr * c2_r4((int)gc) <= C2B_R0 && np * my * mxs <= C2B_R0 &&
         np * (xy + gr) * mxs <= C2B_R1 && np * my * c2_r4(tw) <= C2B_R1;
}

// fills th / tw / nty / ntx / pack of s for a kernel that writes an H x W plane.  Planes that fit whole are packed,
// several to a workgroup; larger planes are tiled with the largest power-of-two tile whose spans fit -- of two with the
// same area the squarer one, whose halo is smaller, then the wider one, whose lines are longer
template <class Fits>
static bool c2_plan(Cno2Shape& s, int H, int W, const Fits& fits) {
  if (H <= C2_TILE && W <= C2_TILE && fits(H, W, true, 1)) {
    int pack = (int)std::max<long>(1, std::min<long>(s.planes, C2_PACK_WORK / ((long)s.h_mid * s.w_mid)));
    while (pack > 1 && !fits(H, W, true, pack)) --pack;
    s.th = H; s.tw = W; s.nty = s.ntx = 1; s.pack = pack;
    return true;
  }
  int th = 0, tw = 0;
  for (int h = C2_TILE; h >= 1; h >>= 1)
    for (int w = C2_TILE; w >= C2_MIN_TW; w >>= 1) {
      const bool better = h * w > th * tw || (h * w == th * tw && (std::min(h, w) > std::min(th, tw) ||
                                                                   (std::min(h, w) == std::min(th, tw) && w > tw)));
      if (better && fits(h, w, false, 1)) { th = h; tw = w; }
    }
  if (th == 0) return false;
  s.th = th; s.tw = tw; s.nty = (H + th - 1) / th; s.ntx = (W + tw - 1) / tw; s.pack = 1;
  return true;
}

static int c2_shape(const char* what, Cno2Shape& s, bool backward, const void* x, const void* scale, const void* shift, int B,
                    int C, int h_in, int w_in, int h_mid, int w_mid, int h_out, int w_out, float slope) {
  RPDE_TRY(cno_check(what, x, scale, shift, B, C, h_in, h_mid, h_out, slope));
  RPDE_TRY(cno_check(what, x, scale, shift, B, C, w_in, w_mid, w_out, slope));
  s = Cno2Shape{B * C, C, h_in, w_in, h_mid, w_mid, h_out, w_out, 0, 0, 0, 0, 0, slope};
  const bool fits = backward
      ? c2_plan(s, h_in, w_in, [&](int th, int tw, bool whole, int np) { return c2_fits_bwd(s, th, tw, whole, np); })
      : c2_plan(s, h_out, w_out, [&](int th, int tw, bool whole, int np) { return c2_fits_fwd(s, th, tw, whole, np); });
  RPDE_CHECK_ARG(fits, "%s: (%d, %d) -> (%d, %d) -> (%d, %d): what one row of %d written points reaches does not fit a "
                 "workgroup's staging area", what, h_in, w_in, h_mid, w_mid, h_out, w_out, C2_MIN_TW);
  const long groups = ((long)s.planes + s.pack - 1) / s.pack;
  RPDE_CHECK_ARG(groups * s.nty * s.ntx < (1L << 31), "%s: too many workgroups", what);
  return RPDE_OK;
}

}  // namespace rpde

using namespace rpde;

extern "C" {

int rpde_cno_act2d_plan(int backward, int B, int C, int h_in, int w_in, int h_mid, int w_mid, int h_out, int w_out, int* th,
                        int* tw, int* pack) {
  RPDE_CHECK_ARG(th && tw && pack, "cno_act2d_plan: null result");
  Cno2Shape s;                      // (no tensor to check here: any non-null pointer stands in for x)
  RPDE_TRY(c2_shape("cno_act2d_plan", s, backward != 0, th, nullptr, nullptr, B, C, h_in, w_in, h_mid, w_mid, h_out, w_out, 0.f));
  *th = s.th; *tw = s.tw; *pack = s.pack;
  return RPDE_OK;
}

int rpde_cno_act2d_fwd(const float* x, const float* scale, const float* shift, float* out, int B, int C, int h_in, int w_in,
                       int h_mid, int w_mid, int h_out, int w_out, float slope, const int32_t* uy_span, const float* uy_w,
                       int uy_taps, const int32_t* ux_span, const float* ux_w, int ux_taps, const int32_t* dy_span,
                       const float* dy_w, int dy_taps, const int32_t* dx_span, const float* dx_w, int dx_taps, void* stream) {
  const char* what = "cno_act2d_fwd";
  Cno2Shape s;
  RPDE_TRY(c2_shape(what, s, false, x, scale, shift, B, C, h_in, w_in, h_mid, w_mid, h_out, w_out, slope));
  RPDE_CHECK_ARG(out, "%s: null tensor", what);
  CnoBand Uy, Ux, Dy, Dx;
  RPDE_TRY(cno_band(what, "U_y", uy_span, uy_w, uy_taps, Uy));
  RPDE_TRY(cno_band(what, "U_x", ux_span, ux_w, ux_taps, Ux));
  RPDE_TRY(cno_band(what, "D_y", dy_span, dy_w, dy_taps, Dy));
  RPDE_TRY(cno_band(what, "D_x", dx_span, dx_w, dx_taps, Dx));
  const bool vx = w_in % 4 == 0 && al16(x), vo = w_out % 4 == 0 && al16(out);
  const long groups = ((long)s.planes + s.pack - 1) / s.pack;
  const dim3 grid((unsigned)(groups * s.nty * s.ntx)), block(C2_THREADS);
  hipStream_t st = as_stream(stream);
  cno_vec_dispatch(vx, vo, [&](auto VX, auto VO) {
    hipLaunchKernelGGL((k_cno2d_act_fwd<decltype(VX)::value, decltype(VO)::value>), grid, block, 0, st, x, scale, shift, out, s, Uy, Ux, Dy, Dx);
  });
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_cno_act2d_bwd(const float* x, const float* scale, const float* shift, const float* g, float* gy, int B, int C,
                       int h_in, int w_in, int h_mid, int w_mid, int h_out, int w_out, float slope, const int32_t* uy_span,
                       const float* uy_w, int uy_taps, const int32_t* ux_span, const float* ux_w, int ux_taps,
                       const int32_t* uyt_span, const float* uyt_w, int uyt_taps, const int32_t* uxt_span, const float* uxt_w,
                       int uxt_taps, const int32_t* dyt_span, const float* dyt_w, int dyt_taps, const int32_t* dxt_span,
                       const float* dxt_w, int dxt_taps, void* stream) {
  const char* what = "cno_act2d_bwd";
  Cno2Shape s;
  RPDE_TRY(c2_shape(what, s, true, x, scale, shift, B, C, h_in, w_in, h_mid, w_mid, h_out, w_out, slope));
  RPDE_CHECK_ARG(g && gy, "%s: null tensor", what);
  CnoBand Uy, Ux, UyT, UxT, DyT, DxT;
  RPDE_TRY(cno_band(what, "U_y", uy_span, uy_w, uy_taps, Uy));
  RPDE_TRY(cno_band(what, "U_x", ux_span, ux_w, ux_taps, Ux));
  RPDE_TRY(cno_band(what, "U_y^T", uyt_span, uyt_w, uyt_taps, UyT));
  RPDE_TRY(cno_band(what, "U_x^T", uxt_span, uxt_w, uxt_taps, UxT));
  RPDE_TRY(cno_band(what, "D_y^T", dyt_span, dyt_w, dyt_taps, DyT));
  RPDE_TRY(cno_band(what, "D_x^T", dxt_span, dxt_w, dxt_taps, DxT));
  const bool vx = w_in % 4 == 0 && al16(x) && al16(gy), vo = w_out % 4 == 0 && al16(g);
  const long groups = ((long)s.planes + s.pack - 1) / s.pack;
  const dim3 grid((unsigned)(groups * s.nty * s.ntx)), block(C2_THREADS);
  hipStream_t st = as_stream(stream);
  cno_vec_dispatch(vx, vo, [&](auto VX, auto VO) {
    hipLaunchKernelGGL((k_cno2d_act_bwd<decltype(VX)::value, decltype(VO)::value>), grid, block, 0, st, x, scale, shift, g, gy, s, Uy, Ux,
                       UyT, UxT, DyT, DxT);
  });
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

}  // extern "C"
