// The rest of a CNO block, both ranks (the activation itself: cno.hip in 1-D, cno2d.hip in 2-D): Conv(k = 3,
// padding = 1) as accumulating GEMMs on shifted views with a deterministic weight gradient on the sliced scaffold it
// shares with the transposed convolution (wgrad_sliced.h), and the two kernels of BatchNorm (per-channel moments,
// per-channel affine combine).  Conv1d is Conv2d on a plane of one row with one row of taps: one tap loop, one
// weight-gradient path and one set of entries (ky = 1 or 3) serve both.  gfx950
// (CDNA4, wave64) only.
#include "wgrad_sliced.h"

namespace rpde {

// ---- Conv(k = 3, padding = 1): weight and bias gradient -----------------------------------------------------------
// gw[co][ci][ty][tx] = sum_{b,y,x} g[b][co][y][x] * x[b][ci][y + ty - KY / 2][x + tx - 1],  gb[co] = sum g[b][co][y][x],
// KY rows of taps: 3 for Conv2d, 1 for Conv1d (H = 1, gw [Cout][Cin][3]), on the sliced scaffold of wgrad_sliced.h:
// g is the narrow operand, the 3 KY shifted taps of x the wide one.  The slices are whole image rows (b, y); Conv1d
// always runs one slice
template <int KY>
struct ConvK3Wgrad {
  static constexpr int T = 3 * KY;
  static constexpr bool G_NARROW = true;
  int H, W, r_lo, b, y, xx;
  long plane;
  __device__ ConvK3Wgrad(int H_, int W_, long p_lo) : H(KY == 1 ? 1 : H_), W(W_), r_lo((int)(p_lo / W_)), plane((long)H * W_) {}
  __device__ __forceinline__ void seek(long i) {               // a slice starts on a row boundary
    const int r = r_lo + (int)(i / W);
    xx = (int)(i % W);
    b = r / H; y = r - b * H;
  }
  __device__ __forceinline__ float narrow(const float* __restrict__ g, int Cout, int co) const {
    return co < Cout ? g[((long)b * Cout + co) * plane + (long)y * W + xx] : 0.f;
  }
  __device__ __forceinline__ void wide(const float* __restrict__ x, int Cin, int ci, float (&xv)[T]) const {
    const bool live = ci < Cin;
    const float* img = x + ((long)b * Cin + (live ? ci : 0)) * plane;
#pragma unroll
    for (int ty = 0; ty < KY; ++ty) {
      const int yy = y + ty - KY / 2;
      const bool row_ok = live && yy >= 0 && yy < H;
#pragma unroll
      for (int tx = 0; tx < 3; ++tx) {
        const int xs = xx + tx - 1;
        xv[ty * 3 + tx] = row_ok && xs >= 0 && xs < W ? img[(long)yy * W + xs] : 0.f;
      }
    }
  }
};

// ---- BatchNorm pieces ---------------------------------------------------------------------------------------------
// sums[c] = (sum a, sum b, sum a b, sum b^2) over (batch, x) of channel c of two [B, C, n] tensors, in double; one
// workgroup per channel, fixed order.  The forward takes mean and variance of z from (z, z), the backward sum gy and
// sum gy z from (gy, z)
__global__ void __launch_bounds__(256)
k_cno_moments(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ sums, int B, int C, int n) {
  __shared__ double red[4][4];
  const int c = blockIdx.x;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  const long total = (long)B * n;
  for (long p = threadIdx.x; p < total; p += 256) {
    const long bb = p / n;
    const long at = (bb * C + c) * n + (p - bb * n);
    const double va = a[at], vb = b[at];
    s[0] += va; s[1] += vb; s[2] += va * vb; s[3] += vb * vb;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double v = wave_sum(s[k]);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    sums[c * 4 + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// out = p0[c] a + p1[c] b + p2[c] (+ residual): a BatchNorm's apply step (p1 null: no b term), its backward
// dz = p0 gy + p1 z + p2, and the residual block's skip add.  The coefficients are doubles and so is the arithmetic,
// rounded once: with few values per channel the backward's three terms cancel to eps / (var + eps) of their size, and
// fp32 coefficients would leave nothing of the result; the kernel stays bound by its bytes
template <bool VEC>
__global__ void __launch_bounds__(256)
k_cno_affine(const float* __restrict__ a, const float* __restrict__ b, const double* __restrict__ p0,
             const double* __restrict__ p1, const double* __restrict__ p2, const float* __restrict__ res,
             float* __restrict__ out, long total, int C, int n) {
  constexpr int W = VEC ? 4 : 1;
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * W;
  if (i >= total) return;
  const int c = (int)((i / n) % C);
  const double k0 = p0[c], k1 = p1 ? p1[c] : 0.0, k2 = p2[c];
  alignas(16) float va[W], vb[W], vr[W], o[W];
  if (VEC) {
    *reinterpret_cast<float4*>(va) = *reinterpret_cast<const float4*>(a + i);
    if (p1) *reinterpret_cast<float4*>(vb) = *reinterpret_cast<const float4*>(b + i);
    if (res) *reinterpret_cast<float4*>(vr) = *reinterpret_cast<const float4*>(res + i);
  } else {
    va[0] = a[i];
    if (p1) vb[0] = b[i];
    if (res) vr[0] = res[i];
  }
#pragma unroll
  for (int k = 0; k < W; ++k) {
    double v = fma(k0, (double)va[k], k2);
    if (p1) v = fma(k1, (double)vb[k], v);
    if (res) v += (double)vr[k];
    o[k] = (float)v;
  }
  if (VEC) *reinterpret_cast<float4*>(out + i) = *reinterpret_cast<float4*>(o);
  else out[i] = o[0];
}

}  // namespace rpde

using namespace rpde;

extern "C" {

// The taps of Conv(k = 3, padding = 1) as accumulating GEMMs on shifted views; wt holds KY
// rows of three taps, [3 KY][Cout][Cin]: KY = 3 for Conv2d, KY = 1 for Conv1d, whose row of taps is the dy = 0 one of
// a plane with H = 1.  Tap (dy, dx) adds W_t src[y + dy][x + dx] to dst[y][x] wherever both lie in the plane; taps
// without a valid range (H = 1 or W = 1) are skipped.  The centre tap goes first, over the flat H W axis (it carries
// the bias and initialises dst); a dx = 0 tap is flat too, (H - 1) W points from a row further on; a dx != 0 tap must
// not wrap across row ends, so it runs row by row through the descriptor's two-level batch (z1: sample, z2: image row)
// on W - 1 points.  (With one image row, H = 1, the second level is idle -- z2 = 0 -- and its stride W cannot move
// launch_gemm's choice of kernel either: the vector path already needs N = W - 1 and ldb = W to be multiples of 4
// together.  Conv1d's three GEMMs are therefore the ones it always ran: centre, left, right.)  transposed: the data
// gradient, the same products with W_t^T and the shifts mirrored
static int cno_conv_taps(const float* src, const float* wt, const float* bias, float* dst, int B, int Csrc, int Cdst, int KY,
                         int H, int W, bool transposed, hipStream_t st) {
  const int Cin = transposed ? Cdst : Csrc, Cout = transposed ? Csrc : Cdst;
  const long plane = (long)H * W;
  static const int order[9] = {4, 1, 7, 0, 2, 3, 5, 6, 8};
  for (int pass = 0; pass < 9; ++pass) {
    int dy = order[pass] / 3 - 1, dx = order[pass] % 3 - 1;
    if ((dy != 0 && H < 2) || (dx != 0 && W < 2)) continue;
    const int t = (dy + KY / 2) * 3 + dx + 1;                   // this tap in wt
    if (transposed) { dy = -dy; dx = -dx; }
    const int ady = dy < 0 ? -dy : dy;
    // dst[y][x] += src[y + dy][x + dx]: first row / column read and written
    const long read_at = (long)std::max(dy, 0) * W + std::max(dx, 0), write_at = (long)std::max(-dy, 0) * W + std::max(-dx, 0);
    rpde_gemm_desc d = gemm_desc();
    d.A = wt + (long)t * Cout * Cin; d.a_kmajor = transposed ? 0 : 1; d.lda = Cin;
    d.b_kmajor = 0; d.ldb = plane; d.ldc = plane;
    d.M = Cdst; d.K = Csrc;
    d.B = src + read_at; d.C = dst + write_at;
    if (dx == 0) {
      d.N = (int)((H - ady) * (long)W);
      d.batch = B; d.sB1 = Csrc * plane; d.sC1 = Cdst * plane;
    } else {
      d.N = W - 1;
      d.batch = B * (H - ady); d.zdiv = H - ady;
      d.sB1 = Csrc * plane; d.sC1 = Cdst * plane; d.sB2 = W; d.sC2 = W;
    }
    d.accumulate = pass > 0;
    if (pass == 0 && bias) { d.bias = bias; d.bias_mode = 2; }
    RPDE_TRY(launch_gemm(d, st));
  }
  return RPDE_OK;
}

// ky = 3 with H = 1 is legal (its outer tap rows have no valid range); ky = 1 is the 1-D entry.  At H = 1 the size
// conditions cannot fail
static int conv_k3_check(const char* what, const void* a, const void* b, const void* c, int B, int Cin, int Cout, int H, int W,
                         int ky) {
  RPDE_CHECK_ARG(a && b && c, "%s: null tensor", what);
  RPDE_CHECK_ARG(ky == 1 || ky == 3, "%s: ky must be 1 (1-D) or 3 (2-D), got %d", what, ky);
  RPDE_CHECK_ARG(B > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, "%s: bad sizes B=%d Cin=%d Cout=%d H=%d W=%d", what, B, Cin,
                 Cout, H, W);
  RPDE_CHECK_ARG(ky == 3 || H == 1, "%s: ky = 1 is the 1-D entry, a plane of one row (H = %d)", what, H);
  RPDE_CHECK_ARG((long)H * W < (1L << 31) && (long)B * H < (1L << 31), "%s: plane too large (H W and B H must stay below 2^31)", what);
  return RPDE_OK;
}

// the units the weight gradient's slices are made of: image rows (b, y); Conv1d is one unit and so one slice
static long conv_k3_units(int B, int H, int ky) { return ky == 1 ? 1 : (long)B * H; }

int rpde_conv_k3_fwd(const float* x, const float* wt, const float* bias, float* out, int B, int Cin, int Cout, int H, int W,
                     int ky, void* stream) {
  RPDE_TRY(conv_k3_check("conv_k3_fwd", x, wt, out, B, Cin, Cout, H, W, ky));
  return cno_conv_taps(x, wt, bias, out, B, Cin, Cout, ky, H, W, false, as_stream(stream));
}

int rpde_conv_k3_bwd_data(const float* g, const float* wt, float* gx, int B, int Cin, int Cout, int H, int W, int ky,
                          void* stream) {
  RPDE_TRY(conv_k3_check("conv_k3_bwd_data", g, wt, gx, B, Cin, Cout, H, W, ky));
  return cno_conv_taps(g, wt, nullptr, gx, B, Cout, Cin, ky, H, W, true, as_stream(stream));
}

int rpde_conv_k3_bwd_weight_slices(int B, int Cin, int Cout, int H, int W, int ky) {
  if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return 0;
  return wgrad_slices(Cin, Cout, conv_k3_units(B, H, ky), (long)B * H * W);
}

int rpde_conv_k3_bwd_weight(const float* x, const float* g, float* gw, float* gb, int B, int Cin, int Cout, int H, int W,
                            int ky, float* partial, int partial_slices, void* stream) {
  const char* what = "conv_k3_bwd_weight";
  RPDE_TRY(conv_k3_check(what, x, g, gw, B, Cin, Cout, H, W, ky));
  const auto run = ky == 1 ? wgrad_sliced<ConvK3Wgrad<1>> : wgrad_sliced<ConvK3Wgrad<3>>;
  return run(what, x, g, gw, gb, B, Cin, Cout, H, W, conv_k3_units(B, H, ky), partial, partial_slices, as_stream(stream));
}

int rpde_cno_moments(const float* a, const float* b, double* sums, int B, int C, int n, void* stream) {
  RPDE_CHECK_ARG(a && b && sums, "cno_moments: null tensor");
  RPDE_CHECK_ARG(B > 0 && C > 0 && n > 0, "cno_moments: bad sizes B=%d C=%d n=%d", B, C, n);
  RPDE_CHECK_ARG((reinterpret_cast<uintptr_t>(sums) & 7) == 0, "cno_moments: sums must be 8-byte aligned");
  hipLaunchKernelGGL(k_cno_moments, dim3((unsigned)C), dim3(256), 0, as_stream(stream), a, b, sums, B, C, n);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_cno_affine(const float* a, const float* b, const double* p0, const double* p1, const double* p2, const float* residual,
                    float* out, int B, int C, int n, void* stream) {
  RPDE_CHECK_ARG(a && p0 && p2 && out, "cno_affine: null tensor");
  RPDE_CHECK_ARG((b == nullptr) == (p1 == nullptr), "cno_affine: b and p1 come together");
  RPDE_CHECK_ARG(B > 0 && C > 0 && n > 0, "cno_affine: bad sizes B=%d C=%d n=%d", B, C, n);
  const long total = (long)B * C * n;
  const bool vec = n % 4 == 0 && al16(a) && al16(out) && (!b || al16(b)) && (!residual || al16(residual));
  const long threads = vec ? total / 4 : total;
  RPDE_CHECK_ARG((threads + 255) / 256 < (1L << 31), "cno_affine: tensor too large for one launch");
  const dim3 grid((unsigned)((threads + 255) / 256));
  if (vec) hipLaunchKernelGGL((k_cno_affine<true>), grid, dim3(256), 0, as_stream(stream), a, b, p0, p1, p2, residual, out, total, C, n);
  else hipLaunchKernelGGL((k_cno_affine<false>), grid, dim3(256), 0, as_stream(stream), a, b, p0, p1, p2, residual, out, total, C, n);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

}  // extern "C"
