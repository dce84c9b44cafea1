// The half-spectrum layer under the generators (ns_solver.hip, etd1d.hip), the random fields and transform entries
// (halfspec.hip) and the spectral losses (spectral_loss.hip, band_energy.hip, etd_residual.hip): one geometry, its
// limits, the 16-byte group helpers and the transforms of a geometry on the full-spectrum real DFT of cf_dft.h.
#pragma once
#include "cf_dft.h"
#include "pointwise.h"

namespace rpde {

constexpr int HS_MIN_N = 4;          // per axis of a generator grid, even
constexpr int HS_MAX_N = 4096;       // per axis: the full-spectrum tables are quadratic in it

// A half spectrum is [images][M][re|im][kp]: rows ky in fft order (signed k1 = ky < M/2 ? ky : ky - M, so the Nyquist
// row counts as -M/2), kx = 0 .. N/2 along the contiguous axis, K = N/2+1 of them, kp = K rounded up to 4, padded
// columns zero.  M = 1: one-dimensional, [images][re|im][kp].
struct HalfSpec { int images, M, N, K, kp; };

inline HalfSpec hs_geom(int images, int M, int N) { return HalfSpec{images, M, N, N / 2 + 1, r4(N / 2 + 1)}; }
inline size_t hs_per(const HalfSpec& g) { return (size_t)g.M * 2 * g.kp; }      // floats of one image
inline size_t hs_elems(const HalfSpec& g) { return (size_t)g.images * hs_per(g); }
// a generator grid: N even in range, M = 1 or even in range, and fan x images -- the largest batch the caller makes of
// them -- within gridDim.y, four times that within the transforms' int rows (always so for M = 1).  fan = 1 is the
// batch as it stands: with the factor four, the 4 x images derivative fields of the plain Navier-Stokes step.  The
// active-scalar step passes 6, so that its 6 x images derivative spectra are held to both limits as a batch of their own
inline bool hs_dims_ok(int images, int M, int N, int fan = 1) {
  const auto axis = [](int n) { return n >= HS_MIN_N && n <= HS_MAX_N && n % 2 == 0; };
  return images > 0 && images <= 65535 / fan && axis(N) && (M == 1 || axis(M)) &&
         4L * fan * images * (M > N ? M : N) < (1L << 31);
}
inline bool hs_dims2_ok(int images, int M, int N, int fan = 1) { return M > 1 && hs_dims_ok(images, M, N, fan); }   // 2-D only
// a loss grid (spectral_loss.hip, band_energy.hip): B C images whose axes may be odd, M = 1: one-dimensional
inline bool hs_loss_dims_ok(int B, int C, int M, int N) {
  return B > 0 && C > 0 && M >= 1 && N >= 2 && M <= HS_MAX_N && N <= HS_MAX_N && (long)B * C * M < (1L << 31);
}

// `what`: the entry's name, a literal or a variable
#define HS_CHECK_WS(what, ws) \
  RPDE_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: the workspace must be 256-byte aligned", what)
#define HS_CHECK_DIMS_2D(what, B, M, N)                                                                           \
  RPDE_CHECK_ARG(hs_dims2_ok(B, M, N),                                                                            \
                 what ": bad B=%d M=%d N=%d (even axes %d .. %d, 4 B max(M, N) < 2^31, B <= 65535)", B, M, N, HS_MIN_N, \
                 HS_MAX_N)
// the same with a fan-out factor, and `what` a variable
#define HS_CHECK_DIMS_2D_FAN(what, B, M, N, fan)                                                                  \
  RPDE_CHECK_ARG(hs_dims2_ok(B, M, N, fan), "%s: bad B=%d M=%d N=%d (even axes %d .. %d, %d B max(M, N) < 2^31, %d B <= 65535)", \
                 what, B, M, N, HS_MIN_N, HS_MAX_N, 4 * (fan), fan)
#define HS_CHECK_DIMS_1D(what, B, N)                                                                              \
  RPDE_CHECK_ARG(hs_dims_ok(B, 1, N), what ": bad B=%d N=%d (N even, %d .. %d, 1 <= B <= 65535)", B, N, HS_MIN_N, \
                 HS_MAX_N)

// ceil(items / 256) blocks, at most `cap`, at least one
inline unsigned hs_blocks(long items, long cap) {
  long nb = (items + 255) / 256;
  if (nb > cap) nb = cap;
  return (unsigned)(nb < 1 ? 1 : nb);
}
// A thread per 16-byte group of kx, grid (blocks, images), grid-stride over an image's `groups`.  hs_block: a block
// per 64 groups where an image has no more (a wave covers them), 256 threads otherwise
inline int hs_block(long groups) { return groups <= 64 ? 64 : 256; }
inline dim3 hs_grid(long groups, int images, int block = 256) {
  long nb = (groups + block - 1) / block;
  if (nb > 256) nb = 256;
  return dim3((unsigned)(nb < 1 ? 1 : nb), images);
}

__device__ __forceinline__ void ld4(const float* p, float (&v)[4]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void st4(float* p, const float (&v)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}

// z [images, M, N] -> spec (torch.fft.rfft2 / rfft, unnormalised) and back (irfft2 / irfft, 1 / (M N)): the plan lookup
// of cf_rfft2_plans and the transform.  rows: scratch of hs_elems(g) floats, null for M = 1
inline int hs_rfft(const HalfSpec& g, const float* z, float* rows, float* spec, hipStream_t st) {
  const rpde_plan *pn, *pm;
  RPDE_TRY(cf_rfft2_plans(&pn, &pm, g.M, g.N, st));
  return cf_rfft2(pn, pm, z, rows, spec, g.images, st);
}
inline int hs_irfft(const HalfSpec& g, const float* spec, float* rows, float* z, hipStream_t st) {
  const rpde_plan *pn, *pm;
  RPDE_TRY(cf_rfft2_plans(&pn, &pm, g.M, g.N, st));
  return cf_irfft2(pn, pm, spec, rows, z, g.images, st);
}

}  // namespace rpde
