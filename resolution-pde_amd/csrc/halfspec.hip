// What the generators share on the half-spectrum layout of halfspec.h: the Gaussian random field in one and two
// dimensions (random_fields.py, GaussianRF1d / GaussianRF) and the transform entries between a field and its spectrum
// (rpde_etd1d_rfft / irfft, rpde_ns2d_rfft2 / irfft2).  gfx950, wave64.  No atomics: identical calls give identical bits.
#include "halfspec.h"

namespace rpde {

// noise [images][M][N][re|im] (coefficients c of the full M x N grid in fft order), se [M][N] = sqrt_eig -> the half
// spectrum h[k] = (se[k] c[k] + conj(se[-k] c[-k])) / 2, kx = 0 .. N/2, -k = ((M - ky) mod M, (N - kx) mod N):
// irfft2(h) is the real part of ifft2(se . c).  grid (blocks, images); a thread per 16-byte group of kx of one row ky,
// whole float4 stores, padded columns zero
__global__ __launch_bounds__(256) void k_grf_half(const float* __restrict__ noise, const float* __restrict__ se,
                                                  float* __restrict__ h, HalfSpec g) {
  const float2* __restrict__ nb = reinterpret_cast<const float2*>(noise) + (long)blockIdx.y * g.M * g.N;
  float* __restrict__ hb = h + (long)blockIdx.y * g.M * 2 * g.kp;
  const int c4n = g.kp / 4, groups = g.M * c4n;
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < groups; v += gridDim.x * blockDim.x) {
    const int ky = v / c4n, kx0 = (v - ky * c4n) * 4;
    const int my = ky ? g.M - ky : 0;
    float re[4], im[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kx = kx0 + j;
      re[j] = 0.f; im[j] = 0.f;
      if (kx < g.K) {
        const int mx = kx ? g.N - kx : 0;
        const long i1 = (long)ky * g.N + kx, i2 = (long)my * g.N + mx;
        const float2 c1 = nb[i1], c2 = nb[i2];
        const float s1 = se[i1], s2 = se[i2];
        re[j] = 0.5f * fmaf(s1, c1.x, s2 * c2.x);
        im[j] = 0.5f * fmaf(s1, c1.y, -(s2 * c2.y));
      }
    }
    st4(hb + (long)ky * 2 * g.kp + kx0, re);
    st4(hb + (long)ky * 2 * g.kp + g.kp + kx0, im);
  }
}

// the workspace holds the half spectrum and, for M > 1, the inverse transform's row spectra
struct GrfWork {
  float *h, *rows;
  GrfWork(Arena& ar, const HalfSpec& g) : h(ar.take(hs_elems(g))), rows(g.M > 1 ? ar.take(hs_elems(g)) : nullptr) {}
};

static int grf(const char* what, const float* noise, const float* sqrt_eig, float* out, const HalfSpec& g, void* ws,
               size_t ws_bytes, void* stream) {
  HS_CHECK_WS(what, ws);
  RPDE_CHECK_ARG(((uintptr_t)noise & 7) == 0, "%s: noise must be 8-byte aligned", what);
  RPDE_CARVE(what, GrfWork, w, ws, ws_bytes, g);
  hipStream_t st = as_stream(stream);
  const long groups = (long)g.M * (g.kp / 4);
  const int blk = hs_block(groups);
  hipLaunchKernelGGL(k_grf_half, hs_grid(groups, g.images, blk), dim3(blk), 0, st, noise, sqrt_eig, w.h, g);
  RPDE_LAUNCH_CHECK();
  return hs_irfft(g, w.h, w.rows, out, st);
}

// a transform entry: the row spectra of M > 1 come from the caller's workspace
static int dft_entry(const char* what, bool inverse, const float* in, float* out, const HalfSpec& g, void* ws,
                     size_t ws_bytes, void* stream) {
  float* rows = nullptr;
  if (g.M > 1) {
    HS_CHECK_WS(what, ws);
    Arena ar(ws, ws_bytes);
    rows = ar.take(hs_elems(g));
    RPDE_CLAIM_WS(what, ar, ws_bytes);
  }
  return inverse ? hs_irfft(g, in, rows, out, as_stream(stream)) : hs_rfft(g, in, rows, out, as_stream(stream));
}

}  // namespace rpde

using namespace rpde;

extern "C" {

int rpde_ns2d_rfft2(const float* w, float* W, int B, int M, int N, void* ws, size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(w && W && ws, "ns2d_rfft2: null pointer");
  HS_CHECK_DIMS_2D("ns2d_rfft2", B, M, N);
  return dft_entry("ns2d_rfft2", false, w, W, hs_geom(B, M, N), ws, ws_bytes, stream);
}

int rpde_ns2d_irfft2(const float* W, float* w, int B, int M, int N, void* ws, size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(w && W && ws, "ns2d_irfft2: null pointer");
  HS_CHECK_DIMS_2D("ns2d_irfft2", B, M, N);
  return dft_entry("ns2d_irfft2", true, W, w, hs_geom(B, M, N), ws, ws_bytes, stream);
}

int rpde_etd1d_rfft(const float* u, float* U, int B, int N, void* stream) {
  RPDE_CHECK_ARG(u && U, "etd1d_rfft: null pointer");
  HS_CHECK_DIMS_1D("etd1d_rfft", B, N);
  return dft_entry("etd1d_rfft", false, u, U, hs_geom(B, 1, N), nullptr, 0, stream);
}

int rpde_etd1d_irfft(const float* U, float* u, int B, int N, void* stream) {
  RPDE_CHECK_ARG(u && U, "etd1d_irfft: null pointer");
  HS_CHECK_DIMS_1D("etd1d_irfft", B, N);
  return dft_entry("etd1d_irfft", true, U, u, hs_geom(B, 1, N), nullptr, 0, stream);
}

size_t rpde_grf2d_ws_bytes(int B, int M, int N) { return hs_dims2_ok(B, M, N) ? ws_measure<GrfWork>(hs_geom(B, M, N)) : 0; }

int rpde_grf2d(const float* noise, const float* sqrt_eig, float* out, int B, int M, int N, void* ws, size_t ws_bytes,
               void* stream) {
  RPDE_CHECK_ARG(noise && sqrt_eig && out && ws, "grf2d: null pointer");
  HS_CHECK_DIMS_2D("grf2d", B, M, N);
  return grf("grf2d", noise, sqrt_eig, out, hs_geom(B, M, N), ws, ws_bytes, stream);
}

size_t rpde_grf1d_ws_bytes(int B, int N) { return hs_dims_ok(B, 1, N) ? ws_measure<GrfWork>(hs_geom(B, 1, N)) : 0; }

int rpde_grf1d(const float* noise, const float* sqrt_eig, float* out, int B, int N, void* ws, size_t ws_bytes,
               void* stream) {
  RPDE_CHECK_ARG(noise && sqrt_eig && out && ws, "grf1d: null pointer");
  HS_CHECK_DIMS_1D("grf1d", B, N);
  return grf("grf1d", noise, sqrt_eig, out, hs_geom(B, 1, N), ws, ws_bytes, stream);
}

}  // extern "C"
