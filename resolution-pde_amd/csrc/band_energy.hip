// Per-sample, per-band spectral energies of a field, forward and backward (rpde.ops.band_energy; utils/loss.py
// BandRelativeL2Loss and SpectrumMatchingLoss are built on it; no counterpart in the reference)
//   E[b, j] = sum_c sum_{(ky,kx): band = j}  c_kx / (M N) |Z[b,c,ky,kx]|^2,   Z = rfft / rfft2 of z, unnormalised,
//   c_kx = 1 at kx = 0 and (even N) kx = N/2, else 2;  band in {-1, 0 .. J-1}, -1: the entry belongs to no band
//   grad_z[b, c] = 2 irfft2(gE[b, band(ky,kx)] Z[b,c,ky,kx]),  weight 0 where band = -1
// on the half-spectrum layer of halfspec.h (hs_rfft / hs_irfft: the plans of the loss, the resizers, the generators).
// The field is x, or x - y formed in fp32 BEFORE the transform (rel_diff of rel_loss.h).
//
// The band table reaches the kernels in two forms, both built once per (grid, table) by rpde.ops:
//   entries [n_entries], start [J+1]   the entries of band j are entries[start[j] .. start[j+1]), each
//                                      (offset << 1) | (c_kx == 2) with offset = ky 2 kp + kx the position of Re in ONE
//                                      image's spectrum (Im sits kp further); forward only
//   band [M][kp]                       the band of every entry, padded columns -1; backward only
// so that a (sample, band) sum reads exactly the entries of its band, not the whole table:
//   k_be_partial   a wave per (sample, band, slot): |Z|^2 c_kx over its share of the band's entries and the C channels in
//                  float64, lanes in a fixed order; k_be_final adds the slots in order and scales by 1 / (M N): no
//                  atomics, identical calls give identical bits, and a sample's energies do not depend on its batch
//   k_be_scale     backward: a thread per 16-byte group of kx gathers gE[b, band] for its four entries and writes
//                  2 gE Z (zeros where band = -1 and in the padded columns), the spectrum the inverse transform reads
// An offset outside the image, a start[] outside entries[] and a band outside 0 .. J-1 are skipped, not trusted.
#include "halfspec.h"
#include "rel_loss.h"
#include "wave.h"

namespace rpde {

constexpr int BE_MAX_BANDS = 4096;

struct BeGeom : HalfSpec { int B, C, J, S; };     // B C images; S partial sums per (sample, band)

// grid (ceil(J / 4), S, samples): wave w of a workgroup takes band 4 blockIdx.x + w; part[(b J + j) S + slot]
__global__ __launch_bounds__(256) void k_be_partial(const float* __restrict__ spec, const int* __restrict__ entries,
                                                    const int* __restrict__ start, int n_entries,
                                                    double* __restrict__ part, BeGeom g) {
  const int lane = threadIdx.x & 63, j = (int)blockIdx.x * 4 + (threadIdx.x >> 6), slot = blockIdx.y;
  if (j >= g.J) return;
  const long per = (long)g.M * 2 * g.kp;
  int e0 = start[j], e1 = start[j + 1];
  if (e0 < 0) e0 = 0;
  if (e1 > n_entries) e1 = n_entries;
  for (int b = blockIdx.z; b < g.B; b += gridDim.z) {
    double acc = 0.0;
    for (int c = 0; c < g.C; ++c) {
      const float* __restrict__ sp = spec + ((long)b * g.C + c) * per;
      for (long e = (long)e0 + slot * 64 + lane; e < e1; e += (long)g.S * 64) {
        const int en = entries[e], off = en >> 1;
        if (off < 0 || off + g.kp >= per) continue;
        const double re = (double)sp[off], im = (double)sp[off + g.kp];
        acc += ((en & 1) ? 2.0 : 1.0) * (re * re + im * im);
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) part[((long)b * g.J + j) * g.S + slot] = acc;
  }
}

__global__ __launch_bounds__(256) void k_be_final(const double* __restrict__ part, float* __restrict__ E, BeGeom g) {
  const double inv = 1.0 / ((double)g.M * (double)g.N);
  const long n = (long)g.B * g.J;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    double s = 0.0;
    for (int q = 0; q < g.S; ++q) s += part[i * g.S + q];
    E[i] = (float)(s * inv);
  }
}

// grid hs_grid(groups of an image, images): w = 2 gE[b, band] Z
__global__ __launch_bounds__(256) void k_be_scale(const float* __restrict__ spec, const int* __restrict__ band,
                                                  const float* __restrict__ gE, float* __restrict__ w, BeGeom g) {
  const long per = (long)g.M * 2 * g.kp;
  const int groups = (int)(per / 4);
  for (int img = blockIdx.y; img < g.images; img += gridDim.y) {
    const float* __restrict__ ge = gE + (long)(img / g.C) * g.J;
    for (int gi = blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += gridDim.x * blockDim.x) {
      const int e = gi * 4, row = e / g.kp, kx0 = e - row * g.kp;
      const int4 bd = *reinterpret_cast<const int4*>(band + (long)(row >> 1) * g.kp + kx0);
      const int bj[4] = {bd.x, bd.y, bd.z, bd.w};
      float v[4];
      ld4(spec + (long)img * per + e, v);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = (bj[i] >= 0 && bj[i] < g.J) ? (2.f * ge[bj[i]]) * v[i] : 0.f;
      st4(w + (long)img * per + e, v);
    }
  }
}

static bool be_dims_ok(int B, int C, int M, int N, int J) { return hs_loss_dims_ok(B, C, M, N) && J >= 1 && J <= BE_MAX_BANDS; }
static BeGeom be_geom(int B, int C, int M, int N, int J) {
  BeGeom g{hs_geom(B * C, M, N), B, C, J, 1};
  g.S = rel_slots((long)C * M * g.K);             // no band owns more terms than a sample has
  return g;
}

}  // namespace rpde

using namespace rpde;

extern "C" {

size_t rpde_band_energy_spec_elems(int B, int C, int M, int N) {
  return be_dims_ok(B, C, M, N, 1) ? hs_elems(hs_geom(B * C, M, N)) : 0;
}

// forward: the difference, the spectrum when it is not kept, the row spectra, the partial sums (doubles)
struct BeFwdWork {
  float *d, *s0, *s1; double* part;
  BeFwdWork(Arena& ar, const BeGeom& g)
      : d(ar.take((size_t)g.images * g.M * g.N)), s0(ar.take(hs_elems(g))), s1(ar.take(hs_elems(g))),
        part(reinterpret_cast<double*>(ar.take((size_t)2 * g.B * g.J * g.S))) {}
};
// backward: the scaled spectrum and the row spectra
struct BeBwdWork {
  float *w, *t1;
  BeBwdWork(Arena& ar, const BeGeom& g) : w(ar.take(hs_elems(g))), t1(ar.take(hs_elems(g))) {}
};

size_t rpde_band_energy_ws_bytes(int B, int C, int M, int N, int J) {
  if (!be_dims_ok(B, C, M, N, J)) return 0;
  const BeGeom g = be_geom(B, C, M, N, J);
  return ws_max(ws_measure<BeFwdWork>(g), ws_measure<BeBwdWork>(g));
}

int rpde_band_energy_fwd(const float* x, const float* y, const int32_t* entries, const int32_t* start, int n_entries,
                         float* E, float* spec, int B, int C, int M, int N, int J, void* ws, size_t ws_bytes,
                         void* stream) {
  RPDE_CHECK_ARG(x && entries && start && E && ws, "band_energy_fwd: null pointer");
  RPDE_CHECK_ARG(be_dims_ok(B, C, M, N, J),
                 "band_energy_fwd: bad B=%d C=%d M=%d N=%d J=%d (axes 2 .. %d; M = 1: one-dimensional; 1 <= J <= %d)", B, C, M, N,
                 J, HS_MAX_N, BE_MAX_BANDS);
  RPDE_CHECK_ARG(n_entries >= 0 && n_entries <= (long)M * (N / 2 + 1), "band_energy_fwd: n_entries=%d for a %d x %d spectrum",
                 n_entries, M, N / 2 + 1);
  HS_CHECK_WS("band_energy_fwd", ws);
  const BeGeom g = be_geom(B, C, M, N, J);
  RPDE_CARVE("band_energy_fwd", BeFwdWork, w, ws, ws_bytes, g);
  hipStream_t st = as_stream(stream);
  float* sp = spec ? spec : w.s0;
  const float* z = x;
  if (y) {
    RPDE_TRY(rel_diff(x, y, w.d, (long)g.images * M * N, st));
    z = w.d;
  }
  RPDE_TRY(hs_rfft(g, z, w.s1, sp, st));
  const unsigned nb = (unsigned)(B < 65535 ? B : 65535);
  hipLaunchKernelGGL(k_be_partial, dim3((J + 3) / 4, g.S, nb), dim3(256), 0, st, sp, entries, start, n_entries, w.part, g);
  RPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_be_final, dim3(hs_blocks((long)B * J, 1024)), dim3(256), 0, st, w.part, E, g);
  RPDE_LAUNCH_CHECK();
  return RPDE_OK;
}

int rpde_band_energy_bwd(const float* spec, const int32_t* band, const float* gE, float* grad_x, int B, int C, int M, int N,
                         int J, void* ws, size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(spec && band && gE && grad_x && ws, "band_energy_bwd: null pointer");
  RPDE_CHECK_ARG(be_dims_ok(B, C, M, N, J),
                 "band_energy_bwd: bad B=%d C=%d M=%d N=%d J=%d (axes 2 .. %d; M = 1: one-dimensional; 1 <= J <= %d)", B, C, M, N,
                 J, HS_MAX_N, BE_MAX_BANDS);
  RPDE_CHECK_ARG(al16(spec) && al16(band), "band_energy_bwd: the spectrum and the band table must be 16-byte aligned");
  HS_CHECK_WS("band_energy_bwd", ws);
  const BeGeom g = be_geom(B, C, M, N, J);
  RPDE_CARVE("band_energy_bwd", BeBwdWork, w, ws, ws_bytes, g);
  hipStream_t st = as_stream(stream);
  const long groups = (long)hs_per(g) / 4;
  const int blk = hs_block(groups);
  hipLaunchKernelGGL(k_be_scale, hs_grid(groups, g.images < 65535 ? g.images : 65535, blk), dim3(blk), 0, st, spec, band, gE, w.w,
                     g);
  RPDE_LAUNCH_CHECK();
  return hs_irfft(g, w.w, w.t1, grad_x, st);
}

}  // extern "C"
