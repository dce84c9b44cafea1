// Spectral resize of channels-first fields (reference: utils/res_utils.py:29-50 `resize`, :93-125 `resize_1d`):
// rfft -> keep the bins both sizes share -> irfft at the new size, times out/in.  The truncated-DFT plans of the
// spectral layers, analysis at the source size and synthesis at the target size (cf_dft.h); no kernel of its own.
#include "pointwise.h"
#include "cf_dft.h"

using namespace rpde;

extern "C" {

static int min2(int a, int b) { return a < b ? a : b; }
static int shared_bins(int n_in, int n_out) { return min2(n_in / 2 + 1, n_out / 2 + 1); }

// the spectrum of the bins both sizes share
struct Resize1dWork {
  float* spec;
  Resize1dWork(Arena& ar, int64_t rows, int k) : spec(ar.take((size_t)rows * 2 * r4(k))) {}
};

size_t rpde_resize1d_ws_bytes(int64_t rows, int n_in, int n_out) {
  return ws_measure<Resize1dWork>(rows, shared_bins(n_in, n_out));
}

int rpde_resize1d(const float* x, float* out, int64_t rows, int n_in, int n_out, void* ws, size_t ws_bytes, void* stream) {
  RPDE_CHECK_ARG(x && out && rows > 0 && n_in > 0 && n_out > 0 && rows < (1L << 31), "resize1d: bad arguments");
  const int k = shared_bins(n_in, n_out);
  RPDE_CARVE("resize1d", Resize1dWork, w, ws, ws_bytes, rows, k);
  hipStream_t st = as_stream(stream);
  const rpde_plan *pa, *ps;
  RPDE_TRY(get_plan(&pa, n_in, k, RPDE_NORM_BACKWARD, 1, PLAN_REAL, st));
  RPDE_TRY(get_plan(&ps, n_out, k, RPDE_NORM_BACKWARD, 1, PLAN_REAL, st));
  RPDE_TRY(cf_analysis(pa, x, w.spec, rows, n_in, 0, st));
  return cf_synthesis(ps, w.spec, out, rows, n_out, st, (float)((double)n_out / (double)n_in));
}

// the kept bins of a 2-D resize: k2 along the contiguous axis, top + bot rows of the other
struct Resize2dBins {
  int k2, top, bot;
  Resize2dBins(int M, int N, int Mo, int No) : k2(shared_bins(N, No)), top(min2((M + 1) / 2, (Mo + 1) / 2)), bot(min2(M / 2, Mo / 2)) {}
};
// the row spectra of the larger grid, going in and coming out, and the kept spectrum
struct Resize2dWork {
  float *s1, *t1, *s2;
  Resize2dWork(Arena& ar, int64_t rows, int mm, const Resize2dBins& b)
      : s1(ar.take((size_t)rows * mm * 2 * r4(b.k2))), t1(ar.take((size_t)rows * mm * 2 * r4(b.k2))),
        s2(ar.take((size_t)rows * 2 * (b.top + b.bot) * r4(b.k2))) {}
};

size_t rpde_resize2d_ws_bytes(int64_t rows, int M, int N, int Mo, int No) {
  return ws_measure<Resize2dWork>(rows, M > Mo ? M : Mo, Resize2dBins(M, N, Mo, No));
}

// x [rows, M, N] -> out [rows, Mo, No]  (rows = batch * channels)
int rpde_resize2d(const float* x, float* out, int64_t rows, int M, int N, int Mo, int No, void* ws, size_t ws_bytes,
                  void* stream) {
  RPDE_CHECK_ARG(x && out && rows > 0 && M > 0 && N > 0 && Mo > 0 && No > 0 && rows * (long)(M > Mo ? M : Mo) < (1L << 31),
                 "resize2d: bad arguments");
  const Resize2dBins b(M, N, Mo, No);
  RPDE_CARVE("resize2d", Resize2dWork, w, ws, ws_bytes, rows, M > Mo ? M : Mo, b);
  hipStream_t st = as_stream(stream);
  const rpde_plan *pn, *pno, *pm, *pmo;
  RPDE_TRY(get_plan(&pn, N, b.k2, RPDE_NORM_BACKWARD, 1, PLAN_REAL, st));
  RPDE_TRY(get_plan(&pno, No, b.k2, RPDE_NORM_BACKWARD, 1, PLAN_REAL, st));
  RPDE_TRY(get_plan(&pm, M, b.top, RPDE_NORM_BACKWARD, 0, PLAN_CPLX, st, b.bot));
  RPDE_TRY(get_plan(&pmo, Mo, b.top, RPDE_NORM_BACKWARD, 0, PLAN_CPLX, st, b.bot));
  RPDE_TRY(cf_rfft2(pn, pm, x, w.s1, w.s2, rows, st));
  return cf_irfft2(pno, pmo, w.s2, w.t1, out, rows, st, (float)(((double)Mo / M) * ((double)No / N)));
}

}  // extern "C"
