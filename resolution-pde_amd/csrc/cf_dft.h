// Truncated DFT of channels-first tensors (cf_dft.hip): the streaming kernels along the contiguous axis, the host layer
// that chooses between them and the GEMMs, and the real 2-D transform built from it
#pragma once
#include "rpde_internal.h"
#include "plan.h"

namespace rpde {
// planar real plans with n % 128 == 0, 2 kp <= 32 and a table that fits 64 KB of LDS
bool cf_h2_eligible(int n, int R);
// ... and, for the synthesis kernel, n <= 512 (its table has n / 16 fragments)
bool cf_h2_syn_eligible(int n, int R);
int cf_build_tables(rpde_plan* p, hipStream_t st);
// B (or, the MFMA operands being symmetric, A) fragments of the table entry(k = y, col = r) = src[r*rs + y*cs], r < R,
// y < n, in the layout of the kernels above ([n/32 up][R/16 up][hi|lo][1 KB], 2^12-scaled, frag_perm order inside a
// 32-step), zero-padded; any R and n
size_t cf_table_bytes(int R, int n);
int cf_table_fragments(const float* src, long rs, long cs, int R, int n, char* out, hipStream_t st);
// spec[rows, 2kp] = alpha * x[rows, n] . T^T          adjoint: T = Fs^T (adjoint of the synthesis) instead of Fa
int cf_analysis_h2(const rpde_plan* pl, int adjoint, const float* x, float* spec, long rows, float alpha, hipStream_t st);
// out[rows, n] = alpha * spec[rows, 2kp] . S^T        adjoint: S = Fa^T (adjoint of the analysis) instead of Fs
int cf_synthesis_h2(const rpde_plan* pl, int adjoint, const float* spec, float* out, long rows, float alpha, hipStream_t st);

// ---- host layer (cf_dft.hip): the kernels above where they cover the shape, the GEMMs otherwise.  `slabs`: scratch of
// thin_slab_floats() entries for a thin product's split reduction (nullptr: never split) ----
int thin_ksplit(long rows, int ncols, int kred);
size_t thin_slab_floats(long rows, int ncols, int kred);
int thin_gemm(rpde_gemm_desc& d, float* slabs, hipStream_t st);
// x[rows, n] -> spec[rows, 2kp], optional activation on the input;  spec[rows, 2kp] -> alpha * out[rows, n] (C2R)
int cf_analysis(const rpde_plan* pl, const float* x, float* spec, long rows, int n, int act_in, hipStream_t st, float* slabs = nullptr);
int cf_synthesis(const rpde_plan* pl, const float* spec, float* out, long rows, int n, hipStream_t st, float alpha = 1.f);
// their adjoints: g[rows, n] . Fs -> gspec[rows, 2kp];  dspec[rows, 2kp] . Fa -> gx[rows, n], through act'(x) when act_in
int cf_synthesis_T(const rpde_plan* pl, const float* g, float* gspec, long rows, int n, hipStream_t st, float* slabs = nullptr);
int cf_analysis_T(const rpde_plan* pl, const float* dspec, float* gx, long rows, int n, int act_in, const float* x, hipStream_t st);
// per (b, c) block GEMM with a shared table: out_z[m_out, width] = T . in_z[k_red, width]  (or T^T . in_z)
int cf_rowdft(const float* table, long ld_table, bool transpose, int m_out, int k_red, const float* in, float* out, int nblocks,
              int width, hipStream_t st);

// ---- real 2-D DFT of z [rows, M, N] (M = pm->n, N = pn->n) to the half spectrum [rows][2R][kp]: R = pm->kp row slots
// of the complex column plan pm (re | im planes per slot), kp = pn->kp padded columns.  pm == nullptr: one-dimensional,
// [rows][2 kp], no scratch.  Both plans RPDE_NORM_BACKWARD: forward unnormalised, inverse 1 / (M N) in the tables.
// cf_rfft2_plans: the pair that keeps the whole spectrum, every row in fft order (pm stays null for M = 1).  The first
// use of a grid builds the tables: it allocates and synchronises the stream once (plan.h).
int cf_rfft2_plans(const rpde_plan** pn, const rpde_plan** pm, int M, int N, hipStream_t st);
// s1, t1: scratch of rows * M * 2 kp floats (the row spectra).  cf_irfft2 is alpha * torch.fft.irfft2: Im of the
// self-conjugate bins of the last axis is ignored (their synthesis table entries are sin(0) = 0)
int cf_rfft2(const rpde_plan* pn, const rpde_plan* pm, const float* z, float* s1, float* spec, long rows, hipStream_t st);
int cf_irfft2(const rpde_plan* pn, const rpde_plan* pm, const float* spec, float* t1, float* z, long rows, hipStream_t st,
              float alpha = 1.f);
}  // namespace rpde
