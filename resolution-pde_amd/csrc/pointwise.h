// Internal declarations of the pointwise / reduction helpers (pointwise.hip).
#pragma once
#include "rpde_internal.h"
#include "workspace.h"

namespace rpde {

// Every plain fold of partial-sum slabs, out[i] = sum_s src[s*stride + i], i < len, runs in one kernel and one summation
// order (slab_partial in pointwise.hip).  Folds collected over several kernels are done by ONE launch
// (the small configurations are launch-bound: a FeedForward backward on the GEMM path has eight of them).
struct FoldJobs {
  static constexpr int MAX = 12;
  int n = 0;
  struct Job { const float* src; float* dst; long stride, len; int S, blk0; } j[MAX];
  bool add(const float* src, float* dst, long len, int S, long stride) {
    if (n >= MAX) return false;
    j[n].src = src; j[n].dst = dst; j[n].len = len; j[n].S = S; j[n].stride = stride; j[n].blk0 = 0;
    ++n;
    return true;
  }
};
// dst[i] = scale * sum (+ dst[i] when accumulate), the same for every job; empties `jobs`
int fold_jobs(FoldJobs& jobs, hipStream_t st, float scale = 1.f, int accumulate = 0);
// the fold of one job
int reduce_slabs(const float* slabs, float* out, long n, int S, long stride, float scale, int accumulate, hipStream_t st);
constexpr int REDUCE_CHUNKS = 64;
// tmp: REDUCE_CHUNKS * n floats of scratch
int reduce_slabs_2pass(const float* slabs, float* out, long n, int S, long stride, float* tmp, hipStream_t st);

size_t colsum_ws_floats(long P, int N);
int colsum(const float* x, float* out, long P, int N, long ld, float* ws, int accumulate, hipStream_t st);

int ff_tail_fwd(const float* z, const float* res, float* out, long P, int C, int layer_norm, float eps,
                const float* gamma, const float* beta, DropCfg drop, int post_act, hipStream_t st);
size_t ff_tail_bwd_ws_floats(long P, int C);
int ff_tail_bwd(const float* z, const float* g, float* dz, long P, int C, int layer_norm, float eps, const float* gamma,
                const float* beta, DropCfg drop, int post_act, float* grad_gamma, float* grad_beta, float* grad_bias,
                int* bias_done, float* ws, hipStream_t st, FoldJobs* defer = nullptr);

int pack_mix_weights(const float* w, float* blk, int Ci, int Co, int K, int keff, hipStream_t st);
int unpack_mix_grad(const float* slabs, float* gw, int Ci, int Co, int K, int keff, int S, long sstride, hipStream_t st);

}  // namespace rpde
