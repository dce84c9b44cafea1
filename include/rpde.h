/*
 * rpde.h -- C ABI of librpde_hip.so: the MI355X (gfx950) implementation of the
 * spectral-convolution hot path of RohanVKashyap/resolution-pde.
 *
 * Boundary rules:
 *   - plain C, raw DEVICE pointers + sizes + a hipStream_t (passed as void*);
 *     no torch types, no exceptions; every entry point returns 0 on success or
 *     a negative rpde_status; rpde_last_error() gives the thread-local message.
 *   - the caller (PyTorch) owns every tensor, including workspaces and the
 *     tensors saved for backward; the library owns only DFT plans (small
 *     device tables) inside opaque handles / an internal mutex-guarded cache.
 *   - all tensors are fp32 and contiguous in the stated layout; complex64
 *     parameters are passed as their (re,im)-interleaved float storage.
 *   - entry points are re-entrant per device and asynchronous on `stream`.
 *
 * Each entry point cites the reference code it replaces (paths are relative to
 * the reference repository root).
 */
#ifndef RPDE_H
#define RPDE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  RPDE_OK = 0,
  RPDE_ERR_ARG = -1,        /* bad shape / null pointer / unsupported option    */
  RPDE_ERR_HIP = -2,        /* a HIP runtime call or launch failed              */
  RPDE_ERR_WORKSPACE = -3,  /* workspace smaller than the *_ws_bytes() answer   */
  RPDE_ERR_MODES = -4       /* modes exceed the spectrum (SpectralConv* quirk Q5) */
} rpde_status;

/* fft_norm as torch.fft spells it */
enum { RPDE_NORM_BACKWARD = 0, RPDE_NORM_ORTHO = 1, RPDE_NORM_FORWARD = 2 };
/* FSpectralConv* `mode` (models/spectral_convolution.py:187-196, 273-281) */
enum { RPDE_MODE_FULL = 0, RPDE_MODE_LOWPASS = 1 };
/* activations (models/spectral_convolution.py:104-106, fno_blocks.py:33,71) */
enum { RPDE_ACT_IDENTITY = 0, RPDE_ACT_GELU = 1, RPDE_ACT_RELU = 2 };
enum { RPDE_EPI_MULAUX = 100 };

const char* rpde_last_error(void);
int rpde_version(void);

/* ---- DFT plans ---------------------------------------------------------
 * Truncated real-DFT tables for (n, modes, norm): the R2C transform restricted
 * to bins [0,modes) and the C2R transform of a spectrum that is zero beyond
 * them (Im(DC)/Im(Nyquist) ignored, as torch.fft.irfft does).  Replaces the
 * torch.fft.rfft / irfft calls at models/spectral_convolution.py:41,54,165,198,
 * 265,284,289,308.  The op entry points below look plans up in an internal
 * cache; create/destroy are exported for callers that want to pre-plan
 * (multi-resolution batches, SURVEY hard part 6). */
typedef struct rpde_plan rpde_plan;
int rpde_plan_create(rpde_plan** plan, int n, int modes, int norm, void* stream);
int rpde_plan_destroy(rpde_plan* plan);
/* copies of the float tables for tests: analysis [2*kp, ldn], synthesis [n, 2*kp] */
int rpde_plan_info(const rpde_plan* plan, int* n, int* modes, int* kp, int* ldn);
/* number of plans the per-process cache holds (every spectral entry point below takes its plans from that cache and
 * builds a missing one on first use: hipMalloc + one stream synchronisation).  Constant across training steps once
 * rpde.ops.warm_plans() has seen the run's grid sizes. */
int rpde_plan_cache_count(void);
int rpde_plan_tables(const rpde_plan* plan, float* analysis_host, float* synthesis_host);

/* ---- generic strided batched GEMM (fp32 MFMA) -----------------------------
 * C[z][m,n] (+)= alpha * sum_k A[z][m,k] * B[z][k,n]  with fused prologue /
 * epilogue.  Everything heavy below is expressed through it; exported so the
 * parity tests and bench.py can time the kernel itself. */
typedef struct {
  const float* A; const float* B; float* C;
  int M, N, K;
  int a_kmajor;            /* 1: A[m*lda+k] (k contiguous)   0: A[k*lda+m]          */
  int b_kmajor;            /* 1: B^T stored, B[n*ldb+k]      0: B[k*ldb+n]          */
  int64_t lda, ldb, ldc;
  int batch, zdiv;         /* z in [0,batch): z1 = z / zdiv, z2 = z % zdiv          */
  int64_t sA1, sA2, sB1, sB2, sC1, sC2;
  int ksplit;              /* >1: split K, partial s goes to C + s*sCk (no epilogue) */
  int64_t sCk;
  float alpha;
  int accumulate;          /* C += result                                           */
  const float* bias; int bias_mode;   /* 0 none, 1 bias[n], 2 bias[m]                */
  /* activation applied to an operand while it is staged (h = act(drop(z))) */
  int act_a, act_b;        /* RPDE_ACT_*                                            */
  /* epilogue: C = acc * act'(drop(aux)) * dropscale   (backward through act), or with
   * RPDE_EPI_MULAUX: C = acc * aux (aux holds a stored derivative)                */
  int epi_dact;            /* RPDE_ACT_*, RPDE_EPI_MULAUX or 0                      */
  /* aux (row stride ldaux) and aux_out (row stride ldc) follow C's batch offsets: entry z is read / written at
   * z1*sC1 + z2*sC2 from their base pointers */
  const float* aux; int64_t ldaux;
  /* dropout shared by prologue / epilogue: element id = point*drop_ld + feature;
   * drop_where: bit 0 mask the A operand, bit 1 the B operand, bit 2 the epilogue's aux */
  float drop_p; uint64_t drop_seed; int64_t drop_ld;
  int write_act;           /* epilogue applies act (RPDE_ACT_*) to the stored value */
  int drop_where;
  /* optional: per-M-tile column sums of the stored C, [ceil(M/128)][N] floats (bias gradients
   * for free); needs M > 64, batch = ksplit = 1 and 16-byte aligned rows */
  float* colsum;
  /* with write_act and a non-null aux_out (same layout as C): the epilogue evaluates the activation
   * once per element, u = dropout(acc+bias): C = act(u), aux_out = act'(u) * dropscale -- so every
   * consumer of the hidden activation and of its derivative is a plain GEMM (drop_where bit 2) */
  float* aux_out;
  /* optional accelerator for a B operand shared by the whole batch (a weight matrix): the images written by
   * rpde_split_weights for this B (same N, K).  Results are bit-identical with and without it; B must
   * still be valid (the native fp32 kernels use it when the split-bf16 path does not apply). */
  const void* b_split;
  /* the same for an A operand shared by the whole batch (e.g. a DFT table): rpde_split_weights(A, a_kmajor,
   * lda, M, K).  With it and an x-major B, K need not be a multiple of 32. */
  const void* a_split;
  /* with accumulate: add this tensor (same layout and strides as C) instead of the old contents of C,
   * i.e. C = alpha*A.B + acc_src -- sums a skip-connection gradient without a separate pass */
  const float* acc_src;
  /* optional device counter folded into drop_seed by the kernel (8 bytes, read once per launch): lets a captured
   * hipGraph draw new masks at every replay -- see rpde_ff_params.seed_epoch */
  const uint64_t* drop_epoch;
} rpde_gemm_desc;
int rpde_gemm_f32(const rpde_gemm_desc* d, void* stream);

/* Pre-split a weight operand for the split-bf16 GEMM path: w is [N,K] (kmajor=1, row stride ld) or [K,N]
 * (kmajor=0); out receives rpde_split_weights_bytes(N,K) bytes: three bf16 images hi/mid/lo with
 * w = hi+mid+lo exactly, laid out as the kernel's LDS stages (k zero-padded to a multiple of 32). */
size_t rpde_split_weights_bytes(int N, int K);
int rpde_split_weights(const float* w, int kmajor, int64_t ld, int N, int K, void* out, void* stream);

/* ---- FSpectralConv1d.forward_fourier  (models/spectral_convolution.py:158-204)
 * x,out [B,n,C] channels-last; w [C,C,K,2]; keff=min(K,n/2+1) is clamped here
 * (quirk Q5).  spec_in [B, 2*kp, C] (kp = keff rounded up to 4) receives the
 * truncated input spectrum and must be kept for the backward call. */
size_t rpde_fspectral1d_ws_bytes(int B, int n, int C, int K);
size_t rpde_fspectral1d_spec_elems(int B, int n, int C, int K);
int rpde_fspectral1d_fwd(const float* x, const float* w, float* out, float* spec_in,
                         int B, int n, int C, int K, int mode, int norm,
                         void* ws, size_t ws_bytes, void* stream);
/* grad_skip (nullable, shaped like x): added into grad_x by the last GEMM's epilogue -- the gradient
 * arriving through a skip connection around the layer (x + FF(spectral(x))) costs no extra pass */
int rpde_fspectral1d_bwd(const float* grad_out, const float* spec_in, const float* w,
                         float* grad_x, float* grad_w, const float* grad_skip,
                         int B, int n, int C, int K, int mode, int norm,
                         void* ws, size_t ws_bytes, void* stream);

/* ---- FSpectralConv2d.forward_fourier  (models/spectral_convolution.py:256-318)
 * x,out [B,M,N,C]; w_y,w_x [C,C,K,2]; norm 'ortho' (hard-coded in the
 * reference, quirk Q4).  spec_y [B*M, 2*kpy, C], spec_x [B*N, 2*kpx, C]. */
size_t rpde_fspectral2d_ws_bytes(int B, int M, int N, int C, int K);
size_t rpde_fspectral2d_spec_elems(int B, int M, int N, int C, int K, int axis /*0:y 1:x*/);
int rpde_fspectral2d_fwd(const float* x, const float* w_y, const float* w_x, float* out,
                         float* spec_y, float* spec_x,
                         int B, int M, int N, int C, int K, int mode,
                         void* ws, size_t ws_bytes, void* stream);
int rpde_fspectral2d_bwd(const float* grad_out, const float* spec_y, const float* spec_x,
                         const float* w_y, const float* w_x,
                         float* grad_x, float* grad_wy, float* grad_wx, const float* grad_skip,
                         int B, int M, int N, int C, int K, int mode,
                         void* ws, size_t ws_bytes, void* stream);
/* The same for FSpectralConv2d.forward_fourier in evaluation: rpde_fspectral2d_prep_bytes (0: nothing to prepare for
 * this shape, use rpde_fspectral2d_fwd) bytes hold the mode-mix weight fragments of both axes; the forward then needs
 * rpde_fspectral2d_eval_ws_bytes of workspace (the spectra live there: nothing is saved for a backward; 0 where
 * rpde_fspectral2d_prep_bytes is 0). */
size_t rpde_fspectral2d_prep_bytes(int M, int N, int C, int K);
size_t rpde_fspectral2d_eval_ws_bytes(int B, int M, int N, int C, int K);
int rpde_fspectral2d_prepare(const float* w_y, const float* w_x, int M, int N, int C, int K,
                             void* prep, size_t prep_bytes, void* stream);
int rpde_fspectral2d_fwd_prepared(const float* x, const void* prep, float* out, int B, int M, int N, int C, int K,
                                  void* ws, size_t ws_bytes, void* stream);

/* The first layer of FFNO2D, whose input is h0 = W_in u + b_in with a thin u [B,M,N,Cin], Cin <= 4: the spectral branch
 * forward_fourier(h0) computed from u (the lifting commutes with the DFT and folds into the mode-mix weights).
 * w_in [C,Cin], b_in [C] or NULL, w_y,w_x [C,C,K,2], out [B,M,N,C].  spec_u: rpde_lifted_fspectral2d_spec_elems floats,
 * the spectra of u along both axes, all the backward needs besides the weights.  The backward returns the branch's
 * gradients of W_in, b_in, w_y, w_x (each may be NULL) and none for u.  rpde_lifted_fspectral2d_ok: 1 where the path
 * covers the shape (the fused 2-D path's shapes; RPDE_LIFTED_SPECTRAL=0 switches it off).  Workspace:
 * rpde_fspectral2d_ws_bytes(B, M, N, C, K). */
int rpde_lifted_fspectral2d_ok(int M, int N, int C, int Cin, int K);
size_t rpde_lifted_fspectral2d_spec_elems(int B, int M, int N, int Cin, int K);
int rpde_lifted_fspectral2d_fwd(const float* u, const float* w_in, const float* b_in, const float* w_y, const float* w_x,
                                float* out, float* spec_u, int B, int M, int N, int C, int Cin, int K,
                                void* ws, size_t ws_bytes, void* stream);
int rpde_lifted_fspectral2d_bwd(const float* grad_out, const float* spec_u, const float* w_in, const float* b_in,
                                const float* w_y, const float* w_x,
                                float* grad_w_in, float* grad_b_in, float* grad_wy, float* grad_wx,
                                int B, int M, int N, int C, int Cin, int K,
                                void* ws, size_t ws_bytes, void* stream);

/* ---- SpectralConv1d.forward  (models/spectral_convolution.py:38-55)
 * x [B,Cin,n] channels-first, w [Cin,Cout,K] complex64 (interleaved floats),
 * out [B,Cout,n]; norm 'backward'.  K > n/2+1 -> RPDE_ERR_MODES (quirk Q5).
 * act_in: activation applied to x while it is read (the FNO block feeds
 * act(previous pre-activation), fno_blocks.py:33).  spec_in [B*Cin, 2*kp]. */
size_t rpde_spectral1d_ws_bytes(int B, int Cin, int Cout, int n, int K);
int rpde_spectral1d_fwd(const float* x, const float* w, float* out, float* spec_in,
                        int B, int Cin, int Cout, int n, int K, int act_in,
                        void* ws, size_t ws_bytes, void* stream);
int rpde_spectral1d_bwd(const float* grad_out, const float* spec_in, const float* w,
                        const float* x, float* grad_x, float* grad_w,
                        int B, int Cin, int Cout, int n, int K, int act_in,
                        void* ws, size_t ws_bytes, void* stream);

/* ---- SpectralConv2d.forward  (models/spectral_convolution.py:79-98)
 * x [B,Cin,M,N], w1,w2 [Cin,Cout,m1,m2] complex64, out [B,Cout,M,N]; rows
 * [0,m1) use w1, rows [M-m1,M) use w2 and win on overlap (quirk Q6).
 * spec_in [B*Cin, 2*R, m2p] planar (R = 2*m1 retained rows). */
size_t rpde_spectral2d_ws_bytes(int B, int Cin, int Cout, int M, int N, int m1, int m2);
size_t rpde_spectral2d_spec_elems(int B, int Cin, int M, int N, int m1, int m2);
int rpde_spectral2d_fwd(const float* x, const float* w1, const float* w2, float* out, float* spec_in,
                        int B, int Cin, int Cout, int M, int N, int m1, int m2, int act_in,
                        void* ws, size_t ws_bytes, void* stream);
int rpde_spectral2d_bwd(const float* grad_out, const float* spec_in, const float* w1, const float* w2,
                        const float* x, float* grad_x, float* grad_w1, float* grad_w2,
                        int B, int Cin, int Cout, int M, int N, int m1, int m2, int act_in,
                        void* ws, size_t ws_bytes, void* stream);

/* ---- FeedForward  (models/custom_layer.py:49-68) + the residual glue of
 * FFNO*.forward (models/ffno.py:118,230) and FSpectralConv1d's act (:154).
 * x [P,dim] channels-last points.  Hidden layer l < L-1: z_l = in_l @ W_l^T + b_l
 * never reaches HBM; the GEMM epilogue evaluates the activation once per element,
 * u = dropout(z_l): hs[l] = gelu(u) ([P,out_l], input of the next GEMM and of the
 * weight-gradient GEMM) and ds[l] = gelu'(u) * dropscale (what backward multiplies
 * by; pass ds = NULL or ds[l] = NULL when no gradient is needed).  The last layer
 * stores z_last ([P,dim]) and out = residual + post_act( LayerNorm( dropout(z_last) ) )
 * (LN optional, residual may be NULL).  Dropout masks come from a counter hash of
 * (seed, layer, element) defined in csrc/drop_hash.h and restated in oracle/dropout_mask.py.
 * Any n_layers >= 1 is accepted, forward and backward alike. */
typedef struct {
  int n_layers; int dim; int factor;
  int layer_norm; float ln_eps;
  float dropout_p; uint64_t seed;      /* p = 0 in eval mode                         */
  int post_act;                        /* RPDE_ACT_*                                 */
  const float* const* weights;         /* [n_layers] W_l [out_l, in_l]               */
  const float* const* biases;          /* [n_layers] b_l [out_l]                     */
  const float* ln_gamma; const float* ln_beta;
  /* optional (may be NULL): device address of a 64-bit counter that every kernel of the call mixes into the seed.
   * A hipGraph replays its launch arguments, so a host-drawn seed alone would repeat one mask for ever; the training
   * step advances this counter on the device once per step (between backward and the next forward), and forward and
   * backward of a step read the same value.  The reference draws its masks from torch's generator
   * (models/custom_layer.py:60, nn.Dropout): against it parity is statistical; against the float64 oracle fed the
   * restated masks it is element by element (tests/test_gpu_dropout_parity.py). */
  const uint64_t* seed_epoch;
} rpde_ff_params;
size_t rpde_feedforward_ws_bytes(int64_t P, int dim, int factor, int n_layers);      /* backward */
/* forward scratch (optional: ws may be NULL; with it each weight is pre-split once per call for the
 * split-bf16 GEMMs -- faster, bit-identical output) */
size_t rpde_feedforward_fwd_ws_bytes(int dim, int factor, int n_layers);
/* 1 when rpde_feedforward_fwd (given its scratch) runs this shape as ONE fused kernel (dim 64, factor 4, three
 * layers: hidden activations never reach HBM).  Pointer contract of the fused path, forward and backward alike:
 *   hs and ds NULL ............ evaluation: only `out` is written;
 *   hs[0..1] and ds[0..1] ..... training: h and d = gelu'(u) * dropscale of both hidden layers and z_last are
 *                               stored by the forward and consumed by rpde_feedforward_bwd;
 *   hs[0..1] only (ds NULL) ... training in recompute mode: hs receive u = dropout(z) and the backward kernels
 *                               re-evaluate gelu / gelu' from them (half the saved bytes; measured slower).
 * The weight gradients of these shapes come from the streaming kernel of csrc/wgrad_h2.hip (for the first layer
 * together with grad_x), bias / gamma / beta gradients from per-workgroup partial sums folded in fixed order. */
int rpde_feedforward_is_fused(int dim, int factor, int n_layers, int64_t P);
int rpde_feedforward_fwd(const rpde_ff_params* p, const float* x, const float* residual,
                         float* const* hs, float* const* ds, float* z_last, float* out, int64_t P,
                         void* ws, size_t ws_bytes, void* stream);
int rpde_feedforward_bwd(const rpde_ff_params* p, const float* x, const float* const* hs,
                         const float* const* ds, const float* z_last,
                         const float* grad_out, float* grad_x,
                         float* const* grad_weights, float* const* grad_biases,
                         float* grad_gamma, float* grad_beta, int64_t P,
                         void* ws, size_t ws_bytes, void* stream);
/* Evaluation with frozen weights (rollouts, all-resolution sweeps, validation): the fused kernel's weight fragments are
 * built once by rpde_feedforward_prepare into a caller-owned buffer of rpde_feedforward_fwd_ws_bytes bytes and reused
 * by rpde_feedforward_fwd_prepared until the caller knows the weights have changed.  Fused shapes only
 * (rpde_feedforward_is_fused); dropout_p must be 0. */
int rpde_feedforward_prepare(const rpde_ff_params* p, void* prep, size_t prep_bytes, void* stream);
int rpde_feedforward_fwd_prepared(const rpde_ff_params* p, const float* x, const float* residual, float* out, int64_t P,
                                  const void* prep, size_t prep_bytes, void* stream);

/* ---- pointwise linear, channels-last: nn.Linear / WNLinear applied to
 * [P,in] (models/ffno.py:113,121,225,233; custom_layer.py:70).  Weight-norm is
 * resolved by the caller into an effective weight. */
size_t rpde_linear_ws_bytes(int64_t P, int in_f, int out_f);
int rpde_linear_fwd(const float* x, const float* w, const float* b, float* out,
                    int64_t P, int in_f, int out_f, void* stream);
int rpde_linear_bwd(const float* x, const float* w, const float* grad_out,
                    float* grad_x, float* grad_w, float* grad_b,
                    int64_t P, int in_f, int out_f, void* ws, size_t ws_bytes, void* stream);

/* Weight normalisation of WNLinear (models/custom_layer.py:70-108: torch.nn.utils.weight_norm on dim 0, parameters
 * weight_g [out,1], weight_v [out,in]):  w = v * (g / |v|_row), and its adjoint -- one launch each where autograd runs
 * a dozen ATen kernels per projection.  grad_v or grad_g may be null. */
int rpde_weight_norm_fwd(const float* v, const float* g, float* w, int out_f, int in_f, void* stream);
int rpde_weight_norm_bwd(const float* v, const float* g, const float* grad_w, float* grad_v, float* grad_g,
                         int out_f, int in_f, void* stream);

/* ---- 1x1 convolution, channels-first: nn.Conv1d/Conv2d(k=1) lifting, bypass
 * and projection (models/fno.py:30,93; fno_blocks.py:29,38-39,67,76-77).
 * x [B,Cin,S], w [Cout,Cin], out [B,Cout,S] (S = flattened spatial size).
 * act_in is applied to x while staged; accumulate adds into out (the FNO
 * block's spectral_conv(x) + bypass_conv(x)). */
size_t rpde_conv1x1_ws_bytes(int B, int Cin, int Cout, int64_t S);
int rpde_conv1x1_fwd(const float* x, const float* w, const float* b, float* out,
                     int B, int Cin, int Cout, int64_t S, int act_in, int accumulate, void* stream);
/* the same with an activation applied to the result before it is stored (evaluation-mode FNO blocks:
 * out = act(spectral + W . x + b) written once, models/fno_blocks.py:25-45 of the reference) */
int rpde_conv1x1_act_fwd(const float* x, const float* w, const float* b, float* out,
                         int B, int Cin, int Cout, int64_t S, int act_in, int accumulate, int act_out, void* stream);
/* evaluation-mode FNOBlock2d in one entry point: out = act_out(SpectralConv2d(x; w1, w2) + Conv2d_1x1(x; wc, bc)),
 * reference models/fno_blocks.py:63-83 with models/spectral_convolution.py:79-98.  The inverse DFT along the last
 * axis, the bypass convolution, bias and activation run as ONE streaming pass over x: the spectral branch is never
 * written.  x [B,Cin,M,N], w1/w2 complex [Cin,Cout,m1,m2] (as float pairs), wc [Cout,Cin], out [B,Cout,M,N].
 * rpde_fnoblock2d_eval_ok: 1 when the shape is covered (Cout <= 32, N % 4 == 0, N divides 1024 or is a multiple of it, and the
 * block's weights plus its rows' 2 * ceil4(m2) spectrum entries fit 64 KB of LDS). */
size_t rpde_fnoblock2d_eval_ws_bytes(int B, int Cin, int Cout, int M, int N, int m1, int m2);
int rpde_fnoblock2d_eval_ok(int Cin, int Cout, int M, int N, int m2);
int rpde_fnoblock2d_eval_fwd(const float* x, const float* w1, const float* w2, const float* wc, const float* bc, float* out,
                             int B, int Cin, int Cout, int M, int N, int m1, int m2, int act_out,
                             void* ws, size_t ws_bytes, void* stream);
/* the LAST block of an FNO2d and its projection MLP in evaluation, one entry point (reference models/fno.py:143-150:
 * fno_blocks[-1] -> projection = mlp2(gelu(mlp1(.)))): out [B,Cq,M,N] = pw2 . gelu(pw1 . act_out(SpectralConv2d(x) +
 * Conv2d_1x1(x)) + pb1) + pb2 with pw1 [Cmid,Cout], pw2 [Cq,Cmid].  The block's output never reaches HBM.  Workspace:
 * rpde_fnoblock2d_eval_ws_bytes.  _ok: Cin = 32, Cout <= 32, Cmid <= 128, Cq <= 4, N % 64 == 0, N <= 1024, m2 <= 16. */
int rpde_fnoblock2d_proj_eval_ok(int Cin, int Cout, int M, int N, int m1, int m2, int Cmid, int Cq);
int rpde_fnoblock2d_proj_eval_fwd(const float* x, const float* w1, const float* w2, const float* wc, const float* bc,
                                  const float* pw1, const float* pb1, const float* pw2, const float* pb2, float* out, int B,
                                  int Cin, int Cout, int M, int N, int m1, int m2, int act_out, int Cmid, int Cq,
                                  void* ws, size_t ws_bytes, void* stream);
/* FNO2d.forward in evaluation, up to and including the first block (reference models/fno.py:121-147:
 * cat(x, gridx, gridy) -> lifting -> fno_blocks[0]), without the lifted field ever being written or read:
 * u [B,1,M,N], gx [M], gy [N] (the grid coordinates, device arrays), wl [C,3], bl [C] (lifting conv), then the block's
 * parameters as for rpde_fnoblock2d_eval_fwd.  out [B,Cout,M,N]. */
size_t rpde_fno2d_lift_block_eval_ws_bytes(int B, int C, int Cout, int M, int N, int m1, int m2);
int rpde_fno2d_lift_block_eval_ok(int Cu, int C, int Cout, int M, int N, int m1, int m2);
int rpde_fno2d_lift_block_eval_fwd(const float* u, const float* gx, const float* gy, const float* wl, const float* bl,
                                   const float* w1, const float* w2, const float* wc, const float* bc, float* out, int B, int C,
                                   int Cout, int M, int N, int m1, int m2, int act_out, void* ws, size_t ws_bytes, void* stream);
/* the projection MLP mlp2(gelu(mlp1(act_in(x)))) of models/fno_blocks.py:38-45,76-83 in one pass, EVALUATION only
 * (the hidden tensor [B,Cmid,S] is never written; training keeps the two convolutions, whose backward needs it):
 * x [B,Cin,S], w1 [Cmid,Cin], b1 [Cmid], w2 [Cout,Cmid], b2 [Cout], out [B,Cout,S].  rpde_conv_mlp_ok: 1 when the
 * shape is covered (Cin 32 with Cmid <= 128, or Cin 64 with Cmid <= 64; Cout <= 4; S % 16 == 0). */
int rpde_conv_mlp_ok(int Cin, int Cmid, int Cout, int64_t S);
int rpde_conv_mlp_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* out,
                      int B, int Cin, int Cmid, int Cout, int64_t S, int act_in, void* stream);
int rpde_conv1x1_bwd(const float* x, const float* w, const float* grad_out,
                     float* grad_x, float* grad_w, float* grad_b,
                     int B, int Cin, int Cout, int64_t S, int act_in, int accumulate_gx,
                     void* ws, size_t ws_bytes, void* stream);

/* ---- grid channels + layout change at the model boundary
 * (models/ffno.py:92,201-222; fno.py:51,121-139): builds the lifted input
 * [.., Cin+G] (channels-last) or [B,Cin+G,S] (channels-first) with
 * endpoint-inclusive linspace coordinates (quirk Q10) generated on device. */
int rpde_concat_grid(const float* x, float* out, int B, int Cin, int M, int N /*1 for 1-D*/,
                     int grid_dims /*0,1,2*/, double lo, double hi, int channels_last,
                     const float* gridx, const float* gridy, void* stream);
/* [B,S,C] <-> [B,C,S] */
int rpde_transpose_cs(const float* in, float* out, int B, int64_t S, int C, int to_channels_first, void* stream);

/* ---- spectral resize: rfft -> shared bins -> irfft at the new size, x out/in
 * (reference: utils/res_utils.py:29-50 `resize`, :93-125 `resize_1d`; used by the
 * all-resolution evaluators, utils/naive_utils.py, utils/resize_utils.py;
 * csrc/resize.hip on the transforms of csrc/cf_dft.h).
 * x [rows, n_in] -> out [rows, n_out];  x [rows, M, N] -> out [rows, Mo, No]. */
size_t rpde_resize1d_ws_bytes(int64_t rows, int n_in, int n_out);
int rpde_resize1d(const float* x, float* out, int64_t rows, int n_in, int n_out,
                  void* ws, size_t ws_bytes, void* stream);
size_t rpde_resize2d_ws_bytes(int64_t rows, int M, int N, int Mo, int No);
int rpde_resize2d(const float* x, float* out, int64_t rows, int M, int N, int Mo, int No,
                  void* ws, size_t ws_bytes, void* stream);

/* ---- error by frequency (reference: utils/frequency_error.py `decompose_error_by_frequency_1d`, one irfft of the
 * batch and one .item() per mode, and `decompose_error_by_frequency_2d`, two irfft2 and two .item() per radial bin;
 * driven by frequency_evaluation.py / utils/multiresolution_analysis.py).  By Parseval those norms are weighted sums
 * of |rfft|^2: one forward transform of (pred - target) -- the difference is formed in fp32 BEFORE the transform --
 * and of target, squared and reduced on the device.
 *   acc [2, n_out] float64: row 0 error energy, row 1 solution energy, ADDED TO (zero it before the first batch);
 *   the reference's magnitudes are sqrt(acc) once the test set has streamed through.  No floating-point atomics:
 *   identical calls give identical bits.
 * 1-D: pred, target [rows, n] (rows = batch * channels), n_out = num_modes <= n/2+1 (more: RPDE_ERR_MODES),
 *   acc[.][k] += w_k / n * sum_rows |Z[row,k]|^2, w_k = 1 at DC and (even n) Nyquist, else 2.
 * 2-D: pred, target [images, H, W]; bins [H, W/2+1] int32 on the device, the radial bin of every half-spectrum entry
 *   or -1 for none, -1 <= bin < n_bins (built and range-checked by the caller: rpde/ops.py radial_bins), n_out = n_bins,
 *   acc[.][i] += 1/(H W) * sum_{(ky,kx) in bin i} w_kx sum_images |Z[image,ky,kx]|^2.
 *   The batch goes through the workspace in chunks of images: rpde_freq_energy2d_ws_bytes stops growing with
 *   `images` once a chunk (16 MiB of half-spectra) is full.
 * Sizes: 2 <= n, H, W <= 4096 (the full-spectrum tables grow with the square of the axis; they are cached per
 * (n, num_modes) for the life of the process); the workspace must be 16-byte aligned.
 * Argument errors (null pointers, sizes out of range, n_bins < 1, short or misaligned workspace) are reported before
 * any device work. */
size_t rpde_freq_energy1d_ws_bytes(int64_t rows, int n, int num_modes);
int rpde_freq_energy1d(const float* pred, const float* target, double* acc, int64_t rows, int n, int num_modes,
                       void* ws, size_t ws_bytes, void* stream);
size_t rpde_freq_energy2d_ws_bytes(int64_t images, int H, int W);
int rpde_freq_energy2d(const float* pred, const float* target, const int32_t* bins, double* acc, int64_t images,
                       int H, int W, int n_bins, void* ws, size_t ws_bytes, void* stream);

/* ---- elementwise activation: out = act(x); backward dx = g * act'(x) */
int rpde_act_fwd(const float* x, float* out, int64_t n, int act, void* stream);
int rpde_act_bwd(const float* x, const float* g, float* dx, int64_t n, int act, void* stream);

/* ---- RelativeL2Loss.forward (utils/loss.py:31-59): rel[b] = |x-y|_2/(|y|_2+1e-8).
 * rel [B]; loss scalar = mean (size_average) or sum; pass loss=NULL for
 * reduction=False.  stats (rpde_rel_l2_stats_elems(B) floats: per-sample diff
 * norm and y norm, then scratch partials) is kept for backward. */
int64_t rpde_rel_l2_stats_elems(int B);
int rpde_rel_l2_fwd(const float* x, const float* y, float* rel, float* loss, float* stats,
                    int B, int64_t per, int size_average, void* stream);
/* grad_rel [B] if reduction=False else NULL with grad_loss a device scalar */
int rpde_rel_l2_bwd(const float* x, const float* y, const float* stats,
                    const float* grad_loss, const float* grad_rel, float* grad_x,
                    int B, int64_t per, int size_average, void* stream);

/* ---- mode-weighted relative L2 loss (csrc/spectral_loss.hip, utils/loss.py SpectralRelativeL2Loss; an interface
 * addition, the reference has none).  x, y [B, C, M, N] fp32 channels-first, M = 1 for one-dimensional fields [B, C, N]; omega [M, N/2+1] >= 0, rows
 * in fft order.  With Z = rfft / rfft2 (unnormalised) and c_kx = 1 at kx = 0 and (even N) kx = N/2, else 2:
 *   E(z)[b] = sum_c sum_k omega_k c_kx / (M N) |Z[b,c,k]|^2,   rel[b] = sqrt(E(x - y)[b]) / (sqrt(E(y)[b]) + 1e-8);
 * x - y is formed in fp32 before the transform; the sums are float64, two deterministic stages without atomics.
 * rel [B] or NULL; loss: device scalar = mean (size_average) or sum, NULL for reduction=False; stats: 2 B floats
 * (sqrt E_d, sqrt E_y per sample) and spec_d (the spec_elems query's count of floats: the spectrum of x - y) are kept for backward.
 * Backward: grad_x[b] = coef_b irfft(omega . spec_d[b]), coef_b = g_b / (sqrt(E_d) (sqrt(E_y) + 1e-8)), 0 where
 * E_d = 0, formed on the device; g_b = grad_rel[b], or grad_loss[0] (/ B when size_average) with grad_rel NULL.
 * No gradient for y.  In 2-D the columns kx = 0 and (even N) kx = N/2 of omega must be symmetric in ky
 * (omega[ky] == omega[(M - ky) % M]): the caller checks it.  Axes 2 .. 4096; the full-spectrum plans are those of the
 * resizers at equal sizes (cf_rfft2_plans, csrc/cf_dft.h, through csrc/halfspec.h; first use of a grid allocates and synchronises).  Argument errors are reported before any
 * device work. */
size_t rpde_wrel_l2_ws_bytes(int B, int C, int M, int N);
size_t rpde_wrel_l2_spec_elems(int B, int C, int M, int N);
int rpde_wrel_l2_fwd(const float* x, const float* y, const float* omega, float* rel, float* loss, float* stats,
                     float* spec_d, int B, int C, int M, int N, int size_average, void* ws, size_t ws_bytes, void* stream);
int rpde_wrel_l2_bwd(const float* spec_d, const float* omega, const float* stats, const float* grad_loss,
                     const float* grad_rel, float* grad_x, int B, int C, int M, int N, int size_average,
                     void* ws, size_t ws_bytes, void* stream);

/* ---- per-sample, per-band spectral energies, forward and backward (csrc/band_energy.hip, rpde.ops.band_energy;
 * utils/loss.py BandRelativeL2Loss and SpectrumMatchingLoss; an interface addition, the reference has none).
 * x, y [B, C, M, N] fp32 channels-first, M = 1 for one-dimensional fields.  The field z is x, or x - y formed in fp32
 * before the transform when y is not NULL.  With Z = rfft / rfft2 (unnormalised), c_kx = 1 at kx = 0 and (even N)
 * kx = N/2, else 2, and a band in {-1, 0 .. J-1} for every entry (ky, kx) of the half spectrum, rows in fft order:
 *   E[b, j] = sum_c sum_{(ky,kx): band = j} c_kx / (M N) |Z[b,c,ky,kx]|^2          E [B, J] floats
 * Entries of band -1 belong to no band; if every entry has one, sum_j E[b, j] = sum |z[b]|^2 (Parseval).
 * Backward, for gE [B, J]:  grad_x[b, c] = 2 irfft2(gE[b, band(ky,kx)] Z[b,c,ky,kx]), weight 0 where band = -1, irfft2
 * with 1 / (M N) and Im of the self-conjugate bins of the last axis ignored.  No gradient for y.  It is the gradient
 * only if, in 2-D, the columns kx = 0 and (even N) kx = N/2 of the band table are symmetric in ky
 * (band[ky] == band[(M - ky) % M]): the caller checks it (rpde.ops.check_band_table).
 * Device tables, int32, built once per (grid, table) by the caller (rpde.ops.band_tables):
 *   forward   entries [n_entries], start [J+1]: band j owns entries[start[j] .. start[j+1]), each entry
 *             (offset << 1) | (c_kx == 2), offset = ky 2 kp + kx: where Re of (ky, kx) sits in ONE image's half spectrum
 *             (Im is kp further), kp = N/2+1 rounded up to 4; entries of band -1 are not listed
 *   backward  band [M][kp]: the band of every entry, the padded columns -1; 16-byte aligned
 * The kernels skip an offset outside the image, a start[] outside entries[] and a band outside 0 .. J-1.
 * spec (the spec_elems query's count of floats, or NULL: not kept) receives the half spectrum of z,
 * [B C][M][re|im][kp] with the padded columns zero, and is what the backward call takes.
 * Grids as rpde_wrel_l2_* (axes 2 .. 4096) with 1 <= J <= 4096: otherwise the two queries return 0.  The transforms
 * and plans are those of rpde_wrel_l2_* (first use of a grid allocates and synchronises).  The sums are float64 in two
 * fixed-order stages without atomics: identical calls give identical bits, and a sample's energies do not depend on
 * the batch around it.  The workspace is 256-byte aligned.  Argument errors are reported before any device work. */
size_t rpde_band_energy_ws_bytes(int B, int C, int M, int N, int J);
size_t rpde_band_energy_spec_elems(int B, int C, int M, int N);
int rpde_band_energy_fwd(const float* x, const float* y, const int32_t* entries, const int32_t* start, int n_entries,
                         float* E, float* spec, int B, int C, int M, int N, int J, void* ws, size_t ws_bytes,
                         void* stream);
int rpde_band_energy_bwd(const float* spec, const int32_t* band, const float* gE, float* grad_x, int B, int C, int M,
                         int N, int J, void* ws, size_t ws_bytes, void* stream);

/* ---- NS vorticity generator (reference: data_generation/ns_2d.py, random_fields.py): 2-D Navier-Stokes in vorticity
 * form on the periodic unit square, pseudo-spectral (csrc/ns_solver.hip), and the Gaussian random field that seeds it
 * and the rfft2 / irfft2 calls (csrc/halfspec.hip), on the half-spectrum layer of csrc/halfspec.h over the 2-D transforms of
 * csrc/cf_dft.h.
 * Grids M x N, both axes even, 4 .. 4096.  A half spectrum is [images][M][re|im][kp] floats: rows ky in fft order
 * (signed k1 = ky < M/2 ? ky : ky - M), kx = k2 = 0 .. N/2 contiguous, kp = N/2+1 rounded up to 4, padded columns zero;
 * the spec_elems query gives the floats of B images.  The rfft2 / irfft2 calls are torch.fft.rfft2 (unnormalised) and
 * irfft2 (1 / (M N); Im of the self-conjugate bins of the last axis ignored) between w [B, M, N] and that layout.
 * The steps call advances W in place by nsteps steps of
 *   psi = W inv_lap,  q = irfft2(2 pi i k2 psi),  v = irfft2(-2 pi i k1 psi),  w_x = irfft2(2 pi i k1 W),
 *   w_y = irfft2(2 pi i k2 W),  F = rfft2(q w_x + v w_y),  W <- c_w W - c_f F + g_h
 * with the tables c_w, c_f, inv_lap [M][kp] (padded columns zero) formed by the caller in float64 and rounded once:
 *   a = dt visc lap / 2, lap = 4 pi^2 (k1^2 + k2^2):  c_w = (1 - a) / (1 + a),  c_f = dt dealias / (1 + a),
 *   inv_lap = 1 / lap (1 at the mean mode),  dealias = |k1| <= (2/3)(M/2) and |k2| <= (2/3)(N/2);
 * g_h = dt / (1 + a) rfft2(f): one spectrum (g_batched = 0) or B (g_batched = 1); the scale call forms it, out =
 * table . spec, once per solve.  Six launches per step on the caller's stream, no host synchronisation, no atomics:
 * identical calls give identical bits, and k calls of n steps equal one call of k n steps bit for bit.
 * The grf2d call: noise [B, M, N, 2] (the complex coefficients of the full grid), sqrt_eig [M, N] -> out [B, M, N] =
 * Re ifft2(sqrt_eig . noise) with 1 / (M N), through the Hermitian-symmetrised half spectrum and the same inverse.
 * State, forcing and tables 16-byte aligned, workspaces (the ns2d ws query covers all four ns2d calls) 256-byte
 * aligned; the ws / spec queries return 0 for sizes the calls refuse (odd or out-of-range axes, 4 B max(M, N) >= 2^31).
 * The full-spectrum plans are those of the mode-weighted loss: the first use of a grid allocates and synchronises.
 * Argument errors are reported before any device work. */
size_t rpde_ns2d_ws_bytes(int B, int M, int N);
size_t rpde_ns2d_spec_elems(int B, int M, int N);
int rpde_ns2d_rfft2(const float* w, float* W, int B, int M, int N, void* ws, size_t ws_bytes, void* stream);
int rpde_ns2d_irfft2(const float* W, float* w, int B, int M, int N, void* ws, size_t ws_bytes, void* stream);
int rpde_ns2d_scale(const float* spec, const float* table, float* out, int B, int M, int N, void* stream);
int rpde_ns2d_steps(float* W, const float* g_h, int g_batched, const float* c_w, const float* c_f, const float* inv_lap,
                    int B, int M, int N, int nsteps, void* ws, size_t ws_bytes, void* stream);
size_t rpde_grf2d_ws_bytes(int B, int M, int N);
int rpde_grf2d(const float* noise, const float* sqrt_eig, float* out, int B, int M, int N,
               void* ws, size_t ws_bytes, void* stream);

/* ---- active-scalar Navier-Stokes generator (csrc/ns_solver.hip, SCALAR; an interface addition, the reference has no
 * generator for its active-matter files): the vorticity equation above with a scalar c that the flow advects and that
 * drives the flow back through buoyancy along axis 2 (Boussinesq; the curl of the force is beta dc/dx1), on the same
 * half-spectrum layer and grids.  The state is two half spectra per sample in the layout above,
 * S = [W_0 .. W_{B-1}, C_0 .. C_{B-1}], 2 B images.  With psi, k1, k2, lap and dealias as above, the steps call advances S
 * in place by nsteps steps of
 *   q = irfft2(2 pi i k2 psi),  v = irfft2(-2 pi i k1 psi),  w_1, w_2 = irfft2(2 pi i k1 W), irfft2(2 pi i k2 W),
 *   c_1, c_2 = irfft2(2 pi i k1 C), irfft2(2 pi i k2 C),
 *   F_w = rfft2(q w_1 + v w_2) - beta 2 pi i k1 C  (C of the old time level),   F_c = rfft2(q c_1 + v c_2),
 *   W <- c_w W - c_f F_w + g_h,   C <- d_w C - d_f F_c
 * with the tables c_w, c_f, d_w, d_f, inv_lap [M][kp] (padded columns zero) formed by the caller in float64 and rounded
 * once (rpde.ops.nsc2d_tables): c_w, c_f, inv_lap as above, and with b = dt kappa lap / 2:
 *   d_w = (1 - b) / (1 + b),  d_f = dt dealias / (1 + b);
 * g_h as above, from rpde_ns2d_scale: one spectrum (g_batched = 0) or B (g_batched = 1); beta a scalar.  Six launches
 * per step on the caller's stream (a fused update + fan-out of the six derivative spectra, the inverse transform of the
 * 6 B images in two launches, the two products, the forward transform of the 2 B products in two launches), no host
 * synchronisation, no atomics: identical calls give identical bits, and k calls of n steps equal one call of k n steps
 * bit for bit.  nsteps == 0 is a no-op.
 * The fields call: out [B, 3, M, N] = (c, q, v) of S, the concentration and the velocity u = (q, v) -- one fan-out and
 * one inverse transform of 3 B images.
 * State, forcing, tables and out 16-byte aligned, the workspace (the ws query covers both calls) 256-byte aligned; the
 * ws query returns 0 for sizes the calls refuse: odd or out-of-range axes, and a B whose 6 B derivative images are
 * no generator grid (6 B > 65535 or 24 B max(M, N) >= 2^31).  The plans are those of the NS generator: the first use
 * of a grid allocates and synchronises.  Argument errors are reported before any device work. */
size_t rpde_nsc2d_ws_bytes(int B, int M, int N);
int rpde_nsc2d_steps(float* S, const float* g_h, int g_batched, const float* c_w, const float* c_f, const float* d_w,
                     const float* d_f, const float* inv_lap, float beta, int B, int M, int N, int nsteps, void* ws,
                     size_t ws_bytes, void* stream);
int rpde_nsc2d_fields(const float* S, const float* inv_lap, float* out, int B, int M, int N, void* ws, size_t ws_bytes,
                      void* stream);

/* ---- 1-D exponential-time-differencing generator (csrc/etd1d.hip; the rfft / irfft and grf1d calls are the M = 1 case of
 * the NS generator's in csrc/halfspec.hip, on the 1-D transforms of csrc/cf_dft.h): every
 * equation u_t = L u - (c/2) (u^2)_x on a periodic domain of length len -- Burgers (L = nu_eff d_xx) and
 * Kuramoto-Sivashinsky (L = -d_xx - nu d_xxxx) -- and the 1-D Gaussian random field.
 * Grid N even, 4 .. 4096.  A half spectrum is [images][re|im][kp] floats, k = 0 .. N/2 contiguous, kp = N/2+1 rounded
 * up to 4, padded columns zero -- the layout above with one row; the spec_elems query gives the floats of B images.  The rfft / irfft calls are
 * torch.fft.rfft (unnormalised) and irfft (1 / N; Im of the mean and Nyquist bins ignored) between u [B, N] and that
 * layout.  With kappa_n = 2 pi n / len, the symbol l_n = c2 kappa_n^2 + c4 kappa_n^4 and the step h, the caller forms
 * seven tables [kp] (padded entries zero) in float64 and rounds them to fp32 once -- ETDRK4 in the Kassam-Trefethen
 * form, z = h l_n, LR = z + r_m, r_m = exp(i pi (m - 1/2) / 32), m = 1 .. 32, <.> the mean over m:
 *   E  = e^z,  E2 = e^(z/2),  Q = h Re<(e^(LR/2) - 1) / LR>,
 *   f1 = h Re<(-4 - LR + e^LR (4 - 3 LR + LR^2)) / LR^3>,  f2 = h Re<(2 + LR + e^LR (-2 + LR)) / LR^3>,
 *   f3 = h Re<(-4 - 3 LR - LR^2 + e^LR (4 - LR)) / LR^3>,
 *   g  = -(c/2) kappa_n dealias_n,  dealias_n = [n <= (2/3)(N/2)] or 1,  g_{N/2} = 0.
 * The steps call advances the spectrum v = U in place by nsteps steps of, with Nhat(w) = i g rfft(irfft(w)^2),
 *   Nv = Nhat(v), a = E2 v + Q Nv;   Na = Nhat(a), b = E2 v + Q Na;   Nb = Nhat(b), c = E2 a + Q (2 Nb - Nv);
 *   Nc = Nhat(c), v <- E v + f1 Nv + 2 f2 (Na + Nb) + f3 Nc.
 * Sixteen launches per step on the caller's stream (per stage: the inverse transform, the square, the forward
 * transform, the fused stage kernel), no host synchronisation, no atomics:
 * identical calls give identical bits, and k calls of n steps equal one call of k n steps bit for bit.
 * The grf1d call: noise [B, N, 2] (complex coefficients in fft order), sqrt_eig [N] -> out [B, N] =
 * Re ifft(sqrt_eig . noise) with 1 / N, through the Hermitian-symmetrised half spectrum and the same inverse.
 * State and tables 16-byte aligned (noise 8), the workspaces of the steps and grf1d calls 256-byte aligned (the
 * transforms alone need none); the ws / spec queries return 0 for sizes the calls refuse (odd or out-of-range N, B outside 1 .. 65535).
 * nsteps == 0 is a no-op.  The first use of a grid builds its plan: it allocates and synchronises once.
 * Argument errors are reported before any device work.
 * The steps_cx call is the same step for a symbol with odd derivatives (advection, dispersion: Korteweg-de Vries),
 *   l_n = c2 kappa_n^2 + c4 kappa_n^4 + i (c1 kappa_n + c3 kappa_n^3),  Im l_{N/2} = 0
 * (an odd derivative of the Nyquist mode vanishes on the grid; its bin of a real field stays real).  E, E2, Q, f1, f2, f3
 * are then complex, each [re|im][kp] floats -- the plane layout of a spectrum, padded columns zero -- and g stays real
 * [kp].  z = h l_n is complex, so the contour is the full circle and the mean is the complex mean, no Re:
 *   LR = z + r_m,  r_m = exp(2 pi i (m - 1/2) / 64),  m = 1 .. 64;   E = e^z,  E2 = e^(z/2),  Q = h <(e^(LR/2) - 1) / LR>,
 *   f1 = h <(-4 - LR + e^LR (4 - 3 LR + LR^2)) / LR^3>,  f2 = h <(2 + LR + e^LR (-2 + LR)) / LR^3>,
 *   f3 = h <(-4 - 3 LR - LR^2 + e^LR (4 - LR)) / LR^3>
 * (the upper half circle with Re<.> above is this mean for real z only; where z is real the imaginary parts are zero).  Same state, workspace (the ws query), launch
 * sequence, alignment and error rules as the steps call; every coefficient product is a complex one in fused
 * multiply-adds.  The steps call itself, its tables and its bits are unchanged. */
size_t rpde_etd1d_ws_bytes(int B, int N);
size_t rpde_etd1d_spec_elems(int B, int N);
int rpde_etd1d_rfft(const float* u, float* U, int B, int N, void* stream);
int rpde_etd1d_irfft(const float* U, float* u, int B, int N, void* stream);
int rpde_etd1d_steps(float* U, const float* E, const float* E2, const float* Q, const float* f1, const float* f2,
                     const float* f3, const float* g, int B, int N, int nsteps, void* ws, size_t ws_bytes, void* stream);
int rpde_etd1d_steps_cx(float* U, const float* E, const float* E2, const float* Q, const float* f1, const float* f2,
                        const float* f3, const float* g, int B, int N, int nsteps, void* ws, size_t ws_bytes,
                        void* stream);
size_t rpde_grf1d_ws_bytes(int B, int N);
int rpde_grf1d(const float* noise, const float* sqrt_eig, float* out, int B, int N, void* ws, size_t ws_bytes,
               void* stream);

/* ---- equation-residual loss of the 1-D ETD family, forward and backward (csrc/etd_residual.hip, rpde.ops.etd1d_residual;
 * utils/loss.py EquationResidualLoss; an interface addition, the reference has none).  It asks a one-step map x = u(t) ->
 * p ~ u(t + D) to satisfy u_t = L u - (c/2) (u^2)_x itself.  p, x [B, N] fp32, grid, length, kappa_n, the symbol l_n
 * (complex in general, Im l_{N/2} = 0) and g_n as in the generator block above; D is the time between the two fields (the
 * snapshot interval of a data set, not a solver's step).  The exact solution obeys
 *   u^(t + D) = e^(D l) u^(t) + int_0^D e^((D - s) l) Nhat(u(t + s)) ds,   Nhat(w) = i g rfft(w^2);
 * interpolating Nhat linearly between the two ends (the exponential trapezoidal rule, ETD2: exact in the linear part
 * however stiff) leaves the residual, with z = D l_n,
 *   r^_n = p^_n - E_n x^_n - m0_n rfft(x^2)_n - m1_n rfft(p^2)_n,
 *   E = e^z,   m0 = D (phi1(z) - phi2(z)) i g,   m1 = D phi2(z) i g,
 *   phi1 = <(e^LR - 1) / LR>,  phi2 = <(e^LR - 1 - LR) / LR^2>,  LR = z + r_m,  r_m = exp(2 pi i (m - 1/2) / 64), m = 1 .. 64,
 * <.> the complex mean.  The caller forms the three tables in float64 / complex128 and rounds them to fp32 once
 * (rpde.ops.etd1d_residual_tables); they are always complex, each [re|im][kp] floats -- the plane layout of a spectrum,
 * padded columns zero, Im E = 0 where z is real, m0 = m1 = 0 at n = 0 and N/2 -- with g (de-aliasing and c) folded in.
 *   rel[b] = sqrt(E_r[b]) / (sqrt(E_x[b]) + 1e-8),   E(z)[b] = sum_n c_n |z^_n|^2 / N,  c_n = 1 at n = 0, N/2, else 2.
 * The rule is second order: the residual of an exact pair falls as D^3 and is meaningful while |D N_tt| is small -- on
 * KS (N = 64, len 16, nu 0.05) rel(exact pair) is 3.5e-4 .. 9.7e-4 at D = 0.05 and 4.8e-3 .. 1.2e-2 at D = 0.1 against
 * 0.15 .. 0.24 and 0.36 .. 0.56 for p = x, and by D ~ 0.4 it is ~ 1 for both (DESIGN.md has the table).
 * affine: four host floats (a_p, b_p, a_x, b_x), NULL = (1, 0, 1, 0).  The residual is formed on a_p p + b_p and
 * a_x x + b_x (a model trained on encoded fields, penalised in physical units) and grad_p is with respect to the raw p.
 * rel [B] or NULL; loss: device scalar = mean (size_average) or sum, NULL for reduction=False; stats: 2 B floats
 * (sqrt E_r, sqrt E_x per sample) and spec_r (the spec_elems query's count of floats: r^, B images) are kept for backward.
 * Forward: one pass decodes, squares, forms the four spectra of [x~ | p~ | x~^2 | p~^2] as float64 sums over the N
 * points and from them r^ (rounded once) and the energies: for a good model r^ is a small remainder of terms of the
 * size of the field, and an fp32 transform's error in x^ would be of that remainder's size
 * (float64, two deterministic stages without atomics: identical calls give identical bits, and a sample's value does not
 * depend on the batch around it).  Backward: one inverse transform of the 2 B spectra [r^ | conj(m1) r^], then
 *   grad_p[b] = a_p coef_b (irfft(r^) - 2 p~ irfft(conj(m1) r^)),  coef_b = g_b / (sqrt(E_r) (sqrt(E_x) + 1e-8)), 0 where
 * E_r = 0; g_b = grad_rel[b], or grad_loss[0] (/ B when size_average) with grad_rel NULL.  No gradient for x: the
 * denominator is a constant of the sample.  N even, 4 .. 4096, 1 <= B <= 16383 (four fields of B images as one batch
 * of the half-spectrum layer): the two queries return 0 otherwise.  Tables and spec_r 16-byte aligned, the workspace (the ws query
 * serves both calls) 256-byte aligned.  On the caller's stream, no host synchronisation (the first use of a grid builds
 * its plan: it allocates and synchronises once).  Argument errors are reported before any device work. */
size_t rpde_etd_residual_ws_bytes(int B, int N);
size_t rpde_etd_residual_spec_elems(int B, int N);
int rpde_etd_residual_fwd(const float* p, const float* x, const float* E, const float* m0, const float* m1,
                          const float* affine, float* rel, float* loss, float* stats, float* spec_r, int B, int N,
                          int size_average, void* ws, size_t ws_bytes, void* stream);
int rpde_etd_residual_bwd(const float* p, const float* spec_r, const float* m1, const float* affine, const float* stats,
                          const float* grad_loss, const float* grad_rel, float* grad_p, int B, int N, int size_average,
                          void* ws, size_t ws_bytes, void* stream);

/* ---- equation-residual loss of the 2-D vorticity equation (csrc/ns_residual.hip; utils/loss.py VorticityResidualLoss;
 * no counterpart in the reference): does the one-step map x = w(t) -> p ~ w(t + D) satisfy the equation of the
 * Navier-Stokes generator above, w_t = -visc lap w - A(w) + f?  Grid, W = rfft2(w), k1, k2, lap, dealias and psi as in
 * the generator block, and A(w) = dealias rfft2(q w_x + v w_y) its discrete advection.  The exponential trapezoidal
 * rule of the 1-D block above with z = -D visc lap (all real):
 *   r^ = d^ - (E - 1) x^ - (m0 + m1) f^ + m0 A(x~) + m1 A(p~),   d = p~ - x~ formed in physical space,
 *   E = e^z,  m0 = D (phi1 - phi2),  m1 = D phi2  (phi1, phi2 on the 64-point contour),
 *   rel[b] = sqrt(E_r[b]) / (sqrt(E_x[b]) + 1e-8),  E(z)[b] = sum c |z^|^2 / (M N),  c = 1 on the columns kx = 0, N/2, else 2.
 * The caller forms the tables in float64 and rounds them once (rpde.ops.ns2d_residual_tables): em1 = E - 1 (expm1),
 * m0 = m0 dealias, m1 = m1 dealias, inv_lap = 1 / lap (lap[0,0] -> 1), each [M][kp] floats with the padded columns zero;
 * forcing_spec: the spectrum (m0 + m1) rfft2(f) of one forcing field for the batch, [M][re|im][kp], not de-aliased (the
 * generator does not), or NULL.  affine, rel, loss, stats and the upstream gradients as in the 1-D block; spec (the
 * spec_elems query's count of floats: [r^ | P^], 2 B images) is kept for backward.
 * Forward: x^ and d^ (d formed per point in float64, never rounded) as separable float64 analyses (rows, then columns)
 * that stay in float64 for the residual -- r^ is a remainder of 1e-3 |x| and an fp32 transform's absolute error in x^
 * would enter through (E - 1) x^ --; P^ = X^ + D^ rounded once, the generator's fan-out of [X^ | P^] to eight derivative
 * spectra, one inverse transform of 8 B images, the two advection products, one forward transform of 2 B, the residual
 * kernel (float64 partial sums per (sample, slot), slots a function of the grid alone) and the family's final kernel.
 * Backward, the exact adjoint of the discrete operator: g = irfft2(m1 r^) and the four fields of p~ rebuilt from P^ in
 * one inverse transform of 5 B images, the four products, one forward transform of 4 B,
 *   G^ = r^ + conj(2 pi i k2 / lap) rfft2(g w_x) + conj(-2 pi i k1 / lap) rfft2(g w_y) + conj(2 pi i k1) rfft2(g q)
 *           + conj(2 pi i k2) rfft2(g v),     grad_p = a_p coef_b irfft2(G^).
 * rpde_ns2d_residual_spectrum is the float64 analysis alone: spec64 and spec32 [B][M][re|im][kp] (doubles, floats) of
 * a x + b, affine = two host floats (a, b) or NULL.
 * Even M, N in 4 .. 4096 and 8 B images within the half-spectrum layer's limits (8 B <= 65535, 32 B max(M, N) < 2^31):
 * the two queries return 0 otherwise.  Fields, tables and spectra 16-byte aligned, the workspace (the ws query
 * serves the three calls: one layout per entry, the largest of them, the forward's) 256-byte aligned.  No atomics, no host synchronisation, everything on the caller's stream (the first use
 * of a grid builds its plans: it allocates and synchronises once).  Argument errors are reported before any device work. */
size_t rpde_ns2d_residual_ws_bytes(int B, int M, int N);
size_t rpde_ns2d_residual_spec_elems(int B, int M, int N);
int rpde_ns2d_residual_spectrum(const float* x, const float* affine, double* spec64, float* spec32, int B, int M, int N,
                                void* ws, size_t ws_bytes, void* stream);
int rpde_ns2d_residual_fwd(const float* p, const float* x, const float* em1, const float* m0, const float* m1,
                           const float* inv_lap, const float* forcing_spec, const float* affine, float* rel, float* loss,
                           float* stats, float* spec, int B, int M, int N, int size_average, void* ws, size_t ws_bytes,
                           void* stream);
int rpde_ns2d_residual_bwd(const float* spec, const float* m1, const float* inv_lap, const float* affine, const float* stats,
                           const float* grad_loss, const float* grad_rel, float* grad_p, int B, int M, int N,
                           int size_average, void* ws, size_t ws_bytes, void* stream);

/* ---- equation-residual loss of the active-scalar system (csrc/nsc_residual.hip; utils/loss.py
 * ActiveScalarResidualLoss; no counterpart in the reference): does the one-step map x = (c, q, v)(t) -> p ~ (c, q, v)(t + D),
 * both [B, 3, M, N], satisfy the equations of the active-scalar generator above (rpde_nsc2d_steps)?  The data are
 * concentration and velocity; the equations evolve (w, c) with w = curl u.  Conventions of the vorticity block above;
 * with the channel spectra x^ and d^ (d = p~ - x~ formed in physical space, ONE affine map for the three channels):
 *   X_c = x^_c,  X_w = 2 pi i k1 x^_v - 2 pi i k2 x^_q   (likewise D_c, D_w;  P = X + D),
 *   N_w(W, C) = dealias (rfft2(q w_1 + v w_2) - beta 2 pi i k1 C),  N_c(W, C) = dealias rfft2(q c_1 + v c_2): the
 *               generator's F_w and F_c; q, v from psi = W / lap, so only the solenoidal part of a velocity advects,
 *   r^_w = D_w - em1_nu X_w + m0_nu N_w(X) + m1_nu N_w(P) - forcing_spec,       z = -D visc lap,
 *   r^_c = D_c - em1_kappa X_c + m0_kappa N_c(X) + m1_kappa N_c(P),             z = -D kappa lap,
 *   delta^ = 2 pi i k1 P_q + 2 pi i k2 P_v  (the divergence of the predicted velocity),
 *   mu = (d^_q[0,0], d^_v[0,0])             (the change of the mean velocity, which the equations conserve),
 *   E_ru = sum_{k != 0} c (|r^_w|^2 + |delta^|^2) / lap / (M N) + |mu|^2 / (M N),   E_rc = sum c |r^_c|^2 / (M N),
 *   rel[b] = sqrt(scalar_weight E_rc + E_ru) / (sqrt(scalar_weight E(x^_c) + E(x^_q) + E(x^_v)) + 1e-8):
 * the vorticity's residual measured as the velocity it induces (energy |r^|^2 / lap), in the norm of the data's channels.
 * The buoyancy is not stiff and sits in N_w, as in the generator.  The tables are those of the vorticity block, once
 * per diffusivity (rpde.ops.nsc2d_residual_tables), m0 and m1 with the mask; forcing_spec as there, at the viscosity.
 * affine, rel, loss, stats and the upstream gradients as in the 1-D block; spec (the spec_elems query's count of
 * floats, 5 B images: [r^_w / lap | scalar_weight r^_c | delta^ / lap, its mean mode holding mu | P_w | P_c]) is kept
 * for backward.
 * Forward: the float64 analysis of the vorticity block over the 3 B images of x~ and over the 3 B images of d; X_w,
 * X_c, P_w, P_c from the float64 channel spectra, rounded once; the generator's fan-out (scalar part on) of the 2 B
 * states [X | P] to twelve derivative spectra per sample, one inverse transform of 12 B images, the four products, one
 * forward transform of 4 B, the residual kernel (everything in float64 from the float64 channel spectra, the buoyancy
 * terms included; partial sums per (sample, slot)) and the family's final kernel.
 * Backward, the exact adjoint of the discrete operator.  With rho_w = r^_w / lap (0 at the mean mode), rho_c =
 * scalar_weight r^_c, rho_d = delta^ / lap, g_w = irfft2(m1_nu rho_w), g_c = irfft2(m1_kappa rho_c) and the six fields of p~
 * rebuilt from (P_w, P_c) in one inverse transform of 8 B images, the six products, one forward transform of 6 B,
 *   G_w = rho_w + conj(2 pi i k2 / lap) rfft2(g_w w_1 + g_c c_1) + conj(-2 pi i k1 / lap) rfft2(g_w w_2 + g_c c_2)
 *               + conj(2 pi i k1) rfft2(g_w q) + conj(2 pi i k2) rfft2(g_w v),
 *   G_c = rho_c + conj(2 pi i k1) rfft2(g_c q) + conj(2 pi i k2) rfft2(g_c v) + conj(-beta 2 pi i k1) m1_nu rho_w,
 *   grad p_c = irfft2(G_c),  grad p_q = irfft2(conj(-2 pi i k2) G_w + conj(2 pi i k1) rho_d + [k = 0] mu_q),
 *   grad p_v = irfft2(conj(2 pi i k1) G_w + conj(2 pi i k2) rho_d + [k = 0] mu_v),   all times a_p coef_b
 * (one inverse transform of 3 B images).
 * rpde_nsc2d_residual_state is the forward up to the fan-out's state alone: state [4][B][M][re|im][kp] floats =
 * (X_w, P_w, X_c, P_c).
 * Even M, N in 4 .. 4096 and 12 B images within the half-spectrum layer's limits (12 B <= 65535, 48 B max(M, N) <
 * 2^31): the two queries return 0 otherwise.  Fields, tables and spectra 16-byte aligned, the workspace 256-byte
 * aligned.  The size query serves the three calls (one layout per entry, the query returns the largest); it is called
 * *_arena_bytes and not *_ws_bytes because the set of *_ws_bytes names is closed: tests/test_workspace_layout_cpu.py
 * pins it, and this query has the same query-against-entry check in tests/test_nsc_residual_cpu.py.  No atomics, no
 * host synchronisation, everything on the caller's stream (the first use of a grid builds its plans: it allocates and
 * synchronises once).  Argument errors are reported before any device work; the finiteness of the affine map is the
 * last of them, behind the verdict on the workspace. */
size_t rpde_nsc2d_residual_arena_bytes(int B, int M, int N);
size_t rpde_nsc2d_residual_spec_elems(int B, int M, int N);
int rpde_nsc2d_residual_state(const float* p, const float* x, const float* affine, float* state, int B, int M, int N,
                              void* ws, size_t ws_bytes, void* stream);
int rpde_nsc2d_residual_fwd(const float* p, const float* x, const float* em1_nu, const float* m0_nu, const float* em1_kappa,
                            const float* m0_kappa, const float* forcing_spec, float scalar_weight, const float* m1_nu,
                            const float* m1_kappa, const float* inv_lap, float beta, const float* affine, float* rel,
                            float* loss, float* stats, float* spec, int B, int M, int N, int size_average, void* ws,
                            size_t ws_bytes, void* stream);
int rpde_nsc2d_residual_bwd(const float* spec, const float* m1_nu, const float* m1_kappa, const float* inv_lap, float beta,
                            const float* affine, const float* stats, const float* grad_loss, const float* grad_rel,
                            float* grad_p, int B, int M, int N, int size_average, void* ws, size_t ws_bytes, void* stream);

/* ---- Darcy flow generator (csrc/darcy.hip; reference: dataloaders/darcy_loader.py and the piececonst_* files of
 * load_darcy_data_from_mat): -div(a grad u) = f on the unit square, u = 0 on the boundary, s x s cells with centres
 * x_i = (i + 1/2) / s, a and u [B, s, s] at the centres.  Finite volumes: an interior face between cells c and n weighs
 * w = 2 a_c a_n / (a_c + a_n), a boundary face of cell c weighs 2 a_c (the wall is half a cell away, u = 0 there), and
 *   (A u)_c = s^2 sum_faces w_face (u_c - u_n),  u_n = 0 across a boundary face,
 * evaluated in this difference form.  The apply call is Au = A u.
 * The solve call runs `iterations` iterations of conjugate gradients from u = 0, preconditioned with the same operator at
 * a = 1 inverted exactly, P^-1 r = S^T (inv_lambda . (S r S^T)) S.  The caller forms both tables [s, s] in float64 and rounds
 * them to fp32 once (rpde.ops.darcy2d_tables):
 *   S[k, i] = sqrt(2 / s) sin(pi (k + 1) (i + 1/2) / s), row k = s - 1 divided by sqrt 2      (DST-II, orthogonal)
 *   inv_lambda[k1, k2] = 1 / (l_k1 + l_k2),  l_k = s^2 (2 - 2 cos(pi (k + 1) / s)).
 * f is one right-hand side [s, s] (f_batched = 0) or B of them.  Nine launches per iteration on the caller's stream, no
 * host synchronisation and no device-to-host read; every scalar (alpha, beta, r.z, the norms, the per-sample state) stays
 * in device memory; no atomics: identical calls give identical bits, and a sample never reads another sample's scalars.
 * A sample freezes -- its alpha and beta are 0 and its u fixed for the rest of the loop -- once its recurrence residual
 * satisfies |r| <= tol |f|, or its p.Ap or r.z is not a positive finite number.  After the loop one more apply gives
 * rel_residual[b] = |f - A u| / |f| (0 for f = 0), the true residual, and frozen_at[b] is the number of iterations the
 * sample took before it froze; `iterations` means it never did.  The iterate is advanced as a two-float sum (its low part
 * lives in the workspace) and u is that sum rounded once: the true residual is the one of the correctly rounded
 * solution, which in fp32 grows like s^2 (7e-6 at s = 32, 1e-4 at 128 for a of order 10, f = 1).
 * The sep2d call: out_b = L in_b R^T for B images [s, s] and two tables [s, s] -- the product form of a separable
 * transform (one batched GEMM with the shared table on the left, one GEMM over [B s, s] on the right); the solver's
 * sine transforms and the cosine-series random field (data_generation/random_fields.py GaussianRFNeumann) go through it.
 * Grids 8 <= s <= 512, s a multiple of 4, 1 <= B <= 65535: the ws query returns 0 otherwise and the calls refuse.
 * Fields and tables 16-byte aligned, workspaces 256-byte aligned (sep2d: B s s floats rounded up to 256 bytes).
 * a must be positive and finite: the caller's contract, not checked here.  Argument errors are reported before any
 * device work. */
size_t rpde_darcy2d_ws_bytes(int B, int s);
int rpde_darcy2d_apply(const float* a, const float* u, float* Au, int B, int s, void* stream);
int rpde_darcy2d_solve(const float* a, const float* f, int f_batched, const float* S, const float* inv_lambda,
                       float* u, float* rel_residual /*[B]*/, int* frozen_at /*[B]*/,
                       int B, int s, int iterations, float tol, void* ws, size_t ws_bytes, void* stream);
int rpde_sep2d(const float* in, const float* L, const float* R, float* out, int B, int s, void* ws, size_t ws_bytes,
               void* stream);

/* ---- equation-residual loss of the Darcy generator (csrc/darcy_residual.hip; utils/loss.py DarcyResidualLoss; no
 * counterpart in the reference): does the map a -> p ~ u satisfy the discrete equation of the generator above?  The
 * equation is steady and the network's input is the coefficient.  With a~ = a_x a + b_x and u~ = a_p p + b_p (affine =
 * four host floats (a_p, b_p, a_x, b_x) or NULL, as in the residual blocks above) and one right-hand side f [s][s],
 *   r_b = f - A(a~_b) u~_b,   A the operator of the apply call, bit for bit,
 *   S, inv_lambda given (the dual norm of the preconditioner P = A(1)):  E_b = sum_k inv_lambda_k (S r_b S^T)_k^2 = r_b . P^-1 r_b,
 *   S = inv_lambda = NULL (L2):                                          E_b = |r_b|^2,
 *   rel[b] = sqrt(E_b) / (D + 1e-8),  D the same norm of f, formed by the caller in float64 (rpde.ops.darcy2d_residual_tables),
 * then mean / sum / the per-sample vector; rel, loss, stats [2 B] = (sqrt(E_b), D) and the upstream gradients as in
 * the residual blocks above.  Every face weight lies in [a_min, a_max], hence a_min P <= A(a) <= a_max P and the dual
 * norm is the energy-norm error of p to within sqrt of the contrast at every grid size; the L2 form grows like s^2
 * (DESIGN.md 10.14).  spec (the spec_elems query's count of floats, B s s) is kept for backward: inv_lambda . (S r S^T),
 * or r for L2.  Forward: one apply kernel (decode on load), then for the dual norm one sep2d and one streaming kernel,
 * then the family's final kernel -- five launches, two for L2.  Backward, A being self-adjoint:
 *   z_b = S^T spec_b S (L2: z = spec),   grad_p = -a_p coef_b A(a~_b) z_b,   coef_b = upstream_b / ((D + 1e-8) sqrt(E_b)),
 * 0 where E_b = 0: one sep2d and one apply kernel -- three launches, one for L2.  It reads the coefficient a again.
 * Limits, alignment and the workspace are the generator's: rpde_darcy2d_ws_bytes(B, s) serves both calls (each carves
 * a layout of its own that fits the solve's), the spec query returns 0 for a grid the generator refuses.  No atomics,
 * no host synchronisation, no device-to-host read: identical calls give identical bits and a batch equals its B = 1
 * calls.  A decoded coefficient that is not positive makes the loss non-finite: the caller's contract, not checked.
 * Argument errors are reported before any device work. */
size_t rpde_darcy2d_residual_spec_elems(int B, int s);
int rpde_darcy2d_residual_fwd(const float* p, const float* a, const float* f, const float* S, const float* inv_lambda,
                              double D, const float* affine, float* rel, float* loss, float* stats, float* spec, int B,
                              int s, int size_average, void* ws, size_t ws_bytes, void* stream);
int rpde_darcy2d_residual_bwd(const float* a, const float* spec, const float* S, const float* affine, const float* stats,
                              const float* grad_loss, const float* grad_rel, float* grad_p, int B, int s, int size_average,
                              void* ws, size_t ws_bytes, void* stream);

/* ---- optimizer step: torch.optim.AdamW as built at main_1d.py:144 / main_2d.py:173 (decoupled weight decay,
 * bias-corrected moments, no amsgrad), one streaming kernel over flat fp32 buffers of n (multiple of 4) elements.
 * The caller passes the step's scalars: 1 - lr*wd, 1 - b1, b2, 1 - b2, lr / (1 - b1^t), sqrt(1 - b2^t), eps. */
int rpde_adamw_step(float* p, const float* g, float* m, float* v, int64_t n,
                    float one_minus_lr_wd, float one_minus_b1, float b2, float one_minus_b2,
                    float step_size, float bc2_sqrt, float eps, void* stream);
/* the same with the step state on the device (step_dev: 8 floats -- [0] t, incremented by the call, [1] lr/(1-b1^t),
 * [2] sqrt(1-b2^t), [3] lr, [4] weight decay, [5] 1 - lr*wd): nothing step-dependent crosses the host, so the step can be
 * captured in a hipGraph.  Called eagerly it stores its lr / weight_decay arguments in step_dev first; while its stream
 * is being captured it does not, and every replay runs with what rpde_adamw_set_hyper_dev put there -- a captured step
 * follows a learning-rate schedule (main_1d.py:145-151, main_2d.py:174-180) without being captured again. */
int rpde_adamw_step_dev(float* p, const float* g, float* m, float* v, int64_t n,
                        float lr, float b1, float b2, float eps, float weight_decay,
                        float* step_dev, void* stream);
int rpde_adamw_set_hyper_dev(float* step_dev, float lr, float weight_decay, void* stream);
/* the update of rpde_adamw_step_dev without advancing the counter (a second buffer of the same optimizer step) */
int rpde_adamw_apply_dev(float* p, const float* g, float* m, float* v, int64_t n,
                         float lr, float b1, float b2, float eps, float weight_decay,
                         const float* step_dev, void* stream);

/* ---- gradient-norm clipping and non-finite step skipping, on the device (csrc/adamw_clip.hip).
 * rpde_grad_norm: norm = sqrt(sum g^2) over n (multiple of 4) floats, squares and sums in float64, two deterministic
 * stages without atomics (one double per workgroup in ws, added in fixed order), rounded to fp32 once; then
 * torch.nn.utils.clip_grad_norm_'s rule  scale = min(1, max_norm / (norm + 1e-6))  with NaN propagating as in
 * torch.clamp and an infinite norm giving 0.  max_norm <= 0 or +inf: measure only, scale 1.  The result is the device
 * record clip_dev, 8 floats:
 *   [0] this step's norm   [1] the scale applied   [2] 1.0 when this step is skipped (skip_nonfinite != 0 and the norm
 *   is NaN or inf), else 0.0   [3] steps seen   [4] steps clipped (scale < 1, not skipped)   [5] steps skipped
 *   [6] largest finite norm seen   [7] sum of the finite norms.
 * [3..7] accumulate over calls until the caller zeroes them; the counters are fp32 and exact up to 2^24 steps.
 * ws: rpde_grad_norm_ws_bytes(n) bytes, 8-byte aligned (0 for an n the call would refuse). */
size_t rpde_grad_norm_ws_bytes(int64_t n);
int rpde_grad_norm(const float* g, int64_t n, float max_norm, int skip_nonfinite, float* clip_dev,
                   void* ws, size_t ws_bytes, void* stream);
/* rpde_adamw_step / _step_dev / _apply_dev behind such a record: the update uses clip_dev[1] * g (g itself is not
 * rewritten), and when clip_dev[2] is set the call changes nothing -- parameters, moments, and for _step_dev the step
 * counter and the words derived from it, stay bit for bit.  With scale 1 the results equal the plain calls' bit for bit. */
int rpde_adamw_step_clip(float* p, const float* g, float* m, float* v, int64_t n,
                         float one_minus_lr_wd, float one_minus_b1, float b2, float one_minus_b2,
                         float step_size, float bc2_sqrt, float eps, const float* clip_dev, void* stream);
int rpde_adamw_step_dev_clip(float* p, const float* g, float* m, float* v, int64_t n,
                             float lr, float b1, float b2, float eps, float weight_decay,
                             float* step_dev, const float* clip_dev, void* stream);
int rpde_adamw_apply_dev_clip(float* p, const float* g, float* m, float* v, int64_t n,
                              float lr, float b1, float b2, float eps, float weight_decay,
                              const float* step_dev, const float* clip_dev, void* stream);

/* ---- CNO: the alias-free activation (csrc/cno.hip; reference models/CNO1d.py:30-45 `CNO_LReLu`, built at
 * main_1d.py:100-104 from conf/model/cno_1d/cno_1d.yaml).  The reference resamples x [B, C, n_in] (channels first) to
 * n_mid = 2 in_size points with F.interpolate(mode="bicubic", antialias=True), applies LeakyReLU and resamples to n_out
 * points: three ATen ops and two round trips of the n_mid-long tensor.  Both resamplings are fixed banded linear maps,
 * so each call below is one kernel whose mid signal lives in LDS only:
 *   fwd:  y = scale[c] * x + shift[c] (scale, shift [C] or both null: y = x; a BatchNorm's apply step),
 *         u = U y,  v = u > 0 ? u : slope * u,  out = D v                                        out [B, C, n_out]
 *   bwd:  gy = U^T ((u > 0 ? 1 : slope) * D^T g)   with u recomputed from x; the gradient with respect to y (the caller
 *         owns the chain rule of its affine); at u == 0 the derivative is slope, torch's convention.   gy [B, C, n_in]
 * n_in, n_mid and n_out are independent.  A band is given as  span [rows][2] int32 (first source, tap count; 8-byte
 * aligned) and weights [rows][taps] fp32 (taps a multiple of 4, zero padded, 16-byte aligned): row i is
 * sum_t weights[i][t] * src[span[i][0] + t].  U: n_mid rows over n_in sources; D: n_out rows over n_mid; U^T: n_in rows
 * over n_mid (for each input, the contiguous run of mid points that read it); D^T: n_mid rows over n_out.  The tables
 * must be those of rpde.ops.cno_tables (torch's antialiased bicubic rule): the workgroup tiling is sized from that
 * filter's support.  Rows that fit a workgroup are packed several to one, longer rows are tiled along x (1024 written
 * points per tile, halved while the mid span of a tile exceeds its LDS); a size ratio at which 32 written points no
 * longer fit is refused with RPDE_ERR_ARG.  No workspace, no atomics: the same inputs give the same bits. */
int rpde_cno_act1d_fwd(const float* x, const float* scale, const float* shift, float* out, int B, int C, int n_in,
                       int n_mid, int n_out, float slope, const int32_t* u_span, const float* u_w, int u_taps,
                       const int32_t* d_span, const float* d_w, int d_taps, void* stream);
int rpde_cno_act1d_bwd(const float* x, const float* scale, const float* shift, const float* g, float* gy, int B, int C,
                       int n_in, int n_mid, int n_out, float slope, const int32_t* u_span, const float* u_w, int u_taps,
                       const int32_t* ut_span, const float* ut_w, int ut_taps, const int32_t* dt_span, const float* dt_w,
                       int dt_taps, void* stream);

/* ---- CNO: the rest of a block (csrc/cno_layers.hip, both ranks; reference models/CNO1d.py:51-164: Conv1d(k=3,
 * padding=1) -> BatchNorm1d -> CNO_LReLu, and the residual block's second BatchNorm plus skip add).  Channels first,
 * contiguous [B, C, n] or [B, C, H, W].
 * conv_k3: Conv(k = 3, padding = 1) of both ranks on [B, C, H, W] with ky rows of three taps: ky = 3 is Conv2d, ky = 1
 *   Conv1d, a plane of one row (H = 1 required) with the dy = 0 row of taps alone; ky = 3 with H = 1 is legal.  The
 *   taps are accumulating rpde_gemm_f32 products on shifted views -- the centre tap over the flat H W axis with the
 *   bias, the two dx = 0 taps flat over (H - 1) W points, the dx != 0 taps row by row through the descriptor's
 *   two-level batch so that no row wraps; taps without a valid range (H = 1 or W = 1) are skipped, so Conv1d runs
 *   three products: centre, tap 0 onto [1, n), tap 2 onto [0, n - 1).  wt is the weight repacked tap-major,
 *   [3 ky][Cout][Cin], tap = 3 ty + tx.  _bwd_data: gx from g with the transposed taps and mirrored shifts.
 *   _bwd_weight: gw [Cout][Cin][ky][3] (torch's layout) and gb [Cout] (or null), fp32, fixed order, no atomics, on the
 *   sliced kernel it shares with upconv below: for ky = 3 the image rows (b, y) are split into slices over enough
 *   workgroups to fill the device when Cout Cin is small, the slices' partial sums go to the caller's `partial`
 *   [slices][3 ky Cout Cin + Cout] floats (rpde_conv_k3_bwd_weight_slices gives the count; with one slice the buffer
 *   is not used and may be null) and a second kernel adds them in slice order; ky = 1 always runs one slice.
 * moments: sums [C][4] doubles = (sum a, sum b, sum a b, sum b^2) per channel over (batch, x).  BatchNorm's forward
 *   reads mean and variance of z from (z, z); its backward reads sum gy and sum gy z from (gy, z).
 * affine: out = p0[c] a + p1[c] b + p2[c] (+ residual); b and p1 both null: no b term.  A BatchNorm's apply step (with the
 *   residual block's skip add), its backward dz = p0 gy + p1 z + p2, and a plain skip add (p0 = 1, p2 = 0).  The
 *   coefficients [C] are doubles and the sum is formed in double and rounded once: the backward's terms cancel to
 *   eps / (var + eps) of their size when a channel has few values. */
int rpde_conv_k3_fwd(const float* x, const float* wt, const float* bias, float* out, int B, int Cin, int Cout, int H, int W,
                     int ky, void* stream);
int rpde_conv_k3_bwd_data(const float* g, const float* wt, float* gx, int B, int Cin, int Cout, int H, int W, int ky,
                          void* stream);
int rpde_conv_k3_bwd_weight_slices(int B, int Cin, int Cout, int H, int W, int ky);
int rpde_conv_k3_bwd_weight(const float* x, const float* g, float* gw, float* gb, int B, int Cin, int Cout, int H, int W,
                            int ky, float* partial, int partial_slices, void* stream);
int rpde_cno_moments(const float* a, const float* b, double* sums, int B, int C, int n, void* stream);
int rpde_cno_affine(const float* a, const float* b, const double* p0, const double* p1, const double* p2, const float* residual,
                    float* out, int B, int C, int n, void* stream);

/* ---- CNO in 2-D (csrc/cno2d.hip; reference models/CNO2d.py, built at main_2d.py:119-124 from
 * conf/model/cno_2d/cno_2d.yaml).  CNO_LReLu resamples a plane x [B, C, h_in, w_in] (channels first, contiguous fp32) to
 * h_mid x w_mid with F.interpolate(mode="bicubic", antialias=True), applies LeakyReLU and resamples to h_out x w_out.
 * The 2-D resampling is the tensor product of the 1-D banded maps above, one table per axis and direction:
 *   fwd:  y = scale[c] * x + shift[c] (or y = x),  u = U_y y U_x^T,  out = D_y lrelu(u) D_x^T       out [B, C, h_out, w_out]
 *   bwd:  gy = U_y^T ((u > 0 ? 1 : slope) * (D_y^T g D_x)) U_x  with u recomputed from x; the gradient with respect to y;
 *         at u == 0 the derivative is slope.                                                        gy [B, C, h_in, w_in]
 * Bands as in 1-D (span [rows][2] int32, weights [rows][taps] fp32, taps a multiple of 4), those of
 * rpde.ops.cno_tables(device, n_in, n_out): U_y h_in -> h_mid, U_x w_in -> w_mid, D_y h_mid -> h_out, D_x w_mid -> w_out,
 * and for the backward their transposed forms (`bwd` of the same tables).  Planes may be rectangular and the ratios
 * non-integer.  A workgroup owns a tile of the written plane (the output in fwd, the input in bwd), 32 x 32 points or
 * the largest power-of-two rectangle below it whose spans fit its LDS; planes that fit whole are packed several to a
 * workgroup; a ratio at which one row of 4 written points does not fit is refused with RPDE_ERR_ARG.  The mid plane
 * lives in LDS only.  No workspace, no atomics: the same inputs give the same bits.
 * rpde_cno_act2d_plan reports the tile (th, tw) and the planes per workgroup the kernels use for a shape (backward: 0
 * or 1); it launches nothing. */
int rpde_cno_act2d_plan(int backward, int B, int C, int h_in, int w_in, int h_mid, int w_mid, int h_out, int w_out, int* th,
                        int* tw, int* pack);
int rpde_cno_act2d_fwd(const float* x, const float* scale, const float* shift, float* out, int B, int C, int h_in, int w_in,
                       int h_mid, int w_mid, int h_out, int w_out, float slope, const int32_t* uy_span, const float* uy_w,
                       int uy_taps, const int32_t* ux_span, const float* ux_w, int ux_taps, const int32_t* dy_span,
                       const float* dy_w, int dy_taps, const int32_t* dx_span, const float* dx_w, int dx_taps, void* stream);
int rpde_cno_act2d_bwd(const float* x, const float* scale, const float* shift, const float* g, float* gy, int B, int C,
                       int h_in, int w_in, int h_mid, int w_mid, int h_out, int w_out, float slope, const int32_t* uy_span,
                       const float* uy_w, int uy_taps, const int32_t* ux_span, const float* ux_w, int ux_taps,
                       const int32_t* uyt_span, const float* uyt_w, int uyt_taps, const int32_t* uxt_span, const float* uxt_w,
                       int uxt_taps, const int32_t* dyt_span, const float* dyt_w, int dyt_taps, const int32_t* dxt_span,
                       const float* dxt_w, int dxt_taps, void* stream);

/* ---- U-Net (csrc/unet.hip; reference models/unet.py, the PDEBench U-Net): what its blocks need beyond conv k3, the
 * BatchNorm kernels and conv1x1 above.  Channels first, contiguous fp32; ky = 1 is the 1-D form, a plane of one row
 * (H = 1) with windows / taps of one row, ky = 2 the 2-D form.  No atomics, fixed summation order.
 * tanh_pool_fwd: act = tanh(scale[c] z + shift[c]) on [B, C, H, W] (scale, shift [C], or both null) and, when `pooled`
 *   is given, the maximum over the non-overlapping ky x 2 windows into pooled [B, C, H / ky, W / 2] in the same pass
 *   (floor division: an odd last row or column belongs to no window; a pooled size of 0 is refused).  A NaN in a window
 *   wins, as in torch's pooling.
 * tanh_pool_bwd: gy = (g_act + scatter(g_pool)) (1 - act^2), the gradient with respect to scale z + shift; g_act or
 *   g_pool may be null, not both.  scatter sends a window's gradient to the first maximum of act in the window's
 *   row-major scan order, recomputed from act.
 * upconv_*: ConvTranspose(kernel_size = 2, stride = 2) with torch's weight layout w [Cin][Cout][ky][2] and bias [Cout]
 *   (or null): out [B, Cout, ky H, 2 W] from x [B, Cin, H, W]; _bwd_data gx from g; _bwd_weight gw (w's layout) and
 *   gb [Cout] (or null) on conv_k3's sliced kernel with the operands' roles exchanged, the points (b, y, x) split into
 *   slices whose partial sums go to `partial` [slices][ky 2 Cin Cout + Cout] floats
 *   (rpde_unet_upconv_bwd_weight_slices gives the count; with one slice the buffer is not used and may be null) and
 *   are added in slice order. */
int rpde_unet_tanh_pool_fwd(const float* z, const float* scale, const float* shift, float* act, float* pooled, int B, int C,
                            int H, int W, int ky, void* stream);
int rpde_unet_tanh_pool_bwd(const float* act, const float* g_act, const float* g_pool, float* gy, int B, int C, int H, int W,
                            int ky, void* stream);
int rpde_unet_upconv_fwd(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int H, int W,
                         int ky, void* stream);
int rpde_unet_upconv_bwd_data(const float* g, const float* w, float* gx, int B, int Cin, int Cout, int H, int W, int ky,
                              void* stream);
int rpde_unet_upconv_bwd_weight_slices(int B, int Cin, int Cout, int H, int W);
int rpde_unet_upconv_bwd_weight(const float* x, const float* g, float* gw, float* gb, int B, int Cin, int Cout, int H, int W,
                                int ky, float* partial, int partial_slices, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RPDE_H */
