/* smx.h — C-ABI of libsmx.so: the MI355X (gfx950) SummaryMixing encoder hot path.
 *
 * The reference (SamsungLabs/SummaryMixing @ 2024_10_08) is pure Python on torch and has NO FFI and no
 * native kernel: every entry point below is NEW.  Each one names the reference lines whose arithmetic it
 * replaces (paths relative to the reference root) so that a maintainer can bind it from the reference's
 * nn.Modules (see INTEGRATION.md for the ctypes stub).
 *
 * Conventions
 *  - every function returns SMX_OK (0) or a negative SMX_E* code; never throws, never aborts;
 *    smx_last_error() returns a thread-local message for the last failing call on this thread.
 *  - all data pointers are DEVICE pointers owned by the caller; the library allocates nothing.
 *  - matrices are row-major with an explicit leading dimension (in ELEMENTS) so column slices of a
 *    wider buffer are addressed without copies.
 *  - dtype is SMX_F32 or SMX_BF16 for activations/weights ("T"); biases, LayerNorm affine, conv taps,
 *    per-utterance side inputs, statistics and all gradients of parameters are always float32.
 *  - last argument is the hipStream_t to launch on (passed as void*); all work is stream ordered and
 *    asynchronous; no global mutable state; safe from several host threads on different streams.
 */
#ifndef SMX_H_
#define SMX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMX_VERSION 100

enum { SMX_OK = 0, SMX_EINVAL = -1, SMX_EUNSUPPORTED = -2, SMX_ELAUNCH = -3 };
enum { SMX_F32 = 0, SMX_BF16 = 1 };
enum { SMX_ACT_NONE = 0, SMX_ACT_GELU = 1, SMX_ACT_SWISH = 2, SMX_ACT_LEAKY_RELU = 3, SMX_ACT_RELU = 4 };
/* how the fp32 side input C0 is indexed by output row n: none | row n | row n / div | row n % div */
enum { SMX_C0_NONE = 0, SMX_C0_ROW = 1, SMX_C0_GROUP = 2, SMX_C0_MOD = 3 };
/* operand storage for smx_gemm: KC = reduce dimension contiguous, KS = reduce dimension strided */
enum { SMX_GEMM_NT = 0, /* A (N,K) KC, B (M,K) KC : Y = X W^T        (torch Linear forward)            */
       SMX_GEMM_NN = 1, /* A (N,K) KC, B (K,M) KS : dX = dZ W        (dgrad; ParallelLinear einsum)     */
       SMX_GEMM_TN = 2  /* A (K,N) KS, B (K,M) KS : dW = dZ^T X      (wgrad)                            */ };
enum { SMX_OUT_T = 0, SMX_OUT_F32 = 1, SMX_OUT_ATOMIC_F32 = 2 };
enum { SMX_PAD_ZERO = 0, SMX_PAD_REFLECT = 1 };

int smx_version(void);
const char* smx_last_error(void);

/* The library's tuning / diagnostic knobs.  They are read from the environment ONCE, when the library is first used, into
 * this struct (never again: no getenv on any call path); smx_get_config returns the values in force.  Every field defaults
 * to the measured-best setting; the SMX_* variable that overrides it is named in the comment.  Ablation switches
 * (SMX_GEMM_ABLATE, SMX_WGROUP_ABLATE, SMX_DWROLL_ABLATE) only exist in builds with -DSMX_DIAG and read 0 otherwise. */
typedef struct smx_config {
  int32_t ln_tile_rows;     /* rows of the LayerNorm-fused GEMM tile (128; see smx_gemm_ln_tile_rows)        */
  int32_t gemm_ablate, wgroup_ablate, dwroll_ablate;   /* SMX_DIAG builds only                                  */
  int32_t diag_build;       /* 1 when the library was compiled with -DSMX_DIAG                               */
  int32_t t256;             /* SMX_T256: 256 x 256 GEMM tile (one workgroup per CU, software-pipelined K loop)
                               0 off, 1 for K >= 2048 (1), 2 for every eligible shape (tests)                  */
  int32_t panel_rows;       /* SMX_PANEL_ROWS: rows per panel of smx_gemm_panel (128 / 64 / 32); 0 = by frame count  */
  int32_t pool_fuse_max_rows;  /* SMX_POOL_FUSE_MAX_ROWS (16 384): smx_pool_bcast_ok(B, T, D) = T <= 4096 and
                                  (B * T <= this many frames or B * ceil(D / 64) >= 256)                            */
  int32_t ln_tile64;        /* SMX_LN_TILE64: the 64 x 256 LayerNorm-fused tile: 0 never, 1 where it fills its rounds better (default), 2 always */
  int32_t lnb_lds;          /* SMX_LNB_LDS: the LayerNorm-backward epilogue of the 128 x 256 tile lands its side rows (ln_x, res, z) in
                               LDS by LDS-DMA, each half-phase's request in flight under the previous one: 1 on (default), 0 the
                               register path (bit-identical results) */
} smx_config;
int smx_get_config(smx_config* out);
/* rows per tile of the LayerNorm-fused GEMMs (SMX_EPI_LN_BWD writes ceil(N / rows) partial row pairs into ln_partial) */
int smx_gemm_ln_tile_rows(void);
/* ... for a given launch: 64 (d_model = 256 at mid-size batches, round 6) or 128 */
int smx_gemm_ln_tile_rows_for(int N, int M);

/* Epilogue of the fused projection GEMM:
 *   v      = acc + bias[m] + C0[map(n), m]
 *   Z[n,m] = v                                   (optional pre-activation store, dtype T)
 *   a      = dropout(act(v)) * row_mask[n]        (dropout: keep(seed, n*M+m) ? x/(1-p) : 0; off when drop_p == 0)
 *   C[n,m] = R[n,m] + alpha * a                  (R optional residual, dtype T)
 * With out_mode SMX_OUT_ATOMIC_F32: C (float32) += alpha * acc and every other epilogue field must be 0. */
typedef struct smx_epilogue {
  const float* bias;   int64_t bias_batch_stride;       /* [M] fp32 or NULL                           */
  const float* c0;     int64_t ldc0; int32_t c0_mode; int32_t c0_div;
  int32_t act;         int32_t out_mode;
  void* z;             int64_t ldz;
  const uint8_t* row_mask;                               /* [N] 1 = valid frame, or NULL               */
  const void* res;     int64_t ldr;
  float alpha;         int32_t flags;                     /* SMX_EPI_C0_POST: add C0 after dropout/mask/alpha      */
  float drop_p;        int32_t drop_cols;                 /* fused inverted dropout (0 = off), applied after act();
                                                           * drop_cols > 0: only the first drop_cols output columns,
                                                           * masks indexed n*drop_cols + m (0: all M, n*M + m)        */
  uint64_t drop_seed;                                     /* counter-based mask, same indexing as smx_dropout       */
  float* colsum;                                          /* [M] fp32 or NULL: colsum[m] += sum_n C[n,m] (fixed order) */
  void* workspace;                                        /* smx_gemm_colsum_workspace(N, M) bytes when colsum is set  */
  /* SMX_EPI_LN_BWD: the GEMM output is the gradient of a LayerNorm's OUTPUT (M = the LayerNorm width) */
  const void* ln_x;    int64_t ln_ldx;                    /* the LayerNorm input (N, M), dtype T                       */
  const float* ln_stats; const float* ln_gamma;           /* (N, 2) mean | rstd of the forward; [M]                    */
  float* ln_partial;                                      /* [ceil(N/smx_gemm_ln_tile_rows())][2][M] per-tile dgamma | dbeta partial rows */
  void* ln_dx2;        int64_t ln_lddx2;                  /* optional second output (see smx_layernorm_bwd: dX2) or NULL */
  const uint8_t* ln_mask2; float ln_alpha2; float ln_drop_p2; uint64_t ln_drop_seed2;
  /* SMX_EPI_LN_FWD: a LayerNorm of the (row-complete) output: lnf_y = act(LN(C)), lnf_stats = (mean, rstd) per row */
  const float* lnf_gamma; const float* lnf_beta; void* lnf_y; int64_t lnf_ldy; float* lnf_stats; float lnf_eps; int32_t lnf_act;
  /* fp32 residual stream (torch autocast semantics: Linear I/O in bf16, the residual adds and LayerNorm inputs in fp32 -
   * Conformer.py:507,530,532-536): SMX_IO_RES_F32 = `res` is float32 (needs out_mode SMX_OUT_F32: C is the new stream
   * tensor); SMX_IO_LNX_F32 = `ln_x` (SMX_EPI_LN_BWD) is float32.  lnf_y is dtype T (the next GEMM's input) unless
   * SMX_IO_LNFY_F32 (the LayerNorm output is itself the stream: the layer-final norm2, Conformer.py:536). */
  int32_t io_flags;    int32_t pad_;
  /* device step counter mixed into this call's fused dropout seed (see smx_step_counter_add), or NULL */
  const uint64_t* epoch;
  /* SMX_EPI_LN_FWD, optional SECOND LayerNorm of the first one's output (a Conformer layer's norm2 followed by the next layer's
   * first LayerNorm, Conformer.py:536 / :507): lnf2_y (dtype T) = LN2(lnf_y values before rounding), lnf2_stats = (mean, rstd).
   * Only where smx_gemm_ln_pair_ok says so (the 128 x 512 tile on the float32 stream); NULL lnf2_y = off. */
  const float* lnf2_gamma; const float* lnf2_beta; void* lnf2_y; int64_t lnf2_ldy; float* lnf2_stats; float lnf2_eps; int32_t pad2_;
} smx_epilogue;
enum { SMX_IO_RES_F32 = 1, SMX_IO_LNX_F32 = 2, SMX_IO_LNFY_F32 = 4 };
/* flags.  SMX_EPI_ACT_GRAD turns the epilogue into the BACKWARD of an upstream activation layer: z is then a
 * read-only INPUT (the pre-activation the forward saved) and
 *   C[n,m] = alpha * dropout(v * act'(z[n,m])) * row_mask[n]
 * so a dgrad GEMM dX = dZ W emits the upstream layer's dZ directly (act/dropout/mask backward fused; `res` must be
 * NULL); with `colsum` the upstream bias gradient comes out of the same launch.  batch == 1, splits == 1. */
/* SMX_EPI_LN_BWD fuses the LayerNorm BACKWARD into the dgrad GEMM that produces the gradient g of the LayerNorm's output
 * (torch.nn.LayerNorm of the Conformer modules, Conformer.py:146,152,458,475): with xhat = (ln_x - mean) * rstd,
 *   C[n,:] = rstd * (g*gamma - mean_m(g*gamma) - xhat * mean_m(g*gamma*xhat)) + res[n,:]     (res = residual gradient)
 * and per-tile partial rows dgamma = sum_n g * xhat, dbeta = sum_n g in ln_partial (fold with smx_reduce_jobs: two jobs,
 * src = ln_partial (+ M), src_stride 2*M, nsrc = ceil(N/128), rows 1, cols M).  Needs the whole LayerNorm row in one
 * tile: dtype bf16, M == 256, aligned operands, N >= 128 (smx_gemm_ln_fused_ok); no bias / dropout / C0.  With
 * lnf_act != 0 the LayerNorm had a fused activation (Y = act(LN(x)), lnf_beta required): g is first multiplied by
 * act'(LN(x)).  With z / act set (and ln_dx2) the second output is alpha2 * D(dX * act'(z)) * mask2 (the consumer's own
 * activation backward).
 * SMX_EPI_LN_FWD (same shape conditions) appends a LayerNorm FORWARD of the finished output rows: the ordinary epilogue
 * writes C (bias, residual, dropout, mask ... as usual), then lnf_y = act(LN(C) * gamma + beta) and lnf_stats. */
enum { SMX_EPI_C0_POST = 1, SMX_EPI_ACT_GRAD = 2, SMX_EPI_LN_BWD = 4, SMX_EPI_LN_FWD = 8 };
int smx_gemm_ln_fused_ok(int dtype, int N, int M, int K);
/* ... and can that epilogue run a SECOND LayerNorm on the first one's output (smx_epilogue.lnf2_*)?  Needs, besides the shape, the
 * float32 residual stream form of the call: SMX_OUT_F32, SMX_IO_RES_F32 residual, no C0 / column sums (else SMX_EUNSUPPORTED). */
int smx_gemm_ln_pair_ok(int dtype, int N, int M, int K);
size_t smx_gemm_colsum_workspace(int N, int M);

/* Batched strided MFMA GEMM  C[b] (N x M) = epilogue( op(A[b]) . op(B[b]) ), reduce length K.
 * Replaces: nn.Linear inside VanillaNN (VanillaNN.py:189-196, summary_mixing.py:207,210,237,257,282),
 * the per-head einsum of ParallelLinear (VanillaNN.py:108-112; batch = n_split), the FFN / pointwise-conv /
 * post-conv Linears of the Conformer layer (Conformer.py:128-157,458-472) and their autograd backward.
 * splits > 1 partitions K over blockIdx (requires out_mode SMX_OUT_ATOMIC_F32). */
int smx_gemm(int layout, int dtype, const void* A, int64_t lda, int64_t strideA, const void* B, int64_t ldb,
             int64_t strideB, void* C, int64_t ldc, int64_t strideC, int N, int M, int K, int batch, int splits,
             const smx_epilogue* epi, void* stream);
/* Which kernel would smx_gemm launch for these arguments?  Same checks, same dispatch, no launch: fills `plan` with the template
 * arguments of the instantiation as a profiler prints them - gemm_kernel<T, a_kc, b_kc, tile_n, tile_m, vec, lnf, gather>
 * (kernel 0) or gemm_tn_dma_kernel (kernel 1).  bench.py groups its in-step records by this symbol. */
typedef struct smx_gemm_plan { int32_t kernel, a_kc, b_kc, tile_n, tile_m, vec, lnf, gather; } smx_gemm_plan;
int smx_gemm_plan_query(int layout, int dtype, const void* A, int64_t lda, int64_t strideA, const void* B, int64_t ldb,
                        int64_t strideB, void* C, int64_t ldc, int64_t strideC, int N, int M, int K, int batch, int splits,
                        const smx_epilogue* epi, smx_gemm_plan* plan);

/* Panel-resident GEMM for the SHORT reductions with WIDE outputs of an encoder layer (bf16, K = 256 or 512, M % 64 == 0):
 *   forward      C = alpha * D(act(A Wp + bias)) * row_mask, optionally saving the pre-activation Z   (epi: act, z, drop_* [drop_cols % 64 == 0], row_mask, alpha; bias: packed, below)
 *   act-grad     C = alpha * D((A Wp) * act'(Z)) * row_mask                                       (epi: SMX_EPI_ACT_GRAD, z = input, act, drop_*, row_mask, alpha)
 * i.e. the FFN up-projection  nn.Linear(d_model, d_ffn) + activation + dropout  (Conformer.py:458-472, Branchformer.py:142-157)
 * and the first half of the autograd backward of the down-projection that follows it (dH = dY W2, then the activation / dropout
 * backward), the two output-bound GEMMs of every encoder layer.  A 128-row panel of A stays in LDS for all M columns and
 * the weight is read in MFMA fragment order straight into registers, so it must be PRE-PACKED:
 *   smx_weight_pack(W, transposed = 0, bias): W is the (M, K) weight of the forward, bias its fp32 [M] bias or NULL;
 *   smx_weight_pack(W, transposed = 1, NULL): W is the (K, M) weight of the Linear whose dgrad this is (dH = dY W: reduce-strided).
 * The bias travels INSIDE the packed image (one more fragment per 32 columns, split into a bf16 high and low part: exact to
 * 2^-17 relative), so smx_gemm_panel takes no epi->bias.  The image has smx_weight_pack_bytes(M, K) bytes (16-byte aligned) and
 * must be re-packed whenever W or the bias change.
 * Same arithmetic as smx_gemm with the same epilogue fields (fp32 accumulation, the same dropout mask for the same seed), except
 * that the activation / its gradient is evaluated on the bf16-ROUNDED pre-activation / product (torch autocast semantics: the
 * Linear's output is a bf16 tensor).  Any other epilogue field (bias, residual, C0, LayerNorm, fp32 output,
 * column sums) returns SMX_EUNSUPPORTED: use smx_gemm.  smx_gemm_panel_ok: can these sizes take the panel path at all? */
int smx_gemm_panel_ok(int dtype, int N, int M, int K);
/* rows per panel the launch for (N, M) would use: 128, or 64 / 32 when a small batch has too few 128-row panels for the chip (round 6) */
int smx_gemm_panel_rows(int N, int M);
size_t smx_weight_pack_bytes(int M, int K);
int smx_weight_pack(int dtype, const void* W, int64_t ldw, int transposed, const float* bias, int M, int K, void* packed, void* stream);
int smx_gemm_panel(int dtype, const void* A, int64_t lda, const void* Wpacked, void* C, int64_t ldc, int N, int M, int K,
                   const smx_epilogue* epi, void* stream);
/* Many smx_weight_pack calls in ONE launch (every packed image of a model, right after the optimizer rewrote the weights): a
 * table of jobs in DEVICE memory with the same per-job requirements as smx_weight_pack; block_start = the prefix sum of
 * smx_weight_pack_job_blocks(M, K) over the jobs before this one, total_blocks = the sum over all of them. */
typedef struct smx_pack_job {
  const void* W; int64_t ldw; const float* bias; void* packed; int32_t M, K, transposed, block_start;
} smx_pack_job;
int smx_weight_pack_job_blocks(int M, int K);
int smx_weight_pack_jobs(int dtype, const smx_pack_job* jobs_dev, int njobs, int total_blocks, void* stream);

/* Weight gradient of a (batched) Linear: dW[b] (M x K) += alpha * dZ[b]^T X[b], reducing over `rows` frames
 * (dZ (rows, M), X (rows, K), both row-major).  Split-K over the frame dimension into fp32 slabs in `workspace`
 * (smx_linear_wgrad_workspace bytes) followed by one fixed-order reduction: bit-reproducible, no atomics.
 * dbias (optional, fp32 [batch][M]): dbias += alpha * column sums of dZ - the bias gradient comes out of the same
 * launch (the kernel sums the dZ tiles it stages anyway), so no separate pass over dZ is needed for it.
 * Autograd backward of every nn.Linear / ParallelLinear on the path. */
size_t smx_linear_wgrad_workspace(int rows, int M, int K, int batch);
int smx_linear_wgrad(int dtype, const void* dZ, int64_t lddz, int64_t strideZ, const void* X, int64_t ldx,
                     int64_t strideX, float* dW, int64_t lddw, int64_t strideW, float* dbias, int rows, int M, int K,
                     int batch, float alpha, void* workspace, void* stream);

/* Deferred variant: only the split-K GEMM; the slabs (and, with want_bias, the bias partials behind them) stay in
 * `workspace` (same size query) for a later smx_reduce_jobs.  Outputs: *nslabs, *slab_stride (floats between slabs of
 * the [batch][M][K] weight image), *bias_offset (floats from the workspace start to the [nslabs][batch][M] bias
 * partials).  Returns SMX_EUNSUPPORTED for shapes the slab path cannot take (K % 4 != 0): use smx_linear_wgrad. */
int smx_linear_wgrad_partial(int dtype, const void* dZ, int64_t lddz, int64_t strideZ, const void* X, int64_t ldx,
                             int64_t strideX, int rows, int M, int K, int batch, int want_bias, void* workspace,
                             int32_t* nslabs, int64_t* slab_stride, int64_t* bias_offset, void* stream);

/* ALL the weight gradients of one encoder layer in one launch (bf16): for every item w
 *   slabs_w[s] (M_w x K_w, fp32) = dZ_w[rows of slice s]^T X_w[rows of slice s],     s < splits
 * and, with want_bias, bias partials [splits][M_w] (column sums of dZ_w) behind the slabs in the item's workspace
 * (smx_wgrad_group_workspace(M, K, splits) bytes, 16-byte aligned); fold them with smx_reduce_jobs
 * (src = workspace, src_stride = M*K, nsrc = splits; bias: src = workspace + splits*M*K floats, src_stride = M).
 * Every item reduces over the SAME `rows` frames (>= 64; the rows % 64 tail is staged zero-filled by the last split), M and K are
 * multiples of 256, operands 16-byte aligned with leading dimensions % 8 == 0.  One 512-thread workgroup per CU owns a
 * (weight, 256 x 256 tile, K slice) item; smx_wgrad_group_splits picks the slice count that fills the chip once.
 * Autograd backward (dW, db) of all the nn.Linear / Conv1d(k=1) modules of a ConformerEncoderLayer /
 * BranchformerEncoderLayer (Conformer.py:479-537, Branchformer.py:243-334) at once. */
#define SMX_WGRAD_GROUP_MAX 16
typedef struct smx_wgrad_item {
  const void* dZ; int64_t lddz;      /* (rows, M) gradient w.r.t. the layer's pre-activation                 */
  const void* X;  int64_t ldx;       /* (rows, K) the layer's input                                          */
  void* workspace;                   /* [splits][M*K] fp32 slabs, then [splits][M] bias partials             */
  int32_t M, K, want_bias, pad;
} smx_wgrad_item;
int smx_wgrad_group_splits(int rows, const smx_wgrad_item* items, int nitems);
size_t smx_wgrad_group_workspace(int M, int K, int splits);
int smx_wgrad_group(int dtype, int rows, const smx_wgrad_item* items, int nitems, int splits, void* stream);

/* Small batches (round 6): the same weight gradients WITHOUT split-K slabs - every 128 x 128 tile of every weight walks all `rows`
 * frames and adds its product INTO the gradient, dW[i] (M x K, float32, row stride lddw) += dZ_i^T X_i, dbias[i] (M) += column sums of
 * dZ_i (NULL: none).  No workspace, no smx_reduce_jobs pass; each gradient element has exactly one writer (bit-reproducible).  M, K
 * multiples of 128.  The slab form above is the one for long batches (its K-slices fill the chip; this one would not). */
typedef struct smx_wgrad_direct_item {
  const void* dZ; int64_t lddz;
  const void* X;  int64_t ldx;
  float* dW; int64_t lddw;
  float* dbias;
  int32_t M, K;
} smx_wgrad_direct_item;
int smx_wgrad_group_direct_ok(int rows, int M, int K);
int smx_wgrad_group_direct(int dtype, int rows, const smx_wgrad_direct_item* items, int nitems, void* stream);

/* One launch for many small fixed-order reductions
 *   dst[i*ldd + j] += alpha * sum_{s < nsrc} src[s*src_stride + i*src_ld + j]      (i < rows, j < cols; src_ld 0 = cols)
 * : weight-gradient slabs, bias partials, LayerNorm dgamma/dbeta partial rows.  `vec` = 1
 * when cols, ldd, src_ld, src_stride are multiples of 4 and src / dst are 16-byte aligned.  jobs and block_starts (njobs + 1 entries,
 * prefix sums of smx_reduce_job_blocks) live in device memory; tables can be cached while the pointers stay valid. */
typedef struct smx_reduce_job {
  const float* src; float* dst; int64_t src_stride; int64_t ldd; int32_t nsrc; int32_t rows; int32_t cols; float alpha;
  int32_t vec; int32_t src_ld;
} smx_reduce_job;
int smx_reduce_job_blocks(const smx_reduce_job* job_host);
int smx_reduce_jobs(const smx_reduce_job* jobs_dev, const int32_t* block_starts_dev, int njobs, int total_blocks,
                    void* stream);

/* Y = R + alpha * act(X W^T + b [+C0]) * mask ; thin wrapper over smx_gemm(NT).
 * Replaces summary_mixing.py:257 (global_proj * mask), :207/:210 (local/summary proj * mask),
 * :282-284 (merge with the per-utterance summary folded in as C0 = sbar W_s^T + b, SMX_C0_GROUP, div=T). */
int smx_linear_act_mask_fwd(int dtype, const void* X, int64_t ldx, const void* W, int64_t ldw, void* Y,
                            int64_t ldy, int N, int M, int K, const smx_epilogue* epi, void* stream);

/* dZ = dropout_mask(seed) * dY * mask * act'(Z)  (elementwise; the mask of the forward's fused dropout is regenerated
 * from the seed), plus fused parameter-gradient side reductions:
 *   dbias[m]          += sum_n dZ[n,m]                      (optional; per-strip partials in `workspace`,
 *                                                            smx_act_mask_bwd_workspace bytes, fixed-order reduce)
 *   dgroup[n/div, m]  += sum over the rows of group n/div   (fp32 atomics, optional; the backward of a
 *                                                            SMX_C0_GROUP side input)
 * Backward of the epilogue above (autograd of summary_mixing.py:207-284). dY is pre-scaled by alpha. */
size_t smx_act_mask_bwd_workspace(int N, int M);
int smx_act_mask_bwd(int dtype, const void* dY, int64_t lddy, const void* Z, int64_t ldz,
                     const uint8_t* row_mask, void* dZ, int64_t lddz, int N, int M, int act, float alpha,
                     float* dbias, float* dgroup, int64_t lddgroup, int group_div, float drop_p, uint64_t drop_seed, const uint64_t* epoch,
                     void* workspace, void* stream);

/* Masked mean over time: out[b,:] = sum_t S[b,t,:] * mask[b,t] / sum_t mask[b,t]   (fp32 out (B,D)).
 * S is (B*T, D) with leading dimension lds.  mask NULL => all valid.  scale_by_count=0 gives the plain sum.
 * inv_count (optional, (B) fp32) receives 1/sum_t mask[b,t].  `workspace` holds
 * smx_masked_mean_workspace(B,T,D) bytes (split-T partial sums, combined in a fixed order => bit-reproducible).
 * A row with zero valid frames yields NaN like the reference.  Replaces summary_mixing.py:218-220, :264-266,
 * :305-307.  This is the HBM-roofline kernel of BASELINE config 5. */
size_t smx_masked_mean_workspace(int B, int T, int D);
int smx_masked_mean_fwd(int dtype, const void* S, int64_t lds, const uint8_t* mask, float* out, float* inv_count,
                        int B, int T, int D, int scale_by_count, void* workspace, void* stream);
/* Backward / broadcast: dS[b,t,:] = g[b,:] * (inv_count ? inv_count[b] : 1) for every t (the row mask is
 * applied by the producer's smx_act_mask_bwd).  Also the forward `repeat` (summary_mixing.py:222,267), there with the
 * training dropout of the concatenated merge input fused in (drop_p > 0: mask = f(seed, row * D + col), the
 * smx_dropout indexing; summary_mixing.py:237-239). */
int smx_masked_mean_bwd(int dtype, const float* g, const float* inv_count, void* dS, int64_t ldds, int B, int T,
                        int D, float drop_p, uint64_t drop_seed, const uint64_t* epoch, void* stream);

/* Small batches (round 6): the masked mean over time AND its broadcast in ONE launch, fixed summation order (no atomics), for
 * smx_pool_bcast_ok(B, T, D) shapes: T <= 4096 and either B * T <= SMX_POOL_FUSE_MAX_ROWS frames (default 16 384) or at least
 * 256 (utterance, 64-column group) pairs, B * ceil(D / 64) >= 256 (a large batch of ordinary utterances fills the chip on its own):
 *   sum[b,:] = sum_t S[b,t,:] * mask_in[b,t];  mean_out[b,:] (optional) = sum (* 1 / count[b] when scale_by_count);
 *   inv_out[b] (optional) = 1 / count[b];
 *   dS[b,t,:] (optional) = D( value[b,:] * (inv_in ? inv_in[b] : 1) ) [* act'(Z[b,t,:]) * mask_out[b,t] when Z / mask_out are given]
 * i.e. smx_masked_mean_fwd followed by smx_masked_mean_bwd (forward `repeat` + the merge input's dropout, summary_mixing.py:218-222,
 * 237-239,264-267) or by smx_masked_mean_bwd_act (the backward of the same lines), without the workspace round trip and two of
 * the three launches.  Dropout (drop_p > 0) and the act / mask backward exclude each other. */
int smx_pool_bcast_ok(int B, int T, int D);
int smx_pool_bcast(int dtype, const void* S, int64_t lds, const uint8_t* mask_in, float* mean_out, const float* inv_in, float* inv_out,
                   void* dS, int64_t ldds, int B, int T, int D, int scale_by_count, float drop_p, uint64_t drop_seed,
                   const uint64_t* epoch, const void* Z, int64_t ldz, const uint8_t* mask_out, int act, void* stream);

/* Same broadcast with the activation / mask backward of the projection that produced the summary columns fused in:
 *   dS[b,t,:] = g[b,:] * inv_count[b] * act'(Z[b,t,:]) * row_mask[b,t]      (Z and/or row_mask given)
 * i.e. the dZ of `s = act(x W_s^T + b) * mask` (summary_mixing.py:210,257) without writing and re-reading the broadcast. */
int smx_masked_mean_bwd_act(int dtype, const float* g, const float* inv_count, void* dS, int64_t ldds, const void* Z,
                            int64_t ldz, const uint8_t* row_mask, int act, int B, int T, int D, void* stream);

/* DynChunk summary (sum_mask path, summary_mixing.py:224-235, :269-280) in O(T): frame t of chunk
 * c = t / chunk sees frames [max(0,(c-left)*chunk), min(T,(c+1)*chunk)) (left < 0: unlimited);
 * out[b,t,:] = sum over that window of S[b,.,:] / window length  (the denominator ignores padding, as the
 * reference's rowsum(sum_mask) does).  bwd is the transposed operator.  workspace:
 * smx_chunk_mean_workspace bytes (per-chunk fp32 sums). */
size_t smx_chunk_mean_workspace(int B, int T, int D, int chunk);
int smx_chunk_mean_fwd(int dtype, const void* S, int64_t lds, void* out, int64_t ldo, int B, int T, int D,
                       int chunk, int left, void* workspace, void* stream);
int smx_chunk_mean_bwd(int dtype, const void* dOut, int64_t ldo, void* dS, int64_t lds, int B, int T, int D,
                       int chunk, int left, void* workspace, void* stream);

/* SummaryMixing-expdecay summary in O(T) (the reference materialises the (T,T) Laplace matrix gamma^|i-j|,
 * summary_mixing.py:316-365, and computes (M s) / rowsum(M), :233-235 - O(T^2)):
 *   fwd: out[b,t,:] = sum_j decay^|t-j| S[b,j,:] / sum_j decay^|t-j|   (j over ALL T frames: padding is ignored in the
 *        denominator exactly like the reference; padded frames of S are zero because the projection is masked);
 *   bwd: dS = M (dOut / rowsum(M))  (M is symmetric).  Two-sided exponential recurrences, chunked scan over T.
 * Only for sum_mask == None; with a DynChunk mask the reference's dense path is kept. */
size_t smx_expdecay_mean_workspace(int B, int T, int D);
int smx_expdecay_mean_fwd(int dtype, const void* S, int64_t lds, void* out, int64_t ldo, int B, int T, int D, float decay,
                          void* workspace, void* stream);
int smx_expdecay_mean_bwd(int dtype, const void* dOut, int64_t ldo, void* dS, int64_t lds, int B, int T, int D, float decay,
                          void* workspace, void* stream);
/* LayerNorm over the last dim with an optional fused activation: Y = act(LN(X))
 * (torch.nn.LayerNorm; Conformer.py:146,152-153,475-476,738).  stats (N,2) fp32 = (mean, rstd), optional in fwd.
 *
 * Forward: smx_layernorm_fwd(&a, stream).  X and Y have dtype `dtype` unless x_f32 = 1: X is then float32 and Y of dtype
 * `dtype` (fp32 residual stream -> bf16 GEMM input: torch.nn.LayerNorm under autocast; bf16 Y needs D % 4 == 0, D <= 2048
 * and aligned rows, else SMX_EUNSUPPORTED).
 * Y2 != NULL: two LayerNorms in ONE pass over the float32 residual stream: Y = LN(X) (float32: `dtype` SMX_F32, `act` none -
 * the layer-final norm2, Conformer.py:536, the next layer's stream input) and Y2 = LN2(Y) (dtype2: the LayerNorm of the next
 * layer's first feed-forward module, Conformer.py:458-459,507) with gamma2 / beta2 / eps2 / stats2.  Equal to the fp32 forward
 * followed by the x_f32 forward to an ulp; Y is not re-read and is stored with the non-temporal hint.  D % 4 == 0, D <= 2048,
 * 16-byte aligned rows (SMX_EUNSUPPORTED otherwise). */
typedef struct smx_ln_fwd {
  int32_t dtype;       int32_t x_f32;        /* dtype of Y (and of X unless x_f32)                                          */
  const void* X;       int64_t ldx;
  const float* gamma;  const float* beta;
  void* Y;             int64_t ldy;
  float* stats;                              /* (N, 2) or NULL                                                              */
  float eps;           int32_t act;
  int32_t N;           int32_t D;
  /* optional second LayerNorm of Y (NULL Y2 = off) */
  const float* gamma2; const float* beta2;
  void* Y2;            int64_t ldy2;
  float* stats2;
  float eps2;          int32_t dtype2;
} smx_ln_fwd;
int smx_layernorm_fwd(const smx_ln_fwd* a, void* stream);

/* Backward: smx_layernorm_bwd(&a, stream).
 *   dX = R + LNbwd(dY * act'(LN(X)))   (R optional residual-gradient, dtype T; LN(X) is recomputed from the stats);
 * dgamma/dbeta += per-block partial sums (in `workspace`, smx_layernorm_bwd_workspace bytes) reduced in a fixed order:
 * bit-reproducible, no atomics.  With dgamma == dbeta == NULL the partial rows [smx_layernorm_bwd_blocks(N)][2][D] stay in the
 * workspace for smx_reduce_jobs: two jobs, src = ws (dgamma) and ws + D (dbeta), src_stride 2*D, rows 1, cols D.
 * dY, R, dX, dX2 have dtype `dtype`; X too unless x_f32 = 1 (float32 X next to bf16 gradients: torch.nn.LayerNorm under
 * autocast; D % 4 == 0, D <= 2048 and aligned rows, else SMX_EUNSUPPORTED).
 * Optional, each from the registers that hold dX:
 *  - dX2 != NULL: a second output  dX2 = alpha2 * Dropout(dX; drop_p2, drop_seed2, index n*D + c) * row_mask2[n]  (D <= 2048)
 *    - the first thing the next backward block does to this gradient (Conformer.py:507,536: the FFN module's 1/2 * dropout;
 *    :146-152,327-331: the conv module's dropout and padding mask), so that block needs no elementwise pass of its own.
 *  - slabs != NULL (instead of dY): the incoming gradient is the sum of `nslab` (1..16) float32 split-K slabs ((N, D) each,
 *    slab_stride elements apart; added in slab order) - the dgrad of the Linear behind the LayerNorm computed by
 *    smx_gemm_panel_slabs: reducer and LayerNorm backward in one launch.  bf16, dgamma = dbeta = NULL (partial rows stay in
 *    `workspace` for smx_reduce_jobs), D <= 2048 and aligned rows.
 *  - Z != NULL: backward THROUGH the activation that produced the LayerNorm's input, X = zact(Z) (Z the saved pre-activation):
 *      dX = zact'(Z) * LNbwd(dY)   (act must be SMX_ACT_NONE: a LayerNorm without a fused activation of its own; no R, no dX2)
 *    - the CSGU of the Branchformer's cgMLP normalises the gate half of GELU(channel_proj1(x)) (Branchformer.py:84-96 via the
 *    upstream ConvolutionalSpatialGatingUnit), so the gradient of that half reaches channel_proj1's dZ without the separate
 *    activation-backward pass over it.  bf16, D <= 2048, D % 8 == 0, 16-byte aligned rows (else SMX_EUNSUPPORTED: run the plain
 *    backward + smx_act_mask_bwd). */
typedef struct smx_ln_bwd {
  int32_t dtype;       int32_t x_f32;
  const void* dY;      int64_t lddy;         /* the incoming gradient, or NULL with slabs                                  */
  const float* slabs;  int64_t slab_stride;
  int32_t nslab;       int32_t act;
  const void* X;       int64_t ldx;
  const float* gamma;  const float* beta;
  const float* stats;                        /* (N, 2) mean | rstd of the forward                                          */
  const void* R;       int64_t ldr;          /* or NULL                                                                     */
  void* dX;            int64_t lddx;
  float* dgamma;       float* dbeta;         /* [D] or both NULL                                                            */
  void* workspace;
  void* dX2;           int64_t lddx2;        /* second output or NULL                                                       */
  const uint8_t* row_mask2;                  /* [N] or NULL                                                                 */
  float alpha2;        float drop_p2;
  uint64_t drop_seed2;
  const uint64_t* epoch;                     /* device step counter mixed into drop_seed2 (smx_step_counter_add), or NULL  */
  const void* Z;       int64_t ldz;          /* pre-activation or NULL                                                      */
  int32_t zact;        int32_t N;
  int32_t D;           int32_t pad_;
} smx_ln_bwd;
int smx_layernorm_bwd(const smx_ln_bwd* a, void* stream);
int smx_layernorm_bwd_blocks(int N);
size_t smx_layernorm_bwd_workspace(int N, int D);

/* Fused GLU + depthwise Conv1d over time (Conformer.py:131-145,317-325):
 *   u[b,t,c] = P[b,t,c] * sigmoid(P[b,t,D+c]);  Y[b,t,c] = bias[c] + sum_j w[c,j] u[b,t+j-(k-1)/2,c]
 * glu=0: u = P (ldp >= D).  pad SMX_PAD_ZERO (Conformer) | SMX_PAD_REFLECT (Branchformer CSGU).
 * chunk > 0: Dynamic Chunk Convolution (Conformer.py:190-313): inputs at or beyond the end of the output
 * frame's own chunk read as zero.  gate != NULL: Y *= gate (CSGU x1*x2).  w (D,k) fp32, bias (D) fp32. */
/* One descriptor for both directions (zero it, then set what the call uses); the backward reads dY through Y / ldy.
 * drop_p > 0 (forward): inverted dropout of Y fused in (mask index = global row * D + channel, as smx_dropout on Y) - the CSGU's
 * own dropout (upstream ConvolutionalSpatialGatingUnit.forward); SMX_EUNSUPPORTED off the rolling CSGU route - run smx_dropout. */
typedef struct smx_dwconv_args {
  int32_t dtype;       int32_t glu;
  const void* P;       int64_t ldp;
  const float* w;      const float* bias;
  const void* gate;    int64_t ldg;          /* or NULL                                                                     */
  void* Y;             int64_t ldy;          /* forward: the output; backward: dY (read only)                               */
  void* dP;            int64_t lddp;         /* backward: same shape as P                                                   */
  void* dgate;         int64_t lddg;         /* backward: = dY * conv, with gate                                            */
  float* dw;           float* dbias;         /* backward: += ; both NULL = leave the partial rows in the workspace          */
  void* workspace;                           /* backward: smx_dwconv1d_glu_bwd_workspace bytes, or NULL                     */
  int32_t B, T, D, k, pad_mode, chunk;
  float drop_p;        int32_t pad_;
  uint64_t drop_seed;  const uint64_t* epoch;
} smx_dwconv_args;
/* The kernel family a call gets and its launch: route SMX_DW_*; chunked = Dynamic Chunk Convolution; deferrable
 * (backward): dw == NULL may leave the partial_rows rows [D][k+1] (taps, then the bias term) in the workspace; grid of the main
 * kernel (grid[0] == 0: empty shape, no launch); rolling routes: seg frames per wave segment, nseg segments per utterance. */
enum { SMX_DW_TILED = 0, SMX_DW_WINDOW = 1, SMX_DW_ROLL = 2, SMX_DW_ROLL_CSGU = 3 };
typedef struct smx_dwconv_plan { int32_t route, chunked, deferrable, partial_rows, grid[3], seg, nseg, pad_; } smx_dwconv_plan;
int smx_dwconv_fwd(const smx_dwconv_args* a, void* stream);
/* dw / dbias += the partial tap gradients in `workspace`, reduced in a fixed order (NULL: the tiled kernel with atomics).  dw == NULL:
 * the plan's partial_rows rows stay there for smx_reduce_jobs (two jobs with src_ld = k+1); SMX_EUNSUPPORTED if not deferrable. */
int smx_dwconv_bwd(const smx_dwconv_args* a, void* stream);
/* The checks and the decision of the two calls above for this descriptor, without a launch (needs no GPU). */
int smx_dwconv_plan_query(const smx_dwconv_args* a, int backward, smx_dwconv_plan* plan);
size_t smx_dwconv1d_glu_bwd_workspace(int B, int T, int D, int k);   /* bytes that hold the partial rows of every route */

/* ---- front-end (arithmetic lives in un-vendored SpeechBrain: parity unpinned, spec = oracle) ----
 * Log-mel filterbank (speechbrain.lobes.features.Fbank, ...transducer.yaml:171-175):
 *   smx_frame_window : frames[b*T+t, j] = window[j] * wav[b, t*hop + j - n_fft/2]  (center=True, zero pad), fp32
 *   DFT              : smx_gemm(NT, F32) of the frames with a [cos | -sin] basis (exact-fp32 MFMA)
 *   smx_mel_db       : power spectrum -> mel filterbank (n_mels x n_bins fp32) -> 10 log10(max(., amin)) -> per-utterance
 *                      top_db clamp; spec (B*T, lds) holds re at column f and im at column im_off + f.
 * Conv subsampling (ConvolutionFrontEnd, ...yaml:247-254): 3x3 / stride 2 / reflect pad 1, channels-last:
 *   smx_im2col_s2 : x (B,T,F,C) -> col (B*ceil(T/2)*ceil(F/2), Kp), column (dt*3+df)*C + c, zero beyond 9*C
 *   conv          : smx_gemm(NT) col x W^T + bias, then smx_layernorm_fwd over (F2*Cout) with fused LeakyReLU
 *   smx_col2im_s2 : backward of im2col (gather form, no atomics). */
/* The same DFT without the frame matrix and at half the reduction length: frames are rows of the zero-padded waveform
 * (wav_padded (B, ldw): n_fft / 2 zeros in front, frame t of utterance b = samples [t hop, t hop + n_fft)), the (symmetric) window is
 * folded into the bases, and the real DFT is split into its cosine part on s[j] = x[j] + x[n - j] (basis_cos (rows_basis, n/2 + 4):
 * window[j] cos(2 pi k j / n) for j <= n/2, zero behind) and its sine part on d[j] = x[j] - x[n - j] (basis_sin (rows_basis, n/2):
 * -window[j] sin(2 pi k j / n)); s and d are formed inside the GEMM's operand loader.  spec (B*T, lds): re at column k, im at im_off + k. */
int smx_dft_frames(const float* wav_padded, int64_t ldw, const float* basis_cos, const float* basis_sin, float* spec, int64_t lds,
                   int im_off, int B, int T, int n_fft, int hop, int rows_basis, void* stream);
int smx_frame_window(const float* wav, int64_t ldw, const float* window, float* frames, int B, int L, int T, int n_fft,
                     int hop, void* stream);
size_t smx_fbank_workspace(int B, int T, int n_mels);
int smx_mel_db(int out_dtype, const float* spec, int64_t lds, int im_off, const float* fb, int n_bins, int n_mels,
               float amin, float top_db, void* out, int B, int T, void* workspace, void* stream);
int smx_im2col_s2(int dtype, const void* x, void* col, int B, int T, int F, int C, int Kp, void* stream);
int smx_col2im_s2(int dtype, const void* dcol, void* dx, int B, int T, int F, int C, int Kp, void* stream);
/* The first conv block in one pass per direction (1 input channel, O = 64, F a multiple of 16 up to 160; SMX_EUNSUPPORTED
 * otherwise: im2col + smx_linear_k16_fwd / smx_gemm + smx_layernorm_*).  X (B,T,F) and Y / dA (B*ceil(T/2), (F/2)*O) dtype T;
 * W9 (O, 9) fp32 taps (dt*3 + df), gamma / beta ((F/2)*O) fp32.
 *   fwd: Y = act(LayerNorm_row(conv3x3_s2_reflect(X) + bias) * gamma + beta), stats (rows, 2) = mean | rstd
 *   bwd: grads[(F/2)*O | (F/2)*O | O*9 | O] += dgamma | dbeta | dW9 | dbias, from dA and X alone (the convolution is recomputed;
 *        nothing of activation size is written); `workspace` = smx_conv1_ln_workspace bytes of per-workgroup partial rows,
 *        folded in a fixed order. */
size_t smx_conv1_ln_workspace(int B, int T, int F, int O);
int smx_conv1_ln_fwd(int dtype, const void* X, const float* W9, const float* bias, const float* gamma, const float* beta, float eps,
                     int act, void* Y, float* stats, int B, int T, int F, int O, void* stream);
int smx_conv1_ln_bwd(int dtype, const void* dA, const void* X, const float* W9, const float* bias, const float* gamma,
                     const float* beta, const float* stats, int act, float* grads, void* workspace, int B, int T, int F, int O,
                     void* stream);
/* Y (N, M) = X (N, 16) W (M, 16)^T + bias: the first block's convolution (9 taps of one input channel in 16 columns) on
 * the VALU, bf16 in / out, fp32 accumulation; dense rows.  SMX_EUNSUPPORTED for other shapes (use smx_gemm). */
int smx_linear_k16_fwd(int dtype, const void* X, const void* W, const float* bias, void* Y, int64_t N, int M, void* stream);
/* The second block's convolution and its weight gradient WITHOUT the (rows, 9 C) patch matrix: the MFMA GEMM kernels gather
 * their operand from the channels-last input X (B,T,F,C) themselves (one tap per K tile / column tile).  Built for bf16, C = 64
 * (SMX_EUNSUPPORTED otherwise: smx_im2col_s2 + smx_gemm / smx_linear_wgrad).  Wg / dWg (O, Kp) GEMM layout (column
 * (dt*3+df)*C + c); Y / dY (B*ceil(T/2)*ceil(F/2), O) dense.
 *   fwd  : Y = conv(X) + bias
 *   wgrad: dWg (fp32) += dY^T patches(X), dbias += column sums of dY; slab split-K + fixed-order reduction (`workspace` =
 *          smx_conv2d_s2_wgrad_workspace bytes, 16-byte aligned). */
int smx_conv2d_s2_fwd(int dtype, const void* X, const void* Wg, const float* bias, void* Y, int B, int T, int F, int C, int O,
                      int Kp, void* stream);
size_t smx_conv2d_s2_wgrad_workspace(int B, int T, int F, int C, int O);
int smx_conv2d_s2_wgrad(int dtype, const void* dY, const void* X, float* dWg, float* dbias, int B, int T, int F, int C, int O,
                        int Kp, void* workspace, void* stream);
/* Direct input gradient of that convolution, without the (rows, 9 C) column matrix: dX (B,T,F,C) from dY
 * (B,ceil(T/2),ceil(F/2),O) and the GEMM-layout weight Wg (O, Kp) (column (dt*3+df)*C + c).  Built for the recipe's second
 * block (bf16, C = 64, O = 32; SMX_EUNSUPPORTED otherwise: use the dgrad GEMM + smx_col2im_s2).  MFMA, no atomics. */
int smx_conv2d_s2_dgrad(int dtype, const void* dY, const void* Wg, void* dX, int B, int T, int F, int C, int O, int Kp,
                        void* stream);

/* y = a*x (+ b*y0): generic strided elementwise helper (dtype T). */
int smx_axpby(int dtype, float a, const void* X, int64_t ldx, float b, const void* Y0, int64_t ldy0, void* Y,
              int64_t ldy, int N, int D, void* stream);
/* Inverted dropout with a counter-based generator: Y[n,c] = keep(seed, n*D+c) ? X[n,c]/(1-p) : 0 (in place allowed).
 * The mask is a pure function of (seed, element index): calling it again on the gradient with the same seed is the
 * backward.  Replaces nn.Dropout at summary_mixing.py:238,283, Conformer.py:157,461-472, TransformerASR.py:353. */
int smx_dropout(int dtype, const void* X, int64_t ldx, void* Y, int64_t ldy, int N, int D, float p, uint64_t seed, const uint64_t* epoch,
                void* stream);
/* Y[n,:] += table[n % R,:] (fp32 table): abs-sine positional encoding added after the input dropout
 * (TransformerASR.py:547-549). */
int smx_add_rowtable(int dtype, void* Y, int64_t ldy, const float* table, int R, int N, int D, void* stream);
/* fp32 -> T cast of a flat buffer (bf16 shadow weights). */
int smx_cast_from_f32(int dtype, const float* src, void* dst, int64_t n, void* stream);
int smx_cast_to_f32(int dtype, const void* src, float* dst, int64_t n, void* stream);

/* Fused AdamW over a flat fp32 parameter buffer (decoupled weight decay, torch.optim.AdamW semantics;
 * recipes/LibriSpeech/.../conformer_summarymixing_transducer.yaml:395-399).  grad_scale multiplies the
 * gradient first (1/world_size and the global-norm clip factor); `gscale_dev` (optional, device fp32[1])
 * is multiplied in as well so the clip factor never visits the host.  shadow (optional) receives the
 * updated parameters cast to bf16. */
int smx_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                   int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                   float grad_scale, const float* gscale_dev, const uint64_t* step_dev, void* stream);
/* smx_adamw_step with the learning rate in device memory: a non-NULL `lr_dev` (fp32[1], written by smx_lr_schedule) replaces
 * `lr`; with lr_dev NULL, or holding lr, the result equals smx_adamw_step's bit for bit. */
int smx_adamw_step_lr(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                      int64_t n, float lr, const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, int step,
                      float grad_scale, const float* gscale_dev, const uint64_t* step_dev, void* stream);
/* Fused torch.optim.SGD (dampening 0) over a flat fp32 range, the second stage of the two-stage recipes
 * (recipes/AISHELL-1/.../hparams: SGD(lr_sgd, momentum=0.99, nesterov=True)):
 *   g = grad * grad_scale * gscale_dev[0] + weight_decay * p;  buf = momentum * buf + g;
 *   p -= lr * (nesterov ? g + momentum * buf : buf);           momentum == 0: p -= lr * g, momentum_buf may be NULL.
 * A zero-initialised buffer gives torch's first step (buf = g) exactly, so no step number is needed.  A non-NULL lr_dev (fp32[1])
 * replaces lr; a device clip factor gscale_dev[0] of exactly 0 skips the whole update (smx_clip_factor's verdict on a non-finite
 * norm: parameters, buffer and shadows untouched).  shadow (optional) receives the updated parameters cast to bf16.
 * 16-byte accesses of param / grad / momentum_buf and 8-byte stores of four shadows where the pointers sit at the same offset
 * from a 16-byte boundary (views of parallel flat buffers do), a scalar head and tail around them; any other alignment runs
 * scalar.  At most SMX_SGD_MAX_BLOCKS blocks of 256 lanes x 4 elements, grid-strided; no atomics: two runs agree bit for bit. */
#define SMX_SGD_MAX_BLOCKS 2048
int smx_sgd_step(float* param, const float* grad, float* momentum_buf, void* shadow_bf16, int64_t n, float lr,
                 const float* lr_dev, float momentum, float weight_decay, int nesterov, float grad_scale,
                 const float* gscale_dev, void* stream);
/* lr_out[0] = the learning rate of update t (counted from 1), evaluated in float64 by one thread and stored as float32.
 * t = step when step > 0, else step_dev[0] (the device step counter, smx_step_counter_add: a captured step follows its schedule
 * on replay).  The rate restates what a recipe gets by calling its scheduler once behind every optimizer step:
 *   t == 1: lr0, the optimizer's own rate.
 *   SMX_LR_NOAM (c0 = lr_initial, c1 = n_warmup_steps, c2 = model_size or 0), t >= 2, n = t - 1:
 *     c0 * norm * min(n^-0.5, n * c1^-1.5), norm = c1^0.5, or c2^-0.5 when c2 > 0.
 *   SMX_LR_WARM_EXP_DECAY (c0 = base rate, c1 = n_warmup_steps, c2 = total_steps, c3 = decay_factor), t >= 2, c = t - 2:
 *     c0 * c / c1 while c < c1, else min(c0, c0 * c3^((c - c1) / c2)). */
#define SMX_LR_NOAM 0
#define SMX_LR_WARM_EXP_DECAY 1
int smx_lr_schedule(int kind, double c0, double c1, double c2, double c3, double lr0, int64_t step,
                    const uint64_t* step_dev, float* lr_out, void* stream);
/* ---- InputNormalization between the filterbank and the CNN front-end (recipe key `normalize`:
 * speechbrain.processing.features.InputNormalization, …transducer.yaml:167-169; upstream-only arithmetic). ----
 * smx_utt_meanstd: mean[b,f] and unbiased std[b,f] over the frames t < len[b] (std clamped below by eps; 0 / 1 when the
 * respective normalisation is off; like torch, the std of fewer than two frames and the mean of none are NaN).  smx_stats_combine: glob = (1-w)*glob + w*mean_b(cur) (w = 1 replaces: the first
 * batch / norm_type "batch").  smx_colnorm: Y = (X - mean[b*stat_stride + f]) / std[...] over (B, T, F) rows b*T + t
 * (stat_stride 0 = shared statistics: "global" / "batch"; F = per-utterance: "sentence"). */
int smx_utt_meanstd(int dtype, const void* X, int64_t ldx, const int32_t* len, float* mean, float* std, int B, int T, int F,
                    int mean_norm, int std_norm, float eps, void* stream);
int smx_stats_combine(const float* cur_mean, const float* cur_std, int B, int F, float* glob_mean, float* glob_std, float weight,
                      void* stream);
int smx_colnorm(int dtype, const void* X, int64_t ldx, const float* mean, const float* std, int64_t stat_stride, void* Y,
                int64_t ldy, int B, int T, int F, void* stream);

/* ---- CTC head after the encoder (recipe keys `log_softmax`, `ctc_cost`:
 * …/LibriSpeech/ASR/transducer/hparams/conformer_summarymixing_transducer.yaml:297-298,331). ----
 * Y = log_softmax(X) over the last dim (N rows of V); bwd: dX = dY - exp(Y) * rowsum(dY).
 * Replaces speechbrain.nnet.activations.Softmax(apply_log=True). */
int smx_log_softmax_fwd(int dtype, const void* X, int64_t ldx, void* Y, int64_t ldy, int N, int V, void* stream);
int smx_log_softmax_bwd(int dtype, const void* dY, int64_t lddy, const void* Y, int64_t ldy, void* dX, int64_t lddx, int N,
                        int V, void* stream);
/* CTC negative log-likelihood per utterance and its gradient; replaces torch.nn.functional.ctc_loss(...,
 * zero_infinity=True) as called by speechbrain.nnet.losses.ctc_loss.
 *   log_probs (B, T, V) row-major with leading dimension ldlp (rows b*T + t), dtype T (log-softmax outputs);
 *   targets int32 (B, Smax) padded, in_len / tgt_len int32 (B) absolute lengths, blank < V;
 *   fwd: nll[b] = -log p(targets_b | x_b)  (+inf when no alignment exists); keeps the forward variables in `workspace`
 *        (smx_ctc_workspace bytes) for the backward;
 *   bwd: grad[b,t,v] = gscale[b] * (exp(lp) - exp(log sum_{s: l'_s = v} alpha*beta/y + nll[b])), zero for t >= in_len[b]
 *        and for utterances with infinite nll (the convention of torch's ctc_loss backward: the gradient w.r.t. the
 *        unnormalised logits; pushing it through smx_log_softmax_bwd leaves it unchanged).  gscale[b] carries the
 *        reduction (1/B, 1/tgt_len, ...) times the upstream gradient.  Must follow smx_ctc_loss_fwd on the same workspace.
 *        The per-label sums follow each label's occurrence chain in a fixed order: no atomics, bit-reproducible. */
size_t smx_ctc_workspace(int B, int T, int Smax);
int smx_ctc_loss_fwd(int dtype, const void* log_probs, int64_t ldlp, const int32_t* targets, const int32_t* in_len,
                     const int32_t* tgt_len, int B, int T, int V, int Smax, int blank, float* nll, void* workspace, void* stream);
int smx_ctc_loss_bwd(int dtype, const void* log_probs, int64_t ldlp, const int32_t* targets, const int32_t* in_len,
                     const int32_t* tgt_len, int B, int T, int V, int Smax, int blank, const float* nll, const float* gscale,
                     void* grad, int64_t ldg, void* workspace, void* stream);

/* ---- Transducer head (recipe keys `Tjoint`, `transducer_lin`, `transducer_cost`: Transducer_joint(joint="sum"), a Linear to the
 * vocabulary and speechbrain.nnet.losses.transducer_loss).  Lattice rows are (b, t, u), u fastest: row = (b T + t) U1 + u, U1 = U + 1;
 * targets int32 (B, U) padded; in_len / tgt_len int32 (B) absolute lengths, clamped to [1, T] / [0, U].  No host synchronisation. ----
 * joint:      H[b,t,u,:] = act(enc[b,t,:] + dec[b,u,:]); enc (B, T, J), dec (B, U1, J), H (B, T, U1, J), contiguous, J %% 4 == 0.
 *             bwd: d_enc = sum_u dH act'(.), d_dec = sum_t dH act'(.) (fixed order: t-block partials in `workspace`).
 * row_stats:  per row of the logits (B T U1 rows of V): lse, lpb = z[blank] - lse, lpy = z[y] - lse (y = targets[b,u], 0 for u = U).
 * loss_fwd:   nll[b] = -log P(y_b | x_b) (fp32); the recursion runs in fp64: alpha = B T U1 + B doubles (the forward variables,
 *             then -log P in fp64), kept for the backward.  U1 <= 2048.
 * loss_bwd:   gb / gy (B T U1 floats) = gscale[b] * d nll / d lpb, d nll / d lpy; exactly 0 outside t < Tb, u <= Ub.
 * logit_grad: dz[n,v] = [v = blank] gb + [v = y] gy - softmax(z)[v] (gb + gy).
 * fused GEMM (smx_transducer_fused_ok: J %% 64 == 0, V %% 4 == 0): z = H W^T + bias (W (V, J) in H's dtype, bias fp32 or null) is
 *   never stored.  gemm_stats: lse / lpb / lpy from per-(row, 128-column tile) partials (smx_transducer_stats_workspace bytes);
 *   gemm_grad: dz (nrows, V; leading dimension lddz %% 4 == 0) of lattice rows [row0, row0 + nrows), recomputed tile by tile,
 *   stored once in H's dtype (columns >= V untouched). */
int smx_transducer_joint_fwd(int dtype, const void* enc, const void* dec, void* H, int B, int T, int U1, int J, int act, void* stream);
size_t smx_transducer_joint_bwd_workspace(int B, int T, int U1, int J);
int smx_transducer_joint_bwd(int dtype, const void* dH, const void* enc, const void* dec, void* d_enc, void* d_dec, int B, int T, int U1,
                             int J, int act, void* workspace, void* stream);
int smx_transducer_row_stats(int dtype, const void* logits, int64_t ld, const int32_t* targets, int B, int T, int U1, int V, int blank,
                             float* lse, float* lpb, float* lpy, void* stream);
int smx_transducer_loss_fwd(const float* lpb, const float* lpy, const int32_t* in_len, const int32_t* tgt_len, int B, int T, int U1,
                            double* alpha, float* nll, void* stream);
int smx_transducer_loss_bwd(const float* lpb, const float* lpy, const double* alpha, const float* gscale,
                            const int32_t* in_len, const int32_t* tgt_len, int B, int T, int U1, float* gb, float* gy, void* stream);
int smx_transducer_logit_grad(int dtype, const void* logits, int64_t ld, const int32_t* targets, const float* lse, const float* gb,
                              const float* gy, int B, int T, int U1, int V, int blank, void* dz, int64_t lddz, void* stream);
int smx_transducer_fused_ok(int dtype, int J, int V);
size_t smx_transducer_stats_workspace(int rows, int V);
int smx_transducer_gemm_stats(int dtype, const void* H, const void* W, const float* bias, const int32_t* targets, int B, int T, int U1,
                              int J, int V, int blank, float* lse, float* lpb, float* lpy, void* workspace, void* stream);
int smx_transducer_gemm_grad(int dtype, const void* H, const void* W, const float* bias, const int32_t* targets, const float* lse,
                             const float* gb, const float* gy, int B, int T, int U1, int J, int V, int blank, int row0, int nrows,
                             void* dz, int64_t lddz, void* stream);

/* ---- Transducer prediction network (recipe keys `emb`, `dec`, recipes/LibriSpeech/ASR/transducer/hparams/
 * conformer_summarymixing_transducer.yaml:301-310: speechbrain.nnet.embedding.Embedding(consider_as_one_hot) and
 * speechbrain.nnet.RNN.LSTM, one layer, unidirectional, batch first; neither source is part of the reference tree - the yardstick is
 * torch.nn.LSTM).  Gate order i, f, g, o (torch's); G = 4 H gate columns.  Supported H: multiples of 32 in [32, 4096]
 * (smx_lstm_ok; SMX_EUNSUPPORTED otherwise); B is free (rows are padded to the 16-row MFMA tile inside the kernels).
 * One launch per time step on `stream`, nothing else: a captured call is a plain chain.  No atomics: bit-reproducible.
 * lstm_fwd:  gates_u = Gx[b,u,:] + h_{u-1} W_hh^T; c_u = f c_{u-1} + i g; h_u = o tanh(c_u).  Gx (B, U, G) fp32 = the input
 *            contribution with BOTH biases folded in (the dense route: smx_gemm with SMX_OUT_F32; the one-hot route:
 *            smx_onehot_gates_fwd).  W_hh (G, H), h0 (B, H) or null, Y (B, U, H), hn (B, H): dtype; c0 (B, H) or null, cn (B, H):
 *            fp32 - the cell state and the gate pre-activations never leave fp32, h is rounded to dtype where it is stored.
 *            For a backward: Hprev (B, U, H) dtype <- h_{u-1} per step (the operand of the dW_hh product), gates (B, U, G) fp32 <-
 *            the ACTIVATED gates, C (B, U, H) fp32 <- c_u; all three null for inference.  U = 1 with h0 / c0 is the decoding step.
 * lstm_bwd:  BPTT from dY (B, U, H) dtype or null, dhn / dcn (B, H) fp32 or null.  W_hh^T (H, G) dtype.  -> dG (B, U, G) dtype (the
 *            gradient of the gate pre-activations: dW_hh += dG^T Hprev, db += colsum dG, dX = dG W_ih through the ordinary GEMM
 *            routes), dh0 and dc0 (B, H) fp32.
 * onehot_rows: Y (rows, V - 1) = the one-hot rows of the int32 tokens with the blank's column removed: column col(k) = k below the
 *            blank, k - 1 above it; the blank (and any token outside [0, V)) gives a zero row.
 * onehot_gates_fwd: Gx[r,:] = keep[r] WihT[col(token[r]),:] + bias; WihT (V - 1, G) = W_ih^T in dtype, bias (G) fp32 = b_ih + b_hh,
 *            keep (rows) fp32 per-token factors (0 or 1/(1-p)) or null.  No one-hot tensor is written.
 * onehot_gates_wgrad: dW_ih (G, V - 1; fp32, leading dimension lddw) [:, col(token[r])] += keep[r] dG[r,:], the rows of one token
 *            summed in ascending order by the workgroup of its first row.  G %% 4 == 0. */
int smx_lstm_ok(int dtype, int H);
int smx_lstm_fwd(int dtype, const float* Gx, const void* Whh, const void* h0, const float* c0, void* Y, void* Hprev, float* gates,
                 float* C, void* hn, float* cn, int B, int U, int H, void* stream);
int smx_lstm_bwd(int dtype, const void* dY, const float* dhn, const float* dcn, const void* WhhT, const float* gates, const float* C,
                 const float* c0, void* dG, float* dc0, float* dh0, int B, int U, int H, void* stream);
int smx_onehot_rows(int dtype, const int32_t* tokens, void* Y, int64_t ldy, int rows, int V, int blank, void* stream);
int smx_onehot_gates_fwd(int dtype, const int32_t* tokens, const float* keep, const void* WihT, int64_t ldw, const float* bias, float* Gx,
                         int rows, int V, int blank, int G, void* stream);
int smx_onehot_gates_wgrad(int dtype, const int32_t* tokens, const float* keep, const void* dG, int64_t lddg, float* dWih, int64_t lddw,
                           int rows, int V, int blank, int G, void* stream);

/* ---- Greedy transducer decoding (recipe key `Greedysearcher`, recipes/LibriSpeech/ASR/transducer/hparams/
 * conformer_summarymixing_transducer.yaml:375-381: speechbrain.decoders.transducer.TransducerBeamSearcher with beam_size 1; its source
 * is not part of the reference tree - the semantics below are SpeechBrain's transducer_greedy_decode written from memory, the
 * yardstick is a float64 restatement of them).  At most one symbol per frame.  Per row b and frame t:
 *   a = act(enc[b,t,:] + pdec[b,:]) (fp32, rounded to dtype);  z = a W_lin^T + b_lin (fp32, never stored);  k = argmax z, the lowest
 *   index on a tie;  k != blank: append k, logp += z[k] - logsumexp(z), one LSTM step on token k (the W_ih^T row gather of
 *   smx_onehot_gates_fwd; c fp32, h rounded to dtype) and pdec = h W_proj^T;  k == blank: the row's state is untouched.
 * Supported (smx_greedy_ok; SMX_EUNSUPPORTED otherwise): H as smx_lstm_ok, J a multiple of 64 in [64, 832], V >= 2; B is free.
 * Three launches per frame on `stream`, the same three whatever the data (logit partials per 128-column tile; select + masked LSTM
 * step; pdec), plus one that clears the outputs: no host synchronisation, no copy to the host, no atomics - a captured call is a
 * plain chain, values are bit-reproducible, and a row's values do not depend on B or on the other rows.
 * State per row: h (B, H) dtype, c (B, H) fp32, pdec (B, J) dtype, frames_seen (B) int32.  Decoding enc[:, :T1] and then
 * enc[:, T1:] on the same state equals decoding enc in one call, bit for bit.
 * greedy_start:  the state before the first frame: one LSTM step from h = c = 0 on the blank (the embedding's zero row: the gates
 *            are `bias` alone), pdec = h W_proj^T, frames_seen = 0.
 * greedy_decode: enc[b,t,:] at enc + b ld_b + t ld_t elements (both strides multiples of 16 bytes); in_len (B) int32: the frames
 *            of THIS call's enc that count per row (frames at or beyond it emit nothing and leave the row's state alone), or null:
 *            all T.  WihT (V - 1, 4H; leading dimension ldw) and bias (4H) fp32 = b_ih + b_hh exactly as smx_onehot_gates_fwd takes
 *            them; Whh (4H, H), Wproj (J, H), Wlin (V, J): dtype; blin (V) fp32 or null.  h_alt (B, H) dtype: the other half of h's
 *            double buffer (workgroups read h while others write the frame's new h), caller-owned, contents undefined on return;
 *            the final state is always in h.  Outputs: tokens (B, T) int32 padded with -1, frames (B, T) int32 (the row's frame
 *            count at each emission, counted from greedy_start across calls; padded with -1), n_tok (B) int32, logp (B) fp32 - ADDED
 *            into, so a stream keeps its running score.  workspace: smx_greedy_workspace(B, V) bytes, 16-byte aligned. */
int smx_greedy_ok(int dtype, int H, int J, int V);
size_t smx_greedy_workspace(int B, int V);
int smx_greedy_start(int dtype, const float* bias, const void* Wproj, void* h, float* c, void* pdec, int32_t* frames_seen, int B, int H,
                     int J, void* stream);
int smx_greedy_decode(int dtype, const void* enc, int64_t ld_b, int64_t ld_t, const int32_t* in_len, const void* WihT, int64_t ldw,
                      const float* bias, const void* Whh, const void* Wproj, const void* Wlin, const float* blin, void* h, void* h_alt,
                      float* c, void* pdec, int32_t* frames_seen, int32_t* tokens, int32_t* frames, int32_t* n_tok, float* logp, int B,
                      int T, int H, int J, int V, int act, int blank, void* workspace, void* stream);

/* ---- RNN language model (recipe key `lm_model`, recipes/LibriSpeech/ASR/transducer/hparams/
 * conformer_summarymixing_transducer.yaml:340-349: speechbrain.lobes.models.RNNLM.RNNLM - a trainable Embedding table, a two-layer
 * speechbrain.nnet.RNN.LSTM of 2048 units, one DNN block and an output Linear; none of these sources is part of the reference tree -
 * the yardstick is torch.nn.Embedding / torch.nn.LSTM).  The decode step (U = 1, a few dozen rows, the state fed back) streams every
 * LSTM weight once, so it is ONE launch per layer whose grid runs over hidden units only:
 * lstm_step: gates[b,:] = bias + x_b W_ih^T + h[b,:] W_hh^T (fp32 sums, gate order i, f, g, o); c'[b] = f c[b] + i g; h'[b] = o tanh(c').
 *            W_ih (4H, I) and W_hh (4H, H) in dtype exactly as torch.nn.LSTM stores them (no transposed image), bias (4H) fp32 =
 *            b_ih + b_hh.  tok == null: x_b = row b of the dense X (B, I; leading dimension ldx, dtype).  tok (B) int32: X is a
 *            (V, I; ldx) table in dtype and x_b = X[tok[b], :] AS STORED (a padding row is not special); a token outside [0, V) reads
 *            as a zero row (smx_onehot_rows' convention).  h (B, H) dtype and c (B, H) fp32: the incoming state, each null = zeros;
 *            h' (B, H) dtype and c' (B, H) fp32 are DISTINCT buffers (other workgroups read h, c and X while h', c' are written):
 *            SMX_EINVAL if they overlap the inputs.  Supported (smx_lstm_step_ok; SMX_EUNSUPPORTED otherwise): H as smx_lstm_ok, I a
 *            multiple of 32 in [32, 4096], ldx a multiple of 8, 16-byte aligned X / W_ih / W_hh / h; B is free: the 16-row batch
 *            tiles are looped inside the workgroup that holds a 32-row weight tile (8 units x 4 gates), so no weight element is
 *            fetched by two workgroups whatever B is, and H = 2048 launches 256 workgroups.  One launch on `stream`, nothing else (a
 *            captured step is a plain chain); no atomics, every sum in a fixed order: bit-reproducible, and a row's values do not
 *            depend on B or on the other rows.
 * gather_rows: Y[r,:] = table[tok[r],:] in dtype (rows x D; table (V, D); leading dimensions ldt, ldy), zeros for a token outside
 *            [0, V).  D, ldt and ldy multiples of 8 elements, 16-byte aligned bases. */
int smx_lstm_step_ok(int dtype, int I, int H);
int smx_lstm_step(int dtype, const void* X, int64_t ldx, const int32_t* tok, int V, const void* Wih, const void* Whh, const float* bias,
                  const void* h, const float* c, void* h_out, float* c_out, int B, int I, int H, void* stream);
int smx_gather_rows(int dtype, const int32_t* tok, const void* table, int64_t ldt, void* Y, int64_t ldy, int rows, int V, int D,
                    void* stream);

/* ---- Split-K over WORKGROUPS for the long reductions of a small batch (round 6; the recipe's 10 x 375 frames) -------------------
 * smx_gemm_panel_slabs: slab[s] (N x M, float32) = A[:, s K : (s + 1) K] . W_s^T for s < nslice on the panel-resident kernel
 *   (A (N, nslice K) bf16; Wpacked = nslice consecutive smx_weight_pack images, image s = the weight's K-slice s, packed WITHOUT a bias;
 *   K = 256 or 512 per slice, M %% 64 == 0, M <= 512).  slabs: nslice * N * M floats, caller-owned.
 * smx_slab_epilogue: C = epilogue(sum_s slab[s]) with the slabs added in a fixed order (bit-reproducible, no atomics) and the
 *   smx_gemm epilogue fields bias, act (+ z saved), drop_*, alpha, row_mask, res (SMX_IO_RES_F32), out_mode (SMX_OUT_T / SMX_OUT_F32)
 *   and SMX_EPI_LN_FWD (lnf_*, SMX_IO_LNFY_F32, lnf2_*) - the LayerNorm(s) that follow the Linear (Conformer.py:458-476,507,530-536)
 *   run on the row in registers: one launch instead of GEMM epilogue + standalone LayerNorm.  Other fields: SMX_EUNSUPPORTED. */
int smx_gemm_panel_slabs_ok(int dtype, int N, int M, int K, int nslice);
int smx_gemm_panel_slabs(int dtype, const void* A, int64_t lda, const void* Wpacked, float* slabs, int N, int M, int K, int nslice,
                         void* stream);
int smx_slab_epilogue_ok(int dtype, int N, int M, int nslab);
int smx_slab_epilogue(int dtype, const float* slabs, int nslab, int64_t slab_stride, void* C, int64_t ldc, int N, int M,
                      const smx_epilogue* epi, void* stream);

/* ---- Sequence-parallel shards (summarymixing_amd/sequence_parallel.py): the boundary arithmetic of the two O(T) summaries inside the
 * kernels (round 6; it ran as float32 elementwise passes over the activations on the host side before).
 * smx_chunk_mean_sharded: the shard holds the whole chunks [c_off, c_off + T / chunk).  phase 1: chunk sums into `workspace`
 *   ((B, T / chunk, D) float32; reverse: scaled by 1 / the GLOBAL window length; left < 0: running sums) - rows of it are what the
 *   shards exchange.  phase 2: window combine + carry[b][c - carry_c0] for carry_c0 <= c < carry_c0 + carry_n (carry_n == 0: one
 *   (B, D) row for every chunk), forward divided by the GLOBAL window length.
 * smx_expdecay_mean_sharded: frames [t_off, t_off + T) of T_glob.  phase 1: ends (2, B, D) <- the states leaving the shard; phase 2:
 *   ends = the states ENTERING it (folded by the caller from the gathered ones), out = the operator with global denominators.
 *   The `ends` contract, both phases: states at TRUE frames - ends[0] is f at the shard's last frame (phase 1) / at the frame before
 *   its first (phase 2), ends[1] is g at the shard's first frame (phase 1) / at the frame after its last (phase 2).  The scan's zero
 *   padding of the shard's last 16-row chunk is never visible to the caller: the library compensates it in both directions
 *   (decay^-pad, pad < 16: finite in float32 for decay >= ~0.01), so the caller's fold is decay^T per shard for any T. */
int smx_chunk_mean_sharded(int dtype, const void* X, int64_t ldx, void* out, int64_t ldo, int B, int T, int D, int chunk, int left,
                           int reverse, int c_off, int phase, const float* carry, int carry_c0, int carry_n, void* workspace, void* stream);
int smx_expdecay_mean_sharded(int dtype, const void* S, int64_t lds, void* out, int64_t ldo, int B, int T, int D, float decay, int mode,
                              int t_off, int T_glob, int phase, float* ends, void* workspace, void* stream);

/* Device step counter (one uint64 in device memory) - an explicit ARGUMENT of every call that uses it, never library
 * state: `epoch` of smx_dropout / smx_masked_mean_bwd(_act) / smx_act_mask_bwd / smx_layernorm_bwd (dX2) /
 * smx_dwconv_args.epoch, smx_epilogue.epoch of the GEMMs, `step_dev` of smx_adamw_step.  With a non-NULL counter a
 * fused / standalone dropout mixes the counter's current value into its seed and smx_adamw_step with step <= 0 takes its
 * bias-correction step from it: a whole training step can then be captured ONCE in a hipGraph (all kernel arguments
 * constant) and replayed - masks and bias correction still advance, because the counter does (smx_step_counter_add is
 * itself a captured kernel).  NULL = the plain by-value behaviour.  The library holds no process-global state besides
 * the read-once smx_config and the per-thread error string. */
int smx_step_counter_add(uint64_t* dev_counter, uint64_t inc, void* stream);
/* id[0] = the id of the hipGraph capture `stream` is recording into (hipStreamGetCaptureInfo), 0 when it is not capturing.  Host
 * bookkeeping only (no launch): the host side stamps cached packed weight images (smx_weight_pack) with it, so that EVERY capture
 * contains its own pack launches and the first eager call after a capture re-packs (round-5 advisor finding). */
int smx_stream_capture_id(void* stream, uint64_t* id);
/* out[0] += sum(x^2) — global grad-norm for clipping (zero out[0] first).  Fixed summation order (per-block partials in
 * `workspace`, smx_sumsq_workspace() bytes, folded by one block; no atomics): data-parallel ranks holding the same
 * all-reduced gradients get bit-identical norms, clip factors and weights. */
size_t smx_sumsq_workspace(void);
int smx_sumsq(const float* x, int64_t n, float* out, void* workspace, void* stream);
/* out[0] = min(1, max_norm / (sqrt(sumsq[0]) * inv_scale + 1e-6)) : clip factor computed on device.  `out` is fp32[2]:
 * when sumsq[0] is NaN / Inf (a bad batch: bf16 overflow, a zero-length utterance) out[0] = 0 and out[1] += 1 (skipped-step
 * counter); smx_adamw_step treats a device factor of exactly 0 as "skip the update" (no decay, no moments, no shadow
 * refresh) - the behaviour of SpeechBrain's Brain.check_gradients for non-finite gradients. */
int smx_clip_factor(const float* sumsq, float max_norm, float inv_scale, float* out, void* stream);

/* ---- Streaming inference (chunk by chunk) of a Dynamic-Chunk-trained Conformer encoder ---------------------------------------
 * The full-utterance DynChunk forward (TransformerASR.py:85-110 summary mask, Conformer.py:190-313 convolution) computed one chunk
 * of C_cur <= C frames per stream at a time, for B equal-length streams.  `counter` is a device step counter (uint64, the
 * smx_step_counter_add convention) holding the index c of the chunk being run; no chunk index is passed by value, so a captured
 * chunk step stays valid on replay.  smx_stream_advance ends a step.  All state buffers are caller-owned and zero-initialised.
 * smx_stream_summary: S (B*C_cur, D) rows of the summary branch (summary_mixing.py:224-235).  out[b, t, :] = (sum of S over the
 *   window of chunk c) / (frames in the window), the window being the chunks [c - left, c] (left = -1: all of [0, c]) and the frame
 *   count min(c, left) * C + C_cur (smx_chunk_mean_fwd's denominator), broadcast to all C_cur rows of stream b.  The chunk's
 *   float32 sums go into the state: ring (B, left, D) float32, slot c % left (left = -1: ring (B, D) is a running sum; left = 0:
 *   ring unused, may be NULL).  Fixed summation order, no atomics.  dtype F32 | BF16, D % 8 == 0, 1 <= C_cur <= C <= 64,
 *   -1 <= left <= 32.
 * smx_dwconv1d_glu_stream: smx_dwconv_fwd's u / Y (glu = 1, zero padding, bias) over one chunk with Dynamic Chunk Convolution.
 *   P (B*C_cur, 2D) pre-GLU rows of the chunk; state (B, H, 2D), H = (k-1)/2, contiguous, compute dtype: the last H pre-GLU rows
 *   before the chunk (zeros before the first: the full forward's zero padding at t < 0).  Y[b, t] reads X = [state; chunk] at
 *   t .. t + k - 1, zero at and beyond the chunk's end.  The state is rewritten IN PLACE with the last H rows of [state; chunk]
 *   (also when C_cur < H): one workgroup owns all H + C_cur rows of its (stream, 64-channel group) and reads them all before it
 *   writes any.  P and Y must not overlap the state.  dtype F32 | BF16, D % 8 == 0, odd k <= 63, 1 <= C_cur <= 64.
 * smx_stream_advance: counter += 1, then pe[r, :] = table[counter * C + r, :] for r < C (zero at and beyond `rows`), one launch:
 *   the next chunk's rows of the positional table (TransformerASR.py:547-549) in a fixed (C, D) buffer. */
int smx_stream_summary(int dtype, const void* S, int64_t lds, void* out, int64_t ldo, float* ring, const uint64_t* counter, int B,
                       int C_cur, int C, int D, int left, void* stream);
int smx_dwconv1d_glu_stream(int dtype, const void* P, int64_t ldp, const float* w, const float* bias, void* state, void* Y,
                            int64_t ldy, int B, int C_cur, int D, int k, void* stream);
int smx_stream_advance(int dtype, uint64_t* counter, const void* table, int64_t ldt, int rows, void* pe, int64_t ldpe, int C, int D,
                       void* stream);

/* ---- Slot streaming: B independent streams, one per batch slot, in one fixed step of B x C rows --------------------------------
 * The lockstep calls above with per-slot state: smx_slot_summary and smx_dwconv1d_glu_slots run the SAME kernel bodies as
 * smx_stream_summary and smx_dwconv1d_glu_stream (a second instantiation, not a copy), which differ only in who holds which rows,
 * where the chunk index comes from and the fresh-state rule below.  Row t of slot b is row b * C + t of every (B*C, .) operand.  counters (B,) int64
 * holds each slot's chunk index c (shared by all layers); counter 0 means fresh state: chunk 0 reads no ring slot, no running sum
 * and no convolution state, so a slot starts a new stream by counters[b] = 0 alone (smx_slot_begin) and no state buffer is
 * cleared.  valid (B,) int32 holds the frames of slot b in this step, 0 .. C: C = a full chunk, 1 .. C-1 = the stream's last,
 * 0 = the slot sits out (nothing of it is read or written, its state is untouched).  Rows at and beyond valid[b] are never loaded
 * (they may hold NaN), and output rows at and beyond valid[b] are not written.  counters / valid / start are device arrays, so a
 * captured step stays valid on replay.  A step is smx_slot_begin, the layers, smx_slot_advance.
 * smx_slot_summary: smx_stream_summary per slot: window of chunk counters[b], frame count min(c, left) * C + valid[b]; for left = -1
 *   the running sum is written, not added to, at chunk 0.  One body, so one fixed summation order: a full chunk gives the bits of
 *   smx_stream_summary on the same inputs.  dtype F32 | BF16, D % 8 == 0, 1 <= C <= 64, -1 <= left <= 32, B <= 65535.
 * smx_dwconv1d_glu_slots: smx_dwconv1d_glu_stream per slot with C_cur = valid[b]: the state (B, H, 2D) reads as zero at chunk 0, and
 *   is rewritten in place with the last H rows of [state; chunk[:valid[b]]] (not at all for valid[b] == 0).  dtype F32 | BF16,
 *   D % 8 == 0, odd k <= 63, 1 <= C <= 64, B <= 65535.
 * smx_slot_begin: the first launch of a step.  counters[b] = 0 where start[b] (uint8 (B,)), then pe[b * C + r, :] =
 *   table[counters[b] * C + r, :] for r < C (zero at and beyond `rows`): each slot's rows of the positional table in a fixed (B*C, D)
 *   buffer.  pe = NULL: counters only (table unused).  Grid (C, B), no per-element division.
 * smx_slot_advance: the last launch of a step.  counters[b] += (valid[b] == C): a sat-out slot or a closing last chunk does not
 *   advance. */
int smx_slot_summary(int dtype, const void* S, int64_t lds, void* out, int64_t ldo, float* ring, const int64_t* counters,
                     const int32_t* valid, int B, int C, int D, int left, void* stream);
int smx_dwconv1d_glu_slots(int dtype, const void* P, int64_t ldp, const float* w, const float* bias, void* state, void* Y,
                           int64_t ldy, const int32_t* valid, const int64_t* counters, int B, int C, int D, int k, void* stream);
int smx_slot_begin(int dtype, int64_t* counters, const uint8_t* start, const void* table, int64_t ldt, int rows, void* pe,
                   int64_t ldpe, int B, int C, int D, void* stream);
int smx_slot_advance(int64_t* counters, const int32_t* valid, int B, int C, void* stream);

/* ---- Feature augmentation: the recipes' fea_augment (…/transducer/hparams/conformer_summarymixing_transducer.yaml:195-245) ------
 * speechbrain.augment.freq_domain.SpectrogramDrop along time (dim 1), SpectrogramDrop along frequency (dim 2) and Warping (bicubic)
 * on x (B, T, F), in that order, as one draw launch and one apply launch.  The draws live in an int32 PARAMETER BLOCK on the device:
 *   [0] flags: SMX_SPECAUG_WARP | SMX_SPECAUG_TIME | SMX_SPECAUG_FREQ (a clear bit: that stage is the identity)
 *   [1] c   [2] w     the warp: output rows [0, w) resample source rows [0, c), output rows [w, T) resample source rows [c, T)
 *   [3] n_time   [4] n_freq     drops per row in force, one value for the whole batch (clamped to the caps)
 *   [5..7] reserved (0)
 *   then (pos, len)[B][n_time_cap]: row b drops the frames pos <= t < pos + len of its first n_time pairs (clipped at T)
 *   then (pos, len)[B][n_freq_cap]: likewise along F
 * A cap is a stage's drop_count_high (0 for an absent stage), at most 32.  smx_specaug_params_bytes: the block's size (0 for
 * arguments out of range).
 * smx_specaug_draw fills a block and writes nothing else: n uniform on [cnt_lo, cnt_hi], len on [len_lo, len_hi), pos on [0, T) or
 *   [0, F); with T - window > window, c uniform on [window, T - window) and w on [c - window + 1, c + window], otherwise the warp
 *   bit stays clear.  `stages`: the flag bits to draw for; the caps of the block are t_cnt_hi / f_cnt_hi of the stages present.
 *   Every value is one 32-bit hash of (seed, *epoch, which value, index) - the counter-based generator of the dropout masks with a
 *   salt of its own - scaled as (h * range) >> 32: no host synchronisation, no atomics, and a captured draw advances with the
 *   device step counter `epoch` (NULL: by value, see smx_step_counter_add).
 * smx_specaug_apply: Y = the three stages applied to X, a pure function of X and the block.  X, Y: (B * T) rows of F elements with
 *   leading dimensions ldx, ldy.  Each output row gathers at most four source rows (torch's bicubic, align_corners = True: position
 *   num / den with num = t * (n_in - 1), den = n_out - 1 in integer arithmetic, taps clamped into the segment, A = -0.75);
 *   a tap dropped along time contributes nothing and is not loaded, so the warp interpolates across the zeroed frames exactly as
 *   the sequential chain does; dropped columns are +0.  float32 accumulation, one rounding.  A row whose position falls on a
 *   source row - every row when the warp bit is clear - is copied bit for bit.  16-byte accesses when F, ldx, ldy are multiples of
 *   4 (F32) / 8 (BF16) and X, Y are 16-byte aligned, element accesses otherwise.  SMX_EUNSUPPORTED: F > 1024, a cap > 32, X == Y,
 *   B > 65535. */
enum { SMX_SPECAUG_WARP = 1, SMX_SPECAUG_TIME = 2, SMX_SPECAUG_FREQ = 4 };
size_t smx_specaug_params_bytes(int B, int n_time_cap, int n_freq_cap);
int smx_specaug_draw(int32_t* params, int B, int T, int F, int stages, int t_len_lo, int t_len_hi, int t_cnt_lo, int t_cnt_hi,
                     int f_len_lo, int f_len_hi, int f_cnt_lo, int f_cnt_hi, int warp_window, uint64_t seed, const uint64_t* epoch,
                     void* stream);
int smx_specaug_apply(int dtype, const void* X, int64_t ldx, void* Y, int64_t ldy, const int32_t* params, int B, int T, int F,
                      int n_time_cap, int n_freq_cap, void* stream);

/* ---- Waveform augmentation: the recipes' wav_augment (…/transducer/hparams/conformer_summarymixing_transducer.yaml:177-192) -----
 * speechbrain.augment.time_domain.SpeedPerturb (speed_perturb, yaml:177-179: orig_freq 16000, speeds [95, 100, 105]) resamples the
 * batch with speechbrain's Resample = torchaudio's polyphase windowed-sinc filter at its defaults (sinc_interp_hann,
 * lowpass_filter_width 6, rolloff 0.99); the Augmenter around it (wav_augment, yaml:181-192) applies that one stage to every batch.
 * With g = gcd(orig_freq, new_freq), o = orig_freq / g, n = new_freq / g, base = min(o, n) * 0.99, width = ceil(6 * o / base) and
 * K = 2 * width + o, phase p in [0, n) has the taps
 *   h[p][k] = sinc(pi t) cos^2(pi t / 12) base / o,  t = clamp(((k - width) / o - p / n) base, -6, 6),  k in [0, K),
 * evaluated in float64 and rounded to float32, and row x[0, L) (zero outside) gives L_out = ceil(n L / o) outputs
 *   y[q n + p] = sum_k h[p][k] x[q o + k - width].
 * The nonzero float32 taps of a phase are one contiguous run; `taps` is the longest run of the plan.
 * smx_resample_plan (host only, touches no GPU; yaml:177-179 fixes the three ratios a recipe needs) fills info[8] =
 *   {o, n, width, K, taps, Q, 0, 0} (Q: whole n-sample output blocks per workgroup tile), *image_bytes (may be NULL) and, when `image`
 *   is not NULL, the PLAN IMAGE of image_bytes bytes (SMX_EINVAL if image_capacity is smaller): int32 info[8], int32 first[n] (index
 *   k of the first nonzero tap of phase p), float32 w[n][taps] (w[p][j] = h[p][first[p] + j], zero behind the run).
 *   SMX_EUNSUPPORTED: a rate <= 0; n * taps > 8192 floats (the table lives in LDS; more than 1024 phases are refused before any tap
 *   is evaluated); K + taps + o + 3 > 4096 samples (one block's input does not fit a workgroup's span).
 * smx_resample (yaml:181-192, the pass wav_augment makes): Y[b][0, L_out) = the resampled X[b][0, L) for b < B, float32, `plan` the
 *   image on the device; writes exactly those elements (ldy >= L_out is the caller's to guarantee: o and n live on the device).
 *   One launch, no allocation, no host synchronisation.  Each output is summed in ascending k with one float32 fused multiply-add
 *   per tap of the run, so two runs agree bit for bit and a unit impulse returns the taps themselves.  16-byte loads when X is
 *   16-byte aligned and ldx % 4 == 0, 16-byte stores when Y is and ldy % 4 == 0, element accesses otherwise (same bits).  No
 *   length masking: the padded tail of a row is resampled like any other sample.  SMX_EINVAL: L < 1, ldx < L;
 *   SMX_EUNSUPPORTED: X == Y, B > 65535.  A block that is not a plan image writes nothing. */
int smx_resample_plan(int orig_freq, int new_freq, int32_t* info, size_t* image_bytes, void* image, size_t image_capacity);
int smx_resample(const float* X, int64_t ldx, float* Y, int64_t ldy, const int32_t* plan, int B, int64_t L, void* stream);

/* ---- Label-smoothed sequence losses and accuracy: the recipes' second loss head ------------------------------------------------
 * speechbrain.nnet.losses.kldiv_loss (`seq_cost` with `label_smoothing`, reduction batchmean:
 * …/LibriSpeech/ASR/transformer/hparams/branchformer_summarymixing.yaml:278-280, and the AISHELL-1 / CommonVoice Branchformer recipes;
 * V = 5000 / 5000 / 1000), speechbrain.nnet.losses.nll_loss (`ce_cost`, label_smoothing 0.1, the cross-entropy multitask head over
 * the prediction network: …/LibriSpeech/ASR/transducer/hparams/conformer_summarymixing_transducer.yaml:319-320) and
 * speechbrain.utils.Accuracy.AccuracyStats (`acc_computer`, the Branchformer recipes' validation).
 * X: (B, U) rows of V elements (F32 or BF16), row (b, u) at X + b * bsx + u * ldx (a truncated view keeps its strides); targets int32,
 * token (b, u) at targets[b * ldt + u].  One target distribution serves both losses: q[v] = off (v != y), q[y] = conf, and
 *   row loss = cst - conf * lp[y] - off * (sum_v lp[v] - lp[y])
 *   nll_loss, smoothing e:  conf = (1 - e) + e / V, off = e / V,       cst = 0
 *   kldiv_loss, 0 < e < 1:  conf = 1 - e,           off = e / (V - 1), cst = conf log conf + (V - 1) off log off
 * With off == 0 the row sum does not enter (a -inf away from y leaves the loss finite).
 * keep[b, u] = (len == NULL || u < len[b]) && (pad_idx < 0 || y != pad_idx); len int32 (B) on the device.  A dropped row is not read.
 * smx_seqloss_fwd, from_logits = 0: X holds log-probabilities.  from_logits = 1: X holds raw logits; the one read of the row carries
 *   an online (max, sum exp), lse = max + log sum, lp[v] = X[v] - lse, sum lp = sum X - V lse, and lse (B * U, 2) receives the fp32
 *   value and the fp32 residual of the fp64 one (the backward's exp(z - lse) needs both once the logits are large).
 *   Outputs: row_loss (B * U) fp32 (0 for a dropped row), row_flags (B * U) int32 (bit 0 kept, bit 1 the row's argmax - first index
 *   among equal entries - is the target), and, from a second launch that folds each utterance in a fixed order (no atomics: two runs
 *   agree bit for bit), utt_loss (B) fp32 = the sum over kept rows, utt_kept (B), utt_hits (B, may be NULL) int32.
 *   A target outside [0, V) on a kept row indexes nothing: its row loss is NaN and it counts as kept and not hit.
 *   fp32 / fp64 arithmetic, the final combination in fp64 rounded once.
 * smx_seqloss_bwd: g (B * U) fp32 = reduction weight * upstream gradient per row.  dX row r at dX + r * lddx, in the input dtype:
 *   from_logits = 0: -g keep q (X, lse unused);  from_logits = 1: g keep (exp(X - lse) - q), lse as the forward wrote it.
 *   Every element of every row is written: exact zeros for dropped rows, NaN for a kept row with a target outside [0, V).
 * A row is cut into 16-byte groups anchored at its first column plus an element tail; a row whose address is 16-byte aligned moves
 * a group per access (every row at V = 1000 or 5000, dense), any other row moves the same groups element by element: same bits either
 * way.  No host synchronisation, no allocation: capturable.
 * SMX_EINVAL: a NULL pointer, V < 1, ldx < V, ldt < U, NaN or negative off; SMX_EUNSUPPORTED: B * U >= 2^31, pad_idx >= V, X == dX. */
int smx_seqloss_fwd(int dtype, int from_logits, const void* X, int64_t ldx, int64_t bsx, const int32_t* targets, int64_t ldt,
                    const int32_t* len, int B, int U, int V, int pad_idx, float conf, float off, float cst, float* row_loss,
                    float* lse, int32_t* row_flags, float* utt_loss, int32_t* utt_kept, int32_t* utt_hits, void* stream);
int smx_seqloss_bwd(int dtype, int from_logits, const void* X, int64_t ldx, int64_t bsx, const int32_t* targets, int64_t ldt,
                    const int32_t* len, int B, int U, int V, int pad_idx, float conf, float off, const float* lse, const float* g,
                    void* dX, int64_t lddx, void* stream);

/* ---- CTC greedy (best-path) decoding of the encoder's CTC head --------------------------------------------------------------------
 * speechbrain.decoders.ctc.ctc_greedy_decode / filter_ctc_output over the head every recipe trains (`ctc_lin` 512 -> 5000 with
 * `ctc_weight: 0.3` in the Branchformer recipes, `proj_ctc` 640 -> 1000 in the transducer recipes): row arg-max, collapse repeats,
 * drop blanks.  The decoder's source is not part of the reference tree; the semantics below are complete in themselves.
 * No call synchronises with the host or allocates (capturable); nothing is atomic and every sum has a fixed order, so two runs agree
 * bit for bit.  A NaN never wins a comparison, and a token is only ever compared, never used as an index.
 * smx_ctc_best_path: X (N, V) logits or log-probabilities (F32 or BF16), row n at X + n * ldx.  tok[n] int32 = the lowest index of the
 *   row maximum (-1 when no entry of the row is a number), lp[n] fp32 = max - logsumexp(row) = -log sum exp(X - max), the maximum's
 *   log-probability (for log-softmax input the maximum itself, up to rounding); NaN when any entry of the row is a NaN.  One wave per
 *   row, 16-byte loads for a 16-byte aligned row and element loads otherwise (same bits), an element tail of V % (4 | 8) columns.
 *   SMX_EINVAL: a NULL pointer, V < 1, ldx < V.
 * smx_ctc_head_best_path: the same two outputs for z = X W^T + bias, X (N, K) with leading dimension ldx and W (V, K) dense, both in
 *   `dtype`; bias (V) fp32 or NULL.  z is never stored: a 128 x 128 MFMA tile per workgroup (fp32 accumulation; F32 operands sum each
 *   32-element stage on its own) leaves per (row, column tile) the tile's max, first arg-max and sum exp(z - max) in the workspace
 *   (smx_ctc_head_workspace(N, V) bytes, 16-byte aligned), and a second launch folds a row's tiles in ascending order (a tie keeps the
 *   lower column).  Columns at and beyond V count as -inf; rows beyond N re-read row N - 1 and are never stored.
 *   Supported (smx_ctc_head_ok; SMX_EUNSUPPORTED otherwise): K a multiple of 64, V >= 2, X / ldx / W 16-byte aligned.
 * smx_ctc_collapse: one wave per utterance over tok / lp (B, T) (frame (b, t) at [b * ld + t]).  in_len (B) int32: the frames of THIS
 *   call that count per row, clamped to [0, T]; NULL: all T.  start (B) uint8 or NULL: non-zero resets the row's state before the call.
 *   State per row, read and written: prev int32 (the last counted frame's token; INT32_MIN before the first frame, which equals no
 *   token), seen int32 (frames counted so far), n_tok int32 (tokens emitted so far), score fp32.
 *   Frame t < in_len[b] emits iff tok[t] != blank && tok[t] >= 0 && tok[t] != (t == 0 ? prev : tok[t - 1]): `a a` gives `a`,
 *   `a blank a` gives `a a`, a -1 emits nothing and a real token after it does.  Emissions go to tokens / frames (B, cap) int32 at
 *   n_tok[b], n_tok[b] + 1, ... in frame order (frames: seen + t, the index from the start of the stream); one at or beyond cap is
 *   not stored while n_tok keeps counting (n_tok > cap tells the caller).  Entries [n_tok, cap) are set to -1 by every call; entries
 *   below the call's first emission are left alone.  score[b] += lp[b, t] for t < in_len[b] as ONE fp32 chain strictly in frame order -
 *   a fixed tree (the left comb), and the only one for which a stream cut into calls gives the bits of the whole.  in_len[b] == 0
 *   without `start` leaves the row's state as it was.
 *   SMX_EINVAL: a NULL pointer, negative sizes, ld < T, blank < 0. */
typedef struct smx_ctc_collapse_args {
  const int32_t* tok;     /* (B, T) */
  const float* lp;        /* (B, T) */
  int64_t ld;             /* row stride of tok and lp (elements) */
  const int32_t* in_len;  /* (B) or NULL */
  const uint8_t* start;   /* (B) or NULL */
  int32_t* prev;          /* (B) state */
  int32_t* seen;          /* (B) state */
  int32_t* n_tok;         /* (B) state */
  float* score;           /* (B) state */
  int32_t* tokens;        /* (B, cap) */
  int32_t* frames;        /* (B, cap) */
  int32_t B, T, blank, cap;
} smx_ctc_collapse_args;  /* 104 bytes */
int smx_ctc_best_path(int dtype, const void* X, int64_t ldx, int N, int V, int32_t* tok, float* lp, void* stream);
int smx_ctc_head_ok(int dtype, int K, int V);
size_t smx_ctc_head_workspace(int N, int V);
int smx_ctc_head_best_path(int dtype, const void* X, int64_t ldx, const void* W, const float* bias, int N, int K, int V, int32_t* tok,
                           float* lp, void* workspace, void* stream);
int smx_ctc_collapse(const smx_ctc_collapse_args* a, void* stream);

/* ---- scaled-dot-product attention (speechbrain.nnet.attention.MultiheadAttention, `attention_type: regularMHA`) -------------------
 * The arithmetic between the in- and out-projections of the module the reference's TransformerDecoderLayer holds twice
 * (speechbrain/lobes/models/transformer/Transformer.py:745-751 builds `self_attn` and `mutihead_attn`, :811-840 runs them: causal
 * self-attention over the tokens, cross-attention over the encoder output) and TransformerLM is made of.
 * Q (B, L, H, D), K / V (B, S, H, D), O / dO / dQ (B, L, H, D), dK / dV (B, S, H, D): each an smx_attn_operand, element
 * (b, row, h, d) at p[b sb + row sr + h sh + d sd].  sd must be 1 and the base and every stride 16-byte aligned (SMX_EUNSUPPORTED
 * otherwise), so q / k / v may be views into one packed (B, L, 3, H, D) or (B, S, 2, H, D) projection output and dq / dk / dv views
 * into the packed gradient buffer; nothing is copied.  dtype F32 or BF16, D in {64, 128, 256, 512}, B, L, S, H >= 1 with no
 * multiple-of-tile requirement (other dtype / D: SMX_EUNSUPPORTED).
 *   s[b,h,i,j] = scale <q_i, k_j> + attn_bias[i ldbias + j]      attn_bias fp32 (L, S) or NULL, shared by batch and heads, -inf = masked
 *   masked also where causal != 0 and j > i + (S - L), and where key_pad[b ldpad + j] != 0 (uint8 (B, S) or NULL)
 *   p = softmax_j(s), fp32, row maximum subtracted;  p~ = keep ? p / (1 - drop_p) : 0 with the library's counter-based mask at index
 *   ((b H + h) L + i) S + j of (drop_seed, epoch): the mask smx_dropout draws on a (B H L, S) matrix with that seed; off at drop_p == 0
 *   O = p~ V,  lse[(b H + h) L + i] = log sum_j exp(s) (fp32).
 * A row whose keys are all masked: O = 0, lse = -inf, zero gradients, never NaN (a stated deviation: torch yields NaN there).
 * Arithmetic: F32 operands use exact fp32 products (v_mfma_f32_16x16x4_f32), BF16 operands the bf16 MFMA; accumulators, softmax, lse
 * and delta are fp32; for BF16, p~ and dS are rounded to bf16 once, as the operand of the product that follows them.
 * smx_attn_fwd: one launch, online softmax over 64-key tiles, writes o and lse; no (B, H, L, S) tensor exists anywhere.
 * smx_attn_bwd: reads dO, q, k, v, lse, writes dq, dk, dv (every element of every row) and delta (B H L fp32 of workspace).  Two
 *   launches: dQ by query tile, which first sums delta_i = sum_j p~_ij dP_ij - rowsum(dO o) taken from the dP bits the gradients use,
 *   so p (dP - delta) cancels exactly for a row with one visible key; o may be passed and is neither read nor checked - then dK / dV
 *   by key tile.
 *   Probabilities are recomputed from lse, the keep mask from the seed; no atomics, one fixed summation order: two runs agree bit for
 *   bit.  dk / dv rows of padded keys are exact zeros.
 * smx_attn_weights: weights[b w_sb + i ldw + j] = (1 / H) sum_h p~[b,h,i,j] (fp32, heads summed in index order; dropped as the
 *   forward when drop_p > 0, which is what torch returns); reads q, k, lse and the masks; masked entries are exact zeros.
 * smx_attn_plan_query: the geometry of the launch `pass` (SMX_ATTN_PASS_*) for the descriptor's
 *   sizes and dtype; needs no GPU and no pointers (those present are checked).
 * No call synchronises with the host or allocates: capturable.  SMX_EINVAL: a NULL operand the pass needs, sizes < 1, drop_p
 * outside [0, 1), ldbias / ldpad / ldw < S. */
enum { SMX_ATTN_PASS_FWD = 0, SMX_ATTN_PASS_BWD_DQ = 1, SMX_ATTN_PASS_BWD_DKV = 2, SMX_ATTN_PASS_WEIGHTS = 3 };
typedef struct smx_attn_operand {
  void* p;
  int64_t sb, sr, sh, sd; /* element strides: batch, row, head, D (sd must be 1) */
} smx_attn_operand;       /* 40 bytes */
typedef struct smx_attn_args {
  int32_t dtype, causal;
  smx_attn_operand q, k, v, o, dO, dq, dk, dv;
  float* lse;              /* (B, H, L) */
  float* delta;            /* (B, H, L) backward workspace */
  const float* attn_bias;  /* (L, S) or NULL */
  int64_t ldbias;
  const uint8_t* key_pad;  /* (B, S) or NULL */
  int64_t ldpad;
  float* weights;          /* (B, L, S), smx_attn_weights only */
  int64_t w_sb, ldw;
  int32_t B, L, S, H, D;
  float scale, drop_p;
  int32_t pad_;
  uint64_t drop_seed;
  const uint64_t* epoch;   /* device step counter mixed into the seed, or NULL */
} smx_attn_args;           /* 448 bytes */
typedef struct smx_attn_plan {
  int32_t rows;            /* rows of the tile a workgroup owns: queries (pass 0, 1, 3) or keys (pass 2) */
  int32_t key_tile;        /* width of the tile it walks: keys (pass 0, 1, 3) or queries (pass 2) */
  int32_t d_chunk;         /* columns of D staged through LDS at a time */
  int32_t lds_bytes, threads, launches;
  int32_t grid[3];
  int32_t pad_;
} smx_attn_plan;           /* 40 bytes */
int smx_attn_fwd(const smx_attn_args* a, void* stream);
int smx_attn_bwd(const smx_attn_args* a, void* stream);
int smx_attn_weights(const smx_attn_args* a, void* stream);
int smx_attn_plan_query(const smx_attn_args* a, int pass, smx_attn_plan* plan);

/* ---- target embedding of the seq2seq decoder ----------------------------------------------------------------------------------------
 * What TransformerASR.forward / decode do to the tokens before the decoder (speechbrain/lobes/models/transformer/): `custom_tgt_module`
 * = NormalizedEmbedding, emb(tokens) * sqrt(d_model) (Transformer.py:991-1021); `tgt + positional_encoding(tgt)` (TransformerASR.py:430,
 * :486) and get_key_padding_mask(tgt, pad_idx) = tgt.eq(pad_idx) (Transformer.py:1024-1060, called at TransformerASR.py:172): five
 * ATen launches forward and an atomic scatter-add backward.
 * smx_tgt_embed_fwd: for every row r < rows (= B U):  Y[r ldy + c] = table[tok[r] ldt + c] * sqrt(D) + pe[(r %% U) ldpe + c]  in out_dtype
 *   (F32 or BF16; table (V, D) and pe (rows [0, U) of the positional table, D columns) are fp32) and key_pad[r] = (tok[r] == pad_idx)
 *   as uint8, the (B, U) layout smx_attn_* read as `key_pad`.  A token outside [0, V) reads as a zero row (smx_gather_rows'
 *   convention): Y = pe, key_pad = 0; the token is compared before the table is indexed.  One launch, 16-byte loads and stores.
 * smx_tgt_embed_bwd: gTable[v ldg + c] += sqrt(D) * sum_{r : tok[r] == v} dY[r lddy + c]  (dY in dy_dtype, gTable fp32 (V, D), sums
 *   fp32), the rows of each v added in ascending r by the one workgroup that owns v: no atomics, two runs agree bit for bit.  Row
 *   pad_idx receives nothing (upstream's table is nn.Embedding(padding_idx = blank_id = 0)), nor does any token outside [0, V); a row
 *   no token names is not written.  One launch.
 * Both: D and the leading dimensions multiples of 8 elements and 16-byte aligned bases (SMX_EUNSUPPORTED otherwise); SMX_EINVAL for a
 * NULL pointer, rows < 0, U / V / D < 1 or a leading dimension < D.  Nothing synchronises with the host or allocates: capturable. */
int smx_tgt_embed_fwd(int out_dtype, const int32_t* tok, const float* table, int64_t ldt, const float* pe, int64_t ldpe, void* Y,
                      int64_t ldy, uint8_t* key_pad, int rows, int U, int V, int D, int pad_idx, void* stream);
int smx_tgt_embed_bwd(int dy_dtype, const int32_t* tok, const void* dY, int64_t lddy, float* gTable, int64_t ldg, int rows, int V, int D,
                      int pad_idx, void* stream);

/* ---- one KV-cached decoding step of the seq2seq decoder (csrc/attn_step.hip) ----------------------------------------------------------
 * What a greedy / teacher-forced search over [TransformerASR.decode, seq_lin] needs per new token instead of running the whole prefix
 * again.  Every position is a device counter the kernels read and advance, so the host issues identical launches at every step.
 * smx_attn_step: one query row per (batch row, head) over a cache.  q, k_new, v_new, o are (B, H, D) (smx_attn_operand; sr is not
 *   read), K and V the caches (B, cap, H, D); sd must be 1 and the base and every stride read 16-byte aligned (SMX_EUNSUPPORTED
 *   otherwise), so q / k_new / v_new may be views into the packed (B, 3, H, D) in-projection output of the step and K / V the two
 *   halves of a packed (B, cap, 2, H, D) cache.  n_keys (B) int32 ON THE DEVICE: the number of visible keys of row b, n; NULL: cap.
 *   With k_new / v_new (self-attention) the call first stores k_new[b], v_new[b] into cache slot n - 1, then attends over slots [0, n);
 *   without (both NULL: cross-attention over the layer's projected memory) it only attends.
 *     o[b,h,:] = softmax_j(scale <q[b,h], K[b,j,h]>) V[b,j,h],  j < n;  fp32 scores, softmax and accumulators, row maximum subtracted.
 *   n outside [1, cap]: o = 0 for that row and nothing is stored.  Slots at or beyond n are never read (they may hold anything), nor
 *   is slot n - 1 of a self-attention call (its key comes from k_new).  F32 or BF16, D in {64, 128, 256, 512}, cap <= 65536 (other:
 *   SMX_EUNSUPPORTED).  Inference only: no dropout, bias, mask or weights output.
 *   Structure: 16-byte loads of K / V from global memory into registers, no LDS tiles, no MFMA; the keys of a row are cut into
 *   plan.splits contiguous chunks of plan.chunk keys (a function of cap alone), one 4-wave workgroup each; the partial (max, sum,
 *   accumulator) triples meet in a fixed order - lane groups, waves, then chunks (a second launch when splits > 1, through
 *   `workspace`, plan.workspace_bytes, 16-byte aligned).  No atomics: two runs agree bit for bit, and row b's output depends neither on
 *   B nor on the other rows.
 * smx_attn_step_plan_query: that geometry for the descriptor's sizes and dtype; needs no GPU and no pointers (those present are checked).
 * smx_s2s_embed_step: Y[b ldy + c] = table[tok[b] ldt + c] * sqrt(D) + pe[pos[b] ldpe + c] in out_dtype (smx_tgt_embed_fwd's formula
 *   and conventions: a token outside [0, V) reads as a zero row; pe NULL adds nothing), then pos[b] += 1 for rows with done[b] == 0:
 *   afterwards pos[b] is the self-attention n_keys[b] of the step.  A row with pos[b] outside [0, max_pos) reads no positional row, is
 *   not advanced and gets done[b] = 1.  D and the leading dimensions multiples of 8 elements, 16-byte aligned bases.
 * smx_s2s_select: per row b of the logits z (B, V) with done[b] == 0, at step n = n_tok[b]:
 *     k = the lowest index of the row maximum (a NaN never wins; -1 when no entry is a number), eos left out while n < min_steps;
 *         forced[b] instead when `forced` is given (teacher forcing / scoring a given hypothesis);
 *     lp = (z[k] - max z) inv_temp - log sum_j exp((z[j] - max z) inv_temp)   (one fp64 inv_temp throughout; fp32 expf of the fp64
 *         exponent, fp32 per-lane sums, the 64 lanes and the final expression in fp64; NaN when the row holds one, -inf for a forced
 *         token outside [0, V));
 *     tokens[b, n] = k, logp_tok[b, n] = lp, score[b] += lp, n_tok[b] = n + 1;  done[b] = 1 when k == eos or n_tok[b] == cap;
 *     tok[b] = k (the next step's input).  A row with done[b] != 0 changes nothing.  One wave per row, no atomics.
 * All: SMX_EINVAL for a NULL pointer the call needs, sizes < 1, a leading dimension smaller than its row, inv_temp <= 0.  Nothing
 * allocates or synchronises with the host: capturable. */
typedef struct smx_attn_step_args {
  int32_t dtype, pad_;
  smx_attn_operand q, k_new, v_new, K, V, o;
  const int32_t* n_keys;   /* (B) device, or NULL */
  void* workspace;         /* plan.workspace_bytes, or NULL when plan.splits == 1 */
  int32_t B, H, D, cap;
  float scale;
  int32_t pad2_;
} smx_attn_step_args;      /* 288 bytes */
typedef struct smx_attn_step_plan {
  int32_t lanes_per_key, keys_per_wave, waves, threads;
  int32_t splits, chunk, launches, lds_bytes;
  int32_t grid[3];
  int32_t pad_;
  int64_t workspace_bytes;
} smx_attn_step_plan;      /* 56 bytes */
typedef struct smx_s2s_select_args {
  const void* logits;      /* (B, V) in dtype */
  int64_t ldz;
  const int32_t* forced;   /* (B) or NULL */
  int32_t* tok;            /* (B) */
  uint8_t* done;           /* (B) */
  int32_t* n_tok;          /* (B) */
  float* score;            /* (B) */
  int32_t* tokens;         /* (B, cap) */
  float* logp_tok;         /* (B, cap) */
  double inv_temp;
  int32_t dtype, B, V, cap, eos, min_steps;
} smx_s2s_select_args;     /* 104 bytes */
int smx_attn_step(const smx_attn_step_args* a, void* stream);
int smx_attn_step_plan_query(const smx_attn_step_args* a, smx_attn_step_plan* plan);
int smx_s2s_embed_step(int out_dtype, const int32_t* tok, const float* table, int64_t ldt, const float* pe, int64_t ldpe, void* Y,
                       int64_t ldy, int32_t* pos, uint8_t* done, int B, int V, int D, int max_pos, void* stream);
int smx_s2s_select(const smx_s2s_select_args* a, void* stream);

/* ---- beam search over an indexed KV cache (csrc/attn_step.hip: smx_attn_step_rows; csrc/beam.hip: smx_s2s_beam_select) -----------------
 * R = B W hypothesis rows, utterance b owns rows [b W, (b + 1) W).  No K / V is copied when the beams of an utterance reorder: the
 * attention step looks the cache row of every key up instead (DESIGN.md I.22 holds the search's definition).
 * smx_attn_step_rows: smx_attn_step (descriptor `s`, s.B = the query rows) with the cache row of a key looked up:
 *   kv_div >= 1: query row r reads cache row r / kv_div and the n_keys entry r / kv_div, so K / V hold ceil(s.B / kv_div) rows and
 *     n_keys as many entries (cross-attention: the W rows of an utterance share its projected memory; nothing is replicated).
 *     kv_div > 1 takes neither k_new / v_new nor anc (SMX_EINVAL).
 *   anc (s.B, cap) int32 on the device, leading dimension ld_anc >= cap, or NULL (self-attention): key j < n - 1 of row r is read from
 *     cache row anc[r, j] at slot j; the step's own key is stored into row r, slot n - 1, and read from k_new / v_new as in
 *     smx_attn_step.  An entry outside [0, s.B) makes that key contribute nothing (as if it were not there); it is compared before it
 *     is used and never becomes an address.  Without k_new / v_new every key j < n goes through anc.  anc must not name, for one
 *     row, the slot the call stores for another (row r', slot n[r'] - 1): the rows that read each other's cache rows are at the same
 *     position, as the hypotheses of an utterance are.
 *   Slots at or beyond n are never read, nor is any (row, slot) anc does not name.  The loads, the splits (a function of cap alone),
 *   the workspace and the combination order are smx_attn_step's, the arithmetic is the same code: with anc[r, j] = r and kv_div = 1
 *   the output has smx_attn_step's bits, with kv_div = W those of smx_attn_step over the cache replicated W times.  One extra 4-byte
 *   load per key per lane group.  No atomics, nothing allocates or synchronises: capturable.
 * smx_attn_step_rows_plan_query: smx_attn_step_plan_query for the indexed entry (the same geometry; kv_div / anc are checked).
 * smx_s2s_beam_select: one step of the search over logits (R, V), two launches that are the same at every step.  Per utterance b
 *   with done[b] == 0, at step n = n_tok[b]:
 *   row launch (one wave per row r with score[r] > -inf): lp[r, v] exactly as smx_s2s_select computes it; the row's first
 *     min(W, V) candidates in the order (logit descending, v ascending) - with `extra` (fp32 (R, V), leading dimension ldx: the hook of
 *     a scorer) in the order (lp + extra descending, v ascending) - found by repeated arg-max "strictly after the previous
 *     (value, index)", the logits are not changed; v == eos is left out while n < min_steps; candidate score = score[r] + lp[r, v]
 *     (+ extra[r, v]: score[r] + (lp + extra)) in fp32; a candidate whose score is NaN or -inf is no candidate (a row holding a NaN
 *     has none).  They go to the (R, W) workspace cand_val / cand_lp / cand_idx, their number to cand_n (R).
 *   utterance launch (one workgroup per utterance): the W best candidates of the utterance's lists, by score descending, then by
 *     (r - b W) V + v ascending; the i-th (parent p, token v) becomes slot i: tokens / logp_tok / anc rows of the parent (read into the
 *     scratch tables s_*, a workgroup barrier, written back) plus [n] = v / lp / b W + p, score = the candidate score, tok = v.
 *     A winner with v == eos - or any winner when n + 1 == cap - enters the utterance's pool instead (eos stored and counted;
 *     final score = sum / (n + 1) when length_norm, else sum; the pool keeps the best W by final score, ties to the earlier
 *     insertion: a full pool replaces its worst entry by a strictly better one) and its slot is dead: score -inf, tok = eos.  So is
 *     every slot beyond the winners.  n_tok[b] = n + 1.  When the pool holds W entries, n + 1 == cap, or no slot is alive, done[b] and
 *     done_row[b W .. (b + 1) W) are set and the pool is written, sorted by final score, to res_*.  A done utterance changes nothing.
 *   W in [1, 128]; SMX_EINVAL for a NULL pointer (extra may be), sizes < 1, ldz < V, inv_temp <= 0, R beyond 2^24.  No atomics. */
typedef struct smx_attn_step_rows_args {
  smx_attn_step_args s;
  const int32_t* anc;      /* (s.B, cap) device, or NULL */
  int64_t ld_anc;
  int32_t kv_div, pad_;
} smx_attn_step_rows_args; /* 312 bytes */
typedef struct smx_s2s_beam_args {
  const void* logits;      /* (R, V) in dtype */
  int64_t ldz;
  const float* extra;      /* (R, V) fp32 or NULL */
  int64_t ldx;
  int32_t* tok;            /* (R) the next step's input tokens */
  float* score;            /* (R) the running sums, -inf: a dead slot */
  uint8_t* done_row;       /* (R) what smx_s2s_embed_step reads */
  uint8_t* done;           /* (B) what the host polls */
  int32_t* n_tok;          /* (B) */
  int32_t* tokens;         /* (R, cap) */
  float* logp_tok;         /* (R, cap) */
  int32_t* anc;            /* (R, cap) */
  int32_t* s_tokens;       /* (R, cap) scratch of the gathers */
  float* s_logp;
  int32_t* s_anc;
  float* cand_val;         /* (R, W) workspace of the row launch */
  float* cand_lp;
  int32_t* cand_idx;
  int32_t* cand_n;         /* (R) */
  int32_t* pool_tokens;    /* (B, W, cap) the pool in insertion slots */
  float* pool_logp;        /* (B, W, cap) */
  int32_t* pool_len;       /* (B, W) */
  float* pool_final;       /* (B, W) */
  float* pool_sum;         /* (B, W) */
  int32_t* pool_seq;       /* (B, W) insertion serial */
  int32_t* pool_cnt;       /* (B) */
  int32_t* pool_ins;       /* (B) insertions so far */
  int32_t* res_tokens;     /* (B, W, cap) the pool sorted, written when the utterance ends */
  float* res_logp;         /* (B, W, cap) */
  int32_t* res_len;        /* (B, W) */
  float* res_final;        /* (B, W) */
  float* res_sum;          /* (B, W) */
  double inv_temp;
  int32_t dtype, B, W, V, cap, eos, min_steps, length_norm;
} smx_s2s_beam_args;       /* 296 bytes */
int smx_attn_step_rows(const smx_attn_step_rows_args* r, void* stream);
int smx_attn_step_rows_plan_query(const smx_attn_step_rows_args* r, smx_attn_step_plan* plan);
int smx_s2s_beam_select(const smx_s2s_beam_args* a, void* stream);

/* ---- CTC prefix scoring for the beam search (csrc/ctc_prefix.hip) --------------------------------------------------------------------
 * The recipes' `ctc_scorer: CTCScorer(eos_index, blank_index, ctc_fc: ctc_lin)` inside `ScorerBuilder(full_scorers: [ctc_scorer],
 * weights: {ctc: ctc_weight_decode})`, handed as `scorer:` to valid_search / test_search
 * (recipes/LibriSpeech/ASR/transformer/hparams/branchformer_summarymixing.yaml:227-240, 257; AISHELL-1 .../branchformer_summarymixing.yaml:
 * 181-189, 200, 211; CommonVoice .../branchformer_summarymixing.yaml:174-183, 194, 205).  DESIGN.md I.23 holds the definition.
 * x (B, T, V) fp32: the log-softmax of ctc_fc(encoder_out), frame t of utterance b at x + (b T + t) ldx; frames t >= T_b =
 * clamp(enc_len[b], 1, T) are never read.  R = B W rows as in smx_s2s_beam_select, whose score / done / n_tok / tokens / anc the
 * three entries read (none is written).  The prefix state of row r at step parity q = n_tok[b] & 1: state + ((q R + r) T + t) 2 holds
 * (r_n[t], r_b[t]) for t < T_b, psi + q R + r the log prefix probability.
 * smx_ctc_prefix_init (once per search, n_tok = 0): slot 0 of every utterance, parity 0: r_n = -inf, r_b = the running sum of
 *   x[t, blank], psi = 0.  Nothing else is written.
 * smx_ctc_prefix_score (before the selection): extra[r, v] = weight * (ctc[r, v] - lp[r, v]), ctc[r, v] = psi(g v) - psi(g), lp the
 *   log-probability of logits[r] at inv_temp in smx_s2s_beam_select's own expressions (row_scan.h: SelRow), so that the selection's
 *   lp + extra is (1 - weight) lp + weight ctc.  One lane per column v, serial over t; the parent's r_b and logaddexp(r_n, r_b) are
 *   staged once per workgroup in LDS (8 T bytes: T <= 4096, SMX_EINVAL beyond).  v == blank: -inf; v == eos: the whole-sequence
 *   probability logaddexp(r_n[T_b - 1], r_b[T_b - 1]); lp == -inf or ctc == -inf: -inf.  A row with score <= -inf (or NaN), a row
 *   of a done utterance, a row with psi(g) = -inf, a row whose logits hold a NaN or no number, and a row at n_tok outside [0, cap)
 *   write -inf into all V columns and read neither x nor their state.
 * smx_ctc_prefix_advance (after the selection): for every slot r of an utterance that is not done, with score[r] > -inf, at
 *   n = n_tok[b] >= 1: parent p = anc[r, n - 1], token c = tokens[r, n - 1]; r_n' / r_b' / psi' of g c from the parent's state at
 *   parity (n - 1) & 1 into row r at parity n & 1.  One wave per row: the lanes stage phi, x[., c], x[., blank] in LDS (12 T bytes),
 *   lane 0 runs the recursion in frame order, the lanes write the state.  A parent outside the utterance's rows or a token outside
 *   [0, V) or equal to blank / eos writes nothing.  A done utterance changes nothing; dead slots are skipped.
 * All fp32 log-domain, no atomics, fixed order: two runs agree bit for bit; nothing allocates or synchronises: capturable.
 * SMX_EINVAL: a NULL pointer the entry needs, sizes < 1, T > 4096, ldx / lde / ldz < V, blank or eos negative, blank >= V, blank ==
 * eos, weight outside (0, 1], inv_temp <= 0, R beyond 2^24. */
typedef struct smx_ctc_prefix_args {
  const float* x;          /* (B, T, V) fp32 CTC log-probabilities */
  int64_t ldx;
  const int32_t* enc_len;  /* (B) */
  const float* score;      /* (R) the search's running sums */
  const uint8_t* done;     /* (B) */
  const int32_t* n_tok;    /* (B) */
  const int32_t* tokens;   /* (R, cap) */
  const int32_t* anc;      /* (R, cap) */
  float* state;            /* (2, R, T, 2) fp32 */
  float* psi;              /* (2, R) fp32 */
  const void* logits;      /* (R, V) in dtype (score only) */
  int64_t ldz;
  float* extra;            /* (R, V) fp32 (score only) */
  int64_t lde;
  double inv_temp;
  float weight;
  int32_t dtype, B, W, V, T, cap, blank, eos, pad_;
} smx_ctc_prefix_args;     /* 160 bytes */
int smx_ctc_prefix_init(const smx_ctc_prefix_args* a, void* stream);
int smx_ctc_prefix_score(const smx_ctc_prefix_args* a, void* stream);
int smx_ctc_prefix_advance(const smx_ctc_prefix_args* a, void* stream);

/* ---- the language model's share of the scorer hook (csrc/lm_score.hip) -----------------------------------------------------------------
 * The recipes' `transformerlm_scorer: TransformerLMScorer(language_model: lm_model, temperature: 1.15)` inside
 * `scorer_test_search: ScorerBuilder(full_scorers: [transformerlm_scorer, ctc_scorer], weights: {ctc: 0.40, transformerlm: 0.60})`
 * (recipes/LibriSpeech/ASR/transformer/hparams/branchformer_summarymixing.yaml:182-191, 233-235, 242-246, 259-269).  DESIGN.md I.24
 * holds the definition.  R = B W rows as in smx_s2s_beam_select, whose score / done / n_tok the entry reads (none is written).
 * smx_lm_score (before the selection, behind smx_ctc_prefix_score when there is one): per row r of the LM's logits z (R, V),
 *     lmlp[r, v] = (z[r, v] - max z[r]) inv_temp - log sum_j exp((z[r, j] - max z[r]) inv_temp)
 *   in smx_s2s_select's expressions (row_scan.h: SelRow - one fp64 inv_temp, fp32 expf of the fp64 exponent, fp32 per-lane sums, the 64
 *   lanes and the final expression in fp64, rounded to fp32), inv_temp = 1 / the LM scorer's temperature; then
 *     accumulate == 0:  extra[r, v]  = weight * lmlp[r, v]        (the LM alone)
 *     accumulate == 1:  extra[r, v] += weight * lmlp[r, v]        (fp32; -inf in extra stays -inf)
 *   A row with score <= -inf (or NaN), a row of a done utterance and a row at n_tok outside [0, cap) score nothing: -inf in all V
 *   columns when accumulate == 0, left as they are when accumulate == 1 (smx_ctc_prefix_score wrote -inf under the same conditions).
 *   A row whose logits hold a NaN or no number: -inf in all V columns in both modes.
 *   One wave per row, two passes over the row (the second comes from L2); 16-byte loads of z and 16-byte loads / stores of extra on
 *   rows that are 16-byte aligned, element by element otherwise, with the same bits.  No atomics, no LDS; nothing allocates or
 *   synchronises: capturable; two runs agree bit for bit.
 * SMX_EINVAL: a NULL pointer, sizes < 1, ldz / lde < V, an unknown dtype, inv_temp <= 0 or not finite, weight <= 0 or not finite,
 * accumulate outside {0, 1}, R beyond 2^24. */
typedef struct smx_lm_score_args {
  const void* logits;      /* (R, V) the LM's logits in dtype */
  int64_t ldz;
  float* extra;            /* (R, V) fp32, what smx_s2s_beam_select reads */
  int64_t lde;
  const float* score;      /* (R) the search's running sums */
  const uint8_t* done;     /* (B) */
  const int32_t* n_tok;    /* (B) */
  double inv_temp;
  float weight;
  int32_t dtype, B, W, V, cap, accumulate, pad_;
} smx_lm_score_args;       /* 96 bytes */
int smx_lm_score(const smx_lm_score_args* a, void* stream);

/* ---- Transducer beam search (csrc/tbeam.hip) ---------------------------------------------------------------------------------------------
 * The transducer recipes' `Beamsearcher: speechbrain.decoders.transducer.TransducerBeamSearcher(beam_size: 10, nbest: 1, lm_module:
 * lm_model, lm_weight: 0.50, state_beam: 2.3, expand_beam: 2.3)` (recipes/LibriSpeech/ASR/transducer/hparams/
 * conformer_summarymixing_transducer.yaml:383-393).  Its source is not part of the reference tree: DESIGN.md I.25 holds the definition,
 * written from memory, and the two caps upstream does not have (E = max expansions per frame, U = max symbols per hypothesis).
 * The unit is the EXPANSION: per utterance b that is not done, one step expands its current best open hypothesis `a` (token
 * cur_tok[b], prediction-network state h_in[b] / c_in[b], LM state lm_*_in[:, b]) at its own frame frames[b]; every step is the same
 * launches, nothing synchronises with the host (which polls `done`), no atomics, fixed summation orders: two runs agree bit for bit
 * and an utterance's result does not depend on B or on the other rows.
 * smx_tbeam_init:   the start of a search: the one hypothesis [blank], sum 0, zero states, picked and staged (cur_tok = blank, the
 *                   staging rows zero); frames / expansions / overflow / n_hyps 0, tokens -1, out_len 0, scores / sums -inf; done[b] =
 *                   (lengths[b] == 0), such an utterance returning the one empty hypothesis with score 0.
 * smx_tbeam_step:   three launches.  h_out / c_out = one LSTM step on cur_tok[b] from h_in / c_in (the W_ih^T row gather of
 *                   smx_onehot_gates_fwd; c fp32, h rounded to dtype - smx_greedy_decode's step); pdec = h_out W_proj^T; z[b,:] =
 *                   act(enc[b, t, :] + pdec[b]) W_lin^T + b_lin with t = clamp(frames[b], 0, T - 1), smx_greedy_decode's arithmetic
 *                   and roundings, stored in fp32.  Rows of done utterances are computed too and read by nobody.
 * smx_tbeam_select: one launch, one workgroup per utterance that is not done.  lp = log-softmax(z[b]) in fp32 (the row code of
 *                   smx_s2s_select at temperature 1), lm = log-softmax(lm_logits[b]) likewise when lm_logits is given; the W best
 *                   of lp in the order (value descending, index ascending), found by repeated arg-max "strictly after the previous
 *                   (value, index)"; best = the first's value, the second's if the first is the blank.  In that order: the blank
 *                   -> the closed list gets (a's prediction, a's sum + lp, a's states); another token k with lp >= best - expand_beam
 *                   -> the open list gets (a's prediction + k, a's sum + lp + lm_weight lm[k], the new states).  A hypothesis of U
 *                   symbols gets no other child than the blank, which it always gets, and sets overflow bit 1.  Then the frame
 *                   ends if the closed list holds W entries; else if this was the frame's E-th expansion (the closed list is filled
 *                   up to W with the best of the open list by key = sum / (symbols + 1), overflow bit 0); else if the open list is
 *                   empty; else if the closed list's best by key has sum >= state_beam + the sum of the open list's best by key
 *                   (a tie on keys takes the earlier insertion).  A frame end advances frames[b], turns the closed list into the
 *                   open list of the next frame (prefixes written out, states copied to the other half of their ping-pong) and, at
 *                   frames[b] == lengths[b], sets done[b] and writes the closed list sorted by key (stable) into tokens (B, nbest, U;
 *                   padded with -1) / out_len / scores (keys) / sums / n_hyps.  Otherwise the open list's best by key is removed and
 *                   staged: cur_tok and the staging rows *_in of the next step.  The new states h_out / c_out / lm_*_out are copied
 *                   into state storage once per expansion.  expansions[b] counts the steps; overflow bit 2: a row without numbers.
 * `state`: smx_tbeam_state_bytes(...) bytes, 16-byte aligned, opaque (lists, nodes, prefixes, state slots; csrc/tbeam.hip TbLayout),
 * initialised by smx_tbeam_init.  lm_logits (B, V; leading dimension ld_lm) in dtype with lm_h_* (lm_L, B, lm_H) dtype and lm_c_*
 * (lm_L, B, lm_H) fp32 - the buffers of RNNLM.step on cur_tok - or all NULL: no LM.  The three entries take the same struct.
 * Supported (smx_tbeam_ok; SMX_EUNSUPPORTED otherwise): H (and lm_H) as smx_lstm_ok, J as smx_greedy_ok, V in [3, 8192], W in [2, 32]
 * and below V, 4 V + 16 (W + E W) bytes within the selection's 60 KB of LDS, 16-byte aligned operands.  SMX_EINVAL: a NULL pointer
 * the entry needs, sizes < 1, nbest outside [1, W], blank outside [0, V), a NaN parameter, staging rows in == out, bad strides. */
typedef struct smx_tbeam_args {
  const void* enc;         /* (B, T, J) dtype: enc[b, t, :] at enc + b ld_b + t ld_t */
  int64_t ld_b, ld_t;
  const int32_t* lengths;  /* (B) frames per utterance, or NULL: all T */
  const void* WihT;        /* (V - 1, 4H; ldw) = W_ih^T */
  int64_t ldw;
  const float* bias;       /* (4H) = b_ih + b_hh */
  const void* Whh;         /* (4H, H) */
  const void* Wproj;       /* (J, H) */
  const void* Wlin;        /* (V, J) */
  const float* blin;       /* (V) or NULL */
  int32_t* cur_tok;        /* (B) the staged hypothesis' last token */
  void* h_in;              /* (B, H) dtype: its prediction-network state */
  float* c_in;             /* (B, H) */
  void* h_out;             /* (B, H) dtype: the state after the step */
  float* c_out;            /* (B, H) */
  void* pdec;              /* (B, J) dtype */
  float* z;                /* (B, V) fp32 joint logits */
  const void* lm_logits;   /* (B, V; ld_lm) dtype, or NULL */
  int64_t ld_lm;
  void* lm_h_in;           /* (lm_L, B, lm_H) dtype */
  float* lm_c_in;          /* (lm_L, B, lm_H) */
  const void* lm_h_out;    /* (lm_L, B, lm_H) dtype */
  const float* lm_c_out;   /* (lm_L, B, lm_H) */
  void* state;             /* smx_tbeam_state_bytes */
  uint8_t* done;           /* (B) what the host polls */
  int32_t* overflow;       /* (B) bit 0: the expansion cap ended a frame; bit 1: a hypothesis reached U symbols; bit 2: a row without numbers */
  int32_t* expansions;     /* (B) steps taken */
  int32_t* frames;         /* (B) frames closed = the current frame */
  int32_t* tokens;         /* (B, nbest, U) */
  int32_t* out_len;        /* (B, nbest) */
  float* scores;           /* (B, nbest) keys */
  float* sums;             /* (B, nbest) */
  int32_t* n_hyps;         /* (B) */
  float lm_weight, state_beam, expand_beam;
  int32_t dtype, B, T, H, J, V, W, nbest;
  int32_t E;               /* max expansions per frame */
  int32_t U;               /* max symbols per hypothesis */
  int32_t act, blank, lm_L, lm_H, pad_;
} smx_tbeam_args;          /* 344 bytes */
int smx_tbeam_ok(int dtype, int H, int J, int V, int W);
size_t smx_tbeam_state_bytes(int dtype, int B, int H, int W, int max_expansions, int max_symbols, int lm_layers, int lm_H);
int smx_tbeam_init(const smx_tbeam_args* a, void* stream);
int smx_tbeam_step(const smx_tbeam_args* a, void* stream);
int smx_tbeam_select(const smx_tbeam_args* a, void* stream);

/* ---- The same search carried across streaming chunks ------------------------------------------------------------------
 * A STREAM is one utterance's search in one batch slot, fed (n_1, n_2, ...) frames over successive chunk calls, each n_k in [0, C].
 * After the call that delivers chunk k the slot's result is the result of the search above over the concatenation of the frames
 * delivered so far - every field, `frames` counted over the whole stream - so after the last chunk it is smx_tbeam_init / _step /
 * _select's result over the whole utterance, bit for bit.  The two entries take the struct above, read for ONE CHUNK: enc (B, C, J)
 * with T = C, lengths (B) REQUIRED = the frames of this chunk per slot (clamped to [0, C]), frames (B) = the frame index inside the
 * chunk (what smx_tbeam_step reads), U required as ever (a stream has no T to derive it from).  smx_tbeam_step and the LM step are
 * used as they are.  What a stream needs beyond the struct - which stays 344 bytes - travels like this:
 *   start          (B) bytes on the device, an extra argument of smx_tbeam_resume: nonzero = the slot begins a new stream;
 *   stream_frames  (B) int32 on the device, an extra argument of both entries: the frames closed over the whole stream, the result's
 *                  `frames` (the struct's `frames` restarts at 0 with every chunk);
 *   the dead flag  the eighth, so far spare, counter of the slot's state block (0 after an init): set when the search ended on a row
 *                  without numbers (overflow bit 2, an empty closed list).  smx_tbeam_state_bytes is what it was.
 * smx_tbeam_resume:        one launch before a chunk's steps, one workgroup per slot.  start[b]: smx_tbeam_init's work for that row
 *                          alone, stream_frames[b] = 0; with lengths[b] == 0 the slot reports the one empty hypothesis, score 0, and
 *                          goes on from the staged [blank] when frames arrive.  Otherwise a dead slot, or one with lengths[b] == 0,
 *                          is left exactly as it was.  Otherwise the slot is re-armed: frames[b] = 0, done[b] = 0 - nothing is
 *                          picked again, the hypothesis staged at the pause is the one to expand.
 * smx_tbeam_select_stream: smx_tbeam_select's kernel instantiated with a flag; one launch.  It differs where frames[b] reaches
 *                          lengths[b]: the result is written as above (rows past n_hyps and tokens past out_len reset to their
 *                          cleared values, the closed list left in insertion order), and then the ordinary frame end is done as
 *                          well - the closed list becomes the open list of the next frame, prefixes written out, this expansion's
 *                          state saved, the survivors' states copied to the other half, the next hypothesis picked and staged -
 *                          and done[b] = 1: for a stream `done` means PAUSED.  An empty closed list ends the search as it does
 *                          above and marks the slot dead.  Every frame end advances stream_frames[b] with frames[b].
 * SMX_EINVAL: NULL start / stream_frames / lengths / state (or any pointer the selection needs), sizes < 1; SMX_EUNSUPPORTED as
 * smx_tbeam_ok and the selection's LDS bound. */
int smx_tbeam_resume(const smx_tbeam_args* a, const uint8_t* start, int32_t* stream_frames, void* stream);
int smx_tbeam_select_stream(const smx_tbeam_args* a, int32_t* stream_frames, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SMX_H_ */
