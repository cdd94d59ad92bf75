/* libdwiseneuro_hip.so — C-ABI of the MI355X-native DwiseNeuro hot path.
 *
 * The reference (lRomul/sensorium) has no native code and no FFI: its hot path is
 * `DwiseNeuro.forward` (src/models/dwiseneuro.py:397-405) + `MicePoissonLoss` (src/losses.py:10-21) driven
 * by `MouseModel.train_step` (src/argus_models.py:43-71), all delegated to torch/cuDNN ops.  This header is
 * the boundary a maintainer binds instead (ctypes stub: INTEGRATION.md): one entry point per fused kernel
 * family plus block-level composites, each citing the reference lines it replaces.
 *
 * Conventions
 *  - plain `extern "C"`, raw device pointers + sizes; no torch types.  The caller (PyTorch) owns and
 *    allocates every buffer, including workspaces; the library never allocates device memory, keeps no
 *    mutable global state, never synchronises, and enqueues only on the passed `stream`
 *    (hipGraph-capturable).  Every call takes an explicit `device` because autograd calls backward from a
 *    worker thread whose current device is not the caller's.
 *  - return value: 0 ok; < 0 argument / unsupported-configuration error; > 0 a hipError_t.
 *    `dwn_last_error()` returns a thread-local message.  Every entry answers its argument errors from the arguments alone, before it
 *    enters the device and with nothing queued or written: -1 null struct or required pointer, -7 a mode it is not built for, -2
 *    geometry (sizes positive, divisibility, dtype / training values, row and grid counts below 2^31), -4 a size that is not
 *    built, then the workspace (-6 for the model's composites, -3 for the analysis entries).  A size entry (*_workspace_bytes,
 *    *_ws_bytes, *_wt_bytes) answers 0 for bad arguments — null, or a geometry its entries refuse — and leaves no error behind.
 *  - activations are channels-last matrices [rows = (b,t,h,w)][C] in `dtype` storage
 *    (DWN_F32 = fp32 parity mode, DWN_BF16 = bf16 storage / fp32 accumulate).  Parameters, BN
 *    coefficients, statistics and gradients of parameters are always fp32.
 *  - channel counts must be multiples of 8 (one 16-byte bf16 vector).
 */
#ifndef DWN_H_
#define DWN_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DWN_ABI_VERSION 7
#define DWN_F32 0
#define DWN_BF16 1
/* How the dtype-f32 GEMMs of a block / cortex layer / readout multiply.  NATIVE: v_mfma_f32_16x16x4_f32.  SPLIT3: each operand
 * as bf16 hi + lo, three bf16 MFMAs (hi*hi + hi*lo + lo*hi, fp32 accumulate): 5.8e-7 relative L2 from NATIVE on the full-width
 * eval forward, a sixth of the matrix-core time.  AUTO: SPLIT3 in the eval-mode forward, NATIVE in training (where the
 * analytically-zero gradients' summation noise would otherwise exceed the parity tests' floors). */
#define DWN_F32_AUTO 0
#define DWN_F32_NATIVE 1
#define DWN_F32_SPLIT3 2
/* BatchNorm mode: the `training` field of dwn_stem_args / dwn_block_args / dwn_cortex_args.
 * EVAL: normalise with the running statistics, keep nothing for a backward (dwn_*_backward returns -7).
 * TRAIN: batch statistics, running statistics and num_batches_tracked updated, intermediates saved, backward built (the gradient
 * w.r.t. the model input included: dwn_stem_backward_input).
 * FROZEN: normalise with the running statistics and do not touch them (as EVAL), take the training kernels and save the same
 * intermediates (as TRAIN), and run a backward in which BatchNorm is the fixed affine map it was in the forward:
 * dx = gamma * invstd_running * dy, dgamma = sum dy * xhat, dbeta = sum dy.  For input gradients (receptive fields, most-exciting
 * inputs) and for fine-tuning with frozen statistics.  The frozen forward follows the training kernels (native fp32 products,
 * materialised / rebuilt y1 per y1_mode), so it equals the EVAL forward to rounding, not bit for bit.  Workspace sizes and
 * dwn_block_forward_writes answer for FROZEN as for TRAIN. */
#define DWN_BN_EVAL 0
#define DWN_BN_TRAIN 1
#define DWN_BN_FROZEN 2
#define DWN_NREP 32 /* replicas of every cross-workgroup statistics buffer: double[DWN_NREP][2][C] */

/* operand loader kinds (how a kernel reads one 16-byte channel vector of an operand) */
#define DWN_LD_PLAIN 0   /* p                                                     */
#define DWN_LD_PE 1      /* p + pe_t[t] + pe_h[h] + pe_w[w]      (dwiseneuro.py:184-192) */
#define DWN_LD_BNACT 2   /* act(v1*p + v2) * gate[b]             (dwiseneuro.py:16-22, 38-43) */
#define DWN_LD_AFFINE2 3 /* v1*p + v2*q + v3                     (BatchNorm backward) */
#define DWN_LD_DY3 4     /* v1*((p*gate[b]+gate2[b])*silu'(v4*q+v5)) + v2*q + v3 (SE + BN3 backward) */
#define DWN_LD_GATE 5    /* p * gate[b]                          (SE gate on a materialised activation) */
#define DWN_LD_CAT1 6    /* columns [0, cat_c1): p (row stride ld); [cat_c1, cat_c1 + cat_c2): q (row stride ld2); beyond: 1.0
                          * — dwn_gemm_tn's P operand only: [dh1 | a0 | 1]^T a0 gives the three raw products of the conv_pw
                          * weight gradient in one pass (dwn_block_backward; csrc/dwn_elementwise.hip k_pw_wgrad_fold) */

typedef struct dwn_load_desc {
    const void* p;
    const void* q;
    long long ld;
    const float* v1;
    const float* v2;
    const float* v3;
    const float* v4;
    const float* v5;
    const float* gate;
    const float* gate2;
    int gate_ld;
    int rows_per_sample;
    int act;
    const float* pe_t;
    const float* pe_h;
    const float* pe_w;
    int pT, pH, pW;
    int pe_ld;
    long long ld2;          /* DWN_LD_CAT1: row stride of q */
    int cat_c1, cat_c2;     /* DWN_LD_CAT1: columns taken from p / from q */
} dwn_load_desc;

#define DWN_EPI_STORE 0
#define DWN_EPI_READOUT 1
#define DWN_EPI_DG 2
#define DWN_EPI_STORE_CAT 3   /* DWN_EPI_STORE + K-concatenated second A operand (a2, K1) + fp32 bias[N] */
#define DWN_EPI_DH3 4         /* see gate3 / dps3 / coef3 below */

/* C[M][N] = load(A)[M][K] . B[N][K]^T  (+ BN statistics / readout / SE-grad epilogues).
 * Replaces nn.Conv3d 1x1x1 (dwiseneuro.py:91,118) and grouped nn.Conv1d k=1 (:207,276). */
typedef struct dwn_gemm_nn_args {
    dwn_load_desc a;
    int a_kind;
    const void* b; long long ldb;
    void* c; long long ldc;
    int M, N, K;
    int groups;
    double* stats;
    int f32_split;      /* dtype f32 only: nonzero = products as bf16 hi/lo splits on the bf16 matrix cores (hi*hi + hi*lo + lo*hi, fp32
                         * accumulate; ~1e-5 relative) instead of the fp32 MFMA — the eval-mode forward sets it, training does not */
    int stat_nchan;
    int epi;
    const float* bias; float sp_beta; float* out_nct; int Tn; int n_valid;
    /* DWN_EPI_DG: y3 = the activated project-conv input z3 = SiLU(BN3(y3)) [M][N] (materialised by the forward);
     * dg[b][n] += sum_{m in sample b} C[m][n] * z3[m][n].  s3 / t3 are reserved and must be NULL. */
    const void* y3; long long ldy3; const float* s3; const float* t3; float* dg; int dg_ld; int rows_per_sample;
    /* optional K-concatenation: columns k >= K1 of the A operand come from a2[m][k - K1] (plain loads);
     * only with epi == DWN_EPI_STORE_CAT, which also adds `bias` (fp32 [N]) before rounding. */
    const void* a2; long long a2_ld; int K1;
    /* optional per-sample weights: rows [b*b_rows_per_sample, (b+1)*b_rows_per_sample) multiply the weight matrix at
     * b + b*b_sample_stride elements (e.g. W . diag(gate_b): the SE gate folded into conv_pwl).  Needs
     * b_rows_per_sample % 128 == 0, groups == 1 and K > one k-tile; 0 = one weight matrix for every row. */
    long long b_sample_stride; int b_rows_per_sample;
    /* DWN_EPI_DH3 (conv_pwl data gradient fused with the SE-gate / SiLU / BatchNorm-3 backward prologue,
     * dwiseneuro.py:113-120 backward): with du = the GEMM result rounded to `dtype`, the kernel stores
     *   dh3[m][n] = (du*gate3[b][n] + dps3[b][n]) * silu'(coef3[0][n]*y3[m][n] + coef3[1][n])
     * into c (y3 = the raw temporal-conv output; b = m / rows_per_sample; gate3/dps3 rows are dg_ld apart) and, when
     * `stats` is set, accumulates sum(dh3) and sum(dh3 * (y3 - coef3[2][n]) * coef3[3][n]) — the two BatchNorm-backward
     * sums.  coef3 is the [4][coef3_ld] table scale, shift, mean, invstd. */
    const float* gate3; const float* dps3; const float* coef3; int coef3_ld;
    /* kernel variant: DWN_NN_AUTO = chosen by shape; DWN_NN_XL128 / DWN_NN_XL256 = the 256-row LDS-DMA kernel with 128- / 256-column
     * tiles wherever its argument constraints hold (bf16, plain loader, store epilogue); DWN_NN_KD = the A-direct kernel (deep K,
     * N % 128 == 0, plain / gate loader, store / K-concat epilogue); DWN_NN_TILE128 = never those kernels (the tests compare them
     * with the 128-row kernel bit for bit) */
    int variant;
    /* DWN_EPI_READOUT, optional: the Softplus beta in DEVICE memory (one fp32).  Non-null: read by the kernel (one uniform load per
     * workgroup) instead of sp_beta — a learnable beta, or one changed between replays of a captured graph.  Plain loader only.
     * Null: sp_beta, and the kernel that ran before this field existed. */
    const float* sp_beta_dev;
} dwn_gemm_nn_args;
#define DWN_NN_AUTO 0
#define DWN_NN_XL128 1
#define DWN_NN_XL256 2
#define DWN_NN_TILE128 3   /* never the 256-row / A-direct kernels: the 128-row persistent kernel (what the tests compare them with) */
#define DWN_NN_KD 4        /* the A-direct kernel (deep K, N % 128 == 0: only the weights pass through LDS) wherever its constraints hold */

/* dW[R][Cc] += sum_m load(P)[m][r] * load(Q)[m][c]   (fp32 atomics; dW must be zeroed by the caller) */
typedef struct dwn_gemm_tn_args {
    dwn_load_desc p; int p_kind;
    dwn_load_desc q; int q_kind;
    int M, R, Cc;
    float* dw; long long lddw;
    int groups;
    int rows_per_split; int nsplit;       /* nsplit <= 0: both chosen by the library.  nsplit > 0 (rows_per_sample == 0): split i
                                           * takes rows [i*rows_per_split, (i+1)*rows_per_split) cut at M; the splits must cover
                                           * every row: rows_per_split <= 0 or nsplit * rows_per_split < M is refused with -2
                                           * before anything is enqueued */
    int R_load;                           /* P columns per group incl. zero padding (>= R; 0 -> R) */
    /* per-sample products: with rows_per_sample > 0 (M % rows_per_sample == 0, groups == 1) the rows of sample b
     * accumulate into dw + b*dw_sample_stride — B separate [R][Cc] matrices P_b = load(P)_b^T load(Q)_b.
     * splits_per_sample is chosen by the library. */
    int rows_per_sample; int splits_per_sample; long long dw_sample_stride;
    /* 1: the caller wants dW = the product, not dW += : when the launch needs only one M-split the tiles are written with plain
     * stores (the 64-byte-segment fp32 atomics are the slow part of a weight gradient with a big output: 16 M floats for a
     * readout) and dW need not be zeroed; when it needs more, the library zeroes dW itself first.  Needs lddw == Cc and
     * rows_per_sample == 0 (the [groups * R][Cc] matrix is one contiguous block). */
    int overwrite;
    /* 1 (ABI 7): dw points to DOUBLE [groups * R][lddw] and the M-split partial tiles are added with fp64 atomics — for products
     * that are later differenced (the Gram pass of dwn_conv_pw_bn_stats: var = w^T (G / n - mu mu^T) w cancels mean^2 against
     * E[y^2], and several hundred fp32 atomic adds per element carry 1e-6 of the SUM).  Not with overwrite / per-sample mode. */
    int dw_f64;
} dwn_gemm_tn_args;

/* depth-wise (1,k,k) conv, stride (1,s,s), pad k/2 — dwiseneuro.py:96-100 */
typedef struct dwn_dw_spatial_fwd_args {
    dwn_load_desc in;   /* DWN_LD_BNACT over raw y1 */
    const float* w;     /* [k*k][C] fp32 tap-major */
    void* out;
    int planes, Hin, Win, Hout, Wout, C, stride, ks;
    double* stats;
    int rows_band;      /* output rows per chunk / band; <= 0: chosen by the library */
    int impl;           /* 0: the library's choice (chained row-walk kernels where they apply); 1: the pair / generic kernels, the
                         * second implementation the tests compare bit for bit */
    /* rebuilt-input mode (a0 != NULL; dwn_dw_spatial_fwd_rc_supported): in.p is NOT read — the kernel rebuilds the rows of
     * y1 = a0 . w1^T it needs on the matrix cores (dwiseneuro.py:90-91) from the block input a0 [rows][a0_ld] (Cin channels) and
     * w1 = conv_pw's weight [C][Cin] rounded to bf16, row-major, and applies in.v1 / in.v2 (BatchNorm-1 scale / shift) + SiLU to
     * the fp32 accumulators (since round 6 the product is not rounded to bf16 first: the result is the reference arithmetic with
     * one rounding fewer than conv_pw's stored output + the stored-input form).  conv_pw + spat_covn_dw in one pass over a 7x
     * narrower input. */
    const void* a0; long long a0_ld; const void* w1; int Cin;
} dwn_dw_spatial_fwd_args;

typedef struct dwn_dw_spatial_bwd_args {
    dwn_load_desc dy;   /* DWN_LD_AFFINE2 over (dh2, y2) */
    dwn_load_desc y1;   /* p = raw y1; v1..v4 = bn1 scale, shift, mean, invstd */
    const float* w;
    void* dh1;
    float* dw;          /* [C][k*k] fp32, accumulated */
    int planes, Hin, Win, Hout, Wout, C, stride, ks;
    double* stats;
    int rows_band;
    int impl;           /* as in dwn_dw_spatial_fwd_args */
    /* rebuilt-y1 mode (a0 != NULL; dwn_dw_spatial_bwd_rc_supported): y1.p is NOT read — the kernel rebuilds the y1 values it needs
     * as a0 . w1^T on the matrix cores (dwiseneuro.py:90-91; the fp32 accumulators, not rounded to bf16: the same values the
     * rebuilt-input forward activates) from the block input a0 [rows][a0_ld] (Cin channels, the positional encoding included)
     * and w1 = conv_pw's weight [C][Cin] rounded to bf16, row-major.  y1.v1..v4 (BatchNorm-1 coefficients) as usual. */
    const void* a0; long long a0_ld; const void* w1; int Cin;
} dwn_dw_spatial_bwd_args;

/* depth-wise (k,1,1) conv along T, pad k/2 — dwiseneuro.py:105-109 */
typedef struct dwn_dw_temporal_fwd_args {
    dwn_load_desc in;
    const float* w;     /* [k][C] */
    void* out;
    int B, T, HW, C, kt;
    double* stats;
    /* eval-mode epilogue (BatchNorm-3 coefficients are known before the pass): with z_scale != NULL the kernel stores
     * z3 = SiLU(z_scale * y3 + z_shift) instead of y3 (y3 rounded to the storage type first, as a stored y3 would read back)
     * and, with pooled != NULL, adds the per-(sample, channel) sums of the stored z3 into pooled [B][C] (zeroed by the
     * caller) — the SqueezeExcite pooling pass (dwiseneuro.py:38-39) without a separate read of y3.  The sums are 64-bit
     * fixed point in units of 2^-32 (sum = pooled * 2^-32): integer adds make them independent of the arrival order. */
    const float* z_scale; const float* z_shift; long long* pooled;
} dwn_dw_temporal_fwd_args;

typedef struct dwn_dw_temporal_bwd_args {
    dwn_load_desc dy; int dy_kind;   /* DWN_LD_AFFINE2: dy3 = v1*p + v2*q + v3 from (dh3, y3); DWN_LD_PLAIN: p = dh3 only and
                                      * y3 is recomputed from y2 inside the kernel (one E-wide pass less); DWN_LD_DY3 */
    dwn_load_desc y2;                /* p = raw y2; v1..v4 = bn2 scale, shift, mean, invstd */
    const float* w;
    void* dh2;
    float* dw;                       /* [C][k] */
    int B, T, HW, C, kt;
    double* stats;
} dwn_dw_temporal_bwd_args;

/* BatchNorm parameter bundle (BatchNormAct, dwiseneuro.py:9-22) */
typedef struct dwn_bn {
    const float* gamma; const float* beta;
    float* running_mean; float* running_var; long long* num_batches_tracked;
    float* coef;    /* [4][C]: scale, shift, mean, invstd — written by forward, read by backward */
    float* dgamma; float* dbeta;   /* backward outputs (may be null in forward) */
} dwn_bn;

/* stem: Conv3d(C_in->C0, 1x1x1) + BN on the NCDHW fp32 input — dwiseneuro.py:306-309 */
typedef struct dwn_stem_args {
    int dtype, training, B, Cin, C0; long long S;   /* S = T*H*W; training: DWN_BN_EVAL / _TRAIN / _FROZEN */
    float eps, momentum;
    const float* x;      /* [B][Cin][S] fp32 */
    const float* w;      /* [C0][Cin] */
    dwn_bn bn;
    const float *pe_t, *pe_h, *pe_w;   /* optional: positional encoding of the FIRST block, added to `out`  */
    int T, H, W;                       /* (dwiseneuro.py:184-192); S = T*H*W                                 */
    void* y0;            /* unused since ABI 2 (the raw conv output is never materialised); may be NULL */
    void* out;           /* BN output [B*S][C0] */
    const void* dout;    /* backward: grad wrt out */
    float* dw;           /* backward: [C0][Cin], written (not accumulated) */
    void* ws; size_t ws_bytes;
    double* xmom;        /* [8 + 8*8] input moments: sum x_k, sum x_k x_l — written by the training forward, read by the
                          * backward (y0 = W0 x is linear in the <= 8 input channels: BatchNorm statistics and the weight
                          * gradient follow from them; saved instead of y0).  Not used with DWN_BN_FROZEN (may be NULL) */
} dwn_stem_args;

/* gradient of the stem's output w.r.t. its NCDHW fp32 input (dwn_stem_args has no dx): with BatchNorm as a fixed affine map,
 * dx[b][k][s] = sum_c w[c][k] * coef[c] * dout[b*S + s][c]   (coef[c] = gamma_c * invstd_c, the first row of dwn_bn.coef as the
 * forward wrote it).  One streaming pass over dout.  training must be DWN_BN_FROZEN: in DWN_BN_TRAIN the batch statistics add
 * terms in x that need the finished sums of the parameter-gradient pass — this call returns -7 for it, and the training-mode
 * input gradient comes from dwn_stem_backward_input (below); DWN_BN_EVAL returns -7 like every backward.
 * C0 a multiple of 8, at most 128 (bf16) / 64 (fp32); Cin <= 8. */
typedef struct dwn_stem_input_grad_args {
    int dtype, training, B, Cin, C0; long long S;
    const float* w;      /* [C0][Cin] */
    const float* coef;   /* [4][C0] of the forward (only the scale row is read) */
    const void* dout;    /* [B*S][C0] in dtype */
    float* dx;           /* [B][Cin][S] fp32, written whole */
} dwn_stem_input_grad_args;

/* one InvertedResidual3d preceded by its PositionalEncoding3d — dwiseneuro.py:136-144, 184-192 */
typedef struct dwn_block_args {
    int dtype, training;                     /* training: DWN_BN_EVAL / _TRAIN / _FROZEN */
    int B, T, Hin, Win, Hout, Wout, Cin, Cmid, Cout, stride, ks, kt, se_r;
    float eps, momentum;
    const void* x; void* out;
    void *y1, *y2, *y3, *y4;
    void* z3;                                /* silu(bn3(y3)), materialised once by the SE pooling pass (saved) */
    int x_has_pe;                            /* 1: x already contains this block's positional encoding          */
    void* a0;                                /* x_has_pe == 0: [M_in][Cin] buffer receiving x + PE (saved)      */
    const float *pe_t, *pe_h, *pe_w;         /* this block's PE tables [T][Cin], [Hin][Cin], [Win][Cin]         */
    const float *out_pe_t, *out_pe_h, *out_pe_w;  /* next block's PE tables ([T|Hout|Wout][Cout]) added to out, or null */
    const float *w_pw, *w_dws, *w_dwt, *w_pwl, *se_wr, *se_br, *se_we, *se_be;
    dwn_bn bn1, bn2, bn3, bn4, bnsc;
    const float* drop_scale;                 /* [B] DropPath factor mask/keep (dwiseneuro.py:46-54) or null */
    const int *hsrc, *wsrc, *hinv, *winv;    /* nearest-interpolation index maps (device int32) */
    float *se_pmean, *se_hidpre, *se_gate;   /* saved SE activations [B][Cmid], [B][se_r], [B][Cmid] */
    /* backward only */
    const void* dout; void* dx;
    void *buf_a, *buf_b;                     /* scratch [max(M_in,M_out)][Cmid], [M_out][Cmid] */
    void *dy4, *da0;                         /* scratch [M_out][Cout], [M_in][Cin] */
    float *dw_pw, *dw_dws, *dw_dwt, *dw_pwl, *dse_wr, *dse_br, *dse_we, *dse_be;   /* overwritten (16-byte aligned) */
    void* ws; size_t ws_bytes;
    /* backward, conv_pwl: 0 = the library chooses by shape between (1) per-sample products dy4_b^T z3_b + a GEMM that
     * recomputes du in its epilogue and (2) the materialised du = dy4 . W2 with a separate reduction pass; 1 / 2 force one
     * (the parity tests run both implementations against the oracle) */
    int pwl_bwd;
    int f32_products;                        /* DWN_F32_AUTO / _NATIVE / _SPLIT3: how dtype f32 multiplies (see below) */
    /* training, bf16: 0 = the library leaves y1 (conv_pw's output, the widest tensor of the block) unmaterialised where both
     * stencils can rebuild it from the block input on the matrix cores (BatchNorm-1 statistics from the Gram matrix of the
     * input) AND that is the faster path (64 input channels): y1 may then be NULL in forward and backward
     * (dwn_block_forward_writes bit 0 clear); 1 = always materialise y1; 2 = y1-free wherever it is built (64 / 128 input channels).
     * Forward and backward of one block must be called with the same value. */
    int y1_mode;
} dwn_block_args;

/* AdaptiveAvgPool3d((None,1,1)) — dwiseneuro.py:374,400 */
typedef struct dwn_pool_args {
    int dtype; long long BT; int HW, C;
    const void* x; void* out; const void* dout; void* dx;
} dwn_pool_args;

/* ShuffleLayer — dwiseneuro.py:228-234 */
typedef struct dwn_cortex_args {
    int dtype, training, B, T, Cin, C, groups;   /* training: DWN_BN_EVAL / _TRAIN / _FROZEN */
    float eps, momentum;
    const void* x; void* out; void* y;      /* y: raw conv output [B*T][C] (saved) */
    const float* w;                         /* [C][Cin/groups] */
    dwn_bn bn, bnsc;
    const float* drop_scale;
    const void* dout; void* dx; float* dw;  /* backward; dw [C][Cin/groups] fp32 (16-byte aligned) is cleared and written by the call */
    const float* dout_mask; int dout_mask_ld; /* optional [B][C] multiplier on dout (readout Dropout1d backward) */
    void* ws; size_t ws_bytes;
    int f32_products;                         /* DWN_F32_AUTO / _NATIVE / _SPLIT3 */
} dwn_cortex_args;

/* Readout — dwiseneuro.py:283-287 */
typedef struct dwn_readout_args {
    int dtype, B, T, Cin, groups, n_out;    /* n_out = N (valid neurons); weight has ceil(N/g)*g rows */
    float softplus_beta;
    const void* x;                          /* [B*T][Cin] */
    const float* w; const float* bias;      /* [Npad][Cin/groups], [Npad] */
    const float* drop_mask;                 /* [B][Cin] Dropout1d factor or null */
    float* out;                             /* [B][N][T] fp32 */
    const float* dout; void* dx; float* dw; float* dbias;   /* backward: dw is overwritten (no zeroing needed), dbias is
                                                              * accumulated with atomics (zeroed by the caller) */
    void* ws; size_t ws_bytes;
    /* optional: the weight in the data gradient's operand layout, [groups][Cin/groups][Rp] in the compute type
     * (dwn_readout_wt_bytes).  Non-null in forward: written by the same pass that packs the forward layout (one read of the
     * fp32 weight for both).  Non-null in backward: used as is — the caller kept it from the forward of the same step —
     * instead of packing the weight again. */
    void* wt;
    int f32_products;                       /* DWN_F32_AUTO (= native here: the readout has no training flag) / _NATIVE / _SPLIT3 */
    /* learnable Softplus beta; both null = the fixed softplus_beta above, and the kernels that ran before these
     * fields existed.
     * beta_dev: one fp32 in device memory, > 0, read by the forward epilogue and by the backward instead of softplus_beta (which
     *   is then ignored).  The same value gives the same bits of out / dx / dw as the fixed path.  Forward needs only this one.
     * dbeta: one fp32 in device memory; dwn_readout_backward OVERWRITES it with sum_{b,n,t} dout * d out / d beta — reduced in
     *   float64, one partial per workgroup in the workspace and a fixed-order finaliser: no atomics, bit-reproducible in both
     *   builds.  dwn_readout_backward wants both pointers or neither (-2 otherwise); dwn_readout_workspace_bytes(a, 1) accounts
     *   for the partials when beta_dev is set. */
    const float* beta_dev; float* dbeta;
} dwn_readout_args;

typedef struct dwn_tensor_entry {
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq; float* ema;
    long long numel; int is_int64; int pad_;
} dwn_tensor_entry;

/* ---- guarded optimizer step: global gradient-norm clipping and the skip of a step with a non-finite gradient,
 * both decided on the device — no host read-back, capturable in a hipGraph.
 * dwn_guarded_entry = the fields of dwn_tensor_entry + the parameter's own step count in DEVICE memory (as torch's fused AdamW
 * keeps it under found_inf): the host cannot know whether a step was skipped, so it cannot count. */
typedef struct dwn_guarded_entry {
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq; float* ema;
    long long numel; int is_int64; int pad_;
    long long* step;                        /* one int64 per parameter (distinct words within a call); may be null for
                                             * dwn_grad_sumsq_multi, which reads grad and numel only */
} dwn_guarded_entry;
/* device-resident; zeroed once by the caller, then written by dwn_step_guard_finalize alone */
typedef struct dwn_step_guard {
    double norm;                            /* sqrt of the summed squares of grad_scale * g over all finite elements */
    float coef;                             /* min(1, max_norm / (norm + 1e-6)) (torch clip_grad_norm_), 1 when clipping is off */
    int skip;                               /* 1 iff skip_nonfinite and nonfinite > 0 */
    long long nonfinite;                    /* Inf / NaN elements among the gradients of this step */
    long long good_steps, skipped_steps;    /* running totals over the calls of dwn_step_guard_finalize */
} dwn_step_guard;
#define DWN_GS_SEG 1024                     /* tensors per sum-of-squares launch (a longer table takes several, one fold) */

/* ---- batch assembly on the device --------------------------------------------------------
 * A trial stays resident in HBM in the reference's on-disk layout (src/datasets.py:37-51, src/data.py:59-70):
 * video [H0][W0][L] (uint8 or float32), behavior [2][L], pupil_center [2][L], responses [N][L] (float32).
 * `dwn_clip_src` names one window of one trial: frame of window position t = frame_start + t*frame_step
 * (IndexesGenerator.make_indexes, src/indexes.py:23-30).  The caller guarantees the frames lie inside [0, length). */
#define DWN_VID_U8 0
#define DWN_VID_F32 1
typedef struct dwn_clip_src {
    const void* video; const float* behavior; const float* pupil_center; const float* responses;
    long long length;
    int video_dtype;
    int frame_start, frame_step;
    int valid;                       /* 0 = slot unused */
} dwn_clip_src;
/* One sample of the batch: `src`, optionally mixed with `mix` (same mouse).
 * mix_mode DWN_MIX_BOX (CutMix, mixers.py:52-67): rows [bbx1,bbx2) x columns [bby1,bby2) of all five input channels come
 * from `mix` — the reference pastes its "x" range onto the row axis, mixers.py:63 — and the target is
 * one_minus_lam*relu(src) + lam*relu(mix) with lam = box area / (H*W) (mixers.py:64-65).
 * mix_mode DWN_MIX_BLEND (Mixup, mixers.py:22-33): inputs AND target are one_minus_lam*src + lam*mix with the drawn lam.
 * Both factors are rounded to float by the caller (torch multiplies a float tensor by the scalar cast to float). */
#define DWN_MIX_BOX 0
#define DWN_MIX_BLEND 1
typedef struct dwn_clip_desc {
    dwn_clip_src src, mix;
    int bbx1, bby1, bbx2, bby2;
    float one_minus_lam, lam;
    int mouse;                       /* owner: index into the per-mouse target table */
    int mix_mode;
} dwn_clip_desc;

/* opt-in kernel-family timer: HIP events recorded on the launch stream around the block-level kernels.
 * Used by bench.py for the live roofline measurement; disabled (mask 0) by default. */
enum {
    DWN_FAM_PW_FWD = 0, DWN_FAM_DWS_FWD, DWN_FAM_DWT_FWD, DWN_FAM_SE_POOL, DWN_FAM_PWL_FWD, DWN_FAM_RESID_FWD,
    DWN_FAM_RESID_BWD, DWN_FAM_PWL_DGRAD, DWN_FAM_PWL_WGRAD, DWN_FAM_BN3_REDUCE, DWN_FAM_DWT_BWD, DWN_FAM_DWS_BWD,
    DWN_FAM_PW_DGRAD, DWN_FAM_PW_WGRAD, DWN_FAM_CORTEX_FWD, DWN_FAM_CORTEX_BWD, DWN_FAM_READOUT_FWD, DWN_FAM_READOUT_BWD,
    DWN_FAM_COUNT
};
/* family_mask bit DWN_PROF_ROCTX: additionally bracket every family launch with a roctx range named after the family
 * ("dwn:pw_fwd", ...) so that rocprofv3 --marker-trace timelines are labelled; the roctx library is dlopen'ed on first use
 * (librocprofiler-sdk-roctx.so, else libroctx64.so) and silently skipped when absent.  The range bit alone records no events. */
#define DWN_PROF_ROCTX (1ull << 63)
int dwn_profile_enable(unsigned long long family_mask, int device);
int dwn_profile_collect(int family, double* total_ms, long long* launches);

int dwn_abi_version(void);
const char* dwn_source_hash(void);         /* sha256[:16] of the source files the library was built from (csrc/Makefile HASH_SRCS) */
int dwn_sizeof(const char* struct_name);   /* sizeof of a struct of this header, -1 if unknown (binding self-check) */
const char* dwn_last_error(void);

/* kernel families */
int dwn_gemm_nn(const dwn_gemm_nn_args* a, int dtype, int device, void* stream);
int dwn_gemm_tn(const dwn_gemm_tn_args* a, int dtype, int device, void* stream);
int dwn_dw_spatial_fwd(const dwn_dw_spatial_fwd_args* a, int dtype, int device, void* stream);
int dwn_dw_spatial_bwd(const dwn_dw_spatial_bwd_args* a, int dtype, int device, void* stream);
/* 1 when dwn_dw_spatial_fwd can run these arguments in rebuilt-input mode (bf16, Cin 64 or 128, C % 64 == 0, the row-walk plane widths) */
int dwn_dw_spatial_fwd_rc_supported(const dwn_dw_spatial_fwd_args* a, int dtype);
/* 1 when dwn_dw_spatial_bwd can run these arguments in rebuilt-y1 mode (bf16, Cin 64 or 128, C % 64 == 0, the row-walk plane widths) */
int dwn_dw_spatial_bwd_rc_supported(const dwn_dw_spatial_bwd_args* a, int dtype);
int dwn_dw_temporal_fwd(const dwn_dw_temporal_fwd_args* a, int dtype, int device, void* stream);
int dwn_dw_temporal_bwd(const dwn_dw_temporal_bwd_args* a, int dtype, int device, void* stream);
/* The two entries above are built for kt 3 and 5 and answer -4 for every other size.  Sizes 7 and 9 have entries of their own, with
 * the same argument structs and the same outputs (y3 or the z3 + pooling epilogue and the statistics forward; dh2, dw [C][kt] and the
 * two BatchNorm-2 backward sums backward).  The backward is built for dy_kind == DWN_LD_PLAIN only, the form dwn_block_backward runs
 * (y3 recomputed from y2, rounded to the storage type as a stored y3 would read back).  Refusals, all answered before the device is
 * entered and with nothing written: kt not 7 or 9 -> -4; C % 8 != 0 -> -2; backward with DWN_LD_AFFINE2 / DWN_LD_DY3 (the stored-y3
 * loaders, built for 3 and 5 only) or any other loader -> -3.  dwn_block_forward / dwn_block_backward take kt 3, 5, 7 and 9. */
int dwn_dw_temporal_wide_fwd(const dwn_dw_temporal_fwd_args* a, int dtype, int device, void* stream);
int dwn_dw_temporal_wide_bwd(const dwn_dw_temporal_bwd_args* a, int dtype, int device, void* stream);
int dwn_bn_finalize(const double* stats, int stat_c, double count, const dwn_bn* bn, int C, int training,
                    float momentum, float eps, int device, void* stream);
int dwn_bn_bwd_finalize(const double* stats, double count, const dwn_bn* bn, float* abc, int C, int device,
                        void* stream);
int dwn_pack_weight(const float* src, void* dst, int groups, int R, int C, int transpose, int Rd, int Cd,
                    int dtype, int device, void* stream);
/* BatchNorm-1 (conv_pw.1.bn, dwiseneuro.py:91-92) in training mode WITHOUT conv_pw's output: y1 = a0 . W1^T is linear in the block
 * input a0 [M][a0_ld] (Cin channels), so its batch mean / variance follow from the Gram matrix a0^T a0 and the column sums 1^T a0
 * (one Cin-wide pass): mean_e = w_e . mu, var_e = w_e^T (G / M - mu mu^T) w_e, with w_pw [E][Cin] rounded to `dtype` first (the
 * weights the matrix cores multiply with).  Writes bn->coef [4][E] = scale, shift, mean, invstd and updates the running statistics
 * and num_batches_tracked like nn.BatchNorm3d.  sc_stats (optional, double[DWN_NREP][2][Cin], zeroed by the caller): receives the
 * shortcut BatchNorm's sums of an identity-map block (sum a0, sum a0^2 per channel) in replica 0.  ws: caller-owned scratch. */
size_t dwn_conv_pw_bn_stats_workspace_bytes(int Cin);    /* replicas x (Cin + 8) * Cin doubles + alignment (8 replicas at Cin = 64) */
int dwn_conv_pw_bn_stats(const void* a0, long long a0_ld, long long M, const float* w_pw, int E, int Cin, const dwn_bn* bn,
                         float momentum, float eps, double* sc_stats, void* ws, size_t ws_bytes, int dtype, int device,
                         void* stream);

/* composites (forward / backward of one reference module each) */
size_t dwn_stem_workspace_bytes(const dwn_stem_args* a);     /* 0 for bad arguments */
int dwn_stem_forward(const dwn_stem_args* a, int device, void* stream);
int dwn_stem_backward(const dwn_stem_args* a, int device, void* stream);
int dwn_stem_input_grad(const dwn_stem_input_grad_args* a, int device, void* stream);
/* dwn_stem_backward + the gradient w.r.t. the NCDHW fp32 input THROUGH the batch statistics, from one accumulation pass over
 * dout (a->x, a->xmom, a->bn.coef as the training forward left them; a->ws sized by dwn_stem_workspace_bytes):
 *   dx[b][k][s] = sum_c w[c][k] scale_c dout[b*S+s][c]  +  sum_j Q[k][j] (x[b][j][s] - xbar_j)  +  q0[k]
 *   Q[k][j] = sum_c a2_c w[c][k] w[c][j],  a2_c = -scale_c invstd_c^2 (sum dout_c (z_c - mean_c)) / M,
 *   q0[k]   = -(1/M) sum_c w[c][k] scale_c sum dout_c,                    M = B*S, z = W0 x.
 * dgamma, dbeta, dw are what dwn_stem_backward writes (same launches, same bits under the deterministic build); then a
 * one-workgroup finaliser forms Q, q0, xbar and one streaming pass over dout and x writes dx.
 * training must be DWN_BN_TRAIN: DWN_BN_EVAL returns -7 like every backward, DWN_BN_FROZEN returns -7 too (its gradient is
 * dwn_stem_backward + dwn_stem_input_grad).  dx: [B][Cin][S] fp32, written whole.  Null dx / x / xmom / dout / dw / ws: -1.
 * The argument checks answer before the device is entered.  C0 and Cin as dwn_stem_input_grad. */
int dwn_stem_backward_input(const dwn_stem_args* a, float* dx, int device, void* stream);
size_t dwn_block_workspace_bytes(const dwn_block_args* a, int backward);     /* 0 for bad arguments */
int dwn_block_forward(const dwn_block_args* a, int device, void* stream);
int dwn_block_backward(const dwn_block_args* a, int device, void* stream);
/* bit 0: dwn_block_forward writes y1; bit 1: it writes y3 (eval mode skips them where the stencil rebuilds y1 / the temporal
 * pass emits z3 directly: the caller may leave those pointers NULL).  Null arguments or a geometry dwn_block_forward refuses: its
 * negative code, with the error set (dwn_block_backward_route likewise) */
int dwn_block_forward_writes(const dwn_block_args* a);
/* bit 0: dwn_block_backward's conv_pw data gradient is dx itself — the shortcut branch's gradient is folded into the one-pass
 * kernel (dwn_pw_bwd_fused_supported; da0 is not written); bit 1: ... through the inverse nearest maps hinv / winv of a strided
 * block.  Answered from the arguments alone, no device (additive under ABI 7). */
int dwn_block_backward_route(const dwn_block_args* a);
int dwn_pool_forward(const dwn_pool_args* a, int device, void* stream);
int dwn_pool_backward(const dwn_pool_args* a, int device, void* stream);
size_t dwn_cortex_workspace_bytes(const dwn_cortex_args* a, int backward);   /* 0 for bad arguments */
int dwn_cortex_forward(const dwn_cortex_args* a, int device, void* stream);
int dwn_cortex_backward(const dwn_cortex_args* a, int device, void* stream);
size_t dwn_readout_workspace_bytes(const dwn_readout_args* a, int backward); /* 0 for bad arguments */
size_t dwn_readout_wt_bytes(const dwn_readout_args* a);                      /* 0 for bad arguments */
int dwn_readout_forward(const dwn_readout_args* a, int device, void* stream);
int dwn_readout_backward(const dwn_readout_args* a, int device, void* stream);

/* MicePoissonLoss — losses.py:10-21.  w = mice_weights[:, m] / sum(mice_weights) (normalised by caller).
 * forward accumulates into *loss_acc (double, zeroed by caller); backward writes dpred. */
int dwn_poisson_loss_forward(const float* pred, const float* target, const float* w, long long per_sample,
                             long long total, float eps, double* loss_acc, int device, void* stream);
int dwn_poisson_loss_backward(const float* pred, const float* target, const float* w, const float* gscale,
                              long long per_sample, long long total, float eps, float* dpred, int device,
                              void* stream);
int dwn_f64_to_f32(const double* src, float* dst, int n, int device, void* stream);

/* fused multi-tensor AdamW (+EMA) — torch.optim.AdamW (true_batch_001.py:45-48) + ModelEma.update (ema.py:47-55).
 * `list` is a DEVICE array of ntensors entries.  step >= 1. */
int dwn_adamw_ema_multi(const dwn_tensor_entry* list, int ntensors, int max_blocks, double lr, double beta1,
                        double beta2, double eps, double weight_decay, long long step, double ema_decay,
                        double grad_scale, int device, void* stream);
int dwn_ema_lerp_multi(const dwn_tensor_entry* list, int ntensors, int max_blocks, double decay, int device,
                       void* stream);

/* Guarded step, three calls on one stream (all tables, pairs, the workspace and the guard are DEVICE memory; argument errors are
 * answered with a negative code before anything touches a device):
 *
 * dwn_grad_sumsq_multi: pair[0] = sum over all entries of (grad_scale * g)^2, accumulated in float64 (the square of a float32 is
 *   exact in double: gradients of 3e25 give a finite sum); pair[1] = the number of elements that are not finite, as a double.
 *   Non-finite elements are counted and left out of the sum.  Entries with a null grad or numel <= 0 contribute nothing; grad may
 *   start at any 4-byte boundary (float4 loads behind a scalar head, scalar tail).  Two stages in a fixed order — max_blocks
 *   workgroups write one partial each into `ws` by a plain store, a one-workgroup launch folds them — without atomics: the same
 *   table and max_blocks give the same bits on every launch, in the deterministic build as well.  `ws` holds
 *   dwn_grad_guard_workspace_bytes(ntensors, max_blocks) bytes, 16-byte aligned.  1 <= max_blocks <= 65536.
 * dwn_step_guard_finalize: adds pair_a and the optional pair_b (the sharded slices' sum after its all-reduce; null otherwise),
 *   writes *guard (see dwn_step_guard; max_norm <= 0 = no clipping) and, unless the step is skipped, adds 1 to the step counter of
 *   each of the ntensors entries of `list` (null list with ntensors = 0: no counters).
 * dwn_adamw_ema_multi_guarded: dwn_adamw_ema_multi with the gradient factor grad_scale * guard->coef and each entry's step count
 *   read from the device (already advanced; 1 - beta^t, lr / bc1 and sqrt(bc2) formed in double and cast to float as there;
 *   entries of different counts ride in one launch).  With guard->skip set, param, exp_avg, exp_avg_sq are not written and the
 *   EMA leg still runs on the unchanged parameter (the reference's GradScaler skips optimizer.step, ModelEma.update runs anyway). */
size_t dwn_grad_guard_workspace_bytes(int ntensors, int max_blocks);
int dwn_grad_sumsq_multi(const dwn_guarded_entry* list, int ntensors, int max_blocks, double grad_scale, void* ws,
                         size_t ws_bytes, double* pair, int device, void* stream);
int dwn_step_guard_finalize(const double* pair_a, const double* pair_b, double max_norm, int skip_nonfinite,
                            const dwn_guarded_entry* list, int ntensors, dwn_step_guard* guard, int device, void* stream);
int dwn_adamw_ema_multi_guarded(const dwn_guarded_entry* list, int ntensors, int max_blocks, double lr, double beta1,
                                double beta2, double eps, double weight_decay, double ema_decay, double grad_scale,
                                const dwn_step_guard* guard, int device, void* stream);


/* conv_pw backward (dwiseneuro.py:90-93 backward) WITHOUT reading y1.  With the BatchNorm-1 backward affine
 *   dy1 = abc[0]*dh1 + abc[1]*y1 + abc[2]   (per channel of E; abc is [3][E])   and   y1 = a0 . W1^T,
 * both products fold the y1 term into Cin x Cin matrices:
 *   da0[M][Cin] = dy1 . W1    = [dh1 | a0] . [diag(abc0) W1 ; W1^T diag(abc1) W1] + abc2 . W1
 *   dw[E][Cin]  = dy1^T . a0  = diag(abc0) (dh1^T a0) + diag(abc1) W1 (a0^T a0) + abc2 (1^T a0)     (fp32, overwritten)
 * so the E-wide traffic is one read of dh1 (dtype == DWN_BF16, M % 128 == 0, and Cin == 64 with E == 448 or 384, or Cin == 128
 * with E == 896 — see
 * dwn_pw_bwd_fused_supported — one kernel computes both products from a single pass) or two (dwn_gemm_nn with the
 * K-concatenated operand + dwn_gemm_tn with the DWN_LD_CAT1 loader).  w_pw = conv_pw.0.weight [E][Cin] fp32 (used as rounded
 * to `dtype`, the values the forward multiplied with).  ws: dwn_pw_backward_workspace_bytes(E, Cin, dtype) bytes, 256-aligned. */
typedef struct dwn_pw_bwd_args {
    const void* dh1; const void* a0; const float* w_pw; const float* abc;
    void* da0; float* dw;
    long long M; int E; int Cin;
    void* ws; size_t ws_bytes;
    /* optional: the gradient of a stride-1 block's shortcut branch (BatchNorm of the channel-tiled block input, dwiseneuro.py:125-134)
     * folded in, so that da0 becomes the block's input gradient:
     *   da0[m][c] += sum_{c' = c + j*Cin < res_C} (res_abc[0][c']*res[m][c'] + res_abc[1][c']*a0[m][c] + res_abc[2][c'])
     * res = the block's output gradient [M][res_C] (`dtype`), res_abc = [3][res_C]; res_C in {Cin, 2*Cin}, Cin 64 / 128.  Only where
     * dwn_pw_bwd_fused_supported (the one-pass kernel's epilogue adds it; on the two-GEMM path it measured slower than the
     * separate pass it replaces: -3 there).  NULL = off. */
    const void* res; const float* res_abc; int res_C;
    /* ... of a strided block: res_hinv [res_Hin] / res_winv [res_Win] = the inverse nearest maps (output row / column an input
     * row / column is sampled into, or -1), M = frames * res_Hin * res_Win; only rows m = (f, hi, wi) with both >= 0 get the sum
     * above, with res read at row (f * res_Hout + ho) * res_Wout + wo.  NULL = identity map (stride 1: res has M rows). */
    const int* res_hinv; const int* res_winv; int res_Hin, res_Win, res_Hout, res_Wout;
} dwn_pw_bwd_args;
int dwn_pw_bwd_fused_supported(int dtype, long long M, int E, int Cin);
size_t dwn_pw_backward_workspace_bytes(int E, int Cin, int dtype);           /* 0 for bad arguments */
int dwn_pw_backward(const dwn_pw_bwd_args* a, int dtype, int device, void* stream);

/* ---- spat_covn_dw WITHOUT a materialised conv_pw output (dwiseneuro.py:90-102; bf16 storage, 3x3, stride 1 or 2,
 * Cin in {64, 128}, E % 64 == 0).  y1 = a0 . W1^T is the widest tensor at input resolution although it is a Cin-deep
 * product of a tensor E/Cin times narrower: the kernel rebuilds each y1 tile from the a0 tile with MFMAs while it
 * stages the stencil's LDS tile, so the forward reads a0 (once per tile, all E/64 channel slices are produced from
 * the LDS-resident copy) and writes y2.  `blob` holds, per 64-channel slice, the LDS images the kernel copies by
 * LDS-DMA: the W1 rows (bf16, bank-swizzled), the pair-packed bf16 stencil weights and the BatchNorm-1 scale / shift;
 * dwn_dw_spatial_rc_prep builds it (after the BatchNorm-1 coefficients are final).
 * round_y1 != 0 rounds the rebuilt y1 to bf16 before the BatchNorm (bit-identical to reading a stored bf16 y1). */
typedef struct dwn_dw_spatial_rc_fwd_args {
    const void* a0; long long a0_ld;   /* block input incl. its positional encoding [planes*Hin*Win][Cin] */
    const void* blob;                  /* dwn_dw_spatial_rc_blob_bytes(E, Cin) bytes */
    void* out;                         /* y2 [planes*Hout*Wout][E] */
    int planes, Hin, Win, Hout, Wout, Cin, E, stride;
    double* stats;                     /* double[DWN_NREP][2][E] sum / sum of squares of y2, or null */
    int rows_band;                     /* output rows per tile; <= 0: chosen by the library */
    int round_y1;
} dwn_dw_spatial_rc_fwd_args;
size_t dwn_dw_spatial_rc_blob_bytes(int E, int Cin);
/* w_pw [E][Cin] fp32 (conv_pw.0.weight), w_dws [9][E] fp32 tap-major, bn1_coef [>=2][E] scale, shift */
int dwn_dw_spatial_rc_prep(const float* w_pw, const float* w_dws, const float* bn1_coef, int E, int Cin, void* blob,
                           int device, void* stream);
int dwn_dw_spatial_rc_supported(int dtype, int Cin, int E, int ks, int stride, int Hin, int Win);
int dwn_dw_spatial_fwd_rc(const dwn_dw_spatial_rc_fwd_args* a, int device, void* stream);

/* StackInputsProcessor + CutMix on the inputs (inputs.py:15-36, mixers.py:52-63) for a whole batch:
 * x [B][5][T][H][W] fp32 = channel 0 the video centre-padded with pad_fill, channels 1-2 behavior, 3-4 pupil_center
 * broadcast over the frame.  `descs` is a DEVICE array of B entries; every video has the same H0 x W0. */
int dwn_assemble_inputs(const dwn_clip_desc* descs, int B, int T, int H0, int W0, int H, int W, float pad_fill,
                        float* x, int device, void* stream);
/* responses_to_tensor + CutMix target blend + construct_mice_sample + collate (responses.py:25-29, mixers.py:64-66,
 * datasets.py:172-187): targets[m] (DEVICE table of n_mice pointers) is [B][n_neurons[m]][T] fp32, fully overwritten —
 * the owner's rows with the target, every other mouse's rows of that sample with zeros; mice_weights [B][n_mice]
 * one-hot.  `max_neurons` = max over n_neurons (host copy, sizes the grid). */
int dwn_assemble_targets(const dwn_clip_desc* descs, int B, int T, float* const* targets, const int* n_neurons,
                         int n_mice, int max_neurons, float* mice_weights, int device, void* stream);

/* ---- gaze shifter: a per-frame translation of ONE channel of the model input, resampled bilinearly.
 * x, out, dout, dx: [B][Cin][T][H][W] fp32 contiguous; shift, dshift: [B][T][2] fp32, (dy, dx) in pixels.  Channel
 * `video_channel` is resampled, every other channel is copied (forward) / passes dout through (backward).  With the plane
 * extended by the constant `fill` outside [0,H) x [0,W), iy = floor(dy), fy = dy - iy (fp32), likewise ix, fx:
 *   out[y][x] = (1-fy)(1-fx) v(y+iy, x+ix)   + (1-fy) fx v(y+iy, x+ix+1)
 *             +    fy (1-fx) v(y+iy+1, x+ix) +    fy  fx v(y+iy+1, x+ix+1)
 * (= grid_sample bilinear, zeros padding, align_corners=True for fill = 0).  A shift of exactly 0 copies the plane bit for bit.
 * A tap whose weight is 0 contributes nothing whatever it holds (Inf, NaN, a non-finite fill); a tap of weight 1 gives its bits.
 * Any finite shift is legal (beyond the frame: out = fill, dx = dshift = 0; the float -> int conversion is clamped); a NaN / Inf
 * shift gives a frame of NaN in out (backward: dx = 0 and dshift = NaN for that frame).  No access leaves the tensors.
 * Backward: dx = the adjoint gather sum_{a,b} w_a w_b dout[y-iy-a][x-ix-b] (out-of-frame terms dropped), dshift[b][t] =
 * sum_{y,x} dout * d out / d (dy, dx) with iy, ix held constant (the right derivative at integer shifts), accumulated in float64
 * by one workgroup per frame in a fixed order.  No atomics anywhere: the same inputs give the same bits, in both builds.
 * dwn_gaze_shift_forward needs x, shift, out.  dwn_gaze_shift_backward needs shift, dout and at least one of dx, dshift (a null
 * one is skipped; both null: -1); dshift also needs x.  Argument errors (null pointer -1, geometry -2) are answered before the
 * device is entered. */
typedef struct dwn_gaze_args {
    int B, Cin, T, H, W;
    int video_channel;
    float fill;
    int pad_;
    const float* x;
    const float* shift;
    float* out;
    const float* dout;
    float* dx;
    float* dshift;
} dwn_gaze_args;
int dwn_gaze_shift_forward(const dwn_gaze_args* a, int device, void* stream);
int dwn_gaze_shift_backward(const dwn_gaze_args* a, int device, void* stream);
/* mean[b][t][k] = mean over H x W of channel c0 + k of x [B][Cin][T][H][W] fp32, k in [0, nc): float64 accumulation in a fixed
 * order (one workgroup per plane, no atomics), so a constant plane returns its constant bit for bit (-0.0 included).  Null
 * pointer -1; non-positive size, or [c0, c0 + nc) outside [0, Cin): -2 — before the device is entered. */
int dwn_plane_mean(const float* x, int B, int Cin, int T, int H, int W, int c0, int nc, float* mean, int device, void* stream);

/* ---- correlation objective: per-neuron Pearson correlation of ONE mouse over the (sample, frame) values of the
 * rows R = {b : w[b * w_stride] != 0}, n = |R| * T, and the loss share * red_j (1 - r_j) with its gradient.
 * pred, target, dpred: [B][N][T] fp32 contiguous ((B, N) tensors: T = 1).  stat: double [DWN_CORR_STAT_ROWS][N], rows
 *   0 mean_p   1 mean_t   2 M2p = sum (p - mean_p)^2   3 M2t   4 C = sum (p - mean_p)(t - mean_t)          (dwn_corr_moments)
 *   5 r = (C/n) / ((sd_p + eps)(sd_t + eps)), sd = sqrt(M2/n)   6 c1 = 1/(n a c)   7 c2 = r/(n sd_p a), 0 where sd_p == 0
 *                                                    with a = sd_p + eps, c = sd_t + eps            (dwn_corr_loss_finalize)
 * count: one double, n (0 when the mouse has no row: every row of stat is then 0, the loss term and dpred are exactly 0 — decided
 * on the device).  Rows with w == 0 are never read (they may hold NaN) and get dpred = 0.
 * dwn_corr_moments: needs pred, target, w, stat, count.  Means in a first sweep, centred sums in a second sweep of the same
 *   workgroup, float64 throughout; one workgroup per tile of DWN_CORR_TILE neurons, rows split over the waves and merged in LDS
 *   in a fixed order.  No atomics: the same inputs give the same bits on every launch and in both builds.
 * dwn_corr_loss_finalize: needs stat, count, share, loss_acc, ws.  Fills rows 5-7 and adds share * rho * sum_j (1 - r_j) to
 *   *loss_acc (double, zeroed by the caller before the first mouse; rho = 1/N for DWN_CORR_MEAN, 1 for DWN_CORR_SUM): one partial
 *   per workgroup into ws, folded by a one-workgroup launch in a fixed order.  ws: dwn_corr_ws_bytes(a) bytes, 8-byte aligned.
 * dwn_corr_loss_backward: needs pred, target, w, stat, share, dpred (gscale: the incoming gradient, a device scalar; null = 1).
 *   dpred = -g share rho [c1 (t - mean_t) - c2 (p - mean_p)], evaluated in float64 and rounded once.
 * share is a DEVICE scalar (fp32).  Nothing is allocated and nothing is read back: every entry can be captured.  Argument errors
 * (null pointer -1, geometry -2, workspace -3) are answered before the device is entered. */
#define DWN_CORR_STAT_ROWS 8
#define DWN_CORR_TILE 16
enum { DWN_CORR_MEAN = 0, DWN_CORR_SUM = 1 };
typedef struct dwn_corr_args {
    int B, N, T;
    int reduction;            /* DWN_CORR_MEAN / DWN_CORR_SUM */
    double eps;               /* added to each standard deviation (> 0) */
    long long w_stride;       /* elements between the weights of consecutive rows (>= 1): a column of mice_weights is passed as is */
    const float* pred;
    const float* target;
    const float* w;
    double* stat;
    double* count;
    const float* share;
    double* loss_acc;
    const float* gscale;
    float* dpred;
    void* ws; size_t ws_bytes;
} dwn_corr_args;
size_t dwn_corr_ws_bytes(const dwn_corr_args* a);
int dwn_corr_moments(const dwn_corr_args* a, int device, void* stream);
int dwn_corr_loss_finalize(const dwn_corr_args* a, int device, void* stream);
int dwn_corr_loss_backward(const dwn_corr_args* a, int device, void* stream);

/* ---- in-silico stimuli: a drifting Gabor rendered into ONE channel of the model input, and the reduction of the
 * input gradient to the Gabor's parameters.  x, out, dout: [B][Cin][T][H][W] fp32 contiguous; params, dparams: [B][8] fp32 in the
 * order cy, cx, sigma, theta, sf, tf, phase, amplitude (pixels, pixels, pixels, radians, cycles/pixel, cycles/frame, radians, grey
 * levels).  For a pixel (y, x) of frame t inside the window rectangle (y0, x0, wh, ww) — wh == ww == 0: the whole plane —
 *   dyp = y - cy, dxp = x - cx, u = dxp cos(theta) + dyp sin(theta), q = sf u - tf t + phase / (2 pi)          (cycles)
 *   e   = exp(-(dxp^2 + dyp^2) / (2 sigma^2))  (DWN_GABOR_GAUSSIAN)   |   1  (DWN_GABOR_NONE: a full-field grating)
 *   raw = background + amplitude e cos(2 pi q),   out = clamp ? min(max(raw, lo), hi) : raw
 * and outside the window the video plane holds `pad`.  Coordinates are those of the plane, not of the window.  The carrier is
 * evaluated at q - rint(q) (an exact reduction) with a sincospi call.  Channel `video_channel` is rendered, every other channel
 * is copied from x bit for bit.
 * dwn_gabor_forward needs x, params, out.  dwn_gabor_backward needs params, dout, dparams, ws and reads only the video channel of
 * dout: dparams[b][k] = sum_{t, y, x} dout * d out / d p_k, where the gradient passes through the clamp iff lo <= raw <= hi (as
 * torch.clamp), `raw` recomputed by the device function of the forward.  Per-pixel products in fp32, sums in float64: one partial
 * per (clip, frame, chunk of 1024 window pixels) into ws (dwn_gabor_workspace_bytes(a) bytes, 8-byte aligned), folded per clip in
 * a fixed order.  No atomics; the grids depend on the geometry alone: the same inputs give the same bits, in both builds.  With
 * DWN_GABOR_NONE dsigma is exactly 0.
 * A clip with a non-finite parameter, or with sigma <= 0 under the Gaussian envelope, renders NaN inside its window and gets NaN in
 * all eight dparams; other clips are untouched.  No parameter is converted to an integer or enters an address.
 * Nothing is allocated and nothing is read back: both entries can be captured.  Argument errors are answered before the device is
 * entered: null pointer -1; geometry -2 (a non-positive size, video_channel outside [0, Cin), a window not inside the plane,
 * clamp with lo > hi or a NaN bound, an unknown envelope); workspace too small or misaligned -3. */
enum { DWN_GABOR_GAUSSIAN = 0, DWN_GABOR_NONE = 1 };
typedef struct dwn_gabor_args {
    int B, Cin, T, H, W;
    int video_channel;
    int envelope;             /* DWN_GABOR_GAUSSIAN / DWN_GABOR_NONE */
    int clamp;                /* 0: out = raw; 1: out = raw clamped to [lo, hi] */
    int y0, x0, wh, ww;       /* the window; wh == ww == 0 (then y0 == x0 == 0): the whole plane */
    float background, lo, hi, pad;
    const float* x;
    const float* params;
    float* out;
    const float* dout;
    float* dparams;
    void* ws; size_t ws_bytes;
} dwn_gabor_args;
size_t dwn_gabor_workspace_bytes(const dwn_gabor_args* a);       /* 0 for arguments the entries would refuse */
int dwn_gabor_forward(const dwn_gabor_args* a, int device, void* stream);
int dwn_gabor_backward(const dwn_gabor_args* a, int device, void* stream);

/* ---- behaviour modulator: a per-neuron gain on a readout's output, driven by the behaviour features of each frame.
 * y, out, dout, dy: [B][N][T] fp32 contiguous (the readouts' layout); h, dh: [B][T][K] fp32; u, du: [N][K]; c, dc: [N];
 * m = max_log_gain.
 *   a[b,n,t]   = c[n] + sum_k h[b,t,k] u[n,k]          (fp32 FMAs, k ascending, starting from c[n])
 *   gain       = exp(m tanh(a))                         in [e^-m, e^m], exactly 1 at a = 0
 *   out[b,n,t] = y[b,n,t] gain
 *   dy = dout gain,   s = dout y gain m sech^2(a),   du[n,k] = sum_{b,t} s h[b,t,k],   dc[n] = sum_{b,t} s,
 *   dh[b,t,k] = sum_n s u[n,k]
 * sech^2(a) = 4 e / (1 + e)^2 with e = exp(-2 |a|): it does not cancel for large |a|.  The products are fp32; the three sums run
 * in float64 in a fixed order through per-workgroup partials in ws (dwn_modulator_ws_bytes(a) bytes, 8-byte aligned; it depends on
 * B, N, T, K alone) and are rounded to fp32 once.  No atomics: the same inputs give the same bits, in both builds.  du, dc and dh
 * are written, not accumulated.  A null dy / dh / du / dc is skipped, and its partials are neither computed nor stored.
 * A frame (b, t) whose h row holds a NaN or an Inf gets NaN in out[b,:,t], dy[b,:,t] and in every sum the frame enters; other
 * frames are untouched.  u = c = 0 returns y (and dout in dy) bit for bit.  No access leaves the tensors for any T.
 * dwn_modulator_forward needs y, h, u, c, out (out must not alias y) and no workspace.  dwn_modulator_backward needs y, h, u, c,
 * dout, ws and at least one of dy, dh, du, dc.  Nothing is allocated and nothing is read back: both entries can be captured.
 * Argument errors are answered before the device is entered: null pointer -1; a non-positive size, K outside [1, 32], a
 * max_log_gain that is not finite and positive, out == y, or a workspace that is too small or misaligned -2. */
typedef struct dwn_modulator_args {
    int B, N, T, K;
    float max_log_gain; int pad_;
    const float* y; const float* h; const float* u; const float* c;
    float* out;
    const float* dout; float* dy; float* dh; float* du; float* dc;
    void* ws; size_t ws_bytes;
} dwn_modulator_args;
size_t dwn_modulator_ws_bytes(const dwn_modulator_args* a);      /* backward only; forward needs none; 0 for refused arguments */
int dwn_modulator_forward(const dwn_modulator_args* a, int device, void* stream);
int dwn_modulator_backward(const dwn_modulator_args* a, int device, void* stream);

/* ---- regularised MEI synthesis: a separable three-axis blur of one channel, per-clip moments of one channel and
 * the two element-wise updates of the pixel-space ascent.  All tensors are [B][Cin][T][H][W] fp32 contiguous and ONE channel of
 * them is used; the window rectangle (y0, x0, wh, ww) — wh == ww == 0 (then y0 == x0 == 0): the whole plane — is the same in
 * every frame.  Nothing is allocated and nothing is read back: every entry can be captured.  No atomics, and every grid depends
 * on the geometry alone: the same inputs give the same bits, in both builds.  No tensor value is converted to an index.
 * Argument errors are answered before the device is entered: null pointer -1; geometry -2 (a non-positive size, a channel
 * outside [0, Cin), a radius outside [0, DWN_BLUR_MAX_RADIUS], a window not inside the plane, lo > hi or a NaN bound, an unknown
 * mode); workspace too small or misaligned -3.  The *_ws_bytes functions return 0 for arguments the entries would refuse.
 *
 * dwn_blur3d: dst[b][c_dst][t][y][x] = sum_{i,j,k} kt[i] kh[j] kw[k] src[b][c_src][t+i-Rt][y+j-Rh][x+k-Rw] inside the window, the
 * source counting as zero outside the window and outside [0, T); inside the plane but outside the window dst[b][c_dst] is written
 * with 0 and the source is not read there; the other channels of dst are not touched.  `taps` is a DEVICE table
 * float[3][2 * DWN_BLUR_MAX_RADIUS + 1] read at run time (axis a = 0, 1, 2 for t, y, x uses entries 0 .. 2 Ra, entry Ra is the
 * centre); the taps are neither assumed symmetric nor normalised.  Evaluated axis by axis in fp32: x and y in one launch (the
 * frame tile and its halo in LDS) into ws, then t from ws into dst; every sum starts from its first product and continues with
 * FMAs in ascending tap order, so a radius of 0 with tap 1.0f is the identity on that axis bit for bit.  ws holds
 * dwn_blur3d_ws_bytes(a) = B T H W floats (4-byte aligned) and must not overlap src or dst; dst may be src, the same channel included (the second launch reads ws only).
 *
 * dwn_clip_moments: stat[b][4] = {n, mean, M2 = sum (x - mean)^2, S2 = sum x^2} in float64 over the n = T wh ww window elements of
 * channel c of clip b.  One workgroup per (clip, chunk of DWN_MOMENTS_CHUNK elements) writes {sum, sum (x - chunk mean)^2, sum x^2}
 * to ws (dwn_clip_moments_ws_bytes(a) bytes, 8-byte aligned); one workgroup per clip folds them in a fixed order:
 * mean = (sum of sums) / n, M2 = sum_chunks (M2_c + n_c (mean_c - mean)^2).  M2 is never formed from raw sums.  A constant clip
 * returns its constant as the mean bit for bit and M2 == 0.
 *
 * dwn_mei_update, in place on the window of channel c of x; stat is the [B][4] table above, read on the device:
 *   DWN_MEI_STEP     x = (float)((double)x + (double)*lr * g * c_b),  c_b = 1 / sqrt(S2_b / n) from the moments of g (channel c_g of
 *                    g [B][Cin_g][T][H][W]); a clip with S2_b == 0 is not written.  lr is a device scalar.
 *   DWN_MEI_PROJECT  sd = sqrt(M2 / n), m = has_mean ? mean_target : mu,
 *                    s = has_contrast ? (FIXED: sd == 0 ? 0 : contrast / sd;  MAX: sd == 0 ? 1 : min(1, contrast / sd)) : 1,
 *                    x = clamp((float)(m + s * ((double)x - mu)), lo, hi) from the moments (mu, M2) of x itself; a clip with
 *                    s == 1 and m == mu (as doubles) is only clamped.
 * A clip whose statistics are not finite becomes NaN inside its window; other clips are untouched.  Pixels outside the window are
 * never written. */
#define DWN_BLUR_MAX_RADIUS 16
#define DWN_BLUR_TAPS_STRIDE (2 * DWN_BLUR_MAX_RADIUS + 1)
#define DWN_MOMENTS_CHUNK 4096
enum { DWN_MEI_STEP = 0, DWN_MEI_PROJECT = 1 };
enum { DWN_MEI_CONTRAST_MAX = 0, DWN_MEI_CONTRAST_FIXED = 1 };
typedef struct dwn_blur3d_args {
    int B, T, H, W;
    int Cin_src, c_src, Cin_dst, c_dst;
    int Rt, Rh, Rw;
    int y0, x0, wh, ww;
    int pad_;
    const float* src;
    float* dst;
    const float* taps;        /* device: float[3][DWN_BLUR_TAPS_STRIDE] */
    void* ws; size_t ws_bytes;
} dwn_blur3d_args;
typedef struct dwn_clip_moments_args {
    int B, Cin, T, H, W, c;
    int y0, x0, wh, ww;
    const float* x;
    double* stat;             /* [B][4] */
    void* ws; size_t ws_bytes;
} dwn_clip_moments_args;
typedef struct dwn_mei_update_args {
    int mode;                 /* DWN_MEI_STEP / DWN_MEI_PROJECT */
    int B, Cin, T, H, W, c;
    int y0, x0, wh, ww;
    int Cin_g, c_g;           /* STEP: the layout of g */
    int has_mean, has_contrast, contrast_mode;
    float lo, hi;
    double mean_target, contrast;
    float* x;
    const float* g;           /* STEP */
    const double* stat;       /* [B][4]: of g (STEP), of x (PROJECT) */
    const float* lr;          /* STEP: device scalar */
} dwn_mei_update_args;
size_t dwn_blur3d_ws_bytes(const dwn_blur3d_args* a);
size_t dwn_clip_moments_ws_bytes(const dwn_clip_moments_args* a);
int dwn_blur3d(const dwn_blur3d_args* a, int device, void* stream);
int dwn_clip_moments(const dwn_clip_moments_args* a, int device, void* stream);
int dwn_mei_update(const dwn_mei_update_args* a, int device, void* stream);

/* ---- trial-level evaluation: per-neuron scores of ONE mouse over whole trials of different length, some of which
 * repeat the same video.  Trial i has a prediction and a target row per neuron; a row is `frames` contiguous fp32 values that start
 * `first` elements into a row of stride ld (elements), so a frame cut is an offset and nothing is copied.  Row starts need 4-byte
 * alignment only: every load is one fp32.  The trials of a group are consecutive in the trial table and have the group's `frames`;
 * a trial that repeats nothing is a group of repeats = 1.  Both tables live in DEVICE memory and are validated by the caller (every
 * row they describe must lie inside its allocation); an entry beyond n_trials, max_repeats or max_frames is not followed.
 *
 * state: double [DWN_TRIAL_STATE_ROWS][N], zero before the first launch; with d.. deviations from the mean of the row's own set:
 *   set A, all (trial, frame), count n_all:                 0 mean_p   1 mean_y   2 M2p   3 M2y   4 C = sum dp dy
 *   set B, the (group, repeat, frame) of groups with repeats >= 2, count n_repeat:
 *                                                           5 mean_y   6 M2y   7 SSres = sum (y - p)^2
 *                                                           8 SSwithin = sum_(g,t) [sum_r (y - ybar_gt)^2] / (R_g - 1)
 *   set C, the (group, frame) averages over repeats, count n_group_frames:
 *                                                           9 mean_pbar   10 mean_ybar   11 M2pbar   12 M2ybar   13 Cbar
 *   set D, the leave-one-out mean loo = (R ybar - y) / (R - 1) over the elements of set B (mean_y and M2y are rows 5, 6):
 *                                                           14 mean_loo   15 M2loo   16 C_y_loo = sum dy dloo
 * dwn_trial_moments: needs trials, groups, state.  One wave owns one neuron for the whole launch (DWN_TRIAL_TILE neurons per
 *   workgroup), its lanes run along the frames and loop over the repeats of a frame, so the averages over repeats, the within-frame
 *   variance and the leave-one-out terms need no traffic between lanes.  Per group: the group means in a first sweep, then in a
 *   second sweep (from cache) the frame means and the sums of deviations from them and of the frame means from the group mean,
 *   float64 throughout; the lanes' partials are added by a fixed butterfly.  The groups are taken in table order and merged into the
 *   state the launch finds with the pairwise (Chan) formulas; an empty side is copied, not divided by.  n_all, n_repeat and
 *   n_group_frames are the counts of the state BEFORE the launch; the caller advances them by what its tables hold (sum R K, and
 *   for R >= 2 sum R K and sum K) and passes the advanced counts to the next launch and to dwn_trial_score_finalize.  No atomics, no
 *   raw sum of squares: launches, splits into several launches at group boundaries, and both builds give the same bits.
 * dwn_trial_score_finalize: needs state, scores, summary, ws; the counts are those AFTER the last launch.
 *   scores: double [DWN_TRIAL_SCORE_ROWS][N]; with pearson(Ma, Mb, Cab, n) = (Cab/n) / ((sqrt(Ma/n) + eps)(sqrt(Mb/n) + eps)):
 *   0 single_trial_corr = pearson(M2p, M2y, C, n_all)            1 corr_to_average = pearson(M2pbar, M2ybar, Cbar, n_group_frames)
 *   2 fev = (TV - NV) / TV   3 feve = 1 - (MSE - NV) / (TV - NV)   with TV = M2y_B / (n_repeat - 1), NV = SSwithin / n_group_frames,
 *   MSE = SSres / n_repeat; NaN where TV <= 0 or TV - NV <= 0      4 oracle_corr = pearson(M2y_B, M2loo, C_y_loo, n_repeat)
 *   A score whose count is 0 is NaN.  summary: double [DWN_TRIAL_SUMMARY] = mean over all N neurons of rows 0, 1, 4 (a NaN neuron
 *   makes the mean NaN), the mean of feve over the neurons with fev >= fev_threshold, the number of those neurons, n_all, n_repeat,
 *   n_group_frames: one partial per workgroup into ws (dwn_trial_score_ws_bytes(a) bytes, 8-byte aligned), folded by a
 *   one-workgroup launch in a fixed order.
 * Nothing is allocated and nothing is read back.  Argument errors are answered before the device is entered: null pointer -1;
 * geometry -2 (N, the table sizes, max_repeats, max_frames, counts that are negative or contradict each other, eps <= 0, a NaN
 * threshold); workspace too small or misaligned -3.  dwn_trial_score_ws_bytes returns 0 for arguments the entries would refuse. */
#define DWN_TRIAL_STATE_ROWS 17
#define DWN_TRIAL_SCORE_ROWS 5
#define DWN_TRIAL_SUMMARY 8
#define DWN_TRIAL_TILE 4
typedef struct dwn_trial_desc {
    const float* pred;
    const float* target;
    long long ld_pred, ld_target;     /* elements between consecutive neurons' rows */
    int first, frames;                /* the kept frames of a row: [first, first + frames) */
} dwn_trial_desc;
typedef struct dwn_trial_group {
    int first_trial, repeats, frames;
} dwn_trial_group;
typedef struct dwn_trial_score_args {
    int N, n_trials, n_groups;
    int max_repeats, max_frames;      /* upper bounds of the group table's repeats and frames */
    int pad_;
    long long n_all, n_repeat, n_group_frames;
    double eps;                       /* finalize: added to each standard deviation (> 0) */
    double fev_threshold;             /* finalize */
    const dwn_trial_desc* trials;     /* device, [n_trials] */
    const dwn_trial_group* groups;    /* device, [n_groups] */
    double* state;
    double* scores;
    double* summary;
    void* ws; size_t ws_bytes;
} dwn_trial_score_args;
size_t dwn_trial_score_ws_bytes(const dwn_trial_score_args* a);
int dwn_trial_moments(const dwn_trial_score_args* a, int device, void* stream);
int dwn_trial_score_finalize(const dwn_trial_score_args* a, int device, void* stream);

/* ---- retinotopic readout gain: a per-neuron gain on a readout's output, driven by the core map sampled at the
 * neuron's own learned position.  y, out, dout, dy: [B][N][T] fp32 contiguous; g: [B][T][Hf][Wf][K] channels-last in g_dtype
 * (DWN_F32 / DWN_BF16); dg: the same shape, always fp32; pos, dpos: [N][2] = (x, y) in normalised coordinates (-1 / +1 are the
 * centres of the first / last cell); weight, dweight: [N][K]; bias, dbias: [N]; m = max_log_gain.
 *   px = (clamp(x, -1, 1) + 1) / 2 * (Wf - 1),  x0 = min(floor(px), max(Wf - 2, 0)),  fx = px - x0,  x1 = min(x0 + 1, Wf - 1)
 *   (y likewise with Hf);  w00 = (1-fy)(1-fx), w01 = (1-fy) fx, w10 = fy (1-fx), w11 = fy fx       (fp32, each product rounded once)
 *   d_c[b,n,t] = sum_k G[b,t,cell_c,k] weight[n,k]        (fp32 FMAs, k ascending, from 0; c = 00, 01, 10, 11)
 *   a          = bias[n] + w00 d00 + w01 d01 + w10 d10 + w11 d11                     (4 FMAs in that order, from bias[n])
 *   out        = y exp(m tanh(a))
 * which is F.grid_sample(bilinear, border, align_corners=True) followed by the behaviour modulator's gain.  Backward:
 *   dy = dout gain,  s = dout y gain m sech^2(a)  (sech^2 = 4 e / (1 + e)^2, e = exp(-2 |a|)),
 *   dbias[n] = sum_{b,t} s,  dweight[n,k] = sum_{b,t} s samp[k],  samp[k] = sum_c w_c G[b,t,cell_c,k],
 *   dpos[n,0] = (Wf - 1)/2 sum_{b,t} s ((1-fy)(d01 - d00) + fy (d11 - d10)),  dpos[n,1] likewise with Hf and fx,
 *   dg[b,t,cell,k] = sum over the neurons n one of whose corners c is `cell`, n ascending, of s w_c weight[n,k].
 * A coordinate strictly outside [-1, 1] is clamped and its dpos entry is exactly 0 (the other coordinate stays live); a one-cell
 * axis (Hf = 1 or Wf = 1) has a zero position gradient.  One decision per neuron: cells, weights and flags are derived once per call
 * (the backward writes them into ws and every pass reads that table; the neurons of every cell are bucketed from it, in index order).  The sums over (b, t) run in float64 through per-workgroup
 * partials in ws and a fixed-order finaliser and are rounded to fp32 once; dg is a float64 sum in ascending neuron order rounded
 * once, written for every cell (exact zeros where no neuron reaches).  No atomics: the same inputs give the same bits, in both
 * builds.  A null dy / dg / dpos / dweight / dbias is skipped, and its partials are neither computed nor stored.
 * A neuron whose position holds a NaN or an Inf gets NaN in its rows of out and dy and in its dweight, dbias and dpos, is left out
 * of dg, and leaves every other neuron's results bit for bit what they are without it.  weight = bias = 0 returns y (and dout in
 * dy) bit for bit.  dwn_spatial_gain_forward needs y, g, pos, weight, bias, out (out must not alias y) and no workspace.
 * dwn_spatial_gain_backward needs y, g, pos, weight, bias, dout, ws (dwn_spatial_gain_ws_bytes(a) bytes, 16-byte aligned; it depends
 * on the sizes B, N, T, Hf * Wf, K alone) and at least one of dy, dg, dpos, dweight, dbias.  Nothing is allocated and nothing is read back: both
 * entries can be captured.  Argument errors are answered before the device is entered: null pointer -1; a non-positive size, K
 * outside [1, 64], Hf * Wf > 256, a g_dtype that is neither DWN_F32 nor DWN_BF16, a max_log_gain that is not finite and positive,
 * out == y, or a workspace that is too small or misaligned -2. */
typedef struct dwn_spatial_gain_args {
    int B, N, T, Hf, Wf, K;
    int g_dtype; float max_log_gain;
    const float* y; const void* g; const float* pos; const float* weight; const float* bias;
    float* out;
    const float* dout; float* dy; float* dg; float* dpos; float* dweight; float* dbias;
    void* ws; size_t ws_bytes;
} dwn_spatial_gain_args;
size_t dwn_spatial_gain_ws_bytes(const dwn_spatial_gain_args* a);   /* backward only; forward needs none; 0 for refused arguments */
int dwn_spatial_gain_forward(const dwn_spatial_gain_args* a, int device, void* stream);
int dwn_spatial_gain_backward(const dwn_spatial_gain_args* a, int device, void* stream);

/* ---- receptive-field mapping: a counter-based noise stimulus, the lagged stimulus/response cross-sums of a
 * batch, and the maps they give.
 *
 * dwn_noise_forward: x, out [B][Cin][T][H][W] fp32 contiguous.  Channel `video_channel` is rendered, every other channel is copied
 * from x bit for bit.  The window (y0, x0, wh, ww) — always explicit — holds gh x gw = (wh / cell) x (ww / cell) cells; cell
 * q = gy gw + gx of frame t of clip b takes word q & 3 of
 *   philox4x32-10(counter = (q >> 2, t / hold, first_clip + b, 0), key = (seed & 0xffffffff, seed >> 32))
 * (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85; round c' = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2),
 * hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))).  DWN_NOISE_BINARY: top bit set -> background + contrast, else background - contrast.
 * DWN_NOISE_SPARSE: thr = floor(density 2^31); word < thr -> background - contrast, word >= 2^32 - thr -> background + contrast,
 * else background.  The three values are formed once in fp32 and never clamped; pixels outside the window hold `pad`.  A clip
 * depends on (seed, first_clip + b) alone.  Needs x, out.
 *
 * dwn_sta_accumulate: x [B][Cin][T][H][W] fp32 (any stimulus), r [B][N][T] fp32, r0 [N] fp32 or NULL (zeros).  With G = gh gw,
 *   u[b,n,t] = r[b,n,t] - r0[n]                                                     (fp32)
 *   v[b,t,g] = (sum of the cell's pixels of channel `channel`, fp32, row-major) * (1 / cell^2) - s0    (each step rounded)
 *   t0 = max(skip, lags - 1);   for t in [t0, T):
 *   Cuv[n][l][g] += sum_b sum_t u[b,n,t] v[b,t-l,g]      (an fp32 fma chain over (b, t) ascending, converted once, added in float64)
 *   U1[n] += sum u, U2[n] += sum u^2;  V1[l][g] += sum v[b,t-l,g], V2[l][g] += sum v^2      (float64 sums in a fixed order)
 * state: double, zero before the first call: Cuv [N][lags][G], then U1 [N], U2 [N], V1 [lags][G], V2 [lags][G]
 * (dwn_sta_state_bytes(a) bytes, 8-byte aligned).  Every element has one owner and a fixed order: no atomics, no scratch, the same
 * bits on every launch and in both builds.  The caller advances its sample count by B (T - t0) per call.  A non-finite response of
 * a neuron reaches only that neuron's rows and its U1 / U2; a non-finite pixel only that cell's columns and its V1 / V2.
 * Needs x, r, state.
 *
 * dwn_sta_finalize: with K = samples (> 0), per (n, l, g) in float64
 *   cov = (Cuv - U1 (V1 / K)) / K,   var_u = (U2 - U1 (U1 / K)) / K,   var_v = (V2 - V1 (V1 / K)) / K,
 *   z = cov sqrt(K) / sqrt(var_u var_v), 0 where either variance is <= 0;
 * cov, z: fp32 [N][lags][gh][gw] (z may be NULL).  summary: double [N][DWN_STA_SUMMARY]:
 *   0 peak lag l* = argmax_l E_l, E_l = sum_g cov^2 (lowest lag wins a tie)   1 z at the argmax-|cov| cell of l* (lowest index wins)
 *   2, 3 cy, cx: centroid in cell units, weights cov^2, over the cells of l* with |cov| >= rel_threshold max_g |cov|
 *   4, 5 sy, sx: weighted standard deviations about it   6 E_l* / sum_l E_l   7 the number of cells kept
 * A neuron whose sum_l E_l is not positive gets lag 0, z 0, NaN in columns 2-5, share 0 and count 0.  One wave per neuron, the
 * lanes' partials added by a fixed butterfly; V1 / K and var_v are formed once into ws (dwn_sta_ws_bytes(a) bytes, 8-byte
 * aligned) by a launch of their own.  Needs state, cov, summary, ws.
 *
 * Nothing is allocated and nothing is read back.  Argument errors are answered before the device is entered: null pointer -1;
 * geometry -2 (a non-positive size, a channel outside [0, Cin), a window not inside the plane, a cell that does not divide the
 * window, hold < 1, an unknown kind, density outside [0, 1], first_clip + B > 2^32, lags < 1, skip < 0, t0 >= T, samples < 1, a
 * rel_threshold outside [0, 1], a misaligned state / summary); workspace too small or misaligned -3.  The size queries return 0 for
 * arguments the entries would refuse. */
enum { DWN_NOISE_BINARY = 0, DWN_NOISE_SPARSE = 1 };
#define DWN_STA_SUMMARY 8
typedef struct dwn_noise_args {
    int B, Cin, T, H, W;
    int video_channel;
    int kind;                 /* DWN_NOISE_BINARY / DWN_NOISE_SPARSE */
    int cell, hold;
    int y0, x0, wh, ww;
    int pad_;
    float background, contrast, density, pad;
    unsigned long long seed;
    long long first_clip;     /* 0 <= first_clip, first_clip + B <= 2^32 */
    const float* x;
    float* out;
} dwn_noise_args;
int dwn_noise_forward(const dwn_noise_args* a, int device, void* stream);

typedef struct dwn_sta_args {
    int B, Cin, T, H, W, N;
    int channel;
    int y0, x0, wh, ww, cell;
    int lags, skip;
    float s0;
    int pad_;
    long long samples;        /* finalize: K */
    double rel_threshold;     /* finalize */
    const float* x;
    const float* r;
    const float* r0;          /* [N] or NULL */
    double* state;
    float* cov;
    float* z;                 /* may be NULL */
    double* summary;
    void* ws; size_t ws_bytes;
} dwn_sta_args;
size_t dwn_sta_state_bytes(const dwn_sta_args* a);
size_t dwn_sta_ws_bytes(const dwn_sta_args* a);
int dwn_sta_accumulate(const dwn_sta_args* a, int device, void* stream);
int dwn_sta_finalize(const dwn_sta_args* a, int device, void* stream);

/* ---- parametric receptive-field fits: an elliptical Gaussian per map by Levenberg-Marquardt, and the temporal
 * profile of a lagged map on that spatial shape.
 *
 * dwn_gauss2d_fit: maps fp32 [R][gh][gw] contiguous; sel int32 [M] device table of rows of `maps`, or NULL (rows 0 .. M-1, which
 * needs M <= R).  With y, x the row and column index of a cell, dx = x - cx, dy = y - cy,
 *   f = b + a exp(-q / 2),   q = (l11 dx)^2 + (l21 dx + l22 dy)^2,   p = (b, a, cy, cx, log l11, l21, log l22)
 * (the Cholesky factor of the precision matrix).  Start: b0 = mean of the perimeter cells (0 and held with fit_baseline = 0);
 * d = m - b0; peak = argmax |d| (lowest index on a tie), a0 = d[peak]; centre and (sy, sx) = the d^2-weighted centroid and standard
 * deviations over the cells with |d| >= rel_threshold |a0|, each sigma floored at 0.5; l11 = 1 / sx, l22 = 1 / sy, l21 = 0.
 * Iteration: Levenberg-Marquardt on S = sum (m - f)^2, analytic Jacobian; (JtJ + lam diag JtJ) dp = Jt r by Cholesky, lam from
 * 1e-3; the proposal is clamped (centre to [-1, gh] x [-1, gw], the two logs so that 1 / l stays in [0.3, 2 max(gh, gw)]); with
 * the step scaled by (|a|, |a|, 1, 1, 1, 1, 1), a largest scaled step below xtol converges; a proposal is accepted only if its S
 * is finite and strictly smaller (lam = max(lam / 10, 1e-12); converged if the decrease is <= ftol S), otherwise lam *= 10, at
 * most 16 tries per iteration (a Cholesky failure is a try).  All arithmetic is float64; every sum over the cells is lane-strided
 * and closed by a fixed xor butterfly, so a row depends on its map and the options alone — not on M, sel, the launch or the build.
 * params double [M][DWN_GAUSS_PARAMS] = p.  table double [M][DWN_GAUSS_TABLE]:
 *   0 status (0 converged, 1 stopped at max_iter or out of tries, 2 no fit)   1 iterations   2 baseline   3 amplitude   4 cy   5 cx
 *   6 sigma_major   7 sigma_minor   8 theta (major axis from the x axis, (-pi/2, pi/2])   9 sse   10 r2 = 1 - S / SS_tot about the
 *   map's mean (0 where SS_tot is 0)   11, 12, 13 se_cy, se_cx, se_amplitude = sqrt(C_ii S / (G - n_par)), C = (JtJ)^-1 at the
 *   solution (NaN where JtJ is not positive definite)   14 lambda   15 row (the row of `maps` that was fitted)
 * Status 2: a constant map, a non-finite value in the map, a0 == 0, or a row outside [0, R): baseline and sse if they are finite
 * (else NaN), amplitude 0, iterations 0, r2 0, lambda 0, NaN in the geometry and standard-error columns and in params 2-6.
 * ws: dwn_gauss2d_ws_bytes(a) bytes, 8-byte aligned: double [M][8], the start vector p0 and S(p0) of every row.
 *
 * dwn_gauss2d_profile: params double [N][DWN_GAUSS_PARAMS] (of dwn_gauss2d_fit), maps fp32 [N][L][gh][gw].  With
 * e_g = exp(-q_g / 2) at the row's params, per lag the linear least-squares fit m_l ~ b_l + a_l e (fit_baseline = 0: a_l e):
 * profile double [N][L] = a_l; separability double [N] = 1 - sum_l SSE_l / sum_l SStot_l with SStot_l about the lag's mean
 * (fit_baseline = 0: about 0), 0 where the denominator is 0.  A row whose params hold a NaN (status 2) gives NaN in both.  One
 * wave per neuron, float64 sums in a fixed order.
 *
 * Errors: null pointer -1; geometry -2 (gh < 3, gw < 3, gh gw > 4096, M < 1, R < 1, sel NULL with M > R, max_iter < 0, a
 * rel_threshold outside [0, 1], xtol or ftol negative or NaN, N or L < 1, misaligned params / table / profile); workspace too small
 * or misaligned -3.  dwn_gauss2d_ws_bytes returns 0 for a geometry the entry refuses. */
#define DWN_GAUSS_PARAMS 7
#define DWN_GAUSS_TABLE 16
typedef struct dwn_gauss2d_args {
    int R, gh, gw, M;
    int fit_baseline, max_iter;
    double rel_threshold, xtol, ftol;
    const float* maps;
    const int* sel;           /* device [M] or NULL */
    double* params;
    double* table;
    void* ws; size_t ws_bytes;
} dwn_gauss2d_args;
size_t dwn_gauss2d_ws_bytes(const dwn_gauss2d_args* a);
int dwn_gauss2d_fit(const dwn_gauss2d_args* a, int device, void* stream);

typedef struct dwn_gauss2d_profile_args {
    int N, L, gh, gw;
    int fit_baseline, pad_;
    const double* params;
    const float* maps;
    double* profile;
    double* separability;
} dwn_gauss2d_profile_args;
int dwn_gauss2d_profile(const dwn_gauss2d_profile_args* a, int device, void* stream);

/* ---- population structure: the N x N correlation matrices of ONE mouse over whole trials, and their comparison.
 * The frame cut and the grouping are those of the trial scores above: segment i is one fp32 row per neuron, `frames` contiguous
 * values that start `first` elements into a row of stride ld (4-byte alignment only, every load is one fp32); the segments of a
 * group are consecutive in the segment table and have the group's `frames`; the group table is a dwn_trial_group table (a trial
 * that repeats nothing is a group of repeats = 1).  Both tables live in DEVICE memory and are validated by the caller; an entry
 * beyond n_segs, max_repeats or max_frames is not followed.  With ybar[g][f] = (1/R) sum_r y[r][f] (float64, repeats in table
 * order) the three sample sets are
 *   DWN_PAIR_TOTAL   every (trial, frame), value y;                              a CHUNK is one trial, K values
 *   DWN_PAIR_SIGNAL  the (group, frame) of groups with R >= 2, value ybar;       a chunk is one group, K values
 *   DWN_PAIR_NOISE   the (group, repeat, frame) of those groups, value y - ybar; a chunk is one group, R K values (repeat-major)
 * The noise set takes NO degrees-of-freedom correction: its co-moment is divided by its sample count R K like the others.
 *
 * state: double [N][N] C, then double [N] mean (dwn_pair_state_bytes(a) bytes, 8-byte aligned, zero before the first launch):
 * C_ij = sum (x_i - mean_i)(x_j - mean_j) over the samples so far, stored full and bit-symmetric.  The caller keeps the sample
 * count n (the state's BEFORE a stage launch, AFTER the last one for finalize) and advances it by what its tables hold.
 *
 * dwn_pair_stage: needs segs, groups, state, ws.  Writes Z = double [cols][ldz] into ws, k-major: column k holds ldz =
 *   dwn_pair_ldz(N) = N rounded up to DWN_PAIR_TILE neurons, contiguous, zero beyond N.  Per chunk, in table order: the chunk's
 *   mean m_b (a first sweep in a fixed order, float64), its n_b values centred about m_b (a second sweep; never a raw sum), one
 *   merge column sqrt(n_a n_b / (n_a + n_b)) (m_b - m_a) with m_a, n_a the running mean and count (0 for an empty state, whose
 *   mean becomes m_b), zero columns up to the next multiple of DWN_PAIR_KSTEP, and mean += (m_b - m_a) n_b / (n_a + n_b).  So
 *   Z Z^T is exactly the pairwise (Chan) merge of the chunks and the product knows nothing about chunks.  cols = the sum over
 *   the chunks of (n_b + 1) rounded up to DWN_PAIR_KSTEP; a chunk that would pass `cols` is not followed.
 * dwn_pair_syrk: needs state, ws (Z as staged).  C += Z Z^T in float64 on v_mfma_f64_16x16x4_f64.  Only the tiles on and below
 *   the diagonal are computed and their owner writes the mirror; every element has one accumulator that starts from C and walks
 *   the columns in ascending order, K is never split: given the same chunks the state's bits do not depend on how the caller
 *   cuts them into launches.
 * dwn_pair_corr_finalize: needs state, out.  out[i][j] = (C_ij / n) / ((sqrt(C_ii / n) + eps)(sqrt(C_jj / n) + eps)) in float64,
 *   stored as double or (out_f32) rounded once to fp32; [N][N] contiguous, apart from the state.  n == 0 gives NaN everywhere, a
 *   constant neuron a row and a column of exact zeros.
 * A non-finite value of neuron i reaches only row i and column i of C and of out (and mean[i]).
 *
 * dwn_pair_compare: A (model), B (data) double [N][N] with leading dimensions lda, ldb; sel int32 [M] device table of neurons or
 *   NULL (neurons 0 .. M-1, which needs M <= N).  per_neuron double [M]: for the selected neuron i the Pearson correlation (the
 *   convention above, with eps) of A[i][j] with B[i][j] over the selected j != i: one wave per row, centred float64 moments in
 *   two sweeps closed by a fixed butterfly.  summary double [DWN_PAIR_SUMMARY]: 0 the number of ordered pairs, 1 the Pearson
 *   correlation over all of them, 2, 3 mean of A, B, 4, 5 their standard deviations, 6 mean |A - B|, 7 RMS of A - B; the row
 *   moments (DWN_PAIR_ROW_STATS doubles per row in ws, dwn_pair_compare_ws_bytes(a) bytes, 8-byte aligned) are merged in row
 *   order with the pairwise formulas by one workgroup.  A NaN entry makes its row's score and the summary NaN, as does a sel
 *   entry outside [0, N); nothing is skipped silently.  M = 1 has no pair: NaN.
 *
 * Nothing is allocated and nothing is read back; no atomics, no scratch; both builds give the same bits.  Argument errors are
 * answered before the device is entered: null pointer -1; geometry -2 (N outside [1, 65535], an unknown kind, table sizes,
 * max_repeats, max_frames, cols not a positive multiple of DWN_PAIR_KSTEP, a negative count or one at or above 2^52, eps <= 0, M
 * outside [1, N] (sel NULL) or [1, 2^20], a leading dimension below N, a misaligned state / out / matrix); workspace too small or
 * misaligned (16 bytes for Z) -3.  The size queries return 0 for arguments the entries would refuse. */
enum { DWN_PAIR_TOTAL = 0, DWN_PAIR_SIGNAL = 1, DWN_PAIR_NOISE = 2 };
#define DWN_PAIR_TILE 64
#define DWN_PAIR_KSTEP 4
#define DWN_PAIR_SUMMARY 8
#define DWN_PAIR_ROW_STATS 8
typedef struct dwn_pair_seg {
    const float* x;
    long long ld;                     /* elements between consecutive neurons' rows */
    int first, frames;                /* the kept frames of a row: [first, first + frames) */
} dwn_pair_seg;
typedef struct dwn_pair_args {
    int N, kind;                      /* DWN_PAIR_TOTAL / _SIGNAL / _NOISE (stage) */
    int n_segs, n_groups;
    int max_repeats, max_frames;      /* upper bounds of the group table's repeats and frames */
    int cols;                         /* columns of Z */
    int out_f32;                      /* finalize: out is fp32 */
    long long n;                      /* samples of the state: before the launch (stage), after the last one (finalize) */
    double eps;                       /* finalize: added to each standard deviation (> 0) */
    const dwn_pair_seg* segs;         /* device, [n_segs] */
    const dwn_trial_group* groups;    /* device, [n_groups] */
    double* state;
    void* out;
    void* ws; size_t ws_bytes;
} dwn_pair_args;
typedef struct dwn_pair_compare_args {
    int N, M;
    long long lda, ldb;
    double eps;
    const double* A;
    const double* B;
    const int* sel;                   /* device [M] or NULL */
    double* per_neuron;
    double* summary;
    void* ws; size_t ws_bytes;
} dwn_pair_compare_args;
long long dwn_pair_ldz(int N);                                   /* 0 for an N the entries refuse */
size_t dwn_pair_state_bytes(const dwn_pair_args* a);
size_t dwn_pair_ws_bytes(const dwn_pair_args* a);                /* Z: cols * dwn_pair_ldz(N) doubles */
size_t dwn_pair_compare_ws_bytes(const dwn_pair_compare_args* a);
int dwn_pair_stage(const dwn_pair_args* a, int device, void* stream);
int dwn_pair_syrk(const dwn_pair_args* a, int device, void* stream);
int dwn_pair_corr_finalize(const dwn_pair_args* a, int device, void* stream);
int dwn_pair_compare(const dwn_pair_compare_args* a, int device, void* stream);

/* ---- Population modes (ABI 7, appended; csrc/dwn_modes.hip): the k leading eigenpairs of a symmetric N x N float64
 * matrix `scale * A` by block subspace iteration with Rayleigh-Ritz extraction, stage by stage and as one driver, and the principal
 * angles between two subspaces.  A: double [N][lda], lda >= N, SYMMETRIC (the product reads A[j][i] where it needs A[i][j]; for an
 * unsymmetric A it computes A^T Q), intended positive semi-definite up to rounding (for an indefinite matrix the iteration finds the
 * subspace dominant in magnitude).  A block is double [N][ld] with ld >= p rounded up to 16; columns [p, p rounded up to 16) are
 * written as zeros by every entry that writes a block.  Small matrices (H, W) are double [p][DWN_MODES_MAXP] row-major.
 *
 * dwn_modes_symm: needs A, Q, Y.  Y = scale * A Q on v_mfma_f64_16x16x4_f64; the sum over j is cut into four quarters of
 *   ((N + 3) / 4 rounded up to 4) terms, each summed in ascending j, and the quarters are added in ascending order.
 * dwn_modes_moments: needs A, moments, ws (dwn_modes_moments_ws_bytes).  moments[0] = scale * sum_i A_ii, moments[1] = scale^2 *
 *   sum_ij A_ij^2, both in float64 in a fixed order (rows strided over 256 threads and closed by a fixed tree).
 * dwn_modes_orth: needs Y, Q (Q may be Y).  Q = orth(Y) by classical Gram-Schmidt applied twice, column by column; a column whose
 *   norm after the projections is at most DWN_MODES_ORTH_C * N * 2^-53 * ||Y||_F becomes an exact zero column.  A NaN stays a NaN.
 * dwn_modes_small_eigh: needs H, W, values.  The eigenpairs of the symmetric p x p matrix H (both triangles are read) by cyclic
 *   Jacobi in one workgroup, at most 30 sweeps: values[DWN_MODES_MAXP] descending (zero beyond p), column c of W the eigenvector
 *   of values[c] with its entry of largest magnitude (lowest index on ties) positive.  A non-finite H gives NaN values and NaN W.
 * dwn_modes_ritz: needs Q, Y, values (theta, as small_eigh wrote them), W, V, residuals, status, ws (dwn_modes_ritz_ws_bytes).
 *   V = Q W, residuals[c] = ||Y W e_c - theta_c V e_c||_2, then status[0] (done) = status[1] (converged) = 1 when
 *   max_{i < k} residuals[i] <= tol * |theta_0|; status[2] (rounds) = 1.  status is int32 [4].
 * dwn_modes_solve: needs A, V, values, residuals, moments, status, ws (dwn_modes_solve_ws_bytes).  The start block (entry (i, c) =
 *   ((double) w + 0.5) * 2^-31 - 1 with w word c & 3 of philox4x32-10(counter = (i, c >> 2, 0, 0), key = (seed & 0xffffffff, seed
 *   >> 32))), its orth, the moments, Q = orth(scale A Q) once, then max_iters rounds of symm, H = sym(Q^T Y), small_eigh, ritz, Q = orth(Y) on one stream;
 *   the decision is taken on the device and the kernels of the rounds after it return at once: nothing is read back.  At the
 *   end the sign rule is applied to the columns of V.  A NaN or Inf in A gives NaN values and converged = 0.
 * dwn_modes_overlap: needs Q (Va), Y (Vb), k, values, ws (dwn_modes_overlap_ws_bytes); values[k] = the singular values of Va^T Vb,
 *   descending, as the square roots of the eigenvalues of (Va^T Vb)^T (Va^T Vb).  With A (B of the comparison) also moments:
 *   [0], [1] as dwn_modes_moments of B and moments[2] = tr(Va^T (scale B) Va).
 *
 * Errors, answered before the device is entered: -1 null pointer; -2 N outside [1, 65535], p outside [1, min(N, DWN_MODES_MAXP)], k
 * outside [1, p], a leading dimension too small, max_iters < 1, scale or tol not finite, tol < 0, misaligned pointer; -3 workspace
 * too small or not 16-byte aligned.  The size queries return 0 for what the entries refuse. */
#define DWN_MODES_MAXP 64
#define DWN_MODES_ORTH_C 8.0
typedef struct dwn_modes_args {
    int N, p, k, max_iters;           /* p: columns of the block, k <= p: the columns the decision looks at */
    long long lda, ldq, ldy, ldv;
    double scale, tol;
    unsigned long long seed;
    const double* A;
    double* Q;
    double* Y;
    double* V;
    double* H;
    double* W;
    double* values;                   /* [DWN_MODES_MAXP] */
    double* residuals;                /* [DWN_MODES_MAXP] */
    double* moments;                  /* [4]: trace, squared Frobenius norm, (overlap) captured numerator, unused */
    int* status;                      /* [4]: done, converged, rounds, unused */
    void* ws;
    size_t ws_bytes;
} dwn_modes_args;
size_t dwn_modes_moments_ws_bytes(const dwn_modes_args* a);
size_t dwn_modes_ritz_ws_bytes(const dwn_modes_args* a);
size_t dwn_modes_solve_ws_bytes(const dwn_modes_args* a);
size_t dwn_modes_overlap_ws_bytes(const dwn_modes_args* a);
int dwn_modes_symm(const dwn_modes_args* a, int device, void* stream);
int dwn_modes_moments(const dwn_modes_args* a, int device, void* stream);
int dwn_modes_orth(const dwn_modes_args* a, int device, void* stream);
int dwn_modes_small_eigh(const dwn_modes_args* a, int device, void* stream);
int dwn_modes_ritz(const dwn_modes_args* a, int device, void* stream);
int dwn_modes_solve(const dwn_modes_args* a, int device, void* stream);
int dwn_modes_overlap(const dwn_modes_args* a, int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DWN_H_ */
