// Prototypes of the glue-kernel launchers (dwn_elementwise.hip).  All return 0 or a negative/positive error code.
#pragma once
#include "dwn_internal.h"

struct ResGeom {
    int BT, T, Hin, Win, Hout, Wout, Cin, Cout;
    const int* hsrc; const int* wsrc;     // [Hout], [Wout]: nearest source index (dwiseneuro.py:127-129)
    const int* hinv; const int* winv;     // [Hin], [Win]: inverse map or -1
};

typedef dwn_tensor_entry TensorListEntry;

struct BnFinJob {
    const double* stats; int stat_c; double count; const float* gamma; const float* beta;
    float* running_mean; float* running_var; long long* nbt; float* coef; int C; int nblocks;
};
// frozen (dwn.h DWN_BN_FROZEN): abc = (scale, 0, 0), dgamma / dbeta from the same sums; count is not read
struct BnBwdJob { const double* stats; double count; const float* coef; float* dgamma; float* dbeta; float* abc; int C; int nblocks; int frozen; };
// one or two BatchNorms per launch: a job with C = 0 (BnFinJob{} / BnBwdJob{}) is no job; nblocks is the launcher's
int k_bn_finalize_train(BnFinJob j0, BnFinJob j1, float momentum, float eps, hipStream_t s);
int k_bn_bwd_finalize(BnBwdJob j0, BnBwdJob j1, hipStream_t s);
int k_bn_finalize_eval(const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                       float* coef, int C, hipStream_t s);
// BatchNorm-1 statistics from the Gram matrix of the block input (y1 never materialised; dwn_elementwise.hip)
// nrep = 1: one full matrix (the gemm_tn route); nrep = gram_nrep() > 1: the replicas of the streaming kernel (dwn_gram.hip: Cin = 64,
// upper tiles), summed in replica order
int k_bn1_gram_finalize(const double* gram, int nrep, const float* w1, int E, int Cin, double count, const float* gamma, const float* beta,
                        float* rm, float* rv, long long* nbt, float momentum, float eps, float* coef, double* sc_stats, int dtype,
                        hipStream_t s);
// the streaming Gram kernel (dwn_gram.hip): replicas per (dtype, Cin) — 1 where it is not built —, and its launcher (*done = false:
// not built for this shape, nothing launched, the caller takes the gemm_tn route)
#define DWN_GRAM_NREP 8
int gram_nrep(int dtype, int Cin);
int k_gram(const void* a0, i64 ld, i64 M, int Cin, double* gram, int dtype, bool* done, hipStream_t s);
int k_ew_apply(const LoadDesc& d, int kind, void* out, i64 ldo, i64 rows, int C, int dtype, hipStream_t s);
// stem through the input moments (no y0 round trip; dwn_elementwise.hip)
int k_stem_xmom(const float* x, int B, int Cin, i64 S, double* mom, hipStream_t s);
int k_stem_bn_finalize(const double* mom, double count, const float* w, const float* gamma, const float* beta, float* rm,
                       float* rv, long long* nbt, float momentum, float eps, float* coef, double* xmom, int C0, int Cin,
                       hipStream_t s);
int k_stem_out(const float* x, const float* w, const float* coef, const float* pe_t, const float* pe_h, const float* pe_w,
               int Tn, int H, int W, int B, int Cin, i64 S, int C0, void* out, int dtype, hipStream_t s);
int k_stem_bwd_acc(const void* dout, const float* x, const double* xmom, double count, int B, int Cin, i64 S, int C0,
                   double* acc, int dtype, hipStream_t s);
int k_stem_bwd_finalize(const double* acc, const double* xmom, const float* w, const float* coef, double count, float* dgamma,
                        float* dbeta, float* dw, int C0, int Cin, hipStream_t s);
int k_stem_bwd_finalize_frozen(const double* acc, const float* w, const float* coef, float* dgamma, float* dbeta, float* dw,
                               int C0, int Cin, hipStream_t s);
int k_stem_input_grad(const void* dout, const float* w, const float* coef, int B, int Cin, i64 S, int C0, float* dx, int dtype,
                      hipStream_t s);
// batch statistics: qx = Q [8][8], q0 [8], x̄ [8] (floats) from the finished sums; dx = frozen term + Q (x - x̄) + q0
int k_stem_bwd_finalize_dx(const double* acc, const double* xmom, const float* w, const float* coef, double count, float* qx,
                           int C0, int Cin, hipStream_t s);
int k_stem_input_grad_train(const void* dout, const float* w, const float* coef, const float* x, const float* qx, int B, int Cin,
                            i64 S, int C0, float* dx, int dtype, hipStream_t s);
int stem_moment_count();
int stem_acc_stride();
int k_shortcut_stats(const LoadDesc& xin, const ResGeom& gm, double* stats, int dtype, hipStream_t s);
int k_residual_fwd(const LoadDesc& xin, const void* y4, const float* coef4, const float* coefsc, const float* dscale,
                   const ResGeom& gm, const float* ope_t, const float* ope_h, const float* ope_w, void* out, int dtype,
                   hipStream_t s);
int k_residual_bwd_reduce(const LoadDesc& xin, const void* y4, const void* dout, const float* coef4,
                          const float* coefsc, const float* dscale, const ResGeom& gm, double* stats4,
                          double* statssc, int dtype, hipStream_t s);
int k_residual_bwd_dy4(const void* y4, const void* dout, const float* abc4, const float* dscale, const ResGeom& gm,
                       void* dy4, int dtype, hipStream_t s);
int k_residual_bwd_dx(const LoadDesc& xin, const void* da0, const void* dout, const float* abcsc, const ResGeom& gm,
                      void* dx, int dtype, hipStream_t s);
int k_se_pool(const LoadDesc& z3, int B, int C, int rows_per_sample, long long* pooled, void* z3out, int dtype, hipStream_t s);
int k_se_mlp_fwd(const long long* pooled_sum, float inv_s, const float* wr, const float* br, const float* we,
                 const float* be, int B, int C, int R, float* pmean, float* hid_pre, float* gate, const float* w2, void* wg, int N2,
                 int dtype, int* folded, hipStream_t s);
int k_se_mlp_bwd(const float* dg, const float* gate, const float* hid_pre, const float* pmean, const float* wr,
                 const float* we, int B, int C, int R, float inv_s, float* dgp, float* dhp, float* dps, float* dwr,
                 float* dbr, float* dwe, float* dbe, hipStream_t s, bool wgrad = true);
int k_bn3_bwd_reduce(const LoadDesc& d, const float* coef3, i64 rows, int C, double* stats, void* dh_out, int dtype, hipStream_t s);
int k_pool_fwd(const void* x, void* out, i64 BT, int HW, int C, int dtype, hipStream_t s);
int k_pool_bwd(const void* dpool, void* dx, i64 BT, int HW, int C, int dtype, hipStream_t s);
int k_cortex_residual_fwd(const void* y, const void* x, const float* coef, const float* coefsc, const float* dscale,
                          int M, int Tn, int Cin, int C, int groups, void* out, int dtype, hipStream_t s);
int k_cortex_stats(const void* y, const void* x, int M, int Cin, int C, double* stats, double* statssc, int dtype, hipStream_t s);
int k_cortex_bwd_reduce(const void* y, const void* x, const void* dout, const float* gmask, int gmask_ld,
                        const float* coef, const float* coefsc, const float* dscale, int M, int Tn, int Cin, int C,
                        int groups, double* stats, double* statssc, int dtype, hipStream_t s);
int k_cortex_bwd_dy(const void* y, const void* dout, const float* gmask, int gmask_ld, const float* coef,
                    const float* abc, const float* dscale, int M, int Tn, int C, int groups, void* dy, int dtype,
                    hipStream_t s);
int k_cortex_bwd_dx(const void* dxmain, const void* x, const void* dout, const float* gmask, int gmask_ld,
                    const float* abcsc, int M, int Tn, int Cin, int C, void* dx, int dtype, hipStream_t s);
int k_pack_weight(const float* src, void* dst, int groups, int R, int C, int transpose, int Rd, int Cd, int dtype,
                  hipStream_t s);
int k_gate_weights(const float* w, const float* gate, void* dst, int B, int N, int K, int dtype, hipStream_t s);
size_t k_readout_dbeta_parts(int B, int Rp, int groups);   // doubles of workspace the dbeta variant of k_readout_dz needs
int k_readout_dz(const float* dout, const float* out, float beta, const float* beta_dev, double* part, float* dbeta, int B, int Tn, int n_valid, int Rg, int Rp,
                 int groups, void* dz, float* db, int dtype, hipStream_t s);
int k_poisson_fwd(const float* pred, const float* target, const float* w, i64 per_sample, i64 total, float eps,
                  double* loss, hipStream_t s);
int k_poisson_bwd(const float* pred, const float* target, const float* w, const float* gscale, i64 per_sample,
                  i64 total, float eps, float* dpred, hipStream_t s);
int k_f64_to_f32(const double* src, float* dst, int n, hipStream_t s);
int k_adamw_ema(const TensorListEntry* list, int ntensors, int max_blocks, float decay_w, float omb1, float beta2,
                float omb2, float eps, float step_size, float bc2_sqrt, float ema_decay, float ema_omd,
                float grad_scale, hipStream_t s);
int k_ema_lerp(const TensorListEntry* list, int ntensors, int max_blocks, float decay, float omd, hipStream_t s);
// guarded step (dwn.h dwn_grad_sumsq_multi / dwn_step_guard_finalize / dwn_adamw_ema_multi_guarded)
int k_grad_sumsq(const dwn_guarded_entry* list, int ntensors, int max_blocks, double grad_scale, void* ws, double* pair,
                 hipStream_t s);
int k_step_guard_finalize(const double* pair_a, const double* pair_b, double max_norm, int skip_nonfinite,
                          const dwn_guarded_entry* list, int ntensors, dwn_step_guard* guard, hipStream_t s);
int k_adamw_ema_guarded(const dwn_guarded_entry* list, int ntensors, int max_blocks, double lr, double beta1, double beta2,
                        double eps, double weight_decay, double ema_decay, double grad_scale, const dwn_step_guard* guard,
                        hipStream_t s);
int k_fill_f32(float* p, float v, int n, hipStream_t s);
int k_pack_weight_dual(const float* src, void* plain, void* tr, int groups, int R, int C, int Rp, int ldp, int ldt, int dtype,
                       hipStream_t s);
int k_pwl_bwd_reduce(const float* P, const float* gate, const float* W, int B, int K, int N, float* dW, float* dg,
                     hipStream_t s);
int k_assemble_inputs(const dwn_clip_desc* descs, int B, int T, int H0, int W0, int H, int W, float pad, float* x,
                      hipStream_t s);
int k_assemble_targets(const dwn_clip_desc* descs, int B, int T, float* const* targets, const int* n_neurons,
                       int n_mice, int max_neurons, float* mice_weights, hipStream_t s);
int k_zero(void* p, size_t nbytes, hipStream_t s);
// gaze shifter (dwn.h dwn_gaze_args; dwn_gaze.hip): arguments checked by the C-ABI layer
int k_gaze_forward(const dwn_gaze_args& a, hipStream_t s);
int k_gaze_backward(const dwn_gaze_args& a, hipStream_t s);      // a.dx and / or a.dshift
int k_plane_mean(const float* x, int B, int Cin, int T, int H, int W, int c0, int nc, float* mean, hipStream_t s);
// correlation objective (dwn.h dwn_corr_args; dwn_corr.hip): arguments checked by the C-ABI layer
size_t k_corr_ws_bytes(int N);
int k_corr_moments(const dwn_corr_args& a, hipStream_t s);
int k_corr_finalize(const dwn_corr_args& a, hipStream_t s);
int k_corr_backward(const dwn_corr_args& a, hipStream_t s);

// in-silico stimuli (dwn.h dwn_gabor_args; dwn_stim.hip): arguments checked by the C-ABI layer
size_t k_gabor_ws_bytes(const dwn_gabor_args& a);
int k_gabor_forward(const dwn_gabor_args& a, hipStream_t s);
int k_gabor_backward(const dwn_gabor_args& a, hipStream_t s);      // partials into a.ws, then the per-clip fold

// regularised MEI synthesis (dwn.h dwn_blur3d_args, dwn_clip_moments_args, dwn_mei_update_args; dwn_mei.hip): arguments checked
// by the C-ABI layer
size_t k_blur3d_ws_bytes(const dwn_blur3d_args& a);
int k_blur3d(const dwn_blur3d_args& a, hipStream_t s);              // in-plane pass into a.ws, then the temporal pass
size_t k_clip_moments_ws_bytes(const dwn_clip_moments_args& a);
int k_clip_moments(const dwn_clip_moments_args& a, hipStream_t s);  // partials into a.ws, then the per-clip fold
int k_mei_update(const dwn_mei_update_args& a, hipStream_t s);
// trial-level evaluation (dwn.h dwn_trial_score_args; dwn_trial_score.hip): arguments checked by the C-ABI layer
size_t k_trial_score_ws_bytes(int N);
int k_trial_moments(const dwn_trial_score_args& a, hipStream_t s);          // merges the tables' groups into a.state
int k_trial_score_finalize(const dwn_trial_score_args& a, hipStream_t s);   // scores, partials into a.ws, then the fold
// behaviour modulator (dwn.h dwn_modulator_args; dwn_modulator.hip): arguments checked by the C-ABI layer
size_t k_modulator_ws_bytes(const dwn_modulator_args& a);
int k_modulator_forward(const dwn_modulator_args& a, hipStream_t s);
int k_modulator_backward(const dwn_modulator_args& a, hipStream_t s);      // a.dy, a.dh, a.du, a.dc: each may be null
// retinotopic readout gain (dwn.h dwn_spatial_gain_args; dwn_spatial.hip): arguments checked by the C-ABI layer
size_t k_spatial_gain_ws_bytes(const dwn_spatial_gain_args& a);
int k_spatial_gain_forward(const dwn_spatial_gain_args& a, hipStream_t s);
int k_spatial_gain_backward(const dwn_spatial_gain_args& a, hipStream_t s); // a.dy, a.dg, a.dpos, a.dweight, a.dbias: each may be null
// receptive-field mapping (dwn.h dwn_noise_args, dwn_sta_args; dwn_stim.hip, dwn_rf.hip): arguments checked by the C-ABI layer
int k_noise_forward(const dwn_noise_args& a, hipStream_t s);
size_t k_sta_state_bytes(const dwn_sta_args& a);
size_t k_sta_ws_bytes(const dwn_sta_args& a);
int k_sta_accumulate(const dwn_sta_args& a, hipStream_t s);                  // cross term, then the four moment vectors
int k_sta_finalize(const dwn_sta_args& a, hipStream_t s);                    // V statistics into a.ws, then one wave per neuron
// parametric receptive-field fits (dwn.h dwn_gauss2d_args; dwn_rf_fit.hip): arguments checked by the C-ABI layer
size_t k_gauss2d_ws_bytes(const dwn_gauss2d_args& a);
int k_gauss2d_fit(const dwn_gauss2d_args& a, hipStream_t s);                  // one wave per map, one launch
int k_gauss2d_profile(const dwn_gauss2d_profile_args& a, hipStream_t s);      // one wave per neuron
// population structure (dwn.h dwn_pair_args, dwn_pair_compare_args; dwn_pairwise.hip): arguments checked by the C-ABI layer
long long k_pair_ldz(int N);
size_t k_pair_compare_ws_bytes(int M);
int k_pair_stage(const dwn_pair_args& a, hipStream_t s);                      // Z into a.ws, advances the state's mean
int k_pair_syrk(const dwn_pair_args& a, hipStream_t s);                       // C += Z Z^T
int k_pair_corr_finalize(const dwn_pair_args& a, hipStream_t s);
int k_pair_compare(const dwn_pair_compare_args& a, hipStream_t s);            // row moments into a.ws, then the one-workgroup merge
// population modes (dwn.h dwn_modes_args; dwn_modes.hip): arguments checked by the C-ABI layer
size_t k_modes_moments_ws_bytes(int N);
size_t k_modes_ritz_ws_bytes(int N);
size_t k_modes_solve_ws_bytes(int N, int p);
size_t k_modes_overlap_ws_bytes(int N, int k, int with_matrix);
int k_modes_symm(const dwn_modes_args& a, hipStream_t s);                     // Y = scale A Q
int k_modes_moments(const dwn_modes_args& a, hipStream_t s);
int k_modes_orth(const dwn_modes_args& a, hipStream_t s);
int k_modes_small_eigh(const dwn_modes_args& a, hipStream_t s);
int k_modes_ritz(const dwn_modes_args& a, hipStream_t s);                     // clears status, rotates, decides
int k_modes_solve(const dwn_modes_args& a, hipStream_t s);
int k_modes_overlap(const dwn_modes_args& a, hipStream_t s);
int k_pw_bwd_prep(const float* w1, const float* abc, int E, int C, void* bp, float* gacc, float* r3, int dtype,
                  const float* res_abc, int res_C, hipStream_t s);
// conv_pw weight gradient from the raw products (see pw_bwd_fused_kernel): tacc [(E + C + 8)][C] fp32 = rows T1 = dh1^T a0,
// Ga = a0^T a0, s = 1^T a0;  dw[e][c] = A1[e] T1[e][c] + A2[e] sum_c' W1[e][c'] Ga[c'][c] + A3[e] s[c]   (W1 as rounded to dtype)
size_t pw_wgrad_tacc_floats(int E, int C);
int k_pw_wgrad_fold(const float* tacc, const float* abc, const float* w1, int E, int C, float* dw, int dtype, hipStream_t s);
// the block backward's parameter-gradient tail: k_se_mlp_bwd's wgrad kernel (wgrad = false there) and k_pw_wgrad_fold in one launch
int k_block_param_tail(const float* dgp, const float* dhp, const float* pmean, const float* hid_pre, int B, int Cse, int R,
                       float* dwr, float* dbr, float* dwe, float* dbe, const float* tacc, const float* abc, const float* w1, int E,
                       int C, float* dw, int dtype, hipStream_t s);

// ---- fused per-call preparation (k_prep): zero ranges, constant fills and weight packs in one launch
enum { PREP_ZERO = 0, PREP_FILL = 1, PREP_PACKW = 2, PREP_PACKDW = 3, PREP_BNEVAL = 4 };
#define PREP_MAX_OPS 16
struct PrepOp {
    int kind, nblocks;
    const float* src; void* dst;
    const float* src2; const float* src3; const float* src4;     // BNEVAL: beta, running_mean, running_var (src = gamma)
    long long n;                       // ZERO: 16-byte units; FILL / PACK* / BNEVAL: elements (channels)
    float v;
    int R, C, transpose, Rd, Cd;       // PACKW: src [groups][R][C] -> dst [groups][Rd][Cd]; PACKDW: C channels, R taps
};
struct PrepArgs {
    int nops;
    PrepOp op[PREP_MAX_OPS];
    PrepArgs() : nops(0) {}
    static int blocks_for(long long n, int cap) { long long b = (n + 255) / 256; return (int)(b > cap ? cap : b); }
    bool zero(void* p, size_t nbytes) {
        if (nbytes == 0) return true;
        if (((size_t)p & 15) || (nbytes & 15) || nops >= PREP_MAX_OPS) return false;
        PrepOp& q = op[nops++]; q = PrepOp(); q.kind = PREP_ZERO; q.dst = p; q.n = (long long)(nbytes / 16); q.nblocks = blocks_for(q.n, 256);
        return true;
    }
    bool fill(float* p, float v, int n) {
        if (n <= 0) return true;
        if (nops >= PREP_MAX_OPS) return false;
        PrepOp& q = op[nops++]; q = PrepOp(); q.kind = PREP_FILL; q.dst = p; q.v = v; q.n = n; q.nblocks = blocks_for(n, 1 << 30);
        return true;
    }
    bool packw(const float* src, void* dst, int groups, int R, int C, int transpose, int Rd, int Cd) {
        if (nops >= PREP_MAX_OPS) return false;
        PrepOp& q = op[nops++]; q = PrepOp(); q.kind = PREP_PACKW; q.src = src; q.dst = dst; q.R = R; q.C = C; q.transpose = transpose;
        q.Rd = Rd; q.Cd = Cd; q.n = (long long)groups * Rd * Cd; q.nblocks = blocks_for(q.n, 1 << 30);
        return true;
    }
    bool packdw(const float* src, float* dst, int C, int taps) {
        if (nops >= PREP_MAX_OPS) return false;
        PrepOp& q = op[nops++]; q = PrepOp(); q.kind = PREP_PACKDW; q.src = src; q.dst = dst; q.C = C; q.R = taps; q.n = (long long)C * taps;
        q.nblocks = blocks_for(q.n, 1 << 30);
        return true;
    }
    // eval-mode BatchNorm coefficients [4][C] = scale, shift, mean, invstd from the running statistics (v = eps)
    bool bneval(const dwn_bn& bn, int C, float eps) {
        if (nops >= PREP_MAX_OPS) return false;
        PrepOp& q = op[nops++]; q = PrepOp(); q.kind = PREP_BNEVAL; q.src = bn.gamma; q.src2 = bn.beta; q.src3 = bn.running_mean;
        q.src4 = bn.running_var; q.dst = bn.coef; q.v = eps; q.n = C; q.C = C; q.nblocks = blocks_for(C, 1 << 30);
        return true;
    }
};
int k_prep(const PrepArgs& pa, int dtype, hipStream_t s);
