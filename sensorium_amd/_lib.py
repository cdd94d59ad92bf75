"""ctypes binding of libdwiseneuro_hip.so (C-ABI: include/dwn.h).

The product path has no fallback: if the shared library is missing or its ABI does not match, importing
this module raises.  Structures mirror include/dwn.h field by field; ``dwn_sizeof`` cross-checks the layout.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

# torch must be imported BEFORE the shared library is loaded: torch ships its own libamdhip64 and the process must
# hold exactly one HIP runtime.  With torch first, the library's DT_NEEDED libamdhip64.so.N binds to the copy torch
# already loaded (same SONAME); loaded the other way round the process ends up with two runtimes and every HIP call
# of this library fails with "no ROCm-capable device is detected".
import torch  # noqa: F401,E402

_HERE = Path(__file__).resolve().parent
# DWN_LIB_PATH: development override (A/B runs of two builds of the same ABI on one box)
# DWN_DETERMINISTIC=1: the ordered-reduction build of the same sources (csrc/Makefile, dwn_common.h) — run-to-run bit-identical
# results, several times slower; for re-run equality checks, not for training
DETERMINISTIC = os.environ.get("DWN_DETERMINISTIC", "0") == "1"
_LIB_NAME = "libdwiseneuro_hip_det.so" if DETERMINISTIC else "libdwiseneuro_hip.so"
LIB_PATH = Path(os.environ["DWN_LIB_PATH"]) if os.environ.get("DWN_LIB_PATH") else _HERE / "csrc" / _LIB_NAME

c_p = C.c_void_p
c_i = C.c_int
c_ll = C.c_longlong
c_f = C.c_float
c_d = C.c_double
c_sz = C.c_size_t

DWN_F32, DWN_BF16 = 0, 1
DWN_NREP = 32
LD_PLAIN, LD_PE, LD_BNACT, LD_AFFINE2, LD_DY3, LD_GATE, LD_CAT1 = 0, 1, 2, 3, 4, 5, 6
EPI_STORE, EPI_READOUT, EPI_DG, EPI_STORE_CAT, EPI_DH3 = 0, 1, 2, 3, 4
NN_AUTO, NN_XL128, NN_XL256, NN_TILE128, NN_KD = 0, 1, 2, 3, 4
F32_AUTO, F32_NATIVE, F32_SPLIT3 = 0, 1, 2
BN_EVAL, BN_TRAIN, BN_FROZEN = 0, 1, 2      # the `training` field of StemArgs / BlockArgs / CortexArgs (include/dwn.h DWN_BN_*)
FAMILIES = ("pw_fwd", "dws_fwd", "dwt_fwd", "se_pool", "pwl_fwd", "resid_fwd", "resid_bwd", "pwl_dgrad", "pwl_wgrad",
            "bn3_reduce", "dwt_bwd", "dws_bwd", "pw_dgrad", "pw_wgrad", "cortex_fwd", "cortex_bwd", "readout_fwd",
            "readout_bwd")


class LoadDesc(C.Structure):
    _fields_ = [("p", c_p), ("q", c_p), ("ld", c_ll), ("v1", c_p), ("v2", c_p), ("v3", c_p), ("v4", c_p),
                ("v5", c_p), ("gate", c_p), ("gate2", c_p), ("gate_ld", c_i), ("rows_per_sample", c_i),
                ("act", c_i), ("pe_t", c_p), ("pe_h", c_p), ("pe_w", c_p), ("pT", c_i), ("pH", c_i),
                ("pW", c_i), ("pe_ld", c_i), ("ld2", c_ll), ("cat_c1", c_i), ("cat_c2", c_i)]


class GemmNNArgs(C.Structure):
    _fields_ = [("a", LoadDesc), ("a_kind", c_i), ("b", c_p), ("ldb", c_ll), ("c", c_p), ("ldc", c_ll),
                ("M", c_i), ("N", c_i), ("K", c_i), ("groups", c_i), ("stats", c_p),
                ("f32_split", c_i), ("stat_nchan", c_i), ("epi", c_i), ("bias", c_p),
                ("sp_beta", c_f), ("out_nct", c_p), ("Tn", c_i), ("n_valid", c_i), ("y3", c_p), ("ldy3", c_ll),
                ("s3", c_p), ("t3", c_p), ("dg", c_p), ("dg_ld", c_i), ("rows_per_sample", c_i),
                ("a2", c_p), ("a2_ld", c_ll), ("K1", c_i), ("b_sample_stride", c_ll), ("b_rows_per_sample", c_i),
                ("gate3", c_p), ("dps3", c_p), ("coef3", c_p), ("coef3_ld", c_i), ("variant", c_i), ("sp_beta_dev", c_p)]


class GemmTNArgs(C.Structure):
    _fields_ = [("p", LoadDesc), ("p_kind", c_i), ("q", LoadDesc), ("q_kind", c_i), ("M", c_i), ("R", c_i),
                ("Cc", c_i), ("dw", c_p), ("lddw", c_ll), ("groups", c_i), ("rows_per_split", c_i),
                ("nsplit", c_i), ("R_load", c_i), ("rows_per_sample", c_i), ("splits_per_sample", c_i),
                ("dw_sample_stride", c_ll), ("overwrite", c_i), ("dw_f64", c_i)]


class DwSpatialFwdArgs(C.Structure):
    _fields_ = [("inp", LoadDesc), ("w", c_p), ("out", c_p), ("planes", c_i), ("Hin", c_i), ("Win", c_i),
                ("Hout", c_i), ("Wout", c_i), ("C", c_i), ("stride", c_i), ("ks", c_i), ("stats", c_p),
                ("rows_band", c_i), ("impl", c_i),
                ("a0", c_p), ("a0_ld", c_ll), ("w1", c_p), ("Cin", c_i)]      # rebuilt-input mode (include/dwn.h)


class DwSpatialBwdArgs(C.Structure):
    _fields_ = [("dy", LoadDesc), ("y1", LoadDesc), ("w", c_p), ("dh1", c_p), ("dw", c_p), ("planes", c_i),
                ("Hin", c_i), ("Win", c_i), ("Hout", c_i), ("Wout", c_i), ("C", c_i), ("stride", c_i),
                ("ks", c_i), ("stats", c_p), ("rows_band", c_i), ("impl", c_i),
                ("a0", c_p), ("a0_ld", c_ll), ("w1", c_p), ("Cin", c_i)]      # rebuilt-y1 mode (include/dwn.h)


class DwTemporalFwdArgs(C.Structure):
    _fields_ = [("inp", LoadDesc), ("w", c_p), ("out", c_p), ("B", c_i), ("T", c_i), ("HW", c_i), ("C", c_i),
                ("kt", c_i), ("stats", c_p), ("z_scale", c_p), ("z_shift", c_p), ("pooled", c_p)]


class DwTemporalBwdArgs(C.Structure):
    _fields_ = [("dy", LoadDesc), ("dy_kind", c_i), ("y2", LoadDesc), ("w", c_p), ("dh2", c_p), ("dw", c_p),
                ("B", c_i), ("T", c_i), ("HW", c_i), ("C", c_i), ("kt", c_i), ("stats", c_p)]


class BN(C.Structure):
    _fields_ = [("gamma", c_p), ("beta", c_p), ("running_mean", c_p), ("running_var", c_p),
                ("num_batches_tracked", c_p), ("coef", c_p), ("dgamma", c_p), ("dbeta", c_p)]


class StemArgs(C.Structure):
    _fields_ = [("dtype", c_i), ("training", c_i), ("B", c_i), ("Cin", c_i), ("C0", c_i), ("S", c_ll),
                ("eps", c_f), ("momentum", c_f), ("x", c_p), ("w", c_p), ("bn", BN),
                ("pe_t", c_p), ("pe_h", c_p), ("pe_w", c_p), ("T", c_i), ("H", c_i), ("W", c_i),
                ("y0", c_p), ("out", c_p),
                ("dout", c_p), ("dw", c_p), ("ws", c_p), ("ws_bytes", c_sz), ("xmom", c_p)]


class StemInputGradArgs(C.Structure):
    _fields_ = [("dtype", c_i), ("training", c_i), ("B", c_i), ("Cin", c_i), ("C0", c_i), ("S", c_ll),
                ("w", c_p), ("coef", c_p), ("dout", c_p), ("dx", c_p)]


class BlockArgs(C.Structure):
    _fields_ = [("dtype", c_i), ("training", c_i),
                ("B", c_i), ("T", c_i), ("Hin", c_i), ("Win", c_i), ("Hout", c_i), ("Wout", c_i), ("Cin", c_i),
                ("Cmid", c_i), ("Cout", c_i), ("stride", c_i), ("ks", c_i), ("kt", c_i), ("se_r", c_i),
                ("eps", c_f), ("momentum", c_f),
                ("x", c_p), ("out", c_p), ("y1", c_p), ("y2", c_p), ("y3", c_p), ("y4", c_p),
                ("z3", c_p), ("x_has_pe", c_i), ("a0", c_p),
                ("pe_t", c_p), ("pe_h", c_p), ("pe_w", c_p),
                ("out_pe_t", c_p), ("out_pe_h", c_p), ("out_pe_w", c_p),
                ("w_pw", c_p), ("w_dws", c_p), ("w_dwt", c_p), ("w_pwl", c_p), ("se_wr", c_p), ("se_br", c_p),
                ("se_we", c_p), ("se_be", c_p),
                ("bn1", BN), ("bn2", BN), ("bn3", BN), ("bn4", BN), ("bnsc", BN),
                ("drop_scale", c_p), ("hsrc", c_p), ("wsrc", c_p), ("hinv", c_p), ("winv", c_p),
                ("se_pmean", c_p), ("se_hidpre", c_p), ("se_gate", c_p),
                ("dout", c_p), ("dx", c_p), ("buf_a", c_p), ("buf_b", c_p), ("dy4", c_p), ("da0", c_p),
                ("dw_pw", c_p), ("dw_dws", c_p), ("dw_dwt", c_p), ("dw_pwl", c_p), ("dse_wr", c_p),
                ("dse_br", c_p), ("dse_we", c_p), ("dse_be", c_p),
                ("ws", c_p), ("ws_bytes", c_sz), ("pwl_bwd", c_i), ("f32_products", c_i), ("y1_mode", c_i)]


class PoolArgs(C.Structure):
    _fields_ = [("dtype", c_i), ("BT", c_ll), ("HW", c_i), ("C", c_i), ("x", c_p), ("out", c_p), ("dout", c_p),
                ("dx", c_p)]


class CortexArgs(C.Structure):
    _fields_ = [("dtype", c_i), ("training", c_i), ("B", c_i), ("T", c_i), ("Cin", c_i), ("C", c_i),
                ("groups", c_i), ("eps", c_f), ("momentum", c_f), ("x", c_p), ("out", c_p), ("y", c_p),
                ("w", c_p), ("bn", BN), ("bnsc", BN), ("drop_scale", c_p), ("dout", c_p), ("dx", c_p),
                ("dw", c_p), ("dout_mask", c_p), ("dout_mask_ld", c_i), ("ws", c_p), ("ws_bytes", c_sz), ("f32_products", c_i)]


class ReadoutArgs(C.Structure):
    _fields_ = [("dtype", c_i), ("B", c_i), ("T", c_i), ("Cin", c_i), ("groups", c_i), ("n_out", c_i),
                ("softplus_beta", c_f), ("x", c_p), ("w", c_p), ("bias", c_p), ("drop_mask", c_p), ("out", c_p),
                ("dout", c_p), ("dx", c_p), ("dw", c_p), ("dbias", c_p), ("ws", c_p), ("ws_bytes", c_sz), ("wt", c_p),
                ("f32_products", c_i), ("beta_dev", c_p), ("dbeta", c_p)]      # learnable Softplus beta: both null = softplus_beta


class TensorEntry(C.Structure):
    _fields_ = [("param", c_p), ("grad", c_p), ("exp_avg", c_p), ("exp_avg_sq", c_p), ("ema", c_p),
                ("numel", c_ll), ("is_int64", c_i), ("pad_", c_i)]


class GuardedEntry(C.Structure):           # TensorEntry + the parameter's device-resident step count (guarded step)
    _fields_ = [("param", c_p), ("grad", c_p), ("exp_avg", c_p), ("exp_avg_sq", c_p), ("ema", c_p),
                ("numel", c_ll), ("is_int64", c_i), ("pad_", c_i), ("step", c_p)]


class StepGuard(C.Structure):
    _fields_ = [("norm", c_d), ("coef", c_f), ("skip", c_i), ("nonfinite", c_ll), ("good_steps", c_ll),
                ("skipped_steps", c_ll)]


class ClipSrc(C.Structure):
    _fields_ = [("video", c_p), ("behavior", c_p), ("pupil_center", c_p), ("responses", c_p), ("length", c_ll),
                ("video_dtype", c_i), ("frame_start", c_i), ("frame_step", c_i), ("valid", c_i)]


class ClipDesc(C.Structure):
    _fields_ = [("src", ClipSrc), ("mix", ClipSrc), ("bbx1", c_i), ("bby1", c_i), ("bbx2", c_i), ("bby2", c_i),
                ("one_minus_lam", c_f), ("lam", c_f), ("mouse", c_i), ("mix_mode", c_i)]


class PwBwdArgs(C.Structure):
    _fields_ = [("dh1", c_p), ("a0", c_p), ("w_pw", c_p), ("abc", c_p), ("da0", c_p), ("dw", c_p),
                ("M", c_ll), ("E", c_i), ("Cin", c_i), ("ws", c_p), ("ws_bytes", c_sz), ("res", c_p), ("res_abc", c_p),
                ("res_C", c_i), ("res_hinv", c_p), ("res_winv", c_p), ("res_Hin", c_i), ("res_Win", c_i), ("res_Hout", c_i),
                ("res_Wout", c_i)]


class DwSpatialRcFwdArgs(C.Structure):
    _fields_ = [("a0", c_p), ("a0_ld", c_ll), ("blob", c_p), ("out", c_p), ("planes", c_i), ("Hin", c_i),
                ("Win", c_i), ("Hout", c_i), ("Wout", c_i), ("Cin", c_i), ("E", c_i), ("stride", c_i),
                ("stats", c_p), ("rows_band", c_i), ("round_y1", c_i)]


class GazeArgs(C.Structure):              # gaze shifter (include/dwn.h dwn_gaze_args)
    _fields_ = [("B", c_i), ("Cin", c_i), ("T", c_i), ("H", c_i), ("W", c_i), ("video_channel", c_i), ("fill", c_f),
                ("pad_", c_i), ("x", c_p), ("shift", c_p), ("out", c_p), ("dout", c_p), ("dx", c_p), ("dshift", c_p)]


class CorrArgs(C.Structure):              # correlation objective (include/dwn.h dwn_corr_args)
    _fields_ = [("B", c_i), ("N", c_i), ("T", c_i), ("reduction", c_i), ("eps", c_d), ("w_stride", c_ll), ("pred", c_p),
                ("target", c_p), ("w", c_p), ("stat", c_p), ("count", c_p), ("share", c_p), ("loss_acc", c_p), ("gscale", c_p),
                ("dpred", c_p), ("ws", c_p), ("ws_bytes", c_sz)]


class GaborArgs(C.Structure):             # in-silico stimuli (include/dwn.h dwn_gabor_args)
    _fields_ = [("B", c_i), ("Cin", c_i), ("T", c_i), ("H", c_i), ("W", c_i), ("video_channel", c_i), ("envelope", c_i),
                ("clamp", c_i), ("y0", c_i), ("x0", c_i), ("wh", c_i), ("ww", c_i), ("background", c_f), ("lo", c_f), ("hi", c_f),
                ("pad", c_f), ("x", c_p), ("params", c_p), ("out", c_p), ("dout", c_p), ("dparams", c_p), ("ws", c_p),
                ("ws_bytes", c_sz)]


class ModulatorArgs(C.Structure):         # behaviour modulator (include/dwn.h dwn_modulator_args)
    _fields_ = [("B", c_i), ("N", c_i), ("T", c_i), ("K", c_i), ("max_log_gain", c_f), ("pad_", c_i), ("y", c_p), ("h", c_p),
                ("u", c_p), ("c", c_p), ("out", c_p), ("dout", c_p), ("dy", c_p), ("dh", c_p), ("du", c_p), ("dc", c_p),
                ("ws", c_p), ("ws_bytes", c_sz)]


class Blur3dArgs(C.Structure):            # regularised MEI synthesis (include/dwn.h dwn_blur3d_args)
    _fields_ = [("B", c_i), ("T", c_i), ("H", c_i), ("W", c_i), ("Cin_src", c_i), ("c_src", c_i), ("Cin_dst", c_i), ("c_dst", c_i),
                ("Rt", c_i), ("Rh", c_i), ("Rw", c_i), ("y0", c_i), ("x0", c_i), ("wh", c_i), ("ww", c_i), ("pad_", c_i),
                ("src", c_p), ("dst", c_p), ("taps", c_p), ("ws", c_p), ("ws_bytes", c_sz)]


class ClipMomentsArgs(C.Structure):       # (include/dwn.h dwn_clip_moments_args)
    _fields_ = [("B", c_i), ("Cin", c_i), ("T", c_i), ("H", c_i), ("W", c_i), ("c", c_i), ("y0", c_i), ("x0", c_i), ("wh", c_i),
                ("ww", c_i), ("x", c_p), ("stat", c_p), ("ws", c_p), ("ws_bytes", c_sz)]


class MeiUpdateArgs(C.Structure):         # (include/dwn.h dwn_mei_update_args)
    _fields_ = [("mode", c_i), ("B", c_i), ("Cin", c_i), ("T", c_i), ("H", c_i), ("W", c_i), ("c", c_i), ("y0", c_i), ("x0", c_i),
                ("wh", c_i), ("ww", c_i), ("Cin_g", c_i), ("c_g", c_i), ("has_mean", c_i), ("has_contrast", c_i),
                ("contrast_mode", c_i), ("lo", c_f), ("hi", c_f), ("mean_target", C.c_double), ("contrast", C.c_double),
                ("x", c_p), ("g", c_p), ("stat", c_p), ("lr", c_p)]


class TrialDesc(C.Structure):             # trial-level evaluation (include/dwn.h dwn_trial_desc: one row of the DEVICE trial table)
    _fields_ = [("pred", c_p), ("target", c_p), ("ld_pred", c_ll), ("ld_target", c_ll), ("first", c_i), ("frames", c_i)]


class TrialGroup(C.Structure):            # (include/dwn.h dwn_trial_group: one row of the DEVICE group table)
    _fields_ = [("first_trial", c_i), ("repeats", c_i), ("frames", c_i)]


class TrialScoreArgs(C.Structure):        # (include/dwn.h dwn_trial_score_args)
    _fields_ = [("N", c_i), ("n_trials", c_i), ("n_groups", c_i), ("max_repeats", c_i), ("max_frames", c_i), ("pad_", c_i),
                ("n_all", c_ll), ("n_repeat", c_ll), ("n_group_frames", c_ll), ("eps", c_d), ("fev_threshold", c_d),
                ("trials", c_p), ("groups", c_p), ("state", c_p), ("scores", c_p), ("summary", c_p), ("ws", c_p), ("ws_bytes", c_sz)]


class PairSeg(C.Structure):               # population structure (include/dwn.h dwn_pair_seg: one row of the DEVICE segment table)
    _fields_ = [("x", c_p), ("ld", c_ll), ("first", c_i), ("frames", c_i)]


class PairArgs(C.Structure):              # (include/dwn.h dwn_pair_args)
    _fields_ = [("N", c_i), ("kind", c_i), ("n_segs", c_i), ("n_groups", c_i), ("max_repeats", c_i), ("max_frames", c_i),
                ("cols", c_i), ("out_f32", c_i), ("n", c_ll), ("eps", c_d), ("segs", c_p), ("groups", c_p), ("state", c_p),
                ("out", c_p), ("ws", c_p), ("ws_bytes", c_sz)]


class PairCompareArgs(C.Structure):       # (include/dwn.h dwn_pair_compare_args)
    _fields_ = [("N", c_i), ("M", c_i), ("lda", c_ll), ("ldb", c_ll), ("eps", c_d), ("A", c_p), ("B", c_p), ("sel", c_p),
                ("per_neuron", c_p), ("summary", c_p), ("ws", c_p), ("ws_bytes", c_sz)]


class ModesArgs(C.Structure):             # population modes (include/dwn.h dwn_modes_args)
    _fields_ = [("N", c_i), ("p", c_i), ("k", c_i), ("max_iters", c_i), ("lda", c_ll), ("ldq", c_ll), ("ldy", c_ll), ("ldv", c_ll),
                ("scale", c_d), ("tol", c_d), ("seed", C.c_ulonglong), ("A", c_p), ("Q", c_p), ("Y", c_p), ("V", c_p), ("H", c_p),
                ("W", c_p), ("values", c_p), ("residuals", c_p), ("moments", c_p), ("status", c_p), ("ws", c_p), ("ws_bytes", c_sz)]


class SpatialGainArgs(C.Structure):       # retinotopic readout gain (include/dwn.h dwn_spatial_gain_args)
    _fields_ = [("B", c_i), ("N", c_i), ("T", c_i), ("Hf", c_i), ("Wf", c_i), ("K", c_i), ("g_dtype", c_i), ("max_log_gain", c_f),
                ("y", c_p), ("g", c_p), ("pos", c_p), ("weight", c_p), ("bias", c_p), ("out", c_p), ("dout", c_p), ("dy", c_p),
                ("dg", c_p), ("dpos", c_p), ("dweight", c_p), ("dbias", c_p), ("ws", c_p), ("ws_bytes", c_sz)]


class NoiseArgs(C.Structure):            # receptive-field mapping (include/dwn.h dwn_noise_args)
    _fields_ = [("B", c_i), ("Cin", c_i), ("T", c_i), ("H", c_i), ("W", c_i), ("video_channel", c_i), ("kind", c_i), ("cell", c_i),
                ("hold", c_i), ("y0", c_i), ("x0", c_i), ("wh", c_i), ("ww", c_i), ("pad_", c_i), ("background", c_f),
                ("contrast", c_f), ("density", c_f), ("pad", c_f), ("seed", C.c_ulonglong), ("first_clip", c_ll), ("x", c_p),
                ("out", c_p)]


class StaArgs(C.Structure):              # (include/dwn.h dwn_sta_args)
    _fields_ = [("B", c_i), ("Cin", c_i), ("T", c_i), ("H", c_i), ("W", c_i), ("N", c_i), ("channel", c_i), ("y0", c_i), ("x0", c_i),
                ("wh", c_i), ("ww", c_i), ("cell", c_i), ("lags", c_i), ("skip", c_i), ("s0", c_f), ("pad_", c_i), ("samples", c_ll),
                ("rel_threshold", c_d), ("x", c_p), ("r", c_p), ("r0", c_p), ("state", c_p), ("cov", c_p), ("z", c_p),
                ("summary", c_p), ("ws", c_p), ("ws_bytes", c_sz)]


class Gauss2dArgs(C.Structure):          # parametric receptive-field fits (include/dwn.h dwn_gauss2d_args)
    _fields_ = [("R", c_i), ("gh", c_i), ("gw", c_i), ("M", c_i), ("fit_baseline", c_i), ("max_iter", c_i), ("rel_threshold", c_d),
                ("xtol", c_d), ("ftol", c_d), ("maps", c_p), ("sel", c_p), ("params", c_p), ("table", c_p), ("ws", c_p),
                ("ws_bytes", c_sz)]


class Gauss2dProfileArgs(C.Structure):   # (include/dwn.h dwn_gauss2d_profile_args)
    _fields_ = [("N", c_i), ("L", c_i), ("gh", c_i), ("gw", c_i), ("fit_baseline", c_i), ("pad_", c_i), ("params", c_p), ("maps", c_p),
                ("profile", c_p), ("separability", c_p)]


CORR_STAT_ROWS, CORR_TILE = 8, 16          # DWN_CORR_STAT_ROWS, DWN_CORR_TILE
CORR_MEAN, CORR_SUM = 0, 1
GABOR_GAUSSIAN, GABOR_NONE = 0, 1          # DWN_GABOR_*
BLUR_MAX_RADIUS, BLUR_TAPS_STRIDE, MOMENTS_CHUNK = 16, 33, 4096      # DWN_BLUR_MAX_RADIUS, DWN_BLUR_TAPS_STRIDE, DWN_MOMENTS_CHUNK
MEI_STEP, MEI_PROJECT = 0, 1               # DWN_MEI_*
MEI_CONTRAST_MAX, MEI_CONTRAST_FIXED = 0, 1
TRIAL_STATE_ROWS, TRIAL_SCORE_ROWS, TRIAL_SUMMARY, TRIAL_TILE = 17, 5, 8, 4      # DWN_TRIAL_*
NOISE_BINARY, NOISE_SPARSE = 0, 1          # DWN_NOISE_*
STA_SUMMARY = 8                            # DWN_STA_SUMMARY
GAUSS_PARAMS, GAUSS_TABLE = 7, 16          # DWN_GAUSS_*
PAIR_TOTAL, PAIR_SIGNAL, PAIR_NOISE = 0, 1, 2                  # DWN_PAIR_*
PAIR_TILE, PAIR_KSTEP, PAIR_SUMMARY, PAIR_ROW_STATS = 64, 4, 8, 8
MODES_MAXP, MODES_ORTH_C = 64, 8.0                             # DWN_MODES_*
MIX_BOX, MIX_BLEND = 0, 1
VID_U8, VID_F32 = 0, 1

_OLD_STRUCTS = {
    "dwn_load_desc": LoadDesc, "dwn_gemm_nn_args": GemmNNArgs, "dwn_gemm_tn_args": GemmTNArgs,
    "dwn_dw_spatial_fwd_args": DwSpatialFwdArgs, "dwn_dw_spatial_bwd_args": DwSpatialBwdArgs,
    "dwn_dw_temporal_fwd_args": DwTemporalFwdArgs, "dwn_dw_temporal_bwd_args": DwTemporalBwdArgs,
    "dwn_bn": BN, "dwn_stem_args": StemArgs, "dwn_block_args": BlockArgs, "dwn_pool_args": PoolArgs,
    "dwn_cortex_args": CortexArgs, "dwn_readout_args": ReadoutArgs, "dwn_tensor_entry": TensorEntry,
    "dwn_clip_src": ClipSrc, "dwn_clip_desc": ClipDesc, "dwn_pw_bwd_args": PwBwdArgs,
    "dwn_dw_spatial_rc_fwd_args": DwSpatialRcFwdArgs,
}
# structs appended after the oldest library an A/B run (DWN_LIB_PATH) may load: that library may not know them.  A new struct
# goes at the end of this dict.
_NEW_STRUCTS = {
    "dwn_stem_input_grad_args": StemInputGradArgs,
    "dwn_guarded_entry": GuardedEntry, "dwn_step_guard": StepGuard, "dwn_gaze_args": GazeArgs,
    "dwn_corr_args": CorrArgs, "dwn_gabor_args": GaborArgs, "dwn_modulator_args": ModulatorArgs,
    "dwn_blur3d_args": Blur3dArgs, "dwn_clip_moments_args": ClipMomentsArgs, "dwn_mei_update_args": MeiUpdateArgs,
    "dwn_trial_desc": TrialDesc, "dwn_trial_group": TrialGroup, "dwn_trial_score_args": TrialScoreArgs,
    "dwn_spatial_gain_args": SpatialGainArgs, "dwn_noise_args": NoiseArgs, "dwn_sta_args": StaArgs,
    "dwn_gauss2d_args": Gauss2dArgs, "dwn_gauss2d_profile_args": Gauss2dProfileArgs,
    "dwn_pair_seg": PairSeg, "dwn_pair_args": PairArgs, "dwn_pair_compare_args": PairCompareArgs,
    "dwn_modes_args": ModesArgs,
}
_STRUCTS = {**_OLD_STRUCTS, **_NEW_STRUCTS}


class _new(tuple):
    """(restype, argtypes) of an entry appended after the oldest library an A/B run (DWN_LIB_PATH) may load: that library may
    lack it (the plain training step calls none of them).  A new entry is written _new(...)."""
    def __new__(cls, restype, argtypes):
        return super().__new__(cls, (restype, argtypes))


# every symbol include/dwn.h declares: (restype, argtypes)
_P = C.POINTER
SYMBOLS = {
    "dwn_abi_version": (c_i, []),
    "dwn_source_hash": (C.c_char_p, []),
    "dwn_sizeof": (c_i, [C.c_char_p]),
    "dwn_last_error": (C.c_char_p, []),
    "dwn_profile_enable": (c_i, [C.c_ulonglong, c_i]),
    "dwn_profile_collect": (c_i, [c_i, _P(c_d), _P(c_ll)]),
    "dwn_gemm_nn": (c_i, [_P(GemmNNArgs), c_i, c_i, c_p]),
    "dwn_gemm_tn": (c_i, [_P(GemmTNArgs), c_i, c_i, c_p]),
    "dwn_dw_spatial_fwd": (c_i, [_P(DwSpatialFwdArgs), c_i, c_i, c_p]),
    "dwn_dw_spatial_bwd": (c_i, [_P(DwSpatialBwdArgs), c_i, c_i, c_p]),
    "dwn_dw_spatial_bwd_rc_supported": (c_i, [_P(DwSpatialBwdArgs), c_i]),
    "dwn_dw_spatial_fwd_rc_supported": (c_i, [_P(DwSpatialFwdArgs), c_i]),
    "dwn_dw_temporal_fwd": (c_i, [_P(DwTemporalFwdArgs), c_i, c_i, c_p]),
    "dwn_dw_temporal_bwd": (c_i, [_P(DwTemporalBwdArgs), c_i, c_i, c_p]),
    "dwn_dw_temporal_wide_fwd": _new(c_i, [_P(DwTemporalFwdArgs), c_i, c_i, c_p]),
    "dwn_dw_temporal_wide_bwd": _new(c_i, [_P(DwTemporalBwdArgs), c_i, c_i, c_p]),
    "dwn_bn_finalize": (c_i, [c_p, c_i, c_d, _P(BN), c_i, c_i, c_f, c_f, c_i, c_p]),
    "dwn_bn_bwd_finalize": (c_i, [c_p, c_d, _P(BN), c_p, c_i, c_i, c_p]),
    "dwn_pack_weight": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "dwn_stem_workspace_bytes": (c_sz, [_P(StemArgs)]),
    "dwn_stem_forward": (c_i, [_P(StemArgs), c_i, c_p]),
    "dwn_stem_backward": (c_i, [_P(StemArgs), c_i, c_p]),
    "dwn_stem_input_grad": _new(c_i, [_P(StemInputGradArgs), c_i, c_p]),
    "dwn_stem_backward_input": _new(c_i, [_P(StemArgs), c_p, c_i, c_p]),
    "dwn_block_workspace_bytes": (c_sz, [_P(BlockArgs), c_i]),
    "dwn_block_forward": (c_i, [_P(BlockArgs), c_i, c_p]),
    "dwn_block_backward": (c_i, [_P(BlockArgs), c_i, c_p]),
    "dwn_block_forward_writes": (c_i, [_P(BlockArgs)]),
    "dwn_block_backward_route": _new(c_i, [_P(BlockArgs)]),
    "dwn_pool_forward": (c_i, [_P(PoolArgs), c_i, c_p]),
    "dwn_pool_backward": (c_i, [_P(PoolArgs), c_i, c_p]),
    "dwn_cortex_workspace_bytes": (c_sz, [_P(CortexArgs), c_i]),
    "dwn_cortex_forward": (c_i, [_P(CortexArgs), c_i, c_p]),
    "dwn_cortex_backward": (c_i, [_P(CortexArgs), c_i, c_p]),
    "dwn_readout_workspace_bytes": (c_sz, [_P(ReadoutArgs), c_i]),
    "dwn_readout_wt_bytes": (c_sz, [_P(ReadoutArgs)]),
    "dwn_readout_forward": (c_i, [_P(ReadoutArgs), c_i, c_p]),
    "dwn_readout_backward": (c_i, [_P(ReadoutArgs), c_i, c_p]),
    "dwn_poisson_loss_forward": (c_i, [c_p, c_p, c_p, c_ll, c_ll, c_f, c_p, c_i, c_p]),
    "dwn_poisson_loss_backward": (c_i, [c_p, c_p, c_p, c_p, c_ll, c_ll, c_f, c_p, c_i, c_p]),
    "dwn_f64_to_f32": (c_i, [c_p, c_p, c_i, c_i, c_p]),
    "dwn_adamw_ema_multi": (c_i, [c_p, c_i, c_i, c_d, c_d, c_d, c_d, c_d, c_ll, c_d, c_d, c_i, c_p]),
    "dwn_ema_lerp_multi": (c_i, [c_p, c_i, c_i, c_d, c_i, c_p]),
    "dwn_grad_guard_workspace_bytes": _new(c_sz, [c_i, c_i]),
    "dwn_grad_sumsq_multi": _new(c_i, [c_p, c_i, c_i, c_d, c_p, c_sz, c_p, c_i, c_p]),
    "dwn_step_guard_finalize": _new(c_i, [c_p, c_p, c_d, c_i, c_p, c_i, c_p, c_i, c_p]),
    "dwn_adamw_ema_multi_guarded": _new(c_i, [c_p, c_i, c_i, c_d, c_d, c_d, c_d, c_d, c_d, c_d, c_p, c_i, c_p]),
    "dwn_conv_pw_bn_stats_workspace_bytes": (c_sz, [c_i]),
    "dwn_conv_pw_bn_stats": (c_i, [c_p, c_ll, c_ll, c_p, c_i, c_i, _P(BN), c_f, c_f, c_p, c_p, c_sz, c_i, c_i, c_p]),
    "dwn_pw_bwd_fused_supported": (c_i, [c_i, c_ll, c_i, c_i]),
    "dwn_pw_backward_workspace_bytes": (c_sz, [c_i, c_i, c_i]),
    "dwn_pw_backward": (c_i, [_P(PwBwdArgs), c_i, c_i, c_p]),
    "dwn_dw_spatial_rc_blob_bytes": (c_sz, [c_i, c_i]),
    "dwn_dw_spatial_rc_prep": (c_i, [c_p, c_p, c_p, c_i, c_i, c_p, c_i, c_p]),
    "dwn_dw_spatial_rc_supported": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i, c_i]),
    "dwn_dw_spatial_fwd_rc": (c_i, [_P(DwSpatialRcFwdArgs), c_i, c_p]),
    "dwn_assemble_inputs": (c_i, [c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p, c_i, c_p]),
    "dwn_assemble_targets": (c_i, [c_p, c_i, c_i, c_p, c_p, c_i, c_i, c_p, c_i, c_p]),
    "dwn_gaze_shift_forward": _new(c_i, [_P(GazeArgs), c_i, c_p]),
    "dwn_gaze_shift_backward": _new(c_i, [_P(GazeArgs), c_i, c_p]),
    "dwn_plane_mean": _new(c_i, [c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_i, c_p]),
    "dwn_corr_ws_bytes": _new(c_sz, [_P(CorrArgs)]),
    "dwn_corr_moments": _new(c_i, [_P(CorrArgs), c_i, c_p]),
    "dwn_corr_loss_finalize": _new(c_i, [_P(CorrArgs), c_i, c_p]),
    "dwn_corr_loss_backward": _new(c_i, [_P(CorrArgs), c_i, c_p]),
    "dwn_gabor_workspace_bytes": _new(c_sz, [_P(GaborArgs)]),
    "dwn_gabor_forward": _new(c_i, [_P(GaborArgs), c_i, c_p]),
    "dwn_gabor_backward": _new(c_i, [_P(GaborArgs), c_i, c_p]),
    "dwn_modulator_ws_bytes": _new(c_sz, [_P(ModulatorArgs)]),
    "dwn_modulator_forward": _new(c_i, [_P(ModulatorArgs), c_i, c_p]),
    "dwn_modulator_backward": _new(c_i, [_P(ModulatorArgs), c_i, c_p]),
    "dwn_blur3d_ws_bytes": _new(c_sz, [_P(Blur3dArgs)]),
    "dwn_clip_moments_ws_bytes": _new(c_sz, [_P(ClipMomentsArgs)]),
    "dwn_blur3d": _new(c_i, [_P(Blur3dArgs), c_i, c_p]),
    "dwn_clip_moments": _new(c_i, [_P(ClipMomentsArgs), c_i, c_p]),
    "dwn_mei_update": _new(c_i, [_P(MeiUpdateArgs), c_i, c_p]),
    "dwn_trial_score_ws_bytes": _new(c_sz, [_P(TrialScoreArgs)]),
    "dwn_trial_moments": _new(c_i, [_P(TrialScoreArgs), c_i, c_p]),
    "dwn_trial_score_finalize": _new(c_i, [_P(TrialScoreArgs), c_i, c_p]),
    "dwn_spatial_gain_ws_bytes": _new(c_sz, [_P(SpatialGainArgs)]),
    "dwn_spatial_gain_forward": _new(c_i, [_P(SpatialGainArgs), c_i, c_p]),
    "dwn_spatial_gain_backward": _new(c_i, [_P(SpatialGainArgs), c_i, c_p]),
    # (the population structure of dwn_pairwise.hip)
    "dwn_pair_ldz": _new(c_ll, [c_i]),
    "dwn_pair_state_bytes": _new(c_sz, [_P(PairArgs)]),
    "dwn_pair_ws_bytes": _new(c_sz, [_P(PairArgs)]),
    "dwn_pair_compare_ws_bytes": _new(c_sz, [_P(PairCompareArgs)]),
    "dwn_pair_stage": _new(c_i, [_P(PairArgs), c_i, c_p]),
    "dwn_pair_syrk": _new(c_i, [_P(PairArgs), c_i, c_p]),
    "dwn_pair_corr_finalize": _new(c_i, [_P(PairArgs), c_i, c_p]),
    "dwn_pair_compare": _new(c_i, [_P(PairCompareArgs), c_i, c_p]),
    # (the population modes of dwn_modes.hip)
    "dwn_modes_moments_ws_bytes": _new(c_sz, [_P(ModesArgs)]),
    "dwn_modes_ritz_ws_bytes": _new(c_sz, [_P(ModesArgs)]),
    "dwn_modes_solve_ws_bytes": _new(c_sz, [_P(ModesArgs)]),
    "dwn_modes_overlap_ws_bytes": _new(c_sz, [_P(ModesArgs)]),
    "dwn_modes_symm": _new(c_i, [_P(ModesArgs), c_i, c_p]),
    "dwn_modes_moments": _new(c_i, [_P(ModesArgs), c_i, c_p]),
    "dwn_modes_orth": _new(c_i, [_P(ModesArgs), c_i, c_p]),
    "dwn_modes_small_eigh": _new(c_i, [_P(ModesArgs), c_i, c_p]),
    "dwn_modes_ritz": _new(c_i, [_P(ModesArgs), c_i, c_p]),
    "dwn_modes_solve": _new(c_i, [_P(ModesArgs), c_i, c_p]),
    "dwn_modes_overlap": _new(c_i, [_P(ModesArgs), c_i, c_p]),
    # (the parametric fits of dwn_rf_fit.hip; tests/test_host_rf.py keeps the five receptive-field entries last)
    "dwn_gauss2d_ws_bytes": _new(c_sz, [_P(Gauss2dArgs)]),
    "dwn_gauss2d_fit": _new(c_i, [_P(Gauss2dArgs), c_i, c_p]),
    "dwn_gauss2d_profile": _new(c_i, [_P(Gauss2dProfileArgs), c_i, c_p]),
    "dwn_noise_forward": _new(c_i, [_P(NoiseArgs), c_i, c_p]),
    "dwn_sta_state_bytes": _new(c_sz, [_P(StaArgs)]),
    "dwn_sta_ws_bytes": _new(c_sz, [_P(StaArgs)]),
    "dwn_sta_accumulate": _new(c_i, [_P(StaArgs), c_i, c_p]),
    "dwn_sta_finalize": _new(c_i, [_P(StaArgs), c_i, c_p]),
}


class DwnError(RuntimeError):
    pass


# csrc/Makefile HASH_SRCS, in its order
HASH_SRCS = ("dwn_api.hip", "dwn_gemm.hip", "dwn_gemm_nn_1.hip", "dwn_gemm_nn_2.hip", "dwn_gemm_nn_3.hip", "dwn_gemm_nn_4.hip", "dwn_gemm_nn_5.hip",
             "dwn_gemm_nn_6.hip", "dwn_gemm_tn.hip", "dwn_gram.hip", "dwn_pw_bwd.hip", "dwn_gemm_xl.hip", "dwn_gemm_kd.hip", "dwn_dwconv.hip", "dwn_dwrc.hip",
             "dwn_dwbwd.hip", "dwn_dwfwd.hip", "dwn_elementwise.hip", "dwn_data.hip", "dwn_gaze.hip", "dwn_modulator.hip", "dwn_spatial.hip", "dwn_mei.hip", "dwn_rf_fit.hip", "dwn_pairwise.hip", "dwn_modes.hip", "dwn_trial_score.hip", "dwn_rf.hip", "dwn_corr.hip", "dwn_stim.hip", "dwn_common.h", "dwn_internal.h",
             "dwn_kernels.h", "dwn_launch.h", "dwn_gemm_nn.h", "dwn_gain.h", "dwn_reduce.h", "dwn_philox.h",
             "../../include/dwn.h")


def source_hash() -> str:
    import hashlib
    h = hashlib.sha256()
    for name in HASH_SRCS:
        h.update((_HERE / "csrc" / name).read_bytes())
    return h.hexdigest()[:16]


def _load():
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(or `make -C {LIB_PATH.parent}`).  sensorium_amd has no fallback path.")
    lib = C.CDLL(str(LIB_PATH), mode=getattr(os, "RTLD_NOW", 2))
    ab = bool(os.environ.get("DWN_LIB_PATH"))      # an explicitly chosen other build: a same-box A/B run of an older library
    for name, proto in SYMBOLS.items():
        if ab and isinstance(proto, _new) and not hasattr(lib, name):
            continue                     # (A/B: a library from before this entry)
        restype, argtypes = proto
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.dwn_abi_version() != 7 and not (ab and lib.dwn_abi_version() == 6):
        raise ImportError("libdwiseneuro_hip.so ABI version mismatch")
    built, have = lib.dwn_source_hash().decode(), source_hash()
    if built != have and not os.environ.get("DWN_LIB_PATH"):        # (an explicitly chosen other build is an A/B run)
        raise ImportError(f"{LIB_PATH.name} was built from other sources (binary {built}, tree {have}): rebuild it with "
                          f"`make -C {LIB_PATH.parent}` — binaries are not in git, so what runs must be what is committed")
    for cname, struct in _STRUCTS.items():
        n = lib.dwn_sizeof(cname.encode())
        if n != C.sizeof(struct) and not (ab and (0 < n < C.sizeof(struct) or cname in _NEW_STRUCTS)):      # (A/B: ABI 7 only appended)
            raise ImportError(f"struct layout mismatch for {cname}: C {n} bytes vs ctypes {C.sizeof(struct)}")
    return lib


lib = _load()


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib.dwn_last_error()
        raise DwnError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")
