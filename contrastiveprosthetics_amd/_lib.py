"""ctypes binding of libcpnative.so (include/cpnative.h).

There is deliberately no CPU fallback: if the HIP library is missing or a call
fails, an exception is raised (the product path must never silently run anything
but the gfx950 kernels).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CPNATIVE_LIB: another build of the same library, e.g. from tools/build_prev.sh (A/B measurements of two builds)
LIB_PATH = os.environ.get("CPNATIVE_LIB") or os.path.join(_HERE, "libcpnative.so")

CP_F32, CP_BF16, CP_FP8 = 0, 1, 2
FP8_STATE_BYTES = 1024            # scale table at the start of a CP_FP8 workspace (csrc/fp8.cuh): zero once after allocating
CP_TASKS, CP_EMG_DIM, CP_D_E, CP_N_BN, CP_N_FC = 41, 12, 16, 9, 7

_fp = C.c_void_p


class cp_params(C.Structure):
    _fields_ = [
        ("conv1_w", _fp), ("conv1_b", _fp), ("conv2_w", _fp), ("conv2_b", _fp),
        ("fc_w", _fp * CP_N_FC), ("fc_b", _fp * CP_N_FC),
        ("bn_g", _fp * CP_N_BN), ("bn_b", _fp * CP_N_BN),
        ("last_w", _fp), ("easy_w", _fp), ("easy_b", _fp),
    ]


class cp_bn_buffers(C.Structure):
    _fields_ = [("running_mean", _fp * CP_N_BN), ("running_var", _fp * CP_N_BN)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)     # cp_allreduce_fn

# cp_config.options bits (include/cpnative.h CP_OPT_*): test / measurement switches of ONE call, 0 in production
OPTIONS = {"unfused_bn_bwd": 1, "unpaired_wgrad": 2, "fp8_bridge": 4, "no_small": 8, "fp8_head_f32": 16,
           "finalize_launches": 32}
CP_TILES_STATIC, CP_TILES_DYNAMIC = 0, 1


class cp_forward_record(C.Structure):
    """What the last cp_encoder_forward left in a workspace: host memory, zeroed, one per workspace buffer (include/cpnative.h)."""
    _fields_ = [("n_windows", C.c_int64), ("path", C.c_int32), ("backwards", C.c_int32), ("transposed", C.c_int32),
                ("pad", C.c_int32), ("join_event", C.c_void_p)]


class cp_config(C.Structure):
    """Everything a call depends on besides its tensors; what a forward pass leaves for the backward is in `record`."""
    _fields_ = [
        ("n_windows", C.c_int64), ("dtype", C.c_int32), ("adabn", C.c_int32),
        ("training", C.c_int32), ("step_state_lo", C.c_uint32),
        ("dp_emg", C.c_float), ("bn_momentum", C.c_float), ("bn_eps", C.c_float), ("step_state_hi", C.c_uint32),
        ("seed", C.c_uint64), ("step", C.c_uint64),
        ("options", C.c_uint32), ("tile_schedule", C.c_int32),
        ("stats_allreduce", C.c_void_p), ("stats_user", C.c_void_p), ("stats_world", C.c_int32), ("reserved0", C.c_int32),
        ("grad_tap", C.c_void_p), ("grad_tap_bytes", C.c_size_t),
        ("aux_stream", C.c_void_p), ("aux_fork", C.c_void_p), ("aux_join", C.c_void_p),
        ("record", C.POINTER(cp_forward_record)),
    ]


class cp_adam_hyper(C.Structure):
    _fields_ = [(n, C.c_float) for n in
                ("lr_emg", "lr_glove", "reg_emg", "reg_glove", "beta1", "beta2", "eps", "grad_scale")]


# every symbol include/cpnative.h declares: (restype, argtypes)
_P = C.POINTER
class cp_glove_params(C.Structure):
    _fields_ = [("w1", C.c_void_p), ("bn_g", C.c_void_p), ("bn_b", C.c_void_p), ("last_w", C.c_void_p),
                ("running_mean", C.c_void_p), ("running_var", C.c_void_p)]


class cp_online_config(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("max_windows", C.c_int32), ("vote", C.c_int32), ("phase", C.c_int32),
                ("n_coef", C.c_int32), ("reserved0", C.c_int32), ("b", C.c_double * 17), ("a", C.c_double * 17)]


class cp_online_gate_config(C.Structure):
    _fields_ = [("vote", C.c_int32), ("min_votes", C.c_int32), ("dwell", C.c_int32), ("release", C.c_int32),
                ("weight", C.c_int32), ("min_margin", C.c_float)]


class cp_online_seq_config(C.Structure):
    _fields_ = [("model", C.c_int32), ("lag", C.c_int32)]


class cp_online_drive_config(C.Structure):
    _fields_ = [("smooth", C.c_int32), ("on_level", C.c_int32), ("off_level", C.c_int32), ("rise", C.c_int32), ("fall", C.c_int32),
                ("bad_after", C.c_int32), ("good_after", C.c_int32)]


class cp_online_kin_config(C.Structure):
    _fields_ = [("smooth", C.c_int32), ("rate", C.c_int32)]


class cp_online_kf_plan(C.Structure):
    _fields_ = [("groups", C.c_uint32), ("iters", C.c_int32), ("lam", C.c_double), ("rho", C.c_double), ("kappa", C.c_double)]


class cp_online_kf_config(C.Structure):
    _fields_ = [("rate", C.c_int32), ("reserved0", C.c_int32)]


class cp_online_realign_config(C.Structure):
    _fields_ = [("max_lag", C.c_int32), ("max_lead", C.c_int32), ("min_len", C.c_int32), ("min_rest", C.c_int32),
                ("context", C.c_int32), ("min_contrast", C.c_int32), ("guard", C.c_int32)]


class cp_online_track_config(C.Structure):
    _fields_ = [("vote", C.c_int32), ("agree", C.c_int32), ("rate", C.c_double), ("min_cosine", C.c_float),
                ("min_margin", C.c_float), ("min_anchor_cosine", C.c_float), ("reserved0", C.c_int32)]


class cp_online_holdout_plan(C.Structure):
    _fields_ = [("train", C.c_uint32), ("eval", C.c_uint32), ("sums_index", C.c_int32), ("min_windows", C.c_int32),
                ("mix", C.c_double)]


class cp_augment(C.Structure):
    """Settings of one cp_gather_groups_aug launch (include/cpnative.h)."""
    _fields_ = [("seed", C.c_uint32), ("salt", C.c_uint32), ("salt_state_lo", C.c_uint32), ("salt_state_hi", C.c_uint32),
                ("shift_min", C.c_int32), ("shift_max", C.c_int32), ("dead_mask", C.c_uint32),
                ("p_drop", C.c_float), ("gain_sigma", C.c_float), ("amp_sigma", C.c_float), ("noise_sigma", C.c_float),
                ("fill", C.c_float), ("mean_std", C.c_void_p), ("item_offset", C.c_int64)]


class cp_step_state(C.Structure):
    """The 32 device bytes a captured step reads its per-step values from (include/cpnative.h)."""
    _fields_ = [("dp_salt", C.c_uint32), ("bc1", C.c_float), ("bc2", C.c_float), ("lr_emg", C.c_float), ("lr_glove", C.c_float),
                ("aug_salt", C.c_uint32), ("pad", C.c_float * 2)]


class cp_debug_fc_gemm_args(C.Structure):
    """One fc-layer GEMM launch on caller buffers (include/cpnative.h): what cp_debug_fc_gemm takes."""
    _fields_ = [("dtype", C.c_int32), ("kind", C.c_int32), ("M", C.c_int64), ("K", C.c_int32), ("F", C.c_int32),
                ("tile_schedule", C.c_int32), ("coef_mod", C.c_int32),
                ("A", C.c_void_p), ("W", C.c_void_p), ("C", C.c_void_p), ("bias", C.c_void_p), ("R", C.c_void_p),
                ("partials", C.c_void_p), ("coef", C.c_void_p),
                ("dp_thresh", C.c_uint32), ("dp_key", C.c_uint32), ("dp_inv_keep", C.c_float), ("reserved0", C.c_int32),
                ("stat_rows_out", C.POINTER(C.c_int32))]


class cp_debug_conv_args(C.Structure):
    """One launch sequence of the large-batch conv front end on caller buffers (include/cpnative.h): what cp_debug_conv takes."""
    _fields_ = [("dtype", C.c_int32), ("kind", C.c_int32), ("n_windows", C.c_int64),
                ("x", C.c_void_p), ("conv1_w", C.c_void_p), ("conv1_b", C.c_void_p), ("conv2_w", C.c_void_p), ("conv2_b", C.c_void_p),
                ("stats1", C.c_void_p), ("gin", C.c_void_p), ("gin_exp", C.c_void_p), ("gcols", C.c_void_p), ("coef", C.c_void_p),
                ("wc", C.c_void_p), ("out", C.c_void_p), ("partials", C.c_void_p), ("slabs", C.c_void_p), ("fold", C.c_void_p),
                ("dw", C.c_void_p), ("db", C.c_void_p),
                ("gcol_rows", C.c_int32), ("reserved0", C.c_int32),
                ("rows_out", C.POINTER(C.c_int32)), ("gcol_rows_out", C.POINTER(C.c_int32))]


class cp_debug_proj_args(C.Structure):
    """One launch sequence of the large-batch 512 -> 16 projection on caller buffers (include/cpnative.h): what cp_debug_proj takes."""
    _fields_ = [("dtype", C.c_int32), ("kind", C.c_int32), ("M", C.c_int64),
                ("Wp", C.c_void_p), ("act", C.c_void_p), ("r_exp", C.c_void_p), ("dz", C.c_void_p), ("scale", C.c_void_p),
                ("shift", C.c_void_p), ("coef", C.c_void_p), ("w32", C.c_void_p), ("blast", C.c_void_p), ("out", C.c_void_p),
                ("slabs", C.c_void_p), ("partials", C.c_void_p), ("praw", C.c_void_p), ("dzsum", C.c_void_p),
                ("dp_thresh", C.c_uint32), ("dp_key", C.c_uint32), ("dp_inv_keep", C.c_float), ("reserved0", C.c_int32),
                ("rows_out", C.POINTER(C.c_int32))]


class cp_debug_fp8_args(C.Structure):
    """One launch sequence of the 8-bit fc path on caller buffers and a caller scale table (include/cpnative.h): what cp_debug_fp8 takes."""
    _fields_ = [("kind", C.c_int32), ("mode", C.c_int32), ("M", C.c_int64), ("K", C.c_int32), ("F", C.c_int32),
                ("coef_mod", C.c_int32), ("t_in", C.c_int32), ("t_r", C.c_int32), ("t_out", C.c_int32), ("t_in2", C.c_int32),
                ("t_r2", C.c_int32),
                ("state", C.c_void_p), ("A", C.c_void_p), ("W", C.c_void_p), ("wsc", C.c_void_p), ("bias", C.c_void_p),
                ("R", C.c_void_p), ("coef", C.c_void_p), ("bn_stats", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p),
                ("C", C.c_void_p), ("partials", C.c_void_p), ("A2", C.c_void_p), ("R2", C.c_void_p), ("partials2", C.c_void_p),
                ("C2", C.c_void_p),
                ("dp_thresh", C.c_uint32), ("dp_key", C.c_uint32), ("dp_inv_keep", C.c_float), ("reserved0", C.c_int32),
                ("rows_out", C.POINTER(C.c_int32))]


class cp_debug_bn_args(C.Structure):
    """One f32 / bf16 BatchNorm or weight-preparation launch sequence on caller buffers (include/cpnative.h): what cp_debug_bn takes."""
    _fields_ = [("dtype", C.c_int32), ("kind", C.c_int32), ("mode", C.c_int32), ("C", C.c_int32), ("nfold", C.c_int32),
                ("K", C.c_int32), ("update_running", C.c_int32), ("reserved0", C.c_int32),
                ("M", C.c_int64), ("count", C.c_double), ("momentum", C.c_float), ("eps", C.c_float),
                ("dp_thresh", C.c_uint32), ("dp_key", C.c_uint32), ("dp_inv_keep", C.c_float), ("reserved1", C.c_int32),
                ("rows", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("running_mean", C.c_void_p),
                ("running_var", C.c_void_p), ("unscale_exp", C.c_void_p), ("scratch", C.c_void_p), ("stats", C.c_void_p),
                ("local", C.c_void_p), ("coef", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p),
                ("r", C.c_void_p), ("g", C.c_void_p), ("partials", C.c_void_p), ("db", C.c_void_p),
                ("params", C.c_void_p), ("bn", C.c_void_p),
                ("W", C.c_void_p), ("b", C.c_void_p), ("s", C.c_void_p), ("t", C.c_void_p),
                ("stats9", C.c_void_p * 9), ("wimg", C.c_void_p * 8), ("bimg", C.c_void_p * 8),
                ("rows_out", C.POINTER(C.c_int32))]


CP_ONLINE_MAX_CLASSES, CP_ONLINE_MAX_VOTE, CP_ONLINE_MAX_WINDOWS, CP_ONLINE_STRIDE = 64, 256, 256, 20
CP_ONLINE_MULTI_MAX_STREAMS, CP_ONLINE_MULTI_MAX_ROWS = 256, 65536
CP_ONLINE_GATE_SCORES, CP_ONLINE_GATE_SWEEP_MAX_CONFIGS = 10, 65536
CP_ONLINE_SEQ_RING, CP_ONLINE_SEQ_MAX_COST, CP_ONLINE_SEQ_FLOOR, CP_ONLINE_SEQ_SWEEP_MAX_CONFIGS = 64, 1 << 28, -(1 << 29), 65536
CP_ONLINE_SUBSET_SCORES, CP_ONLINE_SUBSET_SWEEP_MAX_SUBSETS = 7, 1048576
CP_ONLINE_DRIVE_ONE, CP_ONLINE_DRIVE_MAX_SMOOTH = 4096, 256
CP_ONLINE_MAP_SCORES, CP_ONLINE_MAP_SWEEP_MAX_MAPS = 3, 65536
CP_ONLINE_FINETUNE_CHUNK, CP_ONLINE_FINETUNE_PROJECTION, CP_ONLINE_FINETUNE_ROWS = 64, 1, 2
CP_ONLINE_REALIGN_MAX_ACTIVITY, CP_ONLINE_REALIGN_MAX_REGION = 4095, 4096
CP_ONLINE_TRACK_SCORES, CP_ONLINE_TRACK_SWEEP_MAX_CONFIGS = 8, 65536
CP_ONLINE_TRACK_RESET_RING, CP_ONLINE_TRACK_RESET_ROWS = 0, 1
CP_ONLINE_HOLDOUT_SCORES, CP_ONLINE_HOLDOUT_MAX_PLANS, CP_ONLINE_HOLDOUT_MAX_REPS = 9, 4096, 32
CP_ONLINE_PROTO_MAX_ROWS, CP_ONLINE_PROTO_MAX_ITERS = 4, 64
CP_ONLINE_METRIC_MOMENTS, CP_ONLINE_METRIC_MAX_SHRINKS = 152, 64
CP_ONLINE_METRIC_RESET_RING, CP_ONLINE_METRIC_RESET_ALL = 0, 1
CP_ONLINE_READOUT_MAX_GROUPS, CP_ONLINE_READOUT_MAX_PLANS, CP_ONLINE_READOUT_STAGE, CP_ONLINE_READOUT_X = 16, 256, 16, 513
CP_ONLINE_KIN_MAX_JOINTS, CP_ONLINE_KIN_MAX_SMOOTH, CP_ONLINE_KIN_ONE, CP_ONLINE_KIN_SUMS = 32, 64, 4096, 7
CP_ONLINE_KF_MAX_ITERS, CP_ONLINE_KF_PLANS_PER_LAUNCH, CP_ONLINE_KF_SUMS = 1024, 128, 8

# what the four map sweep entries take behind their workspace: rms, n_windows, mean_std, map_src, map_fill, n_maps, n_classes,
# expected_slot, chunk_rows, scratch, scratch_bytes, pred, voted, scores, class_hits, stream
_MAP_SWEEP_TAIL = [_fp, C.c_int64, _fp, _fp, _fp, C.c_int32, C.c_int32, _fp, C.c_int64, _fp, C.c_size_t, _fp, _fp, _fp, _fp, _fp]
# the *_proj entries (per-stream projections): cfg, n_streams, max_rows, ws, ws_bytes; then index, bank, bank_bytes (enrolment and
# map sweep) or, for the pushes, the arguments of cp_online_multi_push_embed with bank, bank_bytes in front of the stream
_MULTI_HEAD = [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t]
_STREAM_BANK = [C.c_int32, _fp, C.c_size_t]
_PUSH_PROJ_TAIL = [_fp, _fp, C.c_int64, C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, C.c_size_t, _fp]

SYMBOLS = {
    "cp_version": (C.c_int, []),
    "cp_last_error": (C.c_char_p, []),
    "cp_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_float]),
    "cp_gather_groups": (C.c_int, [_fp, C.c_int64, _fp, C.c_int64, _fp, C.c_int64, C.c_int32, _fp, _fp]),
    "cp_gather_oob_count": (C.c_int, [_fp, C.c_int32, _fp]),
    "cp_gather_groups_aug": (C.c_int, [_fp, C.c_int64, _fp, C.c_int64, _fp, C.c_int64, C.c_int32, _fp, _P(cp_augment), _fp]),
    "cp_encoder_forward": (C.c_int, [_P(cp_config), _P(cp_params), _P(cp_bn_buffers), _fp, _fp, C.c_size_t, _fp, _fp]),
    "cp_head": (C.c_int, [_P(cp_config), _P(cp_params), _fp, _fp, C.c_int64, C.c_int32, C.c_int32, _fp, C.c_size_t,
                          _fp, _fp, _fp, _P(cp_params), _fp]),
    "cp_global_negatives_scratch_floats": (C.c_size_t, [C.c_int64]),
    "cp_global_negatives": (C.c_int, [_P(cp_params), _fp, C.c_int64, _fp, _fp, _fp, _fp]),
    "cp_global_negatives_g": (C.c_int, [_P(cp_params), _fp, C.c_int64, _fp, _fp, _fp, _fp]),
    "cp_global_negatives_h": (C.c_int, [C.c_int64, _fp, _fp, _fp, _fp]),
    "cp_head_gneg": (C.c_int, [_P(cp_config), _P(cp_params), _fp, _fp, C.c_int64, C.c_int32, C.c_int32, _fp, C.c_size_t,
                               _fp, _fp, _fp, _P(cp_params), _fp, _fp]),
    "cp_encoder_backward": (C.c_int, [_P(cp_config), _P(cp_params), _fp, _fp, C.c_size_t, _P(cp_params), _fp]),
    "cp_encoder_backward_ev": (C.c_int, [_P(cp_config), _P(cp_params), _fp, _fp, C.c_size_t, _P(cp_params), _fp, _fp]),
    "cp_vote": (C.c_int, [_fp, _fp, C.c_int64, C.c_int32, _fp, _fp, _fp]),
    "cp_subset_vote": (C.c_int, [_fp, _fp, C.c_int64, C.c_int32, _fp, C.c_int64, _fp, _fp, _fp]),
    "cp_confusion": (C.c_int, [_fp, _fp, C.c_int64, _fp, _fp]),
    "cp_preprocess_emg": (C.c_int, [_fp, C.c_int64, C.c_int32, _P(C.c_double), _P(C.c_double), C.c_int32, C.c_int32, C.c_float,
                                    _P(C.c_int32), C.c_int32, _fp, _fp]),
    "cp_emg_stats": (C.c_int, [_fp, C.c_int64, C.c_int32, _fp, C.c_int32, _fp, _fp, _fp]),
    "cp_emg_normalize": (C.c_int, [_fp, C.c_int64, _fp, _fp]),
    "cp_glove_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "cp_glove_forward": (C.c_int, [_P(cp_config), _P(cp_glove_params), _fp, C.c_int64, _fp, C.c_size_t, _fp, _fp]),
    "cp_head_glove": (C.c_int, [_P(cp_config), _fp, _fp, _fp, C.c_int64, C.c_int32, C.c_int32, _fp, C.c_size_t, _fp,
                                C.c_size_t, _fp, _fp, _fp, _fp]),
    "cp_head_temp": (C.c_int, [_P(cp_config), _P(cp_params), _fp, _fp, C.c_int64, C.c_int32, C.c_int32, _fp, C.c_size_t,
                               _fp, _fp, _fp, _P(cp_params), _fp, _fp, _fp]),
    "cp_head_glove_temp": (C.c_int, [_P(cp_config), _fp, _fp, _fp, C.c_int64, C.c_int32, C.c_int32, _fp, C.c_size_t, _fp,
                                     C.c_size_t, _fp, _fp, _fp, _fp, _fp, _fp]),
    "cp_glove_backward": (C.c_int, [_P(cp_config), _P(cp_glove_params), C.c_int64, _fp, C.c_size_t, _P(cp_glove_params), _fp]),
    "cp_optimizer_scratch_floats": (C.c_size_t, [_P(C.c_int64), C.c_int32]),
    "cp_l2_norms": (C.c_int, [_fp, _P(C.c_int64), _P(C.c_int64), _P(C.c_int32), _P(C.c_int32), C.c_int32,
                              _P(cp_adam_hyper), _fp, _fp, _fp]),
    "cp_l2_adam_step": (C.c_int, [_fp, _fp, _fp, _fp, _P(C.c_int64), _P(C.c_int64), _P(C.c_int32), _P(C.c_int32),
                                  C.c_int32, _P(cp_adam_hyper), C.c_int64, _fp, _fp, _fp]),
    "cp_l2_adam_step_graph": (C.c_int, [_fp, _fp, _fp, _fp, _P(C.c_int64), _P(C.c_int64), _P(C.c_int32), _P(C.c_int32),
                                        C.c_int32, _P(cp_adam_hyper), _fp, _fp, _fp, _fp]),
    "cp_debug_hog": (C.c_int, [C.c_int32, C.c_int32, _fp]),
    "cp_profile_enable": (C.c_int, [C.c_uint64, C.c_int32]),
    "cp_profile_disable": (C.c_int, []),
    "cp_profile_resume": (C.c_int, []),
    "cp_profile_summary": (C.c_int, [C.c_int32, _P(C.c_double), _P(C.c_int64)]),
    "cp_debug_activation": (C.c_int, [_P(cp_config), _P(cp_params), _fp, _fp, C.c_size_t, C.c_int32, _fp, _fp]),
    "cp_debug_bn_stats": (C.c_int, [_P(cp_config), _fp, C.c_size_t, C.c_int32, _fp, _fp]),
    "cp_debug_head_grad": (C.c_int, [_P(cp_config), _fp, C.c_size_t, _fp, _fp]),
    "cp_debug_glove_head_grad": (C.c_int, [_P(cp_config), _fp, C.c_size_t, C.c_int64, _fp, _fp]),
    "cp_debug_gemm": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    "cp_debug_fc_gemm": (C.c_int, [_P(cp_debug_fc_gemm_args), _fp]),
    "cp_debug_conv": (C.c_int, [_P(cp_debug_conv_args), _fp]),
    "cp_debug_proj": (C.c_int, [_P(cp_debug_proj_args), _fp]),
    "cp_debug_fp8": (C.c_int, [_P(cp_debug_fp8_args), _fp]),
    "cp_debug_bn": (C.c_int, [_P(cp_debug_bn_args), _fp]),
    "cp_online_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "cp_online_prepare": (C.c_int, [_P(cp_online_config), _P(cp_params), _P(cp_bn_buffers), C.c_float, _fp, C.c_size_t, _fp]),
    "cp_online_set_classes": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, _fp, C.c_int32, _fp]),
    "cp_online_push": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, C.c_int64, _fp, _fp, _fp, _fp, _fp, _fp]),
    "cp_online_reset": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp]),
    "cp_online_adapt_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "cp_online_adapt_prepare": (C.c_int, [_P(cp_online_config), _P(cp_params), _P(cp_bn_buffers), C.c_float, C.c_double, _fp,
                                          C.c_size_t, _fp]),
    "cp_online_adapt_calibrate_scratch_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "cp_online_adapt_calibrate": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, C.c_int64, _fp, C.c_size_t, _fp]),
    "cp_online_adapt_push": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, C.c_int64, _fp, _fp, _fp, _fp, _fp, _fp]),
    "cp_online_adapt_statistics": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, _fp]),
    "cp_online_multi_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "cp_online_multi_prepare": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _P(cp_params), _P(cp_bn_buffers), C.c_float,
                                          _fp, C.c_size_t, _fp]),
    "cp_online_multi_set_classes": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, C.c_int32, _fp, _fp,
                                              C.c_int32, _fp]),
    "cp_online_multi_reset": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, C.c_int32, _fp]),
    "cp_online_multi_push": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, _fp, _fp, C.c_int64, C.c_int32,
                                       _fp, _fp, _fp, _fp, _fp, _fp]),
    "cp_online_multi_adapt_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "cp_online_multi_adapt_prepare": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _P(cp_params), _P(cp_bn_buffers),
                                                C.c_float, _P(C.c_double), _fp, C.c_size_t, _fp]),
    "cp_online_multi_adapt_set_alpha": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, C.c_int32,
                                                  C.c_double, _fp]),
    "cp_online_multi_adapt_reset_statistics": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, C.c_int32,
                                                         _P(cp_bn_buffers), _fp]),
    "cp_online_multi_adapt_calibrate": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, C.c_int32, _fp,
                                                  C.c_int64, _fp, C.c_size_t, _fp]),
    "cp_online_multi_adapt_push": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, _fp, _fp, C.c_int64,
                                             C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp]),
    "cp_online_multi_adapt_statistics": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, C.c_int32, _fp,
                                                   _fp]),
    "cp_online_frontend_state_bytes": (C.c_size_t, []),
    "cp_online_windows": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, C.c_int64, _fp, _fp, _fp]),
    "cp_online_enroll_scratch_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "cp_online_enroll": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, C.c_int64, _fp, C.c_int32, _fp, _fp, C.c_size_t, _fp]),
    "cp_online_adapt_enroll": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, C.c_int64, _fp, C.c_int32, _fp, _fp, C.c_size_t,
                                         _fp]),
    "cp_online_multi_enroll": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, _fp, C.c_int64, _fp, C.c_int32,
                                         _fp, _fp, C.c_size_t, _fp]),
    "cp_online_multi_adapt_enroll": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, C.c_int32, _fp, C.c_int64,
                                               _fp, C.c_int32, _fp, _fp, C.c_size_t, _fp]),
    "cp_online_enroll_table": (C.c_int, [_fp, C.c_int32, _fp, C.c_double, C.c_int32, _fp, _fp]),
    "cp_online_tail_inputs": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, C.c_int64, _fp, _fp, C.c_size_t, _fp]),
    "cp_online_adapt_tail_inputs": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, C.c_int64, _fp, _fp, C.c_size_t, _fp]),
    "cp_online_multi_tail_inputs": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, _fp, C.c_int64, _fp, _fp,
                                              C.c_size_t, _fp]),
    "cp_online_multi_adapt_tail_inputs": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, C.c_int32, _fp,
                                                    C.c_int64, _fp, _fp, C.c_size_t, _fp]),
    "cp_online_finetune_state_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "cp_online_finetune_init": (C.c_int, [_fp, C.c_size_t, C.c_int32, _fp, _fp, _fp, _fp, C.c_int64, C.c_int32, C.c_int32, _fp]),
    "cp_online_finetune_steps": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, C.c_int64, C.c_int32, C.c_int32, C.c_double,
                                           C.c_double, C.c_double, C.c_double, C.c_int32, _fp, _fp]),
    "cp_online_finetune_read": (C.c_int, [_fp, C.c_size_t, C.c_int64, C.c_int32, _fp, _fp, _fp, _fp, _fp]),
    "cp_online_set_projection": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, _fp, _fp]),
    "cp_online_adapt_set_projection": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, _fp, _fp]),
    "cp_online_projection": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, _fp, _fp]),
    "cp_online_adapt_projection": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, _fp, _fp]),
    "cp_online_multi_projection": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, _fp, _fp, _fp]),
    "cp_online_multi_adapt_projection": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, _fp, _fp, _fp]),
    "cp_online_gate_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "cp_online_gate_set_classes": (C.c_int, [_P(cp_online_gate_config), C.c_int32, _fp, C.c_size_t, C.c_int32, _P(C.c_int32),
                                             _P(C.c_float), C.c_int32, _fp]),
    "cp_online_gate_reset": (C.c_int, [_P(cp_online_gate_config), C.c_int32, _fp, C.c_size_t, C.c_int32, _fp]),
    "cp_online_gate_push": (C.c_int, [_P(cp_online_gate_config), C.c_int32, _fp, C.c_size_t, _fp, C.c_int32, _fp, _fp, C.c_int32,
                                      _fp, _fp, _fp, _fp, _fp]),
    "cp_online_drive_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "cp_online_drive_set_profile": (C.c_int, [_P(cp_online_drive_config), C.c_int32, _fp, C.c_size_t, C.c_int32, _P(C.c_int32),
                                              C.c_int32, _P(C.c_float), _P(C.c_float), _P(C.c_int32), _P(C.c_float), _P(C.c_float),
                                              _fp]),
    "cp_online_drive_reset": (C.c_int, [_P(cp_online_drive_config), C.c_int32, _fp, C.c_size_t, C.c_int32, _fp]),
    "cp_online_drive_push": (C.c_int, [_P(cp_online_drive_config), C.c_int32, _fp, C.c_size_t, _fp, C.c_int32, _fp, _fp, _fp,
                                       C.c_int32, _fp, _fp, _fp, _fp]),
    "cp_online_gate_sweep_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "cp_online_gate_sweep": (C.c_int, [_fp, C.c_int32, C.c_int64, C.c_int32, _fp, _fp, _fp, C.c_int32, _fp, C.c_size_t, _fp, _fp,
                                       _fp]),
    "cp_online_seq_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "cp_online_seq_set_model": (C.c_int, [C.c_int32, _fp, C.c_size_t, C.c_int32, _P(C.c_int32), _P(C.c_float), C.c_int32, _fp,
                                          C.c_int32, _fp]),
    "cp_online_seq_reset": (C.c_int, [C.c_int32, _fp, C.c_size_t, C.c_int32, _fp]),
    "cp_online_seq_push": (C.c_int, [C.c_int32, _fp, C.c_size_t, _fp, C.c_int32, _fp, _fp, C.c_int32, _fp, _fp, _fp, _fp]),
    "cp_online_seq_sweep_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "cp_online_seq_sweep": (C.c_int, [_fp, C.c_int32, C.c_int64, C.c_int32, _fp, _fp, C.c_int32, _fp, _fp, C.c_int32, _fp, C.c_size_t,
                                      _fp, _fp, _fp]),
    "cp_online_subset_sweep_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "cp_online_subset_sweep": (C.c_int, [_fp, C.c_int32, C.c_int64, C.c_int32, _fp, _fp, C.c_int32, C.c_int32, _fp, C.c_size_t, _fp,
                                         _fp, _fp]),
    "cp_online_push_mapped": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, C.c_int64, _fp, _fp, _fp, _fp, _fp, _fp, _fp,
                                        _fp]),
    "cp_online_adapt_push_mapped": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, C.c_int64, _fp, _fp, _fp, _fp, _fp, _fp, _fp,
                                              _fp]),
    "cp_online_multi_push_mapped": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, _fp, _fp, C.c_int64,
                                              C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    "cp_online_multi_adapt_push_mapped": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, _fp, _fp, C.c_int64,
                                                    C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    "cp_online_windows_mapped": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, C.c_int64, _fp, _fp, _fp, _fp, _fp]),
    "cp_online_map_sweep_scratch_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "cp_online_map_sweep": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t] + _MAP_SWEEP_TAIL),
    "cp_online_adapt_map_sweep": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t] + _MAP_SWEEP_TAIL),
    "cp_online_multi_map_sweep": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, C.c_int32] + _MAP_SWEEP_TAIL),
    "cp_online_multi_adapt_map_sweep": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, C.c_int32]
                                        + _MAP_SWEEP_TAIL),
    "cp_online_realign_activity": (C.c_int, [_fp, C.c_int32, C.c_int64, _P(C.c_float), _P(C.c_float), _fp, _fp]),
    "cp_online_realign": (C.c_int, [_fp, _fp, C.c_int64, _fp, C.c_int32, _P(cp_online_realign_config), _fp, _fp, _fp, _fp]),
    "cp_online_push_embed": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, C.c_int64, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp,
                                       _fp]),
    "cp_online_adapt_push_embed": (C.c_int, [_P(cp_online_config), _fp, C.c_size_t, _fp, C.c_int64, _fp, _fp, _fp, _fp, _fp, _fp, _fp,
                                             _fp, _fp]),
    "cp_online_multi_push_embed": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, _fp, _fp, C.c_int64,
                                             C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    "cp_online_multi_adapt_push_embed": (C.c_int, [_P(cp_online_config), C.c_int32, C.c_int32, _fp, C.c_size_t, _fp, _fp, C.c_int64,
                                                   C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    "cp_online_track_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "cp_online_track_set_rows": (C.c_int, [_P(cp_online_track_config), C.c_int32, _fp, C.c_size_t, C.c_int32, _P(C.c_int32), _fp,
                                           C.c_int32, _fp]),
    "cp_online_track_reset": (C.c_int, [_P(cp_online_track_config), C.c_int32, _fp, C.c_size_t, C.c_int32, C.c_int32, _fp]),
    "cp_online_track_push": (C.c_int, [_P(cp_online_track_config), C.c_int32, _fp, C.c_size_t, _fp, _fp, _fp, C.c_int32, _fp, _fp,
                                       _fp, C.c_int32, _fp, _fp]),
    "cp_online_track_rows": (C.c_int, [_P(cp_online_track_config), C.c_int32, _fp, C.c_size_t, C.c_int32, _fp, _fp, _fp, _fp]),
    "cp_online_track_sweep": (C.c_int, [_fp, C.c_int64, C.c_int32, _fp, _fp, C.c_int64, _fp, C.c_int32, _fp, _fp, _fp, _fp, _fp]),
    "cp_online_holdout_sums": (C.c_int, [_fp, C.c_int64, C.c_int32, _fp, _fp, _fp, C.c_int32, _fp, _fp]),
    "cp_online_holdout_tables": (C.c_int, [_fp, C.c_int32, C.c_int32, _fp, _fp, C.c_int32, _fp, _fp, _fp]),
    "cp_online_holdout_score": (C.c_int, [_fp, C.c_int64, C.c_int32, _fp, _fp, _fp, _fp, C.c_int32, C.c_int32, _fp, _fp, _fp, _fp, _fp,
                                          _fp]),
    "cp_online_holdout_logits": (C.c_int, [_fp, C.c_int64, C.c_int32, _fp, C.c_int32, _fp, _fp, C.c_int32, _fp]),
    "cp_online_proto_fit": (C.c_int, [_fp, C.c_int64, C.c_int32, _fp, _fp, _P(C.c_int32), C.c_int32, C.c_int32, _fp, _fp, _fp, _fp,
                                      _fp, _fp]),
    "cp_online_group_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "cp_online_group_set_groups": (C.c_int, [C.c_int32, C.c_int32, _fp, C.c_size_t, C.c_int32, _P(C.c_int32), _P(C.c_int32),
                                             C.c_int32, _fp]),
    "cp_online_group_reset": (C.c_int, [C.c_int32, C.c_int32, _fp, C.c_size_t, C.c_int32, _fp]),
    "cp_online_group_push": (C.c_int, [C.c_int32, C.c_int32, _fp, C.c_size_t, _fp, C.c_int32, _fp, _fp, C.c_int32, _fp, _fp, _fp,
                                       _fp, C.c_int32, _fp]),
    "cp_online_metric_moments": (C.c_int, [_fp, C.c_int64, C.c_int32, _fp, _fp, _fp, _fp, _fp]),
    "cp_online_metric_factor": (C.c_int, [_fp, _fp, C.c_int32, C.c_int32, _P(C.c_double), C.c_int32, _fp, _fp, _fp]),
    "cp_online_metric_apply": (C.c_int, [_fp, C.c_int64, _fp, _fp, _fp]),
    "cp_online_metric_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "cp_online_metric_set": (C.c_int, [C.c_int32, C.c_int32, _fp, C.c_size_t, C.c_int32, _fp, _fp, _P(C.c_int32), C.c_int32, _fp]),
    "cp_online_metric_reset": (C.c_int, [C.c_int32, C.c_int32, _fp, C.c_size_t, C.c_int32, C.c_int32, _fp]),
    "cp_online_metric_push": (C.c_int, [C.c_int32, C.c_int32, _fp, C.c_size_t, _fp, _fp, _fp, C.c_int32, _fp, _fp, _fp, C.c_int32,
                                        _fp]),
    "cp_online_readout_scratch_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "cp_online_readout_moments": (C.c_int, [_fp, C.c_int32, C.c_int64, _fp, _fp, _fp, _fp, C.c_int32, C.c_int32, _fp, _fp, _fp, C.c_size_t,
                                            _fp]),
    "cp_online_readout_solve": (C.c_int, [_fp, _fp, C.c_int32, _P(C.c_uint32), _P(C.c_double), C.c_int32, _fp, _fp, _fp, _fp, C.c_size_t,
                                          _fp]),
    "cp_online_readout_apply": (C.c_int, [_fp, C.c_int32, C.c_int64, _fp, _fp, C.c_int32, _fp, _fp, C.c_size_t, _fp]),
    "cp_online_projections_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "cp_online_projections_set": (C.c_int, [C.c_int32, _fp, C.c_size_t, C.c_int32, C.c_int32, _fp, _fp, _fp]),
    "cp_online_projections_get": (C.c_int, [C.c_int32, _fp, C.c_size_t, C.c_int32, C.c_int32, _fp, _fp, _fp, _fp]),
    "cp_online_projections_clear": (C.c_int, [C.c_int32, _fp, C.c_size_t, C.c_int32, C.c_int32, _fp]),
    "cp_online_multi_push_proj": (C.c_int, _MULTI_HEAD + _PUSH_PROJ_TAIL),
    "cp_online_multi_adapt_push_proj": (C.c_int, _MULTI_HEAD + _PUSH_PROJ_TAIL),
    "cp_online_multi_enroll_proj": (C.c_int, _MULTI_HEAD + _STREAM_BANK + [_fp, C.c_int64, _fp, C.c_int32, _fp, _fp, C.c_size_t, _fp]),
    "cp_online_multi_adapt_enroll_proj": (C.c_int, _MULTI_HEAD + _STREAM_BANK + [_fp, C.c_int64, _fp, C.c_int32, _fp, _fp, C.c_size_t,
                                                                                _fp]),
    "cp_online_multi_map_sweep_proj": (C.c_int, _MULTI_HEAD + _STREAM_BANK + _MAP_SWEEP_TAIL),
    "cp_online_multi_adapt_map_sweep_proj": (C.c_int, _MULTI_HEAD + _STREAM_BANK + _MAP_SWEEP_TAIL),
    "cp_online_tail_offset": (C.c_size_t, [_P(cp_online_config), C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "cp_online_kin_moments": (C.c_int, [_fp, C.c_int32, C.c_int64, _fp, _fp, _fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, _fp,
                                        C.c_size_t, _fp]),
    "cp_online_kin_apply": (C.c_int, [_fp, C.c_int32, C.c_int64, _fp, _fp, C.c_int32, C.c_int32, _fp, _fp]),
    "cp_online_kin_score": (C.c_int, [_fp, _fp, C.c_int32, _fp, _P(C.c_uint32), C.c_int32, C.c_int64, C.c_int32, _fp, _fp]),
    "cp_online_kin_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "cp_online_kin_set_model": (C.c_int, [_P(cp_online_kin_config), C.c_int32, _fp, C.c_size_t, C.c_int32, _fp, _fp, C.c_int32,
                                          _P(C.c_float), _P(C.c_float), _P(C.c_int32), _fp]),
    "cp_online_kin_reset": (C.c_int, [_P(cp_online_kin_config), C.c_int32, _fp, C.c_size_t, C.c_int32, _fp]),
    "cp_online_kin_push": (C.c_int, [_P(cp_online_kin_config), C.c_int32, _fp, C.c_size_t, _fp, C.c_int32, C.c_int32, _fp, _fp, _fp,
                                     C.c_int32, _fp, _fp, _fp, _fp]),
    "cp_online_kf_moments": (C.c_int, [_fp, _fp, _fp, C.c_int64, C.c_int32, C.c_int32, _P(C.c_float), _fp, _fp, _fp, _fp, _fp, _fp]),
    "cp_online_kf_design_bytes": (C.c_size_t, [C.c_int32]),
    "cp_online_kf_design": (C.c_int, [_fp, _fp, _fp, _fp, _fp, C.c_int32, C.c_int32, _P(cp_online_kf_plan), C.c_int32, _fp, _fp, _fp,
                                      _fp, _fp, C.c_size_t, _fp]),
    "cp_online_kf_sweep": (C.c_int, [_fp, _fp, _fp, C.c_int64, C.c_int32, _P(C.c_uint32), C.c_int32, _fp, _fp, _P(C.c_float), _fp, _fp,
                                     _fp]),
    "cp_online_kf_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "cp_online_kf_set_model": (C.c_int, [_P(cp_online_kf_config), C.c_int32, _fp, C.c_size_t, C.c_int32, _fp, _fp, C.c_int32,
                                         _P(C.c_float), _P(C.c_float), _P(C.c_int32), _fp, _fp, _fp]),
    "cp_online_kf_reset": (C.c_int, [_P(cp_online_kf_config), C.c_int32, _fp, C.c_size_t, C.c_int32, _fp]),
    "cp_online_kf_push": (C.c_int, [_P(cp_online_kf_config), C.c_int32, _fp, C.c_size_t, _fp, C.c_int32, C.c_int32, _fp, _fp, _fp,
                                    C.c_int32, _fp, _fp, _fp, _fp, _fp]),
}

KERNEL_KINDS = ["gather", "prep", "conv1_fwd", "bn_finalize", "conv2_fwd", "fold", "fc_fwd", "dropout", "proj_fwd",
                "head", "proj_bwd", "bn_bwd", "fc_wgrad", "reduce_slabs", "fc_dgrad", "conv2_wgrad", "conv2_dgrad",
                "conv1_bwd", "optimizer", "fc_dgrad_stats", "fc_dgrad_bn", "fc_fwd_ws", "fc_dgrad_conv"]

_lib = None


class CpNativeError(RuntimeError):
    pass


def load():
    """Load libcpnative.so (built by ``__graft_entry__.build()`` / ``csrc/Makefile``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CpNativeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    # torch first: its wheel carries its own HIP runtime (torch/lib/libamdhip64.so), and the process must end up with ONE runtime -- the
    # one that owns torch's allocations and streams.  With libcpnative.so loaded first the dynamic loader binds it to /opt/rocm's copy,
    # torch then brings its own, and every launch of this library fails with hipErrorNoDevice on the box (seen: build() and smoke() in
    # one process).  Loaded behind torch, the library resolves against the runtime that is already there.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.cp_version() < 112:
        raise CpNativeError("libcpnative.so is older than this binding")
    _lib = lib
    return lib


def check(code: int, what: str):
    if code != 0:
        msg = load().cp_last_error().decode("utf-8", "replace")
        raise CpNativeError(f"{what} failed: {msg}")
