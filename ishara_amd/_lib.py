"""ctypes binding of libishara_hip.so (C ABI declared in include/ishara_hip.h).

There is no CPU fallback: if the shared library is missing this module raises, and every
entry point that needs a GPU fails loudly through IsharaError.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libishara_hip.so")

F32, BF16, F16 = 0, 1, 2
FAMILY_KERAS_HYBRID, FAMILY_TORCH_CONFORMER, FAMILY_TORCH_SQUEEZEFORMER = 0, 1, 2


class IsharaError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [
        ("dim", C.c_int32), ("num_conv_squeeze_blocks", C.c_int32), ("num_conv_conform_blocks", C.c_int32),
        ("num_kernel_sizes", C.c_int32), ("kernel_sizes", C.c_int32 * 8), ("num_conv_per_block", C.c_int32),
        ("dropout_rate", C.c_float), ("num_heads", C.c_int32), ("expansion_factor", C.c_int32),
        ("transformer_kernel_size", C.c_int32), ("frames", C.c_int32), ("features", C.c_int32),
        ("num_classes", C.c_int32), ("top_dim", C.c_int32), ("squeeze_expansion", C.c_int32),
        ("conformer_expansion", C.c_int32), ("head_dropout", C.c_float), ("conformer_attn_dropout", C.c_float),
        ("dtype", C.c_int32), ("max_batch", C.c_int32), ("max_label_len", C.c_int32), ("attn_impl", C.c_int32),
        ("family", C.c_int32), ("reduce_layer_index", C.c_int32), ("recover_layer_index", C.c_int32), ("half_step_residual", C.c_int32),
    ]


class ClipAug(C.Structure):
    """ishara_clip_aug: one clip's augmentation parameters for ishara_clip_batch (64 bytes, field order of the header)."""
    _fields_ = [
        ("offset", C.c_int64), ("n", C.c_int32), ("L1", C.c_int32), ("shift", C.c_int32), ("L2", C.c_int32),
        ("mirror", C.c_int32), ("t0", C.c_int32 * 3), ("t1", C.c_int32 * 3), ("fingers", C.c_int32 * 3),
    ]


class ClipAugEx(C.Structure):
    """ishara_clip_aug_ex: ClipAug plus the spatial affine and the temporal mask for ishara_clip_batch_ex (96 bytes, field order of the header)."""
    _fields_ = [
        ("base", ClipAug), ("m", C.c_float * 4), ("shift_xy", C.c_float), ("m0", C.c_int32), ("m1", C.c_int32), ("reserved", C.c_int32),
    ]


LAYOUT_FLAT, LAYOUT_HANDS_LIPS_XY = 0, 1


class GradStats(C.Structure):
    """ishara_grad_stats: the 16-byte device record of ishara_gradient_stats / ishara_optimizer_step_ex (field order of the header)."""
    _fields_ = [("norm", C.c_float), ("coef", C.c_float), ("nonfinite", C.c_int32), ("skipped", C.c_int32)]


class EmaState(C.Structure):
    """ishara_ema_state: the 16-byte device record of ishara_weight_average (field order of the header)."""
    _fields_ = [("updates", C.c_int64), ("alpha", C.c_float), ("overwrote", C.c_int32)]


class AwpStats(C.Structure):
    """ishara_awp_stats: the 16-byte device record of ishara_awp_perturb (field order of the header)."""
    _fields_ = [("grad_norm", C.c_float), ("delta_norm", C.c_float), ("perturbed", C.c_int32), ("zeroed", C.c_int32)]


class ParamGroup(C.Structure):
    """ishara_param_group: one 16-byte device row of ishara_optimizer_step_groups, per segment (field order of the header)."""
    _fields_ = [("lr_scale", C.c_float), ("wd_scale", C.c_float), ("frozen", C.c_int32), ("reserved", C.c_int32)]


class KdStage(C.Structure):
    """ishara_kd_stage: the distillation stage of ishara_loss_backward_kd (field order of the header)."""
    _fields_ = [("teacher", C.c_void_p), ("inv_temp", C.c_float), ("mode", C.c_int32), ("kd_scale", C.c_float), ("kl_frame", C.c_void_p),
                ("kl_clip", C.c_void_p)]


class NbestStage(C.Structure):
    """ishara_nbest_stage: the n-best stage of ishara_loss_backward_kd, the arguments of ishara_loss_backward_nbest (field order of the header)."""
    _fields_ = [("hyp_idx", C.c_void_p), ("hyp_len", C.c_void_p), ("N", C.c_int32), ("Th", C.c_int32), ("max_len", C.c_int32), ("coef", C.c_void_p),
                ("risk_scale", C.c_float), ("workspace", C.c_void_p)]


class GemmTnCall(C.Structure):
    """ishara_gemm_tn_call: one weight-gradient GEMM of ishara_op_gemm_tn / ishara_debug_gemm_tn_plan (field order of the header)."""
    _fields_ = [
        ("A", C.c_void_p), ("B", C.c_void_p), ("out", C.c_void_p), ("dbias", C.c_void_p), ("bias_rowscale", C.c_void_p),
        ("P", C.c_void_p), ("Q", C.c_void_p), ("W", C.c_void_p), ("G", C.c_void_p), ("Rpart", C.c_void_p),
        ("dtA", C.c_int32), ("dtB", C.c_int32), ("dtM", C.c_int32),
        ("M", C.c_int32), ("Ka", C.c_int32), ("Nb", C.c_int32), ("ka_valid", C.c_int32), ("nb_valid", C.c_int32),
        ("bias_T", C.c_int32), ("psa_T", C.c_int32), ("ldw", C.c_int32), ("reserved", C.c_int32),
    ]


class GemmNtCall(C.Structure):
    """ishara_gemm_nt_call: one forward / dgrad GEMM of ishara_op_gemm_nt / ishara_debug_gemm_nt_route (field order of the header)."""
    _fields_ = [
        ("A", C.c_void_p), ("Bt", C.c_void_p), ("C", C.c_void_p), ("c1", C.c_void_p), ("c0", C.c_void_p),
        ("bias", C.c_void_p), ("addtab", C.c_void_p), ("pre_out", C.c_void_p), ("rowscale", C.c_void_p), ("aux", C.c_void_p), ("resid", C.c_void_p),
        ("q", C.c_void_p), ("k", C.c_void_p), ("vt", C.c_void_p),
        ("dtA", C.c_int32), ("dtM", C.c_int32), ("dtC", C.c_int32), ("op", C.c_int32),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("bt_rows", C.c_int32), ("ldb", C.c_int32),
        ("op_seed", C.c_uint32), ("op_site", C.c_uint32), ("op_rate", C.c_float),
        ("tab_period", C.c_int32), ("act", C.c_int32),
        ("drop_seed", C.c_uint32), ("drop_site", C.c_uint32), ("drop_rate", C.c_float),
        ("T", C.c_int32), ("rowscale_bias", C.c_int32), ("dact", C.c_int32), ("mode", C.c_int32), ("H", C.c_int32), ("dh", C.c_int32),
        ("head_major", C.c_int32),
    ]


class GemmAsExt(C.Structure):
    """ishara_gemm_as_ext: the A-stationary-only fields of ishara_op_gemm_as / ishara_debug_gemm_as_plan (field order of the header)."""
    _fields_ = [
        ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p), ("ln_mean", C.c_void_p), ("ln_rstd", C.c_void_p),
        ("pa_P", C.c_void_p), ("pa_Q", C.c_void_p), ("pro_out", C.c_void_p),
        ("ln_eps", C.c_float), ("ldc", C.c_int32), ("n_valid", C.c_int32), ("as_flags", C.c_int32),
    ]


class GemmAsPlan(C.Structure):
    """ishara_gemm_as_plan: what ishara_debug_gemm_as_plan reports (field order of the header)."""
    _fields_ = [
        ("route", C.c_char_p), ("kernel", C.c_char_p),
        ("rows", C.c_int32), ("gx", C.c_int32), ("gy", C.c_int32), ("nsteps", C.c_int32), ("ring", C.c_int32), ("cs", C.c_int32), ("waves", C.c_int32),
        ("passes", C.c_int32), ("pass_rows", C.c_int32 * 2), ("chunked", C.c_int32), ("hold", C.c_int32), ("inst_mask", C.c_int32), ("prologue", C.c_int32),
    ]


class StreamState(C.Structure):
    """ishara_stream_state: the device arrays of S streaming sessions (field order of the header); passed by address."""
    _fields_ = [
        ("raw", C.c_void_p), ("hand", C.c_void_p), ("counters", C.c_void_p), ("hist", C.c_void_p), ("hist_len", C.c_void_p), ("committed", C.c_void_p),
        ("S", C.c_int32), ("window", C.c_int32), ("T", C.c_int32), ("agree", C.c_int32),
    ]


# name -> (restype, argtypes); every symbol include/ishara_hip.h declares
_P, _I32, _I64, _U32, _F = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_float
SIGNATURES = {
    "ishara_last_error": (C.c_char_p, []),
    "ishara_create": (C.c_int, [C.POINTER(Config), C.POINTER(_P)]),
    "ishara_destroy": (None, [_P]),
    "ishara_param_total": (_I64, [_P]),
    "ishara_param_trainable": (_I64, [_P]),
    "ishara_param_entries": (_I32, [_P]),
    "ishara_param_info": (C.c_int, [_P, _I32, C.POINTER(C.c_char_p), C.POINTER(_I32), C.POINTER(_I64 * 2), C.POINTER(_I64), C.POINTER(_I32)]),
    "ishara_workspace_bytes": (_I64, [_P]),
    "ishara_workspace_plan_check": (_I32, [_P]),
    "ishara_workspace_guard_check": (C.c_int, [_P]),
    "ishara_grad_buckets": (_I32, [_P]),
    "ishara_grad_bucket": (C.c_int, [_P, _I32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ishara_grad_buckets_enable": (C.c_int, [_P]),
    "ishara_grad_bucket_wait": (C.c_int, [_P, _I32, _P]),
    "ishara_bind": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _I64]),
    "ishara_sync_weights": (C.c_int, [_P, _P]),
    "ishara_forward": (C.c_int, [_P, _P, _I32, _P, _I32, _U32, _P]),
    "ishara_forward_ex": (C.c_int, [_P, _P, _I32, _P, _I32, _U32, _P, _P]),
    "ishara_loss_backward_ex": (C.c_int, [_P, _P, _P, _I32, _P, _P, _F, _P, _P]),
    "ishara_frame_lengths": (C.c_int, [_P, _I32, _I32, _I32, _P, _P]),
    "ishara_encoder_forward": (C.c_int, [_P, _P, _I32, _P, _I32, _U32, _P]),
    "ishara_encoder_backward": (C.c_int, [_P, _P, _I32, _P, _P]),
    "ishara_encoder_forward_ex": (C.c_int, [_P, _P, _I32, _P, _I32, _U32, _P, _P, _P]),
    "ishara_encoder_backward_ex": (C.c_int, [_P, _P, _I32, _P, _P, _P, _P]),
    "ishara_encoder_forward_lengths": (C.c_int, [_P, _P, _I32, _P, _I32, _U32, _P, _P]),
    "ishara_encoder_backward_lengths": (C.c_int, [_P, _P, _I32, _P, _P, _P]),
    "ishara_encoder_output_frames": (_I32, [_P]),
    "ishara_loss_backward": (C.c_int, [_P, _P, _P, _I32, _P, _P, _F, _P]),
    "ishara_optimizer_step": (C.c_int, [_P, _F, _F, _P]),
    "ishara_optimizer_iterations": (_I32, [_P]),
    "ishara_optimizer_set_iterations": (C.c_int, [_P, _I32]),
    "ishara_grad_stats_workspace_bytes": (_I64, [_I64]),
    "ishara_gradient_stats": (C.c_int, [_P, _P, _I64, _F, _F, _P, _P, _P]),
    "ishara_gradient_accumulate": (C.c_int, [_P, _P, _P, _I64, _I32, _P]),
    "ishara_optimizer_step_ex": (C.c_int, [_P, _F, _F, _P, _P, _I32, _P]),
    "ishara_weight_average": (C.c_int, [_P, _P, _P, _I64, _F, _I32, _I32, _P, _P, _I32, _P]),
    "ishara_weight_swap": (C.c_int, [_P, _P, _P, _I64, _P]),
    "ishara_awp_workspace_bytes": (_I64, [_I64, _I32]),
    "ishara_awp_perturb": (C.c_int, [_P, _P, _P, _P, _P, _I32, _I64, _F, _F, _I32, _P, _P, _P, _P]),
    "ishara_awp_restore": (C.c_int, [_P, _P, _P, _I64, _P]),
    "ishara_param_groups_workspace_bytes": (_I64, [_I64, _I32]),
    "ishara_optimizer_step_groups": (C.c_int, [_P, _F, _F, _P, _P, _I32, _P, _P, _I32, _P, _P]),
    "ishara_gradient_mask_groups": (C.c_int, [_P, _P, _I64, _P, _P, _I32, _P, _P]),
    "ishara_optimizer_op_step": (C.c_int, [_P, _P, _P, _P, _P, _I64, _I32, _F, _F, _P, _I32, _P]),
    "ishara_optimizer_op_step_groups": (C.c_int, [_P, _P, _P, _P, _P, _I64, _I32, _F, _F, _P, _I32, _P, _P, _I32, _P, _P]),
    "ishara_profile_enable": (C.c_int, [_P, _I32]),
    "ishara_profile_report": (C.c_int, [_P, C.c_char_p, _I32]),
    "ishara_greedy_decode": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _P]),
    "ishara_greedy_decode_ex": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _P, _P]),
    "ishara_preprocess": (C.c_int, [_P, _P, _I32, _P, _P, _P, _I32, _P]),
    "ishara_preprocess_batch": (C.c_int, [_P, _I64, _P, _I32, _I32, _P, _P, _P, _I32, _P]),
    "ishara_stream_append": (C.c_int, [C.POINTER(StreamState), _P, _I64, _P, _P, _P, _P]),
    "ishara_preprocess_sessions": (C.c_int, [_P, _P, _I32, _P, _I32, _I32, _P, _P, _P, _I32, _P]),
    "ishara_stream_agree": (C.c_int, [C.POINTER(StreamState), _P, _P, _P, _P, _I32, _I32, _P, _P, _P]),
    "ishara_edit_distance": (C.c_int, [_P, _P, _I32, _I32, _P, _I32, _P, _P, _P]),
    "ishara_edit_alignment_workspace_bytes": (_I64, [_I32, _I32]),
    "ishara_edit_alignment": (C.c_int, [_P, _P, _I32, _I32, _P, _I32, _I32, _P, _P, _P, _P, _P, _P]),
    "ishara_ctc_beam_workspace_bytes": (_I64, [_I32, _I32, _I32, _I32]),
    "ishara_ctc_beam_decode": (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _F, _F, _P, _P, _P, _P, _P]),
    "ishara_ctc_beam_decode_ex": (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _F, _F, _P, _P, _P, _P, _P, _P]),
    "ishara_ctc_beam_decode_lm": (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _I32, _I32, _F, _F, _P, _P, _P, _P, _P, _P]),
    "ishara_ctc_align_workspace_bytes": (_I64, [_I32, _I32, _I32]),
    "ishara_ctc_align": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "ishara_ctc_align_ex": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ishara_logits_combine": (C.c_int, [_P, C.POINTER(_P), _I32, _I32, _I32, _I32, _P, _P, _I32, _P, _P, _P]),
    "ishara_mbr_select": (C.c_int, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ishara_ctc_score_nbest": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _I32, _I32, _P, _P, _P, _P]),
    "ishara_debug_set_score_group": (C.c_int, [_I32]),
    "ishara_nbest_rescore": (C.c_int, [_P, _P, _I32, _I32, _I32, C.POINTER(_P), _I32, _P, _P, _P, _I32, _I32, _I32, _I32, _F, _F, _P, _P, _P, _P, _P, _P, _P]),
    "ishara_nbest_rescore_p": (C.c_int, [_P, _P, _I32, _I32, _I32, C.POINTER(_P), _I32, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "ishara_rescore_sweep_workspace_bytes": (_I64, [_I32, _I32, _I32]),
    "ishara_rescore_sweep": (C.c_int, [_P, _P, _I32, _I32, _I32, C.POINTER(_P), _I32, _P, _P, _I32, _I32, _I32, _I32, _P, _I32, _I32, _P, _I32, _P, _P, _P, _P,
                                       _P, _P, _P]),
    "ishara_ctc_nbest_grad_workspace_bytes": (_I64, [_I32, _I32, _I32, _I32]),
    "ishara_ctc_nbest_grad": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _I32, _I32, _I32, _P, _P, _F, _P, _I32, _P, _P, _P, _P, _P]),
    "ishara_mwer_weights": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _P, _I32, _P, _I32, _P, _P, _P, _P, _P, _P]),
    "ishara_loss_backward_nbest": (C.c_int, [_P, _P, _P, _I32, _P, _P, _F, _P, _P, _P, _I32, _I32, _I32, _P, _F, _P, _P]),
    "ishara_kd_grad": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _F, _I32, _P, _F, _P, _I32, _P, _P, _P, _P]),
    "ishara_loss_backward_kd": (C.c_int, [_P, _P, _P, _I32, _P, _P, _F, _P, C.POINTER(KdStage), C.POINTER(NbestStage), _P]),
    "ishara_clip_batch": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P]),
    "ishara_clip_batch_ex": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P, _P]),
    "ishara_ctc_workspace_bytes": (_I64, [_I32, _I32, _I32]),
    "ishara_ctc_loss": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P, _F, _P, _P]),
    "ishara_ctc_loss_ex": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P, _F, _P, _P, _P, _U32, _P]),
    "ishara_op_ctc_loss": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P, _F, _P, _P, _P]),
    "ishara_dropout_mask": (C.c_int, [_U32, _U32, _I32, _I32, _F, _P, _P]),
    "ishara_debug_set_as_flags": (C.c_int, [_I32]),
    "ishara_debug_dense_kernel_name": (C.c_char_p, [_I32, _I32, _I32, _I32, _I32, _I32]),
    "ishara_debug_dwconv_kernel_name": (C.c_char_p, [_I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32]),
    "ishara_debug_attn_kernel_name": (C.c_char_p, [_I32, _I32, _I32, _I32, _I32, _I32]),
    "ishara_debug_conv_block_route_name": (C.c_char_p, [_I32, _I32, _I32, _I32, _I32, _I32, _I32]),
    "ishara_debug_set_nt_big": (C.c_int, [_I32]),
    "ishara_debug_force_regstage": (C.c_int, [_I32]),
    "ishara_debug_module_count": (_I32, [_P]),
    "ishara_debug_module_info": (C.c_int, [_P, _I32, C.POINTER(C.c_char_p), C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I32)]),
    "ishara_debug_module_forward": (C.c_int, [_P, _I32, _P, _I32, _P, _I32, _U32, _P]),
    "ishara_debug_module_backward": (C.c_int, [_P, _I32, _P, _I32, _P, _P]),
    "ishara_debug_head_loss_backward": (C.c_int, [_P, _P, _P, _I32, _P, _P, _F, _P, _P]),
    "ishara_debug_module_forward_ex": (C.c_int, [_P, _I32, _P, _I32, _P, _I32, _U32, _P, _P]),
    "ishara_debug_module_backward_ex": (C.c_int, [_P, _I32, _P, _I32, _P, _P, _P]),
    "ishara_op_scratch_bytes": (_I64, [_I32, _I32, _I32]),
    "ishara_op_dense_fwd": (C.c_int, [_I32, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _P]),
    "ishara_op_dense_fwd_ex": (C.c_int, [_I32, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _P]),
    "ishara_op_dense_bwd": (C.c_int, [_I32, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _P, _P]),
    "ishara_op_gemm_tn_scratch_bytes": (_I64, [C.POINTER(GemmTnCall), _I32]),
    "ishara_op_gemm_tn": (C.c_int, [C.POINTER(GemmTnCall), _I32, _P, _P, _P, _P]),
    "ishara_debug_gemm_tn_plan": (C.c_int, [C.POINTER(GemmTnCall), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(_I32), C.POINTER(_I32)]),
    "ishara_op_gemm_nt": (C.c_int, [C.POINTER(GemmNtCall), _P]),
    "ishara_debug_gemm_nt_route": (C.c_int, [C.POINTER(GemmNtCall), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]),
    "ishara_op_gemm_as": (C.c_int, [C.POINTER(GemmNtCall), C.POINTER(GemmAsExt), _P]),
    "ishara_debug_gemm_as_plan": (C.c_int, [C.POINTER(GemmNtCall), C.POINTER(GemmAsExt), C.POINTER(GemmAsPlan)]),
    "ishara_op_qkv_scratch_bytes": (_I64, [_I32, _I32, _I32, _I32]),
    "ishara_op_qkv_fwd": (C.c_int, [_I32, _P, _P, _P, _F, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "ishara_op_classifier_fwd": (C.c_int, [_I32, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _P]),
    "ishara_op_log_softmax_fwd": (C.c_int, [_P, _P, _I32, _I32, _I32, _P]),
    "ishara_op_log_softmax_bwd": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _P]),
    "ishara_op_layernorm_fwd": (C.c_int, [_I32, _P, _P, _P, _F, _P, _P, _P, _I32, _I32, _P]),
    "ishara_op_layernorm_bwd": (C.c_int, [_I32, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _P]),
    "ishara_op_dwconv_fwd": (C.c_int, [_I32, _I32, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P]),
    "ishara_op_dwconv_scratch_bytes": (_I64, [_I32, _I32]),
    "ishara_op_dwconv_fwd_scratch_bytes": (_I64, [_I32, _I32, _I32]),
    "ishara_op_dwconv_fwd_ex": (C.c_int, [_I32, _I32, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P]),
    "ishara_op_dwconv_bwd": (C.c_int, [_I32, _I32, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P]),
    "ishara_op_bn_bwd_apply": (C.c_int, [_I32, _P, _P, _P, _P, _P, _P, _P, _I32, _P, _P, _I32, _I32, _I32, _P]),
    "ishara_op_dwconv_bwd_bn": (C.c_int, [_I32, _I32, _P, _P, _P, _P, _P, _P, _P, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P]),
    "ishara_op_attn_scratch_bytes": (_I64, [_I32, _I32, _I32, _I32]),
    "ishara_op_attn_scratch_layout_bytes": (C.c_int, [_I32, _I32, _I32, _I32, C.POINTER(_I64)]),
    "ishara_op_attn_fwd": (C.c_int, [_I32, _P, _P, _I32, _I32, _I32, _I32, _F, _U32, _U32, _F, _I32, _P, _P]),
    "ishara_op_attn_bwd": (C.c_int, [_I32, _P, _P, _P, _I32, _I32, _I32, _I32, _F, _U32, _U32, _F, _I32, _P, _P]),
    "ishara_op_relattn_scratch_bytes": (_I64, [_I32, _I32, _I32, _I32]),
    "ishara_op_relattn_fwd": (C.c_int, [_I32] + [_P] * 9 + [_I32, _I32, _I32, _I32, _U32, _U32, _F, _P, _P]),
    "ishara_op_relattn_bwd": (C.c_int, [_I32] + [_P] * 14 + [_I32, _I32, _I32, _I32, _U32, _U32, _F, _P, _P]),
    "ishara_relattn_len_scratch_bytes": (_I64, [_I32, _I32, _I32, _I32]),
    "ishara_relattn_len_fwd": (C.c_int, [_I32] + [_P] * 9 + [_I32, _I32, _I32, _I32, _U32, _U32, _F, _P, _I32, _P, _P]),
    "ishara_relattn_len_bwd": (C.c_int, [_I32] + [_P] * 14 + [_I32, _I32, _I32, _I32, _U32, _U32, _F, _P, _I32, _P, _P]),
    "ishara_debug_relattn_kernel_name": (C.c_char_p, [_I32, _I32, _I32, _I32, _I32]),
    "ishara_op_r4_subsample_scratch_bytes": (_I64, [_I32, _I32, _I32, _I32]),
    "ishara_op_r4_subsample_fwd": (C.c_int, [_I32] + [_P] * 6 + [_I32, _I32, _I32, _I32, _P, _P]),
    "ishara_op_r4_subsample_bwd": (C.c_int, [_I32] + [_P] * 10 + [_I32, _I32, _I32, _I32, _P, _P]),
    "ishara_op_r4_time_reduce_scratch_bytes": (_I64, [_I32, _I32, _I32]),
    "ishara_op_r4_time_reduce_fwd": (C.c_int, [_I32] + [_P] * 7 + [_I32, _I32, _I32, _P, _P]),
    "ishara_op_r4_time_reduce_bwd": (C.c_int, [_I32] + [_P] * 9 + [_I32, _I32, _I32, _P, _P]),
    "ishara_op_r4_rows": (C.c_int, [_I32, _I32, _P, _P, _P, _I32, _I32, _I32, _I32, _P]),
}

_lib = None


def load():
    """Load libishara_hip.so (built by ishara_amd/build.py or `make -C ishara_amd/csrc`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IsharaError(f"{LIB_PATH} is missing: build it with `python -m ishara_amd.build` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().ishara_last_error()
        raise IsharaError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")


def ptr(t):
    """Device/host pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    """The current torch stream of the current device, as the library's ishara_stream."""
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def aligned(nbytes: int, device):
    """`nbytes` of device memory at a 256-byte aligned address: (the tensor that owns it, the aligned pointer)."""
    import torch
    t = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device)
    return t, C.c_void_p(t.data_ptr() + (-t.data_ptr()) % 256)
