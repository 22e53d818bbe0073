"""ctypes binding of libtennis_hip.so (include/tennis_hip.h).

The HIP library is the product: there is no CPU fallback.  Importing this
module without the built library, or calling into it without a GPU, raises.
`import torch` happens first so that the library binds to the HIP runtime torch
already loaded (same SONAME libamdhip64.so.7) and device pointers / streams are
interchangeable with torch tensors.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch  # noqa: F401  (must precede CDLL: shares the HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TENNIS_HIP_LIB") or os.path.join(_HERE, "lib", "libtennis_hip.so")   # env: A/B builds while tuning

LAYOUT_NCHW_F32, LAYOUT_NHWC_F16, LAYOUT_NHWC_U8 = 0, 1, 2
ENC_EXACT_WEIGHTS = 1
ENC_FP32 = 4
ENC_FP32X3 = 8
RNN_GRU, RNN_LSTM = 0, 1
POOL_MAX, POOL_MEAN = 0, 1
MATMUL_MODES = {"f32": 0, "fp32x3": 1}      # TN_MATMUL_F32 / TN_MATMUL_FP32X3: the matrix pipe of the backbone training steps


def matmul_mode(name) -> int:
    """The TN_MATMUL_* value of a ``matmul=`` / ``--matmul`` name; touches neither the library nor a device."""
    if name not in MATMUL_MODES:
        raise ValueError(f"matmul must be 'f32' or 'fp32x3', got {name!r}")
    return MATMUL_MODES[name]


class TnParam(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data_host", C.POINTER(C.c_float)), ("numel", C.c_int64)]


class TnKernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("launches", C.c_int), ("ms", C.c_double),
                ("flops", C.c_double), ("bytes", C.c_double)]


class TnParamRow(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("where", C.c_int), ("offset", C.c_int64), ("count", C.c_int64)]


TRAINER_HEAD, TRAINER_GNMT, TRAINER_BACKBONE = 0, 1, 2      # tn_dbg_trainer_params: which handle's table
PARAM_FLAT, PARAM_STATE, PARAM_PTR = 0, 1, 2                # tn_param_row.where

_P = C.c_void_p
_SIGS = {
    "tn_version": (C.c_int, []),
    "tn_last_error": (C.c_char_p, []),
    "tn_ctx_create": (C.c_int, [C.c_int, _P, C.c_int, C.POINTER(_P)]),
    "tn_ctx_stream": (_P, [_P]),
    "tn_ctx_sync": (C.c_int, [_P]),
    "tn_ctx_destroy": (C.c_int, [_P]),
    "tn_densenet121_create": (C.c_int, [_P, C.POINTER(TnParam), C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int,
                                        C.POINTER(_P)]),
    "tn_densenet121_create_ex": (C.c_int, [_P, C.POINTER(TnParam), C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.POINTER(_P)]),
    "tn_densenet121_feature_dim": (C.c_int, [_P]),
    "tn_densenet121_workspace_bytes": (C.c_size_t, [_P]),
    "tn_densenet121_forward": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "tn_densenet121_forward_class_maps": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P]),
    "tn_densenet121_class_map_dims": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "tn_dbg_profile_class_maps": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, C.POINTER(TnKernelStat), C.c_int, C.POINTER(C.c_int)]),
    "tn_dbg_class_maps": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P,
                                    C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "tn_densenet121_set_pipelined": (C.c_int, [_P, C.c_int]),
    "tn_densenet121_join": (C.c_int, [_P, C.c_int]),
    "tn_densenet121_profile": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.POINTER(TnKernelStat), C.c_int,
                                         C.POINTER(C.c_int)]),
    "tn_densenet121_read_tap": (C.c_int, [_P, C.c_char_p, C.c_int, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "tn_densenet121_destroy": (C.c_int, [_P]),
    "tn_dense_create": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.POINTER(_P)]),
    "tn_dense_forward": (C.c_int, [_P, _P, C.c_int, _P]),
    "tn_dense_step_maps": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P]),
    "tn_dense_destroy": (C.c_int, [_P]),
    "tn_birnn_create": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(TnParam), C.c_int, C.c_char_p, C.c_int,
                                  C.c_int, C.POINTER(_P)]),
    "tn_birnn_forward": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P]),
    "tn_birnn_destroy": (C.c_int, [_P]),
    "tn_preproc_create": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "tn_preproc_forward": (C.c_int, [_P, _P, C.c_int, _P]),
    "tn_preproc_destroy": (C.c_int, [_P]),
    "tn_augment_forward": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P]),
    "tn_to_tensor_normalize": (C.c_int, [_P, _P, C.c_long, C.POINTER(C.c_float), C.POINTER(C.c_float), _P]),
    "tn_jpeg_create": (C.c_int, [_P, C.POINTER(_P)]),
    "tn_jpeg_info": (C.c_int, [_P, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                               C.POINTER(C.c_int)]),
    "tn_jpeg_decode": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_size_t), C.c_int, _P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "tn_jpeg_sync_passes": (C.c_int, [_P]),
    "tn_jpeg_destroy": (C.c_int, [_P]),
    "tn_temporal_pool": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "tn_window_head_create": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(TnParam), C.c_int, C.c_char_p, C.c_char_p,
                                        C.c_int, C.c_int, C.POINTER(_P)]),
    "tn_window_head_project": (C.c_int, [_P, _P, C.c_int]),
    "tn_window_head_forward": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "tn_window_head_forward_rows": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "tn_window_head_forward_tam": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "tn_window_head_forward_rows_tam": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P]),
    "tn_window_head_destroy": (C.c_int, [_P]),
    "tn_temporal_pool_arg": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "tn_temporal_pool_windows_arg": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "tn_temporal_pool_rows_arg": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, _P]),
    "tn_temporal_pool_windows": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "tn_temporal_pool_rows": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P]),
    "tn_dbg_window_head_rows_per_group": (C.c_int, [_P, C.c_int]),
    "tn_prf1_update": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P]),
    "tn_event_decoder_create": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(_P)]),
    "tn_event_decoder_run": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "tn_event_decoder_run_switch": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, C.c_int, C.c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "tn_event_decoder_run_transitions": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "tn_event_decoder_run_posteriors": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "tn_event_decoder_destroy": (C.c_int, [_P]),
    "tn_dbg_event_decoder_transition_geometry": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "tn_dbg_event_decoder_geometry": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "tn_dbg_event_decoder_switch_geometry": (C.c_int, [C.POINTER(C.c_int)]),
    "tn_dbg_event_decoder_workspace_bytes": (C.c_int, [_P, C.POINTER(C.c_size_t)]),
    "tn_head_create": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(TnParam), C.c_int, C.c_char_p, C.c_char_p, C.c_int,
                                 C.c_int, C.POINTER(_P)]),
    "tn_head_forward_backward": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P]),
    "tn_head_set_features": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "tn_head_forward_backward_rows": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P]),
    "tn_head_forward_rows": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "tn_head_buffers": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int64)]),
    "tn_head_sgd_step": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_float]),
    "tn_head_read_param": (C.c_int, [_P, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_int64)]),
    "tn_head_destroy": (C.c_int, [_P]),
    "tn_finetune_create": (C.c_int, [_P, C.POINTER(TnParam), C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(_P)]),
    "tn_finetune_forward_backward": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "tn_finetune_buffers": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int64)]),
    "tn_finetune_sgd_step": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_float]),
    "tn_finetune_read_param": (C.c_int, [_P, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_int64)]),
    "tn_finetune_destroy": (C.c_int, [_P]),
    "tn_finetune_set_matmul": (C.c_int, [_P, C.c_int]),
    "tn_finetune_matmul_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tn_cnnrnn_trainer_set_matmul": (C.c_int, [_P, C.c_int]),
    "tn_cnnrnn_trainer_matmul_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tn_gnmt_frames_trainer_set_matmul": (C.c_int, [_P, C.c_int]),
    "tn_gnmt_frames_trainer_matmul_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tn_cnnrnn_trainer_create": (C.c_int, [_P, C.c_int, C.POINTER(TnParam), C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "tn_cnnrnn_trainer_forward_backward": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "tn_cnnrnn_trainer_buffers": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int64), C.POINTER(_P), C.POINTER(_P),
                                            C.POINTER(C.c_int64)]),
    "tn_cnnrnn_trainer_sgd_step": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_float]),
    "tn_cnnrnn_trainer_read_param": (C.c_int, [_P, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_int64)]),
    "tn_cnnrnn_trainer_destroy": (C.c_int, [_P]),
    "tn_gnmt_frames_trainer_create": (C.c_int, [_P, C.POINTER(TnParam), C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.POINTER(_P)]),
    "tn_gnmt_frames_trainer_forward_backward": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "tn_gnmt_frames_trainer_buffers": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int64), C.POINTER(_P), C.POINTER(_P),
                                                 C.POINTER(C.c_int64)]),
    "tn_gnmt_frames_trainer_set_dropout": (C.c_int, [_P, C.c_float, C.c_uint64]),
    "tn_gnmt_frames_trainer_adam_step": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_float]),
    "tn_gnmt_frames_trainer_read_param": (C.c_int, [_P, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_int64)]),
    "tn_gnmt_frames_trainer_destroy": (C.c_int, [_P]),
    "tn_head_set_clip": (C.c_int, [_P, C.c_float]),
    "tn_head_clip_stats": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int64)]),
    "tn_finetune_set_clip": (C.c_int, [_P, C.c_float]),
    "tn_finetune_clip_stats": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int64)]),
    "tn_cnnrnn_trainer_set_clip": (C.c_int, [_P, C.c_float]),
    "tn_cnnrnn_trainer_clip_stats": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int64)]),
    "tn_gnmt_trainer_set_clip": (C.c_int, [_P, C.c_float]),
    "tn_gnmt_trainer_clip_stats": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int64)]),
    "tn_gnmt_frames_trainer_set_clip": (C.c_int, [_P, C.c_float]),
    "tn_gnmt_frames_trainer_clip_stats": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int64)]),
    "tn_dbg_grad_sumsq": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, C.POINTER(C.c_double)]),
    "tn_dbg_rows_pad_skip": (C.c_int, [C.c_int]),
    "tn_dbg_gnmt_trainer_src_grad": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_int]),
    "tn_dbg_gnmt_attention_fwd": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            _P, _P, _P, C.c_int, _P, _P]),
    "tn_dbg_gnmt_attention_bwd": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "tn_dbg_gnmt_attention_outer": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "tn_dbg_gnmt_ce": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "tn_dbg_gnmt_emb_grad": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "tn_dbg_gnmt_beam_step": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P, _P] + [C.c_int] * 6 + [C.c_float, C.c_float, C.c_int, C.c_int]
                              + [_P] * 11 + [C.c_int] + [_P] * 7),
    "tn_dbg_linear_lat": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_int, _P, _P] + [C.c_int] * 6 + [C.POINTER(C.c_int)]),
    "tn_gnmt_trainer_create": (C.c_int, [_P, C.POINTER(TnParam), C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "tn_gnmt_trainer_create_ex": (C.c_int, [_P, C.POINTER(TnParam), C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "tn_gnmt_trainer_dropout_mask": (C.c_int, [_P, C.c_int, C.POINTER(_P)]),
    "tn_gnmt_trainer_forward_backward": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "tn_gnmt_trainer_forward_backward_rows": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "tn_gnmt_trainer_buffers": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int64)]),
    "tn_gnmt_trainer_set_dropout": (C.c_int, [_P, C.c_float, C.c_uint64]),
    "tn_gnmt_trainer_dropout_masks": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)]),
    "tn_gnmt_trainer_adam_step": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_float]),
    "tn_gnmt_trainer_read_param": (C.c_int, [_P, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_int64)]),
    "tn_gnmt_trainer_destroy": (C.c_int, [_P]),
    "tn_gnmt_create": (C.c_int, [_P, C.POINTER(TnParam), C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "tn_gnmt_create_ex": (C.c_int, [_P, C.POINTER(TnParam), C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "tn_gnmt_encode": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P]),
    "tn_gnmt_encode_rows": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, _P]),
    "tn_gnmt_beam_search": (C.c_int, [_P, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, _P, _P, _P,
                                      C.POINTER(C.c_int)]),
    "tn_gnmt_decode_seq": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "tn_gnmt_decode_seq_attention": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "tn_gnmt_beam_search_attention": (C.c_int, [_P, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, _P, _P, _P,
                                                C.POINTER(C.c_int), _P]),
    "tn_masked_softmax_ce": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P]),
    "tn_gnmt_destroy": (C.c_int, [_P]),
    "tn_dbg_conv1x1": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int,
                                 C.c_int, C.c_int, C.c_int]),
    "tn_dbg_conv3x3": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tn_dbg_pack_conv3x3": (C.c_int, [_P, _P]),
    "tn_dbg_conv1x1_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_int, C.c_int]),
    "tn_dbg_conv3x3_dev": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tn_dbg_conv1x1_ex": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, _P]),
    "tn_dbg_conv1x1_head": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P, C.c_int]),
    "tn_dbg_pack_trans_frags": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "tn_dbg_pack_trans_frags_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "tn_dbg_dense_layer_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int,
                                         _P, C.c_int]),
    "tn_dbg_dense_chain_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tn_dbg_linear": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int]),
    "tn_dbg_channel_mean": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, C.c_int64, _P, C.c_size_t, _P, C.c_int]),
    "tn_dbg_stem": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int]),
    "tn_dbg_maxpool": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int]),
    "tn_dbg_head": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_int]),
    "tn_dbg_conv_fp32x3": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int, _P, _P, _P, C.c_int,
                                     C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tn_dbg_maxpool_fp32": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int]),
    "tn_dbg_gemm_tn": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64]),
    "tn_dbg_gemm_nn": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tn_dbg_rnn_wide_route": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tn_dbg_rnn_force_wide": (C.c_int, [C.c_int]),
    "tn_dbg_rnn_wide_launches": (C.c_int, [C.POINTER(C.c_int64)]),
    "tn_dbg_rnn_route": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "tn_dbg_encoder_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(TnKernelStat), C.c_int, C.POINTER(C.c_int)]),
    "tn_dbg_encoder_plan_shared": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(TnKernelStat), C.c_int, C.POINTER(C.c_int),
                                             C.POINTER(C.c_int)]),
    "tn_dbg_trainer_params": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.c_int, C.c_char_p, C.c_char_p, C.POINTER(TnParamRow), C.c_int,
                                        C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tn_dbg_linear_bnrelu": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tn_dbg_linear_fp32x3": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tn_dbg_gemm_tn_fp32x3": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64]),
    "tn_dbg_bn_train": (C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int]),
    "tn_dbg_ft_im2col7": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "tn_dbg_ft_im2col3": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "tn_dbg_ft_col2im3": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "tn_dbg_ft_maxpool": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P]),
    "tn_dbg_ft_avgpool2": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P]),
    "tn_dbg_ft_gap": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "tn_dbg_ft_bn_fold": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, _P, _P]),
    "tn_dbg_ft_bn_running": (C.c_int, [_P, _P, _P, _P, _P, C.c_int]),
    "tn_dbg_pool_max_arg": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "tn_dbg_softmax_ce": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P, _P]),
    "tn_dbg_dense_bwd": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "tn_dbg_colsum": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "tn_dbg_sgd_momentum": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, _P]),
    "tn_dbg_adam": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int64, _P]),
    "tn_dbg_stage_frames": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int64, _P]),
    "tn_dbg_transpose": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "tn_comm_unique_id": (C.c_int, [_P]),
    "tn_comm_create": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, C.POINTER(_P)]),
    "tn_comm_rank": (C.c_int, [_P]),
    "tn_comm_world": (C.c_int, [_P]),
    "tn_comm_device": (C.c_int, [_P]),
    "tn_comm_uses_rccl": (C.c_int, [_P]),
    "tn_allgather_features": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "tn_allreduce_f32": (C.c_int, [_P, _P, C.c_size_t, C.c_int]),
    "tn_allreduce_i64": (C.c_int, [_P, _P, C.c_size_t]),
    "tn_comm_destroy": (C.c_int, [_P]),
    "tn_dbg_pack_strip": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P]),
    "tn_dbg_dense_strip_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "tn_dbg_dense_strip_pair_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "tn_dbg_dense_strip_pair_chain_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int]),
    "tn_dbg_strip_pair_launches": (C.c_int, [C.POINTER(C.c_int64)]),
    "tn_dbg_head_fused_launches": (C.c_int, [C.POINTER(C.c_int64)]),
    "tn_dbg_head_fused": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "tn_densenet121_input_means": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "tn_npy_writer_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "tn_npy_writer_submit": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_int]),
    "tn_npy_writer_drain": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tn_npy_writer_destroy": (C.c_int, [_P]),
    "tn_bn_relu_clamp_fold": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, _P, _P, _P]),
    "tn_fp32x3_split": (C.c_int, [_P, C.c_int64, _P, _P, _P]),
    "tn_round_fp16_calibrated": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_double, _P]),
    "tn_dbg_block7_create": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_void_p)]),
    "tn_dbg_block7_run": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "tn_dbg_block7_run_ts": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "tn_dbg_block7_run_head": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, _P]),
    "tn_dbg_block7_destroy": (None, [_P]),
    "tn_dbg_block14_create": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_void_p)]),
    "tn_dbg_block14_run": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "tn_dbg_block14_run_ts": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "tn_dbg_block14_destroy": (None, [_P]),
    "tn_dbg_block28_create": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_void_p)]),
    "tn_dbg_block28_run": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "tn_dbg_block28_run_ts": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "tn_dbg_block28_destroy": (None, [_P]),
}

_lib = None


def declared_symbols():
    return sorted(_SIGS)


def load():
    """Load libtennis_hip.so; raise loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `make` (or __graft_entry__.build()). "
                "tennis_amd has no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().tn_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"libtennis_hip {what} failed ({rc}): {msg}")


def trainer_params(which: int, dims, prefix_a: str, prefix_b: str | None = None):
    """``tn_dbg_trainer_params``: ([(name, where, offset, count), ...], flat numel, state numel) of a training handle's parameter
    table; touches no device."""
    lib = load()
    d = (C.c_int * len(dims))(*[int(v) for v in dims])
    b = None if prefix_b is None else prefix_b.encode()
    n, numel, ns = C.c_int(), C.c_int64(), C.c_int64()
    check(lib.tn_dbg_trainer_params(which, d, len(dims), prefix_a.encode(), b, None, 0, C.byref(n), None, None), "tn_dbg_trainer_params")
    rows = (TnParamRow * n.value)()
    check(lib.tn_dbg_trainer_params(which, d, len(dims), prefix_a.encode(), b, rows, n.value, C.byref(n), C.byref(numel), C.byref(ns)),
          "tn_dbg_trainer_params")
    return [(r.name.decode(), r.where, r.offset, r.count) for r in rows], numel.value, ns.value


def make_params(params: dict):
    """dict[str, np.ndarray fp32] -> (TnParam array, keepalive list)."""
    keep = []
    arr = (TnParam * len(params))()
    for i, (k, v) in enumerate(params.items()):
        a = np.ascontiguousarray(v, dtype=np.float32)
        name = k.encode()
        keep += [a, name]
        arr[i].name = name
        arr[i].data_host = a.ctypes.data_as(C.POINTER(C.c_float))
        arr[i].numel = a.size
    return arr, keep


class Context:
    """One tn_ctx bound to a torch device and (by default) torch's current stream."""

    def __init__(self, device: int | None = None, stream=None):
        if not torch.cuda.is_available():
            raise RuntimeError("tennis_amd needs a ROCm GPU: torch.cuda.is_available() is False and there is no "
                               "CPU fallback")
        self.lib = load()
        device = default_device() if device is None else int(device)
        self.device = device
        # the process's current device is left alone: the library switches to `device` for the duration of each
        # call (TnDeviceGuard) and torch tensors carry their own device
        if stream is None:
            stream = torch.cuda.current_stream(device)
        self.torch_stream = stream
        h = _P()
        check(self.lib.tn_ctx_create(device, _P(stream.cuda_stream), 0, C.byref(h)), "tn_ctx_create")
        self.handle = h

    def sync(self):
        check(self.lib.tn_ctx_sync(self.handle), "tn_ctx_sync")

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.tn_ctx_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


_default_ctx = {}


def default_device() -> int:
    """The GPU of this process: torch's current device — one process per GPU, so under torchrun that is
    LOCAL_RANK once the launcher (or init_distributed) has called torch.cuda.set_device — else LOCAL_RANK, else 0."""
    if torch.cuda.is_available():
        cur = torch.cuda.current_device()
        if cur != 0 or "LOCAL_RANK" not in os.environ:
            return cur
        lr = int(os.environ["LOCAL_RANK"])
        return lr if lr < torch.cuda.device_count() else cur
    return 0


def default_context(device: int | None = None) -> Context:
    device = default_device() if device is None else int(device)
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


def ptr(t) -> _P:
    return _P(t.data_ptr()) if t is not None else _P(None)
