"""ctypes binding of libfoley_hip.so (include/foley_hip.h).  PyTorch is only the allocator /
stream provider here: every call passes raw device pointers + the current HIP stream.

There is deliberately NO fallback: if the shared library is missing or a call fails, a
`FoleyRuntimeError` is raised - the HIP path is the only implementation of the hot path.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libfoley_hip.so")

DT_F32, DT_BF16, DT_I32, DT_F8E4M3, DT_F8E5M2, DT_F16 = 0, 1, 2, 3, 4, 5
_TORCH2DT = {torch.float32: DT_F32, torch.bfloat16: DT_BF16, torch.int32: DT_I32, torch.float8_e4m3fn: DT_F8E4M3,
             torch.float8_e5m2: DT_F8E5M2, torch.float16: DT_F16}

_DT2TORCH = {v: k for k, v in _TORCH2DT.items()}
SLOT_NAME_MAX = 64      # FOLEY_SLOT_NAME_MAX

EPI_STORE_F32, EPI_STORE_T, EPI_SILU_T, EPI_GELU_T, EPI_SILUGATE_T, EPI_GATE_RES, EPI_DAC = range(7)


class FoleyRuntimeError(RuntimeError):
    pass


class FoleyConfigC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "depth_triple", "depth_single", "hidden", "heads", "mlp_hidden", "conv_hidden", "sync_hidden",
        "cond_dim", "clip_dim", "sync_dim", "latent_dim", "time_freq_dim", "compute_dtype", "dac_dim",
        "dac_n_rates")] + [("dac_rates", C.c_int32 * 8), ("dac_dilations", C.c_int32 * 3)]


class FoleyPlanC(C.Structure):
    _fields_ = [
        ("ncfg", C.c_int32), ("clips", C.c_int32), ("La", C.c_int32), ("Lv", C.c_int32), ("Ls", C.c_int32),
        ("Lt", C.c_int32), ("n_iter", C.c_int32), ("guidance", C.c_float),
        ("text", C.c_void_p), ("clip", C.c_void_p), ("sync", C.c_void_p), ("t_feat", C.c_void_p),
        ("rope_cos", C.c_void_p), ("rope_sin", C.c_void_p), ("rope_len", C.c_int32),
        ("pos_audio_self", C.c_void_p), ("pos_visual_self", C.c_void_p), ("pos_linear", C.c_void_p),
        ("sync_gather", C.c_void_p), ("solver_coef", C.c_void_p),
    ]


class CondSetsC(C.Structure):
    _fields_ = [("n_text", C.c_int32), ("n_vis", C.c_int32), ("text_of", C.POINTER(C.c_int32)), ("vis_of", C.POINTER(C.c_int32))]


class TextTimelineC(C.Structure):
    """foley_text_timeline: n_text sets and the HOST tables [ncfg*clips*(Lv+La)]."""
    _fields_ = [("n_text", C.c_int32), ("set_a", C.POINTER(C.c_int32)), ("set_b", C.POINTER(C.c_int32)), ("alpha", C.POINTER(C.c_float))]


class RowBcastC(C.Structure):
    _fields_ = [("p", C.c_void_p), ("ld", C.c_int64), ("mode", C.c_int32), ("rows_per_cfg", C.c_int32),
                ("L", C.c_int32), ("Ls", C.c_int32), ("period", C.c_int32), ("periodic_cfgs", C.c_int32)]


class QkvSplitDescC(C.Structure):
    _fields_ = [
        ("L", C.c_int32), ("H", C.c_int32), ("nK", C.c_int32),
        ("gain", C.c_void_p * 3), ("pos", C.c_void_p * 3), ("dst", C.c_void_p * 3),
        ("out_dtype", C.c_int32), ("vt_pitch", C.c_int32), ("S_tot", C.c_int32), ("tok_off", C.c_int32),
        ("eps", C.c_float), ("cos_tab", C.c_void_p), ("sin_tab", C.c_void_p),
        ("attn_k", C.c_void_p), ("attn_vt", C.c_void_p), ("attn_out", C.c_void_p),
        ("attn_skv", C.c_int32), ("attn_pitch", C.c_int32), ("attn_bdiv", C.c_int32),
        ("attn_fused", C.POINTER(C.c_int32)),
    ]


def _qkv_fused(self) -> bool:
    return bool(getattr(self, "_flag", C.c_int32(0)).value)


QkvSplitDescC.fused = _qkv_fused


class GemmDescC(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("lda", C.c_int64),
        ("segV", C.c_int32), ("segS", C.c_int32), ("taps", C.c_int32), ("tapC", C.c_int32),
        ("dil", C.c_int32), ("tap0", C.c_int32),
        ("out0", C.c_void_p), ("out1", C.c_void_p),
        ("osegV", C.c_int32), ("out_seg", C.c_int64), ("out_row", C.c_int64), ("out_shift", C.c_int64),
        ("out_check", C.c_int32),
        ("rb", RowBcastC), ("res", C.c_void_p), ("alpha", C.c_void_p), ("alphaC", C.c_int32),
        ("dtype", C.c_int32), ("epilogue", C.c_int32), ("tile", C.c_int32), ("ksplit", C.c_int32),
        ("partials", C.c_void_p), ("partial_slabs", C.c_int32), ("ksplit_used", C.POINTER(C.c_int32)),
        ("qkv", C.POINTER(QkvSplitDescC)), ("rstride", C.c_int32), ("ldw", C.c_int64), ("wfmt", C.c_int32),
        ("partial_dtype", C.c_int32), ("gelu_erf", C.c_int32),
    ]


class GuidanceDescC(C.Structure):
    """foley_guidance_desc: device pointers of the schedule table [n_iter, 2] and the per-clip factors [clips] (0: absent)."""
    _fields_ = [("sched", C.c_void_p), ("clip_scale", C.c_void_p)]


class ProjectionDescC(C.Structure):
    """foley_projection_desc: device pointers of the rows [n_iter, 4], the coefficients [clips, 2] and APG's plane [clips*L, C]
    (0: absent), and the mode (FOLEY_GUIDANCE_APG 1, FOLEY_GUIDANCE_ZERO_STAR 2)."""
    _fields_ = [("rows", C.c_void_p), ("coef", C.c_void_p), ("plane", C.c_void_p), ("mode", C.c_int32)]


class StepDescC(C.Structure):
    """foley_step_desc: every operand of foley_op_solver_step - the core ones, then the optional guidance descriptor, velocity
    ring [hist_slots, clips, C, L], x0 / noise / mask of the edit form and starts / weights of the windows form (0: absent)."""
    _fields_ = [("pred", C.c_void_p), ("x", C.c_void_p), ("x_saved", C.c_void_p), ("d_acc", C.c_void_p),
                ("clips", C.c_int32), ("C", C.c_int32), ("L", C.c_int32), ("ncfg", C.c_int32),
                ("guidance", C.c_float), ("rows_dtype", C.c_int32), ("coef", C.c_void_p), ("step_ptr", C.c_void_p), ("rows_out", C.c_void_p),
                ("gd", GuidanceDescC), ("hist", C.c_void_p), ("hist_slots", C.c_int32), ("x0_clips", C.c_int32),
                ("x0", C.c_void_p), ("noise", C.c_void_p), ("mask", C.c_void_p), ("mask_clips", C.c_int32),
                ("n_win", C.c_int32), ("starts", C.c_void_p), ("weights", C.c_void_p), ("Ltot", C.c_int32)]


class FlowEditDescC(C.Structure):
    """foley_flowedit_desc: every operand of foley_op_flowedit_step / foley_op_flowedit_stage (0: absent)."""
    _fields_ = [("pred", C.c_void_p), ("z", C.c_void_p), ("x_src", C.c_void_p), ("noise", C.c_void_p), ("mask", C.c_void_p),
                ("coef", C.c_void_p), ("step_ptr", C.c_void_p), ("rows_out", C.c_void_p),
                ("V", C.c_int32), ("C", C.c_int32), ("L", C.c_int32), ("n_iter", C.c_int32), ("rows_dtype", C.c_int32),
                ("src_clips", C.c_int32), ("noise_rows", C.c_int32), ("mask_clips", C.c_int32),
                ("g_src", C.c_float), ("g_tar", C.c_float)]


class LoraPairC(C.Structure):
    _fields_ = [("down", C.c_void_p), ("up", C.c_void_p), ("dtype", C.c_int32), ("rank", C.c_int32),
                ("down_ndim", C.c_int32), ("up_ndim", C.c_int32), ("down_shape", C.c_int64 * 3), ("up_shape", C.c_int64 * 3),
                ("scale", C.c_float)]


class ProfEntryC(C.Structure):
    _fields_ = [("label", C.c_char * 80), ("calls", C.c_int32), ("total_ms", C.c_float), ("flop", C.c_double),
                ("bytes", C.c_double), ("kernel", C.c_char * 200)]


PROGRESS_CB = C.CFUNCTYPE(None, C.c_int32, C.c_int32, C.c_void_p)
ABI_VERSION = 13

_SIGNATURES = {
    "foley_abi_version": (C.c_uint32, []),
    "foley_last_error": (C.c_char_p, []),
    "foley_ctx_create": (C.c_int, [C.c_int, C.POINTER(FoleyConfigC), C.POINTER(C.c_void_p)]),
    "foley_ctx_destroy": (None, [C.c_void_p]),
    "foley_set_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "foley_weights_begin": (C.c_int, [C.c_void_p, C.c_int]),
    "foley_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_void_p]),
    "foley_weights_end": (C.c_int, [C.c_void_p, C.c_void_p]),
    "foley_weights_arena": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "foley_weights_slot": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int),
                                     C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "foley_weights_mark_received": (C.c_int, [C.c_void_p]),
    "foley_bcast_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "foley_bcast_local": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "foley_lora_begin": (C.c_int, [C.c_void_p, C.c_void_p]),
    "foley_lora_merge": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(LoraPairC), C.c_void_p]),
    "foley_lora_end": (C.c_int, [C.c_void_p, C.c_void_p]),
    "foley_lora_clear": (C.c_int, [C.c_void_p, C.c_void_p]),
    "foley_lora_backup_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "foley_prepare": (C.c_int, [C.c_void_p, C.POINTER(FoleyPlanC), C.c_void_p]),
    "foley_prepare_sets": (C.c_int, [C.c_void_p, C.POINTER(FoleyPlanC), C.POINTER(CondSetsC), C.c_void_p]),
    "foley_prepare_timeline": (C.c_int, [C.c_void_p, C.POINTER(FoleyPlanC), C.POINTER(TextTimelineC), C.c_void_p]),
    "foley_dit_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "foley_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, PROGRESS_CB, C.c_void_p, C.c_void_p]),
    "foley_abort": (C.c_int, [C.c_void_p]),
    "foley_set_edit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "foley_set_windows": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]),
    "foley_set_flowedit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float,
                                     C.c_float, C.c_void_p]),
    "foley_set_guidance": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_float, C.c_void_p]),
    "foley_set_projected_guidance": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p]),
    "foley_set_step_cache": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_double, C.POINTER(C.c_double), C.c_int,
                                       C.POINTER(C.c_int32), C.c_int, C.c_void_p]),
    "foley_step_cache_report": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int]),
    "foley_set_multistep": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "foley_dac_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "foley_dac_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int,
                                   C.c_void_p, C.c_void_p]),
    "foley_last_elapsed_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "foley_profile_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(ProfEntryC), C.c_int,
                                        C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_void_p]),
    "foley_op_gemm": (C.c_int, [C.POINTER(GemmDescC), C.c_void_p]),
    "foley_op_attention": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 7 + [C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                                        C.c_void_p]),
    "foley_op_attention_hd": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 7 + [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                                           C.c_void_p]),
    "foley_op_attention_timeline": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 7 + [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p]),
    "foley_op_ln_mod_pending": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.POINTER(RowBcastC),
                                          C.POINTER(RowBcastC), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                          C.POINTER(RowBcastC), C.c_void_p]),
    "foley_op_ln_mod_pending2": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.POINTER(RowBcastC),
                                           C.POINTER(RowBcastC), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                           C.POINTER(RowBcastC), C.c_void_p]),
    "foley_op_ln_mod": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.POINTER(RowBcastC),
                                  C.POINTER(RowBcastC), C.c_void_p, C.c_int, C.c_void_p]),
    "foley_op_attention_scatter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "foley_op_qkv_regroup": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "foley_op_resize_aa_u8": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.c_long, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_int, C.c_void_p, C.c_void_p]),
    "foley_op_resample_sinc": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                         C.c_int, C.c_void_p]),
    "foley_op_logmel": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                  C.c_int, C.c_void_p, C.c_void_p]),
    "foley_op_qkv_split": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "foley_op_solver_step": (C.c_int, [C.POINTER(StepDescC), C.c_void_p]),
    "foley_op_windows_stitch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "foley_op_guidance_stats_work": (C.c_int64, [C.c_int, C.c_int]),
    "foley_op_guidance_stats": (C.c_int, [C.POINTER(GuidanceDescC), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                          C.c_void_p, C.c_float, C.c_void_p, C.c_int64, C.c_void_p]),
    "foley_op_guidance_project_work": (C.c_int64, [C.c_int, C.c_int]),
    "foley_op_guidance_project": (C.c_int, [C.POINTER(ProjectionDescC), C.POINTER(GuidanceDescC), C.c_void_p, C.c_int, C.c_int, C.c_int,
                                            C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "foley_op_solver_step_projected": (C.c_int, [C.POINTER(StepDescC), C.POINTER(ProjectionDescC), C.c_void_p]),
    "foley_op_flowedit_step": (C.c_int, [C.POINTER(FlowEditDescC), C.c_void_p]),
    "foley_op_flowedit_stage": (C.c_int, [C.POINTER(FlowEditDescC), C.c_float, C.c_int, C.c_void_p]),
    "foley_op_cache_probe_work": (C.c_int64, [C.c_int, C.c_int]),
    "foley_op_cache_probe": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(RowBcastC), C.POINTER(RowBcastC),
                                       C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "foley_op_cache_delta": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "foley_op_cache_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "foley_op_flow_mix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                    C.c_void_p]),
    "foley_op_latent_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                       C.c_void_p]),
    "foley_op_dac_out": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p]),
    "foley_op_rows_add_act": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "foley_op_add_periodic": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "foley_op_gather_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "foley_op_cast": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_void_p]),
    "foley_op_rows_periodic_check": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "foley_op_dac_in": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p] * 3),
    "foley_op_rows_to_planes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "foley_op_melspec_db": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "foley_op_spec_patches": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "foley_op_window_attention": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "foley_op_loudness_energy": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_double), C.c_void_p,
                                           C.c_int64, C.c_void_p, C.c_void_p]),
    "foley_op_loudness_gate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "foley_op_true_peak": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_float), C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "foley_op_loudness_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_double, C.c_int,
                                          C.POINTER(C.c_float), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_LIB: Optional[C.CDLL] = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen libfoley_hip.so and type its entry points; raises if it is not built."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or os.environ.get("FOLEY_HIP_LIB", LIB_PATH)
    if not os.path.exists(p):
        raise FoleyRuntimeError(
            f"{p} not found - build it with `python __graft_entry__.py build` (hipcc, gfx950). "
            "There is no CPU / PyTorch fallback for the Foley sampling path.")
    lib = C.CDLL(p)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)     # AttributeError if the .so does not export the ABI
        fn.restype = res
        fn.argtypes = args
    if lib.foley_abi_version() != ABI_VERSION:
        raise FoleyRuntimeError("libfoley_hip.so ABI version mismatch")
    if path is None:
        _LIB = lib
    return lib


def _check(lib, rc: int, what: str):
    if rc != 0:
        msg = lib.foley_last_error()
        raise FoleyRuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise FoleyRuntimeError("libfoley_hip.so needs device tensors (got a CPU tensor)")
    if not t.is_contiguous():
        raise FoleyRuntimeError("tensor must be contiguous")
    return t.data_ptr()


_HIP: Optional[C.CDLL] = None


def _hip() -> C.CDLL:
    """The HIP runtime the process has already loaded (device-to-device copies out of library-owned memory)."""
    global _HIP
    if _HIP is None:
        _HIP = C.cdll.LoadLibrary("libamdhip64.so")
        _HIP.hipMemcpy.restype = C.c_int
        _HIP.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return _HIP


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def dt_of(t: torch.Tensor) -> int:
    return _TORCH2DT[t.dtype]


def make_config(dit, dac, compute_dtype: torch.dtype) -> FoleyConfigC:
    c = FoleyConfigC()
    c.depth_triple, c.depth_single, c.hidden, c.heads = dit.depth_triple, dit.depth_single, dit.hidden, dit.heads
    c.mlp_hidden, c.conv_hidden, c.sync_hidden = dit.mlp_hidden, dit.conv_hidden, dit.sync_hidden
    c.cond_dim, c.clip_dim, c.sync_dim = dit.cond_dim, dit.clip_dim, dit.sync_dim
    c.latent_dim, c.time_freq_dim = dit.latent_dim, dit.time_freq_dim
    c.compute_dtype = _TORCH2DT[compute_dtype]
    c.dac_dim, c.dac_n_rates = dac.decoder_dim, len(dac.rates)
    for i, r in enumerate(dac.rates):
        c.dac_rates[i] = r
    for i, d in enumerate(dac.dilations):
        c.dac_dilations[i] = d
    return c


class FoleyContext:
    """Owns one `foley_ctx` on one GPU plus references to every tensor registered with it."""

    def __init__(self, dit_cfg, dac_cfg, compute_dtype: torch.dtype, device: torch.device):
        self.lib = load_library()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise FoleyRuntimeError("FoleyContext needs a HIP device (torch device type 'cuda')")
        self.dit_cfg, self.dac_cfg, self.compute_dtype = dit_cfg, dac_cfg, compute_dtype
        self._cfg = make_config(dit_cfg, dac_cfg, compute_dtype)
        h = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _check(self.lib, self.lib.foley_ctx_create(idx, C.byref(self._cfg), C.byref(h)), "foley_ctx_create")
        self._h = h
        self._keep: Dict[str, torch.Tensor] = {}
        self._plan_keep = None

    def close(self):
        if getattr(self, "_h", None):
            self.lib.foley_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights
    def set_tensor(self, name: str, t: torch.Tensor):
        shape = (C.c_int64 * t.dim())(*t.shape)
        _check(self.lib, self.lib.foley_set_tensor(self._h, name.encode(), _ptr(t), dt_of(t), t.dim(), shape),
               f"foley_set_tensor({name})")
        self._keep[name] = t

    def set_tensors(self, items):
        for k, t in items:
            self.set_tensor(k, t)

    # ---- reference-keyed loading (the library packs on the device; weights.hip)
    def load_reference_state(self, state_dicts, weight_format: int = 0) -> int:
        """Pack reference state dict(s) (DiT and/or DAC, device or CPU tensors) through the C ABI.  Returns the number of
        tensors the sampling path ignored (DAC encoder etc.)."""
        _check(self.lib, self.lib.foley_weights_begin(self._h, int(weight_format)), "foley_weights_begin")
        ignored = 0
        with torch.cuda.device(self.device):
            for sd in state_dicts:
                for k, v in sd.items():
                    if not isinstance(v, torch.Tensor) or not v.is_floating_point():
                        continue
                    t = v.detach().to(self.device).contiguous()
                    shape = (C.c_int64 * t.dim())(*t.shape)
                    rc = self.lib.foley_load_tensor(self._h, k.encode(), t.data_ptr(), dt_of(t), t.dim(), shape, _stream())
                    if rc == 1:
                        ignored += 1
                    else:
                        _check(self.lib, rc, f"foley_load_tensor({k})")
                    torch.cuda.current_stream().synchronize()       # `t` is only borrowed for the call
            _check(self.lib, self.lib.foley_weights_end(self._h, _stream()), "foley_weights_end")
        return ignored

    def weights_arena(self):
        p, n = C.c_void_p(), C.c_uint64()
        _check(self.lib, self.lib.foley_weights_arena(self._h, C.byref(p), C.byref(n)), "foley_weights_arena")
        return int(p.value), int(n.value)

    def weights_slot(self, which):
        """One slot of the ctx-owned arena, by enumeration index (int) or packed name (str): dict(name, ptr, dtype, shape,
        offset, bytes), or None past the last index / for an unknown name.  Read-only (foley_weights_slot)."""
        name_out = C.create_string_buffer(SLOT_NAME_MAX)
        p, dt, nd, shape, off, nb = C.c_void_p(), C.c_int(), C.c_int(), (C.c_int64 * 8)(), C.c_uint64(), C.c_uint64()
        by_name = isinstance(which, str)
        rc = self.lib.foley_weights_slot(self._h, -1 if by_name else int(which), which.encode() if by_name else None, name_out,
                                         C.byref(p), C.byref(dt), C.byref(nd), shape, C.byref(off), C.byref(nb))
        if rc == 1:
            return None
        _check(self.lib, rc, f"foley_weights_slot({which})")
        return {"name": name_out.value.decode(), "ptr": int(p.value), "dtype": _DT2TORCH[dt.value],
                "shape": tuple(shape[i] for i in range(nd.value)), "offset": int(off.value), "bytes": int(nb.value)}

    def weights_slots(self):
        """Every slot of the arena in the library's own order."""
        out, i = [], 0
        while True:
            s = self.weights_slot(i)
            if s is None:
                return out
            out.append(s)
            i += 1

    def weights_slot_tensor(self, which) -> torch.Tensor:
        """A copy of one packed tensor of the ctx-owned arena (device tensor of the slot's dtype and shape)."""
        s = self.weights_slot(which)
        if s is None:
            raise FoleyRuntimeError(f"no packed tensor {which!r} in the weight arena")
        out = torch.empty(s["shape"], dtype=s["dtype"], device=self.device)
        if s["bytes"] != out.numel() * out.element_size():
            raise FoleyRuntimeError(f"slot {s['name']}: {s['bytes']} bytes do not match {s['dtype']} {s['shape']}")
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().synchronize()
            rc = _hip().hipMemcpy(C.c_void_p(out.data_ptr()), C.c_void_p(s["ptr"]), C.c_size_t(s["bytes"]), 3)
        if rc != 0:
            raise FoleyRuntimeError(f"hipMemcpy of slot {s['name']} failed ({rc})")
        return out

    # ---- low-rank adapters merged into the registered weights (csrc/lora.hip; host/lora.py drives these)
    def lora_begin(self):
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.foley_lora_begin(self._h, _stream()), "foley_lora_begin")

    def lora_merge(self, ref_key: str, adapters):
        """All adapters of one reference key: [(down, up, scale), ...] device tensors of one dtype per pair (f32 / bf16 / f16),
        down [r, I(, k)], up [O, r(, 1)].  They are borrowed until lora_end returns - the caller keeps them alive."""
        pairs = (LoraPairC * max(len(adapters), 1))()
        for p, (down, up, scale) in zip(pairs, adapters):
            if down.dtype != up.dtype:
                raise FoleyRuntimeError(f"lora: '{ref_key}': down is {down.dtype}, up is {up.dtype}")
            if down.dim() > 3 or up.dim() > 3 or down.dim() < 1:
                raise FoleyRuntimeError(f"lora: '{ref_key}': shape does not match (down {tuple(down.shape)}, up {tuple(up.shape)})")
            p.down, p.up = _ptr(down), _ptr(up)
            p.dtype = _TORCH2DT.get(down.dtype, -1)
            p.rank = int(down.shape[0])
            p.down_ndim, p.up_ndim = down.dim(), up.dim()
            p.down_shape[:down.dim()] = list(down.shape)
            p.up_shape[:up.dim()] = list(up.shape)
            p.scale = float(scale)
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.foley_lora_merge(self._h, ref_key.encode(), len(adapters), pairs, _stream()),
                   f"foley_lora_merge({ref_key})")

    def lora_end(self):
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.foley_lora_end(self._h, _stream()), "foley_lora_end")

    def lora_clear(self):
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.foley_lora_clear(self._h, _stream()), "foley_lora_clear")

    def lora_backup_bytes(self) -> int:
        n = C.c_uint64()
        _check(self.lib, self.lib.foley_lora_backup_bytes(self._h, C.byref(n)), "foley_lora_backup_bytes")
        return int(n.value)

    def bcast_weights(self, nccl_comm: int, root: int = 0):
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.foley_bcast_weights(self._h, C.c_void_p(nccl_comm), int(root), _stream()),
                   "foley_bcast_weights")

    # ---- run
    def prepare(self, plan: dict):
        """plan: ncfg, clips, La, Lv, Ls, Lt, n_iter, guidance + device tensors (see foley_plan).  Per-clip conditioning
        (host/cond_sets.py): `text_of` / `vis_of` lists of ncfg*clips set indices -> foley_prepare_sets.  A prompt timeline
        (host/prompt_timeline.py): `timeline` = (set_a, set_b, alpha), flat host sequences of ncfg*clips*(Lv+La) entries, with
        plan["text"] holding the text sets -> foley_prepare_timeline."""
        p = FoleyPlanC()
        for k in ("ncfg", "clips", "La", "Lv", "Ls", "Lt", "n_iter", "rope_len"):
            setattr(p, k, int(plan[k]))
        p.guidance = float(plan["guidance"])
        for k in ("text", "clip", "sync", "t_feat", "rope_cos", "rope_sin", "pos_audio_self", "pos_visual_self",
                  "pos_linear", "sync_gather", "solver_coef"):
            setattr(p, k, _ptr(plan[k]))
        with torch.cuda.device(self.device):
            if plan.get("timeline") is not None:
                if plan.get("text_of") is not None:
                    raise FoleyRuntimeError("a prompt timeline does not combine with per-clip set maps")
                sa, sb, al = plan["timeline"]
                n = p.ncfg * p.clips * (p.Lv + p.La)
                if not (len(sa) == len(sb) == len(al) == n):
                    raise FoleyRuntimeError("timeline tables must have ncfg*clips*(Lv+La) entries")
                t = TextTimelineC(int(plan["text"].shape[0]), (C.c_int32 * n)(*sa), (C.c_int32 * n)(*sb), (C.c_float * n)(*al))
                _check(self.lib, self.lib.foley_prepare_timeline(self._h, C.byref(p), C.byref(t), _stream()), "foley_prepare_timeline")
            elif plan.get("text_of") is None:
                _check(self.lib, self.lib.foley_prepare(self._h, C.byref(p), _stream()), "foley_prepare")
            else:
                n = len(plan["text_of"])
                t_of, v_of = (C.c_int32 * n)(*plan["text_of"]), (C.c_int32 * n)(*plan["vis_of"])
                s = CondSetsC(int(plan["text"].shape[0]), int(plan["clip"].shape[0]), t_of, v_of)
                if n != p.ncfg * p.clips or len(plan["vis_of"]) != n:
                    raise FoleyRuntimeError("set maps must have ncfg*clips entries")
                _check(self.lib, self.lib.foley_prepare_sets(self._h, C.byref(p), C.byref(s), _stream()), "foley_prepare_sets")
        self._plan_keep = plan    # the ctx borrows the plan's tables until the next prepare
        self.plan = plan

    def dit_forward(self, latents: torch.Tensor, it: int) -> torch.Tensor:
        pl = self.plan
        out = torch.empty(pl["ncfg"] * pl["clips"] * pl["La"], self.dit_cfg.latent_dim, dtype=torch.float32,
                          device=self.device)
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.foley_dit_forward(self._h, _ptr(latents), int(it), _ptr(out), _stream()),
                   "foley_dit_forward")
        return out

    def sample(self, latents: torch.Tensor, use_graph: bool = False, progress=None) -> torch.Tensor:
        """In-place denoising of `latents` [clips, C, La] fp32.  An exception raised by `progress` (ComfyUI's interrupt:
        comfy.utils.ProgressBar.update raises inside the reference's loop, utils.py:247) stops the loop after the current
        iteration and propagates to the caller, like it does there."""
        raised = []

        def _cb(i, n, _u):
            try:
                progress(i, n)
            except BaseException as e:          # noqa: BLE001 - re-raised below, outside the C frame
                if not raised:
                    raised.append(e)
                self.lib.foley_abort(self._h)

        cb = PROGRESS_CB(_cb) if progress else PROGRESS_CB()
        with torch.cuda.device(self.device):
            rc = self.lib.foley_sample(self._h, _ptr(latents), int(use_graph), cb, None, _stream())
        if raised:
            raise raised[0]
        _check(self.lib, rc, "foley_sample")
        return latents

    def set_edit(self, x0: Optional[torch.Tensor], noise: Optional[torch.Tensor], mask: Optional[torch.Tensor] = None):
        """foley_set_edit after prepare(): x0 [1 | clips, C, La] and noise [clips, C, La] fp32, mask [La] or [1 | clips, La] fp32
        (None: all ones) - all on this context's device; the library copies them.  x0 = noise = None clears the edit state."""
        def _f32(t):
            if t is None:
                return None
            if t.dtype != torch.float32 or t.device != self.device:
                raise FoleyRuntimeError("set_edit: operands must be fp32 tensors on the context's device")
            return t.contiguous()
        x0, noise, mask = _f32(x0), _f32(noise), _f32(mask)
        x0_clips = x0.shape[0] if x0 is not None else 0
        mask_clips = (1 if mask.dim() == 1 else mask.shape[0]) if mask is not None else 0
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.foley_set_edit(self._h, _ptr(x0), x0_clips, _ptr(noise), _ptr(mask), mask_clips, _stream()),
                   "foley_set_edit")
        self._edit_keep = (x0, noise, mask)     # borrowed only until the copies on the stream are done

    def set_flowedit(self, x_src: Optional[torch.Tensor], noise: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                     g_src: float = 2.0, g_tar: float = 4.5, sigma0: float = 1.0):
        """foley_set_flowedit after prepare() of the 2V-clip pair plan: x_src [1 | V, C, La], noise [n_iter | 1, V, C, La], mask [La]
        or [1 | V, La] (None: all ones), fp32 on this context's device; the library copies them.  g_src / g_tar: the CFG scales of
        the source and target branches, sigma0: the sigma the first rows are staged at.  x_src None clears the state; sample()
        then takes and returns z [V, C, La]."""
        def _f32(t):
            if t is None:
                return None
            if t.dtype != torch.float32 or t.device != self.device:
                raise FoleyRuntimeError("set_flowedit: operands must be fp32 tensors on the context's device")
            return t.contiguous()
        x_src, noise, mask = _f32(x_src), _f32(noise), _f32(mask)
        if x_src is not None:
            if x_src.dim() != 3 or noise is None or noise.dim() != 4 or tuple(noise.shape[2:]) != tuple(x_src.shape[1:]):
                raise FoleyRuntimeError("set_flowedit: x_src is [1 | V, C, La] and noise [n_iter | 1, V, C, La]")
            pl = getattr(self, "plan", None)
            if pl is not None and (2 * noise.shape[1] != int(pl["clips"]) or x_src.shape[2] != int(pl["La"])
                                   or (mask is not None and mask.shape[-1] != int(pl["La"]))):
                raise FoleyRuntimeError("set_flowedit: the operands must match the plan (noise of V = clips / 2 variations, La frames)")
        src_clips = x_src.shape[0] if x_src is not None else 0
        noise_rows = noise.shape[0] if noise is not None else 0
        mask_clips = (1 if mask.dim() == 1 else mask.shape[0]) if mask is not None else 0
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.foley_set_flowedit(self._h, _ptr(x_src), src_clips, _ptr(noise), noise_rows, _ptr(mask), mask_clips,
                                                         float(g_src), float(g_tar), float(sigma0), _stream()), "foley_set_flowedit")
        self._flowedit_keep = (x_src, noise, mask)     # borrowed only until the copies on the stream are done

    def set_windows(self, starts, weights: Optional[torch.Tensor]):
        """foley_set_windows after prepare(): `starts` - n_win latent-frame offsets (host ints), `weights` [n_win, La] fp32 on
        this context's device (host/long_form.WindowPlan); the library copies both.  starts = None (or one window) clears it."""
        with torch.cuda.device(self.device):
            if starts is None or weights is None:
                _check(self.lib, self.lib.foley_set_windows(self._h, 0, None, None, _stream()), "foley_set_windows")
                return
            starts = [int(s) for s in starts]
            if weights.dtype != torch.float32 or weights.device != self.device or weights.dim() != 2 or weights.shape[0] != len(starts):
                raise FoleyRuntimeError("set_windows: weights must be [n_win, La] fp32 on the context's device")
            if getattr(self, "plan", None) is not None and weights.shape[1] != int(self.plan["La"]):
                raise FoleyRuntimeError("set_windows: weights must have the plan's La columns")
            weights = weights.contiguous()
            arr = (C.c_int32 * len(starts))(*starts)
            _check(self.lib, self.lib.foley_set_windows(self._h, len(starts), arr, _ptr(weights), _stream()), "foley_set_windows")

    def set_guidance(self, sched: Optional[torch.Tensor], rescale: float = 0.0):
        """foley_set_guidance after prepare(): `sched` [n_iter, 2] fp32 rows {g_video, g_text} per loop iteration (any device;
        the library copies it from the host), `rescale` phi in [0, 1].  sched None and rescale 0 clear the state."""
        arr, n = None, 0
        if sched is not None:
            t = sched.detach().to("cpu", torch.float32).contiguous()
            if t.dim() != 2 or t.shape[1] != 2:
                raise FoleyRuntimeError("set_guidance: the schedule is [n_iter, 2] (g_video, g_text per iteration)")
            n = int(t.shape[0])
            arr = (C.c_float * (2 * n))(*t.flatten().tolist())
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.foley_set_guidance(self._h, arr, n, float(rescale), _stream()), "foley_set_guidance")

    def set_projected_guidance(self, mode: int = 0, rows: Optional[torch.Tensor] = None):
        """foley_set_projected_guidance after prepare(): mode 1 (APG) or 2 (CFG-Zero*) with `rows` [n_iter, 4] fp32 {eta, beta, R,
        live} per loop iteration (tables.projection_rows; any device, the library copies it from the host); mode 0 clears."""
        arr, n = None, 0
        if rows is not None:
            t = rows.detach().to("cpu", torch.float32).contiguous()
            if t.dim() != 2 or t.shape[1] != 4:
                raise FoleyRuntimeError("set_projected_guidance: the rows are [n_iter, 4] (eta, beta, R, live per iteration)")
            n = int(t.shape[0])
            arr = (C.c_float * (4 * n))(*t.flatten().tolist())
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.foley_set_projected_guidance(self._h, int(mode), arr, n, _stream()), "foley_set_projected_guidance")

    def set_step_cache(self, mode: int = 0, skip=None, threshold: float = 0.0, poly=None, interval=None, max_consecutive: int = 0):
        """foley_set_step_cache after prepare() (host/step_cache.py states the policy): mode 0 clears; 1 = schedule with `skip`, one
        0 / 1 entry per iteration of the prepared plan; 2 = threshold with `poly` (highest degree first, None: identity),
        `interval` = (lo, hi) iteration indices that may skip (None: all) and `max_consecutive` (0: no cap)."""
        arr = (C.c_uint8 * len(skip))(*[1 if v else 0 for v in skip]) if skip is not None else None
        pol = (C.c_double * len(poly))(*[float(k) for k in poly]) if poly else None
        itv = (C.c_int32 * 2)(int(interval[0]), int(interval[1])) if interval is not None else None
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.foley_set_step_cache(self._h, int(mode), arr, len(skip) if skip is not None else 0, float(threshold),
                                                           pol, len(poly) if poly else 0, itv, int(max_consecutive or 0), _stream()),
                   "foley_set_step_cache")

    def set_multistep(self, order: int = 0):
        """foley_set_multistep after prepare(): order 2 or 3 switches the step to its history kernel (the plan's solver_coef rows
        carry the Adams-Bashforth weights, tables.solver_table(multistep_order=)); 0 or 1 clears the state."""
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.foley_set_multistep(self._h, int(order), _stream()), "foley_set_multistep")

    def step_cache_report(self):
        """(rel, skipped) of the last sample() under the step cache: per iteration the measured change (-1.0: not measured -
        iteration 0, and every iteration of schedule mode) and 0 / 1."""
        n = int(self.plan["n_iter"])
        rel, sk = (C.c_float * n)(), (C.c_int32 * n)()
        _check(self.lib, self.lib.foley_step_cache_report(self._h, rel, sk, n), "foley_step_cache_report")
        return list(rel), list(sk)

    def abort(self) -> None:
        """Ask a foley_sample running on another thread to stop after its current iteration (it raises FoleyRuntimeError)."""
        _check(self.lib, self.lib.foley_abort(self._h), "foley_abort")

    def dac_decode(self, latents: torch.Tensor) -> torch.Tensor:
        clips, _c, T = latents.shape
        hop = self.dac_cfg.hop
        wave = torch.empty(clips, 1, T * hop, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.foley_dac_decode(self._h, _ptr(latents), clips, T, _ptr(wave), _stream()),
                   "foley_dac_decode")
        return wave

    def dac_encode(self, wave: torch.Tensor) -> torch.Tensor:
        """DAC.encode (continuous=True): wave [clips, 1, T] fp32 on the GPU -> posterior parameters
        [clips, 2*latent, T'] (rows [:latent] mean, [latent:] logvar).  The waveform is right-padded
        to a multiple of the hop like DAC.preprocess (dac.py:225-234)."""
        cfg = self.dac_cfg
        rates = list(cfg.encoder_rates)
        hop = 1
        for r in rates:
            hop *= r
        clips, _one, T = wave.shape
        Tp = -(-T // hop) * hop
        if Tp != T:
            wave = torch.nn.functional.pad(wave, (0, Tp - T))
        wave = wave.contiguous().float()
        out = torch.empty(clips, 2 * cfg.latent_dim, Tp // hop, dtype=torch.float32, device=self.device)
        arr = (C.c_int32 * len(rates))(*rates)
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.foley_dac_encode(self._h, _ptr(wave), clips, Tp, cfg.encoder_dim, arr, len(rates),
                                                       _ptr(out), _stream()), "foley_dac_encode")
        return out

    def profile_forward(self, latents: torch.Tensor, it: int = 0, repeats: int = 2):
        """Per-op HIP-event profile of the eager DiT forward: list of dicts (label, calls_per_forward, avg_us =
        the dispatch's own start->stop time, flop / bytes per launch) + the cost of an empty event bracket in us."""
        cap = 64
        arr = (ProfEntryC * cap)()
        n, br = C.c_int(0), C.c_float(0.0)
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.foley_profile_forward(self._h, _ptr(latents), int(it), int(repeats), arr, cap,
                                                            C.byref(n), C.byref(br), _stream()), "foley_profile_forward")
        out = []
        for e in arr[:n.value]:
            calls = max(e.calls, 1)
            out.append({"label": e.label.decode(), "kernel": e.kernel.decode(errors="replace"), "calls_per_forward": e.calls / repeats,
                        "avg_us": 1e3 * e.total_ms / calls,
                        "flop_per_launch": e.flop / calls, "bytes_per_launch": e.bytes / calls})
        return out, 1e3 * br.value

    def last_elapsed_ms(self) -> float:
        ms = C.c_float()
        _check(self.lib, self.lib.foley_last_elapsed_ms(self._h, C.byref(ms)), "foley_last_elapsed_ms")
        return float(ms.value)


# ----------------------------------------------------------------------------- op-level wrappers (tests, microbench)
def bcast_local(buffers_per_device: Sequence[Sequence[torch.Tensor]]) -> float:
    """foley_bcast_local: `buffers_per_device[d][i]` is buffer i (uint8, same size on every device) on the d-th device; the
    root's (d = 0) contents reach every other device in ONE grouped RCCL launch.  Returns the wall time in seconds.  RCCL is
    the copy PyTorch ships (loaded into the process here if torch.distributed has not done so yet)."""
    import time
    lib = load_library()
    ndev, nbuf = len(buffers_per_device), len(buffers_per_device[0])
    devs = [b[0].device.index for b in buffers_per_device]
    if len(set(devs)) != ndev:
        raise FoleyRuntimeError("bcast_local: one entry per distinct device")
    for b in buffers_per_device:
        if len(b) != nbuf or any(t.device != b[0].device or not t.is_contiguous() for t in b):
            raise FoleyRuntimeError("bcast_local: every device carries the same buffers")
    rccl = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
    if os.path.exists(rccl):
        C.CDLL(rccl, mode=C.RTLD_GLOBAL)
    dev_arr = (C.c_int * ndev)(*devs)
    ptrs = (C.c_void_p * (ndev * nbuf))(*[t.data_ptr() for b in buffers_per_device for t in b])
    sizes = (C.c_uint64 * nbuf)(*[t.numel() * t.element_size() for t in buffers_per_device[0]])
    for d in devs:
        torch.cuda.synchronize(d)
    t0 = time.perf_counter()
    _check(lib, lib.foley_bcast_local(ndev, dev_arr, nbuf, ptrs, sizes), "foley_bcast_local")
    return time.perf_counter() - t0


def rowbcast(t: Optional[torch.Tensor], mode: int = 0, rows_per_cfg: int = 1, L: int = 1,
             ld: Optional[int] = None, Ls: int = 0, period: int = 0, periodic_cfgs: int = 0) -> RowBcastC:
    """mode 2: `t` holds Ls rows per cfg; token l of a clip reads row nearest_exact(l) (tables.nearest_exact_index).  period > 0:
    only `period` rows per cfg are stored - for every cfg half, or (periodic_cfgs = k > 0) for the first k halves only, the
    others following with all their Ls rows."""
    r = RowBcastC()
    r.Ls, r.period, r.periodic_cfgs = Ls, period, periodic_cfgs
    if t is not None and not t.is_cuda:
        raise FoleyRuntimeError("row-broadcast operand must live on the GPU")
    r.p = t.data_ptr() if t is not None else None     # views allowed: rows are addressed through `ld`
    r.ld = int(ld if ld is not None else (t.shape[-1] if t is not None else 0))
    r.mode, r.rows_per_cfg, r.L = mode, rows_per_cfg, L
    r._keepalive = t    # the struct only carries a raw pointer: keep the tensor alive with it
    return r


def op_gemm(A, W, bias=None, **kw) -> int:
    """Thin wrapper over foley_op_gemm (arguments: gemm_desc).  Returns the K split the launcher used."""
    lib = load_library()
    d = gemm_desc(A, W, bias, **kw)
    _check(lib, lib.foley_op_gemm(C.byref(d), _stream()), "foley_op_gemm")
    return int(d._used.value)


def gemm_desc(A, W, bias=None, *, M=None, epilogue=EPI_STORE_F32, out0=None, out1=None, ldc=None, conv=None,
              convT=None, rb: Optional[RowBcastC] = None, res=None, alpha=None, alphaC=1, tile=0, ksplit=0,
              partials=None, qkv: Optional["QkvSplitDescC"] = None, sconv=None, lda: Optional[int] = None,
              ldw: Optional[int] = None, NK=None, gelu_erf: bool = False, vrows=None) -> GemmDescC:
    """foley_gemm_desc of one GEMM.  conv=(seg, C, taps, dil) ; convT=(Tin, Cin, stride, Cout) ; vrows=(segV, segS) with M ;
    sconv=(Tin, Cin, stride): strided conv k=2*stride, pad ceil(stride/2) over clips of Tin rows.
    partials: fp32 [slabs, M, N] workspace for the deferred split-K of the gated-residual epilogue.
    After the launch, d._used holds the K split the launcher used."""
    d = GemmDescC()
    N, K = NK if NK is not None else W.shape      # NK: logical shape when W / A are row-padded storage (lda / ldw)
    d.A, d.W, d.bias = _ptr(A), _ptr(W), _ptr(bias) if bias is not None else None
    d.N, d.K = N, K
    if W.dtype in (torch.float8_e4m3fn, torch.float8_e5m2):      # fp8 weight storage, bf16 (or fp16) activations
        d.dtype, d.wfmt = dt_of(A) if A.dtype == torch.float16 else DT_BF16, (1 if W.dtype == torch.float8_e4m3fn else 2)
    else:
        d.dtype = dt_of(W)
    d.epilogue, d.tile, d.ksplit = epilogue, tile, ksplit
    d.gelu_erf = 1 if gelu_erf else 0
    if convT is not None:
        Tin, Cin, s, Cout = convT
        clips = A.numel() // (Tin * Cin)
        d.M, d.lda = clips * (Tin + 1), Cin
        d.segV, d.segS, d.taps, d.tapC, d.dil, d.tap0 = Tin + 1, Tin, 2, Cin, 1, -1
        d.osegV, d.out_seg, d.out_row = Tin + 1, Tin * s * Cout, s * Cout
        d.out_shift, d.out_check = -((s + 1) // 2) * Cout, 1
    elif sconv is not None:
        Tin, Cin, st_ = sconv
        clips = A.numel() // (Tin * Cin)
        Tout = Tin // st_
        d.M, d.lda = clips * Tout, Cin
        d.segV, d.segS, d.taps, d.tapC, d.dil, d.tap0 = Tout, Tin, 2 * st_, Cin, 1, -((st_ + 1) // 2)
        d.rstride = st_
        d.osegV, d.out_seg, d.out_row, d.out_shift, d.out_check = d.M, 0, (ldc or N), 0, 0
    elif conv is not None:
        seg, Cc, taps, dil = conv
        d.M = A.numel() // Cc if M is None else M
        d.lda = Cc
        d.segV, d.segS, d.taps, d.tapC, d.dil, d.tap0 = seg, seg, taps, Cc, dil, -((taps - 1) // 2) * dil
        d.osegV, d.out_seg, d.out_row, d.out_shift, d.out_check = d.M, 0, (ldc or N), 0, 0
    else:
        d.M = A.shape[0] if M is None else M
        d.lda = K
        d.segV, d.segS, d.taps, d.tapC, d.dil, d.tap0 = d.M, d.M, 1, K, 1, 0
        d.osegV, d.out_seg, d.out_row, d.out_shift, d.out_check = d.M, 0, (ldc or N), 0, 0
    if vrows is not None:      # virtual rows: row r of the product reads source row (r // segV) * segS + r % segV
        d.segV, d.segS = vrows
    if epilogue == EPI_SILUGATE_T and ldc is None and convT is None:
        d.out_row = N // 2
    if lda is not None:
        d.lda = lda
    if ldw is not None:
        d.ldw = ldw
    d.out0, d.out1 = _ptr(out0) if out0 is not None else None, _ptr(out1) if out1 is not None else None
    if rb is not None:
        d.rb = rb
    d.res = _ptr(res) if res is not None else None
    d.alpha = _ptr(alpha) if alpha is not None else None
    d.alphaC = alphaC
    d._used = C.c_int32(1)
    d.ksplit_used = C.pointer(d._used)
    if partials is not None:      # fp32 slabs, or slabs in the (16-bit) operand dtype
        d.partials, d.partial_slabs = _ptr(partials), partials.shape[0]
        d.partial_dtype = 0 if partials.dtype == torch.float32 else dt_of(partials)
    if qkv is not None:
        d.qkv = C.pointer(qkv)
    return d


def op_attention(q, k, v, outA, outB, split: int, kv_bdiv: int = 1):
    """fp32 q/k/v [B,H,S,hd], or bf16 / fp16 q/k [B,H,S,hd] with v transposed [B,H,hd,pitch]; hd = 128, 96 or 64."""
    lib = load_library()
    Bq, H, Sq, hd = q.shape
    Skv = k.shape[2]
    vt_pitch = v.shape[3] if q.dtype in (torch.bfloat16, torch.float16) else 0
    _check(lib, lib.foley_op_attention_hd(_ptr(q), _ptr(k), _ptr(v), dt_of(q), vt_pitch, Bq, H, Sq, Skv, kv_bdiv,
                                          _ptr(outA), _ptr(outB), split, dt_of(outB), hd, _stream()), "foley_op_attention_hd")


def op_attention_timeline(q, k, v, set_a, set_b, alpha, outA, outB, split: int):
    """foley_op_attention_timeline: q [Bq,H,Sq,128]; k [n_sets,H,Skv,128]; v [n_sets,H,Skv,128] (fp32) or transposed
    [n_sets,H,128,pitch] (bf16 / fp16, Skv <= 96); set_a / set_b int32 and alpha fp32 [Bq,Sq] on the device."""
    lib = load_library()
    Bq, H, Sq, hd = q.shape
    n_sets, Skv = k.shape[0], k.shape[2]
    half = q.dtype in (torch.bfloat16, torch.float16)
    if hd != 128 or k.shape[1] != H or k.shape[3] != 128 or k.dtype != q.dtype or v.dtype != q.dtype or v.shape[0] != n_sets or \
            v.shape[1] != H or (v.shape[2] != 128 if half else tuple(v.shape[2:]) != (Skv, 128)):
        raise FoleyRuntimeError("op_attention_timeline: q [Bq,H,Sq,128], k [n_sets,H,Skv,128], v [n_sets,H,Skv,128] or transposed [n_sets,H,128,pitch]")
    for t, dt in ((set_a, torch.int32), (set_b, torch.int32), (alpha, torch.float32)):
        if t.dtype != dt or t.numel() != Bq * Sq or t.device != q.device:
            raise FoleyRuntimeError("op_attention_timeline: set_a / set_b int32 and alpha fp32 of [Bq, Sq] on q's device")
    if outA.numel() != Bq * split * H * 128 or outB.numel() != Bq * (Sq - split) * H * 128 or outA.dtype != outB.dtype:
        raise FoleyRuntimeError("op_attention_timeline: outA [Bq*split, H*128] and outB [Bq*(Sq-split), H*128] of one dtype")
    _check(lib, lib.foley_op_attention_timeline(_ptr(q), _ptr(k), _ptr(v), dt_of(q), v.shape[3] if half else 0, Bq, H, Sq, Skv, n_sets,
                                                _ptr(set_a), _ptr(set_b), _ptr(alpha), _ptr(outA), _ptr(outB), split, dt_of(outB),
                                                _stream()), "foley_op_attention_timeline")


def op_attention_scatter(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out_rows: torch.Tensor, out: torch.Tensor,
                         grp_q: int = 0, grp_kv: int = 0) -> None:
    """Attention at head_dim 64 (operands as op_qkv_regroup returns them) whose query (g, t) is written to row out_rows[g, t] of
    out [rows, H*64] (foley_op_attention_scatter).  grp_q / grp_kv > 0 (16-bit operands): block-diagonal - each sequence is a pack
    of groups of grp_q queries that attend their own grp_kv keys only."""
    lib = load_library()
    G, H, Sq, hd = q.shape
    half = q.dtype in (torch.bfloat16, torch.float16)
    Skv = k.shape[2]
    if hd != 64 or out_rows.dtype != torch.int32 or out_rows.numel() != G * Sq or out.dim() != 2 or out.shape[1] != H * 64 or \
            not out.is_contiguous() or not out_rows.is_contiguous() or out_rows.device != q.device or out.device != q.device or \
            k.shape[:2] != q.shape[:2] or not (q.is_contiguous() and k.is_contiguous()
                                                                                                       and v.is_contiguous()):
        raise FoleyRuntimeError("op_attention_scatter: head_dim 64, contiguous q / k / v of one (G, H), int32 out_rows [G, Sq], contiguous out [rows, H*64]")
    if (grp_q > 0) != (grp_kv > 0) or (grp_q > 0 and not half):
        raise FoleyRuntimeError("op_attention_scatter: grp_q and grp_kv come together and need 16-bit operands")
    _check(lib, lib.foley_op_attention_scatter(_ptr(q), _ptr(k), _ptr(v), dt_of(q), v.shape[3] if half else 0, G, H, Sq, Skv,
                                               grp_q, grp_kv, _ptr(out_rows), _ptr(out), out.shape[0], dt_of(out), _stream()), "foley_op_attention_scatter")


def op_qkv_regroup(qkv: torch.Tensor, heads: int, idx_q: torch.Tensor, idx_kv: torch.Tensor):
    """qkv [rows, 3*heads*64] (fp32 / bf16 / fp16) -> (q [G,H,Sq,64], k [G,H,Skv,64], v): v [G,H,Skv,64] for fp32 operands, v
    TRANSPOSED [G,H,64,ceil32(Skv)] (zeros beyond Skv) for 16-bit operands - what op_attention reads.  idx_q [G,Sq] / idx_kv [G,Skv]
    int32 source rows on the device."""
    lib = load_library()
    G, Sq = idx_q.shape
    Skv = idx_kv.shape[1]
    if qkv.dim() != 2 or qkv.shape[1] != 3 * heads * 64 or idx_kv.shape[0] != G or idx_q.dtype != torch.int32 or idx_kv.dtype != torch.int32:
        raise FoleyRuntimeError("op_qkv_regroup: qkv [rows, 3*H*64], int32 index tables with one row per group")
    if not (qkv.is_contiguous() and idx_q.is_contiguous() and idx_kv.is_contiguous()) or idx_q.device != qkv.device or idx_kv.device != qkv.device:
        raise FoleyRuntimeError("op_qkv_regroup: contiguous qkv (the kernel's row pitch is 3*H*64) and contiguous index tables on qkv's device")
    half = qkv.dtype in (torch.bfloat16, torch.float16)
    pitch = (Skv + 31) // 32 * 32 if half else 0
    q = torch.empty(G, heads, Sq, 64, device=qkv.device, dtype=qkv.dtype)
    k = torch.empty(G, heads, Skv, 64, device=qkv.device, dtype=qkv.dtype)
    v = torch.empty((G, heads, 64, pitch) if half else (G, heads, Skv, 64), device=qkv.device, dtype=qkv.dtype)
    _check(lib, lib.foley_op_qkv_regroup(_ptr(qkv), qkv.shape[0], dt_of(qkv), heads, _ptr(idx_q), G, Sq, _ptr(idx_kv), Skv, _ptr(q), _ptr(k), _ptr(v),
                                         pitch, _stream()), "foley_op_qkv_regroup")
    return q, k, v


def op_resize_aa_u8(x: torch.Tensor, axis: int, len_out: int, xmin: torch.Tensor, xsize: torch.Tensor, weights: torch.Tensor,
                     precision: int) -> torch.Tensor:
    """One pass of the antialiased uint8 resize along `axis` of a contiguous uint8 tensor (foley_op_resize_aa_u8): tables xmin /
    xsize int32 [len_out], weights int16 [len_out, kmax] on the device (host/encoders.py::aa_tables)."""
    lib = load_library()
    if x.dtype != torch.uint8 or not x.is_contiguous() or xmin.dtype != torch.int32 or xsize.dtype != torch.int32 or \
            weights.dtype != torch.int16 or weights.shape[0] != len_out or xmin.numel() != len_out or xsize.numel() != len_out:
        raise FoleyRuntimeError("op_resize_aa_u8: contiguous uint8 frames; int32 xmin / xsize [len_out], int16 weights [len_out, kmax]")
    axis %= x.dim()
    shape = list(x.shape)
    outer = 1
    for d in shape[:axis]:
        outer *= d
    inner = 1
    for d in shape[axis + 1:]:
        inner *= d
    len_in = shape[axis]
    shape[axis] = len_out
    out = torch.empty(shape, device=x.device, dtype=torch.uint8)
    if out.numel():
        _check(lib, lib.foley_op_resize_aa_u8(_ptr(x), outer, len_in, inner, len_out, _ptr(xmin), _ptr(xsize), _ptr(weights),
                                              weights.shape[1], precision, _ptr(out), _stream()), "foley_op_resize_aa_u8")
    return out


def op_resample_sinc(x: torch.Tensor, orig: int, new: int, taps: torch.Tensor, width: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B, N] fp32 -> [B, ceil(N * new / orig)] fp32 (foley_op_resample_sinc; orig / new reduced by their gcd, taps [new, ntaps]
    fp32 on the device from host/sync_score.py::sinc_resample_taps).  out: a contiguous fp32 [B, ceil(N * new / orig)] to write
    into (allocated when None)."""
    lib = load_library()
    if x.dim() != 2 or x.dtype != torch.float32 or taps.dtype != torch.float32 or taps.dim() != 2 or taps.shape[0] != new:
        raise FoleyRuntimeError("op_resample_sinc: x [B, N] fp32, taps [new, ntaps] fp32")
    B, N = x.shape
    n_out = -(-N * new // orig)
    if out is None:
        out = torch.empty(B, n_out, device=x.device, dtype=torch.float32)
    if tuple(out.shape) != (B, n_out) or out.dtype != torch.float32:
        raise FoleyRuntimeError("op_resample_sinc: out [B, ceil(N * new / orig)] fp32")
    _check(lib, lib.foley_op_resample_sinc(_ptr(x), B, N, orig, new, _ptr(taps), taps.shape[1], width, _ptr(out), n_out, _stream()),
           "foley_op_resample_sinc")
    return out


def op_logmel(w16: torch.Tensor, basis: torch.Tensor, mel_lo: torch.Tensor, mel_len: torch.Tensor, mel_w: torch.Tensor,
              out_dtype: torch.dtype = torch.float32, with_mel: bool = False, out: Optional[torch.Tensor] = None,
              mel_out: Optional[torch.Tensor] = None):
    """16 kHz waveform [B, N16] fp32 -> AST patch matrix [B*S*72, 256] in out_dtype (foley_op_logmel), S = (N16 - 10240) // 5120 + 1;
    with_mel: also the normalised log-mel [B*S, 128, 66] fp32.  Tables from host/sync_score.py::logmel_tables.  out / mel_out:
    contiguous tensors of those shapes to write into (out's dtype replaces out_dtype; mel_out implies with_mel)."""
    lib = load_library()
    if w16.dim() != 2 or w16.dtype != torch.float32 or w16.shape[1] < 10240:
        raise FoleyRuntimeError("op_logmel: w16 [B, N16 >= 10240] fp32")
    if basis.numel() != 2 * 400 * 544 or mel_lo.numel() != 128 or mel_len.numel() != 128 or mel_w.dim() != 2 or mel_w.shape[0] != 128 or \
            mel_lo.dtype != torch.int32 or mel_len.dtype != torch.int32 or mel_w.dtype != torch.float32 or basis.dtype != torch.float32:
        raise FoleyRuntimeError("op_logmel: basis [2, 400, 544] fp32, int32 mel_lo / mel_len [128], mel_w [128, pitch] fp32")
    B, N16 = w16.shape
    S = (N16 - 10240) // 5120 + 1
    with_mel = with_mel or mel_out is not None
    patches = torch.empty(B * S * 72, 256, device=w16.device, dtype=out_dtype) if out is None else out
    mel = torch.empty(B * S, 128, 66, device=w16.device, dtype=torch.float32) if with_mel and mel_out is None else mel_out
    if tuple(patches.shape) != (B * S * 72, 256) or (mel is not None and (tuple(mel.shape) != (B * S, 128, 66) or mel.dtype != torch.float32)):
        raise FoleyRuntimeError("op_logmel: out [B*S*72, 256], mel_out [B*S, 128, 66] fp32")
    _check(lib, lib.foley_op_logmel(_ptr(w16), B, N16, _ptr(basis), _ptr(mel_lo), _ptr(mel_len), _ptr(mel_w), mel_w.shape[1],
                                    _ptr(patches), dt_of(patches), _ptr(mel) if with_mel else None, _stream()), "foley_op_logmel")
    return (patches, mel) if with_mel else patches


def op_melspec_db(x: torch.Tensor, starts: torch.Tensor, basis: torch.Tensor, mel_lo: torch.Tensor, mel_len: torch.Tensor,
                  mel_w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """48 kHz waveform [B, N >= 1024] fp32 -> dB-mel spectrograms [B * W, 1001, 64] fp32 of the ten-second windows that start at
    starts [W] int32 (foley_op_melspec_db; N < 480000: one window, the extractor's repeatpad).  Tables from
    host/clap_score.py::melspec_tables.  out: a contiguous fp32 [B * W, 1001, 64] to write into (allocated when None)."""
    lib = load_library()
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[1] < 1024 or starts.dtype != torch.int32 or starts.dim() != 1 or starts.numel() < 1:
        raise FoleyRuntimeError("op_melspec_db: x [B, N >= 1024] fp32, starts [W] int32")
    if basis.numel() != 2 * 1024 * 544 or basis.dtype != torch.float32 or mel_lo.numel() != 64 or mel_len.numel() != 64 or \
            mel_lo.dtype != torch.int32 or mel_len.dtype != torch.int32 or mel_w.dim() != 2 or mel_w.shape[0] != 64 or mel_w.dtype != torch.float32:
        raise FoleyRuntimeError("op_melspec_db: basis [2, 1024, 544] fp32, int32 mel_lo / mel_len [64], mel_w [64, pitch] fp32")
    B, N = x.shape
    W = starts.numel()
    if W > 1 and N < 480000:
        raise FoleyRuntimeError("op_melspec_db: a clip below ten seconds has one window")
    if out is None:
        out = torch.empty(B * W, 1001, 64, device=x.device, dtype=torch.float32)
    if tuple(out.shape) != (B * W, 1001, 64) or out.dtype != torch.float32:
        raise FoleyRuntimeError("op_melspec_db: out [B * W, 1001, 64] fp32")
    _check(lib, lib.foley_op_melspec_db(_ptr(x), B, N, _ptr(starts), W, _ptr(basis), _ptr(mel_lo), _ptr(mel_len), _ptr(mel_w),
                                        mel_w.shape[1], _ptr(out), _stream()), "foley_op_melspec_db")
    return out


def op_spec_patches(spec: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, resize_idx: Optional[torch.Tensor],
                    resize_w: Optional[torch.Tensor], Tq: int, ratio: int, out_dtype: torch.dtype, Kp: int) -> torch.Tensor:
    """spec [G, T, F] fp32 -> patch matrix [G * (ratio F / 4) * (Tq / 4), Kp] in out_dtype (foley_op_spec_patches): BatchNorm affine
    per bin, the 4-tap time resize (resize_idx int32 / resize_w fp32 [ratio * Tq, 4], or None for T == ratio * Tq), the fold of
    reshape_mel2img and the im2col of the 4x4 patch embedding; columns [16, Kp) are zero."""
    lib = load_library()
    if spec.dim() != 3 or spec.dtype != torch.float32:
        raise FoleyRuntimeError("op_spec_patches: spec [G, T, F] fp32")
    G, T, F = spec.shape
    if scale.numel() != F or shift.numel() != F or scale.dtype != torch.float32 or shift.dtype != torch.float32:
        raise FoleyRuntimeError("op_spec_patches: fp32 scale / shift [F]")
    if (resize_idx is None) != (resize_w is None):
        raise FoleyRuntimeError("op_spec_patches: the resize table is index and weight together")
    if resize_idx is not None and (resize_idx.dtype != torch.int32 or resize_w.dtype != torch.float32 or
                                   tuple(resize_idx.shape) != (ratio * Tq, 4) or tuple(resize_w.shape) != (ratio * Tq, 4)):
        raise FoleyRuntimeError("op_spec_patches: resize_idx int32 / resize_w fp32 [ratio * Tq, 4]")
    if resize_idx is None and T != ratio * Tq:
        raise FoleyRuntimeError("op_spec_patches: without a resize table T must equal ratio * Tq")
    if F % 4 or Tq % 4:
        raise FoleyRuntimeError("op_spec_patches: F and Tq must be multiples of 4")
    out = torch.empty(G * (ratio * F // 4) * (Tq // 4), Kp, device=spec.device, dtype=out_dtype)
    _check(lib, lib.foley_op_spec_patches(_ptr(spec), G, T, F, _ptr(scale), _ptr(shift), _ptr(resize_idx), _ptr(resize_w), Tq, ratio,
                                          _ptr(out), dt_of(out), Kp, _stream()), "foley_op_spec_patches")
    return out


def op_window_attention(qkv: torch.Tensor, heads: int, table: torch.Tensor, bias: torch.Tensor, mask: Optional[torch.Tensor] = None,
                        out: Optional[torch.Tensor] = None, win_tokens: int = 64) -> torch.Tensor:
    """Windowed attention straight from a fused projection (foley_op_window_attention): qkv [rows, 3 * heads * 32], table
    [n_win, 64] int32 source rows, bias [heads, 64, 64] fp32, mask [nW, 64, 64] fp32 or None (window g reads mask g % nW) ->
    out [rows, >= heads * 32] in qkv's dtype (allocated [rows, heads * 32] when None; rows no window names keep their content).
    The library refuses any head dim but 32 and any window but 64 tokens; the table's VALUES are the caller's to check."""
    lib = load_library()
    if qkv.dim() != 2 or table.dim() != 2 or table.dtype != torch.int32 or table.shape[1] != win_tokens or bias.dtype != torch.float32 or \
            tuple(bias.shape) != (heads, win_tokens, win_tokens):
        raise FoleyRuntimeError("op_window_attention: qkv [rows, 3*H*hd], int32 table [n_win, tokens], fp32 bias [H, tokens, tokens]")
    if mask is not None and (mask.dtype != torch.float32 or mask.dim() != 3 or tuple(mask.shape[1:]) != (win_tokens, win_tokens)):
        raise FoleyRuntimeError("op_window_attention: fp32 mask [nW, tokens, tokens]")
    rows = qkv.shape[0]
    if out is None:
        out = torch.empty(rows, heads * 32, device=qkv.device, dtype=qkv.dtype)
    if out.dim() != 2 or out.shape[0] != rows or out.dtype != qkv.dtype or out.stride(1) != 1:
        raise FoleyRuntimeError("op_window_attention: out [rows, >= H*32] in qkv's dtype, unit column stride")
    _check(lib, lib.foley_op_window_attention(_ptr(qkv), dt_of(qkv), rows, qkv.shape[1], heads, win_tokens, _ptr(table), table.shape[0],
                                              _ptr(bias), _ptr(mask), mask.shape[0] if mask is not None else 0, out.data_ptr(),
                                              out.stride(0), _stream()), "foley_op_window_attention")
    return out


def op_ln_mod(x, eps, shift: Optional[RowBcastC], scale: Optional[RowBcastC], out):
    lib = load_library()
    M, D = x.shape
    _check(lib, lib.foley_op_ln_mod(_ptr(x), M, D, eps, C.byref(shift) if shift else None,
                                    C.byref(scale) if scale else None, _ptr(out), dt_of(out), _stream()),
           "foley_op_ln_mod")


EPI_QKV_SPLIT = 7


def qkv_split_desc(L, H, gains: Sequence, poss: Sequence, dsts: Sequence, S_tot, tok_off, eps, cos, sin,
                   vt_pitch: int = 0, attn=None) -> QkvSplitDescC:
    """Descriptor of the fused head-split epilogue (op_gemm(..., epilogue=EPI_QKV_SPLIT, qkv=desc)).
    attn = (k [sets,H,Skv,128], vt [sets,H,128,pitch], out [M,H*128], bdiv): ask for the attention against those cached
    keys in the same epilogue; desc.fused() tells after the launch whether the library took that form."""
    q = QkvSplitDescC()
    q.L, q.H, q.nK = L, H, len(dsts)
    for i in range(len(dsts)):
        q.gain[i] = _ptr(gains[i]) if gains[i] is not None else None
        q.pos[i] = _ptr(poss[i]) if poss[i] is not None else None
        q.dst[i] = _ptr(dsts[i])
    q.out_dtype, q.vt_pitch, q.S_tot, q.tok_off, q.eps = dt_of(dsts[0]), vt_pitch, S_tot, tok_off, eps
    q.cos_tab, q.sin_tab = _ptr(cos), _ptr(sin)
    q._keepalive = (list(gains), list(poss), list(dsts), cos, sin)
    if attn is not None:
        k, vt, out, bdiv = attn
        q.attn_k, q.attn_vt, q.attn_out = _ptr(k), _ptr(vt), _ptr(out)
        q.attn_skv, q.attn_pitch, q.attn_bdiv = k.shape[2], vt.shape[3], bdiv
        q._flag = C.c_int32(0)
        q.attn_fused = C.pointer(q._flag)
        q._keepalive += (k, vt, out)
    return q


def op_ln_mod_pending(x, eps, shift: Optional[RowBcastC], scale: Optional[RowBcastC], out, partials, k: int, bias,
                      gate: RowBcastC):
    """LayerNorm of x after x += gate * (sum(partials[:k]) + bias), x updated in place.  `partials`: fp32, or out's
    16-bit dtype (the slabs a GEMM with 16-bit `partials` left)."""
    lib = load_library()
    M, D = x.shape
    pdt = 0 if partials.dtype == torch.float32 else dt_of(partials)
    _check(lib, lib.foley_op_ln_mod_pending2(_ptr(x), M, D, eps, C.byref(shift) if shift else None,
                                             C.byref(scale) if scale else None, _ptr(out), dt_of(out), _ptr(partials), pdt,
                                             k, _ptr(bias) if bias is not None else None, C.byref(gate), _stream()),
           "foley_op_ln_mod_pending2")


def op_qkv_split(qkv, L, H, gains: Sequence, poss: Sequence, dsts: Sequence, S_tot, tok_off, eps, cos, sin,
                 vt_pitch: int = 0):
    lib = load_library()
    nK = len(dsts)
    M = qkv.shape[0]
    arr = lambda xs: (C.c_void_p * nK)(*[(_ptr(x) if x is not None else None) for x in xs])
    _check(lib, lib.foley_op_qkv_split(_ptr(qkv), M, L, H, nK, arr(gains), arr(poss), arr(dsts), dt_of(dsts[0]),
                                       vt_pitch, S_tot, tok_off, eps, _ptr(cos), _ptr(sin), _stream()),
           "foley_op_qkv_split")


def _rows_dt(rows_out) -> int:
    return DT_F32 if rows_out is None else dt_of(rows_out)      # rows_out None: the step stages no model input rows


def _windows_tables(x, starts, weights):
    clips, _c, L = x.shape
    if starts.dtype != torch.int32 or weights.dtype != torch.float32 or tuple(weights.shape) != (starts.numel(), L):
        raise FoleyRuntimeError("windows ops: starts [n_win] int32 and weights [n_win, L] fp32 on the device")
    if clips % starts.numel() != 0:
        raise FoleyRuntimeError("windows ops: clips must be a multiple of n_win")
    return int(starts.numel())


def guidance_desc(sched: Optional[torch.Tensor] = None, clip_scale: Optional[torch.Tensor] = None) -> GuidanceDescC:
    """Guidance descriptor of op_solver_step(gd=) and foley_op_guidance_stats: sched [n_iter, 2] fp32 and clip_scale [clips] fp32 device tensors (None: absent)."""
    for t, what in ((sched, "sched"), (clip_scale, "clip_scale")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise FoleyRuntimeError(f"guidance_desc: {what} must be a contiguous fp32 tensor")
    if sched is not None and (sched.dim() != 2 or sched.shape[1] != 2):
        raise FoleyRuntimeError("guidance_desc: sched is [n_iter, 2]")
    return GuidanceDescC(_ptr(sched), _ptr(clip_scale))


def projection_desc(mode: int, rows: Optional[torch.Tensor], coef: Optional[torch.Tensor], plane: Optional[torch.Tensor] = None) -> ProjectionDescC:
    """Projection descriptor of op_guidance_project and op_solver_step(proj=): rows [n_iter, 4], coef [clips, 2] and plane
    [clips*L, C] fp32 device tensors (plane None: CFG-Zero*)."""
    for t, what in ((rows, "rows"), (coef, "coef"), (plane, "plane")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise FoleyRuntimeError(f"projection_desc: {what} must be a contiguous fp32 tensor")
    if rows is not None and (rows.dim() != 2 or rows.shape[1] != 4):
        raise FoleyRuntimeError("projection_desc: rows is [n_iter, 4]")
    return ProjectionDescC(_ptr(rows), _ptr(coef), _ptr(plane), int(mode))


def op_solver_step(pred, x, x_saved, d_acc, ncfg, guidance, coef, step_ptr, rows_out, *, gd: Optional[GuidanceDescC] = None,
                   hist: Optional[torch.Tensor] = None, slots: Optional[int] = None, edit=None, windows=None,
                   proj: Optional[ProjectionDescC] = None, projected_entry: bool = False):
    """foley_op_solver_step: x_saved / d_acc may be None for single-stage tables (euler), rows_out None to leave the next input
    rows unstaged.  gd: a guidance_desc; hist: a velocity ring [slots, clips, C, L] fp32 (slots 1 or 2, taken from the tensor
    unless given).  edit=(x0 [1 | clips, C, L], noise [clips, C, L], mask [1 | clips, L] or [L] or None: all ones) selects the
    edit form, windows=(starts [n_win] int32, weights [n_win, L] fp32, Ltot) with x [variations*n_win, C, L] the windows form.
    proj: a projection_desc - the step goes through foley_op_solver_step_projected (projected_entry: that entry with a null
    descriptor, which is foley_op_solver_step bit for bit)."""
    lib = load_library()
    clips, Cc, L = x.shape
    if hist is not None and (hist.dtype != torch.float32 or not hist.is_contiguous() or hist.dim() != 4
                             or tuple(hist.shape[1:]) != (clips, Cc, L)):
        raise FoleyRuntimeError("op_solver_step: hist is a contiguous fp32 tensor [slots, clips, C, L]")
    d = StepDescC(_ptr(pred), _ptr(x), _ptr(x_saved), _ptr(d_acc), clips, Cc, L, ncfg, float(guidance), _rows_dt(rows_out),
                  _ptr(coef), _ptr(step_ptr), _ptr(rows_out))
    if gd is not None:
        d.gd = gd
    d.hist = _ptr(hist)
    d.hist_slots = int(slots) if slots is not None else (int(hist.shape[0]) if hist is not None else 0)
    if edit is not None:
        x0, noise, mask = edit
        d.x0, d.x0_clips, d.noise, d.mask = _ptr(x0), int(x0.shape[0]), _ptr(noise), _ptr(mask)
        d.mask_clips = (1 if mask.dim() == 1 else int(mask.shape[0])) if mask is not None else 0
    if windows is not None:
        starts, weights, Ltot = windows
        d.n_win, d.starts, d.weights, d.Ltot = _windows_tables(x, starts, weights), _ptr(starts), _ptr(weights), int(Ltot)
    if proj is not None or projected_entry:
        _check(lib, lib.foley_op_solver_step_projected(C.byref(d), C.byref(proj) if proj is not None else None, _stream()),
               "foley_op_solver_step_projected")
        return
    _check(lib, lib.foley_op_solver_step(C.byref(d), _stream()), "foley_op_solver_step")


def flowedit_desc(pred, z, x_src, noise, mask, coef, step_ptr, rows_out, g_src: float, g_tar: float) -> FlowEditDescC:
    """foley_flowedit_desc from device tensors: z [V, C, L], x_src [1 | V, C, L], noise [noise_rows, V, C, L], mask [L] or
    [1 | V, L] or None, coef [n_iter, 8]; pred / coef / step_ptr may be None for op_flowedit_stage, rows_out for op_flowedit_step."""
    V, Cc, L = z.shape
    for t, what in ((pred, "pred"), (z, "z"), (x_src, "x_src"), (noise, "noise"), (mask, "mask"), (coef, "coef")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise FoleyRuntimeError(f"flowedit_desc: {what} must be a contiguous fp32 tensor")
    if x_src.dim() != 3 or tuple(x_src.shape[1:]) != (Cc, L) or noise.dim() != 4 or tuple(noise.shape[1:]) != (V, Cc, L):
        raise FoleyRuntimeError("flowedit_desc: x_src [src_clips, C, L] and noise [noise_rows, V, C, L] must match z [V, C, L]")
    if mask is not None and mask.shape[-1] != L:
        raise FoleyRuntimeError("flowedit_desc: mask must have L columns")
    if pred is not None and tuple(pred.shape) != (4 * V * L, Cc):
        raise FoleyRuntimeError("flowedit_desc: pred is [2*2V*L, C]")
    if rows_out is not None and (rows_out.numel() != 4 * V * L * Cc or not rows_out.is_contiguous()):
        raise FoleyRuntimeError("flowedit_desc: rows_out is [2*2V*L, C]")
    mask_clips = (1 if mask.dim() == 1 else int(mask.shape[0])) if mask is not None else 0
    return FlowEditDescC(_ptr(pred), _ptr(z), _ptr(x_src), _ptr(noise), _ptr(mask), _ptr(coef), _ptr(step_ptr), _ptr(rows_out),
                         V, Cc, L, int(coef.shape[0]) if coef is not None else int(noise.shape[0]), _rows_dt(rows_out),
                         int(x_src.shape[0]), int(noise.shape[0]), mask_clips, float(g_src), float(g_tar))


def op_flowedit_step(pred, z, x_src, noise, mask, coef, step_ptr, rows_out, g_src: float, g_tar: float) -> None:
    """foley_op_flowedit_step: one FlowEdit iteration on z [V, C, L] in place from pred [2*2V*L, C]; rows_out [2*2V*L, C] (or
    None) receives the next model input rows of both branches; *step_ptr is read as the iteration and advanced."""
    lib = load_library()
    d = flowedit_desc(pred, z, x_src, noise, mask, coef, step_ptr, rows_out, g_src, g_tar)
    _check(lib, lib.foley_op_flowedit_step(C.byref(d), _stream()), "foley_op_flowedit_step")


def op_flowedit_stage(z, x_src, noise, rows_out, sigma: float, noise_row: int = 0) -> None:
    """foley_op_flowedit_stage: rows_out [2*2V*L, C] from z, x_src and noise row `noise_row` at `sigma`."""
    lib = load_library()
    d = flowedit_desc(None, z, x_src, noise, None, None, None, rows_out, 0.0, 0.0)
    _check(lib, lib.foley_op_flowedit_stage(C.byref(d), float(sigma), int(noise_row), _stream()), "foley_op_flowedit_stage")


# The four names callers used before ABI 13, kept as plain forwards so that code written against them still runs.  Options go through
# as keywords, so a further one is added to op_solver_step alone.
def op_solver_step_edit(pred, x, x_saved, d_acc, ncfg, guidance, coef, step_ptr, rows_out, x0, noise, mask=None):
    op_solver_step(pred, x, x_saved, d_acc, ncfg, guidance, coef, step_ptr, rows_out, edit=(x0, noise, mask))


def op_solver_step_windows(pred, x, x_saved, d_acc, ncfg, guidance, coef, step_ptr, rows_out, starts, weights, Ltot):
    op_solver_step(pred, x, x_saved, d_acc, ncfg, guidance, coef, step_ptr, rows_out, windows=(starts, weights, Ltot))


def op_solver_step_guided(gd, *core, **options):
    op_solver_step(*core, gd=gd, **options)


def op_solver_step_hist(hist, *core, **options):
    op_solver_step(*core, hist=hist, **options)


def op_guidance_stats(pred, clips, L, ncfg, guidance, sched, step_ptr, rescale, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """foley_op_guidance_stats: pred [ncfg*clips*L, C] fp32 -> the rescale factors [clips] fp32 (new, or `out`)."""
    lib = load_library()
    if pred.dtype != torch.float32 or pred.dim() != 2 or pred.shape[0] != ncfg * clips * L:
        raise FoleyRuntimeError("op_guidance_stats: pred [ncfg*clips*L, C] fp32")
    if out is None:
        out = torch.empty(clips, dtype=torch.float32, device=pred.device)
    n = int(lib.foley_op_guidance_stats_work(clips, L))
    work = torch.empty(max(n, 1), dtype=torch.float32, device=pred.device)
    gd = guidance_desc(sched, out)
    _check(lib, lib.foley_op_guidance_stats(C.byref(gd), _ptr(pred), clips, int(pred.shape[1]), L, ncfg, float(guidance),
                                            _ptr(step_ptr), float(rescale), _ptr(work), n, _stream()), "foley_op_guidance_stats")
    return out


def op_guidance_project(proj: ProjectionDescC, pred, clips, La, guidance, sched, step_ptr) -> None:
    """foley_op_guidance_project: pred [2*clips*La, C] fp32 -> proj.coef [clips, 2] (and, APG, proj.plane updated in place)."""
    lib = load_library()
    if pred.dtype != torch.float32 or pred.dim() != 2 or pred.shape[0] != 2 * clips * La:
        raise FoleyRuntimeError("op_guidance_project: pred [2*clips*La, C] fp32")
    n = int(lib.foley_op_guidance_project_work(clips, La))
    work = torch.empty(max(n, 1), dtype=torch.float32, device=pred.device)
    gd = guidance_desc(sched, None)
    _check(lib, lib.foley_op_guidance_project(C.byref(proj), C.byref(gd), _ptr(pred), clips, int(pred.shape[1]), La, float(guidance),
                                              _ptr(step_ptr), _ptr(work), n, _stream()), "foley_op_guidance_project")


def op_cache_probe(a0: torch.Tensor, Bc: int, eps: float, shift: Optional[RowBcastC], scale: Optional[RowBcastC], m_prev: torch.Tensor,
                   rel: Optional[torch.Tensor] = None) -> torch.Tensor:
    """foley_op_cache_probe: a0 [Bc*La, D] fp32 -> m over m_prev, the change per batch row [Bc] fp32 (new, or `rel`)."""
    lib = load_library()
    M, D = a0.shape
    if a0.dtype != torch.float32 or M % Bc or m_prev.dtype != torch.float32 or m_prev.numel() != a0.numel():
        raise FoleyRuntimeError("op_cache_probe: a0 [Bc*La, D] and m_prev of its size, fp32")
    La = M // Bc
    n = int(lib.foley_op_cache_probe_work(Bc, La))
    work = torch.empty(n, dtype=torch.float32, device=a0.device)
    rel = rel if rel is not None else torch.empty(Bc, dtype=torch.float32, device=a0.device)
    _check(lib, lib.foley_op_cache_probe(_ptr(a0), Bc, La, D, float(eps), C.byref(shift) if shift else None,
                                         C.byref(scale) if scale else None, m_prev.data_ptr(), _ptr(work), n,
                                         _ptr(rel), _stream()), "foley_op_cache_probe")
    return rel


def op_cache_delta(aN: torch.Tensor, delta: torch.Tensor):
    """foley_op_cache_delta: delta <- aN - delta in place (fp32, any shape; views with a pitch are not supported)."""
    lib = load_library()
    if aN.dtype != torch.float32 or delta.dtype != torch.float32 or aN.numel() != delta.numel():
        raise FoleyRuntimeError("op_cache_delta: two fp32 tensors of one size")
    _check(lib, lib.foley_op_cache_delta(_ptr(aN), _ptr(delta), aN.numel(), _stream()), "foley_op_cache_delta")


def op_cache_apply(audio: torch.Tensor, delta: torch.Tensor):
    """foley_op_cache_apply: audio += delta in place (fp32)."""
    lib = load_library()
    if audio.dtype != torch.float32 or delta.dtype != torch.float32 or audio.numel() != delta.numel():
        raise FoleyRuntimeError("op_cache_apply: two fp32 tensors of one size")
    _check(lib, lib.foley_op_cache_apply(_ptr(audio), _ptr(delta), audio.numel(), _stream()), "foley_op_cache_apply")


def op_windows_stitch(x: torch.Tensor, starts: torch.Tensor, weights: torch.Tensor, Ltot: int) -> torch.Tensor:
    """foley_op_windows_stitch: x [variations*n_win, C, L] fp32 -> new [variations, C, Ltot] fp32."""
    lib = load_library()
    if x.dtype != torch.float32 or x.dim() != 3:
        raise FoleyRuntimeError("op_windows_stitch: x [variations*n_win, C, L] fp32")
    clips, Cc, L = x.shape
    n_win = _windows_tables(x, starts, weights)
    out = torch.empty(clips // n_win, Cc, int(Ltot), dtype=torch.float32, device=x.device)
    _check(lib, lib.foley_op_windows_stitch(_ptr(x), clips, n_win, Cc, L, int(Ltot), _ptr(starts), _ptr(weights), _ptr(out),
                                            _stream()), "foley_op_windows_stitch")
    return out


def op_flow_mix(noise: torch.Tensor, x0: torch.Tensor, sigma: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """foley_op_flow_mix: sigma*noise + (1 - sigma)*x0 -> [clips, C, L] fp32 (new, or `out`); x0 [1 | clips, C, L] (1: shared)."""
    lib = load_library()
    if noise.dtype != torch.float32 or x0.dtype != torch.float32 or noise.dim() != 3 or x0.dim() != 3:
        raise FoleyRuntimeError("op_flow_mix: noise [clips, C, L] and x0 [1 | clips, C, L] fp32")
    clips, Cc, L = noise.shape
    if tuple(x0.shape[1:]) != (Cc, L):
        raise FoleyRuntimeError(f"op_flow_mix: x0 {tuple(x0.shape)} does not match noise {tuple(noise.shape)}")
    if out is None:
        out = torch.empty_like(noise)
    elif out.dtype != torch.float32 or out.shape != noise.shape:
        raise FoleyRuntimeError("op_flow_mix: out must be fp32 of noise's shape")
    _check(lib, lib.foley_op_flow_mix(_ptr(noise), _ptr(x0), x0.shape[0], clips, Cc, L, float(sigma), _ptr(out), _stream()),
           "foley_op_flow_mix")
    return out


def op_latent_rows(x, ncfg, out):
    lib = load_library()
    clips, Cc, L = x.shape
    _check(lib, lib.foley_op_latent_rows(_ptr(x), clips, Cc, L, ncfg, _ptr(out), dt_of(out), _stream()),
           "foley_op_latent_rows")


def op_dac_out(s, w, bias, out):
    lib = load_library()
    B, T, Cc = s.shape
    _check(lib, lib.foley_op_dac_out(_ptr(s), _ptr(w), _ptr(bias), B, T, Cc, _ptr(out), _stream()),
           "foley_op_dac_out")


def _f32(*ts):
    for t in ts:
        if t is not None and t.dtype != torch.float32:
            raise FoleyRuntimeError("fp32 operand expected")


def op_rows_add_act(a: Optional[torch.Tensor], v: Optional[torch.Tensor], out: torch.Tensor, act_silu: bool):
    """foley_op_rows_add_act: out [R, D] (fp32 / bf16 / fp16) = act(a + v); a [R, D] fp32 or None, v [D] fp32 or None."""
    lib = load_library()
    R, D = out.shape
    _f32(a, v)
    if (a is not None and tuple(a.shape) != (R, D)) or (v is not None and v.numel() != D):
        raise FoleyRuntimeError("op_rows_add_act: a [R, D] and v [D] must match out [R, D]")
    _check(lib, lib.foley_op_rows_add_act(_ptr(a), _ptr(v), R, D, int(bool(act_silu)), _ptr(out), dt_of(out), _stream()),
           "foley_op_rows_add_act")


def op_add_periodic(x: torch.Tensor, pos: torch.Tensor, out: torch.Tensor):
    """foley_op_add_periodic: out [R, D] = x [R, D] + pos [period, D] row r % period."""
    lib = load_library()
    R, D = x.shape
    _f32(x, pos)
    if pos.dim() != 2 or pos.shape[1] != D or tuple(out.shape) != (R, D):
        raise FoleyRuntimeError("op_add_periodic: x [R, D], pos [period, D], out [R, D]")
    _check(lib, lib.foley_op_add_periodic(_ptr(x), _ptr(pos), R, D, pos.shape[0], _ptr(out), dt_of(out), _stream()),
           "foley_op_add_periodic")


def op_gather_rows(src: torch.Tensor, idx: torch.Tensor, groups: int, out: torch.Tensor):
    """foley_op_gather_rows: src [groups*src_rows, D] fp32, idx [n_idx] int32 in [0, src_rows) -> out [groups*n_idx, D] fp32."""
    lib = load_library()
    _f32(src, out)
    n_idx, D = idx.numel(), src.shape[1]
    if idx.dtype != torch.int32 or src.shape[0] % groups or tuple(out.shape) != (groups * n_idx, D):
        raise FoleyRuntimeError("op_gather_rows: int32 idx, src [groups*src_rows, D], out [groups*n_idx, D]")
    src_rows = src.shape[0] // groups
    if int(idx.min()) < 0 or int(idx.max()) >= src_rows:
        raise FoleyRuntimeError("op_gather_rows: index outside [0, src_rows)")
    _check(lib, lib.foley_op_gather_rows(_ptr(src), _ptr(idx), n_idx, groups, src_rows, D, _ptr(out), _stream()),
           "foley_op_gather_rows")


def op_cast(src: torch.Tensor, dst: torch.Tensor):
    """foley_op_cast: dst = src converted element by element (fp32 <-> bf16 / fp16, fp32 -> fp32)."""
    lib = load_library()
    if src.numel() != dst.numel():
        raise FoleyRuntimeError("op_cast: element counts differ")
    _check(lib, lib.foley_op_cast(_ptr(src), dt_of(src), _ptr(dst), dt_of(dst), src.numel(), _stream()), "foley_op_cast")


def op_rows_periodic_check(x: torch.Tensor, period: int, flags: torch.Tensor):
    """foley_op_rows_periodic_check: x [groups, rows, D] fp32; flags [groups] int32, flags[g] |= 1 when group g is not periodic."""
    lib = load_library()
    groups, rows, D = x.shape
    _f32(x)
    if flags.dtype != torch.int32 or flags.numel() < min(groups, 32):
        raise FoleyRuntimeError("op_rows_periodic_check: int32 flags, one per group")
    _check(lib, lib.foley_op_rows_periodic_check(_ptr(x), groups, rows, int(period), D, _ptr(flags), _stream()),
           "foley_op_rows_periodic_check")


def op_dac_in(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, alpha: torch.Tensor, out0: torch.Tensor, out1: torch.Tensor):
    """foley_op_dac_in: x [B, T] fp32, w [7, C] (tap-major), bias / alpha [C] -> out0 = conv, out1 = snake(conv), both [B*T, C]."""
    lib = load_library()
    B, T = x.shape
    Cc = bias.numel()
    _f32(x, w, bias, alpha, out0, out1)
    if w.numel() != 7 * Cc or alpha.numel() != Cc or tuple(out0.shape) != (B * T, Cc) or tuple(out1.shape) != (B * T, Cc):
        raise FoleyRuntimeError("op_dac_in: w [7, C], bias / alpha [C], out0 / out1 [B*T, C]")
    _check(lib, lib.foley_op_dac_in(_ptr(x), _ptr(w), _ptr(bias), _ptr(alpha), B, T, Cc, _ptr(out0), _ptr(out1), _stream()),
           "foley_op_dac_in")


def op_rows_to_planes(rows: torch.Tensor, B: int, out: torch.Tensor):
    """foley_op_rows_to_planes: rows [B*T, C] fp32 -> out [B, C, T] fp32."""
    lib = load_library()
    _f32(rows, out)
    Cc = rows.shape[1]
    if rows.shape[0] % B or tuple(out.shape) != (B, Cc, rows.shape[0] // B):
        raise FoleyRuntimeError("op_rows_to_planes: rows [B*T, C], out [B, C, T]")
    _check(lib, lib.foley_op_rows_to_planes(_ptr(rows), B, rows.shape[0] // B, Cc, _ptr(out), _stream()), "foley_op_rows_to_planes")


# ----------------------------------------------------------------------------- loudness / true peak (host/loudness.py)
def _wave(x: torch.Tensor, what: str):
    """x [B, C, N] fp32 on the device, C 1 or 2, rows at one pitch ld >= N (a slice of a longer buffer is fine) -> (ptr, B, C, N, ld)."""
    if x.dim() != 3 or x.dtype != torch.float32 or x.shape[1] not in (1, 2) or x.shape[0] < 1 or x.shape[2] < 1:
        raise FoleyRuntimeError(f"{what}: x [B, C in (1, 2), N] fp32")
    if not x.is_cuda:
        raise FoleyRuntimeError("libfoley_hip.so needs device tensors (got a CPU tensor)")
    B, Cc, N = x.shape
    ld = x.stride(1) if Cc > 1 else (x.stride(0) if B > 1 else N)
    if x.stride(2) != 1 or ld < N or (Cc > 1 and B > 1 and x.stride(0) != Cc * ld):
        raise FoleyRuntimeError(f"{what}: the rows of x must lie at one pitch >= N with unit sample stride")
    return x.data_ptr(), B, Cc, N, ld


def op_loudness_energy(x: torch.Tensor, T: torch.Tensor) -> torch.Tensor:
    """foley_op_loudness_energy: x [B, C, N] fp32 -> K-weighted hop energies e [B, C, N // 4800] fp64.  T: the 4x4 fp64 transition
    matrix of one 480-sample chunk (host/loudness.py::chunk_transition), a CPU tensor."""
    lib = load_library()
    ptr, B, Cc, N, ld = _wave(x, "op_loudness_energy")
    if T.is_cuda or T.dtype != torch.float64 or tuple(T.shape) != (4, 4):
        raise FoleyRuntimeError("op_loudness_energy: T is a [4, 4] fp64 CPU tensor")
    nh = N // 4800
    e = torch.empty(B, Cc, nh, device=x.device, dtype=torch.float64)
    if nh:
        work = torch.empty(B * Cc * nh * 40, device=x.device, dtype=torch.float64)
        T16 = (C.c_double * 16)(*T.reshape(-1).tolist())
        _check(lib, lib.foley_op_loudness_energy(ptr, B, Cc, N, ld, T16, _ptr(work), work.numel(), _ptr(e), _stream()),
               "foley_op_loudness_energy")
    return e


def op_loudness_gate(e: torch.Tensor):
    """foley_op_loudness_gate: e [B, C, nh] fp64 -> (lufs [B], gamma [B], block_lufs [B, max(nh - 3, 0)]) fp64 on the device."""
    lib = load_library()
    if e.dim() != 3 or e.dtype != torch.float64 or e.shape[1] not in (1, 2):
        raise FoleyRuntimeError("op_loudness_gate: e [B, C in (1, 2), nh] fp64")
    B, Cc, nh = e.shape
    lufs = torch.empty(B, device=e.device, dtype=torch.float64)
    gamma = torch.empty(B, device=e.device, dtype=torch.float64)
    blocks = torch.empty(B, max(nh - 3, 0), device=e.device, dtype=torch.float64)
    _check(lib, lib.foley_op_loudness_gate(_ptr(e) if nh else _ptr(lufs), B, Cc, nh, _ptr(lufs), _ptr(gamma),
                                           _ptr(blocks) if nh > 3 else None, _stream()), "foley_op_loudness_gate")
    return lufs, gamma, blocks


def _taps36(taps: torch.Tensor):
    if taps.is_cuda or taps.dtype != torch.float32 or tuple(taps.shape) != (3, 12):
        raise FoleyRuntimeError("true-peak taps: a [3, 12] fp32 CPU tensor (host/loudness.py::true_peak_taps)")
    return (C.c_float * 36)(*taps.reshape(-1).tolist())


def op_true_peak(x: torch.Tensor, taps: torch.Tensor, with_sample_peak: bool = True, with_envelope: bool = False):
    """foley_op_true_peak: x [B, C, N] fp32 -> (true_peak [B], sample_peak [B] or None, envelope [B, N] or None), linear fp32."""
    lib = load_library()
    ptr, B, Cc, N, ld = _wave(x, "op_true_peak")
    tp = torch.empty(B, device=x.device, dtype=torch.float32)
    sp = torch.empty(B, device=x.device, dtype=torch.float32) if with_sample_peak else None
    env = torch.empty(B, N, device=x.device, dtype=torch.float32) if with_envelope else None
    _check(lib, lib.foley_op_true_peak(ptr, B, Cc, N, ld, _taps36(taps), _ptr(tp), _ptr(sp), _ptr(env), _stream()),
           "foley_op_true_peak")
    return tp, sp, env


def op_loudness_apply(x: torch.Tensor, gain: torch.Tensor, limiter: bool = False, ceiling: float = 1.0, lookahead: int = 240,
                      taps: Optional[torch.Tensor] = None, with_gain_curve: bool = False):
    """foley_op_loudness_apply: y = gain[b] * x (one fp32 multiply), or with `limiter` the look-ahead limiter under the linear
    `ceiling` with `lookahead` samples; a gain of 0 copies the clip unchanged.  Returns y [B, C, N] (and g [B, N] with
    with_gain_curve, limiter mode only)."""
    lib = load_library()
    ptr, B, Cc, N, ld = _wave(x, "op_loudness_apply")
    if gain.dtype != torch.float32 or gain.numel() != B:
        raise FoleyRuntimeError("op_loudness_apply: gain [B] fp32")
    if limiter and taps is None:
        raise FoleyRuntimeError("op_loudness_apply: the limiter needs the true-peak taps")
    if with_gain_curve and not limiter:
        raise FoleyRuntimeError("op_loudness_apply: the gain curve exists in limiter mode only")
    y = torch.empty(B, Cc, N, device=x.device, dtype=torch.float32)
    g = torch.empty(B, N, device=x.device, dtype=torch.float32) if with_gain_curve else None
    _check(lib, lib.foley_op_loudness_apply(ptr, B, Cc, N, ld, _ptr(gain), int(bool(limiter)), float(ceiling), int(lookahead),
                                            _taps36(taps) if limiter else None, _ptr(y), N, _ptr(g), _stream()),
           "foley_op_loudness_apply")
    return (y, g) if with_gain_curve else y
