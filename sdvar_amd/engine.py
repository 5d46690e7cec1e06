"""ctypes binding of libsdvar_hip.so (include/sdvar_hip.h) and the host-side sampling loops built on it.

PyTorch is plumbing here: it owns the weight tensors and a few staging buffers (device memory + streams); every
operation of the draft -> verify loop is a call into the C ABI.  There is NO fallback: if the shared library is missing
or a call fails this module raises - the product path never routes through torch ops or the CPU oracle.

Reference loops restated on top of the ABI:
  * `Sampler.plain_ar`  - VAR.autoregressive_infer_cfg         (/root/reference/models/var.py:127-215)
  * `Sampler.spec_decode` - SDVAR.sdvar_autoregressive_infer_cfg_parallel_v1 with the resolved semantics of
    SURVEY.md App. C.1 (models/var.py:949-1070 draft/verify, 1160-1227 acceptance, 1318-1372 loop policy).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from .ladder import Ladder, as_ladder
from .noise import exponential_noise

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libsdvar_hip.so")
MAX_STAGES = 16
ABI_VERSION = 5
# GEMM arithmetic of the transformer blocks: 'f32' = fp32-in/fp32-accumulate MFMA; 'bf16x3' = exact 3-way bf16 split of both
# operands, 6 bf16 MFMA products, fp32 accumulate (fp32-accurate, 2.67x the matrix-pipe throughput).  See DESIGN.md section 4.
#   'f16x2' = two fp16 planes per operand (x ~ xh + xl to 2^-22), 3 fp16 MFMA products, fp32 accumulate: half the matrix work of bf16x3 at the same
#             measured accuracy while activations stay inside the fp16 range (csrc/gemm_f16x2.hip).
GEMM_MODES = ("f32", "bf16x3", "f16x2")
#   'f16'   = engine only (ModelCtx, SDVAR_GEMM_MODE, VAR.gemm_mode / tf_gemm_mode): an f16x2 model whose block and head GEMMs run as ONE fp16 product on the high
#             planes (csrc/gemm_half.hip) in calls of at least `h16_min_m` rows (default 2704, measured: tools/f16_mode_bench.py; sdvar_debug_set_variant / SDVAR_H16_MIN_M); smaller calls are f16x2's,
#             bit for bit.  fp16-autocast accuracy, NOT the fp32 modes' 1e-3 logit bar: sampled ids differ from the reference's.  See DESIGN.md section 4.
ENGINE_GEMM_MODES = GEMM_MODES + ("f16",)
HALF_KERNEL_CODE = 1128                     # last_gemm_cfg()["bm"] / sdvar_debug_plan_gemm's kernel code of the 128 x 128 half kernel
PLAN_FLAG_F16 = 8                           # sdvar_debug_plan_gemm: mode 2 with this flag bit = the plan of a gemm_mode 'f16' model
DEFAULT_GEMM_MODE = "f16x2"
PROF_CLASSES = ("gemm", "attention", "ln_modulate", "qk_norm_append", "sampler", "verify", "quant", "embed_misc", "attention_small", "gemm_small")


class SdvarError(RuntimeError):
    pass


class _ModelDesc(C.Structure):
    _fields_ = [("depth", C.c_int32), ("n_stages", C.c_int32), ("patch_nums", C.c_int32 * MAX_STAGES), ("vocab", C.c_int32),
                ("cvae", C.c_int32), ("num_classes", C.c_int32), ("max_batch", C.c_int32), ("max_chunk_stages", C.c_int32), ("kv_dtype", C.c_int32), ("gemm_mode", C.c_int32)]


class _VaeDesc(C.Structure):
    _fields_ = [("ch", C.c_int32), ("z_channels", C.c_int32), ("n_mult", C.c_int32), ("ch_mult", C.c_int32 * 8), ("num_res_blocks", C.c_int32),
                ("max_batch", C.c_int32), ("latent_hw", C.c_int32), ("plane_format", C.c_int32)]


_P, _I, _D, _U64, _U32 = C.c_void_p, C.c_int32, C.c_double, C.c_uint64, C.c_uint32
# name -> (restype, argtypes); must list every symbol declared in include/sdvar_hip.h (tests/test_abi.py checks it)
_SIGNATURES = {
    "sdvar_abi_version": (_I, []),
    "sdvar_last_error": (C.c_char_p, []),
    "sdvar_model_create": (_I, [C.POINTER(_ModelDesc), C.POINTER(_P)]),
    "sdvar_model_destroy": (_I, [_P]),
    "sdvar_model_bind_embed": (_I, [_P] * 8),
    "sdvar_model_bind_block": (_I, [_P, _I] + [_P] * 13),
    "sdvar_model_bind_shared_aln": (_I, [_P, _P, _P]),
    "sdvar_model_bind_head": (_I, [_P] * 6),
    "sdvar_model_begin": (_I, [_P, _I, _P, _P]),
    "sdvar_model_begin_cond": (_I, [_P, _I, _P, _P]),
    "sdvar_model_begin_rows": (_I, [_P, _I, _P, _P]),
    "sdvar_embed_teacher": (_I, [_P, _P, _P, _P]),
    "sdvar_model_export_prologue": (_I, [_P, _P, _P, _P, _P]),
    "sdvar_model_place_first": (_I, [_P, _P, _I, _P]),
    "sdvar_kv_len": (_I, [_P]),
    "sdvar_kv_set_len": (_I, [_P, _I]),
    "sdvar_kv_set_origin": (_I, [_P, _I]),
    "sdvar_head_forward": (_I, [_P, _P, _I, _P, _P]),
    "sdvar_embed_next": (_I, [_P, _P, _I, _P, _I, _I, _P]),
    "sdvar_embed_next_at": (_I, [_P, _P, _I, _I, _P, _I, _I, _P]),
    "sdvar_stage_forward": (_I, [_P, _P, _I, _I, _P, _P]),
    "sdvar_stage_first": (_I, [_P, _P, _P]),
    "sdvar_stage_forward_masked": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "sdvar_quant_create": (_I, [_I, C.POINTER(_I), _I, _I, _I, _I, C.POINTER(_P)]),
    "sdvar_quant_destroy": (_I, [_P]),
    "sdvar_quant_bind": (_I, [_P, _P, C.POINTER(_P), C.POINTER(_P)]),
    "sdvar_quant_next": (_I, [_P, _I, _P, _I, _P, _P, _I, _P]),
    "sdvar_quant_next_from": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _P]),
    "sdvar_quant_next_h": (_I, [_P, _I, _P, _P, _P, _I, _P]),
    "sdvar_quant_encode": (_I, [_P, _P, _I, _P, _P, _P, _P]),
    "sdvar_quant_encode_stats": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "sdvar_gumbel_mix": (_I, [_P, _P, _I, _I, _D, _D, _P, _U64, _U32, _U32, _P, _P]),
    "sdvar_vae_create": (_I, [C.POINTER(_VaeDesc), C.POINTER(_P)]),
    "sdvar_vae_destroy": (_I, [_P]),
    "sdvar_vae_tensor_count": (_I, [C.POINTER(_VaeDesc)]),
    "sdvar_vae_bind": (_I, [_P, C.POINTER(_P), _I, _P]),
    "sdvar_vae_decode": (_I, [_P, _P, _I, _P, _P]),
    "sdvar_vae_decode_raw": (_I, [_P, _P, _I, _P, _P]),
    "sdvar_vae_enc_create": (_I, [C.POINTER(_VaeDesc), C.POINTER(_P)]),
    "sdvar_vae_enc_destroy": (_I, [_P]),
    "sdvar_vae_enc_tensor_count": (_I, [C.POINTER(_VaeDesc)]),
    "sdvar_vae_enc_bind": (_I, [_P, C.POINTER(_P), _I, _P]),
    "sdvar_vae_enc_encode": (_I, [_P, _P, _I, _P, _P]),
    "sdvar_cfg_sample": (_I, [_P, _I, _I, _I, _D, _I, _D, _P, _U64, _U32, _U32, _P, _I, _P, _P]),
    "sdvar_verify_accept": (_I, [_P, _I, _I, _I, _I, C.POINTER(_I), C.POINTER(_D), _P, _I, _D, _P, _P, _P]),
    "sdvar_cfg_combine": (_I, [_P, _I, _I, _I, _I, C.POINTER(_I), C.POINTER(_D), _P, _P]),
    "sdvar_cfg_sample_rows": (_I, [_P, _I, _I, _I, _P, _P, _P, _I, _P, _U32, _P, _I, _P, _P]),
    "sdvar_verify_accept_rows": (_I, [_P, _I, _I, _I, _I, C.POINTER(_I), _P, _I, _P, _I, _D, _I, _I, _D, _P, _P, _P, _P, _P, _P]),
    "sdvar_cfg_combine_rows": (_I, [_P, _I, _I, _I, _I, C.POINTER(_I), _P, _I, _P, _P]),
    "sdvar_gumbel_mix_rows": (_I, [_P, _P, _I, _I, _D, _D, _P, _P, _I, _U32, _P, _P]),
    "sdvar_cfg_sample_forced": (_I, [_P, _I, _I, _I, _D, _I, _D, _P, _U64, _U32, _U32, _P, _I, _P, _P, _P, _I, _P]),
    "sdvar_cfg_sample_rows_forced": (_I, [_P, _I, _I, _I, _P, _P, _P, _I, _P, _U32, _P, _I, _P, _P, _P, _I, _P]),
    "sdvar_verify_accept_forced": (_I, [_P, _I, _I, _I, _I, C.POINTER(_I), C.POINTER(_D), _P, _I, _D, _I, _I, _D, _P, _P, _P, _P, _P, _P, _I, _P]),
    "sdvar_verify_accept_rows_forced": (_I, [_P, _I, _I, _I, _I, C.POINTER(_I), _P, _I, _P, _I, _D, _I, _I, _D, _P, _P, _P, _P, _P, _P, _I, _P]),
    "sdvar_mask_tokens": (_I, [_P, _I, _I, _I, C.POINTER(_I), _P, _P]),
    "sdvar_img_composite": (_I, [_P, _P, _P, _I, _I, C.c_int64, _P, _P]),
    "sdvar_xent_stats": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P]),
    "sdvar_img_err_stats": (_I, [_P, _P, C.c_int64, _P, _I, _P]),
    "sdvar_xent_train_fwd": (_I, [_P, C.c_int64, _P, C.c_int64, _I, _D, C.c_int64, _P, _P, _P, _P, _P, _I, _P]),
    "sdvar_xent_train_bwd": (_I, [_P, C.c_int64, _P, _P, _P, _I, _P, C.c_int64, _I, _D, C.c_int64, _P, _I, _P]),
    "sdvar_verify_accept_ex": (_I, [_P, _I, _I, _I, _I, C.POINTER(_I), C.POINTER(_D), _P, _I, _D, _I, _I, _D, _P, _P, _P, _P, _P, _P]),
    "sdvar_op_gemm": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _P, _I, _I, _P]),
    "sdvar_op_ln_modulate": (_I, [_P, _P, _P, _P, _P, _U64, _I, _I, _I, _I, _I, _P]),
    "sdvar_op_split_planes_f16": (_I, [_P, _P, _I, _I, _U64, _P, _P]),
    "sdvar_op_gemm_f16x2": (_I, [_P, _U64, _P, _U64, _P, _P, _P, _I, _P, _U64, _I, _I, _I, _I, _P, _I, _P, _I, _I, _P]),
    "sdvar_op_split_planes": (_I, [_P, _P, _I, _I, _U64, _P]),
    "sdvar_op_gemm_bf16x3": (_I, [_P, _U64, _P, _U64, _P, _P, _I, _P, _U64, _I, _I, _I, _I, _P, _I, _P, _I, _I, _P]),
    "sdvar_op_qk_norm_append": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "sdvar_op_attention": (_I, [_P, _P, _P, _I, _P, _P, _U64, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_I), C.POINTER(_I), _P]),
    "sdvar_op_conv_weight_planes": (_I, [_P, _P, _I, _I, _I, _U64, _I, _P, _P]),
    "sdvar_op_vae_prep": (_I, [_P, _P, _P, _P, _P, _U64, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "sdvar_op_conv_planes": (_I, [_P, _U64, _U64, _I, _P, _U64, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _U64, _I, _P]),
    "sdvar_op_conv_planes_ex": (_I, [_P, _U64, _U64, _I, _P, _U64, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _U64, _I, _I, _U64, _P, _P, C.POINTER(_I), _P]),
    "sdvar_op_upconv_weights": (_I, [_P, _P, _I, _I, _P]),
    "sdvar_op_vae_gn_stats": (_I, [_P, _I, _I, _I, _I, _P, _P, _P]),
    "sdvar_op_vae_attn": (_I, [_P, _P, _I, _I, _I, _P, _U64, _I, _P]),
    "sdvar_op_vae_conv_out": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "sdvar_op_vae_img_planes":(_I, [_P, _P, _U64, _I, _I, _I, _I, _I, _P]),
    "sdvar_op_vae_s2d_planes": (_I, [_P, _P, _U64, _I, _I, _I, _I, _I, _I, _P]),
    "sdvar_op_vae_s2d_weights": (_I, [_P, _P, _I, _I, _P]),
    "sdvar_op_quant_nearest": (_I, [_P, _I, _P, _I, _I, _P, _P, _P]),
    "sdvar_op_noise_fill": (_I, [_P, _I, _I, _I, _U64, _U32, _U32, _P]),
    "sdvar_op_sdpa": (_I, [_P, _P, _P, _P, C.POINTER(C.c_int64), _P, _I, C.POINTER(C.c_int64), _P, _I, _I, _I, _I, _I, _D, _P]),
    "sdvar_op_sdpa_lse": (_I, [_P, _P, _P, _P, _P, C.POINTER(C.c_int64), _P, _I, C.POINTER(C.c_int64), _P, _I, _I, _I, _I, _I, _D, _P]),
    "sdvar_op_sdpa_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64), _P, _I, C.POINTER(C.c_int64), _P, _I, _I, _I, _I, _I, _D, _P]),
    "sdvar_op_transpose_operand": (_I, [_P, _I, _I, _I, _I, _P, _U64, _P, _P]),
    "sdvar_op_gelu_operand": (_I, [_P, _I, _I, _I, _I, _P, _U64, _P]),
    "sdvar_op_gelu_bwd": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _U64, _P, _U64, _P, _U64, _P, _P]),
    "sdvar_op_colsum": (_I, [_P, _I, _I, _I, _P, _P]),
    "sdvar_op_scale_pair": (_I, [_P, _U64, _P, _I, _P, _P]),
    "sdvar_op_sdpa_skip_map": (_I, [_P, _I, C.POINTER(C.c_int64), _I, _I, _I, _I, _P, _P]),
    "sdvar_op_sdpa_h": (_I, [_P, _P, _P, _P, C.POINTER(C.c_int64), _I, _I, _I, _I, _I, _I, _D, _P]),
    "sdvar_op_sdpa_hm": (_I, [_P, _P, _P, _P, C.POINTER(C.c_int64), _I, _I, _I, _P, _I, C.POINTER(C.c_int64), _P, _I, _I, _I, _I, _I, _D, _P]),
    "sdvar_op_sdpa_hm_lse": (_I, [_P, _P, _P, _P, _P, C.POINTER(C.c_int64), _I, _I, _I, _P, _I, C.POINTER(C.c_int64), _P, _I, _I, _I, _I, _I, _D, _P]),
    "sdvar_op_sdpa_h_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64), _I, _I, _I, _P, _I, C.POINTER(C.c_int64), _P, _I, _I, _I, _I, _I, _D,
                                 _P]),
    "sdvar_op_gemm_h": (_I, [_P, _P, _I, _P, _P, _I, _I, _P, _P, _I, _I, _I, _I, _P]),
    "sdvar_op_gemm_h_ex": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "sdvar_op_half_operand": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "sdvar_op_gelu_bwd_h": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "sdvar_op_grad_operands": (_I, [_P, _I, _I, _I, _I, _P, _P, _U64, _P, _U64, _P, _P]),
    "sdvar_op_grad_operands_h": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "sdvar_op_operand_transpose_h": (_I, [_P, _I, _I, _P, _P]),
    "sdvar_op_adaln_fwd": (_I, [_P, _P, _I, C.c_int64, _P, _I, C.c_int64, _P, _I, _I, _I, _D, _P]),
    "sdvar_op_adaln_bwd_ws_bytes": (C.c_int64, [_I, _I, _I]),
    "sdvar_op_adaln_bwd": (_I, [_P, _P, _I, C.c_int64, _P, _P, _P, _I, _P, _I, _I, _P, _I, _I, _I, _D, _P]),
    "sdvar_op_gate_add_fwd": (_I, [_P, _P, _I, _P, _I, C.c_int64, _P, _P, _I, _I, _I, _P]),
    "sdvar_op_gate_add_bwd_ws_bytes": (C.c_int64, [_I, _I, _I]),
    "sdvar_op_gate_add_bwd": (_I, [_P, _P, _I, _P, _I, C.c_int64, _P, _P, _P, _I, _P, _I, _I, _I, _P]),
    "sdvar_op_qknorm_fwd": (_I, [_P, _I, _P, _P, _P, _D, _P, _P, _P, _I, _I, _I, _P]),
    "sdvar_op_qknorm_bwd_ws_bytes": (C.c_int64, [_I, _I, _I]),
    "sdvar_op_qknorm_bwd": (_I, [_P, _I, _P, _P, _D, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "sdvar_op_cond_lin_fwd": (_I, [_P, _I, C.c_int64, _P, _I, _P, _P, _I, _I, _I, _I, _P]),
    "sdvar_op_cond_lin_bwd_ws_bytes": (C.c_int64, [_I, _I, _I]),
    "sdvar_op_cond_lin_bwd": (_I, [_P, _P, _I, C.c_int64, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sdvar_op_embed_fwd": (_I, [_P, _I, _P, _D, _P, _P, C.c_int64, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "sdvar_op_embed_bwd_ws_bytes": (C.c_int64, [_I, _I, _I, _I]),
    "sdvar_op_embed_bwd": (_I, [_P, _I, _P, _P, _I, _P, _D, _P, _P, C.c_int64, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "sdvar_optim_grad_stats": (_I, [_P, _I, _P, _P, _D, _D, _D, _P, _U64, _P]),
    "sdvar_optim_adamw_step": (_I, [_P, _I, _D, _D, _D, _P, _U64, _P]),
    "sdvar_debug_set_gemm_cfg": (_I, [_I, _I]),
    "sdvar_debug_set_gemm_stamps": (_I, [_P]),
    "sdvar_debug_set_qkv_fuse": (_I, [_I]),
    "sdvar_debug_set_rowblk": (_I, [_I]),
    "sdvar_op_gemm_rowblk": (_I, [_P, _I, _P, _P, _I, _I, _P, _U64, _P, _U64, _P, _P, _P, _I, _P, _U64, _I, _I, _I, _I, _P, _I, _P, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sdvar_debug_set_variant": (_I, [C.c_char_p, _I]),
    "sdvar_debug_get_gemm_cfg": (_I, [C.POINTER(_I)]),
    "sdvar_debug_get_conv_cfg": (_I, [C.POINTER(_I)]),
    "sdvar_debug_get_conv_plan": (_I, [C.POINTER(_I)]),
    "sdvar_debug_plan_gemm": (_I, [_I, _I, _I, _I, _I, C.POINTER(_I)]),
    "sdvar_debug_set_f16x2_guard": (_I, [_I]),
    "sdvar_debug_get_f16x2_guard": (_I, [C.POINTER(_U64), _I]),
    "sdvar_prof_enable": (_I, [_I]),
    "sdvar_prof_collect": (_I, [C.POINTER(_D), C.POINTER(C.c_int64), C.POINTER(_D), C.POINTER(_D)]),
}

_lib = None


def load_library(path: str = LIB_PATH):
    """dlopen the HIP library and attach prototypes.  Raises (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise SdvarError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                         f"(make -C sdvar_amd/csrc); there is no CPU fallback for the sampler")
    lib = C.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    if lib.sdvar_abi_version() != ABI_VERSION:
        raise SdvarError("libsdvar_hip.so ABI version mismatch")
    _lib = lib
    return lib


def _check(rc: int):
    if rc != 0:
        raise SdvarError(f"libsdvar_hip error {rc}: {_lib.sdvar_last_error().decode()}")


def _ptr(t: Optional[torch.Tensor]):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device tensors must be contiguous CUDA(HIP) tensors"
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t: torch.Tensor, dev) -> torch.Tensor:
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


# ------------------------------------------------------------------------------------------------------- objects
class ModelCtx:
    """sdvar_model_t for one VAR transformer given its state_dict (reference key names)."""

    def __init__(self, sd: Dict[str, torch.Tensor], depth: int, patch_nums: Sequence[int], max_batch: int, max_chunk: int,
                 device, num_classes: int = 1000, kv_fp16: bool = False, gemm_mode: Optional[str] = None):
        self.lib = load_library()
        self.lad = as_ladder(patch_nums)
        self.depth, self.Cw, self.H = depth, 64 * depth, depth
        self.V = sd["head.weight"].shape[0]
        self.device = torch.device(device)
        self.max_batch, self.max_chunk = max_batch, max_chunk
        d = _ModelDesc()
        d.depth, d.n_stages, d.vocab, d.cvae, d.num_classes = depth, self.lad.S, self.V, sd["word_embed.weight"].shape[1], num_classes
        d.max_batch, d.max_chunk_stages, d.kv_dtype = max_batch, max_chunk, (1 if kv_fp16 else 0)
        self.kv_fp16 = bool(kv_fp16)
        self.gemm_mode = gemm_mode or os.environ.get("SDVAR_GEMM_MODE", DEFAULT_GEMM_MODE)
        if self.gemm_mode not in ENGINE_GEMM_MODES:
            raise SdvarError(f"gemm_mode {self.gemm_mode!r}: expected one of {ENGINE_GEMM_MODES}")
        d.gemm_mode = ENGINE_GEMM_MODES.index(self.gemm_mode)
        for i, p in enumerate(self.lad.patch_nums):
            d.patch_nums[i] = p
        self.h = C.c_void_p()
        with torch.cuda.device(self.device):
            _check(self.lib.sdvar_model_create(C.byref(d), C.byref(self.h)))
            self._keep: List[torch.Tensor] = []
            self.bind(sd)

    def bind(self, sd: Dict[str, torch.Tensor]):
        dev, k = self.device, self._keep
        k.clear()
        def w(name):
            t = _f32(sd[name], dev); k.append(t); return _ptr(t)
        st = _stream()
        _check(self.lib.sdvar_model_bind_embed(self.h, w("class_emb.weight"), w("pos_start"), w("pos_1LC"), w("lvl_embed.weight"),
                                               w("word_embed.weight"), w("word_embed.bias"), st))
        shared = "shared_ada_lin.1.weight" in sd                 # shared_aln=True checkpoints (VAR-d36-s): var.py:16-19, 81
        if shared:
            _check(self.lib.sdvar_model_bind_shared_aln(self.h, w("shared_ada_lin.1.weight"), w("shared_ada_lin.1.bias")))
        for i in range(self.depth):
            p = f"blocks.{i}."
            _check(self.lib.sdvar_model_bind_block(
                self.h, i, None if shared else w(p + "ada_lin.1.weight"), w(p + "ada_gss") if shared else w(p + "ada_lin.1.bias"),
                w(p + "attn.mat_qkv.weight"), w(p + "attn.q_bias"),
                w(p + "attn.v_bias"), w(p + "attn.scale_mul_1H11") if (p + "attn.scale_mul_1H11") in sd else None,      # absent: attn_l2_norm=False (basic_var.py:66-72)
                w(p + "attn.proj.weight"), w(p + "attn.proj.bias"),
                w(p + "ffn.fc1.weight"), w(p + "ffn.fc1.bias"), w(p + "ffn.fc2.weight"), w(p + "ffn.fc2.bias"), st))
        _check(self.lib.sdvar_model_bind_head(self.h, w("head_nm.ada_lin.1.weight"), w("head_nm.ada_lin.1.bias"), w("head.weight"), w("head.bias"), st))

    # thin wrappers ----------------------------------------------------------------------------------------------
    def begin(self, labels: torch.Tensor):
        assert labels.dtype == torch.int64 and labels.is_cuda
        self.B = labels.shape[0]; self.R = 2 * self.B
        _check(self.lib.sdvar_model_begin(self.h, self.B, _ptr(labels), _stream()))

    def begin_cond(self, cond: torch.Tensor):
        """The prologue from the conditioning rows (2B, C) themselves (`sos` of var.py:319-345) instead of labels."""
        assert cond.dtype == torch.float32 and cond.is_cuda and cond.dim() == 2 and cond.shape[1] == self.Cw and cond.shape[0] % 2 == 0
        self.B = cond.shape[0] // 2; self.R = 2 * self.B
        _check(self.lib.sdvar_model_begin_cond(self.h, self.B, _ptr(cond.contiguous()), _stream()))

    def begin_rows(self, labels: torch.Tensor):
        """The prologue for R unpaired rows (teacher forcing): row r conditioned on labels[r], num_classes = unconditional.  R <= 2 max_batch."""
        assert labels.dtype == torch.int64 and labels.is_cuda and labels.dim() == 1
        self.B, self.R = 0, labels.shape[0]
        _check(self.lib.sdvar_model_begin_rows(self.h, labels.shape[0], _ptr(labels.contiguous()), _stream()))

    def embed_teacher(self, xv: Optional[torch.Tensor], x: torch.Tensor):
        """Teacher-forcing input x (R, L, C) of the current begin_rows call from xv (R, L-1, Cvae) (var.py:230-235)."""
        _check(self.lib.sdvar_embed_teacher(self.h, _ptr(xv), _ptr(x), _stream()))

    def export_prologue(self):
        """(cond (R,C), lvl_pos (1,L,C), first_token_map (R,1,C)) of the current call (R = 2B for a CFG call), as SDVAR.init_param returns them."""
        f = dict(device=self.device, dtype=torch.float32)
        R = self.R
        cond, lvl, first = torch.empty(R, self.Cw, **f), torch.empty(1, self.lad.L, self.Cw, **f), torch.empty(R, 1, self.Cw, **f)
        _check(self.lib.sdvar_model_export_prologue(self.h, _ptr(cond), _ptr(lvl), _ptr(first), _stream()))
        return cond, lvl, first

    def place_first(self, x: torch.Tensor, ltot: int):
        _check(self.lib.sdvar_model_place_first(self.h, _ptr(x), ltot, _stream()))

    def embed_next(self, nxt: torch.Tensor, s_next: int, x: torch.Tensor, ltot: int, tok_off: int):
        _check(self.lib.sdvar_embed_next(self.h, _ptr(nxt), s_next, _ptr(x), ltot, tok_off, _stream()))

    def embed_next_at(self, nxt: torch.Tensor, s_next: int, pos_begin: int, x: torch.Tensor, ltot: int, tok_off: int):
        """embed_next with explicit lvl_pos rows (the resumed sampler of var.py:319-443 counts positions from the stage it starts at)."""
        _check(self.lib.sdvar_embed_next_at(self.h, _ptr(nxt), s_next, pos_begin, _ptr(x), ltot, tok_off, _stream()))

    def forward(self, x: torch.Tensor, s0: int, n: int, logits: torch.Tensor, bias: Optional[torch.Tensor] = None):
        """All blocks + head over stages s0 .. s0+n-1.  bias: explicit additive mask (l, K) instead of the block-causal rows (mask ablations)."""
        if bias is None:
            _check(self.lib.sdvar_stage_forward(self.h, _ptr(x), s0, n, _ptr(logits), _stream()))
        else:
            _check(self.lib.sdvar_stage_forward_masked(self.h, _ptr(x), s0, n, _ptr(bias), _ptr(logits), _stream()))

    def forward_first(self, logits: torch.Tensor):
        """Stage 0 from the model's own first-token map: equals place_first + forward(x, 0, 1), bit for bit.  After begin(labels) it is one launch that copies
        the call's rows out of the per-class stage-0 table (include/sdvar_hip.h: sdvar_stage_first); otherwise the computed pass."""
        _check(self.lib.sdvar_stage_first(self.h, _ptr(logits), _stream()))

    def kv_len(self) -> int:
        return self.lib.sdvar_kv_len(self.h)

    def kv_set_len(self, n: int):
        _check(self.lib.sdvar_kv_set_len(self.h, n))

    def kv_set_origin(self, stage: int):
        """Empty cache whose first key will be the first token of `stage` (hand-off sampler, var.py:817-824)."""
        _check(self.lib.sdvar_kv_set_origin(self.h, stage))

    def head_forward(self, x: torch.Tensor, l: int, logits: torch.Tensor):
        """VAR.get_logits (var.py:119-125) on x (2B, l, C) -> logits (2B, l, V)."""
        _check(self.lib.sdvar_head_forward(self.h, _ptr(x), l, _ptr(logits), _stream()))

    def close(self):
        if self.h:
            self.lib.sdvar_model_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class QuantCtx:
    """sdvar_quant_t from the VQVAE state_dict (quantize.embedding / quantize.quant_resi.*, any of the three Phi layouts)."""

    def __init__(self, vae_sd: Dict[str, torch.Tensor], patch_nums: Sequence[int], max_batch: int, device, prefix: str = "quantize."):
        self.lib = load_library()
        self.lad = as_ladder(patch_nums)
        self.device = torch.device(device)
        self.codebook = _f32(vae_sd[prefix + "embedding.weight"], self.device)
        self.V, self.Cv = self.codebook.shape
        from .weights import phi_names_in
        names = phi_names_in(vae_sd, prefix + "quant_resi.")          # PhiPartiallyShared (qresi_ls.<k>), PhiShared (qresi) or PhiNonShared (<k>): quant.py:27-32
        n_phi = len(names)
        if n_phi == 0:
            raise SdvarError(f"no Phi convolution under {prefix}quant_resi.* in the state_dict")
        self.pw = [_f32(vae_sd[n + ".weight"], self.device) for n in names]
        self.pb = [_f32(vae_sd[n + ".bias"], self.device) for n in names]
        pn = (_I * self.lad.S)(*self.lad.patch_nums)
        self.h = C.c_void_p()
        self.max_batch = int(max_batch)
        with torch.cuda.device(self.device):
            _check(self.lib.sdvar_quant_create(self.lad.S, pn, self.Cv, self.V, max_batch, n_phi, C.byref(self.h)))
        aw = (_P * n_phi)(*[t.data_ptr() for t in self.pw]); ab = (_P * n_phi)(*[t.data_ptr() for t in self.pb])
        _check(self.lib.sdvar_quant_bind(self.h, _ptr(self.codebook), aw, ab))

    def next(self, si: int, ids: torch.Tensor, ids_stride: int, f_hat: torch.Tensor, nxt: Optional[torch.Tensor], B: int, f_in: Optional[torch.Tensor] = None):
        """quant.py:187-196 for stage si.  f_in given: f_hat = f_in + Phi(...) (f_in is left untouched), else f_hat += Phi(...)."""
        nx = _ptr(nxt) if nxt is not None else None
        if f_in is None:
            _check(self.lib.sdvar_quant_next(self.h, si, C.c_void_p(ids.data_ptr()), ids_stride, _ptr(f_hat), nx, B, _stream()))
        else:
            _check(self.lib.sdvar_quant_next_from(self.h, si, C.c_void_p(ids.data_ptr()), ids_stride, _ptr(f_in), _ptr(f_hat), nx, B, _stream()))

    def next_h(self, si: int, h: torch.Tensor, f_hat: torch.Tensor, nxt: Optional[torch.Tensor], B: int):
        """The same from feature vectors h (B, pn^2, Cvae) instead of ids (more_smooth=True, var.py:206-210)."""
        _check(self.lib.sdvar_quant_next_h(self.h, si, _ptr(h), _ptr(f_hat), _ptr(nxt) if nxt is not None else None, B, _stream()))

    def encode(self, f: torch.Tensor, per_scale: bool = False):
        """f_to_idxBl_or_fhat (quant.py:135-166, using_znorm=False) of f (B, Cvae, HW, HW) on the device -> (ids (B, L) int64, final f_hat,
        f_hat after every scale (S, B, Cvae, HW, HW) or None)."""
        B, HW = f.shape[0], self.lad.patch_nums[-1]
        if f.dtype != torch.float32 or not f.is_contiguous() or f.device != self.device:
            f = f.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(f.shape[1:]) != (self.Cv, HW, HW) or B > self.max_batch:
            raise SdvarError(f"encode: f {tuple(f.shape)} does not fit (max_batch {self.max_batch}, {self.Cv} x {HW}^2)")
        ids = torch.empty(B, self.lad.L, device=self.device, dtype=torch.int64)
        f_hat = torch.empty_like(f)
        ps = torch.empty(self.lad.S, *f.shape, device=self.device, dtype=torch.float32) if per_scale else None
        _check(self.lib.sdvar_quant_encode(self.h, _ptr(f), B, _ptr(ids), _ptr(f_hat), _ptr(ps), _stream()))
        return ids, f_hat, ps

    def encode_stats(self, f: torch.Tensor, per_scale: bool = False, straight_through: bool = False):
        """VectorQuantizer2.forward in eval mode (quant.py:52-104) on the device: `encode` (the same launches, the same bits) -> (ids, f_hat, per_scale or
        None, hits (S, V) int32 = bincount of every scale's ids, sqerr (S,) float64 = sum (f_hat_s - f)^2 after every scale, f_st or None = the
        straight-through (f_hat - f) + f of quant.py:98)."""
        B, HW = f.shape[0], self.lad.patch_nums[-1]
        if f.dtype != torch.float32 or not f.is_contiguous() or f.device != self.device:
            f = f.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(f.shape[1:]) != (self.Cv, HW, HW) or B > self.max_batch:
            raise SdvarError(f"encode_stats: f {tuple(f.shape)} does not fit (max_batch {self.max_batch}, {self.Cv} x {HW}^2)")
        ids = torch.empty(B, self.lad.L, device=self.device, dtype=torch.int64)
        f_hat = torch.empty_like(f)
        ps = torch.empty(self.lad.S, *f.shape, device=self.device, dtype=torch.float32) if per_scale else None
        hits = torch.empty(self.lad.S, self.V, device=self.device, dtype=torch.int32)
        sqerr = torch.empty(self.lad.S, device=self.device, dtype=torch.float64)
        f_st = torch.empty_like(f) if straight_through else None
        _check(self.lib.sdvar_quant_encode_stats(self.h, _ptr(f), B, _ptr(ids), _ptr(f_hat), _ptr(ps), _ptr(hits), _ptr(sqerr), _ptr(f_st), _stream()))
        return ids, f_hat, ps, hits, sqerr, f_st

    def gumbel_mix(self, masked: torch.Tensor, B: int, l: int, ratio: float, tau: float, e: Optional[torch.Tensor], seed: int, draw: int, image_offset: int,
                   h_out: torch.Tensor):
        """var.py:206-208 + helpers.py:22-36: soft codebook mix of the masked CFG logits under gumbel noise -> h (B, l, Cvae)."""
        _check(self.lib.sdvar_gumbel_mix(self.h, _ptr(masked), B, l, float(ratio), float(tau), _ptr(e) if e is not None else None, seed & (2**64 - 1), draw,
                                         image_offset, _ptr(h_out), _stream()))

    def gumbel_mix_rows(self, masked: torch.Tensor, B: int, l: int, ratio: float, tau: float, e: Optional[torch.Tensor], rows: "RowParams", draw: int,
                        h_out: torch.Tensor):
        """gumbel_mix with image b's Philox key and image counter from the image table of `rows`."""
        _check(self.lib.sdvar_gumbel_mix_rows(self.h, _ptr(masked), B, l, float(ratio), float(tau), _ptr(e) if e is not None else None, rows.img_ptr(), rows.B,
                                              draw, _ptr(h_out), _stream()))

    def close(self):
        if self.h:
            self.lib.sdvar_quant_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


CONV_MODES = ("bf16x3", "f16x2", "f16")
_CONV_PLANE_FORMAT = {"bf16x3": 3, "f16x2": 2, "f16": 6}          # sdvar_vae_desc.plane_format (include/sdvar_hip.h)


def resolve_conv_mode(conv_mode: Optional[str], encoder: bool = False) -> str:
    """The operand mode of a VQVAE context's convolutions: the argument, else SDVAR_CONV_MODE, else the default.  "f16" (decoders only, opt-in) is an f16x2
    decoder whose convolutions multiply the high fp16 planes alone - not fp32-accurate.  An encoder feeds a nearest-code search whose ids
    would move, so it reads the environment's "f16" as "f16x2" and refuses an explicit one.  Decided before any device call."""
    if encoder and conv_mode == "f16":
        raise SdvarError("conv_mode 'f16' is a decoder mode: the encoder feeds the nearest-code search and stays fp32-accurate; expected 'bf16x3' or 'f16x2'")
    mode = conv_mode or os.environ.get("SDVAR_CONV_MODE", DEFAULT_GEMM_MODE if DEFAULT_GEMM_MODE != "f32" else "f16x2")
    if encoder and not conv_mode and mode == "f16":
        mode = "f16x2"
    if mode not in (CONV_MODES[:2] if encoder else CONV_MODES):
        raise SdvarError(f"conv_mode {mode!r}: expected " + ("'bf16x3' or 'f16x2'" if encoder else "'bf16x3', 'f16x2' or 'f16'"))
    return mode


class VaeCtx:
    """sdvar_vae_t from the VQVAE state_dict: `fhat_to_img` (vqvae.py:62-63) as hand-written HIP (csrc/conv.hip, csrc/vae.hip)."""

    def __init__(self, vae_sd: Dict[str, torch.Tensor], max_batch: int, device, latent_hw: int = 16, ch: Optional[int] = None,
                 ch_mult: Sequence[int] = (1, 1, 2, 2, 4), num_res_blocks: int = 2, conv_mode: Optional[str] = None):
        self.conv_mode = resolve_conv_mode(conv_mode)       # operands of the convolutions; "f16": one fp16 product per convolution (opt-in)
        self.lib = load_library()
        self.device = torch.device(device)
        z = vae_sd["post_quant_conv.weight"].shape[0]
        ch = ch if ch is not None else vae_sd["decoder.norm_out.weight"].shape[0] // ch_mult[0]
        d = _VaeDesc()
        d.ch, d.z_channels, d.n_mult, d.num_res_blocks, d.max_batch, d.latent_hw = ch, z, len(ch_mult), num_res_blocks, max_batch, latent_hw
        d.plane_format = _CONV_PLANE_FORMAT[self.conv_mode]
        for i, m in enumerate(ch_mult):
            d.ch_mult[i] = m
        self.desc, self.max_batch, self.latent_hw, self.z = d, max_batch, latent_hw, z
        self.out_hw = latent_hw << (len(ch_mult) - 1)
        names = self.tensor_names(vae_sd, ch_mult, num_res_blocks)
        self.tensors = []                                   # keeps the device copies alive: biases and GroupNorm affine stay borrowed
        for n in names:
            self.tensors += [_f32(vae_sd[n + ".weight"], self.device), _f32(vae_sd[n + ".bias"], self.device)]
        want = self.lib.sdvar_vae_tensor_count(C.byref(d))
        if want != len(self.tensors):
            raise SdvarError(f"VQVAE decoder layout mismatch: the library expects {want} tensors, the state_dict walk found {len(self.tensors)}")
        self.h = C.c_void_p()
        with torch.cuda.device(self.device):
            _check(self.lib.sdvar_vae_create(C.byref(d), C.byref(self.h)))
            arr = (_P * len(self.tensors))(*[t.data_ptr() for t in self.tensors])
            _check(self.lib.sdvar_vae_bind(self.h, arr, len(self.tensors), _stream()))

    @staticmethod
    def tensor_names(vae_sd, ch_mult: Sequence[int] = (1, 1, 2, 2, 4), num_res_blocks: int = 2):
        """Module prefixes (each contributes .weight then .bias) in the order sdvar_vae_bind consumes them (include/sdvar_hip.h)."""
        names = ["post_quant_conv", "decoder.conv_in"]
        res = lambda p, sc: [p + ".norm1", p + ".conv1", p + ".norm2", p + ".conv2"] + ([p + ".nin_shortcut"] if sc else [])
        att = lambda p: [p + ".norm", p + ".qkv", p + ".proj_out"]
        names += res("decoder.mid.block_1", False) + att("decoder.mid.attn_1") + res("decoder.mid.block_2", False)
        for lv in reversed(range(len(ch_mult))):
            for i in range(num_res_blocks + 1):
                p = f"decoder.up.{lv}.block.{i}"
                names += res(p, p + ".nin_shortcut.weight" in vae_sd)
                if lv == len(ch_mult) - 1:
                    names += att(f"decoder.up.{lv}.attn.{i}")
            if lv != 0:
                names.append(f"decoder.up.{lv}.upsample.conv")
        return names + ["decoder.norm_out", "decoder.conv_out"]

    def decode(self, f_hat: torch.Tensor, out: Optional[torch.Tensor] = None, clamp: bool = True) -> torch.Tensor:
        """f_hat (B, Cvae, h, w) fp32 on the device -> image (B, 3, H, W) in [-1, 1]; runs on torch's current stream.  clamp=False: the unclamped
        image of VQVAE.forward (vqvae.py:59, sdvar_vae_decode_raw)."""
        B = f_hat.shape[0]
        if f_hat.dtype != torch.float32 or not f_hat.is_contiguous() or f_hat.device != self.device:
            f_hat = f_hat.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(f_hat.shape[1:]) != (self.z, self.latent_hw, self.latent_hw) or B > self.max_batch:
            raise SdvarError(f"decode: f_hat {tuple(f_hat.shape)} does not fit (max_batch {self.max_batch}, {self.z} x {self.latent_hw}^2)")
        if out is None:
            out = torch.empty(B, 3, self.out_hw, self.out_hw, device=self.device, dtype=torch.float32)
        _check((self.lib.sdvar_vae_decode if clamp else self.lib.sdvar_vae_decode_raw)(self.h, _ptr(f_hat), B, _ptr(out), _stream()))
        return out

    def decode_raw(self, f_hat: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self.decode(f_hat, out, clamp=False)

    def close(self):
        if self.h:
            self.lib.sdvar_vae_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VaeEncCtx:
    """sdvar_vae_enc_t from the VQVAE state_dict: f = quant_conv(encoder(img)) (vqvae.py:66) as hand-written HIP (csrc/conv.hip, csrc/vae.hip)."""

    def __init__(self, vae_sd: Dict[str, torch.Tensor], max_batch: int, device, latent_hw: int = 16, ch: Optional[int] = None,
                 ch_mult: Sequence[int] = (1, 1, 2, 2, 4), num_res_blocks: int = 2, conv_mode: Optional[str] = None):
        self.conv_mode = resolve_conv_mode(conv_mode, encoder=True)          # as VaeCtx, without the decoder-only "f16"
        self.lib = load_library()
        self.device = torch.device(device)
        if "encoder.conv_in.weight" not in vae_sd:
            raise SdvarError("VaeEncCtx: the state_dict holds no encoder (a VQVAE built with with_encoder=False)")
        z = vae_sd["quant_conv.weight"].shape[0]
        ch = ch if ch is not None else vae_sd["encoder.conv_in.weight"].shape[0]
        d = _VaeDesc()
        d.ch, d.z_channels, d.n_mult, d.num_res_blocks, d.max_batch, d.latent_hw = ch, z, len(ch_mult), num_res_blocks, max_batch, latent_hw
        d.plane_format = _CONV_PLANE_FORMAT[self.conv_mode]
        for i, m in enumerate(ch_mult):
            d.ch_mult[i] = m
        self.desc, self.max_batch, self.latent_hw, self.z = d, max_batch, latent_hw, z
        self.img_hw = latent_hw << (len(ch_mult) - 1)
        names = self.tensor_names(vae_sd, ch_mult, num_res_blocks)
        self.tensors = []                                   # keeps the device copies alive: biases and GroupNorm affine stay borrowed
        for n in names:
            self.tensors += [_f32(vae_sd[n + ".weight"], self.device), _f32(vae_sd[n + ".bias"], self.device)]
        want = self.lib.sdvar_vae_enc_tensor_count(C.byref(d))
        if want != len(self.tensors):
            raise SdvarError(f"VQVAE encoder layout mismatch: the library expects {want} tensors, the state_dict walk found {len(self.tensors)}")
        self.h = C.c_void_p()
        with torch.cuda.device(self.device):
            _check(self.lib.sdvar_vae_enc_create(C.byref(d), C.byref(self.h)))
            arr = (_P * len(self.tensors))(*[t.data_ptr() for t in self.tensors])
            _check(self.lib.sdvar_vae_enc_bind(self.h, arr, len(self.tensors), _stream()))

    @staticmethod
    def tensor_names(vae_sd, ch_mult: Sequence[int] = (1, 1, 2, 2, 4), num_res_blocks: int = 2):
        """Module prefixes (each contributes .weight then .bias) in the order sdvar_vae_enc_bind consumes them (include/sdvar_hip.h)."""
        names = ["encoder.conv_in"]
        res = lambda p, sc: [p + ".norm1", p + ".conv1", p + ".norm2", p + ".conv2"] + ([p + ".nin_shortcut"] if sc else [])
        att = lambda p: [p + ".norm", p + ".qkv", p + ".proj_out"]
        for lv in range(len(ch_mult)):
            for i in range(num_res_blocks):
                p = f"encoder.down.{lv}.block.{i}"
                names += res(p, p + ".nin_shortcut.weight" in vae_sd)
                if lv == len(ch_mult) - 1:
                    names += att(f"encoder.down.{lv}.attn.{i}")
            if lv != len(ch_mult) - 1:
                names.append(f"encoder.down.{lv}.downsample.conv")
        names += res("encoder.mid.block_1", False) + att("encoder.mid.attn_1") + res("encoder.mid.block_2", False)
        return names + ["encoder.norm_out", "encoder.conv_out", "quant_conv"]

    def encode(self, img: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """img (B, 3, H, W) fp32 on the device -> f (B, Cvae, H/16, W/16); runs on torch's current stream."""
        B = img.shape[0]
        if img.dtype != torch.float32 or not img.is_contiguous() or img.device != self.device:
            img = img.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(img.shape[1:]) != (3, self.img_hw, self.img_hw) or B > self.max_batch:
            raise SdvarError(f"encode: img {tuple(img.shape)} does not fit (max_batch {self.max_batch}, 3 x {self.img_hw}^2)")
        if out is None:
            out = torch.empty(B, self.z, self.latent_hw, self.latent_hw, device=self.device, dtype=torch.float32)
        _check(self.lib.sdvar_vae_enc_encode(self.h, _ptr(img), B, _ptr(out), _stream()))
        return out

    def close(self):
        if self.h:
            self.lib.sdvar_vae_enc_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------------- per-image parameters
def _as_rows(name: str, v, kind):
    """A sampling argument as given: a python scalar stays one (-> `kind`); a sequence, numpy array or tensor becomes a list of `kind`."""
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().tolist() if v.dim() else v.item()
    elif isinstance(v, np.ndarray):
        v = v.tolist()
    if isinstance(v, (list, tuple)):
        return [kind(x) for x in v]
    try:
        return kind(v)
    except (TypeError, ValueError):
        raise SdvarError(f"{name}: expected a number or a sequence of numbers, got {type(v).__name__}") from None


def scalar_arg(who: str, **named):
    """The paths without per-image tables: a sequence where they take one number is refused by name, before anything is launched."""
    for name, v in named.items():
        if isinstance(v, Noise):
            if v.per_image:
                raise SdvarError(f"{who}: per-image seeds / image offsets are not supported on this path (plain_ar and spec_decode take them)")
        elif isinstance(v, (list, tuple, np.ndarray)) or (isinstance(v, torch.Tensor) and v.dim() > 0):
            raise SdvarError(f"{who}: {name} must be one number on this path, not a sequence (plain_ar and spec_decode take per-image values)")


class _RowImage(C.Structure):                  # sdvar_row_image of include/sdvar_hip.h
    _fields_ = [("top_k", C.c_int32), ("use_top_p", C.c_int32), ("top_p_thr", C.c_float), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32),
                ("index", C.c_uint32), ("reserved", C.c_uint32 * 2)]


ROW_IMAGE_DTYPE = np.dtype([("top_k", "<i4"), ("use_top_p", "<i4"), ("top_p_thr", "<f4"), ("seed_lo", "<u4"), ("seed_hi", "<u4"), ("index", "<u4"),
                            ("reserved", "<u4", (2,))])
assert ROW_IMAGE_DTYPE.itemsize == C.sizeof(_RowImage) == 32


class RowParams:
    """Per-image (cfg_b, top_k_b, top_p_b, seed_b, index_b) of one sampler call as the tables of include/sdvar_hip.h: `fac` (S, B, 2) float32
    = float32(1 + t), float32(t) with t = cfg_b * s / (S - 1) (Ladder.cfg_t; the roundings the scalar entry points apply to their t), and `img`, one
    sdvar_row_image per image.  Built on the host with numpy, uploaded ONCE (`dev`: one buffer, the factor table then the image table); the kernels
    read the row of their image, nothing is copied per stage or per round."""

    def __init__(self, B: int, lad: Ladder, cfg, top_k, top_p, seeds: Sequence[int], index: Sequence[int], device=None):
        col = {}
        for name, v, kind in (("cfg", cfg, float), ("top_k", top_k, int), ("top_p", top_p, float)):
            v = _as_rows(name, v, kind)
            if isinstance(v, list) and len(v) != B:
                raise SdvarError(f"{name}: {len(v)} entries for a batch of {B} images")
            col[name] = v if isinstance(v, list) else [v] * B
        if len(seeds) != B or len(index) != B:
            raise SdvarError(f"seed / image_offset: {len(seeds)} / {len(index)} entries for a batch of {B} images")
        if min(col["top_k"]) < 0:
            raise SdvarError(f"top_k: {col['top_k']}: a negative top_k (0 = off)")
        self.B, self.S = B, lad.S
        self.cfg, self.top_k, self.top_p = col["cfg"], col["top_k"], col["top_p"]
        self.seeds, self.index = [int(x) & (2**64 - 1) for x in seeds], [int(x) & 0xFFFFFFFF for x in index]
        self.fac = np.empty((lad.S, B, 2), np.float32)
        for s in range(lad.S):
            for b in range(B):
                t = lad.cfg_t(self.cfg[b], s)
                self.fac[s, b, 0], self.fac[s, b, 1] = np.float32(1.0 + t), np.float32(t)
        self.img = np.zeros(B, ROW_IMAGE_DTYPE)
        self.img["top_k"] = self.top_k
        self.img["use_top_p"] = [1 if p > 0.0 else 0 for p in self.top_p]
        self.img["top_p_thr"] = [np.float32(1.0 - p) for p in self.top_p]
        self.img["seed_lo"] = [x & 0xFFFFFFFF for x in self.seeds]
        self.img["seed_hi"] = [x >> 32 for x in self.seeds]
        self.img["index"] = self.index
        self.dev = None
        self.upload(device)

    def upload(self, device):
        """One device buffer: the factor table, then the image table.  The one host-to-device copy of a sampler call."""
        self.img_off = self.fac.nbytes
        if device is not None:
            host = np.concatenate([np.ascontiguousarray(self.fac).reshape(-1).view(np.uint8), np.ascontiguousarray(self.img).view(np.uint8).reshape(-1)])
            self.dev = torch.from_numpy(host).to(device)

    @classmethod
    def from_tables(cls, fac: np.ndarray, img: np.ndarray, device=None) -> "RowParams":
        """Tables built by the caller: fac (n_stages, B, 2) float32 holding float32(1 + t), float32(t) of any t, img (B,) ROW_IMAGE_DTYPE."""
        self = cls.__new__(cls)
        self.fac, self.img = np.ascontiguousarray(fac, np.float32), np.ascontiguousarray(img, ROW_IMAGE_DTYPE)
        self.S, self.B = self.fac.shape[0], self.fac.shape[1]
        if self.fac.ndim != 3 or self.fac.shape[2] != 2 or self.img.shape != (self.B,):
            raise SdvarError(f"RowParams.from_tables: fac {self.fac.shape} / img {self.img.shape}: expected (n_stages, B, 2) and (B,)")
        if self.B and int(self.img["top_k"].min()) < 0:
            raise SdvarError("top_k: a negative top_k (0 = off)")
        self.dev = None
        self.upload(device)
        return self

    @staticmethod
    def build(B: int, lad: Ladder, cfg, top_k, top_p, noise: "Noise", device=None) -> Optional["RowParams"]:
        """None when every argument is a scalar: the scalar entry points then run, with the launches they always had."""
        if not noise.per_image and all(not isinstance(_as_rows(n, v, k), list) for n, v, k in (("cfg", cfg, float), ("top_k", top_k, int), ("top_p", top_p, float))):
            return None
        seeds, index = noise.rows(B)
        return RowParams(B, lad, cfg, top_k, top_p, seeds, index, device)

    def fac_ptr(self, s: int):
        return C.c_void_p(self.dev.data_ptr() + 8 * self.B * s)

    def img_ptr(self):
        return C.c_void_p(self.dev.data_ptr() + self.img_off)

    def img_host_ptr(self):
        return C.c_void_p(self.img.ctypes.data)


# ------------------------------------------------------------------------------------------------------- noise
class Noise:
    """Where the Exp(1) draw noise q comes from (sdvar_amd/noise.py explains why it is explicit).
    kind = 'device': Philox generated inside the sampler kernel (fast path, no host traffic);
           'host'  : the same Philox stream computed on the host in float64 and uploaded (portable parity mode);
           'torch' : torch.empty(B*l, V).exponential_(generator=cpu_gen), the reference's own CPU stream on this host;
           callable: fn(draw, B, l, V) -> float32 array/tensor (B*l, V) or (B, l, V).
    `seed` and `image_offset` may be sequences (one entry per image of the call) for 'device' and 'host': image b then draws the Philox stream with
    key seed[b] and image counter image_offset[b] - what a one-image call with that seed and offset draws.  With a sequence of seeds the counter defaults
    to 0 for every image; with a scalar seed it stays image_offset + b.  'torch' and callable noise have one stream: a sequence raises SdvarError."""

    def __init__(self, kind="device", seed=0, image_offset=0, fn: Optional[Callable] = None, generator: Optional[torch.Generator] = None):
        seed, image_offset = _as_rows("seed", seed, int), _as_rows("image_offset", image_offset, int)
        self.per_image = not (isinstance(seed, int) and isinstance(image_offset, int))
        if self.per_image and kind not in ("device", "host"):
            raise SdvarError(f"Noise: a sequence of seeds / image offsets needs the Philox stream (kind 'device' or 'host'), not {kind!r} noise: it has one generator")
        self.kind, self.seed, self.image_offset, self.fn, self.gen = kind, seed, image_offset, fn, generator
        if kind == "torch" and generator is None:
            self.gen = torch.Generator(device="cpu"); self.gen.manual_seed(self.seed)

    def rows(self, B: int):
        """(seed_b, index_b) of the B images of a call: the Philox key and image counter of each."""
        sd, io = self.seed, self.image_offset
        for name, v in (("seed", sd), ("image_offset", io)):
            if not isinstance(v, int) and len(v) != B:
                raise SdvarError(f"{name}: {len(v)} entries for a batch of {B} images")
        if isinstance(sd, int):
            idx = [io + b for b in range(B)] if isinstance(io, int) else list(io)
            return [sd] * B, idx
        return list(sd), ([io] * B if isinstance(io, int) else list(io))

    def tensor(self, draw: int, B: int, l: int, V: int, device) -> Optional[torch.Tensor]:
        if self.kind == "device":
            return None
        if self.kind == "host" and self.per_image:
            q = torch.from_numpy(np.concatenate([exponential_noise(s_, draw, 1, l, V, i_) for s_, i_ in zip(*self.rows(B))], 0))
        elif self.kind == "host":
            q = torch.from_numpy(exponential_noise(self.seed, draw, B, l, V, self.image_offset))
        elif self.kind == "torch":
            q = torch.empty(B * l, V).exponential_(1, generator=self.gen)
        else:
            q = self.fn(draw, B, l, V)
            q = torch.from_numpy(np.ascontiguousarray(q)) if isinstance(q, np.ndarray) else q
        return q.reshape(B * l, V).to(device=device, dtype=torch.float32, non_blocking=False).contiguous()


def cfg_sample(logits: torch.Tensor, B: int, l: int, V: int, t: float, top_k: int, top_p: float, q: Optional[torch.Tensor], seed: int, draw: int,
               image_offset: int, ids_out: torch.Tensor, ids_off: int, ids_stride: int, dbg_masked: Optional[torch.Tensor] = None):
    lib = load_library()
    _check(lib.sdvar_cfg_sample(_ptr(logits), B, l, V, float(t), int(top_k), float(top_p), _ptr(q) if q is not None else None, seed & (2**64 - 1),
                                draw, image_offset, C.c_void_p(ids_out.data_ptr() + 8 * ids_off), ids_stride,
                                _ptr(dbg_masked) if dbg_masked is not None else None, _stream()))


def cfg_sample_rows(logits: torch.Tensor, B: int, l: int, V: int, rows: RowParams, si: int, q: Optional[torch.Tensor], draw: int, ids_out: torch.Tensor,
                    ids_off: int, ids_stride: int, dbg_masked: Optional[torch.Tensor] = None):
    """cfg_sample with image b's own parameters: stage `si`'s factor slice and the image table of `rows` (device tables, uploaded when it was built)."""
    _check(load_library().sdvar_cfg_sample_rows(_ptr(logits), B, l, V, rows.fac_ptr(si), rows.img_ptr(), rows.img_host_ptr(), rows.B,
                                                _ptr(q) if q is not None else None, draw, C.c_void_p(ids_out.data_ptr() + 8 * ids_off), ids_stride,
                                                _ptr(dbg_masked) if dbg_masked is not None else None, _stream()))


# ---- masked sampling (include/sdvar_hip.h "masked sampling"): forced tokens, the pixel mask -> token table, the pixel composite
def _edit_tensor(who: str, name: str, t, dtype, numel: int, dev, align: int = 1, exact: bool = True) -> None:
    """One dense operand of the masked-sampling calls, checked BEFORE its pointer is taken (as _xent_tensor / _embed_tensor do); exact=False: `numel` is the
    least the kernel touches (a table or an output addressed at a stride inside a larger buffer)."""
    if not isinstance(t, torch.Tensor):
        raise SdvarError(f"{who}: {name} is not a tensor")
    if not t.is_cuda or (dev is not None and t.device != dev):
        raise SdvarError(f"{who}: {name} is on {t.device}; every operand must be on one GPU")
    if t.dtype != dtype:
        raise SdvarError(f"{who}: {name} is {t.dtype}, expected {dtype}")
    if (t.numel() != numel) if exact else (t.numel() < numel):
        raise SdvarError(f"{who}: {name} has {t.numel()} elements, expected {'' if exact else 'at least '}{numel}")
    if not t.is_contiguous():
        raise SdvarError(f"{who}: {name} with strides {tuple(t.stride())} is not dense (pass {name}.contiguous())")
    if t.data_ptr() % align:
        raise SdvarError(f"{who}: {name} is not {align}-byte aligned (pass {name}.clone())")


def _forced_operands(who: str, logits, B: int, l: int, V: int, q, ids_out, ids_off: int, ids_stride: int, dbg_masked, gen, force_ids, force_off: int,
                     force_stride: int):
    """Everything the forced sampler kernels assume about their operands; returns the three offset pointers (ids, gen, force_ids)."""
    if min(B, l) < 1 or V < 4 or V % 4 or V > 4096:
        raise SdvarError(f"{who}: B = {B}, l = {l}, V = {V}: B and l must be positive and V a multiple of 4 up to 4096")
    if min(ids_off, force_off) < 0 or ids_stride < ids_off + l or force_stride < force_off + l:
        raise SdvarError(f"{who}: {l} tokens at offset {ids_off} / {force_off} do not fit rows of stride {ids_stride} (ids) / {force_stride} (gen, force_ids)")
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda:
        raise SdvarError(f"{who}: logits must be a GPU tensor")
    dev = logits.device
    _edit_tensor(who, "logits", logits, torch.float32, 2 * B * l * V, dev, 16, exact=False)
    if q is not None:
        _edit_tensor(who, "q", q, torch.float32, B * l * V, dev, 16)
    if dbg_masked is not None:
        _edit_tensor(who, "dbg_masked", dbg_masked, torch.float32, B * l * V, dev, 4, exact=False)
    _edit_tensor(who, "ids_out", ids_out, torch.int64, (B - 1) * ids_stride + ids_off + l, dev, 8, exact=False)
    _edit_tensor(who, "gen", gen, torch.uint8, (B - 1) * force_stride + force_off + l, dev, 1, exact=False)
    _edit_tensor(who, "force_ids", force_ids, torch.int64, (B - 1) * force_stride + force_off + l, dev, 8, exact=False)
    return (C.c_void_p(ids_out.data_ptr() + 8 * ids_off), C.c_void_p(gen.data_ptr() + force_off), C.c_void_p(force_ids.data_ptr() + 8 * force_off))


def cfg_sample_forced(logits: torch.Tensor, B: int, l: int, V: int, t: float, top_k: int, top_p: float, q: Optional[torch.Tensor], seed: int, draw: int,
                      image_offset: int, ids_out: torch.Tensor, ids_off: int, ids_stride: int, gen: torch.Tensor, force_ids: torch.Tensor, force_off: int,
                      force_stride: int, dbg_masked: Optional[torch.Tensor] = None):
    """sdvar_cfg_sample_forced: cfg_sample, but token (b, tok) with gen[b * force_stride + force_off + tok] == 0 is not sampled: its id is
    force_ids[b * force_stride + force_off + tok] (clamped into [0, V)) and its row of dbg_masked is left alone.  gen uint8, force_ids int64, dense device tensors."""
    who = "cfg_sample_forced"
    p_ids, p_gen, p_force = _forced_operands(who, logits, B, l, V, q, ids_out, ids_off, ids_stride, dbg_masked, gen, force_ids, force_off, force_stride)
    lib = load_library()
    with _on_device(logits.device):
        _check(lib.sdvar_cfg_sample_forced(_ptr(logits), B, l, V, float(t), int(top_k), float(top_p), _ptr(q), seed & (2**64 - 1), draw, image_offset, p_ids, ids_stride,
                                           _ptr(dbg_masked), p_gen, p_force, force_stride, _stream()))


def cfg_sample_rows_forced(logits: torch.Tensor, B: int, l: int, V: int, rows: RowParams, si: int, q: Optional[torch.Tensor], draw: int, ids_out: torch.Tensor,
                           ids_off: int, ids_stride: int, gen: torch.Tensor, force_ids: torch.Tensor, force_off: int, force_stride: int,
                           dbg_masked: Optional[torch.Tensor] = None):
    """sdvar_cfg_sample_rows_forced: cfg_sample_rows with the forced tokens of cfg_sample_forced."""
    who = "cfg_sample_rows_forced"
    p_ids, p_gen, p_force = _forced_operands(who, logits, B, l, V, q, ids_out, ids_off, ids_stride, dbg_masked, gen, force_ids, force_off, force_stride)
    if not isinstance(rows, RowParams) or rows.dev is None or rows.dev.device != logits.device or rows.B != B or not 0 <= si < rows.S:
        raise SdvarError(f"{who}: rows must be a RowParams uploaded to the logits' GPU for {B} images, and si = {si} one of its stages")
    lib = load_library()
    with _on_device(logits.device):
        _check(lib.sdvar_cfg_sample_rows_forced(_ptr(logits), B, l, V, rows.fac_ptr(si), rows.img_ptr(), rows.img_host_ptr(), rows.B, _ptr(q), draw, p_ids, ids_stride,
                                                _ptr(dbg_masked), p_gen, p_force, force_stride, _stream()))


def mask_tokens(mask_px: torch.Tensor, patch_nums: Sequence[int], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sdvar_mask_tokens: mask_px (B, H, H) uint8 on the GPU (non-zero = regenerate the pixel) -> gen (B, L) uint8, stage s at columns [begin(s), begin(s) + pn_s^2).
    Token (i, j) of a stage with side pn owns pixel rows [floor(i H / pn), ceil((i + 1) H / pn)) and the same span of columns; it is sampled (1) iff
    2 * (set pixels in its window) >= (pixels in its window).  Integer and exact; no host synchronisation."""
    who = "mask_tokens"
    pns = [int(p) for p in patch_nums]
    if not isinstance(mask_px, torch.Tensor) or mask_px.dim() != 3 or mask_px.shape[1] != mask_px.shape[2] or mask_px.shape[0] < 1 or mask_px.shape[1] < 1:
        raise SdvarError(f"{who}: mask_px must be a (B, H, H) uint8 GPU tensor, got {tuple(mask_px.shape) if isinstance(mask_px, torch.Tensor) else type(mask_px).__name__}")
    B, H = int(mask_px.shape[0]), int(mask_px.shape[1])
    if not 1 <= len(pns) <= MAX_STAGES or min(pns) < 1 or max(pns) > H:
        raise SdvarError(f"{who}: patch_nums {tuple(pns)}: 1 to {MAX_STAGES} stages with sides in [1, H = {H}]")
    _edit_tensor(who, "mask_px", mask_px, torch.uint8, B * H * H, None)
    L = sum(p * p for p in pns)
    if out is None:
        out = torch.empty(B, L, dtype=torch.uint8, device=mask_px.device)
    else:
        _edit_tensor(who, "out", out, torch.uint8, B * L, mask_px.device)
    lib = load_library()
    with _on_device(mask_px.device):
        _check(lib.sdvar_mask_tokens(_ptr(mask_px), B, H, len(pns), (_I * len(pns))(*pns), _ptr(out), _stream()))
    return out


def img_composite(gen_img: torch.Tensor, orig: torch.Tensor, mask_px: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sdvar_img_composite: out = mask_px ? (gen_img + 1) * 0.5 : (orig + 1) * 0.5 with the two roundings of torch's x.add(1).mul(0.5).  gen_img, orig (B, C, H, W) fp32,
    mask_px (B, H, W) uint8, all dense on one GPU; out may be gen_img (or orig) itself.  16-byte accesses when the pointers allow, scalar ones otherwise."""
    who = "img_composite"
    if not isinstance(gen_img, torch.Tensor) or gen_img.dim() != 4 or gen_img.numel() == 0:
        raise SdvarError(f"{who}: gen_img must be a non-empty (B, C, H, W) fp32 GPU tensor")
    B, Cc, H, W = (int(x) for x in gen_img.shape)
    _edit_tensor(who, "gen_img", gen_img, torch.float32, B * Cc * H * W, None, 4)
    dev = gen_img.device
    for name, t, shape, dtype in (("orig", orig, (B, Cc, H, W), torch.float32), ("mask_px", mask_px, (B, H, W), torch.uint8)):
        if isinstance(t, torch.Tensor) and tuple(t.shape) != shape:
            raise SdvarError(f"{who}: {name} has shape {tuple(t.shape)}, expected {shape}")
        _edit_tensor(who, name, t, dtype, int(np.prod(shape)), dev, 4 if dtype == torch.float32 else 1)
    if out is None:
        out = torch.empty_like(gen_img)
    else:
        if isinstance(out, torch.Tensor) and tuple(out.shape) != (B, Cc, H, W):
            raise SdvarError(f"{who}: out has shape {tuple(out.shape)}, expected {(B, Cc, H, W)}")
        _edit_tensor(who, "out", out, torch.float32, B * Cc * H * W, dev, 4)
    lib = load_library()
    with _on_device(dev):
        _check(lib.sdvar_img_composite(_ptr(gen_img), _ptr(orig), _ptr(mask_px), B, Cc, H * W, _ptr(out), _stream()))
    return out


def handoff_mask(lad: Ladder, entry_num: int, sd_mask: int) -> torch.Tensor:
    """The (pindex, pindex) additive mask of SDVAR.sdvar_autoregressive_infer_cfg_sd_test3 for sd_mask 1, 2, 4, 5 (var.py:557-578, 777-798), pindex =
    tokens of stages 0 .. entry_num.  attn_bias_for_sdmasking: token i sees itself and every token of EARLIER stages (not its own stage's other
    tokens); attn_bias_for_block: token i sees exactly its own stage.  Masks 2 and 5 open the entry stage's rows completely."""
    p, s0 = lad.cum[entry_num], lad.begin(entry_num)
    blk = torch.cat([torch.full((n,), i) for i, n in enumerate(lad.lens)])[:p]
    bi, bj = blk.view(p, 1), blk.view(1, p)
    if sd_mask in (1, 2):
        ok = (bj < bi) | torch.eye(p, dtype=torch.bool)
    else:
        ok = bi == bj
    m = torch.where(ok, 0.0, float("-inf")).to(torch.float32)
    if sd_mask in (2, 5):
        m[s0:p, :] = 0.0
    return m.contiguous()


GUMBEL_DRAW = 0x40000000      # Philox `draw` of a stage's gumbel noise = its sampler draw | GUMBEL_DRAW (the reference draws it right after the multinomial)


@dataclass
class MatchRule:
    """Token rule of the acceptance scan.  'top1' is basic_token_matching (var.py:1199-1203, what the reference's advanced_token_matching
    stub falls back to); 'topk' / 'kl' / token_level are the rules its docstring sketches (var.py:1229-1243), reference-unpinned:
      topk        draft id among the target's `top_k` best CFG logits
      kl          KL(softmax target || softmax draft) of the token's two CFG distributions <= kl_thr
      token_level the first stage that fails the batch threshold is not re-drafted: its matching tokens are kept, the others take the
                  target's argmax, and the stage is committed (the target contributes tokens; no gamma decay, no forced accepts)."""
    rule: str = "top1"
    top_k: int = 1
    kl_thr: float = 0.0
    token_level: bool = False

    @property
    def code(self) -> int:
        return {"top1": 0, "topk": 1, "kl": 2}[self.rule]

    @property
    def basic(self) -> bool:
        return self.rule == "top1" and not self.token_level


def verify_accept(logits: torch.Tensor, B: int, lens: Sequence[int], V: int, ts: Sequence[float], ids: torch.Tensor, ids_off: int, ids_stride: int,
                  thr: float, counts: torch.Tensor, argmax_out: Optional[torch.Tensor] = None, rule: Optional[MatchRule] = None,
                  draft_logits: Optional[torch.Tensor] = None, match_out: Optional[torch.Tensor] = None, corrected_out: Optional[torch.Tensor] = None,
                  rows: Optional[RowParams] = None, s0: int = 0, gen: Optional[torch.Tensor] = None, gen_off: int = 0, gen_stride: int = 0):
    """`rows`: the CFG factors of (stage s0 + j, image b) come from its factor table and `ts` is ignored.
    `gen` (uint8, dense, on the logits' GPU): the forced entry points - token (b, i) of the chunk with gen[b * gen_stride + gen_off + i] == 0 is a forced token: it is
    left out of counts[j], counts[17 + j] counts the sampled tokens only, a stage without any is accepted, and the optional outputs hold match 1 / corrected = the
    draft id / argmax -1 there (include/sdvar_hip.h)."""
    lib = load_library()
    n = len(lens)
    o = lambda t: _ptr(t) if t is not None else None
    r = rule or MatchRule()
    if gen is not None:
        who, lsum = "verify_accept", int(sum(lens))
        if B < 1 or lsum < 1 or gen_off < 0 or gen_stride < gen_off + lsum or ids_off < 0 or ids_stride < ids_off + lsum:
            raise SdvarError(f"{who}: {lsum} tokens at offset {ids_off} / {gen_off} do not fit rows of stride {ids_stride} (ids) / {gen_stride} (gen)")
        _edit_tensor(who, "gen", gen, torch.uint8, (B - 1) * gen_stride + gen_off + lsum, logits.device, 1, exact=False)
        _edit_tensor(who, "ids", ids, torch.int64, (B - 1) * ids_stride + ids_off + lsum, logits.device, 8, exact=False)
        p_ids, p_gen = C.c_void_p(ids.data_ptr() + 8 * ids_off), C.c_void_p(gen.data_ptr() + gen_off)
        if rows is not None:
            _check(lib.sdvar_verify_accept_rows_forced(_ptr(logits), B, lsum, V, n, (_I * n)(*lens), rows.fac_ptr(s0), rows.B, p_ids, ids_stride, float(thr), r.code,
                                                       int(r.top_k), float(r.kl_thr), o(draft_logits), _ptr(counts), o(argmax_out), o(match_out), o(corrected_out), p_gen,
                                                       gen_stride, _stream()))
        else:
            _check(lib.sdvar_verify_accept_forced(_ptr(logits), B, lsum, V, n, (_I * n)(*lens), (_D * n)(*[float(t) for t in ts]), p_ids, ids_stride, float(thr), r.code,
                                                  int(r.top_k), float(r.kl_thr), o(draft_logits), _ptr(counts), o(argmax_out), o(match_out), o(corrected_out), p_gen,
                                                  gen_stride, _stream()))
        return
    if rows is not None:
        _check(lib.sdvar_verify_accept_rows(_ptr(logits), B, int(sum(lens)), V, n, (_I * n)(*lens), rows.fac_ptr(s0), rows.B,
                                            C.c_void_p(ids.data_ptr() + 8 * ids_off), ids_stride, float(thr), r.code, int(r.top_k), float(r.kl_thr),
                                            o(draft_logits), _ptr(counts), o(argmax_out), o(match_out), o(corrected_out), _stream()))
        return
    _check(lib.sdvar_verify_accept_ex(_ptr(logits), B, int(sum(lens)), V, n, (_I * n)(*lens), (_D * n)(*[float(t) for t in ts]),
                                      C.c_void_p(ids.data_ptr() + 8 * ids_off), ids_stride, float(thr), r.code, int(r.top_k), float(r.kl_thr),
                                      o(draft_logits), _ptr(counts), o(argmax_out), o(match_out), o(corrected_out), _stream()))


def cfg_combine(logits: torch.Tensor, B: int, lens: Sequence[int], V: int, ts: Sequence[float], rows: Optional[RowParams] = None, s0: int = 0) -> List[torch.Tensor]:
    """var.py:1062-1067 on a verified chunk's raw logits (2B, sum(lens), V): the per-stage CFG logits (B, l_j, V), one kernel (csrc/sampler.hip).
    `rows`: per-image factors of stages s0 .. from its table (`ts` ignored)."""
    n, lsum = len(lens), int(sum(lens))
    out = torch.empty(B, lsum, V, dtype=torch.float32, device=logits.device)
    if rows is not None:
        _check(load_library().sdvar_cfg_combine_rows(_ptr(logits), B, lsum, V, n, (_I * n)(*lens), rows.fac_ptr(s0), rows.B, _ptr(out), _stream()))
        return list(out.split([int(x) for x in lens], dim=1))
    _check(load_library().sdvar_cfg_combine(_ptr(logits), B, lsum, V, n, (_I * n)(*lens), (_D * n)(*[float(t) for t in ts]), _ptr(out), _stream()))
    return list(out.split([int(x) for x in lens], dim=1))


def xent_stats(logits: torch.Tensor, targets: torch.Tensor, tail: int, sums: torch.Tensor, accumulate: bool = False, nll_out: Optional[torch.Tensor] = None,
               argmax_out: Optional[torch.Tensor] = None):
    """sdvar_xent_stats: logits (B, L, V) fp32, targets (B, L) int64 -> sums (4,) float64 {sum nll, sum tail nll, #correct, #tail correct} over the
    last `tail` tokens of each image (VARTrainer.eval_ep, trainer.py:66-75); optional per-token nll (B, L) fp32 and argmax (B, L) int64."""
    B, L, V = logits.shape
    assert logits.dtype == torch.float32 and targets.dtype == torch.int64 and tuple(targets.shape) == (B, L)
    assert sums.dtype == torch.float64 and sums.numel() == 4
    assert nll_out is None or (nll_out.dtype == torch.float32 and nll_out.numel() == B * L)
    assert argmax_out is None or (argmax_out.dtype == torch.int64 and argmax_out.numel() == B * L)
    load_library()
    _check(_lib.sdvar_xent_stats(_ptr(logits), _ptr(targets), B, L, V, tail, _ptr(nll_out), _ptr(argmax_out), _ptr(sums), int(bool(accumulate)), _stream()))


XENT_REDUCTIONS = ("none", "mean", "sum")          # sdvar_xent_train_bwd's reduction codes
XENT_NT_STORES = False          # dlogits with non-temporal stores: measured within 2 % of plain stores for the kernel alone, and 11 us slower once a consumer reads the gradient back at B <= 16


def _on_device(dev):
    """The launch context of a tensor's device: nothing to enter when it is the current one (the usual case; the guard costs more host time than the call)."""
    return contextlib.nullcontext() if dev.index == torch.cuda.current_device() else torch.cuda.device(dev)


def _xent_tensor(who: str, name: str, t, dtype, numel: int, dev, align: int) -> None:
    """One dense operand of the xent_train calls: everything the kernel assumes about it, checked BEFORE its pointer is taken."""
    if not isinstance(t, torch.Tensor):
        raise SdvarError(f"{who}: {name} is not a tensor")
    if not t.is_cuda or (dev is not None and t.device != dev):
        raise SdvarError(f"{who}: {name} is on {t.device}; every operand must be on the logits' GPU")
    if t.dtype != dtype:
        raise SdvarError(f"{who}: {name} is {t.dtype}, expected {dtype}")
    if t.numel() != numel:
        raise SdvarError(f"{who}: {name} has {t.numel()} elements, expected {numel}")
    if not t.is_contiguous():
        raise SdvarError(f"{who}: {name} with strides {tuple(t.stride())} is not dense (pass {name}.contiguous())")
    if t.data_ptr() % align:
        raise SdvarError(f"{who}: {name} is not {align}-byte aligned (pass {name}.clone())")


def _xent_logits(who: str, logits, targets):
    """(rows, V, ld) of the (rows, V) fp32 logits, read in place at row stride ld, and the check of targets (rows,) int64."""
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda:
        raise SdvarError(f"{who}: logits must be a GPU tensor")
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise SdvarError(f"{who}: logits are {logits.dtype} with {logits.dim()} dims, expected a float32 (rows, V) tensor")
    rows, V = logits.shape
    if rows < 1 or rows > 0x7FFFFFFF or V < 4 or V % 4:
        raise SdvarError(f"{who}: logits of shape {(rows, V)}: rows must be in [1, 2^31 - 1] and V a positive multiple of 4")
    ld = V if rows == 1 else logits.stride(0)
    if logits.stride(1) != 1 or ld < V or ld % 4 or logits.data_ptr() % 16:
        raise SdvarError(f"{who}: logits with strides {tuple(logits.stride())} at address % 16 == {logits.data_ptr() % 16}: rows must have unit column stride, a row "
                         f"stride >= V that is a multiple of 4, and 16-byte alignment (pass logits.clone(memory_format=torch.contiguous_format))")
    _xent_tensor(who, "targets", targets, torch.int64, rows, logits.device, 8)
    return rows, V, ld


def xent_train_fwd(logits: torch.Tensor, targets: torch.Tensor, label_smoothing: float = 0.0, ignore_index: int = -100, reduction: str = "none",
                   want_lse: bool = True):
    """sdvar_xent_train_fwd: logits (rows, V) fp32 (row stride >= V, read in place), targets (rows,) int64 -> (loss (rows,) fp32, lse (rows,) fp32 or None,
    sums (2,) float64 {sum of loss over counted rows, counted rows} or None, reduced 0-dim fp32 or None).  reduction 'none' launches no reduction (sums and reduced
    None); 'mean' / 'sum' also leave the reduced value on the device.  No host synchronisation."""
    who = "xent_train_fwd"
    if reduction not in XENT_REDUCTIONS:
        raise SdvarError(f"{who}: reduction {reduction!r} is not one of {XENT_REDUCTIONS}")
    eps = float(label_smoothing)
    if not 0.0 <= eps <= 1.0:
        raise SdvarError(f"{who}: label_smoothing {label_smoothing} is outside [0, 1]")
    rows, V, ld = _xent_logits(who, logits, targets)
    dev = logits.device
    loss = torch.empty(rows, dtype=torch.float32, device=dev)
    lse = torch.empty(rows, dtype=torch.float32, device=dev) if want_lse else None
    part = sums = reduced = None
    if reduction != "none":
        part = torch.empty(2 * ((rows + 3) // 4), dtype=torch.float64, device=dev)
        sums = torch.empty(2, dtype=torch.float64, device=dev)
        reduced = torch.empty((), dtype=torch.float32, device=dev)
    lib = load_library()
    with _on_device(dev):
        _check(lib.sdvar_xent_train_fwd(C.c_void_p(logits.data_ptr()), ld, _ptr(targets), rows, V, eps, int(ignore_index), _ptr(loss), _ptr(lse), _ptr(part), _ptr(sums),
                                        _ptr(reduced), int(reduction == "mean"), _stream()))
    return loss, lse, sums, reduced


def xent_train_bwd(logits: torch.Tensor, targets: torch.Tensor, lse: torch.Tensor, grad: torch.Tensor, reduction: str = "none", sums: Optional[torch.Tensor] = None,
                   label_smoothing: float = 0.0, ignore_index: int = -100, nt_stores: Optional[bool] = None) -> torch.Tensor:
    """sdvar_xent_train_bwd: the gradient (rows, V) fp32, dense, of xent_train_fwd's loss with respect to the logits.  grad: the upstream gradient ON THE DEVICE, (rows,)
    fp32 for reduction 'none', one fp32 element for 'mean' / 'sum'; 'mean' also takes the forward's sums (the division by the counted rows happens in the kernel).
    nt_stores: non-temporal stores for the result (None: XENT_NT_STORES).  No host synchronisation."""
    who = "xent_train_bwd"
    if reduction not in XENT_REDUCTIONS:
        raise SdvarError(f"{who}: reduction {reduction!r} is not one of {XENT_REDUCTIONS}")
    eps = float(label_smoothing)
    if not 0.0 <= eps <= 1.0:
        raise SdvarError(f"{who}: label_smoothing {label_smoothing} is outside [0, 1]")
    rows, V, ld = _xent_logits(who, logits, targets)
    dev = logits.device
    _xent_tensor(who, "lse", lse, torch.float32, rows, dev, 4)
    _xent_tensor(who, "grad", grad, torch.float32, rows if reduction == "none" else 1, dev, 4)
    if reduction == "mean":
        _xent_tensor(who, "sums", sums, torch.float64, 2, dev, 8)
    dlogits = torch.empty(rows, V, dtype=torch.float32, device=dev)
    nt = XENT_NT_STORES if nt_stores is None else bool(nt_stores)
    lib = load_library()
    with _on_device(dev):
        _check(lib.sdvar_xent_train_bwd(C.c_void_p(logits.data_ptr()), ld, _ptr(targets), _ptr(lse), _ptr(grad), XENT_REDUCTIONS.index(reduction),
                                        _ptr(sums) if reduction == "mean" else None, rows, V, eps, int(ignore_index), _ptr(dlogits), int(nt), _stream()))
    return dlogits


OPTIM_CHUNK = 32768                    # SDVAR_OPTIM_CHUNK: elements of one tensor per workgroup of csrc/optim.hip
OPTIM_TENSORS_PER_LAUNCH = 48          # SDVAR_OPTIM_TENSORS_PER_LAUNCH: descriptors carried in the arguments of one launch


class _OptimTensor(C.Structure):
    """sdvar_optim_tensor_t"""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("step", C.c_void_p), ("numel", C.c_int64),
                ("lr", C.c_double), ("weight_decay", C.c_double)]


def optim_table(rows):
    """rows: (param, grad, exp_avg, exp_avg_sq, step addresses, numel, lr, weight_decay) per tensor -> the host array both optim calls take.  Built afresh for every
    step (gradient addresses change); the library copies what it needs into each launch, so the array may be dropped as soon as the calls return."""
    return (_OptimTensor * len(rows))(*rows)


def optim_ws_bytes(numels) -> int:
    """Bytes of the workspace of the two optim calls for tensors of these sizes: a 4-float record, 2 floats per tensor, one double per chunk."""
    return 16 + 8 * len(numels) + 8 * sum((int(n) + OPTIM_CHUNK - 1) // OPTIM_CHUNK for n in numels)


def optim_grad_stats(table, grad_scale: Optional[torch.Tensor], found_inf: Optional[torch.Tensor], max_norm: float, beta1: float, beta2: float, ws: torch.Tensor) -> None:
    """sdvar_optim_grad_stats on the current device and stream: fills ws (a uint8 / float32 device tensor of optim_ws_bytes) with the record {norm, coef, skip, gscale},
    advances the step counters by 1 - skip and leaves the per-tensor bias corrections.  grad_scale / found_inf: one-element float32 device tensors or None."""
    lib = load_library()
    _check(lib.sdvar_optim_grad_stats(table, len(table), _ptr(grad_scale), _ptr(found_inf), float(max_norm), float(beta1), float(beta2), _ptr(ws),
                                      ws.numel() * ws.element_size(), _stream()))


def optim_adamw_step(table, beta1: float, beta2: float, eps: float, ws: torch.Tensor) -> None:
    """sdvar_optim_adamw_step on the current device and stream, after optim_grad_stats with the same table and ws: one read of g, p, m, v and one write of p, m, v."""
    lib = load_library()
    _check(lib.sdvar_optim_adamw_step(table, len(table), float(beta1), float(beta2), float(eps), _ptr(ws), ws.numel() * ws.element_size(), _stream()))


TRAIN_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}          # dtype codes of csrc/adaln_train.hip
TRAIN_MAX_C = 3072
TRAIN_CHUNK = 32          # rows of one image per workgroup of the two backward kernels: fixes the workspace size and the order of the column sums


def _train_rows(who: str, name: str, t, dtypes, like: Optional[torch.Tensor] = None):
    """A (B, L, C) operand of the adaln / gate_add calls, read in place: a GPU tensor of one of `dtypes`, dense and 16-byte aligned, C % 4 == 0 in [4, TRAIN_MAX_C];
    with `like`, of its shape and on its GPU.  Returns (B, L, C)."""
    if not isinstance(t, torch.Tensor):
        raise SdvarError(f"{who}: {name} is not a tensor")
    if not t.is_cuda:
        raise SdvarError(f"{who}: {name} is a CPU tensor; the kernels run on the GPU and there is no CPU path (move it with .cuda())")
    if t.dtype not in dtypes:
        want = " or ".join(str(d) for d in dtypes)
        hint = f"pass {name}.float()" if torch.float32 in dtypes else f"pass a {want} tensor"
        raise SdvarError(f"{who}: {name} is {t.dtype}; it must be {want} ({hint})")
    if t.dim() != 3:
        raise SdvarError(f"{who}: {name} has shape {tuple(t.shape)}; expected (B, L, C)")
    B, L, Cc = t.shape
    if Cc < 4 or Cc > TRAIN_MAX_C or Cc % 4:
        raise SdvarError(f"{who}: C = {Cc} of {name} is outside the supported range: C must be a multiple of 4 in [4, {TRAIN_MAX_C}] (pad the channel dimension)")
    if B < 1 or L < 1 or B * L > 2 ** 29:
        raise SdvarError(f"{who}: {name} has shape {tuple(t.shape)}; B and L must be at least 1 and B * L at most 2^29 (split the batch)")
    if like is not None and (tuple(t.shape) != tuple(like.shape) or t.device != like.device):
        raise SdvarError(f"{who}: {name} has shape {tuple(t.shape)} on {t.device}; expected {tuple(like.shape)} on {like.device}")
    if not t.is_contiguous() or t.data_ptr() % 16:
        raise SdvarError(f"{who}: {name} with strides {tuple(t.stride())} at address % 16 == {t.data_ptr() % 16} is not dense and 16-byte aligned "
                         f"(pass {name}.clone(memory_format=torch.contiguous_format))")
    return B, L, Cc


def train_vec_in_place(t: torch.Tensor) -> bool:
    """The 16-byte rule of a modulation vector (B, 1, C) / (1, 1, C) / (B, C): unit last stride, a 16-byte aligned base and, with more than one row, a batch stride
    that is a non-negative multiple of 16 bytes.  The unbind(2) views of a (B, 1, 6, C) or (B, 1, 2, C) buffer meet it."""
    per16 = 16 // t.element_size()
    bs = t.stride(0) if t.shape[0] > 1 else 0
    return (t.shape[-1] == 1 or t.stride(-1) == 1) and t.data_ptr() % 16 == 0 and bs >= 0 and bs % per16 == 0


def _train_vec(who: str, name: str, t, B: int, Cc: int, dev):
    """A modulation vector of the adaln / gate_add calls -> (dtype code, batch stride in elements, rows = B or 1)."""
    if not isinstance(t, torch.Tensor):
        raise SdvarError(f"{who}: {name} is not a tensor")
    if not t.is_cuda or t.device != dev:
        raise SdvarError(f"{who}: {name} is on {t.device}; every operand must be on x's GPU ({dev}); there is no CPU path")
    if t.dtype not in TRAIN_DTYPES:
        raise SdvarError(f"{who}: {name} is {t.dtype}; it must be float32, float16 or bfloat16 (pass {name}.float())")
    shp = tuple(t.shape)
    if not (shp in ((B, 1, Cc), (1, 1, Cc), (B, Cc))):
        raise SdvarError(f"{who}: {name} of shape {shp} does not broadcast against (B, L, C) = ({B}, L, {Cc}); expected ({B}, 1, {Cc}), (1, 1, {Cc}) or ({B}, {Cc}) "
                         f"(reshape it to one row of C values per image)")
    if not train_vec_in_place(t):
        raise SdvarError(f"{who}: {name} with strides {tuple(t.stride())} at address % 16 == {t.data_ptr() % 16} breaks the 16-byte rule: unit last stride, base and "
                         f"batch stride multiples of 16 bytes (pass {name}.contiguous())")
    rows = shp[0]
    return TRAIN_DTYPES[t.dtype], (t.stride(0) if rows > 1 else 0), rows


def _train_one_half(who: str, **named) -> None:
    halves = {n: t.dtype for n, t in named.items() if isinstance(t, torch.Tensor) and t.dtype in (torch.float16, torch.bfloat16)}
    if len(set(halves.values())) > 1:
        raise SdvarError(f"{who}: float16 mixed with bfloat16 ({', '.join(f'{n} is {d}' for n, d in halves.items())}); use one half dtype, or pass .float()")


def _train_row_scale(who: str, rs, B: int, dev):
    if rs is None:
        return None
    if not isinstance(rs, torch.Tensor) or not rs.is_cuda or rs.device != dev:
        raise SdvarError(f"{who}: row_scale must be a tensor on x's GPU ({dev}); there is no CPU path")
    if rs.dtype != torch.float32 or tuple(rs.shape) != (B,) or not rs.is_contiguous():
        raise SdvarError(f"{who}: row_scale is {rs.dtype} of shape {tuple(rs.shape)}; expected a dense float32 ({B},) tensor (pass row_scale.float().reshape({B}))")
    return rs


def adaln_bwd_ws_bytes(B: int, L: int, Cc: int) -> int:
    """Bytes of sdvar_op_adaln_bwd's workspace: B * ceil(L / TRAIN_CHUNK) * 2 * C floats."""
    n = int(load_library().sdvar_op_adaln_bwd_ws_bytes(B, L, Cc))
    if n < 0:
        raise SdvarError(f"adaln_bwd_ws_bytes: {_lib.sdvar_last_error().decode()}")
    return n


def gate_add_bwd_ws_bytes(B: int, L: int, Cc: int) -> int:
    """Bytes of sdvar_op_gate_add_bwd's workspace: B * ceil(L / TRAIN_CHUNK) * C floats."""
    n = int(load_library().sdvar_op_gate_add_bwd_ws_bytes(B, L, Cc))
    if n < 0:
        raise SdvarError(f"gate_add_bwd_ws_bytes: {_lib.sdvar_last_error().decode()}")
    return n


def adaln_fwd(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """sdvar_op_adaln_fwd: ((x - mean) * rstd) * (scale + 1) + shift for x (B, L, C) fp32 dense; scale / shift (B, 1, C), (1, 1, C) or (B, C), each fp32 / fp16 / bf16,
    read in place under the 16-byte rule (train_vec_in_place).  Returns (B, L, C) fp32.  No host synchronisation."""
    who = "adaln_fwd"
    B, L, Cc = _train_rows(who, "x", x, (torch.float32,))
    _train_one_half(who, scale=scale, shift=shift)
    sdt, sbs, _ = _train_vec(who, "scale", scale, B, Cc, x.device)
    hdt, hbs, _ = _train_vec(who, "shift", shift, B, Cc, x.device)
    out = torch.empty(B, L, Cc, dtype=torch.float32, device=x.device)
    lib = load_library()
    with _on_device(x.device):
        _check(lib.sdvar_op_adaln_fwd(_ptr(x), C.c_void_p(scale.data_ptr()), sdt, sbs, C.c_void_p(shift.data_ptr()), hdt, hbs, _ptr(out), B, L, Cc, float(eps), _stream()))
    return out


def adaln_bwd(x: torch.Tensor, scale: torch.Tensor, g: torch.Tensor, eps: float, shift_dtype: torch.dtype, scale_rows: int, shift_rows: int,
              need=(True, True, True)):
    """sdvar_op_adaln_bwd: (dx (B, L, C) fp32, dscale (scale_rows, C) in scale's dtype, dshift (shift_rows, C) in shift_dtype) for the upstream gradient g (B, L, C) fp32
    dense; an entry of `need` that is False is not computed (None).  *_rows = B or 1 (1: summed over the images).  No host synchronisation."""
    who = "adaln_bwd"
    B, L, Cc = _train_rows(who, "x", x, (torch.float32,))
    _train_rows(who, "g", g, (torch.float32,), x)
    sdt, sbs, _ = _train_vec(who, "scale", scale, B, Cc, x.device)
    if shift_dtype not in TRAIN_DTYPES or scale_rows not in (1, B) or shift_rows not in (1, B):
        raise SdvarError(f"{who}: shift_dtype {shift_dtype}, scale_rows {scale_rows}, shift_rows {shift_rows}: a float32 / float16 / bfloat16 dtype and 1 or B = {B} rows")
    nx, ns, nh = (bool(n) for n in need)
    if not (nx or ns or nh):
        return None, None, None
    dev = x.device
    dx = torch.empty(B, L, Cc, dtype=torch.float32, device=dev) if nx else None
    dscale = torch.empty(scale_rows, Cc, dtype=scale.dtype, device=dev) if ns else None
    dshift = torch.empty(shift_rows, Cc, dtype=shift_dtype, device=dev) if nh else None
    ws = torch.empty(adaln_bwd_ws_bytes(B, L, Cc) // 4, dtype=torch.float32, device=dev) if ns or nh else None
    lib = load_library()
    with _on_device(dev):
        _check(lib.sdvar_op_adaln_bwd(_ptr(x), C.c_void_p(scale.data_ptr()), sdt, sbs, _ptr(g), _ptr(dx), _ptr(dscale), scale_rows, _ptr(dshift), TRAIN_DTYPES[shift_dtype],
                                      shift_rows, _ptr(ws), B, L, Cc, float(eps), _stream()))
    return dx, dscale, dshift


def gate_add_fwd(x: torch.Tensor, y: torch.Tensor, gamma: torch.Tensor, row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sdvar_op_gate_add_fwd: x + (y * gamma) * row_scale[b] for x (B, L, C) fp32 and y (B, L, C) fp32 / fp16 / bf16, both dense; gamma as adaln_fwd's scale; row_scale (B,)
    fp32 or None.  Returns (B, L, C) fp32; y is not modified.  No host synchronisation."""
    who = "gate_add_fwd"
    B, L, Cc = _train_rows(who, "x", x, (torch.float32,))
    _train_rows(who, "y", y, tuple(TRAIN_DTYPES), x)
    _train_one_half(who, y=y, gamma=gamma)
    gdt, gbs, _ = _train_vec(who, "gamma", gamma, B, Cc, x.device)
    rs = _train_row_scale(who, row_scale, B, x.device)
    out = torch.empty(B, L, Cc, dtype=torch.float32, device=x.device)
    lib = load_library()
    with _on_device(x.device):
        _check(lib.sdvar_op_gate_add_fwd(_ptr(x), _ptr(y), TRAIN_DTYPES[y.dtype], C.c_void_p(gamma.data_ptr()), gdt, gbs, _ptr(rs), _ptr(out), B, L, Cc, _stream()))
    return out


def gate_add_bwd(g: torch.Tensor, y: torch.Tensor, gamma: torch.Tensor, row_scale: Optional[torch.Tensor], gamma_rows: int, need=(True, True)):
    """sdvar_op_gate_add_bwd: (dy (B, L, C) in y's dtype, dgamma (gamma_rows, C) in gamma's dtype) for the upstream gradient g (B, L, C) fp32 dense - which is also the
    gradient of x, as it is.  An entry of `need` that is False is not computed (None).  No host synchronisation."""
    who = "gate_add_bwd"
    B, L, Cc = _train_rows(who, "g", g, (torch.float32,))
    _train_rows(who, "y", y, tuple(TRAIN_DTYPES), g)
    gdt, gbs, _ = _train_vec(who, "gamma", gamma, B, Cc, g.device)
    rs = _train_row_scale(who, row_scale, B, g.device)
    if gamma_rows not in (1, B):
        raise SdvarError(f"{who}: gamma_rows {gamma_rows} must be 1 or B = {B}")
    ny, ng = (bool(n) for n in need)
    if not (ny or ng):
        return None, None
    dev = g.device
    dy = torch.empty(B, L, Cc, dtype=y.dtype, device=dev) if ny else None
    dgamma = torch.empty(gamma_rows, Cc, dtype=gamma.dtype, device=dev) if ng else None
    ws = torch.empty(gate_add_bwd_ws_bytes(B, L, Cc) // 4, dtype=torch.float32, device=dev) if ng else None
    lib = load_library()
    with _on_device(dev):
        _check(lib.sdvar_op_gate_add_bwd(_ptr(g), _ptr(y), TRAIN_DTYPES[y.dtype], C.c_void_p(gamma.data_ptr()), gdt, gbs, _ptr(rs), _ptr(dy), _ptr(dgamma), gamma_rows,
                                         _ptr(ws), B, L, Cc, _stream()))
    return dy, dgamma


COND_MAX_M, COND_MAX_K = 64, 4096          # csrc/cond_train.hip: the batch rows and the in_features of a conditioning linear
COND_SLAB = 64                              # rows of W per workgroup of its backward: fixes the workspace size and the order of dc's sum over n


def cond_lin_shape_ok(M: int, N: int, K: int) -> bool:
    """The shape limits of sdvar_op_cond_lin_fwd / _bwd."""
    return 1 <= M <= COND_MAX_M and 8 <= K <= COND_MAX_K and K % 8 == 0 and N >= 8 and N % 8 == 0 and N * K < 2 ** 31


def cond_rows_in_place(t: torch.Tensor) -> bool:
    """The 16-byte rule of the (M, K) operand c: unit last stride, a 16-byte aligned base and, with more than one row, a row stride of at least K that is a multiple
    of 16 bytes (4 float32 elements, 8 half ones)."""
    per16 = 16 // t.element_size()
    return t.stride(1) == 1 and t.data_ptr() % 16 == 0 and (t.shape[0] <= 1 or (t.stride(0) >= t.shape[1] and t.stride(0) % per16 == 0))


def _cond_operands(who: str, c, weight, dtype):
    """The checks common to cond_lin_fwd / cond_lin_bwd -> (M, N, K, c's code, ldc, w's code, arithmetic code).  Nothing here touches the library."""
    for name, t in (("c", c), ("weight", weight)):
        if not isinstance(t, torch.Tensor):
            raise SdvarError(f"{who}: {name} is not a tensor")
        if not t.is_cuda:
            raise SdvarError(f"{who}: {name} is a CPU tensor; the kernels run on the GPU and there is no CPU path (move it with .cuda())")
        if t.dtype not in TRAIN_DTYPES:
            raise SdvarError(f"{who}: {name} is {t.dtype}; it must be float32, float16 or bfloat16 (pass {name}.float())")
        if t.dim() != 2:
            raise SdvarError(f"{who}: {name} has shape {tuple(t.shape)}; expected a matrix ({'M, K' if name == 'c' else 'N, K'})")
    if dtype not in TRAIN_DTYPES:
        raise SdvarError(f"{who}: dtype {dtype} is not an arithmetic code (float32, float16 or bfloat16)")
    for name, t in (("c", c), ("weight", weight)):
        if t.dtype != torch.float32 and t.dtype != dtype:
            raise SdvarError(f"{who}: {name} is {t.dtype} next to {dtype} arithmetic; every operand must be float32 or the arithmetic's own dtype (pass {name}.float())")
    (M, K), N = c.shape, weight.shape[0]
    if weight.shape[1] != K or weight.device != c.device:
        raise SdvarError(f"{who}: weight has shape {tuple(weight.shape)} on {weight.device}; expected (N, {K}) on c's device {c.device}")
    if not cond_lin_shape_ok(M, N, K):
        raise SdvarError(f"{who}: M = {M}, N = {N}, K = {K} is outside the limits: 1 <= M <= {COND_MAX_M}, K a multiple of 8 in [8, {COND_MAX_K}], N a multiple of 8, "
                         f"N * K < 2^31 (larger batches belong to the GEMM seam)")
    if not cond_rows_in_place(c):
        raise SdvarError(f"{who}: c with strides {tuple(c.stride())} at address % 16 == {c.data_ptr() % 16} breaks the 16-byte rule: unit last stride, base and row "
                         f"stride multiples of 16 bytes (pass c.clone(memory_format=torch.contiguous_format))")
    if not weight.is_contiguous() or weight.data_ptr() % 16:
        raise SdvarError(f"{who}: weight with strides {tuple(weight.stride())} at address % 16 == {weight.data_ptr() % 16} is not dense and 16-byte aligned "
                         f"(pass weight.clone(memory_format=torch.contiguous_format))")
    return M, N, K, TRAIN_DTYPES[c.dtype], (c.stride(0) if M > 1 else K), TRAIN_DTYPES[weight.dtype], TRAIN_DTYPES[dtype]


def _cond_dense(who: str, name: str, t, dtype, shape, dev):
    if t is None:
        return
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev:
        raise SdvarError(f"{who}: {name} must be a tensor on c's GPU ({dev}); there is no CPU path")
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.data_ptr() % 16:
        raise SdvarError(f"{who}: {name} is {t.dtype} of shape {tuple(t.shape)}, strides {tuple(t.stride())}, address % 16 == {t.data_ptr() % 16}; expected a dense, "
                         f"16-byte aligned {dtype} tensor of shape {tuple(shape)}")


def _launch_ctx(dev):
    return _on_device(dev) if dev.type == "cuda" else contextlib.nullcontext()


def _addr(t: Optional[torch.Tensor]):
    """The address of an operand whose layout has been checked, or of a tensor allocated here."""
    return None if t is None else C.c_void_p(t.data_ptr())


def cond_lin_bwd_ws_bytes(M: int, N: int, K: int) -> int:
    """Bytes of sdvar_op_cond_lin_bwd's workspace: ceil(N / COND_SLAB) * M * K floats."""
    n = int(load_library().sdvar_op_cond_lin_bwd_ws_bytes(M, N, K))
    if n < 0:
        raise SdvarError(f"cond_lin_bwd_ws_bytes: {_lib.sdvar_last_error().decode()}")
    return n


def cond_lin_fwd(c: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], dtype: torch.dtype) -> torch.Tensor:
    """sdvar_op_cond_lin_fwd: silu(c) W^T + b for c (M, K) read in place under the 16-byte rule (cond_rows_in_place), weight (N, K) dense, bias (N,) float32 or None;
    `dtype` is the arithmetic: float32 (float32 operands only) or a half dtype (each operand float32 or that dtype; autocast's contract).  Returns (M, N) in `dtype`.
    No host synchronisation."""
    who = "cond_lin_fwd"
    M, N, K, cdt, ldc, wdt, adt = _cond_operands(who, c, weight, dtype)
    _cond_dense(who, "bias", bias, torch.float32, (N,), c.device)
    y = torch.empty(M, N, dtype=dtype, device=c.device)
    lib = load_library()
    with _launch_ctx(c.device):
        _check(lib.sdvar_op_cond_lin_fwd(_addr(c), cdt, ldc, _addr(weight), wdt, _addr(bias), _addr(y), adt, M, N, K, _stream()))
    return y


def cond_lin_bwd(dy: torch.Tensor, c: torch.Tensor, weight: torch.Tensor, dtype: torch.dtype, need=(True, True, True)):
    """sdvar_op_cond_lin_bwd: (dc (M, K) in c's dtype, dW (N, K) in the weight's dtype, db (N,) float32) for the upstream gradient dy (M, N) dense in `dtype`; an entry
    of `need` that is False is not computed (None), and W is read only for dc.  The workspace is allocated here, for dc only.  No host synchronisation."""
    who = "cond_lin_bwd"
    M, N, K, cdt, ldc, wdt, adt = _cond_operands(who, c, weight, dtype)
    _cond_dense(who, "dy", dy, dtype, (M, N), c.device)
    if dy is None:
        raise SdvarError(f"{who}: dy is None")
    nc, nw, nb = (bool(n) for n in need)
    if not (nc or nw or nb):
        return None, None, None
    dev = c.device
    dc = torch.empty(M, K, dtype=c.dtype, device=dev) if nc else None
    dw = torch.empty(N, K, dtype=weight.dtype, device=dev) if nw else None
    db = torch.empty(N, dtype=torch.float32, device=dev) if nb else None
    ws = torch.empty(cond_lin_bwd_ws_bytes(M, N, K) // 4, dtype=torch.float32, device=dev) if nc else None
    lib = load_library()
    with _launch_ctx(dev):
        _check(lib.sdvar_op_cond_lin_bwd(_addr(dy), _addr(c), cdt, ldc, _addr(weight), wdt, _addr(dc), _addr(dw), _addr(db), _addr(ws), adt, M, N, K, _stream()))
    return dc, dw, db


EMBED_MAX_K = 64          # csrc/embed_train.hip: Cvae, the in_features of word_embed
EMBED_TOK = 8             # tokens per workgroup of its backward: fixes the workspace size and the order of dW's sum


def embed_xv_in_place(t: torch.Tensor) -> bool:
    """The 16-byte rule of the (B, rows, K) operand xv: unit last stride, a 16-byte aligned base, row and batch strides that are multiples of 4 elements, rows that do
    not overlap.  The reference's slice x_BLCv_wo_first_l[:, :ed - first_l] meets it."""
    B, rows, K = t.shape
    return (t.stride(2) == 1 and t.data_ptr() % 16 == 0 and (rows <= 1 or (t.stride(1) >= K and t.stride(1) % 4 == 0))
            and (B <= 1 or (t.stride(0) % 4 == 0 and t.stride(0) >= (rows - 1) * (t.stride(1) if rows > 1 else 0) + K)))


def _embed_tensor(who: str, name: str, t, dtypes, hint: str):
    if not isinstance(t, torch.Tensor):
        raise SdvarError(f"{who}: {name} is not a tensor")
    if not t.is_cuda:
        raise SdvarError(f"{who}: {name} is a CPU tensor; the kernels run on the GPU and there is no CPU path (move it with .cuda())")
    if t.dtype not in dtypes:
        raise SdvarError(f"{who}: {name} is {t.dtype}; it must be {' or '.join(str(d) for d in dtypes)} ({hint})")


def _embed_dense(who: str, name: str, t, shape, dev):
    if tuple(t.shape) != tuple(shape):
        raise SdvarError(f"{who}: {name} has shape {tuple(t.shape)}; expected {tuple(shape)}")
    if t.device != dev:
        raise SdvarError(f"{who}: {name} is on {t.device}; every operand must be on label's GPU ({dev})")
    if not t.is_contiguous() or t.data_ptr() % 16:
        raise SdvarError(f"{who}: {name} with strides {tuple(t.stride())} at address % 16 == {t.data_ptr() % 16} is not dense and 16-byte aligned "
                         f"(pass {name}.clone(memory_format=torch.contiguous_format))")


def _embed_operands(who: str, label, xv, word_w, lvl_1L, drop, first_l: int, tokens: Optional[int]):
    """The checks common to embed_fwd / embed_bwd -> (B, T, L, K, C, label's int64 flag, r, rate, xv's batch and row strides).  Nothing here touches the library."""
    _embed_tensor(who, "label_B", label, (torch.int64, torch.int32), "pass label_B.long()")
    _embed_tensor(who, "lvl_1L", lvl_1L, (torch.int64,), "pass lvl_1L.long()")
    _embed_tensor(who, "word_w", word_w, (torch.float32,), "the parameters are float32 master weights: pass word_w.float()")
    dev = label.device
    if label.dim() != 1 or label.shape[0] < 1:
        raise SdvarError(f"{who}: label_B has shape {tuple(label.shape)}; expected (B,) with B >= 1")
    B = label.shape[0]
    _embed_dense(who, "label_B", label, (B,), dev)
    if lvl_1L.dim() not in (1, 2) or lvl_1L.numel() != lvl_1L.shape[-1] or lvl_1L.numel() < 1:
        raise SdvarError(f"{who}: lvl_1L has shape {tuple(lvl_1L.shape)}; expected (1, L) or (L,)")
    L = lvl_1L.shape[-1]
    _embed_dense(who, "lvl_1L", lvl_1L, lvl_1L.shape, dev)
    if word_w.dim() != 2:
        raise SdvarError(f"{who}: word_w has shape {tuple(word_w.shape)}; expected (C, K)")
    Cc, K = word_w.shape
    if Cc < 4 or Cc > TRAIN_MAX_C or Cc % 4:
        raise SdvarError(f"{who}: C = {Cc} (word_w.shape[0]) is outside the supported range: a multiple of 4 in [4, {TRAIN_MAX_C}] (pad the channel dimension)")
    if K < 4 or K > EMBED_MAX_K or K % 4:
        raise SdvarError(f"{who}: K = {K} (word_w.shape[1], Cvae) is outside the supported range: a multiple of 4 in [4, {EMBED_MAX_K}] (use linear_grad for a wider word_embed)")
    _embed_dense(who, "word_w", word_w, (Cc, K), dev)
    T = L if tokens is None else int(tokens)
    if not (1 <= first_l <= T <= L):
        raise SdvarError(f"{who}: tokens = {T} is outside [first_l, L] = [{first_l}, {L}] (pos_start has {first_l} rows, lvl_1L {L} entries)")
    if B * T > 2 ** 29:
        raise SdvarError(f"{who}: B * tokens = {B * T} is above 2^29 (split the batch)")
    xbs = xrs = 0
    if T > first_l:
        _embed_tensor(who, "x_BLCv_wo_first_l", xv, (torch.float32,), "pass x_BLCv_wo_first_l.float()")
        if xv.dim() != 3 or xv.shape[0] != B or xv.shape[2] != K or xv.shape[1] < T - first_l or xv.device != dev:
            raise SdvarError(f"{who}: x_BLCv_wo_first_l has shape {tuple(xv.shape)} on {xv.device}; expected ({B}, >= {T - first_l}, {K}) on {dev}")
        if not embed_xv_in_place(xv):
            raise SdvarError(f"{who}: x_BLCv_wo_first_l with strides {tuple(xv.stride())} at address % 16 == {xv.data_ptr() % 16} breaks the 16-byte rule: unit last "
                             f"stride, base, row and batch strides multiples of 16 bytes (pass x_BLCv_wo_first_l.clone(memory_format=torch.contiguous_format))")
        xbs, xrs = (xv.stride(0) if B > 1 else 0), (xv.stride(1) if xv.shape[1] > 1 else K)
    elif xv is not None and not isinstance(xv, torch.Tensor):
        raise SdvarError(f"{who}: x_BLCv_wo_first_l is not a tensor")
    r, rate = None, 0.0
    if drop is not None:
        if not isinstance(drop, (tuple, list)) or len(drop) != 2:
            raise SdvarError(f"{who}: drop must be None or (r, rate): the float32 (B,) uniform draws and the drop rate")
        r, rate = drop
        _embed_tensor(who, "drop's r", r, (torch.float32,), "draw it with torch.rand(B, device=label_B.device)")
        _embed_dense(who, "drop's r", r, (B,), dev)
        rate = float(rate)
    return B, T, L, K, Cc, (1 if label.dtype == torch.int64 else 0), r, rate, xbs, xrs


def embed_bwd_ws_bytes(B: int, T: int, Cc: int, K: int) -> int:
    """Bytes of sdvar_op_embed_bwd's workspace: T * C + ceil(T / EMBED_TOK) * C * K floats."""
    n = int(load_library().sdvar_op_embed_bwd_ws_bytes(B, T, Cc, K))
    if n < 0:
        raise SdvarError(f"embed_bwd_ws_bytes: {_lib.sdvar_last_error().decode()}")
    return n


def embed_fwd(label, xv, class_emb, pos_start, word_w, word_b, lvl_emb, pos_1LC, lvl_1L, tokens: Optional[int] = None, drop=None, out_dtype: torch.dtype = torch.float32,
              who: str = "embed_fwd"):
    """sdvar_op_embed_fwd: (x (B, T, C) in out_dtype, cond (B, C) float32) from label (B,) int32 / int64, xv (B, >= T - first_l, K) float32 read in place under the 16-byte
    rule (embed_xv_in_place; None allowed when T == first_l), the float32 parameters class_emb (NC1, C), pos_start (1, first_l, C), word_w (C, K), word_b (C,),
    lvl_emb (S, C), pos_1LC (1, L, C) - dense, 16-byte aligned - and lvl_1L (1, L) int64.  T = tokens (None: L); drop = None or (r (B,) float32, rate).  No host
    synchronisation.  `who` names the caller in the refusals."""
    if out_dtype not in TRAIN_DTYPES:
        raise SdvarError(f"{who}: out_dtype {out_dtype} is not float32, float16 or bfloat16")
    for name, t in (("class_emb", class_emb), ("pos_start", pos_start), ("word_b", word_b), ("lvl_emb", lvl_emb), ("pos_1LC", pos_1LC)):
        _embed_tensor(who, name, t, (torch.float32,), f"the parameters are float32 master weights: pass {name}.float()")
    if pos_start.dim() not in (2, 3) or pos_start.numel() != pos_start.shape[-2] * pos_start.shape[-1]:
        raise SdvarError(f"{who}: pos_start has shape {tuple(pos_start.shape)}; expected (1, first_l, C)")
    first_l = pos_start.shape[-2]
    B, T, L, K, Cc, i64, r, rate, xbs, xrs = _embed_operands(who, label, xv, word_w, lvl_1L, drop, first_l, tokens)
    dev = label.device
    if class_emb.dim() != 2 or lvl_emb.dim() != 2:
        raise SdvarError(f"{who}: class_emb has shape {tuple(class_emb.shape)} and lvl_emb {tuple(lvl_emb.shape)}; expected (NC1, {Cc}) and (S, {Cc})")
    NC1, S = class_emb.shape[0], lvl_emb.shape[0]
    _embed_dense(who, "class_emb", class_emb, (NC1, Cc), dev)
    _embed_dense(who, "pos_start", pos_start, tuple(pos_start.shape[:-2]) + (first_l, Cc), dev)
    _embed_dense(who, "word_b", word_b, (Cc,), dev)
    _embed_dense(who, "lvl_emb", lvl_emb, (S, Cc), dev)
    _embed_dense(who, "pos_1LC", pos_1LC, ((1, L, Cc) if pos_1LC.dim() == 3 else (L, Cc)), dev)
    x = torch.empty(B, T, Cc, dtype=out_dtype, device=dev)
    cond = torch.empty(B, Cc, dtype=torch.float32, device=dev)
    lib = load_library()
    with _launch_ctx(dev):
        _check(lib.sdvar_op_embed_fwd(_addr(label), i64, _addr(r), rate, _addr(lvl_1L), _addr(xv) if T > first_l else None, xbs, xrs, _addr(class_emb), _addr(pos_start),
                                      _addr(word_w), _addr(word_b), _addr(lvl_emb), _addr(pos_1LC), _addr(x), TRAIN_DTYPES[out_dtype], _addr(cond), B, T, L, first_l, Cc, K, S,
                                      NC1, _stream()))
    return x, cond


EMBED_GRADS = ("xv", "class_emb", "pos_start", "word_w", "word_b", "lvl_emb", "pos_1LC")


def embed_bwd(g, gc, label, xv, word_w, lvl_1L, tokens: Optional[int], drop, first_l: int, NC1: int, S: int, need=(False, True, True, True, True, True, True),
              who: str = "embed_bwd"):
    """sdvar_op_embed_bwd: the gradients EMBED_GRADS = (dxv in xv's full shape, dclass (NC1, C), dpos_start (1, first_l, C), dW (C, K), dbias (C,), dlvl (S, C),
    dpos_1LC (1, L, C)), all float32, for the upstream gradients g (B, T, C) of x - float32, float16 or bfloat16, dense - and gc (B, C) float32 of cond; either may be
    None.  An entry of `need` that is False is not computed (None).  The workspace is allocated here.  No host synchronisation."""
    B, T, L, K, Cc, i64, r, rate, xbs, xrs = _embed_operands(who, label, xv, word_w, lvl_1L, drop, first_l, tokens)
    dev = label.device
    gdt = 0
    if g is not None:
        _embed_tensor(who, "g", g, tuple(TRAIN_DTYPES), "the gradient of x in x's dtype")
        _embed_dense(who, "g", g, (B, T, Cc), dev)
        gdt = TRAIN_DTYPES[g.dtype]
    if gc is not None:
        _embed_tensor(who, "gc", gc, (torch.float32,), "the gradient of cond_BD is float32")
        _embed_dense(who, "gc", gc, (B, Cc), dev)
    need = tuple(bool(n) for n in need)
    if len(need) != 7:
        raise SdvarError(f"{who}: need has {len(need)} entries; expected one per gradient of {EMBED_GRADS}")
    if not any(need):
        return (None,) * 7
    nx, ncls, nps, nw, nb, nl, npos = need
    if nx and not isinstance(xv, torch.Tensor):
        raise SdvarError(f"{who}: the gradient of x_BLCv_wo_first_l is asked for but it is None")
    f = dict(dtype=torch.float32, device=dev)
    if g is None and gc is None:          # nothing reached either output
        shapes = (tuple(xv.shape) if nx else None, (NC1, Cc), (1, first_l, Cc), (Cc, K), (Cc,), (S, Cc), (1, L, Cc))
        return tuple(torch.zeros(sh, **f) if n else None for n, sh in zip(need, shapes))
    dxv = None
    if nx:          # a row of xv the forward did not read has a zero gradient; without such rows in the call (T == first_l) nothing is launched for it
        dxv, nx = (torch.empty(tuple(xv.shape), **f), True) if T > first_l else (torch.zeros(tuple(xv.shape), **f), False)
    if not (nx or ncls or nps or nw or nb or nl or npos):
        return dxv, None, None, None, None, None, None
    dcls = torch.empty(NC1, Cc, **f) if ncls else None
    dps = torch.empty(1, first_l, Cc, **f) if nps else None
    dw = torch.empty(Cc, K, **f) if nw else None
    db = torch.empty(Cc, **f) if nb else None
    dl = torch.empty(S, Cc, **f) if nl else None
    dpos = torch.empty(1, L, Cc, **f) if npos else None
    ws = torch.empty(embed_bwd_ws_bytes(B, T, Cc, K) // 4, **f) if g is not None and (nps or nw or nb or nl or npos) else None
    lib = load_library()
    with _launch_ctx(dev):
        _check(lib.sdvar_op_embed_bwd(_addr(g), gdt, _addr(gc), _addr(label), i64, _addr(r), rate, _addr(lvl_1L), _addr(xv) if T > first_l else None, xbs, xrs, _addr(word_w),
                                      _addr(dpos), _addr(dps), _addr(dl), _addr(dcls), _addr(db), _addr(dw), _addr(dxv) if nx else None, (xv.shape[1] if nx else 0), _addr(ws), B, T, L, first_l,
                                      Cc, K, S, NC1, _stream()))
    return dxv, dcls, dps, dw, db, dl, dpos


QKNORM_MAX_H = 48


def _qknorm_qkv(who: str, qkv):
    """The (B, L, 3, H, 64) operand of the qknorm calls, read in place: a GPU tensor, float32 / float16 / bfloat16, dense and 16-byte aligned.  Returns (B, L, H)."""
    if not isinstance(qkv, torch.Tensor):
        raise SdvarError(f"{who}: qkv is not a tensor")
    if qkv.dtype not in TRAIN_DTYPES:
        raise SdvarError(f"{who}: qkv is {qkv.dtype}; it must be float32, float16 or bfloat16 (pass qkv.float())")
    if qkv.dim() != 5 or qkv.shape[2] != 3:
        raise SdvarError(f"{who}: qkv has shape {tuple(qkv.shape)}; expected (B, L, 3, H, 64)")
    B, L, _, H, hd = qkv.shape
    if hd != 64:
        raise SdvarError(f"{who}: head dim {hd} of qkv; only 64 is supported")
    if H < 1 or H > QKNORM_MAX_H:
        raise SdvarError(f"{who}: H = {H} heads of qkv is outside the supported range [1, {QKNORM_MAX_H}]")
    if B < 1 or L < 1 or B * L > 2 ** 29:
        raise SdvarError(f"{who}: qkv has shape {tuple(qkv.shape)}; B and L must be at least 1 and B * L at most 2^29 (split the batch)")
    if not qkv.is_cuda:
        raise SdvarError(f"{who}: qkv is a CPU tensor; the kernels run on the GPU and there is no CPU path (move it with .cuda())")
    if not qkv.is_contiguous() or qkv.data_ptr() % 16:
        raise SdvarError(f"{who}: qkv with strides {tuple(qkv.stride())} at address % 16 == {qkv.data_ptr() % 16} is not dense and 16-byte aligned "
                         f"(pass qkv.clone(memory_format=torch.contiguous_format))")
    return B, L, H


def _qknorm_vec(who: str, name: str, t, n: int, dev, optional: bool = True):
    """scale_log (H) / q_bias / v_bias (C): a dense float32 vector on qkv's GPU, 16-byte aligned; None passes when optional."""
    if t is None and optional:
        return None
    if not isinstance(t, torch.Tensor):
        raise SdvarError(f"{who}: {name} is not a tensor")
    if not t.is_cuda or t.device != dev:
        raise SdvarError(f"{who}: {name} is on {t.device}; every operand must be on qkv's GPU ({dev}); there is no CPU path")
    if t.dtype != torch.float32 or tuple(t.shape) != (n,) or not t.is_contiguous() or t.data_ptr() % 16:
        raise SdvarError(f"{who}: {name} is {t.dtype} of shape {tuple(t.shape)} at address % 16 == {t.data_ptr() % 16}; expected a dense, 16-byte aligned float32 ({n},) "
                         f"tensor (pass {name}.float().reshape({n}).clone())")
    return t


def qknorm_grad_in_place(t: torch.Tensor) -> bool:
    """The stride rule of an upstream gradient of the qknorm backward, (B, L, H, 64) in any dim order: unit last stride, every other stride a non-negative multiple of 4
    elements, the base aligned to 4 elements.  The permute(0, 2, 1, 3) views the seam's attention backward returns meet it."""
    return t.stride(-1) == 1 and t.data_ptr() % (4 * t.element_size()) == 0 and all(s >= 0 and s % 4 == 0 for s in t.stride()[:-1])


def _qknorm_grad(who: str, name: str, g, dtype, B: int, L: int, H: int, dev):
    """An upstream gradient given as a (B, L, H, 64) tensor (any strides under the rule above) or None -> its (b, h, l) strides."""
    if g is None:
        return (0, 0, 0)
    if not isinstance(g, torch.Tensor) or not g.is_cuda or g.device != dev:
        raise SdvarError(f"{who}: {name} must be a tensor on qkv's GPU ({dev}); there is no CPU path")
    if g.dtype != dtype:
        raise SdvarError(f"{who}: {name} is {g.dtype}; expected {dtype}")
    if tuple(g.shape) != (B, L, H, 64):
        raise SdvarError(f"{who}: {name} has shape {tuple(g.shape)}; expected ({B}, {L}, {H}, 64)")
    if not qknorm_grad_in_place(g):
        raise SdvarError(f"{who}: {name} with strides {tuple(g.stride())} at address % 16 == {g.data_ptr() % 16} breaks the stride rule: unit last stride, the others "
                         f"non-negative multiples of 4 elements, base aligned to 4 elements (pass {name}.clone(memory_format=torch.contiguous_format))")
    return (g.stride(0), g.stride(2), g.stride(1))


def qknorm_bwd_ws_bytes(B: int, L: int, H: int) -> int:
    """Bytes of sdvar_op_qknorm_bwd's workspace: B * ceil(L / TRAIN_CHUNK) * 3 * 64 H floats."""
    n = int(load_library().sdvar_op_qknorm_bwd_ws_bytes(B, L, H))
    if n < 0:
        raise SdvarError(f"qknorm_bwd_ws_bytes: {_lib.sdvar_last_error().decode()}")
    return n


def qknorm_fwd(qkv: torch.Tensor, scale_log: torch.Tensor, max_log: float, q_bias: Optional[torch.Tensor] = None, v_bias: Optional[torch.Tensor] = None):
    """sdvar_op_qknorm_fwd: qkv (B, L, 3, H, 64) fp32 / fp16 / bf16 dense -> (q, k, v): q = normalize(qkv[:, :, 0] + q_bias) * exp(min(scale_log, max_log)) and
    k = normalize(qkv[:, :, 1]), both (B, L, H, 64) fp32; v = qkv[:, :, 2] + v_bias, (B, L, H, 64) in qkv's dtype - None without a v_bias (nothing is written then).
    scale_log (H), q_bias / v_bias (64 H) fp32.  No host synchronisation."""
    who = "qknorm_fwd"
    B, L, H = _qknorm_qkv(who, qkv)
    dev = qkv.device
    _qknorm_vec(who, "scale_log", scale_log, H, dev, optional=False)
    _qknorm_vec(who, "q_bias", q_bias, 64 * H, dev)
    _qknorm_vec(who, "v_bias", v_bias, 64 * H, dev)
    q = torch.empty(B, L, H, 64, dtype=torch.float32, device=dev)
    k = torch.empty(B, L, H, 64, dtype=torch.float32, device=dev)
    v = torch.empty(B, L, H, 64, dtype=qkv.dtype, device=dev) if v_bias is not None else None
    lib = load_library()
    with _on_device(dev):
        _check(lib.sdvar_op_qknorm_fwd(_ptr(qkv), TRAIN_DTYPES[qkv.dtype], _ptr(q_bias), _ptr(v_bias), _ptr(scale_log), float(max_log), _ptr(q), _ptr(k), _ptr(v), B, L, H,
                                       _stream()))
    return q, k, v


def qknorm_bwd(qkv: torch.Tensor, scale_log: torch.Tensor, max_log: float, q_bias: Optional[torch.Tensor], dq, dk, dv, need=(True, True, True, True)):
    """sdvar_op_qknorm_bwd: (dqkv (B, L, 3, H, 64) in qkv's dtype, dscale_log (H), dq_bias (64 H), dv_bias (64 H), the three sums fp32) for the upstream gradients dq, dk
    (fp32) and dv (qkv's dtype), each a (B, L, H, 64) tensor read through its strides (qknorm_grad_in_place) or None (zero, not read).  An entry of `need` that is False is
    not computed (None).  No host synchronisation."""
    who = "qknorm_bwd"
    B, L, H = _qknorm_qkv(who, qkv)
    dev = qkv.device
    _qknorm_vec(who, "scale_log", scale_log, H, dev, optional=False)
    _qknorm_vec(who, "q_bias", q_bias, 64 * H, dev)
    strides = (C.c_int64 * 9)(*_qknorm_grad(who, "dq", dq, torch.float32, B, L, H, dev), *_qknorm_grad(who, "dk", dk, torch.float32, B, L, H, dev),
                              *_qknorm_grad(who, "dv", dv, qkv.dtype, B, L, H, dev))
    nx, ns, nq, nv = (bool(n) for n in need)
    if not (nx or ns or nq or nv):
        return None, None, None, None
    dqkv = torch.empty(B, L, 3, H, 64, dtype=qkv.dtype, device=dev) if nx else None
    dscale = torch.empty(H, dtype=torch.float32, device=dev) if ns else None
    dqb = torch.empty(64 * H, dtype=torch.float32, device=dev) if nq else None
    dvb = torch.empty(64 * H, dtype=torch.float32, device=dev) if nv else None
    ws = torch.empty(qknorm_bwd_ws_bytes(B, L, H) // 4, dtype=torch.float32, device=dev) if ns or nq or nv else None
    raw = lambda t: None if t is None else C.c_void_p(t.data_ptr())          # strided: read through grad_strides
    lib = load_library()
    with _on_device(dev):
        _check(lib.sdvar_op_qknorm_bwd(_ptr(qkv), TRAIN_DTYPES[qkv.dtype], _ptr(q_bias), _ptr(scale_log), float(max_log), raw(dq), raw(dk), raw(dv), strides, _ptr(dqkv),
                                       _ptr(dscale), _ptr(dqb), _ptr(dvb), _ptr(ws), B, L, H, _stream()))
    return dqkv, dscale, dqb, dvb


def img_err_stats(a: torch.Tensor, b: torch.Tensor, sums: torch.Tensor, accumulate: bool = False):
    """sdvar_img_err_stats: a, b fp32 device tensors of one shape -> sums (2,) float64 {sum |a - b|, sum (a - b)^2}, overwritten or (accumulate) added to
    (fixed-order fp64 reduction: repeated calls are bit-identical)."""
    load_library()
    if a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32 or a.device != b.device or a.numel() == 0:
        raise SdvarError(f"img_err_stats: a {tuple(a.shape)} {a.dtype} and b {tuple(b.shape)} {b.dtype} must be equally shaped, non-empty fp32 tensors on one device")
    if sums.dtype != torch.float64 or sums.numel() != 2 or sums.device != a.device:
        raise SdvarError("img_err_stats: sums must be 2 float64 on the tensors' device")
    a, b = a.contiguous(), b.contiguous()
    _check(_lib.sdvar_img_err_stats(_ptr(a), _ptr(b), a.numel(), _ptr(sums), int(bool(accumulate)), _stream()))


def gemm_h_ex(x: torch.Tensor, w: torch.Tensor, M: int, N: int, K: int, epilogue: int, w_scale: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None, ldo: int = 0, h_out: Optional[torch.Tensor] = None, pre_out: Optional[torch.Tensor] = None,
              res: Optional[torch.Tensor] = None, ldres: int = 0, gate: Optional[torch.Tensor] = None, rows_per_gate: int = 1, gate_stride: int = 0) -> None:
    """sdvar_op_gemm_h_ex: the half kernel as GEMM mode 'f16' launches it.  x, w: fp16 K-blocked operands (M x K), (N x K) (the high plane of an f16x2 operand);
    w_scale: one float32 on the device or None; bias (N,) float32 or None.  epilogue 0: out fp32 rows of ldo; 1: h_out = the fp16 operand (M x N) of gelu(.), pre_out
    (M, N) fp16 or None; 2: out = res + (.) * gate[(m // rows_per_gate) * gate_stride + n], res / out fp32 rows of ldres / ldo (res may be out).  Buffers may be larger
    than the kernel writes (guard strips); sizes are checked as minimums here, the arithmetic's own constraints by the library.  No host synchronisation."""
    who = "gemm_h_ex"
    dev = x.device

    def chk(name, t, dtype, numel):
        if t is None:
            return
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != dev or not t.is_cuda or not t.is_contiguous() or t.numel() < numel:
            raise SdvarError(f"{who}: {name} must be a contiguous {dtype} tensor of at least {numel} elements on {dev}")
    if min(M, N, K) < 1:
        raise SdvarError(f"{who}: M={M} N={N} K={K}")
    chk("x", x, torch.float16, M * K); chk("w", w, torch.float16, N * K)
    chk("w_scale", w_scale, torch.float32, 1); chk("bias", bias, torch.float32, N)
    chk("out", out, torch.float32, (M - 1) * ldo + N); chk("res", res, torch.float32, (M - 1) * ldres + N)
    chk("h_out", h_out, torch.float16, M * N); chk("pre_out", pre_out, torch.float16, M * N)
    if gate is not None:
        chk("gate", gate, torch.float32, ((M - 1) // max(rows_per_gate, 1)) * gate_stride + N)
    lib = load_library()
    with _on_device(dev):
        _check(lib.sdvar_op_gemm_h_ex(_addr(x), _addr(w), 1, _addr(w_scale), _addr(bias), _addr(out), ldo, _addr(h_out), _addr(pre_out), _addr(res), ldres, _addr(gate),
                                      rows_per_gate, gate_stride, M, N, K, epilogue, _stream()))


def set_variant(name: str, value: int) -> None:
    """sdvar_debug_set_variant: a process-wide kernel switch by name (csrc/gemm_plan.h), e.g. 'h16_min_m'; value < 0 = back to the environment / default."""
    _check(load_library().sdvar_debug_set_variant(name.encode(), int(value)))


def last_gemm_cfg() -> Dict[str, int]:
    """Test aid: row tile and K split of the last f16x2 GEMM call of this thread, and how many launches since the last read took the hybrid tail split /
    finished q and k in the QKV epilogue (reading resets the two counters).  bm == HALF_KERNEL_CODE: the last launch was mode f16's half kernel."""
    v = (_I * 4)()
    _check(load_library().sdvar_debug_get_gemm_cfg(v))
    return dict(bm=v[0], split=v[1], tail_launches=v[2], fused_qkv_launches=v[3])


_GUARD_ON = False


def f16x2_guard(on: bool):
    """Debug switch (mode f16x2): count saturated / non-finite / tiny elements of every GEMM operand plane written inside stage_forward.
    While it is on, every sampler call ends with a device sync and reports the counters of that call in `SampleResult.stats["f16x2_guard"]`."""
    global _GUARD_ON
    _check(load_library().sdvar_debug_set_f16x2_guard(1 if on else 0))
    _GUARD_ON = bool(on)
    if on:
        f16x2_guard_collect(reset=True)


def f16x2_guard_collect(reset: bool = True) -> Dict[str, int]:
    v = (_U64 * 4)()
    _check(load_library().sdvar_debug_get_f16x2_guard(v, 1 if reset else 0))
    return dict(elements=int(v[0]), saturated=int(v[1]), non_finite=int(v[2]), tiny=int(v[3]))


def prof_enable(on: bool):
    _check(load_library().sdvar_prof_enable(1 if on else 0))


def prof_collect() -> Dict[str, Dict[str, float]]:
    k = len(PROF_CLASSES)
    ms, n, fl, by = (_D * k)(), (C.c_int64 * k)(), (_D * k)(), (_D * k)()
    _check(load_library().sdvar_prof_collect(ms, n, fl, by))
    return {PROF_CLASSES[i]: dict(ms=ms[i], launches=int(n[i]), flops=fl[i], bytes=by[i]) for i in range(k)}


# ------------------------------------------------------------------------------------------------------- sampling loops
@dataclass
class SampleResult:
    ids: torch.Tensor                      # (B, L) int64 accepted token ids, stage s at columns [begin(s), begin(s)+l_s)
    f_hat: torch.Tensor                    # (B, Cvae, HW, HW)
    stats: Dict[str, object] = field(default_factory=dict)
    trace: Dict[str, list] = field(default_factory=dict)
    gen: Optional[torch.Tensor] = None     # masked sampling (VAR.autoregressive_infer_cfg_edit): the (B, L) uint8 token table, 1 = sampled, 0 = the image's own id


class Sampler:
    """Buffers + loops for one (draft, target) pair (or a single model for plain AR) on one GPU."""

    def __init__(self, target: ModelCtx, quant: QuantCtx, draft: Optional[ModelCtx] = None):
        self.t, self.d, self.q = target, draft, quant
        self.lad: Ladder = target.lad
        self.dev = target.device
        B, V, lad = target.max_batch, target.V, self.lad
        lens = lad.lens
        self.lmax_t = max(sum(lens[s:s + target.max_chunk]) for s in range(lad.S))
        f = dict(device=self.dev, dtype=torch.float32)
        self.x_t = torch.empty(2 * B * self.lmax_t * target.Cw, **f)
        self._xt = [self.x_t, None]             # second target input buffer: allocated when the run-ahead path first needs it
        self._verify_stream = None
        self.logits_t = torch.empty(2 * B * self.lmax_t * V, **f)
        if draft is not None:
            assert draft.lad.patch_nums == lad.patch_nums and draft.V == V
            self.x_d = torch.empty(2 * B * lens[-1] * draft.Cw, **f)
            self.logits_d = torch.empty(2 * B * lens[-1] * V, **f)
        g = target.max_chunk
        self.ids = torch.zeros(B, lad.L, device=self.dev, dtype=torch.int64)
        self.f_work = torch.zeros(B, quant.Cv, lad.HW, lad.HW, **f)
        self.f_acc = torch.zeros_like(self.f_work)
        self._fs = [[torch.zeros_like(self.f_work) for _ in range(g)], None]      # f_hat snapshots / next-stage inputs of a round; the second
        self._nx = [[torch.empty(B * lens[-1] * quant.Cv, **f) for _ in range(g)], None]    # slot exists once the optimistic path runs
        self._slot = 0
        self.nxt_cur = torch.empty(B * lens[-1] * quant.Cv, **f)
        self.counts = torch.zeros(40, device=self.dev, dtype=torch.int32)
        self.counts_ra = torch.zeros(4 * lad.S, 40, device=self.dev, dtype=torch.int32)     # one counter row per enqueued verification
        self._counts_pin = torch.zeros(4 * lad.S, 40, dtype=torch.int32).pin_memory()
        self._row = 0
        self.counts_host = torch.zeros(40, dtype=torch.int32).pin_memory()
        self._lazy: Dict[str, torch.Tensor] = {}      # buffers only some paths need (more_smooth, KL rule, token-level acceptance, hand-off)

    def _buf(self, name: str, numel: int, dtype=torch.float32) -> torch.Tensor:
        t = self._lazy.get(name)
        if t is None or t.numel() < numel or t.dtype != dtype:
            t = self._lazy[name] = torch.empty(numel, device=self.dev, dtype=dtype)
        return t

    def _sample_stage(self, logits: torch.Tensor, B: int, si: int, cfg: float, top_k: int, top_p: float, noise: Noise, draw: int,
                      more_smooth: bool, f_hat: torch.Tensor, nxt: Optional[torch.Tensor], f_in: Optional[torch.Tensor] = None, keep_masked: bool = False,
                      rows: Optional[RowParams] = None, forced=None):
        """CFG + top-k/top-p + multinomial (var.py:199-202), then the token -> feature step (var.py:205-211): codebook rows of the sampled ids,
        or with more_smooth=True the gumbel-softmax mix of the masked logits (var.py:206-208).  `rows`: image b's own parameters (cfg, top_k, top_p ignored).
        `forced`: (gen, force_ids), each (B, L): the forced entry points - a token with gen == 0 takes its id from force_ids instead of being sampled."""
        lad, V, L, qz = self.lad, self.t.V, self.lad.L, self.q
        l = lad.lens[si]
        q = noise.tensor(draw, B, l, V, self.dev)
        masked = self._buf("masked", B * lad.lens[-1] * V) if (more_smooth or keep_masked) else None          # the CFG logits after top-k / top-p (-inf = removed)
        if forced is not None:
            gen, force_ids = forced
            if rows is not None:
                cfg_sample_rows_forced(logits, B, l, V, rows, si, q, draw, self.ids, lad.begin(si), L, gen, force_ids, lad.begin(si), L, masked)
            else:
                cfg_sample_forced(logits, B, l, V, lad.cfg_t(cfg, si), top_k, top_p, q, noise.seed, draw, noise.image_offset, self.ids, lad.begin(si), L,
                                  gen, force_ids, lad.begin(si), L, masked)
        elif rows is not None:
            cfg_sample_rows(logits, B, l, V, rows, si, q, draw, self.ids, lad.begin(si), L, masked)
        else:
            cfg_sample(logits, B, l, V, lad.cfg_t(cfg, si), top_k, top_p, q, noise.seed, draw, noise.image_offset, self.ids, lad.begin(si), L, masked)
        last = si == lad.S - 1
        if not more_smooth:
            qz.next(si, self.ids[:, lad.begin(si):], L, f_hat, None if last else nxt, B, f_in=f_in)
            return masked
        assert f_in is None
        ratio = si / (lad.S - 1)
        tau = max(0.27 * (1 - ratio * 0.95), 0.005)                           # var.py:207
        e = noise.tensor(draw | GUMBEL_DRAW, B, l, V, self.dev)                # the generator's next (B, l, V) exponential draw (helpers.py:26)
        h = self._buf("h_soft", B * lad.lens[-1] * qz.Cv)
        if rows is not None:
            qz.gumbel_mix_rows(masked, B, l, ratio, tau, e, rows, draw | GUMBEL_DRAW, h)
        else:
            qz.gumbel_mix(masked, B, l, ratio, tau, e, noise.seed, draw | GUMBEL_DRAW, noise.image_offset, h)
        qz.next_h(si, h, f_hat, None if last else nxt, B)
        return masked

    def _f16_stats(self, stats: Dict[str, object]):
        """GEMM mode f16 only: stats['gemm_mode'] = (target's, draft's) and stats['last_gemm_half'] = whether the call's last GEMM launch (the head of its last forward)
        ran on the half kernel, i.e. whether that forward had at least h16_min_m rows."""
        modes = (self.t.gemm_mode, self.d.gemm_mode if self.d is not None else None)
        if "f16" in modes:
            stats["gemm_mode"] = modes
            stats["last_gemm_half"] = last_gemm_cfg()["bm"] == HALF_KERNEL_CODE

    def _forced_arg(self, who: str, B: int, force_ids, gen, more_smooth: bool, trusted_ids: bool):
        """The mask arguments of plain_ar and of the speculative loop, checked before anything is launched: (gen, force_ids), or None without a mask."""
        if force_ids is None and gen is None:
            return None
        V, L = self.t.V, self.lad.L
        if force_ids is None or gen is None:
            raise SdvarError(f"{who}: force_ids and gen go together (both (B, L)), got only {'gen' if force_ids is None else 'force_ids'}")
        if more_smooth:
            raise SdvarError(f"{who}: more_smooth=True with a mask (force_ids / gen) is not supported: the gumbel mix of a forced token is undefined")
        for name, t, dtype in (("force_ids", force_ids, torch.int64), ("gen", gen, torch.uint8)):
            if isinstance(t, torch.Tensor) and tuple(t.shape) != (B, L):
                raise SdvarError(f"{who}: {name} has shape {tuple(t.shape)}, expected (B, L) = {(B, L)}")
            _edit_tensor(who, name, t, dtype, B * L, self.ids.device, 8 if dtype == torch.int64 else 1)
        if not trusted_ids and bool(((force_ids < 0) | (force_ids >= V)).any()):
            raise SdvarError(f"{who}: force_ids holds ids outside [0, V = {V})")
        return (gen, force_ids)

    @property
    def f_snap(self):
        return self._fs[self._slot]

    @property
    def nxt(self):
        return self._nx[self._slot]

    # ---- VAR.autoregressive_infer_cfg (var.py:127-215) up to the decode
    def plain_ar(self, labels: torch.Tensor, cfg: float, top_k: int, top_p: float, noise: Noise, trace: bool = False,
                 more_smooth: bool = False, force_ids: Optional[torch.Tensor] = None, gen: Optional[torch.Tensor] = None,
                 trusted_ids: bool = False) -> SampleResult:
        """`force_ids` (B, L) int64 and `gen` (B, L) uint8, both or neither: masked sampling - token (b, i) is sampled where gen[b, i] != 0 and takes force_ids[b, i]
        elsewhere (in-painting: the image's own ids outside the edit region); a sampled token draws what the unmasked call would draw on the same logits.  Every
        force_ids value must lie in [0, V): checked once before the first launch (one reduction, one synchronisation) unless trusted_ids=True."""
        m, qz, lad = self.t, self.q, self.lad
        B, V, S, L = labels.shape[0], m.V, lad.S, lad.L
        forced = self._forced_arg("plain_ar", B, force_ids, gen, more_smooth, trusted_ids)
        res = SampleResult(ids=self.ids[:B], f_hat=self.f_work[:B])
        with torch.cuda.device(self.dev):
            rows = RowParams.build(B, lad, cfg, top_k, top_p, noise, self.dev)          # None for scalar arguments: the scalar launches
            m.begin(labels)
            f_hat = self.f_work[:B]; f_hat.zero_()
            for si in range(S):
                l = lad.lens[si]
                if si == 0:
                    m.forward_first(self.logits_t)
                else:
                    m.forward(self.x_t, si, 1, self.logits_t)
                if trace:
                    res.trace.setdefault("logits", []).append(self.logits_t[:2 * B * l * V].view(2 * B, l, V).clone())
                self._sample_stage(self.logits_t, B, si, cfg, top_k, top_p, noise, si, more_smooth, f_hat, self.nxt[0], rows=rows, forced=forced)
                if si != S - 1:
                    m.embed_next(self.nxt[0], si + 1, self.x_t, lad.lens[si + 1], 0)
            m.kv_set_len(0)
        res.stats = dict(target_calls=S, draft_stage_calls=0, forced_accepts=0, accepted_tokens=0)
        self._f16_stats(res.stats)
        if _GUARD_ON:
            res.stats["f16x2_guard"] = f16x2_guard_collect()
        return res

    # ---- VAR.autoregressive_infer_cfg_sd_helper1 (var.py:319-443): a run of `step` stages of the plain sampler from a handed-in state
    def resume_ar(self, cond: torch.Tensor, current_step: int, step: int, next_map: Optional[torch.Tensor], f_hat: torch.Tensor, cfg: float, top_k: int,
                  top_p: float, noise: Noise, more_smooth: bool = False):
        """Stages current_step .. current_step + step - 1 with the conditioning rows `cond` (2B, C) = `sos`, the next-scale map `next_map`
        (B, Cvae, pn, pn) of stage current_step and the running f_hat, which is updated IN PLACE as the reference's quantizer does (quant.py:191).
        The KV cache starts EMPTY: var.py:368 toggles kv_caching(True), which drops it (basic_var.py:87), so the resumed stages attend to themselves
        and to each other, not to the stages before current_step; and `cur_L` starts at 0 there too (var.py:352: the skipped stages do not advance
        it), so stage si is embedded with the lvl_pos rows begin(si) - begin(current_step) .. - both are the reference's behaviour, pinned by
        tests/golden/ar_d4_256_helper1.npz.  Draw index of stage si = si.
        Returns the four histories of var.py:436-443: input maps (B, l, Cvae) of the stages run that are not stage 0, then the raw next map
        (B, Cvae, pn', pn') after the last one (f_hat itself after the final stage); f_hat (the same tensor step + 1 times - the reference appends
        the object it then updates in place); CFG-combined logits (B, l, V) as the sampler left them (-inf at the entries top-k / top-p removed:
        helpers.py:10,15 mask the appended tensor in place); token ids (B, l)."""
        scalar_arg("resume_ar", cfg=cfg, top_k=top_k, top_p=top_p, noise=noise)
        m, qz, lad = self.t, self.q, self.lad
        S, V, L, lens, Cv = lad.S, m.V, lad.L, lad.lens, qz.Cv
        B = cond.shape[0] // 2
        if not (0 <= current_step < S and step >= 1):
            raise SdvarError(f"resume_ar: current_step {current_step}, step {step} (ladder has {S} stages)")
        if f_hat.shape != (B, Cv, lad.patch_nums[-1], lad.patch_nums[-1]) or not f_hat.is_cuda or f_hat.dtype != torch.float32 or not f_hat.is_contiguous():
            raise SdvarError("resume_ar: f_hat must be a contiguous fp32 GPU tensor (B, Cvae, pn_last, pn_last)")
        if current_step > 0 and (next_map is None or next_map.numel() != B * Cv * lens[current_step]):
            raise SdvarError(f"resume_ar: stage {current_step} needs its next-scale map (B, Cvae, {lad.patch_nums[current_step]}, {lad.patch_nums[current_step]})")
        inputs, f_hist, logit_hist, id_hist = [], [], [], []
        end = min(current_step + step, S)
        with torch.cuda.device(self.dev):
            m.begin_cond(cond)
            m.kv_set_origin(current_step)
            nxt = self.nxt[0]
            for si in range(current_step, end):
                l = lens[si]
                if si == 0:
                    m.place_first(self.x_t, l)
                else:
                    if si == current_step:
                        rows = next_map.to(torch.float32).reshape(B, Cv, l).transpose(1, 2).contiguous()          # var.py:382
                        nxt[:B * l * Cv].view(B, l, Cv).copy_(rows)
                    inputs.append(nxt[:B * l * Cv].view(B, l, Cv).clone())
                    m.embed_next_at(nxt, si, lad.begin(si) - lad.begin(current_step), self.x_t, l, 0)              # var.py:385 with cur_L counted from current_step
                f_hist.append(f_hat)
                m.forward(self.x_t, si, 1, self.logits_t)
                masked = self._sample_stage(self.logits_t, B, si, cfg, top_k, top_p, noise, si, more_smooth, f_hat, nxt, keep_masked=True)
                logit_hist.append(masked[:B * l * V].view(B, l, V).clone())           # var.py:405-408: the CFG logits, masked in place by helpers.py:10,15 before the caller sees them
                id_hist.append(self.ids[:B, lad.begin(si):lad.begin(si) + l].clone())
            f_hist.append(f_hat)
            if end == S:
                inputs.append(f_hat)                                                                               # quant.py:196: the last stage hands back f_hat twice
            else:
                pn = lad.patch_nums[end]
                inputs.append(nxt[:B * pn * pn * Cv].view(B, pn * pn, Cv).transpose(1, 2).reshape(B, Cv, pn, pn).clone())
            m.kv_set_len(0)
        return inputs, f_hist, logit_hist, id_hist

    # ---- SDVAR.sdvar_autoregressive_infer_cfg_sd_test3 (var.py:604-865): the draft samples stages < entry_num, the target the rest
    def handoff(self, labels: torch.Tensor, cfg: float, top_k: int, top_p: float, noise: Noise, entry_num: int, sd_mask: int = 0,
                more_smooth: bool = False, force_ids=None, gen=None) -> SampleResult:
        """sd_mask 0: the target starts at the entry stage with an empty KV cache - it does not condition on the draft's prefix
        (var.py:817-824).  sd_mask 3: the target first runs the whole prefix + entry stage through its blocks under the block-causal
        mask (var.py:789, 802-804: this fills its cache), then - literally as the reference does - takes the entry stage's logits from
        the INPUT token map, not from the block output (var.py:809-811).  One noise stream: draw index = stage (var.py:642, 689, 831)."""
        assert self.d is not None, "the hand-off sampler needs a draft model"
        if force_ids is not None or gen is not None:
            raise SdvarError("handoff: masked sampling (force_ids / gen) is not supported here: use plain_ar or spec_decode")
        scalar_arg("handoff", cfg=cfg, top_k=top_k, top_p=top_p, noise=noise)
        d, t, qz, lad = self.d, self.t, self.q, self.lad
        B, V, S, L, lens = labels.shape[0], t.V, lad.S, lad.L, lad.lens
        if not (0 <= entry_num <= S):
            raise SdvarError(f"entry_num {entry_num} outside [0, {S}]")
        if sd_mask not in (0, 1, 2, 3, 4, 5):
            raise SdvarError(f"sd_mask {sd_mask}: the reference defines 0 .. 5 (var.py:777-798)")
        res = SampleResult(ids=self.ids[:B], f_hat=self.f_work[:B])
        prefill = sd_mask != 0 and entry_num < S
        pindex = lad.cum[entry_num] if entry_num < S else L
        if prefill and t.max_chunk < entry_num + 1:
            raise SdvarError(f"sd_mask={sd_mask} prefills stages 0..{entry_num} in one pass: the target context needs max_chunk >= {entry_num + 1}")
        with torch.cuda.device(self.dev):
            f_hat = self.f_work[:B]; f_hat.zero_()
            d.begin(labels); t.begin(labels)
            x_pre = self._buf("x_prefill", 2 * B * pindex * t.Cw) if prefill else None
            if prefill:
                t.place_first(x_pre, pindex)
            d.place_first(self.x_d, lens[0])
            for si in range(min(entry_num, S)):                                  # var.py:669-723
                d.forward(self.x_d, si, 1, self.logits_d)
                self._sample_stage(self.logits_d, B, si, cfg, top_k, top_p, noise, si, more_smooth, f_hat, self.nxt[0])
                if si != S - 1:
                    d.embed_next(self.nxt[0], si + 1, self.x_d, lens[si + 1], 0)
                    if prefill:                                                 # draft_token_hub -> target embedding of the prefix (var.py:713, 753)
                        t.embed_next(self.nxt[0], si + 1, x_pre, pindex, lad.begin(si + 1))
            d.kv_set_len(0)
            for si in range(entry_num, S):                                       # var.py:768-859
                l = lens[si]
                if si == entry_num:
                    if prefill:
                        ent = self._buf("x_entry", 2 * B * l * t.Cw)             # the entry stage's slice of the input map, kept: the forward clobbers x
                        src = x_pre[:2 * B * pindex * t.Cw].view(2 * B, pindex, t.Cw)[:, lad.begin(si):pindex]
                        ent[:2 * B * l * t.Cw].view(2 * B, l, t.Cw).copy_(src)
                        bias = None if sd_mask == 3 else handoff_mask(lad, entry_num, sd_mask).to(self.dev)         # 3 = the block-causal rows the kernels derive themselves
                        t.forward(x_pre, 0, entry_num + 1, self._buf("logits_prefill", 2 * B * pindex * V), bias)   # fills the cache; its logits are not used
                        t.head_forward(ent, l, self.logits_t)
                    else:
                        t.kv_set_origin(si)
                        if si == 0:
                            t.place_first(self.x_t, l)
                        else:
                            t.embed_next(self.nxt[0], si, self.x_t, l, 0)
                        t.forward(self.x_t, si, 1, self.logits_t)
                else:
                    t.forward(self.x_t, si, 1, self.logits_t)
                self._sample_stage(self.logits_t, B, si, cfg, top_k, top_p, noise, si, more_smooth, f_hat, self.nxt[0])
                if si != S - 1:
                    t.embed_next(self.nxt[0], si + 1, self.x_t, lens[si + 1], 0)
            t.kv_set_len(0)
        res.stats = dict(target_calls=S - min(entry_num, S), draft_stage_calls=min(entry_num, S), forced_accepts=0, accepted_tokens=0, entry_num=entry_num, sd_mask=sd_mask)
        return res

    # ---- speculative draft -> verify loop, as the reference's four steps
    def spec_begin(self, labels: torch.Tensor, cfg: float, gamma: int, top_k: int, top_p: float, noise: Noise, thr: float = 0.5,
                   match: Optional[MatchRule] = None, force_ids: Optional[torch.Tensor] = None, gen: Optional[torch.Tensor] = None,
                   trusted_ids: bool = False, who: str = "spec_begin") -> "SpecState":
        """SDVAR._initialize_inference_state (var.py:871-947): both prologues, empty caches, counters.
        `force_ids` / `gen` / `trusted_ids`: the mask of plain_ar, for spec_decode (the step-wise helpers of sdvar_amd.var.SDVAR refuse such a state)."""
        assert self.d is not None, "the speculative loop needs a draft model"
        assert 1 <= gamma <= self.t.max_chunk, f"gamma {gamma} exceeds the engine's max_chunk {self.t.max_chunk}"
        forced = self._forced_arg(who, labels.shape[0], force_ids, gen, False, trusted_ids)
        with torch.cuda.device(self.dev):
            rows = RowParams.build(labels.shape[0], self.lad, cfg, top_k, top_p, noise, self.dev)        # per-image parameters: one table for the whole loop
            self.d.begin(labels); self.t.begin(labels)
            self.f_acc[:labels.shape[0]].zero_()
        self._row, self._slot = 0, 0
        return SpecState(sampler=self, labels=labels, B=labels.shape[0], cfg=cfg, gamma=gamma, top_k=top_k, top_p=top_p, noise=noise, thr=thr,
                         total_stages=self.lad.S, patch_nums=self.lad.patch_nums, match=match or MatchRule(), rows=rows, forced=forced)

    def spec_draft(self, st: "SpecState") -> int:
        """SDVAR.draft_generate_batch (var.py:949-1024): g = min(gamma, S - cur) draft stages (forward, CFG, sample, quant,
        next-stage inputs for BOTH models).  Token ids land in self.ids, f_hat snapshots in self.f_snap."""
        d, t, qz, lad = self.d, self.t, self.q, self.lad
        B, V, S, L, lens, cur = st.B, t.V, lad.S, lad.L, lad.lens, st.current_stage
        g = min(st.gamma, S - cur)
        if g <= 0:
            return 0
        st.g, st.glen = g, lens[cur:cur + g]
        lsum = sum(st.glen)
        offs = [sum(st.glen[:j]) for j in range(g)]
        keep_logits = st.match.rule == "kl"        # the KL rule compares the two models' distributions: keep the draft's logits of the round
        dl = self._buf("draft_logits", 2 * self.t.max_batch * self.lmax_t * V) if keep_logits else None
        with torch.cuda.device(self.dev):
            x_t = self._xt[st.xt_idx]
            if cur == 0:
                if g > 1:                                  # the draft's stage 0 and a one-stage verify take forward_first: only a chunk needs the first-token map in x
                    t.place_first(x_t, lsum)
            else:
                d.embed_next(self.nxt_cur, cur, self.x_d, lens[cur], 0); t.embed_next(self.nxt_cur, cur, x_t, lsum, 0)
            for j in range(g):
                s = cur + j
                lg = dl[2 * B * V * offs[j]:] if keep_logits else self.logits_d
                if s == 0:
                    d.forward_first(lg)
                else:
                    d.forward(self.x_d, s, 1, lg)
                st.stats["draft_stage_calls"] += 1
                q = st.noise.tensor(st.draw, B, lens[s], V, self.dev)
                if st.forced is not None:                  # under a mask the draft's forced tokens are the image's own ids
                    gen, force_ids = st.forced
                    if st.rows is not None:
                        cfg_sample_rows_forced(lg, B, lens[s], V, st.rows, s, q, st.draw, self.ids, lad.begin(s), L, gen, force_ids, lad.begin(s), L)
                    else:
                        cfg_sample_forced(lg, B, lens[s], V, lad.cfg_t(st.cfg, s), st.top_k, st.top_p, q, st.noise.seed, st.draw, st.noise.image_offset,
                                          self.ids, lad.begin(s), L, gen, force_ids, lad.begin(s), L)
                elif st.rows is not None:
                    cfg_sample_rows(lg, B, lens[s], V, st.rows, s, q, st.draw, self.ids, lad.begin(s), L)
                else:
                    cfg_sample(lg, B, lens[s], V, lad.cfg_t(st.cfg, s), st.top_k, st.top_p, q, st.noise.seed, st.draw, st.noise.image_offset,
                               self.ids, lad.begin(s), L)
                st.draw += 1
                last = s == S - 1
                # f_hat snapshot j = snapshot j-1 (the accepted prefix for j = 0) + this stage: written directly, nothing is copied
                qz.next(s, self.ids[:, lad.begin(s):], L, self.f_snap[j][:B], None if last else self.nxt[j], B, f_in=self.f_acc[:B] if j == 0 else self.f_snap[j - 1][:B])
                if j + 1 < g:
                    d.embed_next(self.nxt[j], s + 1, self.x_d, lens[s + 1], 0)
                    t.embed_next(self.nxt[j], s + 1, x_t, lsum, offs[j + 1])
        st.drafted = True
        return g

    def spec_verify_forward(self, st: "SpecState") -> torch.Tensor:
        """SDVAR.target_verify_batch (var.py:1026-1070): ONE target forward over the drafted stages under the block-causal
        rows; returns the raw logits view (2B, lsum, V)."""
        assert st.drafted, "draft_generate_batch must run before target_verify_batch"
        lsum = sum(st.glen)
        with torch.cuda.device(self.dev):
            if st.current_stage == 0 and st.g == 1:
                self.t.forward_first(self.logits_t)
            else:
                self.t.forward(self._xt[st.xt_idx], st.current_stage, st.g, self.logits_t)
        st.stats["target_calls"] += 1
        st.target_calls += 1
        st.verified = True
        return self.logits_t[:2 * st.B * lsum * self.t.V].view(2 * st.B, lsum, self.t.V)

    def spec_accept(self, st: "SpecState"):
        """SDVAR.basic_token_matching (var.py:1160-1227) on the verified chunk: (n_accept, matched per stage)."""
        assert st.verified
        lad, cur, g = self.lad, st.current_stage, st.g
        mr = st.match
        with torch.cuda.device(self.dev):
            corr = self._buf("ids_corr", self.t.max_batch * self.lmax_t, torch.int64) if mr.token_level else None
            verify_accept(self.logits_t, st.B, st.glen, self.t.V, st.chunk_ts(cur, g), self.ids, lad.begin(cur), lad.L, st.thr, self.counts,
                          rule=mr, draft_logits=self._lazy.get("draft_logits") if mr.rule == "kl" else None, corrected_out=corr, rows=st.rows, s0=cur,
                          **st.gen_args(cur))
            self.counts_host.copy_(self.counts, non_blocking=False)            # the one host sync of the round
        c = self.counts_host.tolist()
        st.totals = st.round_totals(c, st.glen)
        if st.accept_scope == "global":            # batch-wide decision across ranks (reference-literal for one big batch)
            from . import dist as D
            n, _, _ = D.global_accept(c[:g], c[17:17 + g], st.thr, self.dev)
            # the DECISION is global; the counts handed back stay this rank's own: every statistic built from them (accepted / corrected tokens,
            # rounds[].matched) is per rank and summed once by dist.gather_counters - global counts here would be added world-size times
            return n, c[:g]
        return c[16], c[:g]

    def spec_correct(self, st: "SpecState", n_acc: int, matched: Sequence[int]) -> int:
        """Token-level partial acceptance (the 'partial accept / token-level rollback' item of var.py:1229-1243): stage cur + n_acc failed the
        batch threshold; keep its tokens that satisfy the rule, give the others the target's argmax (both already chosen by the verify kernel),
        rebuild that stage's f_hat snapshot and next-scale input from the corrected ids, and return the number of stages to commit."""
        lad, B, cur, j = self.lad, st.B, st.current_stage, n_acc
        s, l, lsum, off = cur + j, st.glen[j], sum(st.glen), sum(st.glen[:j])
        with torch.cuda.device(self.dev):
            corr = self._lazy["ids_corr"][:B * lsum].view(B, lsum)
            self.ids[:B, lad.begin(s):lad.begin(s) + l].copy_(corr[:, off:off + l])
            last = s == lad.S - 1
            self.q.next(s, self.ids[:, lad.begin(s):], lad.L, self.f_snap[j][:B], None if last else self.nxt[j], B, f_in=self.f_acc[:B] if j == 0 else self.f_snap[j - 1][:B])
        st.stats["corrected_tokens"] = st.stats.get("corrected_tokens", 0) + st.totals[j] - matched[j]          # under a mask: sampled tokens only
        st.stats["corrected_stages"] = st.stats.get("corrected_stages", 0) + 1
        return n_acc + 1

    def spec_commit(self, st: "SpecState", n_acc: int, forced: bool = False, accepted_tokens: Optional[int] = None):
        """SDVAR.update_state_with_accepted_tokens (var.py:1245-1282) + `current_stage += n` (var.py:1349-1350), and the
        rollback of both KV caches to the accepted prefix (absent in the reference)."""
        lad, B, cur = self.lad, st.B, st.current_stage
        with torch.cuda.device(self.dev):
            if n_acc > 0:
                self.f_acc[:B].copy_(self.f_snap[n_acc - 1][:B])
                if not forced:
                    st.stats["accepted_tokens"] += sum(st.glen[:n_acc]) if accepted_tokens is None else accepted_tokens
                if cur + n_acc < lad.S:
                    self.nxt_cur.copy_(self.nxt[n_acc - 1])
                st.current_stage = cur = cur + n_acc
                st.accept_count += n_acc
            keep = lad.begin(cur) if cur < lad.S else lad.L
            self.d.kv_set_len(keep); self.t.kv_set_len(keep)
        st.drafted = st.verified = False

    def spec_end(self, st: "SpecState"):
        with torch.cuda.device(self.dev):
            self.d.kv_set_len(0); self.t.kv_set_len(0)
        st.stats["gamma_final"] = st.gamma

    def spec_decode(self, labels: torch.Tensor, cfg: float, gamma: int, top_k: int, top_p: float, noise: Noise, thr: float = 0.5,
                    trace: bool = False, run_ahead: bool = True, accept_scope: str = "shard", match: Optional[MatchRule] = None,
                    force_ids: Optional[torch.Tensor] = None, gen: Optional[torch.Tensor] = None, trusted_ids: bool = False) -> SampleResult:
        """The whole loop with the policy of var.py:1318-1372 (gamma only decreases; forced accept at gamma == 1; never break).
        run_ahead: once gamma has dropped to 1 the draft no longer waits for the verifier (see _spec_run_ahead); same results.
        accept_scope "global": the batch-wide decision is taken across ranks (one all-reduce per round), always in lock-step.
        `force_ids` (B, L) int64 and `gen` (B, L) uint8, both or neither, checked as plain_ar checks them: masked sampling.  The draft samples token (b, i) where
        gen[b, i] != 0 and takes force_ids[b, i] elsewhere; a forced token is no draft prediction, so the acceptance rate of a stage is matched / SAMPLED tokens of
        the batch, a stage without a sampled token is accepted, and rounds[].total, stats["sampled_tokens"] and corrected_tokens count sampled tokens only.  The
        overlap paths are kept.  Without a mask the launches and the results are those of the unmasked loop."""
        st = self.spec_begin(labels, cfg, gamma, top_k, top_p, noise, thr, match, force_ids=force_ids, gen=gen, trusted_ids=trusted_ids, who="spec_decode")
        st.accept_scope = accept_scope
        run_ahead = run_ahead and st.match.basic        # the richer rules run in lock-step
        res = SampleResult(ids=self.ids[:st.B], f_hat=self.f_acc[:st.B], stats=st.stats)
        optimistic = False                     # speculate on acceptance only after a round that was accepted in full
        while st.current_stage < st.total_stages:
            if run_ahead and st.accept_scope == "shard" and not trace:
                if st.gamma == 1:
                    self._spec_run_ahead(st)
                    break
                if optimistic:
                    self._spec_optimistic(st)
                    optimistic = False
                    continue
            cur = st.current_stage
            g = self.spec_draft(st)
            lg = self.spec_verify_forward(st)
            if trace:
                res.trace.setdefault("target_logits", []).append((cur, g, lg.clone()))
                res.trace.setdefault("draft_ids", []).append(self.ids[:st.B, self.lad.begin(cur):self.lad.begin(cur) + sum(st.glen)].clone())      # the round's drafts (B, lsum)
            n_acc, matched = self.spec_accept(st)
            forced, acc_tok = False, None
            if n_acc < g and st.match.token_level:
                acc_tok = sum(st.glen[:n_acc]) + matched[n_acc]
                n_acc = self.spec_correct(st, n_acc, matched)
            elif n_acc == 0:                                                    # var.py:1353-1364
                if st.gamma > 1:
                    st.gamma -= 1
                else:
                    n_acc, forced = 1, True
                    st.stats["forced_accepts"] += 1
            st.stats["rounds"].append(dict(stage=cur, g=g, matched=matched, total=st.totals, n_accept=n_acc, forced=forced))
            optimistic = n_acc == g and not forced
            self.spec_commit(st, n_acc, forced, acc_tok)
        self.spec_end(st)
        if st.forced is not None:              # every stage is committed by exactly one round, as one of its first n_accept stages
            st.stats["sampled_tokens"] = sum(sum(r["total"][:r["n_accept"]]) for r in st.stats["rounds"])
        self._f16_stats(res.stats)
        if _GUARD_ON:
            res.stats["f16x2_guard"] = f16x2_guard_collect()
        return res

    def _ensure_second_stream(self):
        if self._verify_stream is None:
            self._verify_stream = torch.cuda.Stream(device=self.dev, priority=torch.cuda.current_stream(self.dev).priority)
            self._xt[1] = torch.empty_like(self.x_t)
        if self._fs[1] is None:
            self._fs[1] = [torch.zeros_like(t) for t in self._fs[0]]
            self._nx[1] = [torch.empty_like(t) for t in self._nx[0]]
            self._f_prev = [torch.zeros_like(self.f_acc) for _ in range(2)]
            self._nxt_prev = [torch.empty_like(self.nxt_cur) for _ in range(2)]
        return self._verify_stream

    def _spec_optimistic(self, st: "SpecState"):
        """gamma > 1 and the previous round was accepted in full: draft the next round before the verdict on the current one is
        known.  Every round is committed as if accepted (per-round slots keep its f_hat snapshots, next-stage inputs and the
        state before it); the verifier runs on the second stream, its counters come back through pinned memory, and the host
        reads the verdict of round r after it has enqueued round r+1.  A verdict short of full acceptance rolls the state back
        to what the lock-step loop would hold (accepted prefix, gamma policy, draw counter, both KV cursors), discards the
        speculative round and returns to lock-step.  Results and counters equal the lock-step loop's."""
        lad, B, V, S = self.lad, st.B, self.t.V, self.lad.S
        with torch.cuda.device(self.dev):
            D = torch.cuda.current_stream(self.dev)
            T = self._ensure_second_stream()
            T.wait_stream(D)
            t_done, pend, n = [], None, 0
            while st.current_stage < S and st.gamma > 1:
                slot = n & 1
                if n >= 2:
                    D.wait_event(t_done[n - 2])                 # last verification that read this slot's target input
                self._slot = st.xt_idx = slot
                self._f_prev[slot][:B].copy_(self.f_acc[:B]); self._nxt_prev[slot].copy_(self.nxt_cur)
                cur = st.current_stage
                g = self.spec_draft(st)
                ready = torch.cuda.Event(); ready.record(D)
                T.wait_event(ready)
                row = self._row; self._row += 1
                with torch.cuda.stream(T):
                    self.t.forward(self._xt[slot], cur, g, self.logits_t)
                    verify_accept(self.logits_t, B, st.glen, V, st.chunk_ts(cur, g), self.ids, lad.begin(cur), lad.L, st.thr,
                                  self.counts_ra[row], rows=st.rows, s0=cur, **st.gen_args(cur))
                    self._counts_pin[row].copy_(self.counts_ra[row], non_blocking=True)
                    ev = torch.cuda.Event(); ev.record(T); t_done.append(ev)
                st.stats["target_calls"] += 1
                st.target_calls += 1
                info = dict(cur=cur, g=g, glen=list(st.glen), slot=slot, draw_after=st.draw, row=row, ev=ev)
                self.spec_commit(st, g, forced=True)            # optimistic: all g stages; the counters are settled by _resolve
                n += 1
                if pend is not None and not self._resolve(st, pend):
                    st.stats["draft_stage_calls"] -= info["g"]  # the speculative round is discarded, as if never drafted
                    st.stats["target_calls"] -= 1
                    st.target_calls -= 1
                    st.stats["discarded_speculative_rounds"] = st.stats.get("discarded_speculative_rounds", 0) + 1
                    pend = None
                    break
                pend = info
            if pend is not None:
                self._resolve(st, pend)
            self._slot = st.xt_idx = 0
            D.wait_stream(T)

    def _resolve(self, st: "SpecState", p: dict) -> bool:
        """Verdict of an optimistically committed round; rolls back when it was not accepted in full.  True = accepted in full."""
        lad, B = self.lad, st.B
        p["ev"].synchronize()
        c = self._counts_pin[p["row"]].tolist()
        g, glen, n_acc, matched = p["g"], p["glen"], c[16], c[:p["g"]]
        st.stats["accepted_tokens"] += sum(glen[:n_acc])
        st.stats["rounds"].append(dict(stage=p["cur"], g=g, matched=matched, total=st.round_totals(c, glen), n_accept=n_acc, forced=False))
        if n_acc == g:
            return True
        slot = p["slot"]
        if n_acc > 0:
            self.f_acc[:B].copy_(self._fs[slot][n_acc - 1][:B])
            self.nxt_cur.copy_(self._nx[slot][n_acc - 1])
        else:
            self.f_acc[:B].copy_(self._f_prev[slot][:B]); self.nxt_cur.copy_(self._nxt_prev[slot])
            st.gamma -= 1                                      # var.py:1353-1356 (this path only runs with gamma > 1)
        st.accept_count -= (st.current_stage - (p["cur"] + n_acc))
        st.current_stage = p["cur"] + n_acc
        st.draw = p["draw_after"]
        keep = lad.begin(st.current_stage)
        self.d.kv_set_len(keep); self.t.kv_set_len(keep)
        st.drafted = st.verified = False
        return False

    def _spec_run_ahead(self, st: "SpecState"):
        """The tail of the loop at gamma == 1.  There a round always advances one stage with the DRAFT's tokens - accepted, or
        force-accepted (var.py:1357-1364) - so the verify result only feeds the counters, and since gamma never grows again
        this holds to the end.  The draft of stage s+1 therefore need not wait for the verification of stage s: the target
        forwards + acceptance scans run on a second HIP stream one round behind (target input double-buffered, one counter row
        per round, read back once at the end); the launch-bound early stages of one model fill the gaps of the other."""
        lad, B, V = self.lad, st.B, self.t.V
        with torch.cuda.device(self.dev):
            D = torch.cuda.current_stream(self.dev)
            T = self._ensure_second_stream()
            T.wait_stream(D)                                   # earlier rounds ran the target on the caller's stream
            row0 = self._row
            t_done, meta = [], []
            r = 0
            while st.current_stage < st.total_stages:
                cur = st.current_stage
                if r >= 2:
                    D.wait_event(t_done[r - 2])                # the target forward that last used this input buffer
                st.xt_idx = r & 1
                g = self.spec_draft(st)                        # gamma == 1: one stage
                ready = torch.cuda.Event(); ready.record(D)
                T.wait_event(ready)
                with torch.cuda.stream(T):
                    if cur == 0:
                        self.t.forward_first(self.logits_t)
                    else:
                        self.t.forward(self._xt[st.xt_idx], cur, 1, self.logits_t)
                    verify_accept(self.logits_t, B, st.glen, V, st.chunk_ts(cur, 1), self.ids, lad.begin(cur), lad.L, st.thr, self.counts_ra[row0 + r],
                                  rows=st.rows, s0=cur, **st.gen_args(cur))
                    ev = torch.cuda.Event(); ev.record(T); t_done.append(ev)
                st.stats["target_calls"] += 1
                st.target_calls += 1
                meta.append((cur, g, list(st.glen)))
                self.spec_commit(st, 1, forced=True)           # data movement of an accepted and of a forced stage is the same; counters below
                r += 1
            st.xt_idx = 0
            D.wait_stream(T)
            self._row = row0 + r
            c = self.counts_ra[row0:row0 + r].cpu().tolist()   # the one host sync of the tail
        for (cur, g, glen), row in zip(meta, c):
            n_acc, matched, forced = row[16], row[:g], False
            if n_acc == 0:
                n_acc, forced = 1, True
                st.stats["forced_accepts"] += 1
            else:
                st.stats["accepted_tokens"] += sum(glen[:n_acc])
            st.stats["rounds"].append(dict(stage=cur, g=g, matched=matched, total=st.round_totals(row, glen), n_accept=n_acc, forced=forced))


@dataclass
class SpecState:
    """Run state of the speculative loop; the public counters carry the reference's names (var.py:912-943)."""
    sampler: "Sampler"
    labels: torch.Tensor
    B: int
    cfg: float
    gamma: int
    top_k: int
    top_p: float
    noise: Noise
    thr: float
    total_stages: int
    patch_nums: tuple
    current_stage: int = 0
    accept_count: int = 0
    reject_count: int = 0
    target_calls: int = 0
    more_smooth: bool = False                     # stored and never read on the speculative path, as in the reference (var.py:1315 vs 949-1024)
    match: "MatchRule" = field(default_factory=lambda: MatchRule())
    accept_scope: str = "shard"                   # "shard": this process decides alone; "global": all-reduce of the match counts
    draw: int = 0
    xt_idx: int = 0                               # which target input buffer the current round uses (run-ahead double buffer)
    g: int = 0
    glen: list = field(default_factory=list)
    drafted: bool = False
    verified: bool = False
    stats: Dict[str, object] = field(default_factory=lambda: dict(target_calls=0, draft_stage_calls=0, forced_accepts=0, accepted_tokens=0, rounds=[], gamma_final=0))
    rows: Optional["RowParams"] = None            # per-image (cfg, top_k, top_p, seed, index) tables; None = the scalar fields above
    forced: Optional[tuple] = None                # masked sampling: (gen (B, L) uint8, force_ids (B, L) int64); None = no mask
    totals: list = field(default_factory=list)    # tokens per stage that the last spec_accept counted (under a mask: the sampled ones)

    def gen_args(self, cur: int) -> dict:
        """The mask arguments of verify_accept for a chunk that starts at stage `cur`; empty without a mask (the unforced entry points)."""
        if self.forced is None:
            return {}
        lad = self.sampler.lad
        return dict(gen=self.forced[0], gen_off=lad.begin(cur), gen_stride=lad.L)

    def round_totals(self, counts: Sequence[int], glen: Sequence[int]) -> list:
        """rounds[].total: under a mask the sampled tokens per stage, read from the counter row of the verification; B * l without one."""
        return [int(x) for x in counts[17:17 + len(glen)]] if self.forced is not None else [self.B * n for n in glen]

    def chunk_ts(self, cur: int, g: int):
        """The scalar CFG factors of stages cur .. cur + g - 1 (unused when `rows` carries them per image)."""
        return [] if self.rows is not None else [self.sampler.lad.cfg_t(self.cfg, cur + j) for j in range(g)]

    @property
    def draft_f_hat(self) -> torch.Tensor:        # f_hat of the accepted prefix (after the last commit)
        return self.sampler.f_acc[:self.B]

    @property
    def target_f_hat(self) -> torch.Tensor:
        return self.sampler.f_acc[:self.B]
