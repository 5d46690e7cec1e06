"""Drop-in HIP operators for the reference's module-level operator slots (models/basic_var.py:15-30).

The reference calls four module globals on its hot path: `flash_attn_func` / `memory_efficient_attention` / `slow_attn` (basic_var.py:113-117) and
`fused_mlp_func` (basic_var.py:46-50, captured per FFN at :36).  This module provides all four on the library's kernels, for a
maintainer of the reference who wants the kernels without adopting the sampling loop:

    from sdvar_amd import seam
    import models.basic_var as basic_var
    seam.install(basic_var, model)          # slots + the fused_mlp_func every FFN captured at construction
    seam.enable_flash(basic_var, model)     # optional: flash_attn_func for the cached, unmasked calls under autocast (fp16 / bf16 operands)

    seam.install_amp(basic_var, model)      # a model run under torch.autocast: the two lines above + slow_attn_amp for the MASKED calls (half / mixed operands)

    seam.install_train(basic_var, model)    # fp32 TRAINING: slow_attn_grad (HIP forward + backward under autograd); the FFN goes back to the reference's own fc2(act(fc1(x)))
    seam.install_train(basic_var, model, ffn=True)      # ... and fused_mlp_func_grad: the FFN's forward and backward on HIP too

    seam.install_train_amp(basic_var, model)    # TRAINING under torch.autocast (fp16 + GradScaler, or bf16): slow_attn_amp_grad + flash_attn_func_grad

    seam.install_train_amp(basic_var, model, ffn="half")     # ... and fused_mlp_func_amp_grad: the FFN on the half matrix cores too, forward and backward
    seam.install_amp(basic_var, model, ffn_half=True)        # inference under autocast with fused_mlp_func_amp in the FFN slots

    seam.install_trainer(trainer)           # the VARTrainer's train_loss / val_loss (trainer.py:37-38): label-smoothed cross-entropy, HIP forward + backward

    seam.install_train(basic_var, model, ffn=True, adaln=True)        # ... and the blocks' adaLN modulations and gated residual lines (adaln_modulate / gated_residual)
    seam.install_train_amp(basic_var, model, ffn="half", adaln=True)  # the same under autocast; seam.uninstall_adaln(model) takes the bound forwards off again

    seam.install_train(basic_var, model, ffn=True, adaln=True, qknorm=True)   # ... and attn_l2_norm's QK normalisation between the QKV GEMM and the attention (qk_l2norm)
    seam.install_train_amp(basic_var, model, ffn="half", adaln=True, qknorm=True)    # the same under autocast; seam.install_qknorm(model) alone for inference,
                                                                                     # seam.uninstall_qknorm(model) takes the bound forwards off again

    seam.install_train(basic_var, model, ffn=True, adaln=True, qknorm=True, linears=True)    # ... and every dense nn.Linear (mat_qkv, proj, ada_lin, word_embed, head):
    seam.install_train_amp(basic_var, model, ffn="half", adaln=True, qknorm=True, linears=True)   # linear_grad / linear_amp_grad, picked per call; seam.install_linears(model)
                                                                                     # alone for inference, seam.uninstall_linears(model) takes them off again

    seam.install_train(basic_var, model, ffn=True, adaln=True, qknorm=True, linears=True, cond=True)    # ... and the conditioning path Sequential(SiLU, Linear) of every
    seam.install_train_amp(basic_var, model, ffn="half", adaln=True, qknorm=True, linears=True, cond=True)   # block and of the head norm: ada_lin, a skinny kernel of its
                                                                                     # own (batches of at most 64 rows); seam.install_cond(model) alone for inference,
                                                                                     # seam.uninstall_cond(model) takes the bound forwards off again

    seam.install_optimizer(var_opt)         # the AmpOptimizer's AdamW (utils/amp_sc.py): unscale + clip_grad_norm_ + AdamW.step as two passes on HIP (seam.AdamW)

Inference only, except slow_attn_grad / memory_efficient_attention_grad (fp32 operands; backward = sdvar_op_sdpa_bwd, no gradient for the mask, no double backward),
slow_attn_amp_grad / memory_efficient_attention_amp_grad / flash_attn_func_grad (the half and mixed operands of autocast; backward = sdvar_op_sdpa_h_bwd) and
fused_mlp_func_grad (fp32 operands; backward = four GEMMs on operands from csrc/mlp_bwd.hip, no double backward) and fused_mlp_func_amp_grad (autocast's half dtype;
sdvar_op_gemm_h on operands from csrc/mlp_half.hip):
no backward, no dropout, head dim 64.  `slow_attn`, `memory_efficient_attention` and `fused_mlp_func` take fp32 operands only;
`flash_attn_func` takes fp16 or bf16 operands only (and no mask); `slow_attn_amp` / `memory_efficient_attention_amp` take a half value with query and key each
half or fp32, and masks.  Anything else raises SdvarError - there is no fall-back to torch.
Torch is used for device memory and the current stream only; bool masks go to the kernel as bytes.
cross_entropy / CrossEntropyLoss / install_trainer are the trainer's loss slots (trainer.py:37-38): label-smoothed cross-entropy on float32 logits, differentiable
(forward = sdvar_xent_train_fwd, backward = sdvar_xent_train_bwd; one float per row saved, no double backward).
adaln_modulate / gated_residual are the glue of a block (basic_var.py:152-159, 172-174; the reference's unfilled `fused_add_norm_fn`, :149): the modulated LayerNorm
and the gated residual line with DropPath's per-image factor, float32 x with float32 or half modulation vectors and branch outputs, differentiable
(csrc/adaln_train.hip: sdvar_op_adaln_fwd / _bwd, sdvar_op_gate_add_fwd / _bwd; x and scale, resp. y, gamma and row_scale saved; no double backward).  A half
scale is widened to float32 before the + 1, where torch's scale.add(1) rounds the sum to half.
qk_l2norm is what SelfAttention.forward does between the QKV GEMM and the attention call when attn_l2_norm is on (basic_var.py:93-105): bias add, per-head L2
normalisation of q and k and the learnt per-head scale of q, one kernel per direction (csrc/qknorm_train.hip: sdvar_op_qknorm_fwd / _bwd; qkv, the biases and the scale
parameter saved; no double backward).  The float32 master bias is added in float32 to the GEMM's output, where autocast rounds acc + half(bias) to half inside the GEMM.
linear / linear_grad / linear_amp / linear_amp_grad are F.linear on the operator GEMMs of the configured mode, resp. on the half matrix cores (csrc/linear_train.hip:
sdvar_op_grad_operands / _h read dy once for both gradient GEMMs and db; the amp path saves the forward's half operand of x, 2 M K bytes; no double backward).
ada_lin is Sequential(SiLU, Linear(D, 6C)) of a block and Sequential(SiLU, Linear(D, 2C)) of the head norm (basic_var.py:147, 156, 170, 173): M is the batch, all the
bytes are in W, so it streams W once per direction in plain float32 vector code with the SiLU folded into the read of cond (csrc/cond_train.hip: sdvar_op_cond_lin_fwd /
_bwd; cond and the weight saved; no operand planes, no weight-operand cache, independent of seam.configure; no double backward).  The float32 sum dy W enters the SiLU
derivative unrounded, where autocast rounds it to half first.
AdamW / install_optimizer are the optimizer step outside the blocks (utils/amp_sc.py:39-75, train.py:118): torch's decoupled AdamW on float32 parameters with the
GradScaler's unscale, clip_grad_norm_'s global norm and the non-finite skip folded into two passes over the tensors (csrc/optim.hip: sdvar_optim_grad_stats,
sdvar_optim_adamw_step); the norm stays on the device as `global_grad_norm`, the reference's late-clipping slot.  The gradients are read, never modified.

Operand rule of the attention slots: every token row 16-byte aligned (data_ptr % 16 == 0, every stride a multiple of 4 elements, last stride 1).  The
reference's permuted views of one (B, L, 3, H, 64) buffer, its (B, H, L, 64) caches and xformers' (B, L, H, 64) tensors all meet it and are
read in place; a tensor that does not is copied once into a fresh dense tensor.
A query row whose keys are ALL masked has no defined value (NaN); other rows are unaffected.
The same rule holds for flash_attn_func's half operands with 2-byte elements: data_ptr % 16 == 0, every stride a multiple of 8 elements, last stride 1 (the
unbind(dim=2) views of one (B, L, 3, H, 64) buffer and torch.cat caches meet it).
"""
from __future__ import annotations

import ctypes as C
import math
import types
from collections import OrderedDict
from typing import Optional

import torch

from . import engine as E
from .engine import SdvarError

__all__ = ["configure", "slow_attn", "memory_efficient_attention", "flash_attn_func", "slow_attn_amp", "memory_efficient_attention_amp", "fused_mlp_func", "install",
           "enable_flash", "install_amp", "clear_caches", "slow_attn_grad", "memory_efficient_attention_grad", "install_train",
           "fused_mlp_func_grad", "slow_attn_amp_grad", "memory_efficient_attention_amp_grad", "flash_attn_func_grad", "install_train_amp",
           "cross_entropy", "CrossEntropyLoss", "install_trainer", "fused_mlp_func_amp", "fused_mlp_func_amp_grad", "adaln_modulate", "gated_residual",
           "uninstall_adaln", "qk_l2norm", "install_qknorm", "uninstall_qknorm", "AdamW", "install_optimizer", "linear", "linear_grad", "linear_amp", "linear_amp_grad",
           "install_linears", "uninstall_linears", "ada_lin", "install_cond", "uninstall_cond", "cond_serves"]

_gemm_mode = E.DEFAULT_GEMM_MODE
# (data_ptr, _version, shape, strides) -> (mask, skip map).  The entry holds the mask itself: while it is cached its memory cannot be handed to another tensor, so
# a key can never describe two different masks.  Small on purpose: a model has a handful of masks (teacher forcing: one; the hand-off sampler: five).
_SKIP_MAPS: "OrderedDict[tuple, tuple]" = OrderedDict()
_SKIP_MAPS_MAX = 8
# (kind, mode, data_ptr, shape) -> (weight, _version, planes, scale): GEMM operand planes of a weight ("n": as stored, none in mode f32; "t": of its transpose, for the
# backward).  A weight updated in place replaces its own entry.  A d30 model has 60 FFN weights; with the dense linears (linears=True) a d36 model holds
# 36 blocks x 5 weights x 2 kinds + head and word_embed = 364 entries, and an LRU visited in model order that is one entry short misses on EVERY access.
_WEIGHT_PLANES: "OrderedDict[tuple, tuple]" = OrderedDict()
_WEIGHT_PLANES_MAX = 512


def configure(gemm_mode: Optional[str] = None) -> None:
    """GEMM arithmetic of fused_mlp_func: one of engine.GEMM_MODES (default: the library's, engine.DEFAULT_GEMM_MODE).  'f16x2' saturates activations
    (x and the GELU output) at +-65504 and loses relative precision below ~1e-3; 'bf16x3' and 'f32' have no range limit."""
    global _gemm_mode
    if gemm_mode is not None:
        if gemm_mode not in E.GEMM_MODES:
            raise SdvarError(f"seam.configure: gemm_mode {gemm_mode!r} is not one of {E.GEMM_MODES}")
        _gemm_mode = gemm_mode


def clear_caches() -> None:
    _SKIP_MAPS.clear()
    _WEIGHT_PLANES.clear()


_HALF_DTYPES = {torch.float16: 1, torch.bfloat16: 2}          # sdvar_op_sdpa_h's dtype codes


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _gpu_tensor(who: str, name: str, t) -> None:
    if not isinstance(t, torch.Tensor):
        raise SdvarError(f"{who}: {name} is not a tensor")
    if not t.is_cuda:
        raise SdvarError(f"{who}: {name} is a CPU tensor (the kernels run on the GPU; there is no CPU path)")


def _token_rows(t: torch.Tensor) -> torch.Tensor:
    """A 4-D operand as the attention kernels read its token rows: t itself when every row is 16-byte aligned (last stride 1, data_ptr % 16 == 0, every other
    stride a multiple of 16 bytes - 4 float32 elements, 8 half ones), else ONE fresh dense copy.  clone, not .contiguous(): a dense tensor at a misaligned address
    (a slice of a flat buffer) is its own .contiguous() and would come back as itself."""
    s0, s1, s2, last = t.stride()
    m = 4 if t.dtype == torch.float32 else 8
    if last == 1 and t.data_ptr() % 16 == 0 and s0 % m == 0 and s1 % m == 0 and s2 % m == 0:
        return t
    return t.clone(memory_format=torch.contiguous_format)


def _skip_map(mask: torch.Tensor, kind: int, bstr, Bb: int, Hb: int, Lq: int, Lk: int) -> torch.Tensor:
    key = (mask.data_ptr(), mask._version, tuple(mask.shape), tuple(mask.stride()), mask.dtype, Lq)       # Lq: a (.., 1, Lk) mask broadcasts over any number of rows
    hit = _SKIP_MAPS.get(key)
    if hit is not None:
        _SKIP_MAPS.move_to_end(key)
        return hit[1]
    smap = torch.empty(((Lq + 127) // 128) * ((Lk + 63) // 64), dtype=torch.uint8, device=mask.device)
    E._check(E.load_library().sdvar_op_sdpa_skip_map(_p(mask), kind, bstr, Bb, Hb, Lq, Lk, _p(smap), E._stream()))
    _SKIP_MAPS[key] = (mask, smap)
    while len(_SKIP_MAPS) > _SKIP_MAPS_MAX:
        _SKIP_MAPS.popitem(last=False)
    return smap


_NO_MASK = (None, 0, None, None)


def _mask_args(who: str, mask, B: int, H: int, Lq: int, Lk: int, half):
    """(mask as the kernel reads it, bias kind, bias strides, skip map) of an attention mask; all None / 0 without one.  half = the operands' half dtype when the kernel
    also takes an additive mask of that dtype (kind 3; the skip map's kind is 3 for fp16, 4 for bf16), else None."""
    if mask is None:
        return _NO_MASK
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda:
        raise SdvarError(f"{who}: the mask is a CPU tensor (or no tensor)")
    if mask.dtype == torch.bool:
        kind = skind = 2
    elif mask.dtype == torch.float32:
        kind = skind = 1
    elif half is not None and mask.dtype == half:
        kind, skind = 3, 2 + _HALF_DTYPES[half]
    elif half is not None and mask.dtype in _HALF_DTYPES:
        raise SdvarError(f"{who}: the mask is {mask.dtype} but the operands are {half}; a half-precision mask must have the operands' dtype")
    elif half is not None:
        raise SdvarError(f"{who}: the mask is {mask.dtype}; float32 (additive), {half} (additive) or bool (keep) only")
    else:
        raise SdvarError(f"{who}: the mask is {mask.dtype}; float32 (additive) or bool (keep) only")
    if mask.dim() > 4:
        raise SdvarError(f"{who}: the mask has {mask.dim()} dims")
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    while mask.dim() < 4:
        mask = mask.unsqueeze(0)
    mb, mh, mq, mk = mask.shape
    if mb not in (1, B) or mh not in (1, H) or mq not in (1, Lq) or mk != Lk:
        raise SdvarError(f"{who}: a mask of shape {tuple(mask.shape)} does not broadcast to {(B, H, Lq, Lk)} (the key dimension must be materialised)")
    if mask.stride(3) != 1 and Lk > 1:
        mask = mask.contiguous()
    sb, sh, sr = (0 if n == 1 else s for n, s in zip(mask.shape[:3], mask.stride()[:3]))
    bstr = (C.c_int64 * 3)(sb, sh, sr)
    # the skip map looks at the bias's OWN batch / head slices (one where it broadcasts or is expanded), every one of the Lq rows
    smap = _skip_map(mask, skind, bstr, 1 if sb == 0 else B, 1 if sh == 0 else H, Lq, Lk)
    return mask, kind, bstr, smap


_QKV, _QKV_FLASH = ("query", "key", "value"), ("q", "k", "v")             # what the slots' signatures call their operands


def _attn_check(who: str, names, q, k, v, idx, policy: str, twin: Optional[str] = None, mask=None):
    """The operand check of every attention slot.  names: the slot's words for its operands; idx = positions of (batch, head, token) in their dims.  policy: "f32"
    (float32 only), "half" (three operands of one half dtype) or "mixed" (value fixes the half dtype, query and key are each that dtype or float32; three float32
    operands are the fp32 slots' case).  twin: None for a slot that has a backward, else the end of the refusal of an operand that requires grad - the slot's
    differentiable twin.  mask: the mask of a slot that has a backward, refused when it requires grad.  Returns (B, H, Lq, Lk, half): _mask_args' arguments, half =
    None for three float32 operands.  A call with several faults reports the one its slot has always reported first, hence the two places of the head dim and of the
    mask's check."""
    for name, t in zip(names, (q, k, v)):
        _gpu_tensor(who, name, t)
        if policy == "f32":
            if t.dtype != torch.float32:
                hint = (" - the autocast slots (slow_attn_amp, flash_attn_func) have no backward; use slow_attn_amp_grad / flash_attn_func_grad"
                        if twin is None and t.dtype in _HALF_DTYPES else "")
                raise SdvarError(f"{who}: {name} is {t.dtype}; only float32 operands are supported{hint}")
        elif policy == "half":
            if t.dtype == torch.float32:
                raise SdvarError(f"{who}: {name} is torch.float32; this slot takes float16 / bfloat16 operands - use slow_attn or memory_efficient_attention for float32")
            if t.dtype not in _HALF_DTYPES:
                raise SdvarError(f"{who}: {name} is {t.dtype}; only float16 and bfloat16 operands are supported")
        elif t.dtype != torch.float32 and t.dtype not in _HALF_DTYPES:
            raise SdvarError(f"{who}: {name} is {t.dtype}; only float32, float16 and bfloat16 operands are supported")
        if twin is not None and t.requires_grad and torch.is_grad_enabled():
            raise SdvarError(f"{who}: {name} requires grad and grad mode is on; no backward exists (call under torch.no_grad(){twin})")
        if t.dim() != 4:
            raise SdvarError(f"{who}: {name} has {t.dim()} dims, expected 4")
        if policy != "half" and t.shape[-1] != 64:
            raise SdvarError(f"{who}: head dim {t.shape[-1]}; only 64 is supported")
    mask_grad = isinstance(mask, torch.Tensor) and mask.requires_grad and torch.is_grad_enabled()
    if mask_grad and policy == "mixed":
        raise SdvarError(f"{who}: the mask requires grad; there is no gradient for the mask")
    half = None
    if policy == "half":
        if q.dtype != k.dtype or q.dtype != v.dtype:
            raise SdvarError(f"{who}: mixed dtypes: q {q.dtype}, k {k.dtype}, v {v.dtype} (all three must be float16 or all three bfloat16)")
        for t in (q, k, v):
            if t.shape[-1] != 64:
                raise SdvarError(f"{who}: head dim {t.shape[-1]}; only 64 is supported")
        half = v.dtype
    elif policy == "mixed" and v.dtype == torch.float32:
        if q.dtype != torch.float32 or k.dtype != torch.float32:
            raise SdvarError(f"{who}: value is torch.float32 next to query {q.dtype} / key {k.dtype}: value fixes the dtype of the product and of the result, and a "
                             "float32 value only goes with float32 query and key")
    elif policy == "mixed":
        half = v.dtype
        for name, t in zip(names, (q, k)):
            if t.dtype != half and t.dtype != torch.float32:
                raise SdvarError(f"{who}: mixed half dtypes: {name} is {t.dtype}, value is {half} (query and key must each be {half} or float32)")
    ib, ih, it = idx
    B, H, Lq, Lk = q.shape[ib], q.shape[ih], q.shape[it], k.shape[it]
    # the float32 entries refuse an empty batch themselves; the half slots have always done it here
    if k.shape != v.shape or k.shape[ib] != B or k.shape[ih] != H or Lq < 1 or Lk < 1 or (half is not None and (B < 1 or H < 1)):
        raise SdvarError(f"{who}: shapes do not match: {names[0]} {tuple(q.shape)}, {names[1]} {tuple(k.shape)}, {names[2]} {tuple(v.shape)}")
    if q.device != k.device or q.device != v.device:
        raise SdvarError(f"{who}: operands live on different devices")
    if mask_grad:
        raise SdvarError(f"{who}: the mask requires grad; there is no gradient for the mask")
    return B, H, Lq, Lk, half


def _wants_grad(q, k, v) -> bool:
    return torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad)


def _sdpa_launch(q, k, v, idx, scale: float, margs, dims, want_lse: bool):
    """The forward launch of every attention slot, on checked operands.  margs: _mask_args' result; dims: _attn_check's.  Allocates the (B, Lq, H, 64) output (and the
    (B, H, Lq) log-sum-exp rows) and picks the entry: float32 operands -> sdvar_op_sdpa / _lse; half operands without a mask, without a float32 query or key and
    without lse -> sdvar_op_sdpa_h (what flash_attn_func launches: the same bits); any other -> sdvar_op_sdpa_hm / _hm_lse.  Returns (q, k, v) as they were read
    (in place, or each one's copy), out and lse."""
    B, H, Lq, Lk, half = dims
    mask, kind, bstr, smap = margs
    q, k, v = _token_rows(q), _token_rows(k), _token_rows(v)
    out = torch.empty((B, Lq, H, 64), dtype=half or torch.float32, device=q.device)
    lse = torch.empty((B, H, Lq), dtype=torch.float32, device=q.device) if want_lse else None
    (ib, ih, it), sq, sk, sv, so = idx, q.stride(), k.stride(), v.stride(), out.stride()
    strides = (C.c_int64 * 12)(sq[ib], sq[ih], sq[it], sk[ib], sk[ih], sk[it], sv[ib], sv[ih], sv[it], so[0], so[2], so[1])
    lib = E.load_library()
    outs = (_p(out), _p(lse)) if want_lse else (_p(out),)
    tail = (B, H, Lq, Lk, 64, float(scale), E._stream())
    if half is None:
        entry = lib.sdvar_op_sdpa_lse if want_lse else lib.sdvar_op_sdpa
        rc = entry(_p(q), _p(k), _p(v), *outs, strides, _p(mask), kind, bstr, _p(smap), *tail)
    else:
        qf, kf = int(q.dtype == torch.float32), int(k.dtype == torch.float32)
        if kind == 0 and not qf and not kf and not want_lse:
            rc = lib.sdvar_op_sdpa_h(_p(q), _p(k), _p(v), _p(out), strides, _HALF_DTYPES[half], *tail)
        else:
            entry = lib.sdvar_op_sdpa_hm_lse if want_lse else lib.sdvar_op_sdpa_hm
            rc = entry(_p(q), _p(k), _p(v), *outs, strides, _HALF_DTYPES[half], qf, kf, _p(mask), kind, bstr, _p(smap), *tail)
    E._check(rc)
    return q, k, v, out, lse


def _sdpa(who: str, q, k, v, idx, scale: float, mask: Optional[torch.Tensor]) -> torch.Tensor:
    """The float32 inference slots.  idx = positions of (batch, head, token) in the operands' dims.  Returns the (B, Lq, H, 64) output buffer."""
    dims = _attn_check(who, _QKV, q, k, v, idx, "f32", twin="")
    return _sdpa_launch(q, k, v, idx, scale, _mask_args(who, mask, *dims), dims, False)[3]


def slow_attn(query, key, value, scale: float, attn_mask=None, dropout_p: float = 0.0):
    """The `slow_attn` slot (basic_var.py:25-30, called at :117): softmax(scale q k^T + attn_mask) v.  query (B, H, Lq, 64), key / value (B, H, Lk, 64) fp32 on the
    GPU, any strides meeting the alignment rule (read in place), else one fresh dense copy.  attn_mask: float32 additive or bool keep-mask, broadcastable to
    (B, H, Lq, Lk) with the key dimension materialised; views (mask[:, :, :ed, :ed]) are read in place.  Returns a (B, H, Lq, 64) VIEW of a (B, Lq, H, 64)
    buffer, so the caller's .transpose(1, 2).reshape(B, L, C) is free."""
    if dropout_p and dropout_p > 0:
        raise SdvarError("slow_attn: dropout_p > 0 is not supported (inference only)")
    return _sdpa("slow_attn", query, key, value, (0, 1, 2), scale, attn_mask).permute(0, 2, 1, 3)


def memory_efficient_attention(q, k, v, attn_bias=None, p: float = 0.0, scale: Optional[float] = None):
    """The xformers slot (basic_var.py:21, called at :115): q (B, Lq, H, 64), k / v (B, Lk, H, 64), attn_bias as for slow_attn ((B, H, Lq, Lk) or broadcastable);
    returns (B, Lq, H, 64).  The same kernel as slow_attn with other strides."""
    if p and p > 0:
        raise SdvarError("memory_efficient_attention: p > 0 (dropout) is not supported (inference only)")
    return _sdpa("memory_efficient_attention", q, k, v, (0, 2, 1), 1.0 / math.sqrt(64.0) if scale is None else scale, attn_bias)


class _SdpaFn(torch.autograd.Function):
    """softmax(scale q k^T + mask) v with a HIP backward, on checked operands (dims = _attn_check's result).  Three float32 operands: forward = sdvar_op_sdpa_lse,
    backward = one sdvar_op_sdpa_bwd call (csrc/attention_sdpa_bwd.hip).  Half / mixed operands: forward = sdvar_op_sdpa_hm_lse, backward = one sdvar_op_sdpa_h_bwd
    call (csrc/attention_sdpa_h_bwd.hip)."""

    @staticmethod
    def forward(ctx, q, k, v, mask, idx, scale, who, dims):
        margs = _mask_args(who, mask, *dims)
        q, k, v, out, lse = _sdpa_launch(q, k, v, idx, scale, margs, dims, True)
        mask, kind, bstr, smap = margs
        ctx.save_for_backward(q, k, v, out, lse, *(() if mask is None else (mask, smap)))
        ctx.sdpa = (idx, float(scale), kind, bstr, dims[:4], dims[4], who)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        idx, scale, kind, bstr, (B, H, Lq, Lk), half, who = ctx.sdpa
        if half is not None and dout.dtype != half:
            raise SdvarError(f"{who}: the gradient of the output is {dout.dtype} but the output is {half}; the backward reads dout in the output's dtype")
        q, k, v, out, lse, *rest = ctx.saved_tensors
        mask, smap = rest if rest else (None, None)
        dout = _token_rows(dout)
        dq, dk, dv = (torch.empty((B, L, H, 64), dtype=t.dtype, device=q.device) if need else None
                      for need, L, t in zip(ctx.needs_input_grad[:3], (Lq, Lk, Lk), (q, k, v)))
        if dq is None and dk is None and dv is None:
            return (None,) * 8
        delta = torch.empty(B * H * Lq, dtype=torch.float32, device=q.device)
        def bht(t, order=(0, 2, 1)):        # a tensor's (batch, head, token) strides; the (B, L, H, 64) buffers' order by default
            s = (0, 0, 0, 0) if t is None else t.stride()
            return s[order[0]], s[order[1]], s[order[2]]
        strides = (C.c_int64 * 24)(*bht(q, idx), *bht(k, idx), *bht(v, idx), *bht(out), *bht(dout), *bht(dq), *bht(dk), *bht(dv))
        ptrs = (_p(q), _p(k), _p(v), _p(out), _p(dout), _p(lse), _p(delta), _p(dq), _p(dk), _p(dv), strides)
        tail = (_p(mask), kind, bstr, _p(smap), B, H, Lq, Lk, 64, scale, E._stream())
        if half is None:
            E._check(E.load_library().sdvar_op_sdpa_bwd(*ptrs, *tail))
        else:
            E._check(E.load_library().sdvar_op_sdpa_h_bwd(*ptrs, _HALF_DTYPES[half], int(q.dtype == torch.float32), int(k.dtype == torch.float32), *tail))
        if idx == (0, 1, 2):                # (B, H, L, 64) operands: views of the (B, L, H, 64) buffers
            dq, dk, dv = (None if t is None else t.permute(0, 2, 1, 3) for t in (dq, dk, dv))
        return dq, dk, dv, None, None, None, None, None


def _sdpa_grad(who: str, q, k, v, idx, scale: float, mask) -> torch.Tensor:
    """The differentiable float32 attention slots.  idx = positions of (batch, head, token) in the operands' dims.  Returns the (B, Lq, H, 64) output buffer."""
    dims = _attn_check(who, _QKV, q, k, v, idx, "f32", mask=mask)
    if not _wants_grad(q, k, v):            # what the inference twin launches: the same bits, no LSE
        return _sdpa_launch(q, k, v, idx, scale, _mask_args(who, mask, *dims), dims, False)[3]
    return _SdpaFn.apply(q, k, v, mask, idx, scale, who, dims)


def slow_attn_grad(query, key, value, scale: float, attn_mask=None, dropout_p: float = 0.0):
    """slow_attn under autograd (the reference's trainer runs loss.backward() through basic_var.py:117): layouts, mask rules, alignment and copy-once rule and the returned
    (B, H, Lq, 64) view as for slow_attn.  With grad mode off, or no operand requiring grad, it IS slow_attn (same launch, same bits).  Otherwise the forward also
    writes the log-sum-exp rows (sdvar_op_sdpa_lse; the output bits do not change) and the backward is one sdvar_op_sdpa_bwd call on the fp32 matrix cores: no score
    matrix in memory, masked tiles skipped, deterministic.  Gradients come back as (B, H, L, 64) views of fresh dense (B, L, H, 64) buffers; only those autograd asks
    for are computed.  An upstream gradient that misses the alignment rule is copied once.  No dropout (the reference trains with attn_drop = 0), no gradient for the
    mask, no double backward, float32 only."""
    if dropout_p and dropout_p > 0:
        raise SdvarError("slow_attn_grad: dropout_p > 0 is not supported (the reference trains with attn_drop = 0)")
    return _sdpa_grad("slow_attn_grad", query, key, value, (0, 1, 2), scale, attn_mask).permute(0, 2, 1, 3)


def memory_efficient_attention_grad(q, k, v, attn_bias=None, p: float = 0.0, scale: Optional[float] = None):
    """memory_efficient_attention under autograd: q (B, Lq, H, 64), k / v (B, Lk, H, 64), attn_bias as for slow_attn_grad; returns (B, Lq, H, 64); gradients are dense
    (B, L, H, 64).  The same kernels as slow_attn_grad with other strides."""
    if p and p > 0:
        raise SdvarError("memory_efficient_attention_grad: p > 0 (dropout) is not supported (the reference trains with attn_drop = 0)")
    return _sdpa_grad("memory_efficient_attention_grad", q, k, v, (0, 2, 1), 1.0 / math.sqrt(64.0) if scale is None else scale, attn_bias)


def flash_attn_func(q, k, v, dropout_p: float = 0.0, softmax_scale: Optional[float] = None, causal: bool = False, window_size=(-1, -1), softcap: float = 0.0,
                    alibi_slopes=None, deterministic: bool = False, return_attn_probs: bool = False):
    """The `flash_attn_func` slot (flash-attn's signature; basic_var.py:23, called at :113 when no mask is passed and qkv is not fp32): softmax(softmax_scale q k^T) v.
    q (B, Lq, H, 64), k / v (B, Lk, H, 64), all three float16 or all three bfloat16 on the GPU; operands meeting the alignment rule are read in place, any other is
    copied once into a dense, freshly allocated tensor.  softmax_scale=None means 1/sqrt(64).  Returns a contiguous (B, Lq, H, 64) tensor of the operand dtype.  fp32 accumulation, the
    softmax weights rounded to the operand dtype (nearest even) for the P V product; deterministic always (`deterministic` is accepted and ignored)."""
    who = "flash_attn_func"
    _flash_options(who, dropout_p, causal, window_size, softcap, alibi_slopes, return_attn_probs, False)
    dims = _attn_check(who, _QKV_FLASH, q, k, v, (0, 2, 1), "half", twin=", or use flash_attn_func_grad")
    return _sdpa_launch(q, k, v, (0, 2, 1), 1.0 / math.sqrt(64.0) if softmax_scale is None else softmax_scale, _NO_MASK, dims, False)[3]


def _flash_options(who: str, dropout_p, causal, window_size, softcap, alibi_slopes, return_attn_probs, grad: bool) -> None:
    """The rejections of flash-attn's own keywords; grad = the caller has a backward."""
    if dropout_p and dropout_p > 0:
        raise SdvarError(f"{who}: dropout_p > 0 is not supported " + ("(the reference trains with attn_drop = 0)" if grad else "(inference only)"))
    if causal:
        raise SdvarError(f"{who}: causal=True is not supported (the reference's cached calls pass no mask)")
    if window_size is not None and tuple(window_size) != (-1, -1):
        raise SdvarError(f"{who}: window_size {tuple(window_size)} is not supported (only (-1, -1), no sliding window)")
    if softcap:
        raise SdvarError(f"{who}: softcap {softcap} is not supported (only 0)")
    if alibi_slopes is not None:
        raise SdvarError(f"{who}: alibi_slopes is not supported")
    if return_attn_probs:
        raise SdvarError(f"{who}: return_attn_probs=True is not supported (no score matrix is ever written)")


def _sdpa_amp(who: str, q, k, v, idx, scale: float, mask) -> torch.Tensor:
    """The attention slots under torch.autocast; three float32 operands are the float32 slots' call.  idx = positions of (batch, head, token) in the operands' dims.
    Returns the (B, Lq, H, 64) output buffer."""
    dims = _attn_check(who, _QKV, q, k, v, idx, "mixed", twin=", or use slow_attn_amp_grad / memory_efficient_attention_amp_grad")
    return _sdpa_launch(q, k, v, idx, scale, _mask_args(who, mask, *dims), dims, False)[3]


def slow_attn_amp(query, key, value, scale: float, attn_mask=None, dropout_p: float = 0.0):
    """The `slow_attn` slot for a model run under torch.autocast (basic_var.py:117 with half or mixed operands): softmax(scale q k^T + attn_mask) v on the
    half-precision matrix cores.  query (B, H, Lq, 64), key / value (B, H, Lk, 64) on the GPU.  `value` fixes the dtype: float16 or bfloat16, and then query and key
    are EACH that dtype or float32 (with attn_l2_norm the reference's normalised q, and on the GPU its k, arrive in float32); a float32 operand is rounded to the half
    dtype (nearest even) inside the kernel as it is read - the bits of a prior .to(dtype), without the pass over memory.  All three float32: slow_attn itself (same
    bits, float32 result).  attn_mask: float32 additive, bool keep-mask or additive in the operands' half dtype, broadcastable to (B, H, Lq, Lk) with the key dimension
    materialised; views and stride-0 expansions are read in place; the mask is added to the fp32 score.  Operands meeting their alignment rule (float32: strides % 4,
    half: strides % 8, data_ptr % 16) are read in place, any other is copied once into a fresh dense tensor.  Without a mask and with three half operands the call is
    flash_attn_func's kernel.  Returns a (B, H, Lq, 64) VIEW of a fresh (B, Lq, H, 64) buffer of the half dtype, as torch's SDPA returns under autocast."""
    if dropout_p and dropout_p > 0:
        raise SdvarError("slow_attn_amp: dropout_p > 0 is not supported (inference only)")
    return _sdpa_amp("slow_attn_amp", query, key, value, (0, 1, 2), scale, attn_mask).permute(0, 2, 1, 3)


def memory_efficient_attention_amp(q, k, v, attn_bias=None, p: float = 0.0, scale: Optional[float] = None):
    """The xformers slot under torch.autocast (basic_var.py:115): q (B, Lq, H, 64), k / v (B, Lk, H, 64), dtypes and attn_bias as for slow_attn_amp; an expanded
    (stride-0) (B, H, Lq, Lk) bias is read through its strides and never materialised.  Returns (B, Lq, H, 64).  The same kernel as slow_attn_amp with other strides."""
    if p and p > 0:
        raise SdvarError("memory_efficient_attention_amp: p > 0 (dropout) is not supported (inference only)")
    return _sdpa_amp("memory_efficient_attention_amp", q, k, v, (0, 2, 1), 1.0 / math.sqrt(64.0) if scale is None else scale, attn_bias)


def _sdpa_amp_grad(who: str, q, k, v, idx, scale: float, mask) -> torch.Tensor:
    """The differentiable attention slots under torch.autocast: _sdpa_amp's operand rules, minus its refusal of operands that require grad.  Returns the
    (B, Lq, H, 64) output buffer."""
    dims = _attn_check(who, _QKV, q, k, v, idx, "mixed", mask=mask)
    if dims[4] is None:
        return _sdpa_grad(who, q, k, v, idx, scale, mask)           # three fp32 operands: the fp32 slots' path, unchanged
    if not _wants_grad(q, k, v):
        return _sdpa_amp(who, q, k, v, idx, scale, mask)            # what the inference twin launches: the same bits, no LSE
    return _SdpaFn.apply(q, k, v, mask, idx, scale, who, dims)


def slow_attn_amp_grad(query, key, value, scale: float, attn_mask=None, dropout_p: float = 0.0):
    """slow_attn_amp under autograd (the reference's mixed-precision trainer runs loss.backward() through basic_var.py:117 under torch.autocast): layouts, dtype rules
    (value fixes the half dtype; query and key each that dtype or float32), mask rules, alignment and copy-once rule and the returned (B, H, Lq, 64) view as for
    slow_attn_amp.  With grad mode off, or no operand requiring grad, it IS slow_attn_amp (same launch, same bits); three float32 operands go to slow_attn_grad's path.
    Otherwise the forward is sdvar_op_sdpa_hm_lse (slow_attn_amp's output bits, plus the log-sum-exp rows) and the backward one sdvar_op_sdpa_h_bwd call on the
    half-precision matrix cores: P recomputed in fp32 from the rounded operands, P and dS rounded once to the half dtype for the second products, fp32 accumulation,
    no clamping (an fp16 overflow is +-inf, which a GradScaler needs to see), no score matrix in memory, masked tiles skipped, deterministic.  Gradients come back as
    (B, H, L, 64) views of fresh dense (B, L, H, 64) buffers in each operand's OWN dtype (float32 for a float32 query / key, unrounded); only those autograd asks for
    are computed.  An upstream gradient that misses the alignment rule is copied once; one whose dtype is not the output's raises.  No dropout, no gradient for the
    mask, no double backward."""
    if dropout_p and dropout_p > 0:
        raise SdvarError("slow_attn_amp_grad: dropout_p > 0 is not supported (the reference trains with attn_drop = 0)")
    return _sdpa_amp_grad("slow_attn_amp_grad", query, key, value, (0, 1, 2), scale, attn_mask).permute(0, 2, 1, 3)


def memory_efficient_attention_amp_grad(q, k, v, attn_bias=None, p: float = 0.0, scale: Optional[float] = None):
    """memory_efficient_attention_amp under autograd: q (B, Lq, H, 64), k / v (B, Lk, H, 64), dtypes and attn_bias as for slow_attn_amp_grad; returns (B, Lq, H, 64);
    gradients are dense (B, L, H, 64).  The same kernels as slow_attn_amp_grad with other strides."""
    if p and p > 0:
        raise SdvarError("memory_efficient_attention_amp_grad: p > 0 (dropout) is not supported (the reference trains with attn_drop = 0)")
    return _sdpa_amp_grad("memory_efficient_attention_amp_grad", q, k, v, (0, 2, 1), 1.0 / math.sqrt(64.0) if scale is None else scale, attn_bias)


def flash_attn_func_grad(q, k, v, dropout_p: float = 0.0, softmax_scale: Optional[float] = None, causal: bool = False, window_size=(-1, -1), softcap: float = 0.0,
                         alibi_slopes=None, deterministic: bool = False, return_attn_probs: bool = False):
    """flash_attn_func under autograd: signature, operand rules (three float16 or three bfloat16 (B, L, H, 64) operands, no mask) and rejections as flash_attn_func.
    With grad mode off, or no operand requiring grad, it IS flash_attn_func (same launch, same bits).  Otherwise memory_efficient_attention_amp_grad's function
    without a bias: the output has flash_attn_func's bits, gradients are dense (B, L, H, 64) tensors of the operand dtype."""
    who = "flash_attn_func_grad"
    _flash_options(who, dropout_p, causal, window_size, softcap, alibi_slopes, return_attn_probs, True)
    dims = _attn_check(who, _QKV_FLASH, q, k, v, (0, 2, 1), "half")
    if not _wants_grad(q, k, v):
        return flash_attn_func(q, k, v, softmax_scale=softmax_scale)
    return _SdpaFn.apply(q, k, v, None, (0, 2, 1), 1.0 / math.sqrt(64.0) if softmax_scale is None else softmax_scale, who, dims)


def _dense16(t: torch.Tensor) -> torch.Tensor:
    """t itself when it is dense and 16-byte aligned, else one fresh dense copy (.contiguous() would hand back a dense tensor at a misaligned address)."""
    return t if t.is_contiguous() and t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _cached_planes(kind: str, w: torch.Tensor, mode: str, make):
    """One entry per (kind, mode, weight): an entry whose weight has been updated in place since (its _version moved - every step of a training loop) is REPLACED,
    so a loop strands no stale plane sets."""
    key = (kind, mode, w.data_ptr(), tuple(w.shape))
    hit = _WEIGHT_PLANES.get(key)
    if hit is not None and hit[1] == w._version:
        _WEIGHT_PLANES.move_to_end(key)
        return hit[2], hit[3]
    planes, sc = make()
    _WEIGHT_PLANES[key] = (w, w._version, planes, sc)
    _WEIGHT_PLANES.move_to_end(key)
    while len(_WEIGHT_PLANES) > _WEIGHT_PLANES_MAX:
        _WEIGHT_PLANES.popitem(last=False)
    return planes, sc


_OPERAND_FORMAT = {"f32": 0, "f16x2": 2, "bf16x3": 3}       # csrc/mlp_bwd.hip
_OPERAND_PLANES = {"f32": 1, "f16x2": 2, "bf16x3": 3}


def _split_planes(t: torch.Tensor, mode: str, rows: int, cols: int, scale: Optional[torch.Tensor] = None, st=None) -> torch.Tensor:
    """The K-blocked operand planes of a dense fp32 (rows, cols) tensor in mode f16x2 (scale: the device scale the split writes, or None for the unscaled split)
    or bf16x3.  st: the current stream, when the caller has looked it up already."""
    planes = torch.empty(_OPERAND_PLANES[mode], rows * cols, dtype=torch.int16, device=t.device)
    st = E._stream() if st is None else st
    if mode == "f16x2":
        E._check(E.load_library().sdvar_op_split_planes_f16(_p(t), _p(planes), rows, cols, rows * cols, _p(scale), st))
    else:
        E._check(E.load_library().sdvar_op_split_planes(_p(t), _p(planes), rows, cols, rows * cols, st))
    return planes


def _weight_planes(w: torch.Tensor, mode: str):
    def make():
        sc = torch.zeros(4, dtype=torch.float32, device=w.device) if mode == "f16x2" else None
        return _split_planes(w.detach().contiguous(), mode, *w.shape, sc), sc
    return _cached_planes("n", w, mode, make)


def _pad32(n: int) -> int:
    return (n + 31) // 32 * 32


def _transposed_operand(t: torch.Tensor, mode: str, scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The GEMM operand of t^T for a dense, 16-byte aligned fp32 (rows, cols) tensor: (cols x pad32(rows)), fp32 in mode f32, else K-blocked planes; the kernel
    writes the zero tail."""
    rows, cols = t.shape
    n = cols * _pad32(rows)
    out = torch.empty(_OPERAND_PLANES[mode], n, dtype=torch.float32 if mode == "f32" else torch.int16, device=t.device)
    E._check(E.load_library().sdvar_op_transpose_operand(_p(t), t.stride(0), rows, cols, _OPERAND_FORMAT[mode], _p(out), n, _p(scale), E._stream()))
    return out


def _weight_planes_t(w: torch.Tensor, mode: str):
    """(operand of w^T, scale): the dgrad GEMMs' weight operand, cached like the forward's.  In mode f16x2 it carries the forward planes' scale."""
    def make():
        sc = _weight_planes(w, mode)[1] if mode == "f16x2" else None
        return _transposed_operand(_dense16(w.detach()), mode, sc), sc
    return _cached_planes("t", w, mode, make)


def _mlp_check(who: str, x, weight1, weight2, bias1, bias2, activation, return_residual, process_group, amp: bool, grad: bool, bias_shapes: bool = True):
    """The argument checks of the FFN slots.  amp: the dtype policy - False: float32 operands only; True: every operand float32 or the call's half dtype (x.dtype when
    x is half, else the GPU's autocast dtype).  grad = the caller has a backward.  bias_shapes=False: fused_mlp_func alone has never looked at its biases' shapes.
    Returns (half or None, Cin, hid, Cout).  Nothing here touches the library."""
    if activation != "gelu_approx":
        raise SdvarError(f"{who}: activation {activation!r}; only 'gelu_approx' (tanh GELU) is built")
    if return_residual:
        raise SdvarError(f"{who}: return_residual=True is not supported")
    if process_group is not None:
        raise SdvarError(f"{who}: a process group (tensor-parallel MLP) is not supported")
    named = [("x", x), ("weight1", weight1), ("weight2", weight2)]
    if bias1 is not None:
        named.append(("bias1", bias1))
    if bias2 is not None:
        named.append(("bias2", bias2))
    refuse = not grad and torch.is_grad_enabled()
    for name, t in named:
        _gpu_tensor(who, name, t)
        if amp:
            if t.dtype != torch.float32 and t.dtype not in _HALF_DTYPES:
                raise SdvarError(f"{who}: {name} is {t.dtype}; only float32, float16 and bfloat16 operands are supported")
        elif t.dtype != torch.float32:
            raise SdvarError(f"{who}: {name} is {t.dtype}; only float32 operands are supported")
        elif refuse and t.requires_grad:
            raise SdvarError(f"{who}: {name} requires grad and grad mode is on; no backward exists (call under torch.no_grad())")
    half = None
    if amp:
        half = x.dtype if x.dtype in _HALF_DTYPES else _autocast_gpu_dtype()
        if half not in _HALF_DTYPES:
            twin = "fused_mlp_func_grad" if grad else "fused_mlp_func"
            raise SdvarError(f"{who}: x is {x.dtype} and torch.autocast is not enabled for the GPU with float16 / bfloat16: there is no half dtype to compute in - "
                             f"call it under torch.autocast or with a half x, or use fused_mlp_func / {twin} for float32 arithmetic")
        for name, t in named:
            if t.dtype != torch.float32 and t.dtype != half:
                raise SdvarError(f"{who}: mixed half dtypes: {name} is {t.dtype} but the half dtype of the call is {half} (every operand must be {half} or float32)")
            if refuse and t.requires_grad:
                raise SdvarError(f"{who}: {name} requires grad and grad mode is on; no backward exists (call under torch.no_grad(), or use fused_mlp_func_amp_grad)")
    if weight1.dim() != 2 or weight2.dim() != 2 or x.dim() < 1 or x.shape[-1] != weight1.shape[1] or weight2.shape[1] != weight1.shape[0]:
        raise SdvarError(f"{who}: shapes do not chain: x {tuple(x.shape)}, weight1 {tuple(weight1.shape)}, weight2 {tuple(weight2.shape)}")
    Cin, hid, Cout = weight1.shape[1], weight1.shape[0], weight2.shape[0]
    if Cin % 32 or hid % 32:
        raise SdvarError(f"{who}: in_features {Cin} and hidden_features {hid} must be multiples of 32")
    if amp and Cout % 8:
        raise SdvarError(f"{who}: out_features {Cout} must be a multiple of 8")
    for name, b, n in (("bias1", bias1, hid), ("bias2", bias2, Cout)) if bias_shapes else ():
        if b is not None and tuple(b.shape) != (n,):
            raise SdvarError(f"{who}: {name} has shape {tuple(b.shape)}, expected ({n},)")
    if amp and any(t.device != x.device for _, t in named):
        raise SdvarError(f"{who}: operands live on different devices")
    return half, Cin, hid, Cout


def _gemm_nt(mode: str, A, B, wscale, out, M: int, N: int, K: int, bias=None, epilogue: int = 0, planes=None, st=None) -> None:
    """epilogue(A (M x K) . B (N x K)^T + bias) on operands of `mode` (fp32 dense, or K-blocked planes); wscale: the f16x2 GEMM's device scale pointer or None;
    epilogue 1 = tanh GELU.  The result goes to out (M, N) fp32 and / or, in the plane modes, to `planes`: the operand planes the next GEMM reads.  st: the current
    stream, when the caller has looked it up already."""
    lib, st, ldp = E.load_library(), E._stream() if st is None else st, 0 if planes is None else M * N
    if mode == "f32":
        E._check(lib.sdvar_op_gemm(_p(A), K, _p(B), _p(bias), _p(out), N, M, N, K, epilogue, None, 0, None, 1, 0, st))
    elif mode == "f16x2":
        E._check(lib.sdvar_op_gemm_f16x2(_p(A), M * K, _p(B), N * K, wscale, _p(bias), _p(out), N, _p(planes), ldp, M, N, K, epilogue, None, 0, None, 1, 0, st))
    else:
        E._check(lib.sdvar_op_gemm_bf16x3(_p(A), M * K, _p(B), N * K, _p(bias), _p(out), N, _p(planes), ldp, M, N, K, epilogue, None, 0, None, 1, 0, st))


def _mlp_forward(x, weight1, weight2, bias1, bias2, mode: str, keep_pre: bool):
    """(out, xr, pre).  keep_pre False: the inference launches (fc1 with the GELU epilogue).  True: fc1 with the bias epilogue leaves pre (M, hid) in memory and
    sdvar_op_gelu_operand writes what the GELU epilogue would have - the same bits, so `out` is the same in both."""
    Cin, hid, Cout = weight1.shape[1], weight1.shape[0], weight2.shape[0]
    xr = x.detach().reshape(-1, Cin).contiguous()
    M = xr.shape[0]
    out = torch.empty(tuple(x.shape[:-1]) + (Cout,), dtype=torch.float32, device=x.device)
    if M == 0:
        return out, xr, None
    b1 = torch.zeros(hid, dtype=torch.float32, device=x.device) if bias1 is None else bias1.detach().contiguous()
    b2 = torch.zeros(Cout, dtype=torch.float32, device=x.device) if bias2 is None else bias2.detach().contiguous()
    pre = torch.empty(M, hid, dtype=torch.float32, device=x.device) if keep_pre else None
    st, f32 = E._stream(), mode == "f32"
    # xo, h: the operands of fc1 and fc2 - dense fp32 in mode f32, else planes, which fc1 writes through its plane output
    if f32:
        (w1, s1), (w2, s2), xo = (weight1.detach().contiguous(), None), (weight2.detach().contiguous(), None), xr
        h = torch.empty(M, hid, dtype=torch.float32, device=x.device)
    else:
        (w1, s1), (w2, s2) = _weight_planes(weight1, mode), _weight_planes(weight2, mode)
        xo = _split_planes(xr, mode, M, Cin, st=st)
        h = torch.empty(_OPERAND_PLANES[mode], M * hid, dtype=torch.int16, device=x.device)
    if keep_pre:
        _gemm_nt(mode, xo, w1, _p(s1), pre, M, hid, Cin, b1, st=st)
        E._check(E.load_library().sdvar_op_gelu_operand(_p(pre), M, hid, _OPERAND_FORMAT[mode], int(mode == "f16x2"), _p(h), 0 if f32 else M * hid, st))
    else:
        _gemm_nt(mode, xo, w1, _p(s1), h if f32 else None, M, hid, Cin, b1, 1, None if f32 else h, st)
    _gemm_nt(mode, h, w2, _p(s2), out, M, Cout, hid, b2, st=st)
    return out, xr, pre


def fused_mlp_func(x, weight1, weight2, bias1=None, bias2=None, activation: str = "gelu_approx", save_pre_act: bool = False, return_residual: bool = False,
                   checkpoint_lvl: int = 0, heuristic=0, process_group=None):
    """The `fused_mlp_func` slot (flash_attn.ops.fused_dense signature; basic_var.py:46-50): fc2(gelu_tanh(fc1(x))), x (..., C) fp32 on the GPU, weight1 (hidden, C),
    weight2 (out, hidden).  Two launches of the operator GEMMs of the configured mode (seam.configure): fc1 with the GELU epilogue writing the operand planes of fc2
    directly.  C and hidden must be multiples of 32.  save_pre_act / checkpoint_lvl / heuristic only matter to a backward and are ignored."""
    _mlp_check("fused_mlp_func", x, weight1, weight2, bias1, bias2, activation, return_residual, process_group, False, False, bias_shapes=False)
    return _mlp_forward(x, weight1, weight2, bias1, bias2, _gemm_mode, False)[0]


class _MlpGrad(torch.autograd.Function):
    """fc2(gelu_tanh(fc1(x))) with a HIP backward: four NT GEMMs of the forward's mode on operands produced by csrc/mlp_bwd.hip.  Saved: x, the weights and pre."""

    @staticmethod
    def forward(ctx, x, weight1, weight2, bias1, bias2, mode):
        out, xr, pre = _mlp_forward(x, weight1, weight2, bias1, bias2, mode, True)
        ctx.save_for_backward(xr, weight1, weight2, pre)
        ctx.mlp = (mode, tuple(x.shape))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        xr, weight1, weight2, pre = ctx.saved_tensors
        mode, xshape = ctx.mlp
        nx, nw1, nw2, nb1, nb2 = ctx.needs_input_grad[:5]
        Cin, hid, Cout = weight1.shape[1], weight1.shape[0], weight2.shape[0]
        M, dev = xr.shape[0], xr.device
        f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        if M == 0:
            z = lambda need, *shape: torch.zeros(*shape, dtype=torch.float32, device=dev) if need else None
            return z(nx, *xshape), z(nw1, hid, Cin), z(nw2, Cout, hid), z(nb1, hid), z(nb2, Cout), None
        lib, st, fmt, npl, Mp = E.load_library(), E._stream(), _OPERAND_FORMAT[mode], _OPERAND_PLANES[mode], _pad32(M)
        kind, h16, el = int(mode == "f16x2"), mode == "f16x2", torch.float32 if mode == "f32" else torch.int16
        operand = lambda n: torch.empty(npl, n, dtype=el, device=dev)
        dy = _dense16(dy.reshape(M, Cout))          # stride-0 expansions, transposed consumers, a dense tensor at a misaligned address: one fresh dense copy
        xr = _dense16(xr)
        need_dh = nx or nw1 or nb1
        dx = dw1 = dw2 = db1 = db2 = None
        if nb2:
            db2 = f32(Cout)
            E._check(lib.sdvar_op_colsum(_p(dy), Cout, M, Cout, _p(db2), st))
        # f16x2: the gradient operands carry a per-tensor power-of-two scale (gradients of an fp32 run sit far below the range the unscaled split resolves)
        sdy = torch.zeros(4, dtype=torch.float32, device=dev) if h16 and (need_dh or nw2) else None
        sdp = torch.zeros(4, dtype=torch.float32, device=dev) if h16 and need_dh else None
        off = lambda sc, floats: None if sc is None else C.c_void_p(sc.data_ptr() + 4 * floats)
        dpre = dpre_t = h_t = part = None
        if need_dh:
            w2t, s2 = _weight_planes_t(weight2, mode)
            dyo = dy if mode == "f32" else _split_planes(dy, mode, M, Cout, sdy, st)
            if h16:
                E._check(lib.sdvar_op_scale_pair(None, 0, _p(sdy), 0, _p(s2), st))
            dh = f32(M, hid)
            _gemm_nt(mode, dyo, w2t, off(sdy, 2), dh, M, hid, Cout, st=st)
            if h16:          # |gelu'| <= 1.13: half of dh's scale keeps dpre inside the range without a second pass
                E._check(lib.sdvar_op_scale_pair(_p(dh), M * hid, _p(sdp), 1, _p(_weight_planes(weight1, mode)[1]) if nx else None, st))
            if nx:
                dpre = operand(M * hid)
            if nw1:
                dpre_t = operand(hid * Mp)
            if nb1:
                part = f32(Mp // 32, hid)
        else:
            dh = None
            if h16 and nw2:
                E._check(lib.sdvar_op_scale_pair(_p(dy), M * Cout, _p(sdy), 0, None, st))
        if nw2:
            h_t = operand(hid * Mp)
        if need_dh or nw2:
            E._check(lib.sdvar_op_gelu_bwd(_p(dh), _p(pre), M, hid, fmt, kind, _p(sdp), _p(dpre), M * hid, _p(dpre_t), hid * Mp, _p(h_t), hid * Mp, _p(part), st))
        if nx:
            w1t, _ = _weight_planes_t(weight1, mode)
            dx = f32(M, Cin)
            _gemm_nt(mode, dpre, w1t, off(sdp, 2), dx, M, Cin, hid, st=st)
            dx = dx.view(xshape)
        if nw2:
            dw2 = f32(Cout, hid)
            _gemm_nt(mode, _transposed_operand(dy, mode, sdy), h_t, off(sdy, 0), dw2, Cout, hid, Mp, st=st)
        if nw1:
            dw1 = f32(hid, Cin)
            _gemm_nt(mode, dpre_t, _transposed_operand(xr, mode), off(sdp, 0), dw1, hid, Cin, Mp, st=st)
        if nb1:
            db1 = f32(hid)
            E._check(lib.sdvar_op_colsum(_p(part), hid, Mp // 32, hid, _p(db1), st))
        return dx, dw1, dw2, db1, db2, None


def fused_mlp_func_grad(x, weight1, weight2, bias1=None, bias2=None, activation: str = "gelu_approx", save_pre_act: bool = False, return_residual: bool = False,
                        checkpoint_lvl: int = 0, heuristic=0, process_group=None):
    """fused_mlp_func under autograd (the reference's trainer runs loss.backward() through basic_var.py:46-50): signature, operand rules and argument errors as
    fused_mlp_func, plus out_features % 32 == 0.  With grad mode off, or no operand requiring grad, it IS fused_mlp_func (same launches, same bits).  Otherwise fc1
    runs with the bias epilogue and leaves the pre-activation (M, hidden) fp32 in memory - the only saved tensor besides x and the weights - and one more kernel
    writes the GELU operand the fused epilogue would have written: the output has fused_mlp_func's bits in every mode.  Backward: dh = dy W2, dpre = dh gelu'(pre),
    dx = dpre W1, dW2 = dy^T h, dW1 = dpre^T x as four NT GEMMs of the configured mode (the mode of the forward call) on operands written by csrc/mlp_bwd.hip
    (transposed, zero-padded to K % 32 == 0; h recomputed from pre with the forward's bits), db2 / db1 by a fixed-order column sum.  Deterministic; only the
    gradients autograd asks for are computed (frozen weights cost no wgrad GEMM, an x without grad no dgrad GEMM), and a gradient computed alone has the bits it
    has in the full run.  Mode f16x2 splits the gradient operands with a per-tensor power-of-two scale.  No double backward, float32 only; save_pre_act /
    checkpoint_lvl / heuristic are accepted and ignored."""
    who = "fused_mlp_func_grad"
    _, Cin, hid, Cout = _mlp_check(who, x, weight1, weight2, bias1, bias2, activation, return_residual, process_group, False, True)
    tensors = [t for t in (x, weight1, weight2, bias1, bias2) if t is not None]
    if not torch.is_grad_enabled() or not any(t.requires_grad for t in tensors):
        return _mlp_forward(x, weight1, weight2, bias1, bias2, _gemm_mode, False)[0]            # what the inference twin launches: the same bits
    if Cout % 32:
        raise SdvarError(f"{who}: out_features {Cout} must be a multiple of 32 under grad (it is K of the dh = dy W2 product)")
    if any(t.device != x.device for t in tensors):
        raise SdvarError(f"{who}: operands live on different devices")
    return _MlpGrad.apply(x, weight1, weight2, bias1, bias2, _gemm_mode)


# ------------------------------------------------------------------------------------------------------------------ the half-precision FFN (torch.autocast)
def _autocast_gpu_dtype():
    """The autocast dtype of the GPU when autocast is enabled for it, else None."""
    if hasattr(torch, "get_autocast_dtype"):
        return torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else None
    return torch.get_autocast_gpu_dtype() if torch.is_autocast_enabled() else None


def _in_code(t: torch.Tensor) -> int:
    """sdvar_op_half_operand's input code: 0 = float32, else the half dtype's."""
    return 0 if t.dtype == torch.float32 else _HALF_DTYPES[t.dtype]


def _half_operand(t: torch.Tensor, half, transpose: bool, part: Optional[torch.Tensor] = None, want_out: bool = True):
    """The K-blocked `half` operand of a dense, 16-byte aligned 2-D tensor (fp32: rounded to nearest even as it is read; half: its bits) or of its transpose
    ((cols x pad32(rows)), zero tail written by the kernel)."""
    rows, cols = t.shape
    out = torch.empty(cols * _pad32(rows) if transpose else rows * cols, dtype=torch.int16, device=t.device) if want_out else None
    # ldx = cols, not t.stride(0): a one-row tensor counts as dense whatever its row stride is
    E._check(E.load_library().sdvar_op_half_operand(_p(t), _in_code(t), cols, rows, cols, _HALF_DTYPES[half], int(transpose), _p(out), _p(part), E._stream()))
    return out


def _weight_operand_h(w: torch.Tensor, half, transpose: bool) -> torch.Tensor:
    """The half operand of a weight ("hn") or of its transpose ("ht"), cached per (kind, half dtype, weight); an entry whose weight moved on is replaced."""
    return _cached_planes("ht" if transpose else "hn", w, f"{half}/{w.dtype}", lambda: (_half_operand(_dense16(w.detach()), half, transpose), None))[0]


def _bias_f32(b: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if b is None else _dense16(b.detach().float())


def _gemm_h(half, A, B, bias, out, M: int, N: int, K: int) -> None:
    """out (M, N) dense, fp32 or `half` = A (M x K) . B (N x K)^T + bias on half operands (sdvar_op_gemm_h, epilogue 0)."""
    dt = _HALF_DTYPES[half]
    E._check(E.load_library().sdvar_op_gemm_h(_p(A), _p(B), dt, _p(bias), _p(out), 0 if out.dtype == torch.float32 else dt, N, None, None, M, N, K, 0, E._stream()))


def _mlp_amp_forward(x, weight1, weight2, bias1, bias2, half, keep_pre: bool):
    """(out, xr, p).  The two launches of sdvar_op_gemm_h behind one operand pass over x; keep_pre: fc1's epilogue also writes p (M, hid) row-major in `half` -
    the other outputs keep their bits."""
    Cin, hid, Cout = weight1.shape[1], weight1.shape[0], weight2.shape[0]
    lib, st, dt = E.load_library(), E._stream(), _HALF_DTYPES[half]
    xr = _dense16(x.detach().reshape(-1, Cin))
    M = xr.shape[0]
    out = torch.empty(tuple(x.shape[:-1]) + (Cout,), dtype=half, device=x.device)
    if M == 0:
        return out, xr, None
    xop = _half_operand(xr, half, False)
    w1op, w2op = _weight_operand_h(weight1, half, False), _weight_operand_h(weight2, half, False)
    b1, b2 = _bias_f32(bias1), _bias_f32(bias2)
    hop = torch.empty(M * hid, dtype=torch.int16, device=x.device)
    p = torch.empty(M, hid, dtype=half, device=x.device) if keep_pre else None
    E._check(lib.sdvar_op_gemm_h(_p(xop), _p(w1op), dt, _p(b1), None, 0, 0, _p(hop), _p(p), M, hid, Cin, 1, st))
    E._check(lib.sdvar_op_gemm_h(_p(hop), _p(w2op), dt, _p(b2), _p(out), dt, Cout, None, None, M, Cout, hid, 0, st))
    return out, xr, p


def fused_mlp_func_amp(x, weight1, weight2, bias1=None, bias2=None, activation: str = "gelu_approx", save_pre_act: bool = False, return_residual: bool = False,
                       checkpoint_lvl: int = 0, heuristic=0, process_group=None):
    """The `fused_mlp_func` slot for a model run under torch.autocast: fc2(gelu_tanh(fc1(x))) on the HALF matrix cores, what autocast's own F.linear / F.gelu pair
    computes.  The half dtype is x.dtype when x is float16 / bfloat16, else the GPU's autocast dtype; with neither it raises (use fused_mlp_func).  x (..., C), weight1
    (hidden, C), weight2 (out, hidden) are each float32 or that dtype - a float32 operand is rounded to nearest even as it is read, the bits of .to(dtype) without the
    pass over memory - and the biases are float32 or half and enter as float32.  Contract: p = half(fp32acc(x_h W1_h^T) + b1), h = half(gelu_tanh(float(p))),
    y = half(fp32acc(h W2_h^T) + b2); nothing is clamped, an fp16 overflow is +-inf.  Two launches of sdvar_op_gemm_h (one fp16 / bf16 MFMA per product where mode f16x2
    issues three); weight operands are cached per (weight, dtype) and replaced when the weight is updated in place.  C and hidden must be multiples of 32, out of 8.
    Returns (..., out) in the half dtype.  Deterministic.  save_pre_act / checkpoint_lvl / heuristic are accepted and ignored."""
    half, _, _, _ = _mlp_check("fused_mlp_func_amp", x, weight1, weight2, bias1, bias2, activation, return_residual, process_group, True, False)
    return _mlp_amp_forward(x, weight1, weight2, bias1, bias2, half, False)[0]


class _MlpAmpGrad(torch.autograd.Function):
    """The half-precision FFN with a HIP backward: four launches of sdvar_op_gemm_h on operands produced by csrc/mlp_half.hip.  Saved: x, the weights and the half
    pre-activation p."""

    @staticmethod
    def forward(ctx, x, weight1, weight2, bias1, bias2, half):
        out, xr, p = _mlp_amp_forward(x, weight1, weight2, bias1, bias2, half, True)
        ctx.save_for_backward(xr, weight1, weight2, *(() if p is None else (p,)))
        ctx.mlp = (half, tuple(x.shape), None if bias1 is None else bias1.dtype, None if bias2 is None else bias2.dtype)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        xr, weight1, weight2, *rest = ctx.saved_tensors
        half, xshape, b1dt, b2dt = ctx.mlp
        nx, nw1, nw2, nb1, nb2 = ctx.needs_input_grad[:5]
        Cin, hid, Cout = weight1.shape[1], weight1.shape[0], weight2.shape[0]
        M, dev = xr.shape[0], xr.device
        if dy.dtype != half:
            raise SdvarError(f"fused_mlp_func_amp_grad: the gradient of the output is {dy.dtype} but the output is {half}; the backward reads dy in the output's dtype")
        if M == 0:
            z = lambda need, dtype, *shape: torch.zeros(*shape, dtype=dtype, device=dev) if need else None
            return z(nx, xr.dtype, *xshape), z(nw1, weight1.dtype, hid, Cin), z(nw2, weight2.dtype, Cout, hid), z(nb1, b1dt, hid), z(nb2, b2dt, Cout), None
        p = rest[0]
        lib, st, dt, Mp = E.load_library(), E._stream(), _HALF_DTYPES[half], _pad32(M)
        f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        operand = lambda n: torch.empty(n, dtype=torch.int16, device=dev)
        dy = _dense16(dy.reshape(M, Cout))          # stride-0 expansions, transposed consumers, a dense tensor at a misaligned address: one fresh dense copy
        need_dh = nx or nw1 or nb1
        dx = dw1 = dw2 = db1 = db2 = None
        dyt = None
        if nw2 or nb2:                               # dy^T, and db2's 32-row partials from the same pass
            part2 = f32(Mp // 32, Cout) if nb2 else None
            dyt = _half_operand(dy, half, True, part2, want_out=bool(nw2))
            if nb2:
                db2 = f32(Cout)
                E._check(lib.sdvar_op_colsum(_p(part2), Cout, Mp // 32, Cout, _p(db2), st))
                db2 = db2.to(b2dt)
        dh = dpre = dpre_t = h_t = part = None
        if need_dh:
            dh = f32(M, hid)
            _gemm_h(half, _half_operand(dy, half, False), _weight_operand_h(weight2, half, True), None, dh, M, hid, Cout)
            dpre = operand(M * hid) if nx else None
            dpre_t = operand(hid * Mp) if nw1 else None
            part = f32(Mp // 32, hid) if nb1 else None
        if nw2:
            h_t = operand(hid * Mp)
        if need_dh or nw2:
            E._check(lib.sdvar_op_gelu_bwd_h(_p(dh), _p(p), M, hid, dt, _p(dpre), _p(dpre_t), _p(h_t), _p(part), st))
        if nx:
            dx = torch.empty(M, Cin, dtype=xr.dtype, device=dev)
            _gemm_h(half, dpre, _weight_operand_h(weight1, half, True), None, dx, M, Cin, hid)
            dx = dx.view(xshape)
        if nw2:
            dw2 = torch.empty(Cout, hid, dtype=weight2.dtype, device=dev)
            _gemm_h(half, dyt, h_t, None, dw2, Cout, hid, Mp)
        if nw1:
            dw1 = torch.empty(hid, Cin, dtype=weight1.dtype, device=dev)
            _gemm_h(half, dpre_t, _half_operand(xr, half, True), None, dw1, hid, Cin, Mp)
        if nb1:
            db1 = f32(hid)
            E._check(lib.sdvar_op_colsum(_p(part), hid, Mp // 32, hid, _p(db1), st))
            db1 = db1.to(b1dt)
        return dx, dw1, dw2, db1, db2, None


def fused_mlp_func_amp_grad(x, weight1, weight2, bias1=None, bias2=None, activation: str = "gelu_approx", save_pre_act: bool = False, return_residual: bool = False,
                            checkpoint_lvl: int = 0, heuristic=0, process_group=None):
    """fused_mlp_func_amp under autograd (the reference's mixed-precision trainer runs loss.backward() through basic_var.py:46-50 under torch.autocast): signature,
    dtype rule, operand rules and argument errors as fused_mlp_func_amp, plus out_features % 32 == 0 under grad.  With grad mode off, or no operand requiring grad, it
    IS fused_mlp_func_amp (same launches, same bits).  Otherwise fc1's epilogue also writes the half pre-activation p (M, hidden) - the only tensor saved besides x and
    the weights, half of what fused_mlp_func_grad saves - and the output keeps its bits.  Backward: dh = fp32acc(dy W2_h), dpre = half(dh gelu'(p)), dx = dpre W1_h,
    dW2 = dy^T h, dW1 = dpre^T x_h as four launches of sdvar_op_gemm_h on operands written by csrc/mlp_half.hip (transposed, zero-padded to K % 32 == 0; h recomputed
    from p with the forward's bits), db1 = sum dpre and db2 = sum dy by fixed-order column sums of the rounded values.  Gradients come back in each operand's OWN dtype:
    unrounded float32 for a float32 x / weight / bias (the reference's case: float32 x and master weights), half otherwise.  dy must have the output's dtype; one that
    is not dense or not 16-byte aligned is copied once.  Deterministic; only the gradients autograd asks for are computed, and each has the bits it has in the full
    run.  Nothing is clamped: an fp16 overflow is +-inf and reaches the GradScaler.  No double backward."""
    who = "fused_mlp_func_amp_grad"
    half, Cin, hid, Cout = _mlp_check(who, x, weight1, weight2, bias1, bias2, activation, return_residual, process_group, True, True)
    tensors = [t for t in (x, weight1, weight2, bias1, bias2) if t is not None]
    if not torch.is_grad_enabled() or not any(t.requires_grad for t in tensors):
        return _mlp_amp_forward(x, weight1, weight2, bias1, bias2, half, False)[0]            # what the inference twin launches: the same bits
    if Cout % 32:
        raise SdvarError(f"{who}: out_features {Cout} must be a multiple of 32 under grad (it is K of the dh = dy W2 product)")
    return _MlpAmpGrad.apply(x, weight1, weight2, bias1, bias2, half)


# ------------------------------------------------------------------------------------------------------- the dense linears (csrc/linear_train.hip)
def _linear_check(who: str, x, weight, bias, amp: bool, grad: bool):
    """The argument checks of the four linear functions.  amp / grad as for _mlp_check.  Returns (half or None, K, N).  Nothing here touches the library."""
    named = [("x", x), ("weight", weight)] + ([] if bias is None else [("bias", bias)])
    refuse = not grad and torch.is_grad_enabled()
    for name, t in named:
        _gpu_tensor(who, name, t)
        if t.dtype == torch.float64:
            raise SdvarError(f"{who}: {name} is torch.float64; only float32" + (", float16 and bfloat16 operands" if amp else " operands") + f" are supported - pass {name}.float()")
        if amp:
            if t.dtype != torch.float32 and t.dtype not in _HALF_DTYPES:
                raise SdvarError(f"{who}: {name} is {t.dtype}; only float32, float16 and bfloat16 operands are supported")
        elif t.dtype in _HALF_DTYPES:
            raise SdvarError(f"{who}: {name} is {t.dtype}; this function takes float32 operands only - use {'linear_amp_grad' if grad else 'linear_amp'} for half operands")
        elif t.dtype != torch.float32:
            raise SdvarError(f"{who}: {name} is {t.dtype}; only float32 operands are supported")
    half = None
    if amp:
        half = x.dtype if x.dtype in _HALF_DTYPES else _autocast_gpu_dtype()
        if half not in _HALF_DTYPES:
            raise SdvarError(f"{who}: x is {x.dtype} and torch.autocast is not enabled for the GPU with float16 / bfloat16: there is no half dtype to compute in - "
                             f"call it under torch.autocast or with a half x, or use {'linear_grad' if grad else 'linear'} for float32 arithmetic")
        for name, t in named:
            if t.dtype != torch.float32 and t.dtype != half:
                raise SdvarError(f"{who}: mixed half dtypes: {name} is {t.dtype} but the half dtype of the call is {half} (every operand must be {half} or float32)")
    if refuse:
        for name, t in named:
            if t.requires_grad:
                raise SdvarError(f"{who}: {name} requires grad and grad mode is on; no backward exists (call under torch.no_grad(), or use {who}_grad)")
    if weight.dim() != 2 or x.dim() < 1 or x.shape[-1] != weight.shape[1]:
        raise SdvarError(f"{who}: shapes do not chain: x {tuple(x.shape)}, weight {tuple(weight.shape)} (x (..., K) with weight (N, K))")
    N, K = weight.shape
    if K % 32:
        raise SdvarError(f"{who}: in_features {K} (the last dim of x) must be a multiple of 32")
    if amp and N % 8:
        raise SdvarError(f"{who}: out_features {N} (weight.shape[0]) must be a multiple of 8")
    if bias is not None and tuple(bias.shape) != (N,):
        raise SdvarError(f"{who}: bias has shape {tuple(bias.shape)}, expected ({N},)")
    if any(t.device != x.device for _, t in named):
        raise SdvarError(f"{who}: operands live on different devices; move weight and bias to x's device")
    return half, K, N


def _linear_wants_grad(who: str, x, weight, bias, N: int) -> bool:
    if not torch.is_grad_enabled() or not any(t is not None and t.requires_grad for t in (x, weight, bias)):
        return False
    if N % 32:
        raise SdvarError(f"{who}: out_features {N} (weight.shape[0]) must be a multiple of 32 under grad (it is K of the dx = dy W product)")
    return True


def _rows16(x: torch.Tensor, K: int) -> torch.Tensor:
    """x (..., K) as the dense, 16-byte aligned (M, K) matrix the kernels read: a view where x is one, else one copy.  A single row is given the row stride K (a one-row
    slice of a wider buffer counts as dense whatever its row stride is, and a kernel's leading dimension is a stride)."""
    xr = _dense16(x.detach().reshape(-1, K))
    return xr.as_strided((1, K), (K, 1)) if xr.shape[0] == 1 else xr


def _linear_forward(x, weight, bias, mode: str):
    """(out, xr): x W^T + b as one operator GEMM of `mode` behind one operand pass over x (none in mode f32)."""
    N, K = weight.shape
    xr = _rows16(x, K)
    M = xr.shape[0]
    out = torch.empty(tuple(x.shape[:-1]) + (N,), dtype=torch.float32, device=x.device)
    if M == 0:
        return out, xr
    st = E._stream()
    b = None if bias is None else _dense16(bias.detach())
    if mode == "f32":
        _gemm_nt(mode, xr, _dense16(weight.detach()), None, out, M, N, K, b, st=st)
    else:
        w, sw = _weight_planes(weight, mode)
        _gemm_nt(mode, _split_planes(xr, mode, M, K, st=st), w, _p(sw), out, M, N, K, b, st=st)
    return out, xr


def linear(x, weight, bias=None):
    """F.linear on the operator GEMMs of the configured mode (seam.configure): x (..., K) W (N, K)^T + bias (N,) -> (..., N), float32 operands on the GPU, K % 32 == 0.
    One GEMM launch behind one operand pass over x (modes f16x2 / bf16x3; mode f16x2 saturates x at +-65504 as fused_mlp_func does); the weight's operand planes come
    from the FFN's cache and are replaced when the weight is updated in place.  x is read in place when dense and 16-byte aligned, else copied once.  Inference only:
    an operand that requires grad while grad mode is on raises (use linear_grad).  Anything else raises SdvarError - there is no fall-back to torch."""
    _linear_check("linear", x, weight, bias, False, False)
    return _linear_forward(x, weight, bias, _gemm_mode)[0]


class _LinearGrad(torch.autograd.Function):
    """x W^T + b with a HIP backward: two NT GEMMs of the forward's mode on operands one sdvar_op_grad_operands pass writes.  Saved: x (dense (M, K)) and the weight;
    nothing of x when the weight is frozen."""

    @staticmethod
    def forward(ctx, x, weight, bias, mode):
        out, xr = _linear_forward(x, weight, bias, mode)
        ctx.save_for_backward(weight, *((xr,) if ctx.needs_input_grad[1] else ()))
        ctx.lin = (mode, tuple(x.shape))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        weight, *rest = ctx.saved_tensors
        mode, xshape = ctx.lin
        nx, nw, nb = ctx.needs_input_grad[:3]
        N, K = weight.shape
        M, dev = math.prod(xshape[:-1]), dy.device
        f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        if M == 0:
            z = lambda need, *shape: torch.zeros(*shape, dtype=torch.float32, device=dev) if need else None
            return z(nx, *xshape), z(nw, N, K), z(nb, N), None
        if dy.dtype != torch.float32:
            raise SdvarError(f"linear_grad: the gradient of the output is {dy.dtype} but the output is float32")
        lib, st, fmt, npl, Mp = E.load_library(), E._stream(), _OPERAND_FORMAT[mode], _OPERAND_PLANES[mode], _pad32(M)
        h16, el = mode == "f16x2", torch.float32 if mode == "f32" else torch.int16
        dy = _dense16(dy.reshape(M, N))             # stride-0 expansions, transposed consumers, a dense tensor at a misaligned address: one fresh dense copy
        off = lambda sc, floats: None if sc is None else C.c_void_p(sc.data_ptr() + 4 * floats)
        wt = sdy = None
        if nx:
            wt, swt = _weight_planes_t(weight, mode)
        if h16 and (nx or nw):       # the gradient operands carry a per-tensor power-of-two scale: the absmax pass, the one other read of dy
            sdy = torch.zeros(4, dtype=torch.float32, device=dev)
            E._check(lib.sdvar_op_scale_pair(_p(dy), M * N, _p(sdy), 0, _p(swt) if nx else None, st))
        dyo = torch.empty(npl, M * N, dtype=el, device=dev) if nx and mode != "f32" else None
        dyt = torch.empty(npl, N * Mp, dtype=el, device=dev) if nw else None
        part = f32(Mp // 32, N) if nb else None
        if dyo is not None or dyt is not None or part is not None:
            E._check(lib.sdvar_op_grad_operands(_p(dy), N, M, N, fmt, _p(sdy), _p(dyo), M * N, _p(dyt), N * Mp, _p(part), st))
        dx = dw = db = None
        if nx:
            dx = f32(M, K)
            _gemm_nt(mode, dy if mode == "f32" else dyo, wt, off(sdy, 2), dx, M, K, N, st=st)
            dx = dx.view(xshape)
        if nw:
            dw = f32(N, K)
            _gemm_nt(mode, dyt, _transposed_operand(rest[0], mode), off(sdy, 0), dw, N, K, Mp, st=st)
        if nb:
            db = f32(N)
            E._check(lib.sdvar_op_colsum(_p(part), N, Mp // 32, N, _p(db), st))
        return dx, dw, db, None


def linear_grad(x, weight, bias=None):
    """linear under autograd (the reference's mat_qkv, proj, ada_lin, word_embed and head, and fc1 / fc2 where the FFN slot is empty): signature, operand rules and argument
    errors as linear, plus out_features % 32 == 0 under grad.  With grad mode off, or nothing requiring grad, it IS linear (same launches, same bits).  Backward:
    dx = dy W, dW = dy^T x as two NT GEMMs of the configured mode (the mode of the forward call), db = sum_m dy.  dy is read ONCE: one sdvar_op_grad_operands pass
    writes the row-major operand for dx, the transposed, zero-padded operand for dW and db's 32-row partials (finished by a fixed-order column sum); in mode f16x2 the
    per-tensor power-of-two scale's absmax pass comes before it.  Saved: x as a dense (M, K) tensor and the weight; nothing of x when the weight does not require grad.
    Only the gradients autograd asks for are computed (a frozen weight costs no wgrad GEMM and no transposed operand, an x without grad no dgrad GEMM), each has the
    bits it has in the full run, and repeats are bit-identical: no atomics, no host synchronisation.  A dy that is not dense or not 16-byte aligned is copied once.
    M == 0 returns zeros without a launch.  No double backward, float32 only."""
    who = "linear_grad"
    _, K, N = _linear_check(who, x, weight, bias, False, True)
    if not _linear_wants_grad(who, x, weight, bias, N):
        return _linear_forward(x, weight, bias, _gemm_mode)[0]            # what the inference twin launches: the same bits
    return _LinearGrad.apply(x, weight, bias, _gemm_mode)


def _linear_amp_forward(x, weight, bias, half):
    """(out, xop): half(fp32acc(x_h W_h^T) + b) as one sdvar_op_gemm_h launch behind one operand pass over x; xop = the half operand of x (None when M == 0)."""
    N, K = weight.shape
    xr = _rows16(x, K)
    M = xr.shape[0]
    out = torch.empty(tuple(x.shape[:-1]) + (N,), dtype=half, device=x.device)
    if M == 0:
        return out, None
    xop = _half_operand(xr, half, False)
    _gemm_h(half, xop, _weight_operand_h(weight, half, False), _bias_f32(bias), out, M, N, K)
    return out, xop


def linear_amp(x, weight, bias=None):
    """F.linear for a model run under torch.autocast, on the HALF matrix cores, under fused_mlp_func_amp's dtype rule: the half dtype is x.dtype when x is float16 /
    bfloat16, else the GPU's autocast dtype; with neither it raises (use linear).  x (..., K), weight (N, K) and bias (N,) are each float32 or that dtype - a float32
    operand is rounded to nearest even as it is read, the bias enters as float32.  Contract: y = half(fp32acc(x_h W_h^T) + b); nothing is clamped, an fp16 overflow is
    +-inf.  K % 32 == 0, N % 8 == 0.  One sdvar_op_gemm_h launch behind one operand pass over x; the weight's half operand comes from the FFN's cache.  Returns (..., N)
    in the half dtype.  Inference only: an operand that requires grad while grad mode is on raises (use linear_amp_grad)."""
    half, _, _ = _linear_check("linear_amp", x, weight, bias, True, False)
    return _linear_amp_forward(x, weight, bias, half)[0]


class _LinearAmpGrad(torch.autograd.Function):
    """The half-precision linear with a HIP backward: two sdvar_op_gemm_h launches on operands one sdvar_op_grad_operands_h pass writes.  Saved: the forward's half
    OPERAND of x (2 M K bytes; sdvar_op_operand_transpose_h turns it into the operand of x^T) and the weight; nothing of x when the weight is frozen."""

    @staticmethod
    def forward(ctx, x, weight, bias, half):
        out, xop = _linear_amp_forward(x, weight, bias, half)
        ctx.save_for_backward(weight, *((xop,) if ctx.needs_input_grad[1] and xop is not None else ()))
        ctx.lin = (half, tuple(x.shape), x.dtype, None if bias is None else bias.dtype)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        weight, *rest = ctx.saved_tensors
        half, xshape, xdt, bdt = ctx.lin
        nx, nw, nb = ctx.needs_input_grad[:3]
        N, K = weight.shape
        M, dev = math.prod(xshape[:-1]), dy.device
        if dy.dtype != half:
            raise SdvarError(f"linear_amp_grad: the gradient of the output is {dy.dtype} but the output is {half}; the backward reads dy in the output's dtype")
        if M == 0:
            z = lambda need, dtype, *shape: torch.zeros(*shape, dtype=dtype, device=dev) if need else None
            return z(nx, xdt, *xshape), z(nw, weight.dtype, N, K), z(nb, bdt, N), None
        lib, st, dt, Mp = E.load_library(), E._stream(), _HALF_DTYPES[half], _pad32(M)
        operand = lambda need, n: torch.empty(n, dtype=torch.int16, device=dev) if need else None
        dy = _dense16(dy.reshape(M, N))             # stride-0 expansions, transposed consumers, a dense tensor at a misaligned address: one fresh dense copy
        dyo, dyt = operand(nx, M * N), operand(nw, N * Mp)
        part = torch.empty(Mp // 32, N, dtype=torch.float32, device=dev) if nb else None
        dx = dw = db = None
        if nx or nw or nb:
            E._check(lib.sdvar_op_grad_operands_h(_p(dy), dt, N, M, N, dt, _p(dyo), _p(dyt), _p(part), st))
        if nx:
            dx = torch.empty(M, K, dtype=xdt, device=dev)
            _gemm_h(half, dyo, _weight_operand_h(weight, half, True), None, dx, M, K, N)
            dx = dx.view(xshape)
        if nw:
            xt = torch.empty(K * Mp, dtype=torch.int16, device=dev)
            E._check(lib.sdvar_op_operand_transpose_h(_p(rest[0]), M, K, _p(xt), st))
            dw = torch.empty(N, K, dtype=weight.dtype, device=dev)
            _gemm_h(half, dyt, xt, None, dw, N, K, Mp)
        if nb:
            db = torch.empty(N, dtype=torch.float32, device=dev)
            E._check(lib.sdvar_op_colsum(_p(part), N, Mp // 32, N, _p(db), st))
            db = db.to(bdt)
        return dx, dw, db, None


def linear_amp_grad(x, weight, bias=None):
    """linear_amp under autograd: signature, dtype rule, operand rules and argument errors as linear_amp, plus out_features % 32 == 0 under grad.  With grad mode off, or
    nothing requiring grad, it IS linear_amp (same launches, same bits).  Backward: dx = fp32acc(dy W_h), dW = fp32acc(dy^T x_h) as two sdvar_op_gemm_h launches,
    db = sum_m dy of the rounded values in a fixed order.  dy is read ONCE: one sdvar_op_grad_operands_h pass writes both operands and db's partials.  Saved: the
    forward's half operand of x - 2 M K bytes where an fp32 x would cost 4 M K; sdvar_op_operand_transpose_h makes the operand of x^T from it - and the weight; nothing
    of x when the weight does not require grad.  Gradients come back in each operand's OWN dtype: unrounded float32 for a float32 x / weight / bias (the reference's
    case: float32 activations into head and master weights), half otherwise.  dy must have the output's dtype; one that is not dense or not 16-byte aligned is copied
    once.  Only the gradients autograd asks for are computed, each with the bits it has in the full run; deterministic; nothing is clamped: an fp16 overflow is +-inf
    and reaches the GradScaler.  M == 0 returns zeros without a launch.  No double backward."""
    who = "linear_amp_grad"
    half, K, N = _linear_check(who, x, weight, bias, True, True)
    if not _linear_wants_grad(who, x, weight, bias, N):
        return _linear_amp_forward(x, weight, bias, half)[0]            # what the inference twin launches: the same bits
    return _LinearAmpGrad.apply(x, weight, bias, half)


def _linear_module_forward(self, input):
    """nn.Linear.forward on the seam, chosen at call time: a half input, or autocast enabled for the GPU with float16 / bfloat16 -> linear_amp_grad; else linear_grad.
    The reference's word_embed runs inside autocast(enabled=False) on a float32 x (models/var.py:225-231) and takes the float32 path in the middle of an autocast run;
    its head runs under autocast on a .float()-ed input (:125) and takes the half path."""
    if (isinstance(input, torch.Tensor) and input.dtype in _HALF_DTYPES) or _autocast_gpu_dtype() in _HALF_DTYPES:
        return linear_amp_grad(input, self.weight, self.bias)
    return linear_grad(input, self.weight, self.bias)


def _install_linears(who: str, model) -> None:
    if model is None:
        raise SdvarError(f"{who}: linears=True binds a forward on the model's own nn.Linear modules; pass the model (model=None has nothing to bind)")
    for m in model.modules():
        if isinstance(m, torch.nn.Linear) and m.in_features % 32 == 0 and m.out_features % 32 == 0:
            m.forward = types.MethodType(_linear_module_forward, m)


def install_linears(model) -> None:
    """Bind the seam's linear on every nn.Linear of `model` whose in_features and out_features are multiples of 32 (others are left with torch), for inference on top
    of install() / install_amp() or on top of any other install_* call.  One bound forward, dispatching at call time: a half input, or autocast enabled for the GPU ->
    linear_amp_grad; otherwise linear_grad (each is its inference twin under torch.no_grad()).  Only calls of the MODULE are served: the reference's SelfAttention
    calls F.linear(input=x, weight=self.mat_qkv.weight, ...) directly (basic_var.py:93), so without qknorm=True - whose bound forward calls self.mat_qkv(x) - the QKV
    GEMM stays with torch; likewise fc1 / fc2 are reached only where the FFN slot is None."""
    _install_linears("install_linears", model)


def uninstall_linears(model) -> None:
    """Delete the instance-level `forward` that install_linears / install_train(..., linears=True) / install_train_amp(..., linears=True) bound: nn.Linear's own forward
    is back."""
    for m in model.modules():
        f = m.__dict__.get("forward")
        if getattr(f, "__func__", None) is _linear_module_forward:
            del m.forward


class _XentGrad(torch.autograd.Function):
    """Label-smoothed cross-entropy with a HIP backward: forward = sdvar_xent_train_fwd, backward = one sdvar_xent_train_bwd call (csrc/xent_train.hip).  Saved: the
    logits, the targets and lse (one float per row); reduction 'mean' also keeps the forward's two doubles {sum, counted rows}."""

    @staticmethod
    def forward(ctx, logits, target, eps, reduction, ignore_index):
        loss, lse, sums, reduced = E.xent_train_fwd(logits, target, eps, ignore_index, reduction, True)
        ctx.save_for_backward(logits, target, lse, *(() if sums is None else (sums,)))
        ctx.xent = (eps, reduction, ignore_index)
        return loss if reduction == "none" else reduced

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            raise SdvarError("cross_entropy: double backward (backward(create_graph=True), or torch.autograd.grad of a gradient) is not supported; "
                             "call backward() without create_graph")
        if not ctx.needs_input_grad[0]:
            return (None,) * 5
        logits, target, lse, *rest = ctx.saved_tensors
        eps, reduction, ignore_index = ctx.xent
        if g.dtype != torch.float32:
            raise SdvarError(f"cross_entropy: the gradient of the loss is {g.dtype} but the loss is float32")
        g = g.contiguous()            # a stride-0 expansion (loss.sum().backward()) becomes rows floats; a dense gradient is read in place
        return E.xent_train_bwd(logits, target, lse, g, reduction, rest[0] if rest else None, eps, ignore_index), None, None, None, None


def cross_entropy(input, target, label_smoothing: float = 0.0, reduction: str = "none", ignore_index: int = -100, weight=None):
    """The loss of the reference's trainer (trainer.py:37-38, called at :112 and reduced at :116-120) with torch's definition of label smoothing:
    loss = (1 - eps)(lse - x_t) + eps (lse - mean_j x_j).  input (N, V) float32 on the GPU, V a multiple of 4; rows with unit column stride, a row stride that is a
    multiple of 4 and 16-byte alignment are read in place (logits[:n], logits[:, :V] of a wider buffer), anything else is copied once.  target (N,) int64 class
    indices.  reduction 'none' -> (N,) float32; 'mean' (divided by the rows whose target is not ignore_index, as torch) / 'sum' -> a 0-dim float32 tensor, reduced in
    float64 in a fixed order.  A target == ignore_index gives loss 0 and gradient 0; any other target outside [0, V) gives NaN for that row's loss and gradient (torch
    asserts on the device instead) and leaves every other row alone.  One pass over the logits, one float per row saved for the backward, which is one read and one
    write; deterministic; neither direction synchronises with the host.  Under torch.no_grad(), or when input does not require grad, the same kernel runs without
    writing lse: the same loss bits.  Not autocast-aware: the input must already be float32 (the reference's get_logits ends in .float(), var.py:125).  No class
    weights, no soft targets, no double backward."""
    who = "cross_entropy"
    if weight is not None:
        raise SdvarError(f"{who}: weight= (per-class weights) is not supported; pass weight=None (the reference's trainer uses none) and weigh the 'none' losses yourself")
    if reduction not in E.XENT_REDUCTIONS:
        raise SdvarError(f"{who}: reduction {reduction!r} is not one of {E.XENT_REDUCTIONS}")
    eps = float(label_smoothing)
    if not 0.0 <= eps <= 1.0:
        raise SdvarError(f"{who}: label_smoothing {label_smoothing} is outside [0, 1]")
    if not isinstance(input, torch.Tensor) or not isinstance(target, torch.Tensor):
        raise SdvarError(f"{who}: input and target must be tensors")
    if input.dtype in _HALF_DTYPES or input.dtype == torch.float64:
        raise SdvarError(f"{who}: input is {input.dtype}; only float32 logits are supported - pass input.float() (the reference's get_logits already ends in .float())")
    if input.dtype != torch.float32:
        raise SdvarError(f"{who}: input is {input.dtype}; only float32 logits are supported")
    if input.dim() != 2:
        raise SdvarError(f"{who}: input has {input.dim()} dims, expected (N, V) - flatten it as the trainer does: input.view(-1, V), target.view(-1)")
    if not input.is_cuda or not target.is_cuda or input.device != target.device:
        raise SdvarError(f"{who}: input ({input.device}) and target ({target.device}) must be on one GPU (the kernels run on the GPU; there is no CPU path)")
    if target.dtype != torch.int64 or target.dim() != 1 or target.shape[0] != input.shape[0]:
        raise SdvarError(f"{who}: target is {target.dtype} of shape {tuple(target.shape)}; expected int64 class indices of shape ({input.shape[0]},) (no soft targets)")
    N, V = input.shape
    if N < 1 or V < 4 or V % 4:
        raise SdvarError(f"{who}: input of shape {(N, V)}: N must be at least 1 and V a positive multiple of 4")
    target = target.detach().contiguous()
    grad = torch.is_grad_enabled() and input.requires_grad
    x = input if grad else input.detach()
    ld = V if N == 1 else x.stride(0)
    if x.stride(1) != 1 or ld < V or ld % 4 or x.data_ptr() % 16:
        x = x.clone(memory_format=torch.contiguous_format)           # differentiable: the gradient flows back through the copy
    if grad:
        return _XentGrad.apply(x, target, eps, reduction, int(ignore_index))
    loss, _, _, reduced = E.xent_train_fwd(x, target, eps, int(ignore_index), reduction, False)
    return loss if reduction == "none" else reduced


class CrossEntropyLoss:
    """nn.CrossEntropyLoss's call shape on cross_entropy: a plain callable (no parameters, no buffers) for the trainer's `train_loss` / `val_loss` attributes
    (trainer.py:37-38)."""

    def __init__(self, label_smoothing: float = 0.0, reduction: str = "mean", ignore_index: int = -100, weight=None):
        if weight is not None:
            raise SdvarError("CrossEntropyLoss: weight= (per-class weights) is not supported; pass weight=None")
        if reduction not in E.XENT_REDUCTIONS:
            raise SdvarError(f"CrossEntropyLoss: reduction {reduction!r} is not one of {E.XENT_REDUCTIONS}")
        if not 0.0 <= float(label_smoothing) <= 1.0:
            raise SdvarError(f"CrossEntropyLoss: label_smoothing {label_smoothing} is outside [0, 1]")
        self.label_smoothing, self.reduction, self.ignore_index = float(label_smoothing), reduction, int(ignore_index)

    def __call__(self, input, target):
        return cross_entropy(input, target, self.label_smoothing, self.reduction, self.ignore_index)

    forward = __call__

    def __repr__(self) -> str:
        return f"seam.CrossEntropyLoss(label_smoothing={self.label_smoothing}, reduction={self.reduction!r}, ignore_index={self.ignore_index})"


def install_trainer(trainer) -> None:
    """Set the two loss attributes of a VARTrainer-like object (trainer.py:36-38): `train_loss` = CrossEntropyLoss(label_smoothing=trainer.label_smooth,
    reduction='none') - the loss train_step backpropagates (:112-120) - and `val_loss` = CrossEntropyLoss(label_smoothing=0.0, reduction='mean'), which eval_ep and
    the log lines call.  The trainer's code is not edited: both are instance attributes it looks up at every call."""
    if not hasattr(trainer, "label_smooth"):
        raise SdvarError("install_trainer: the object has no `label_smooth` attribute (a VARTrainer sets it at trainer.py:36); set train_loss / val_loss yourself "
                         "with seam.CrossEntropyLoss")
    trainer.train_loss = CrossEntropyLoss(label_smoothing=trainer.label_smooth, reduction="none")
    trainer.val_loss = CrossEntropyLoss(label_smoothing=0.0, reduction="mean")


# ------------------------------------------------------------------------------------------------------- the optimizer step (csrc/optim.hip)
_OPT_IGNORED = {"fused": None, "foreach": None, "capturable": False, "differentiable": False}          # torch's keywords that select an implementation: accepted, kept in the groups, unused


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW's update (decoupled weight decay, no amsgrad, no maximize) with GradScaler's unscale and clip_grad_norm_ folded in, as two passes over the
    gradients and the state (csrc/optim.hip: sdvar_optim_grad_stats, sdvar_optim_adamw_step) - what the reference's AmpOptimizer.backward_clip_step (utils/amp_sc.py:39-75)
    issues as unscale_, clip_grad_norm_ and AdamW.step.  It can stand in as the `opt_clz` of train.py:118: torch's `fused`, `foreach`, `capturable` and `differentiable`
    keywords are accepted and ignored; amsgrad=True or maximize=True raise SdvarError.
    step(): pass 1 reads every gradient once and leaves on the device norm = |g|_2 * inv_scale (float64 sums in a fixed order), coef = 1 when grad_clip <= 0, else
    min(1, grad_clip / (norm + 1e-6)) (clip_grad_norm_'s definition), and skip = 1 when a gradient element or the norm is not finite or `found_inf` > 0; pass 2 applies
        g' = g * (inv_scale * coef);  p <- p (1 - lr wd);  m <- b1 m + (1 - b1) g';  v <- b2 v + (1 - b2) g'^2;  p <- p - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
    with one read of g, p, m, v and one write of p, m, v.  On a skipped step nothing is written: p, m, v and every `step` keep their bits.  THE GRADIENTS ARE NEVER
    MODIFIED: after torch's clip_grad_norm_ `.grad` holds the clipped values, here it holds what backward() left (the reference drops the gradients on the next line).
    `grad_scale` and `found_inf`, the attributes GradScaler.step sets on an optimizer with _step_supports_amp_scaling, are honoured as torch's fused AdamW honours them:
    inv_scale = 1 / grad_scale, or 1 when it is None (the caller already ran unscale_: the reference's flow).  After every step() `global_grad_norm` is a 0-dim float32
    device tensor, the norm of the UNSCALED gradients before clipping (non-finite if they were) - the attribute that switches the reference's AmpOptimizer to late
    clipping (amp_sc.py:34-35, 70-71) - and `stats_record` the float32 device tensor {norm, coef, skip, inv_scale * coef}; both are set without a host synchronisation.
    The `_version` of every parameter and state tensor handed to the kernels moves at each step(), a skipped one included (the host does not know), as after torch's
    in-place update: fused_mlp_func's cached weight planes are rebuilt and autograd refuses a stale saved tensor.
    float32 parameters, gradients and state on ONE GPU only; parameters must be contiguous; a non-contiguous gradient is copied once; parameters without a gradient and
    zero-element parameters are skipped.  Everything else raises SdvarError naming the parameter's index (its position over all groups): there is no fall-back to torch.
    betas and eps must be the same in every group (lr and weight_decay are per group).  These checks happen in step(): the object is built, saved and loaded without a
    GPU.  State keys are torch's (`step`: 0-dim float32 device tensor, `exp_avg`, `exp_avg_sq`): a state_dict() loads into torch.optim.AdamW and back; `step` counters a
    non-fused torch checkpoint keeps on the CPU are moved to the device at the next step().  step() launches on the current stream, never synchronises with the host
    (no .item(), no get_scale()) and takes no closure."""

    _step_supports_amp_scaling = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_clip: float = 0.0, amsgrad: bool = False, maximize: bool = False,
                 **torch_kwargs):
        who = "seam.AdamW"
        if amsgrad or maximize:
            raise SdvarError(f"{who}: amsgrad={amsgrad}, maximize={maximize}: neither is supported (the kernel is plain decoupled AdamW); pass False")
        unknown = sorted(set(torch_kwargs) - set(_OPT_IGNORED))
        if unknown:
            raise SdvarError(f"{who}: unknown keyword(s) {unknown}; beside torch.optim.AdamW's own arguments only grad_clip is taken")
        if not (isinstance(betas, (tuple, list)) and len(betas) == 2 and all(0.0 <= float(b) < 1.0 for b in betas)):
            raise SdvarError(f"{who}: betas={betas!r} must be two numbers in [0, 1)")
        for name, val in (("lr", lr), ("eps", eps), ("weight_decay", weight_decay)):
            if not float(val) >= 0.0:
                raise SdvarError(f"{who}: {name}={val} must be >= 0")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, **{**_OPT_IGNORED, **torch_kwargs})
        super().__init__(params, defaults)
        self.grad_clip = float(grad_clip)
        self.global_grad_norm = None          # present from construction: AmpOptimizer looks for the attribute (amp_sc.py:34-35)
        self.stats_record = None

    def __getstate__(self):
        return {**super().__getstate__(), "grad_clip": self.grad_clip}

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("grad_clip", 0.0)
        self.global_grad_norm = self.stats_record = None

    @staticmethod
    def _state_of(who: str, idx: int, p, st: dict):
        """The parameter's state in the form the kernels read: created on first use, a loaded checkpoint's tensors moved to the parameter's GPU as float32."""
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            return st
        missing = [k for k in ("step", "exp_avg", "exp_avg_sq") if k not in st]
        if missing:
            raise SdvarError(f"{who}: the state of parameter {idx} has no {' / '.join(missing)} (not an Adam / AdamW state)")
        s = st["step"]
        if not isinstance(s, torch.Tensor):
            st["step"] = torch.tensor(float(s), dtype=torch.float32, device=p.device)
        elif s.device != p.device or s.dtype != torch.float32 or s.dim() != 0:
            if s.numel() != 1:
                raise SdvarError(f"{who}: the `step` of parameter {idx} has {s.numel()} elements, expected 1")
            st["step"] = s.detach().to(device=p.device, dtype=torch.float32).reshape(())
        for k in ("exp_avg", "exp_avg_sq"):
            t = st[k]
            if not isinstance(t, torch.Tensor) or t.numel() != p.numel():
                raise SdvarError(f"{who}: `{k}` of parameter {idx} does not have the parameter's {p.numel()} elements")
            if t.device != p.device or t.dtype != torch.float32 or not t.is_contiguous():
                st[k] = t.detach().to(device=p.device, dtype=torch.float32).contiguous()
        return st

    @torch.no_grad()
    def step(self, closure=None):
        who = "seam.AdamW.step"
        if closure is not None:
            raise SdvarError(f"{who}: a closure is not supported; evaluate the loss and call backward() before step()")
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        rows, numels, keep, written = [], [], [], []
        dev = betas = eps = None
        idx = -1
        for gi, group in enumerate(self.param_groups):
            if group.get("amsgrad") or group.get("maximize"):
                raise SdvarError(f"{who}: group {gi} has amsgrad={group.get('amsgrad')}, maximize={group.get('maximize')}: neither is supported")
            gb, ge = (float(group["betas"][0]), float(group["betas"][1])), float(group["eps"])
            if betas is None:
                betas, eps = gb, ge
            elif gb != betas or ge != eps:
                raise SdvarError(f"{who}: group {gi} has betas={gb}, eps={ge} but group 0 has betas={betas}, eps={eps}: one pair of betas and one eps per optimizer "
                                 f"(lr and weight_decay may differ)")
            lr, wd = float(group["lr"]), float(group["weight_decay"])
            for p in group["params"]:
                idx += 1
                g = p.grad
                if g is None or p.numel() == 0:
                    continue
                if not p.is_cuda:
                    raise SdvarError(f"{who}: parameter {idx} is on {p.device}; the kernels run on the GPU and there is no CPU path")
                if p.dtype != torch.float32:
                    raise SdvarError(f"{who}: parameter {idx} is {p.dtype}; only float32 parameters, gradients and state are supported")
                if dev is None:
                    dev = p.device
                elif p.device != dev:
                    raise SdvarError(f"{who}: parameter {idx} is on {p.device} but an earlier one is on {dev}: one optimizer per GPU")
                if not p.is_contiguous():
                    raise SdvarError(f"{who}: parameter {idx} with strides {tuple(p.stride())} is not contiguous (it is updated in place and cannot be copied)")
                if g.is_sparse or g.layout != torch.strided:
                    raise SdvarError(f"{who}: the gradient of parameter {idx} is sparse ({g.layout}); dense gradients only")
                if g.dtype != torch.float32 or g.device != dev:
                    raise SdvarError(f"{who}: the gradient of parameter {idx} is {g.dtype} on {g.device}, expected float32 on {dev}")
                if not g.is_contiguous():
                    g = g.contiguous()          # copied once; the copy lives until the launches are enqueued (the caching allocator reuses it in stream order)
                    keep.append(g)
                st = self._state_of(who, idx, p, self.state[p])
                rows.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr(), p.numel(), lr, wd))
                numels.append(p.numel())
                written.extend((p, st["exp_avg"], st["exp_avg_sq"], st["step"]))
        if not rows:
            self.stats_record = torch.tensor([0.0, 1.0, 0.0, 1.0], dtype=torch.float32, device=dev)
            self.global_grad_norm = self.stats_record[0]
            return None
        for name, t in (("grad_scale", grad_scale), ("found_inf", found_inf)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.float32 and t.numel() == 1):
                raise SdvarError(f"{who}: {name} must be a one-element float32 tensor on {dev} (what GradScaler.step sets), got {t!r}")
        table = E.optim_table(rows)
        with E._on_device(dev):
            ws = torch.empty(E.optim_ws_bytes(numels) // 4, dtype=torch.float32, device=dev)          # fresh every step: global_grad_norm stays valid after the next one
            E.optim_grad_stats(table, grad_scale, found_inf, self.grad_clip, betas[0], betas[1], ws)
            E.optim_adamw_step(table, betas[0], betas[1], eps, ws)
        torch._C._increment_version(written)          # the kernels write through raw pointers: autograd's saved-tensor check and the seam's weight-plane cache go by _version
        self.stats_record = ws[:4]
        self.global_grad_norm = ws[0]
        return None


def install_optimizer(var_opt) -> None:
    """Replace the torch.optim.AdamW (or Adam) of an AmpOptimizer-like object (utils/amp_sc.py:15-37) by a seam.AdamW over the same parameters: every param group entry
    is carried over (the `lr_sc` / `wd_sc` keys lr_wd_annealing reads included) and every state tensor; grad_clip = var_opt.grad_clip; and the two flags are set to what
    the reference's constructor computes for an optimizer that has `global_grad_norm`: early_clipping = False, late_clipping = grad_clip > 0 - backward_clip_step then
    runs no clip_grad_norm_ of its own and reads the norm after the step.  Any other optimizer class, an amsgrad / maximize group, or a torch.optim.Adam whose weight
    decay is the coupled L2 kind (weight_decay != 0 without decoupled_weight_decay) raises SdvarError: the kernel computes the decoupled form only.  The reference's code
    is not edited."""
    who = "install_optimizer"
    old = getattr(var_opt, "optimizer", None)
    if not isinstance(old, (torch.optim.AdamW, torch.optim.Adam)):
        raise SdvarError(f"{who}: var_opt.optimizer is a {type(old).__name__}; only torch.optim.AdamW / Adam can be replaced by seam.AdamW")
    if not hasattr(var_opt, "grad_clip"):
        raise SdvarError(f"{who}: the object has no `grad_clip` attribute (an AmpOptimizer sets it at amp_sc.py:33)")
    groups = []
    for gi, group in enumerate(old.param_groups):
        if group.get("amsgrad") or group.get("maximize"):
            raise SdvarError(f"{who}: group {gi} has amsgrad={group.get('amsgrad')}, maximize={group.get('maximize')}: neither is supported")
        if not isinstance(old, torch.optim.AdamW) and not group.get("decoupled_weight_decay", False) and float(group["weight_decay"]) != 0.0:
            raise SdvarError(f"{who}: group {gi} of a torch.optim.Adam has weight_decay={group['weight_decay']} as an L2 term in the gradient; seam.AdamW decays the "
                             f"weights directly (use AdamW, decoupled_weight_decay=True or weight_decay=0)")
        groups.append(dict(group))
    new = AdamW(groups, grad_clip=float(var_opt.grad_clip))
    for p, st in old.state.items():
        new.state[p] = dict(st)
    var_opt.optimizer = new
    var_opt.early_clipping = False
    var_opt.late_clipping = float(var_opt.grad_clip) > 0


def _set_ffn_slots(module, model, slot) -> None:
    """The `fused_mlp_func` global of the module and, with a model, every `ffn.fused_mlp_func` its FFN modules captured at construction (basic_var.py:36)."""
    module.fused_mlp_func = slot
    if model is not None:
        for m in model.modules():
            if hasattr(m, "fused_mlp_func") and not callable(getattr(type(m), "fused_mlp_func", None)):
                m.fused_mlp_func = slot


def _set_using_flash(model) -> None:
    """`using_flash = True` on every submodule of a model that has the attribute (the reference decides it at construction, basic_var.py:81)."""
    if model is not None:
        for m in model.modules():
            if hasattr(m, "using_flash"):
                m.using_flash = True


def install(module, model=None) -> None:
    """Set the `slow_attn` and `fused_mlp_func` globals of a basic_var-like module; with a model, also every `ffn.fused_mlp_func` its FFN modules captured at
    construction (basic_var.py:36).  `memory_efficient_attention` is left alone: setting it would not switch an existing model to it (using_xform is decided at
    construction, basic_var.py:82); assign seam.memory_efficient_attention yourself before building the model if you want the BLHc route."""
    module.slow_attn = slow_attn
    _set_ffn_slots(module, model, fused_mlp_func)


def enable_flash(module, model=None) -> None:
    """Set the `flash_attn_func` global of a basic_var-like module; with a model, also `using_flash = True` on every submodule that has a `using_flash` attribute
    (the reference decides that flag at construction, basic_var.py:81, from whether flash-attn could be imported).  Separate from install(): the slot only serves
    half-precision operands, i.e. a model run under torch.autocast."""
    module.flash_attn_func = flash_attn_func
    _set_using_flash(model)


def install_amp(module, model=None, ffn_half: bool = False) -> None:
    """For a model run under torch.autocast: install(), then enable_flash(), then `module.slow_attn = slow_attn_amp`, which serves the masked calls (the
    teacher-forced pass, the verifier's attn_bias, the hand-off prefill) on the half or mixed operands autocast delivers.  ffn_half=False (default): the FFN slots
    keep install()'s float32 fused_mlp_func.  ffn_half=True: they become fused_mlp_func_amp, the FFN on the half matrix cores in autocast's dtype.
    `memory_efficient_attention` is left alone for the reason install() documents; assign seam.memory_efficient_attention_amp yourself before building the model if
    you want the BLHc route."""
    install(module, model)
    enable_flash(module, model)
    module.slow_attn = slow_attn_amp
    if ffn_half:
        _set_ffn_slots(module, model, fused_mlp_func_amp)


def install_train(module, model=None, ffn: bool = False, adaln: bool = False, qknorm: bool = False, linears: bool = False, cond: bool = False,
                  embed: bool = False) -> None:
    """For TRAINING the reference in fp32 with the seam's operators: `module.slow_attn = slow_attn_grad`.  ffn=False (default): `module.fused_mlp_func = None` plus
    `m.fused_mlp_func = None` on every FFN of `model` that captured one, so that the reference runs its own fc2(act(fc1(x))) under autograd (basic_var.py:52) - the
    state it is in without flash-attn installed.  ffn=True: those slots are set to fused_mlp_func_grad instead (HIP forward + backward for the FFN, out_features % 32
    == 0).  `memory_efficient_attention` is left alone for the reason install() documents; assign seam.memory_efficient_attention_grad yourself before building the
    model if you want the BLHc route.  A model trained under torch.autocast needs install_train_amp instead: the slots set here are float32 only, and flash_attn_func
    and the _amp slots still raise on operands that require grad.  adaln=True (needs the model) also binds an instance-level `forward` on every submodule that has
    `ln_wo_grad`: blocks (those with attn, ffn and ada_lin or ada_gss) run basic_var.py:152-159 with adaln_modulate for the two modulations and gated_residual for the
    two residual lines - DropPath's per-image factor, drawn as helpers.py:43-45 draws it, goes in as row_scale - and head norms run :172-174 on adaln_modulate;
    attn and ffn are still called as modules, so the slots above keep working.  uninstall_adaln(model) removes the bound forwards.  adaln=False (default) binds
    nothing.  qknorm=True (needs the model) binds an instance-level `forward` on every submodule that has `mat_qkv` and attn_l2_norm=True: basic_var.py:90-119 with
    qk_l2norm between the QKV GEMM and the attention call; the attention slots are still read from the reference module at call time.  uninstall_qknorm(model) removes
    them.  qknorm=False (default) binds nothing.  linears=True (needs the model) binds install_linears' forward on every nn.Linear whose in_features and out_features
    are multiples of 32: mat_qkv (reached through qknorm=True's forward only - the class forward calls F.linear itself, basic_var.py:93), proj, the Linear inside
    ada_lin, word_embed and head, and fc1 / fc2 where ffn=False leaves them to the module - linear_grad, forward and backward on HIP.  uninstall_linears(model)
    removes them.  linears=False (default) binds nothing.  cond=True (needs the model) binds install_cond's forward on every Sequential(SiLU, Linear) - the ada_lin of
    the blocks and of the head norm: ada_lin, one kernel forward and two backward for the batches cond_serves() accepts (at most 64 rows; above 16 rows at most 2^23
    weights), float32 arithmetic here; with linears=True the Linear
    inside keeps its bound forward for larger batches and its weight stays out of the weight-operand cache otherwise.  uninstall_cond(model) removes them.  cond=False
    (default) binds nothing.  embed=True (needs the model) binds install_embed's forward on the VAR-like module itself: var.py:217-259 with teacher_embed - one kernel -
    for everything in front of the blocks; word_embed's module forward is no longer called.  uninstall_embed(model) removes it.  embed=False (default) binds nothing."""
    if adaln:
        _install_adaln("install_train", model)
    if qknorm:
        _install_qknorm("install_train", model)
    if linears:
        _install_linears("install_train", model)
    if cond:
        _install_cond("install_train", model)
    if embed:
        _install_embed("install_train", model)
    module.slow_attn = slow_attn_grad
    _set_ffn_slots(module, model, fused_mlp_func_grad if ffn else None)


def install_train_amp(module, model=None, ffn=False, adaln: bool = False, qknorm: bool = False, linears: bool = False, cond: bool = False,
                      embed: bool = False) -> None:
    """For TRAINING the reference under torch.autocast (utils/amp_sc.py; fp16 with a GradScaler, or bf16): `module.slow_attn = slow_attn_amp_grad` and
    `module.flash_attn_func = flash_attn_func_grad`, and with a model `using_flash = True` on every submodule that has the attribute (as enable_flash does), so that
    the unmasked calls on half operands take the flash slot.  The FFN slots are handled as install_train handles them: ffn=False (default) sets them to None and the
    reference runs its own fc2(act(fc1(x))) under autocast; ffn=True sets them to fused_mlp_func_grad.  That function takes float32 operands ONLY and is not
    autocast-aware: it runs its own fp32-operand GEMMs whatever autocast says, and RAISES SdvarError on a half-precision x.  The reference's FFN input is the output
    of a LayerNorm and the adaLN modulation, which autocast keeps in float32, so ffn=True works there; a model that hands its FFN a half x must use ffn=False or
    ffn="half".  ffn="half" sets them to fused_mlp_func_amp_grad: the FFN's forward and backward on the half matrix cores in autocast's dtype (float32 or half x,
    float32 master weights; out_features % 32 == 0).  `memory_efficient_attention` is left alone for the reason install() documents; assign
    seam.memory_efficient_attention_amp_grad yourself before building the model if you want the BLHc route.  adaln=True: as install_train's; under autocast the
    modulation vectors and the branch outputs arrive in half and are read as they are.  qknorm=True: as install_train's; under autocast qkv arrives in half, q and k
    leave in float32 and v in half (the mixed operands slow_attn_amp_grad takes).  linears=True: as install_train's; the bound forward picks linear_amp_grad where
    autocast is enabled (or the input is half) and linear_grad where it is not - word_embed inside autocast(enabled=False), var.py:225-231.  cond=True: as
    install_train's; under autocast ada_lin computes in the autocast dtype and returns half, also for the float32 cond the head norm is given (var.py:125, 248).  embed=True: as
    install_train's; the blocks are handed x_BLC in float32 when adaln=True's forward is bound on them (the seam's float32 residual stream - the reference's own forward
    casts x_BLC to half, which adaln_modulate refuses, so adaln=True needs embed=True to run the reference model under autocast) and in the autocast dtype otherwise."""
    if adaln:
        _install_adaln("install_train_amp", model)
    if qknorm:
        _install_qknorm("install_train_amp", model)
    if linears:
        _install_linears("install_train_amp", model)
    if cond:
        _install_cond("install_train_amp", model)
    if embed:
        _install_embed("install_train_amp", model)
    if isinstance(ffn, str):
        if ffn != "half":
            raise SdvarError(f"install_train_amp: ffn={ffn!r}; expected False, True or 'half'")
        slot = fused_mlp_func_amp_grad
    else:
        slot = fused_mlp_func_grad if ffn else None
    module.slow_attn = slow_attn_amp_grad
    module.flash_attn_func = flash_attn_func_grad
    _set_using_flash(model)
    _set_ffn_slots(module, model, slot)


# ------------------------------------------------------------------------------------------------------- adaLN modulation and gated residual (csrc/adaln_train.hip)
def _train_x(x):
    """x as the kernels read it: itself when dense and 16-byte aligned, else one dense copy (differentiable).  Anything else is left for the engine's checks to name."""
    if isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 3 and x.dtype in E.TRAIN_DTYPES and (not x.is_contiguous() or x.data_ptr() % 16):
        return x.clone(memory_format=torch.contiguous_format)
    return x


def _train_vec(t):
    """A modulation vector as the kernels read it: itself under the 16-byte rule, else one dense copy (differentiable)."""
    if isinstance(t, torch.Tensor) and t.is_cuda and t.dim() in (2, 3) and t.dtype in E.TRAIN_DTYPES and not E.train_vec_in_place(t):
        return t.clone(memory_format=torch.contiguous_format)
    return t


def _train_grad(who: str, g: torch.Tensor) -> torch.Tensor:
    if g.dtype != torch.float32:
        raise SdvarError(f"{who}: the gradient of the output is {g.dtype} but the output is float32")
    return _dense16(g)          # a stride-0 expansion (out.sum().backward()) becomes one dense tensor; a dense gradient is read in place


def _no_double_backward(who: str) -> None:
    if torch.is_grad_enabled():
        raise SdvarError(f"{who}: double backward (backward(create_graph=True), or torch.autograd.grad of a gradient) is not supported; "
                         "call backward() without create_graph")


class _AdalnGrad(torch.autograd.Function):
    """adaln_modulate with a HIP backward (sdvar_op_adaln_fwd / sdvar_op_adaln_bwd).  Saved: x and scale; mean and rstd are recomputed in the backward with the
    forward's code."""

    @staticmethod
    def forward(ctx, x, scale, shift, eps):
        h = E.adaln_fwd(x, scale, shift, eps)
        ctx.save_for_backward(x, scale)
        ctx.ada = (eps, shift.dtype, tuple(shift.shape))
        return h

    @staticmethod
    def backward(ctx, g):
        _no_double_backward("adaln_modulate")
        nx, ns, nh = ctx.needs_input_grad[:3]
        if not (nx or ns or nh):
            return None, None, None, None
        x, scale = ctx.saved_tensors
        eps, hdtype, hshape = ctx.ada
        dx, ds, dh = E.adaln_bwd(x, scale, _train_grad("adaln_modulate", g), eps, hdtype, scale.shape[0], hshape[0], (nx, ns, nh))
        return dx, None if ds is None else ds.view(scale.shape), None if dh is None else dh.view(hshape), None


def adaln_modulate(x, scale, shift, eps: float = 1e-6):
    """The modulated LayerNorm of a block and of the head norm (basic_var.py:157-158, :174: `ln_wo_grad(x).mul(scale.add(1)).add_(shift)`) as one kernel per direction:
    h = ((x - mean) * rstd) * (scale + 1) + shift, mean = the row mean, rstd = 1 / sqrt(var + eps) with the biased two-pass variance, every operation in float32.
    x (B, L, C) float32 on the GPU, C a multiple of 4 in [4, 3072]; a dense, 16-byte aligned x is read in place, anything else is copied once.  scale and shift are
    (B, 1, C), (1, 1, C) or (B, C), each float32, float16 or bfloat16 on its own (one half dtype per call): rows with unit last stride and 16-byte alignment - the
    unbind(2) views of the reference's (B, 1, 6, C) / (B, 1, 2, C) buffers - are read in place, anything else is copied once.  A half scale is widened to float32
    BEFORE the + 1, where torch's `scale.add(1)` rounds 1 + scale to half: this side is the more accurate one and differs from autocast's eager result by up to half
    a half ulp of 1 + scale.  Returns (B, L, C) float32.  Differentiable: dx, and dscale / dshift summed over L (and over B for a (1, 1, C) operand) in float32 in a
    fixed order and rounded once to the operand's own dtype; nothing is clamped (an fp16 overflow is inf and reaches the GradScaler); no atomics, repeats are
    bit-identical; only the gradients autograd asks for are computed.  Saved for the backward: x and scale.  Under torch.no_grad(), or when nothing requires grad,
    the same forward kernel runs: the same bits.  Neither direction synchronises with the host.  No double backward."""
    who = "adaln_modulate"
    x, scale, shift = _train_x(x), _train_vec(scale), _train_vec(shift)
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (x, scale, shift)):
        E._train_rows(who, "x", x, (torch.float32,))          # argument errors before autograd wraps them
        return _AdalnGrad.apply(x, scale, shift, float(eps))
    d = lambda t: t.detach() if isinstance(t, torch.Tensor) else t
    return E.adaln_fwd(d(x), d(scale), d(shift), float(eps))


class _GateAddGrad(torch.autograd.Function):
    """gated_residual with a HIP backward (sdvar_op_gate_add_fwd / sdvar_op_gate_add_bwd).  Saved: y, gamma and row_scale - nothing when only x needs a gradient."""

    @staticmethod
    def forward(ctx, x, y, gamma, row_scale):
        out = E.gate_add_fwd(x, y, gamma, row_scale)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            ctx.save_for_backward(y, gamma, *(() if row_scale is None else (row_scale,)))
        return out

    @staticmethod
    def backward(ctx, g):
        _no_double_backward("gated_residual")
        nx, ny, ng = ctx.needs_input_grad[:3]
        dy = dgamma = None
        if ny or ng:
            y, gamma, *rest = ctx.saved_tensors
            dy, dgamma = E.gate_add_bwd(_train_grad("gated_residual", g), y, gamma, rest[0] if rest else None, gamma.shape[0], (ny, ng))
            if dgamma is not None:
                dgamma = dgamma.view(gamma.shape)
        elif g.dtype != torch.float32:
            raise SdvarError(f"gated_residual: the gradient of the output is {g.dtype} but the output is float32")
        return (g if nx else None), dy, dgamma, None


def gated_residual(x, y, gamma, row_scale=None):
    """The residual line of a block (basic_var.py:157-158: `x + drop_path(branch.mul_(gamma))`) as one kernel: out = x + (y * gamma) * row_scale[b], without row_scale
    x + y * gamma.  x (B, L, C) float32; y (B, L, C) float32, float16 or bfloat16 (under autocast: the output of proj / fc2), not modified; gamma under
    adaln_modulate's rules for scale; row_scale (B,) float32 without gradient: DropPath's per-image factor, 0 or 1 / keep.  Half operands are widened and the products
    formed in float32, where the reference multiplies in half.  Returns (B, L, C) float32.  Differentiable: the gradient of x is the upstream gradient itself (no
    kernel, no copy), dy = g * gamma * row_scale[b] in y's dtype (exactly 0 on a dropped image), dgamma[b, c] = row_scale[b] * sum_l g y in gamma's dtype, summed in
    float32 in a fixed order and rounded once.  Saved for the backward: y, gamma, row_scale.  The other rules are adaln_modulate's."""
    who = "gated_residual"
    x, y, gamma = _train_x(x), _train_x(y), _train_vec(gamma)
    if isinstance(row_scale, torch.Tensor):
        if row_scale.requires_grad and torch.is_grad_enabled():
            raise SdvarError(f"{who}: row_scale requires grad; it carries no gradient (pass row_scale.detach())")
        row_scale = row_scale.detach()
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (x, y, gamma)):
        E._train_rows(who, "x", x, (torch.float32,))
        return _GateAddGrad.apply(x, y, gamma, row_scale)
    d = lambda t: t.detach() if isinstance(t, torch.Tensor) else t
    return E.gate_add_fwd(d(x), d(y), d(gamma), row_scale)


def _drop_path_scale(dp, y):
    """DropPath's per-image factor for the branch output y, drawn as the reference draws it (helpers.py:43-45) so that the generator moves as it does there; None when
    the module drops nothing (nn.Identity, drop_prob == 0, or eval mode)."""
    p = getattr(dp, "drop_prob", 0.0)
    if not p or not dp.training:
        return None
    keep = 1 - p
    r = y.new_empty((y.shape[0],) + (1,) * (y.dim() - 1)).bernoulli_(keep)
    if keep > 0.0 and getattr(dp, "scale_by_keep", True):
        r.div_(keep)
    return r.view(y.shape[0]).float()


def _adaln_block_forward(self, x, cond_BD, attn_bias):
    """AdaLNSelfAttn.forward (basic_var.py:152-159) on adaln_modulate / gated_residual; attn and ffn are called as modules."""
    if hasattr(self, "ada_gss"):
        gamma1, gamma2, scale1, scale2, shift1, shift2 = (self.ada_gss + cond_BD).unbind(2)
    else:
        gamma1, gamma2, scale1, scale2, shift1, shift2 = self.ada_lin(cond_BD).view(-1, 1, 6, x.shape[-1]).unbind(2)
    eps = getattr(self.ln_wo_grad, "eps", 1e-6)
    y = self.attn(adaln_modulate(x, scale1, shift1, eps), attn_bias=attn_bias)
    x = gated_residual(x, y, gamma1, _drop_path_scale(self.drop_path, y))
    y = self.ffn(adaln_modulate(x, scale2, shift2, eps))
    return gated_residual(x, y, gamma2, _drop_path_scale(self.drop_path, y))


def _adaln_head_forward(self, x_BLC, cond_BD):
    """AdaLNBeforeHead.forward (basic_var.py:172-174) on adaln_modulate."""
    scale, shift = self.ada_lin(cond_BD).view(-1, 1, 2, x_BLC.shape[-1]).unbind(2)
    return adaln_modulate(x_BLC, scale, shift, getattr(self.ln_wo_grad, "eps", 1e-6))


def _install_adaln(who: str, model) -> None:
    if model is None:
        raise SdvarError(f"{who}: adaln=True binds a forward on the model's own blocks and head norm; pass the model (model=None has nothing to bind)")
    for m in model.modules():
        if not hasattr(m, "ln_wo_grad"):
            continue
        if hasattr(m, "attn"):
            if not (hasattr(m, "ffn") and (hasattr(m, "ada_lin") or hasattr(m, "ada_gss"))):
                raise SdvarError(f"{who}: {type(m).__name__} has ln_wo_grad and attn but no ffn / ada_lin / ada_gss; adaln=True knows AdaLNSelfAttn-like blocks only")
            m.forward = types.MethodType(_adaln_block_forward, m)
        else:
            if not hasattr(m, "ada_lin"):
                raise SdvarError(f"{who}: {type(m).__name__} has ln_wo_grad but neither attn nor ada_lin; adaln=True knows AdaLNBeforeHead-like head norms only")
            m.forward = types.MethodType(_adaln_head_forward, m)


def uninstall_adaln(model) -> None:
    """Delete the instance-level `forward` that install_train(..., adaln=True) / install_train_amp(..., adaln=True) bound: the class's own forward is back."""
    for m in model.modules():
        f = m.__dict__.get("forward")
        if getattr(f, "__func__", None) in (_adaln_block_forward, _adaln_head_forward):
            del m.forward


# ------------------------------------------------------------------------------------------------------- the conditioning linears (csrc/cond_train.hip)
def _ada_lin_check(who: str, cond, weight, bias):
    """The argument checks of ada_lin -> (arithmetic dtype, M, N, K).  Nothing here touches the library."""
    named = [("cond", cond), ("weight", weight)] + ([] if bias is None else [("bias", bias)])
    for name, t in named:
        _gpu_tensor(who, name, t)
        if t.dtype == torch.float64:
            raise SdvarError(f"{who}: {name} is torch.float64; only float32, float16 and bfloat16 operands are supported - pass {name}.float()")
        if t.dtype != torch.float32 and t.dtype not in _HALF_DTYPES:
            raise SdvarError(f"{who}: {name} is {t.dtype}; only float32, float16 and bfloat16 operands are supported")
    halves = {t.dtype for _, t in named if t.dtype in _HALF_DTYPES}
    if len(halves) > 1:
        raise SdvarError(f"{who}: float16 mixed with bfloat16 ({', '.join(f'{n} is {t.dtype}' for n, t in named if t.dtype in _HALF_DTYPES)}); use one half dtype, or pass .float()")
    dtype = cond.dtype if cond.dtype in _HALF_DTYPES else _autocast_gpu_dtype()
    if dtype not in _HALF_DTYPES:
        dtype = torch.float32
    for name, t in named:
        if t.dtype in _HALF_DTYPES and t.dtype != dtype:
            if dtype == torch.float32:
                raise SdvarError(f"{who}: {name} is {t.dtype} next to float32 arithmetic (cond is float32 and torch.autocast is not enabled for the GPU); call it under "
                                 f"torch.autocast, pass a half cond, or pass {name}.float()")
            raise SdvarError(f"{who}: float16 mixed with bfloat16: {name} is {t.dtype} but the half dtype of the call is {dtype}; use one half dtype, or pass {name}.float()")
    if weight.dim() != 2 or cond.dim() < 1 or cond.shape[-1] != weight.shape[1]:
        raise SdvarError(f"{who}: shapes do not chain: cond {tuple(cond.shape)}, weight {tuple(weight.shape)} (cond (..., K) with weight (N, K))")
    N, K = weight.shape
    if bias is not None and tuple(bias.shape) != (N,):
        raise SdvarError(f"{who}: bias has shape {tuple(bias.shape)}, expected ({N},)")
    if any(t.device != cond.device for _, t in named):
        raise SdvarError(f"{who}: operands live on different devices; move weight and bias to cond's device")
    if K < 8 or K > E.COND_MAX_K or K % 8:
        raise SdvarError(f"{who}: in_features {K} (the last dim of cond) must be a multiple of 8 in [8, {E.COND_MAX_K}]; use linear_grad / linear_amp_grad behind torch's SiLU")
    if N < 8 or N % 8 or N * K >= 2 ** 31:
        raise SdvarError(f"{who}: out_features {N} (weight.shape[0]) must be a multiple of 8, at least 8, with N * K below 2^31; use linear_grad / linear_amp_grad behind torch's SiLU")
    M = cond.numel() // K
    if M > E.COND_MAX_M:
        raise SdvarError(f"{who}: cond has {M} rows; this kernel serves batches of at most {E.COND_MAX_M} rows - larger products belong to the GEMMs: use linear_grad / "
                         f"linear_amp_grad behind torch's SiLU")
    return dtype, M, N, K


def _cond_rows(cond: torch.Tensor, K: int) -> torch.Tensor:
    """cond (..., K) as the (M, K) matrix the kernels read: a view where its rows meet the 16-byte rule (unit last stride, aligned base, row stride a multiple of
    16 bytes - a column slice of a wider buffer is read in place), else one dense copy."""
    xr = cond.detach().reshape(-1, K)
    return xr if E.cond_rows_in_place(xr) else xr.clone(memory_format=torch.contiguous_format)


def _ada_lin_forward(cond, weight, bias, dtype, M: int, N: int, K: int):
    if M == 0:
        return torch.empty(tuple(cond.shape[:-1]) + (N,), dtype=dtype, device=cond.device)
    y = E.cond_lin_fwd(_cond_rows(cond, K), _dense16(weight.detach()), _bias_f32(bias), dtype)
    return y.view(tuple(cond.shape[:-1]) + (N,))


class _AdaLinGrad(torch.autograd.Function):
    """ada_lin with a HIP backward (sdvar_op_cond_lin_fwd / sdvar_op_cond_lin_bwd).  Saved: cond and the weight; s = silu(cond) is recomputed in the backward with the
    forward's code."""

    @staticmethod
    def forward(ctx, cond, weight, bias, dtype, dims):
        y = _ada_lin_forward(cond, weight, bias, dtype, *dims)
        ctx.save_for_backward(cond, weight)
        ctx.cl = (dtype, dims, None if bias is None else bias.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        _no_double_backward("ada_lin")
        nc, nw, nb = ctx.needs_input_grad[:3]
        if not (nc or nw or nb):
            return None, None, None, None, None
        cond, weight = ctx.saved_tensors
        dtype, (M, N, K), bdt = ctx.cl
        if dy.dtype != dtype:
            raise SdvarError(f"ada_lin: the gradient of the output is {dy.dtype} but the output is {dtype}; the backward reads dy in the output's dtype")
        if M == 0:
            z = lambda need, t, *shape: torch.zeros(*shape, dtype=t, device=dy.device) if need else None
            return z(nc, cond.dtype, *cond.shape), z(nw, weight.dtype, N, K), z(nb, bdt, N), None, None
        dy = _dense16(dy.reshape(M, N))             # a stride-0 expansion (y.sum().backward()) or a misaligned gradient: one fresh dense copy
        dc, dw, db = E.cond_lin_bwd(dy, _cond_rows(cond, K), _dense16(weight.detach()), dtype, (nc, nw, nb))
        return None if dc is None else dc.view(cond.shape), dw, None if db is None else db.to(bdt), None, None


def ada_lin(cond, weight, bias=None):
    """The conditioning path of a block and of the head norm, `Sequential(SiLU, Linear)(cond)` (basic_var.py:147, 156; :170, 173), as one kernel forward and two
    backward: y = silu(cond) W^T + b.  cond (..., K), weight (N, K), bias (N,) on the GPU -> (..., N).  A skinny product - the rows are the batch, at most 64 - so
    nothing of the GEMM seam is involved: no matrix cores, no operand planes, no weight-operand cache, and seam.configure(gemm_mode=...) has NO influence; W is
    streamed once per direction and the SiLU is folded into the read of cond (x / (1 + expf(-x)), the same code in both directions).
    Arithmetic (fused_mlp_func_amp's dtype rule): cond.dtype when cond is float16 / bfloat16, else the GPU's autocast dtype when autocast is enabled, else float32.
    float32: float32 operands only, every product enters a float32 sum by one fmaf in an order that depends on K alone, result float32.  Half (autocast's contract):
    s = silu(cond) is rounded once to the half dtype, a float32 weight is rounded to it as it is read (the bits of .to(dtype)), the sums are float32, the float32
    bias is added to the float32 sum, the result is rounded once to half and an overflow is +-inf; a float32 cond under autocast - the head norm's case, var.py:125,
    248 - gives a half result.  A row's bits do not depend on the batch size or on the other rows.
    Differentiable: dW = dy^T s (float32 sums over the batch in row order, written in the weight's own dtype: unrounded float32 for float32 master weights),
    db = sum_m dy, dcond = (dy W) silu'(cond) rounded once to cond's dtype.  THE ONE NUMERICAL DIFFERENCE from torch's autocast: there dy W is rounded to half before
    the SiLU derivative multiplies it; here the float32 sum goes into the derivative unrounded - this side is the more accurate one.  Only the gradients autograd
    asks for are computed (a frozen weight costs no dW, a cond without grad no read of W at all), each with the bits it has in the full run; no atomics, repeats are
    bit-identical; neither direction synchronises with the host.  Saved for the backward: cond and weight, nothing else.  With grad mode off, or nothing requiring
    grad, the same forward launch gives the same bits.  cond is read in place when its rows have unit last stride, a row stride that is a multiple of 4 elements
    (8 when half) and a 16-byte aligned base, else copied once; a dy that is not dense or not 16-byte aligned is copied once.  M == 0 returns without a launch.
    Limits: at most 64 rows (beyond: linear_grad / linear_amp_grad), K % 8 == 0 in [8, 4096], N % 8 == 0.  Above 16 rows the kernels are bound by arithmetic, not by
    the bytes of W, and lose to the GEMM path on a large weight (d30's ada_lin at 32 rows): install_cond's forward does not hand such calls here (cond_serves).  CPU tensors, float64, float16 mixed with bfloat16, a half
    weight next to float32 arithmetic and shapes that do not chain raise SdvarError - there is no fall-back to torch.  No double backward."""
    who = "ada_lin"
    dtype, M, N, K = _ada_lin_check(who, cond, weight, bias)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (cond, weight, bias)):
        return _AdaLinGrad.apply(cond, weight, bias, dtype, (M, N, K))
    return _ada_lin_forward(cond, weight, bias, dtype, M, N, K)


# Where the bound forward hands a call to ada_lin.  Up to 16 rows the kernels stream W once and are bound by its bytes.  Beyond, the forward takes a pass over W per 16
# rows and both directions are bound by their 2 M N K flop of plain fp32 fmaf: measured at 32 rows (tools/seam_cond_bench.py) that still beats the GEMM path
# at N K = 2.1 M - 7.4 M (d16's ada_lin and head norm, d30's head norm) and loses to it at 22 M (d30's ada_lin), so wide batches are served up to 2^23 weights only.
COND_WIDE_ROWS = 16
COND_WIDE_MAX_WEIGHTS = 1 << 23


def cond_serves(rows: int, N: int, K: int) -> bool:
    """Whether install_cond's bound forward calls ada_lin for a batch of `rows` rows into a Linear(K, N): at most 64 rows, and above 16 rows at most 2^23 weights."""
    return rows <= E.COND_MAX_M and (rows <= COND_WIDE_ROWS or N * K <= COND_WIDE_MAX_WEIGHTS)


def _cond_seq_forward(self, input):
    """nn.Sequential(SiLU, Linear).forward on ada_lin; a batch that cond_serves() declines (more than 64 rows; more than 16 rows into a large Linear) takes the class's
    own forward (and with it whatever is bound on the Linear)."""
    lin = self[1]
    if isinstance(input, torch.Tensor) and input.dim() >= 1 and input.shape[-1] > 0 and not cond_serves(input.numel() // input.shape[-1], lin.out_features, lin.in_features):
        return torch.nn.Sequential.forward(self, input)
    return ada_lin(input, lin.weight, lin.bias)


def _cond_served(m) -> bool:
    """Sequential(SiLU(inplace=False), Linear) with nn.Linear's own forward and sizes inside ada_lin's limits."""
    if not isinstance(m, torch.nn.Sequential) or len(m) != 2:
        return False
    act, lin = m[0], m[1]
    if type(act) is not torch.nn.SiLU or act.inplace or not isinstance(lin, torch.nn.Linear) or type(lin).forward is not torch.nn.Linear.forward:
        return False
    return E.cond_lin_shape_ok(1, lin.out_features, lin.in_features)


def _install_cond(who: str, model) -> None:
    if model is None:
        raise SdvarError(f"{who}: cond=True binds a forward on the model's own Sequential(SiLU, Linear) modules; pass the model (model=None has nothing to bind)")
    for m in model.modules():
        if _cond_served(m):
            m.forward = types.MethodType(_cond_seq_forward, m)


def install_cond(model) -> None:
    """Bind ada_lin on every nn.Sequential of `model` that is exactly (nn.SiLU(inplace=False), nn.Linear) with nn.Linear's own forward and sizes inside ada_lin's
    limits: the ada_lin of every block and of the head norm.  A Sequential around a Linear SUBCLASS with a forward of its own (the reference's shared_ada_lin, whose
    SharedAdaLin reshapes its result, var.py:16-19), an in-place SiLU or any other length is left alone.  The bound forward serves batches of at most 64 rows, and of
    more than 16 rows only into a Linear of at most 2^23 weights (cond_serves: beyond that the kernels, bound by plain fp32 arithmetic, lose to the GEMM path - d30's
    ada_lin at B = 32); any other batch goes through nn.Sequential.forward, the path it takes today (through linears=True's forward where that is installed).  A served weight never enters
    the weight-operand cache.  uninstall_cond(model) removes the bound forwards."""
    _install_cond("install_cond", model)


def uninstall_cond(model) -> None:
    """Delete the instance-level `forward` that install_cond / install_train(..., cond=True) / install_train_amp(..., cond=True) bound: nn.Sequential's own is back."""
    for m in model.modules():
        f = m.__dict__.get("forward")
        if getattr(f, "__func__", None) is _cond_seq_forward:
            del m.forward


# ------------------------------------------------------------------------------------------------------- the teacher-forcing input embedding (csrc/embed_train.hip)
def _embed_xv(xv, rows=None):
    """x_BLCv_wo_first_l as the kernels read it: of a half tensor the `rows` rows the call uses go through .float() (var.py:231 converts the slice, not the whole
    tensor), a float32 one is read in place under engine.embed_xv_in_place - the reference's slice of a longer tensor meets it - and copied once otherwise (all
    differentiable).  Anything else is left for the engine's checks to name."""
    if not isinstance(xv, torch.Tensor) or not xv.is_cuda or xv.dim() != 3:
        return xv
    if xv.dtype in _HALF_DTYPES:
        xv = (xv if rows is None or not 0 <= rows < xv.shape[1] else xv[:, :rows]).float()
    if xv.dtype == torch.float32 and not E.embed_xv_in_place(xv):
        xv = xv.clone(memory_format=torch.contiguous_format)
    return xv


def _embed_param(t):
    """A parameter or index vector as the kernels read it: itself when dense and 16-byte aligned, else one dense copy (differentiable)."""
    if isinstance(t, torch.Tensor) and t.is_cuda and (not t.is_contiguous() or t.data_ptr() % 16):
        return t.clone(memory_format=torch.contiguous_format)
    return t


class _EmbedGrad(torch.autograd.Function):
    """teacher_embed with a HIP backward (sdvar_op_embed_fwd / sdvar_op_embed_bwd).  Saved: label, r, xv and the word-embedding weight - nothing of x's size; the
    effective labels are recomputed in the backward with the forward's code.  lvl_1L, a buffer without gradient, is kept by reference."""

    @staticmethod
    def forward(ctx, label, xv, class_emb, pos_start, word_w, word_b, lvl_emb, pos_1LC, lvl_1L, tokens, r, rate, out_dtype):
        drop = None if r is None else (r, rate)
        x, cond = E.embed_fwd(label, xv, class_emb, pos_start, word_w, word_b, lvl_emb, pos_1LC, lvl_1L, tokens, drop, out_dtype, who="teacher_embed")
        ctx.set_materialize_grads(False)
        kept = [t for t in (label, r, xv, word_w) if t is not None]
        ctx.save_for_backward(*kept)
        ctx.emb = (r is not None, xv is not None, rate, tokens, lvl_1L, pos_start.shape[-2], class_emb.shape[0], lvl_emb.shape[0], out_dtype,
                   tuple(pos_start.shape), tuple(pos_1LC.shape))
        return x, cond

    @staticmethod
    def backward(ctx, g, gc):
        who = "teacher_embed"
        _no_double_backward(who)
        need = tuple(ctx.needs_input_grad[1:8])
        if not any(need) or (g is None and gc is None):
            return (None,) * 13
        has_r, has_xv, rate, tokens, lvl_1L, first_l, NC1, S, out_dtype, ps_shape, pos_shape = ctx.emb
        saved = list(ctx.saved_tensors)
        label = saved.pop(0)
        r = saved.pop(0) if has_r else None
        xv = saved.pop(0) if has_xv else None
        word_w = saved.pop(0)
        if g is not None:
            if g.dtype != out_dtype:
                raise SdvarError(f"{who}: the gradient of x_BLC is {g.dtype} but x_BLC is {out_dtype}; the backward reads it in the output's dtype")
            g = _dense16(g)          # a stride-0 expansion (out.sum().backward()) or a misaligned gradient: one fresh dense copy
        if gc is not None:
            if gc.dtype != torch.float32:
                raise SdvarError(f"{who}: the gradient of cond_BD is {gc.dtype} but cond_BD is float32")
            gc = _dense16(gc)
        dxv, dcls, dps, dw, db, dl, dpos = E.embed_bwd(g, gc, label, xv, word_w, lvl_1L, tokens, None if r is None else (r, rate), first_l, NC1, S, need, who=who)
        return (None, dxv, dcls, None if dps is None else dps.view(ps_shape), dw, db, dl, None if dpos is None else dpos.view(pos_shape), None, None, None, None, None)


def teacher_embed(label_B, x_BLCv_wo_first_l, class_emb, pos_start, word_w, word_b, lvl_emb, pos_1LC, lvl_1L, tokens=None, drop=None, out_dtype=torch.float32):
    """The prologue of a teacher-forced training step (VAR.forward, var.py:225-243: condition drop, class_emb gather, expand + pos_start, word_embed, cat, lvl_embed
    gather, + pos_1LC, the cast to the blocks' dtype) as ONE kernel forward - and one pass over the gradient plus a small launch per parameter group backward:
        j_b = r[b] < rate ? num_classes : label_B[b]      (drop = (r, rate); drop=None: label_B[b]);       cond_BD[b] = class_emb[j_b]
        x_BLC[b, l] = (class_emb[j_b] + pos_start[l]) + (lvl_emb[lvl_1L[l]] + pos_1LC[l])                   l <  first_l = pos_start.shape[-2]
        x_BLC[b, l] = (word_w x_BLCv_wo_first_l[b, l - first_l] + word_b) + (lvl_emb[lvl_1L[l]] + pos_1LC[l])    first_l <= l < tokens (None: L)
    -> (x_BLC (B, tokens, C) in out_dtype, cond_BD (B, C) float32).  label_B (B,) int64 or int32; x_BLCv_wo_first_l (B, >= tokens - first_l, K) float32 - a half tensor
    goes through .float() as in the reference - read in place (the reference's slice of a longer tensor included) when its rows are 16-byte aligned, else copied once;
    None allowed when tokens == first_l.  The parameters are the float32 master weights, dense: class_emb (num_classes + 1, C), pos_start (1, first_l, C), word_w (C, K),
    word_b (C,), lvl_emb (S, C), pos_1LC (1, L, C); lvl_1L (1, L) int64, the model's buffer.  r (B,) float32 is compared with float32(rate), as torch compares a
    float32 tensor with a Python number.  C % 4 == 0 in [4, 3072], K % 4 == 0 in [4, 64].
    Bits: the rows l < first_l and cond_BD carry the bits of torch's own float32 expression.  The word rows add the K products in the order k = 0 .. K - 1 with one fmaf
    each, where torch's GEMM picks its own order: THE numerical difference from the reference in float32.  out_dtype float16 / bfloat16 rounds the float32 value once:
    the bits of x_BLC.to(out_dtype), without a cast launch.  A row's bits do not depend on B.
    A label outside [0, num_classes] or a level outside [0, S) is never used as an index: the rows it would have fed are NaN and it adds nothing to the gradient of
    class_emb / lvl_emb (torch raises a device-side assert instead).
    Differentiable in both outputs: gradients of class_emb (rows no image selects are 0; repeated labels are added in image order), pos_start, word_w, word_b, lvl_emb
    (stages beyond `tokens` are 0), pos_1LC (rows beyond `tokens` are 0) and, where it requires grad, x_BLCv_wo_first_l - all float32 sums in a fixed order that depends
    on the shapes alone (include/sdvar_hip.h), no atomics, repeats bit-identical; only the gradients autograd asks for are computed, each with the bits it has in the
    full run; a missing upstream gradient costs nothing; a half upstream gradient is widened as it is read and nothing is clamped (an inf reaches the GradScaler).
    Saved for the backward: label_B, r, x_BLCv_wo_first_l and word_w - nothing of x_BLC's size.  There is no operand cache: an in-place update of a parameter is seen
    by the next call.  Under torch.no_grad(), or when nothing requires grad, the same forward kernel runs: the same bits.  Neither direction synchronises with the
    host.  CPU tensors, float64, half parameters, shapes that do not agree, C / K / tokens outside their limits raise SdvarError - there is no fall-back to torch.  No
    double backward."""
    who = "teacher_embed"
    if out_dtype not in E.TRAIN_DTYPES:
        raise SdvarError(f"{who}: out_dtype {out_dtype} is not float32, float16 or bfloat16")
    r = rate = None
    if drop is not None:
        if not isinstance(drop, (tuple, list)) or len(drop) != 2:
            raise SdvarError(f"{who}: drop must be None or (r, rate): the float32 (B,) uniform draws and the drop rate")
        r, rate = drop
        if isinstance(r, torch.Tensor):
            if r.requires_grad and torch.is_grad_enabled():
                raise SdvarError(f"{who}: drop's r requires grad; it carries no gradient (pass r.detach())")
            r = _embed_param(r.detach())
        rate = float(rate)
        drop = (r, rate)
    rows = None          # the rows of x_BLCv_wo_first_l this call reads, where the shapes say so (the engine names what is wrong with them otherwise)
    if isinstance(pos_start, torch.Tensor) and pos_start.dim() >= 2 and isinstance(lvl_1L, torch.Tensor) and lvl_1L.dim() >= 1:
        rows = (lvl_1L.shape[-1] if tokens is None else int(tokens)) - pos_start.shape[-2]
    xv = _embed_xv(x_BLCv_wo_first_l, rows)
    label_B, lvl_1L = _embed_param(label_B), _embed_param(lvl_1L)
    params = [_embed_param(t) for t in (class_emb, pos_start, word_w, word_b, lvl_emb, pos_1LC)]
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in [xv] + params):
        return _EmbedGrad.apply(label_B, xv, *params, lvl_1L, tokens, r, rate, out_dtype)
    d = lambda t: t.detach() if isinstance(t, torch.Tensor) else t
    return E.embed_fwd(d(label_B), d(xv), *(d(t) for t in params), d(lvl_1L), tokens, drop, out_dtype, who=who)


_EMBED_NEEDS = ("class_emb", "pos_start", "word_embed", "lvl_embed", "pos_1LC", "lvl_1L", "blocks", "get_logits", "begin_ends", "prog_si", "cond_drop_rate")


def _embed_var_forward(self, label_B, x_BLCv_wo_first_l):
    """VAR.forward (var.py:217-259) with teacher_embed in front of the blocks.  The uniform draws of the condition drop are taken once per call, at rate 0 too, so the
    generator moves as in the reference.  The blocks' dtype is the GPU's autocast dtype (float32 without autocast) - no matmul probe.  The residual stream leaves the
    kernel in float32 when blocks[0] carries adaln=True's bound forward (the seam keeps a float32 residual stream: adaln_modulate and gated_residual take and return
    float32), else in the blocks' dtype, as the reference casts it."""
    L = self.lvl_1L.shape[-1]
    ed = self.begin_ends[self.prog_si][1] if self.prog_si >= 0 else L
    B = x_BLCv_wo_first_l.shape[0]
    r = torch.rand(B, device=label_B.device)
    main_type = _autocast_gpu_dtype()
    if main_type not in _HALF_DTYPES:
        main_type = torch.float32
    fp32_stream = getattr(self.blocks[0].__dict__.get("forward"), "__func__", None) is _adaln_block_forward
    we = self.word_embed
    x_BLC, cond_BD = teacher_embed(label_B, x_BLCv_wo_first_l, self.class_emb.weight, self.pos_start, we.weight, we.bias, self.lvl_embed.weight, self.pos_1LC, self.lvl_1L,
                                   tokens=ed, drop=(r, self.cond_drop_rate), out_dtype=torch.float32 if fp32_stream else main_type)
    attn_bias = self.attn_bias_for_masking[:, :, :ed, :ed].to(dtype=main_type)
    cond_BD_or_gss = self.shared_ada_lin(cond_BD).to(dtype=main_type)
    for blk in self.blocks:
        x_BLC = blk(x=x_BLC, cond_BD=cond_BD_or_gss, attn_bias=attn_bias)
    # Stage 0 (prog_si == 0) has no word rows, and the reference keeps word_embed in the graph with two `* 0` terms on the logits (var.py:250-258; DDP needs every
    # parameter to receive a gradient).  Nothing of the kind is needed here: word_embed's weight and bias are operands of teacher_embed at every stage, and with
    # tokens == first_l its backward returns exact zeros for them, not None.
    return self.get_logits(x_BLC.float(), cond_BD)


def _install_embed(who: str, model) -> None:
    if model is None:
        raise SdvarError(f"{who}: embed=True binds a forward on the model itself; pass the model (model=None has nothing to bind)")
    hosts = [m for m in model.modules() if all(hasattr(m, n) for n in _EMBED_NEEDS)]
    if not hosts:
        missing = [n for n in _EMBED_NEEDS if not hasattr(model, n)]
        raise SdvarError(f"{who}: embed=True found no VAR-like module: {type(model).__name__} has no {' / '.join(missing)} (needed: {', '.join(_EMBED_NEEDS)})")
    for m in hosts:
        extra = [n for n in ("attn_bias_for_masking", "shared_ada_lin") if not hasattr(m, n)]
        we = m.word_embed
        if extra or not isinstance(getattr(we, "weight", None), torch.Tensor) or not isinstance(getattr(we, "bias", None), torch.Tensor):
            what = " / ".join(extra) if extra else "word_embed.weight / word_embed.bias (a Linear with a bias)"
            raise SdvarError(f"{who}: {type(m).__name__} has no {what}; embed=True knows VAR-like models only")
        m.forward = types.MethodType(_embed_var_forward, m)


def install_embed(model) -> None:
    """Bind an instance-level `forward(label_B, x_BLCv_wo_first_l)` on the module of `model` that has class_emb, pos_start, word_embed, lvl_embed, pos_1LC, lvl_1L,
    blocks, get_logits, begin_ends, prog_si and cond_drop_rate (the reference's VAR): var.py:217-259 with teacher_embed for everything in front of the blocks.
    word_embed's module forward is not called on this path, so with linears=True its weight never enters the weight-operand cache.  Under autocast the blocks are handed
    a float32 x_BLC when adaln=True's forward is bound on them - which is what lets install_train_amp(..., adaln=True) run the reference model: its own forward casts
    x_BLC to half, which adaln_modulate refuses - and the autocast dtype otherwise.  A model without one of the attributes raises.  uninstall_embed(model) removes it."""
    _install_embed("install_embed", model)


def uninstall_embed(model) -> None:
    """Delete the instance-level `forward` that install_embed / install_train(..., embed=True) / install_train_amp(..., embed=True) bound: the class's own is back."""
    for m in model.modules():
        f = m.__dict__.get("forward")
        if getattr(f, "__func__", None) is _embed_var_forward:
            del m.forward


# ------------------------------------------------------------------------------------------------------- attn_l2_norm's QK normalisation (csrc/qknorm_train.hip)
_QK_LAYOUTS = ("BHLc", "BLHc")


def _qk_views(layout: str, *ts):
    """The (B, L, H, 64) buffers as the layout's views: BLHc as they are, BHLc permuted (what the seam's attention reads in place)."""
    return tuple(t if layout == "BLHc" else t.permute(0, 2, 1, 3) for t in ts)


def _qk_grad(who: str, name: str, g, dtype, layout: str):
    """An upstream gradient in the layout's dim order -> a (B, L, H, 64) view, read in place under engine.qknorm_grad_in_place, else copied once."""
    if g is None:
        return None
    if g.dtype != dtype:
        raise SdvarError(f"{who}: the gradient of {name} is {g.dtype} but {name} is {dtype}")
    if layout == "BHLc":
        g = g.permute(0, 2, 1, 3)
    return g if E.qknorm_grad_in_place(g) else g.clone(memory_format=torch.contiguous_format)


class _QkNormGrad(torch.autograd.Function):
    """qk_l2norm with a HIP backward (sdvar_op_qknorm_fwd / sdvar_op_qknorm_bwd).  Saved: qkv, scale_log and the biases; the norms are recomputed in the backward with
    the forward's code.  Without a v_bias the returned v is a view of the input qkv."""

    @staticmethod
    def forward(ctx, qkv, scale_log, q_bias, v_bias, max_log, layout):
        q, k, v = E.qknorm_fwd(qkv, scale_log, max_log, q_bias, v_bias)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(qkv, scale_log, *(t for t in (q_bias,) if t is not None))
        ctx.qkn = (max_log, layout)
        if v is None:
            v = qkv[:, :, 2]
        return _qk_views(layout, q, k, v)

    @staticmethod
    def backward(ctx, dq, dk, dv):
        who = "qk_l2norm"
        _no_double_backward(who)
        nx, ns, nq, nv = ctx.needs_input_grad[:4]
        if not (nx or ns or nq or nv) or (dq is None and dk is None and dv is None):
            return (None,) * 6
        qkv, scale_log, *rest = ctx.saved_tensors
        max_log, layout = ctx.qkn
        dq, dk, dv = _qk_grad(who, "q", dq, torch.float32, layout), _qk_grad(who, "k", dk, torch.float32, layout), _qk_grad(who, "v", dv, qkv.dtype, layout)
        dqkv, ds, dqb, dvb = E.qknorm_bwd(qkv, scale_log, max_log, rest[0] if rest else None, dq, dk, dv, (nx, ns, nq, nv))
        return dqkv, ds, dqb, dvb, None, None


def qk_l2norm(qkv, scale_log, max_log: float, q_bias=None, v_bias=None, layout: str = "BHLc"):
    """What SelfAttention.forward does between the QKV GEMM and the attention call when attn_l2_norm is on (basic_var.py:93-105), as one kernel per direction:
        xq = qkv[:, :, 0] + q_bias;  q = xq / max(|xq|, 1e-12) * exp(min(scale_log[h], max_log));  k = xk / max(|xk|, 1e-12), xk = qkv[:, :, 1];  v = qkv[:, :, 2] + v_bias
    with the norms over each head's 64 channels.  qkv (B, L, 3, H, 64) float32, float16 or bfloat16 on the GPU (the bias-free QKV GEMM's output, viewed), 1 <= H <= 48;
    a dense, 16-byte aligned qkv is read in place, anything else is copied once.  scale_log (H) float32: the raw parameter (`scale_mul_1H11.view(H)`); max_log: its
    clamp (`max_scale_mul`).  q_bias / v_bias (64 H) float32 or None.  Every operation is float32 on the widened values.  Returns (q, k, v): q and k float32, v in
    qkv's dtype, as views of dense (B, L, H, 64) buffers - layout "BHLc": (B, H, L, 64), what slow_attn reads in place; "BLHc": (B, L, H, 64), what flash_attn_func and
    memory_efficient_attention read.  Without a v_bias, v is the view of qkv the reference would have produced: nothing is written or copied.  A head with a norm
    below 1e-12 gives x / 1e-12 (a zero head: exact zeros).
    THE numerical difference from the reference: under autocast the reference's F.linear rounds acc + half(bias) to half once, inside the GEMM.  Here the float32
    master bias is added in float32 to the half GEMM output; for q that sum is never rounded back to half, for v it is rounded once.
    Differentiable: dqkv in qkv's dtype with all three slots written by one kernel (an fp16 overflow is +-inf and reaches the GradScaler; nothing is clamped),
    dscale_log (zero for a head above max_log, passed at equality, as clamp_max does), dq_bias and dv_bias in float32, summed in a fixed order without atomics: repeats
    are bit-identical; only the gradients autograd asks for are computed.  Upstream gradients of q and k must be float32 and that of v in qkv's dtype; they are read
    through their strides (the permuted views the seam's attention backward returns) when the last stride is 1 and the others are multiples of 4, else copied once.
    Saved for the backward: qkv, scale_log, q_bias.  Under torch.no_grad(), or when nothing requires grad, the same forward kernel runs: the same bits.  Neither
    direction synchronises with the host.  No double backward."""
    who = "qk_l2norm"
    if layout not in _QK_LAYOUTS:
        raise SdvarError(f"{who}: layout {layout!r}; expected 'BHLc' or 'BLHc'")
    if isinstance(qkv, torch.Tensor) and qkv.is_cuda and qkv.dim() == 5 and qkv.dtype in E.TRAIN_DTYPES and (not qkv.is_contiguous() or qkv.data_ptr() % 16):
        qkv = qkv.clone(memory_format=torch.contiguous_format)
    vecs = [t if not isinstance(t, torch.Tensor) or (t.is_contiguous() and t.data_ptr() % 16 == 0) else t.clone(memory_format=torch.contiguous_format)
            for t in (scale_log, q_bias, v_bias)]
    scale_log, q_bias, v_bias = vecs
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (qkv, scale_log, q_bias, v_bias)):
        E._qknorm_qkv(who, qkv)          # argument errors before autograd wraps them
        return _QkNormGrad.apply(qkv, scale_log, q_bias, v_bias, float(max_log), layout)
    d = lambda t: t.detach() if isinstance(t, torch.Tensor) else t
    q, k, v = E.qknorm_fwd(d(qkv), d(scale_log), float(max_log), d(q_bias), d(v_bias))
    return _qk_views(layout, q, k, d(qkv)[:, :, 2] if v is None else v)


def _qknorm_attn_forward(self, x, attn_bias):
    """SelfAttention.forward (basic_var.py:90-119) with qk_l2norm between the QKV GEMM and the attention call.  mat_qkv is called as a module without a bias (the
    biases go into the kernel); the attention slots and the route choice are read from the class forward's own globals at call time, as the reference reads them."""
    B, L, Cc = x.shape
    H = self.num_heads
    ns = type(self).forward.__globals__
    qkv = self.mat_qkv(x)
    main_type = qkv.dtype
    using_flash = self.using_flash and attn_bias is None and main_type != torch.float32
    blhc = using_flash or self.using_xform
    q, k, v = qk_l2norm(qkv.view(B, L, 3, H, Cc // H), self.scale_mul_1H11.view(H), self.max_scale_mul, self.q_bias, self.v_bias, "BLHc" if blhc else "BHLc")
    dim_cat = 1 if blhc else 2
    if self.caching:
        if self.cached_k is None:
            self.cached_k, self.cached_v = k, v
        else:
            k = self.cached_k = torch.cat((self.cached_k, k), dim=dim_cat)
            v = self.cached_v = torch.cat((self.cached_v, v), dim=dim_cat)
    dropout_p = self.attn_drop if self.training else 0.0
    if using_flash:
        oup = ns["flash_attn_func"](q.to(dtype=main_type), k.to(dtype=main_type), v.to(dtype=main_type), dropout_p=dropout_p, softmax_scale=self.scale).view(B, L, Cc)
    elif self.using_xform:
        bias = None if attn_bias is None else attn_bias.to(dtype=main_type).expand(B, H, -1, -1)
        oup = ns["memory_efficient_attention"](q.to(dtype=main_type), k.to(dtype=main_type), v.to(dtype=main_type), attn_bias=bias, p=dropout_p,
                                               scale=self.scale).view(B, L, Cc)
    else:
        oup = ns["slow_attn"](query=q, key=k, value=v, scale=self.scale, attn_mask=attn_bias, dropout_p=dropout_p).transpose(1, 2).reshape(B, L, Cc)
    return self.proj_drop(self.proj(oup))


_QKNORM_NEEDS = ("q_bias", "v_bias", "scale_mul_1H11", "proj")


def _install_qknorm(who: str, model) -> None:
    if model is None:
        raise SdvarError(f"{who}: qknorm=True binds a forward on the model's own attention modules; pass the model (model=None has nothing to bind)")
    for m in model.modules():
        if not hasattr(m, "mat_qkv") or not getattr(m, "attn_l2_norm", False):
            continue
        missing = [n for n in _QKNORM_NEEDS if not hasattr(m, n)]
        if missing:
            raise SdvarError(f"{who}: {type(m).__name__} has mat_qkv and attn_l2_norm=True but no {' / '.join(missing)}; qknorm knows SelfAttention-like modules only")
        m.forward = types.MethodType(_qknorm_attn_forward, m)


def install_qknorm(model) -> None:
    """Bind the qk_l2norm forward on every attention module of `model` that has attn_l2_norm=True (modules without it are left alone), for inference or on top of any
    of the install_* calls; the attention slots keep working as they are installed.  A module that has mat_qkv but no q_bias / v_bias / scale_mul_1H11 / proj raises."""
    _install_qknorm("install_qknorm", model)


def uninstall_qknorm(model) -> None:
    """Delete the instance-level `forward` that install_qknorm / install_train(..., qknorm=True) / install_train_amp(..., qknorm=True) bound: the class's own forward is
    back."""
    for m in model.modules():
        f = m.__dict__.get("forward")
        if getattr(f, "__func__", None) is _qknorm_attn_forward:
            del m.forward
