"""A stand-in for one trained VAR step, for tests/test_gpu_seam_linear.py and tests/test_seam_linear_host.py: a block with every dense linear a VAR block has
(ada_lin = Sequential(SiLU, Linear), mat_qkv, proj, fc1, fc2), a `word_embed` called inside autocast(enabled=False) on a float32 input and a `head` called under
autocast on a .float()-ed input - the two call sites that decide which path seam's bound nn.Linear.forward takes.  Written for these tests; the attribute names are the
ones seam's installers look for (ln_wo_grad, attn, ffn, ada_lin, mat_qkv, attn_l2_norm, q_bias, v_bias, scale_mul_1H11, proj, fused_mlp_func, using_flash).

This module is also the `module` argument of the installers: its globals slow_attn / flash_attn_func / memory_efficient_attention / fused_mlp_func are the operator
slots, read at call time."""
from __future__ import annotations

import math
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

C, H, B, L, CVAE, V = 128, 2, 2, 21, 32, 64
MAX_LOG = math.log(100.0)


def _torch_attn(query, key, value, scale, attn_mask=None, dropout_p=0.0):
    return F.scaled_dot_product_attention(query, key, value, attn_mask=attn_mask, dropout_p=dropout_p, scale=scale)


slow_attn = _torch_attn
flash_attn_func = memory_efficient_attention = fused_mlp_func = None
_SLOTS = ("slow_attn", "flash_attn_func", "memory_efficient_attention", "fused_mlp_func")


def save_slots():
    me = sys.modules[__name__]
    return {n: getattr(me, n) for n in _SLOTS}


def restore_slots(saved) -> None:
    me = sys.modules[__name__]
    for n, v in saved.items():
        setattr(me, n, v)


class SelfAttn(nn.Module):
    def __init__(self, Cc, heads):
        super().__init__()
        self.num_heads, self.head_dim, self.attn_l2_norm, self.scale = heads, Cc // heads, True, 1
        self.scale_mul_1H11 = nn.Parameter(torch.full((1, heads, 1, 1), 4.0).log() + 0.25 * torch.randn(1, heads, 1, 1))
        self.max_scale_mul = MAX_LOG
        self.mat_qkv = nn.Linear(Cc, 3 * Cc, bias=False)
        self.q_bias, self.v_bias = nn.Parameter(0.5 * torch.randn(Cc)), nn.Parameter(0.5 * torch.randn(Cc))
        self.register_buffer("zero_k_bias", torch.zeros(Cc))
        self.proj, self.proj_drop, self.attn_drop = nn.Linear(Cc, Cc), nn.Identity(), 0.0
        self.using_flash = self.using_xform = False
        self.caching, self.cached_k, self.cached_v = False, None, None

    def forward(self, x, attn_bias):
        """Bias-free QKV product plus the q / v biases, unit-length q and k per head, q times its clamped learnt scale, masked attention, output projection."""
        n_img, n_tok, width = x.shape
        heads, hd = self.num_heads, self.head_dim
        qkv = F.linear(x, self.mat_qkv.weight)
        q, k, v = (t.reshape(n_img, n_tok, heads, hd).transpose(1, 2) for t in qkv.split(width, dim=-1))          # each (B, H, L, hd)
        q = q + self.q_bias.view(1, heads, 1, hd).to(q.dtype)
        v = v + self.v_bias.view(1, heads, 1, hd).to(v.dtype)
        gain = torch.exp(torch.clamp(self.scale_mul_1H11, max=self.max_scale_mul))
        q = gain * q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        k = k / k.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        mixed = slow_attn(query=q, key=k, value=v, scale=self.scale, attn_mask=attn_bias, dropout_p=0.0)
        return self.proj_drop(self.proj(mixed.transpose(1, 2).reshape(n_img, n_tok, width)))


class FFN(nn.Module):
    def __init__(self, Cc):
        super().__init__()
        self.fused_mlp_func = None
        self.fc1, self.act, self.fc2 = nn.Linear(Cc, 4 * Cc), nn.GELU(approximate="tanh"), nn.Linear(4 * Cc, Cc)

    def forward(self, x):
        if self.fused_mlp_func is not None:
            return self.fused_mlp_func(x=x, weight1=self.fc1.weight, weight2=self.fc2.weight, bias1=self.fc1.bias, bias2=self.fc2.bias, activation="gelu_approx",
                                       save_pre_act=self.training, return_residual=False, checkpoint_lvl=0, heuristic=0, process_group=None)
        return self.fc2(self.act(self.fc1(x)))


class Block(nn.Module):
    def __init__(self, Cc, heads):
        super().__init__()
        self.C, self.drop_path = Cc, nn.Identity()
        self.attn, self.ffn, self.ln_wo_grad = SelfAttn(Cc, heads), FFN(Cc), nn.LayerNorm(Cc, eps=1e-6, elementwise_affine=False)
        self.ada_lin = nn.Sequential(nn.SiLU(inplace=False), nn.Linear(Cc, 6 * Cc))

    def forward(self, x, cond_BD, attn_bias):
        """Two gated residual branches, each behind a LayerNorm modulated by its own rows of ada_lin's output (rows: gate 1, gate 2, scale 1, scale 2, shift 1, shift 2)."""
        rows = self.ada_lin(cond_BD).reshape(cond_BD.shape[0], 6, 1, self.C)
        gate_a, gate_f, scale_a, scale_f, shift_a, shift_f = (rows[:, i] for i in range(6))
        x = x + gate_a * self.attn(self.ln_wo_grad(x) * (1 + scale_a) + shift_a, attn_bias=attn_bias)
        return x + gate_f * self.ffn(self.ln_wo_grad(x) * (1 + scale_f) + shift_f)


class Model(nn.Module):
    """tokens' features (B, L, CVAE) -> word_embed (float32, autocast off) -> one block -> head (under autocast, on a .float()-ed input) -> float32 logits (B, L, V)."""

    def __init__(self, Cc=C, heads=H, cvae=CVAE, vocab=V):
        super().__init__()
        self.word_embed = nn.Linear(cvae, Cc)
        self.block = Block(Cc, heads)
        self.head = nn.Linear(Cc, vocab)
        self.odd = nn.Linear(Cc, 10)            # out_features % 32 != 0: never bound, never called

    def forward(self, feats, cond, attn_bias=None):
        wide = self.head.weight.dtype           # float32 master weights: the reference's .float(); float64 in the reference run of the tests
        with torch.autocast(feats.device.type, enabled=False):
            x = self.word_embed(feats.to(wide))
        x = self.block(x, cond, attn_bias)
        return self.head(x.to(wide)).to(wide)


def model_and_inputs():
    """(model, feats, cond, w, mask) on the CPU in float32, from a fixed seed; w weighs the logits in the loss; the mask is block-causal over stages of 1, 4 and 16."""
    g = torch.Generator().manual_seed(9173)
    torch.manual_seed(9173)
    m = Model()
    feats, cond, w = (torch.randn(s, generator=g) for s in ((B, L, CVAE), (B, C), (B, L, V)))
    stage = torch.tensor([0] + [1] * 4 + [2] * 16)
    mask = torch.where(stage.view(L, 1) >= stage.view(1, L), 0.0, -torch.inf).view(1, 1, L, L)
    return m, feats, cond, w, mask


def loss_and_grads(m, feats, cond, w, mask, autocast=None, scale=1.0):
    """The loss (mean of w * logits, times `scale`) and the gradient of every parameter that took part."""
    m.zero_grad(set_to_none=True)
    with torch.autocast(feats.device.type, dtype=autocast or torch.bfloat16, enabled=autocast is not None):
        out = m(feats, cond, mask)
    loss = (out.to(w.dtype) * w).mean() * scale
    loss.backward()
    res = {"loss": loss.detach().clone()}
    res.update({n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None})
    return res
