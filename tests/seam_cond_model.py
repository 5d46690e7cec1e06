"""A stand-in for the conditioning path of one trained VAR step, for tests/test_gpu_seam_cond.py and tests/test_seam_cond_host.py.  Written for these tests: a block
whose `ada_lin` = Sequential(SiLU, Linear(D, 6C)) feeds two modulated, gated branches; a head norm whose `ada_lin` = Sequential(SiLU, Linear(D, 2C)) is fed the float32
condition also under autocast; and the two Sequentials seam.install_cond must leave alone - one around an nn.Linear SUBCLASS whose forward reshapes its result, one with
an in-place SiLU.  The attention and FFN modules and the operator slots are those of tests/seam_linear_model.py (SM), which is also the `module` argument of the
installers; the attribute names are the ones seam's installers look for (ln_wo_grad, attn, ffn, ada_lin, drop_path)."""
from __future__ import annotations

import torch
import torch.nn as nn

import seam_linear_model as SM

C, H, B, L, D, V, G = 128, 2, 8, 21, 128, 64, 24


class Block(nn.Module):
    def __init__(self, width, heads, cond_dim):
        super().__init__()
        self.C, self.drop_path = width, nn.Identity()
        self.attn, self.ffn, self.ln_wo_grad = SM.SelfAttn(width, heads), SM.FFN(width), nn.LayerNorm(width, eps=1e-6, elementwise_affine=False)
        self.ada_lin = nn.Sequential(nn.SiLU(inplace=False), nn.Linear(cond_dim, 6 * width))

    def forward(self, x, cond_BD, attn_bias):
        """Six rows of conditioning per image: two gates, two scales, two shifts; each branch sees a modulated LayerNorm and re-enters through its gate."""
        gate_a, gate_f, scale_a, scale_f, shift_a, shift_f = self.ada_lin(cond_BD).view(-1, 1, 6, self.C).unbind(2)
        x = x + self.attn(self.ln_wo_grad(x) * (scale_a + 1) + shift_a, attn_bias=attn_bias) * gate_a
        return x + self.ffn(self.ln_wo_grad(x) * (scale_f + 1) + shift_f) * gate_f


class HeadNorm(nn.Module):
    def __init__(self, width, cond_dim):
        super().__init__()
        self.C, self.ln_wo_grad = width, nn.LayerNorm(width, eps=1e-6, elementwise_affine=False)
        self.ada_lin = nn.Sequential(nn.SiLU(inplace=False), nn.Linear(cond_dim, 2 * width))

    def forward(self, x, cond_BD):
        scale, shift = self.ada_lin(cond_BD).view(-1, 1, 2, self.C).unbind(2)
        return self.ln_wo_grad(x) * (scale + 1) + shift


class PairedLinear(nn.Linear):
    """An nn.Linear with a forward of its own: the result leaves as (B, 1, 2, out / 2)."""

    def forward(self, c):
        return super().forward(c).view(-1, 1, 2, self.out_features // 2)


class Model(nn.Module):
    """x0 (B, L, C) and cond (B, D) -> block -> two small conditioning terms (the Sequentials that stay with torch) -> head norm -> head -> float32 logits (B, L, V)."""

    def __init__(self, width=C, heads=H, cond_dim=D, vocab=V, pair=G):
        super().__init__()
        self.block = Block(width, heads, cond_dim)
        self.head_nm = HeadNorm(width, cond_dim)
        self.head = nn.Linear(width, vocab)
        self.paired = nn.Sequential(nn.SiLU(inplace=False), PairedLinear(cond_dim, 2 * pair))          # sizes inside ada_lin's limits: excluded by its class alone
        self.inplace = nn.Sequential(nn.SiLU(inplace=True), nn.Linear(cond_dim, width))

    def forward(self, x0, cond, attn_bias=None):
        wide = self.head.weight.dtype               # float32 master weights; float64 in the reference run of the tests
        x = self.block(x0.to(wide), cond, attn_bias)
        lift, tilt = self.paired(cond).unbind(2)    # (B, 1, G) each
        x = x * (1 + 0.05 * lift.to(wide).mean(-1, keepdim=True)) + 0.05 * tilt.to(wide).mean(-1, keepdim=True)
        x = x + 0.05 * self.inplace(cond.clone()).to(wide).unsqueeze(1)
        return self.head(self.head_nm(x.to(wide), cond.to(wide)).to(wide)).to(wide)


def model_and_inputs():
    """(model, x0, cond, w, mask) on the CPU in float32, from a fixed seed; w weighs the logits in the loss; the mask is SM's block-causal one (stages of 1, 4, 16)."""
    g = torch.Generator().manual_seed(5521)
    torch.manual_seed(5521)
    m = Model()
    x0, cond, w = (torch.randn(s, generator=g) for s in ((B, L, C), (B, D), (B, L, V)))
    stage = torch.tensor([0] + [1] * 4 + [2] * 16)
    mask = torch.where(stage.view(L, 1) >= stage.view(1, L), 0.0, -torch.inf).view(1, 1, L, L)
    return m, x0, cond, w, mask


loss_and_grads = SM.loss_and_grads
