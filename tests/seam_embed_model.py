"""A small VAR-shaped stand-in for tests/test_gpu_seam_embed.py and tests/test_seam_embed_host.py.  Written for these tests: it has the attributes seam.install_embed
looks for (class_emb, pos_start, word_embed, lvl_embed, pos_1LC, lvl_1L, blocks, get_logits, begin_ends, prog_si, cond_drop_rate, plus attn_bias_for_masking and
shared_ada_lin = nn.Identity()), one block and the head norm of tests/seam_cond_model.py, and a forward of its own that - like the model it stands in for - hands the
blocks a stream in the autocast dtype.  The `module` argument of the installers is tests/seam_linear_model.py (SM)."""
from __future__ import annotations

import torch
import torch.nn as nn

import seam_cond_model as CM
import seam_linear_model as SM

PNS, C, H, K, V, NUM_CLASSES, B = (2, 3, 4), 128, 2, 32, 64, 5, 3          # first_l = 4: at prog_si 0 the tokens still attend to one another


def _autocast_dtype(device_type: str):
    if hasattr(torch, "get_autocast_dtype"):
        return torch.get_autocast_dtype(device_type) if torch.is_autocast_enabled(device_type) else None
    if device_type == "cuda":
        return torch.get_autocast_gpu_dtype() if torch.is_autocast_enabled() else None
    return torch.get_autocast_cpu_dtype() if torch.is_autocast_cpu_enabled() else None


class Model(nn.Module):
    def __init__(self, pns=PNS, width=C, heads=H, cvae=K, vocab=V, num_classes=NUM_CLASSES):
        super().__init__()
        sizes = [p * p for p in pns]
        self.first_l, self.L, self.C, self.Cvae, self.num_classes = sizes[0], sum(sizes), width, cvae, num_classes
        self.begin_ends, at = [], 0
        for n in sizes:
            self.begin_ends.append((at, at + n)); at += n
        self.prog_si, self.cond_drop_rate = -1, 0.3
        self.class_emb = nn.Embedding(num_classes + 1, width)
        self.pos_start = nn.Parameter(0.5 * torch.randn(1, self.first_l, width))
        self.word_embed = nn.Linear(cvae, width)
        self.lvl_embed = nn.Embedding(len(pns), width)
        self.pos_1LC = nn.Parameter(0.5 * torch.randn(1, self.L, width))
        stage = torch.cat([torch.full((n,), i) for i, n in enumerate(sizes)])
        self.register_buffer("lvl_1L", stage.view(1, self.L).long())
        self.register_buffer("attn_bias_for_masking", torch.where(stage.view(-1, 1) >= stage.view(1, -1), 0.0, -torch.inf).view(1, 1, self.L, self.L))
        self.shared_ada_lin = nn.Identity()
        self.blocks = nn.ModuleList([CM.Block(width, heads, width)])
        self.head_nm = CM.HeadNorm(width, width)
        self.head = nn.Linear(width, vocab)

    def get_logits(self, h, cond_BD):
        wide = self.head.weight.dtype
        return self.head(self.head_nm(h.to(wide), cond_BD).to(wide)).to(wide)

    def forward(self, label_B, feats_wo_first):
        """Labels, some replaced by the extra "no class" row; one start row per image; the embedded features of the later tokens; stage and position added; the block
        under the block-causal mask; logits for the first `ed` tokens."""
        wide, kind = self.head.weight.dtype, label_B.device.type          # float32 master weights; float64 in the reference run of the tests
        ed = self.L if self.prog_si < 0 else self.begin_ends[self.prog_si][1]
        n_img = feats_wo_first.shape[0]
        with torch.autocast(kind, enabled=False):
            dropped = torch.rand(n_img, device=label_B.device) < self.cond_drop_rate
            cond = self.class_emb(torch.where(dropped, self.num_classes, label_B))
            rows = cond[:, None, :] + self.pos_start
            if ed > self.first_l:
                rows = torch.cat((rows, self.word_embed(feats_wo_first[:, :ed - self.first_l].to(wide))), dim=1)
            rows = rows + (self.lvl_embed(self.lvl_1L[0, :ed])[None] + self.pos_1LC[:, :ed])
        stream = _autocast_dtype(kind) or wide
        x, c_in, mask = rows.to(stream), self.shared_ada_lin(cond).to(stream), self.attn_bias_for_masking[:, :, :ed, :ed].to(stream)
        for blk in self.blocks:
            x = blk(x=x, cond_BD=c_in, attn_bias=mask)
        out = self.get_logits(x.to(wide), cond)
        if ed == self.first_l:          # the word embedding took no part: keep it in the graph with a zero gradient
            out = out + 0 * (self.word_embed.weight.sum() + self.word_embed.bias.sum())
        return out


def model_and_inputs():
    """(model, label (B,), feats (B, L - first_l, K), w (B, L, V)) on the CPU in float32 from a fixed seed; w weighs the logits in the loss."""
    g = torch.Generator().manual_seed(7741)
    torch.manual_seed(7741)
    m = Model()
    label = torch.tensor([4, 0, 4])
    feats, w = torch.randn(B, m.L - m.first_l, K, generator=g), torch.randn(B, m.L, V, generator=g)
    return m, label, feats, w


def loss_and_grads(m, label, feats, w, autocast=None, scale=1.0):
    """The loss (mean of w * logits over the tokens the model returns, times `scale`) and the gradient of every parameter that took part."""
    m.zero_grad(set_to_none=True)
    with torch.autocast(label.device.type, dtype=autocast or torch.bfloat16, enabled=autocast is not None):
        out = m(label, feats)
    loss = (out.to(w.dtype) * w[:, :out.shape[1]]).mean() * scale
    loss.backward()
    res = {"loss": loss.detach().clone()}
    res.update({n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None})
    return res
