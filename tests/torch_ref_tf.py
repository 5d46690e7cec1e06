"""PyTorch-CPU restatement of the teacher-forced VAR.forward (reference models/var.py:217-259) on top of oracle.var_oracle.OracleVAR:
the embedding is built here, the blocks and head are OracleVAR.forward over all S stages under the block-causal mask.  Pinned against the
reference fixtures of tests/golden/make_tf_golden.py by tests/test_var_forward_host.py; the full-width GPU test compares against it."""
import torch

from oracle import var_oracle as orc


def tf_input(model: "orc.OracleVAR", labels: torch.Tensor, xv: torch.Tensor):
    """(x (B, L, C), cond (B, C)): token 0 = (class_emb[label] + pos_start) + lvl_pos[0], token t = word_embed(xv[:, t-1]) + lvl_pos[t]."""
    sd = model.sd
    cond = sd["class_emb.weight"][labels]
    lvl_1L = torch.cat([torch.full((n,), i, dtype=torch.int64) for i, n in enumerate(model.lens)])
    lvl_pos = sd["lvl_embed.weight"][lvl_1L] + sd["pos_1LC"][0]
    sos = (cond + sd["pos_start"][0, 0]).unsqueeze(1)
    words = torch.nn.functional.linear(xv.float(), sd["word_embed.weight"], sd["word_embed.bias"])
    return torch.cat((sos, words), 1) + lvl_pos.unsqueeze(0), cond


@torch.no_grad()
def tf_logits(model: "orc.OracleVAR", labels: torch.Tensor, xv: torch.Tensor) -> torch.Tensor:
    x, cond = tf_input(model, labels, xv)
    model.kv_reset()
    out = model.forward(x, cond, 0, model.S)
    model.kv_reset()
    return out
