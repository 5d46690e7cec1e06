#!/usr/bin/env python3
"""Generate tests/golden/tf_*.npz by running the REFERENCE teacher-forced VAR.forward (models/var.py:217-259, imported from the reference, CPU).

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_tf_golden.py
The reference never travels to the GPU box; only the .npz outputs (data) are committed.  The model is built by the reference's own
build_vae_var, loaded with sdvar_amd.weights.var_state_dict (strict=True), put in eval mode with cond_drop_rate = 0.  Its inputs are the
reference-made ground-truth ids and idxBl_to_var_input of tests/golden/encode_256.npz / encode_512.npz, so the chain image -> ids -> input
-> logits is entirely the reference's.

Recorded per case and token: lse, argmax, the top-2 margin, the nll of the ground-truth id, the 8 largest logits and 8 fixed random
columns (with their indices), two full logits rows, and the eval_ep statistics (trainer.py:66-75) computed with the reference trainer's
nn.CrossEntropyLoss: L_mean, L_tail, acc_mean, acc_tail of the batch.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")

import models as ref_models                      # noqa: E402  (the reference)
from sdvar_amd.ladder import LADDER_256, LADDER_512   # noqa: E402
from sdvar_amd.weights import var_state_dict     # noqa: E402

torch.set_grad_enabled(False)
torch.set_num_threads(8)
WSEED = 1234
N_RAND = 8
# (name, encode fixture, depth, labels, shared_aln, attn_l2_norm)
CASES = (("tf_d4_256_stress", "encode_256", 4, (3, 977), False, True),
         ("tf_d4_256_uncond", "encode_256", 4, (1000, 1000), False, True),
         ("tf_d4_512_stress", "encode_512", 4, (207,), False, True),
         ("tf_d4_256_sharedaln", "encode_256", 4, (3, 977), True, True),
         ("tf_d4_256_nol2", "encode_256", 4, (3, 977), False, False))


def eval_stats(logits, gt, last_l):
    """trainer.py:66-75 for one batch, divided by B (tot = B)."""
    B, L, V = logits.shape
    val_loss = torch.nn.CrossEntropyLoss(label_smoothing=0.0, reduction="mean")
    L_mean = val_loss(logits.view(-1, V), gt.view(-1)) * B
    L_tail = val_loss(logits[:, -last_l:].reshape(-1, V), gt[:, -last_l:].reshape(-1)) * B
    acc_mean = (logits.argmax(dim=-1) == gt).sum() * (100 / gt.shape[1])
    acc_tail = (logits[:, -last_l:].argmax(dim=-1) == gt[:, -last_l:]).sum() * (100 / last_l)
    return [float(v) / B for v in (L_mean, L_tail, acc_mean, acc_tail)]


def build_case(name, enc, depth, labels, shared_aln, l2):
    e = np.load(os.path.join(OUT, enc + ".npz"))
    pns = tuple(int(p) for p in e["patch_nums"])
    assert pns in (LADDER_256, LADDER_512)
    _, var = ref_models.build_vae_var(device="cpu", patch_nums=pns, depth=depth, shared_aln=shared_aln, attn_l2_norm=l2)
    var.load_state_dict(var_state_dict(depth, pns, "stress", WSEED, shared_aln=shared_aln, attn_l2_norm=l2), strict=True)
    var.eval()
    var.cond_drop_rate = 0.0
    B = len(labels)
    gt = torch.from_numpy(e["ids"][:B]).long()
    xv = torch.from_numpy(e["var_input"][:B]).float()
    lab = torch.tensor(labels, dtype=torch.int64)
    t0 = time.time()
    logits = var(lab, xv).float()
    dt = time.time() - t0
    L, V = logits.shape[1], logits.shape[2]
    last_l = pns[-1] ** 2
    lg = logits.double()
    lse = torch.logsumexp(lg, -1)
    top = lg.topk(N_RAND, dim=-1)
    nll = lse - lg.gather(-1, gt.unsqueeze(-1)).squeeze(-1)
    g = np.random.Generator(np.random.Philox(key=[WSEED, 99]))
    rcols = torch.from_numpy(g.integers(0, V, size=(B, L, N_RAND))).long()
    rows_bt = np.array([[0, L - 1], [B - 1, L // 2]], dtype=np.int64)
    out = dict(patch_nums=np.array(pns), depth=np.array(depth), wseed=np.array(WSEED), labels=np.array(labels, dtype=np.int64),
               shared_aln=np.array(int(shared_aln)), attn_l2_norm=np.array(int(l2)), encode=np.array(enc),
               lse=lse.float().numpy(), argmax=logits.argmax(-1).numpy().astype(np.int16), margin=(top.values[..., 0] - top.values[..., 1]).float().numpy(),
               nll=nll.float().numpy(), top_idx=top.indices.numpy().astype(np.int16), top_val=top.values.float().numpy(),
               rand_idx=rcols.numpy().astype(np.int16), rand_val=logits.gather(-1, rcols).numpy(),
               rows_bt=rows_bt, rows=np.stack([logits[b, t].numpy() for b, t in rows_bt]),
               stats=np.array(eval_stats(logits, gt, last_l)))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    sz = os.path.getsize(path)
    assert sz < 1 << 20, f"{name}: {sz} bytes"
    print(f"[tf golden] {name}: reference forward {dt:.2f}s, |logit| max {logits.abs().max():.2f}, min margin {out['margin'].min():.2e}, "
          f"stats {out['stats'].round(4).tolist()}, {sz} bytes")


def main():
    for c in CASES:
        build_case(*c)


if __name__ == "__main__":
    main()
