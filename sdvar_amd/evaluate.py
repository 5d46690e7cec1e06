"""Validation loss and accuracy of a VAR checkpoint on real images: VARTrainer.eval_ep (reference trainer.py:55-84) on the HIP path.

Per batch: image -> VQVAE.img_to_idxBl (ground-truth ids) -> VectorQuantizer2.idxBl_to_var_input -> VAR.forward (teacher-forced logits)
-> sdvar_xent_stats, which adds {sum nll, sum tail nll, #correct, #tail correct} to four float64 sums kept on the device across batches.
After the last batch the sums and the image count are all-reduced over the ranks (sdvar_amd.dist; RCCL on the GPU, gloo in tests) and
divided as the reference divides them.  `var.cond_drop_rate = 0` makes the numbers deterministic: VAR.forward applies the reference's
condition dropout in eval mode too.

`eval_vae` is the tokenizer's counterpart: reconstruction error, VQ loss and codebook usage of a VQVAE checkpoint over the same kind of loader.
"""
from __future__ import annotations

import time
from typing import Iterable, List, Tuple

import numpy as np
import torch

from . import dist as D
from . import engine as E


@torch.no_grad()
def eval_ep(var, vae, ld_val: Iterable) -> Tuple[float, float, float, float, int, float]:
    """-> (L_mean, L_tail, acc_mean, acc_tail, tot, seconds) over the (inp_B3HW in [-1, 1], label_B) batches of `ld_val`, as VARTrainer.eval_ep:
    L_mean = mean cross-entropy over all B*L tokens, L_tail over the last patch_nums[-1]^2 tokens of each image, acc_* = percentage of tokens whose
    argmax (lowest index on ties) equals the target; tot = images over all ranks.  The model is put in eval mode for the pass and restored."""
    stt = time.time()
    dev = var._device()
    L, last_l = var.L, var.patch_nums[-1] ** 2
    sums = torch.zeros(4, dtype=torch.float64, device=dev)
    tot = 0
    training = var.training
    var.eval()
    try:
        for inp_B3HW, label_B in ld_val:
            B = int(label_B.shape[0])
            inp_B3HW = inp_B3HW.to(dev, non_blocking=True)
            label_B = label_B.to(dev, non_blocking=True)
            gt_idx_Bl = vae.img_to_idxBl(inp_B3HW)
            gt_BL = torch.cat(gt_idx_Bl, dim=1).contiguous()
            x_BLCv_wo_first_l = vae.quantize.idxBl_to_var_input(gt_idx_Bl)
            logits_BLV = var(label_B, x_BLCv_wo_first_l)
            with torch.cuda.device(dev):
                E.xent_stats(logits_BLV, gt_BL, last_l, sums, accumulate=True)
            tot += B
    finally:
        var.train(training)
    s_nll, s_tail, n_cor, n_tail_cor, tot_all = D.allreduce_eval_sums(sums, tot)
    tot = round(tot_all)
    if tot == 0:
        raise E.SdvarError("eval_ep: the validation loader yielded no images")
    return (s_nll / L / tot, s_tail / last_l / tot, n_cor * (100.0 / L) / tot, n_tail_cor * (100.0 / last_l) / tot, tot, time.time() - stt)


@torch.no_grad()
def eval_vae(vae, ld_val: Iterable) -> Tuple[float, float, float, List[float], int, float]:
    """-> (rec_mse, rec_l1, vq_loss, usage_S, tot, seconds) over the (inp_B3HW in [-1, 1], label_B) batches of `ld_val` (the labels are not used).
    Per batch VQVAE.forward (vqvae.py:56-59: encoder -> VectorQuantizer2.forward -> decoder, no clamp) and sdvar_img_err_stats, which adds
    {sum |rec - inp|, sum (rec - inp)^2} to two float64 sums kept on the device.  rec_mse / rec_l1 = those sums over all pixels of all images;
    vq_loss = the image-weighted mean of the batches' mean_vq_loss; usage_S[s] = percentage of the V codes that scale s hit at least once over the
    whole loader (hits summed in int64); tot = images over all ranks.  Sums and hits are all-reduced over the ranks (sdvar_amd.dist).  The model is put
    in eval mode for the pass and restored."""
    stt = time.time()
    dev = vae.quantize.embedding.weight.device
    S, V = len(vae.quantize.v_patch_nums), vae.quantize.vocab_size
    sums = torch.zeros(2, dtype=torch.float64, device=dev)
    hits = np.zeros((S, V), dtype=np.int64)
    vq_w, n_elems, tot = 0.0, 0, 0
    training = vae.training
    vae.eval()
    try:
        for inp_B3HW, _label_B in ld_val:
            B = int(inp_B3HW.shape[0])
            inp_B3HW = inp_B3HW.to(dev, non_blocking=True)
            if inp_B3HW.dtype != torch.float32:
                inp_B3HW = inp_B3HW.float()
            rec_B3HW, _, vq, hits_SV = vae._forward_hip(inp_B3HW, False)
            with torch.cuda.device(dev):
                E.img_err_stats(rec_B3HW, inp_B3HW, sums, accumulate=True)
            hits += hits_SV.cpu().numpy()
            vq_w += vq * B
            n_elems += inp_B3HW.numel()
            tot += B
    finally:
        vae.train(training)
    s_l1, s_l2, vq_all, n_all, tot_all, hits_all = D.allreduce_vae_sums(sums, vq_w, n_elems, tot, hits)
    tot = round(tot_all)
    if tot == 0:
        raise E.SdvarError("eval_vae: the validation loader yielded no images")
    usage_S = [int(np.count_nonzero(hits_all[s])) * 100.0 / V for s in range(S)]
    return (s_l2 / n_all, s_l1 / n_all, vq_all / tot, usage_S, tot, time.time() - stt)
