#!/usr/bin/env python3
"""Tokenizer validation timing: VQVAE.forward (encoder -> quantiser with statistics -> unclamped decoder) against the same batch through
img_to_reconstructed_img(last_one=True), and the statistics launches on their own: the quantiser chain with and without them
(QuantCtx.encode_stats / encode on the same f), sdvar_img_err_stats on the reconstruction, and eval_vae's per-batch copy of the hit counts to the host.
python tools/vae_eval_bench.py [--iters 10] [--batches 8 32]        (256^2 images, the default conv mode; one JSON line per batch size)"""
import argparse, json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdvar_amd import engine as E
from sdvar_amd.ladder import LADDER_256
from sdvar_amd.vqvae import VQVAE
from sdvar_amd.weights import vae_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--batches", type=int, nargs="+", default=[8, 32])
a = ap.parse_args()
dev = torch.device("cuda:0")
torch.set_grad_enabled(False)


def timed(fn, iters):
    for _ in range(2): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(iters): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / iters * 1e3


pns = LADDER_256
sd = vae_state_dict(pns, "perf", 1236, with_encoder=True)
for B in a.batches:
    vae = VQVAE(vocab_size=4096, ch=160, v_patch_nums=pns).to(dev)
    vae.load_state_dict(dict(sd), strict=True)
    img = (torch.rand(B, 3, 256, 256, device=dev) * 2 - 1).contiguous()
    fwd_ms = timed(lambda: vae(img, ret_usages=True), a.iters)
    rec_ms = timed(lambda: vae.img_to_reconstructed_img(img, last_one=True), a.iters)
    f = vae.img_to_f(img)
    q = vae.quantize._ctx(dev, B, pns)
    enc_ms = timed(lambda: q.encode(f), a.iters)
    stats_ms = timed(lambda: q.encode_stats(f, straight_through=True), a.iters)
    rec = vae(img)[0]
    sums = torch.zeros(2, dtype=torch.float64, device=dev)
    hits = q.encode_stats(f)[3]
    copy_ms = timed(lambda: hits.cpu().numpy(), a.iters)          # eval_vae's per-batch blocking copy of the (S, V) int32 hit counts
    err_ms = timed(lambda: E.img_err_stats(rec, img, sums, accumulate=True), a.iters)
    print(json.dumps({"img": 256, "B": B, "conv_mode": vae._hip_ctx.conv_mode, "forward_ms": round(fwd_ms, 3), "forward_img_per_s": round(B / fwd_ms * 1e3, 1),
                      "reconstruct_ms": round(rec_ms, 3), "reconstruct_img_per_s": round(B / rec_ms * 1e3, 1), "quant_encode_ms": round(enc_ms, 3),
                      "quant_encode_stats_ms": round(stats_ms, 3), "quant_stats_launches_ms": round(stats_ms - enc_ms, 3), "img_err_stats_ms": round(err_ms, 3), "hits_copy_ms": round(copy_ms, 3),
                      "stats_share_of_forward": round((stats_ms - enc_ms + err_ms) / fwd_ms, 4)}))
    vae.refresh_hip()
    del vae
