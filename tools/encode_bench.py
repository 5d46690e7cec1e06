#!/usr/bin/env python3
"""VQVAE image encoding timing: f = quant_conv(encoder(img)) on the HIP encoder (csrc/vae.hip, csrc/conv.hip) and the ten-scale residual
quantisation (csrc/quant.hip), per batch, with the convolutions' TF/s from their algorithmic FLOPs.
python tools/encode_bench.py [--iters 10]        (cases: 256^2 B = 8 and 512^2 B = 2, operand formats f16x2 and bf16x3; one JSON line per case)"""
import argparse, json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdvar_amd import engine as E
from sdvar_amd.ladder import LADDER_256, LADDER_512
from sdvar_amd.weights import vae_state_dict


def encoder_flops(img_hw, ch=160, ch_mult=(1, 1, 2, 2, 4), nrb=2, z=32):
    """Multiply-adds x 2 of every convolution and of the attention products for one image."""
    fl, H, cprev = 2.0 * img_hw * img_hw * 3 * ch * 9, img_hw, ch
    conv = lambda H, ci, co, k: 2.0 * H * H * ci * co * k
    for lv, m in enumerate(ch_mult):
        c = ch * m
        for _ in range(nrb):
            fl += conv(H, cprev, c, 9) + conv(H, c, c, 9) + (conv(H, cprev, c, 1) if cprev != c else 0.0)
            cprev = c
            if lv == len(ch_mult) - 1:
                fl += conv(H, c, 3 * c, 1) + conv(H, c, c, 1) + 4.0 * (H * H) ** 2 * c
        if lv != len(ch_mult) - 1:
            fl += conv(H // 2, c, c, 9)
            H //= 2
    c = cprev
    fl += 2 * (2 * conv(H, c, c, 9)) + conv(H, c, 3 * c, 1) + conv(H, c, c, 1) + 4.0 * (H * H) ** 2 * c
    return fl + conv(H, c, z, 9) + conv(H, z, z, 9)


ap = argparse.ArgumentParser(); ap.add_argument("--iters", type=int, default=10)
a = ap.parse_args()
dev = torch.device("cuda:0")
torch.set_grad_enabled(False)


def timed(fn, iters):
    for _ in range(2): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(iters): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / iters * 1e3


for pns, B in ((LADDER_256, 8), (LADDER_512, 2)):
    sd = vae_state_dict(pns, "perf", 1236, with_encoder=True)
    hw = pns[-1]
    img = (torch.rand(B, 3, hw * 16, hw * 16, device=dev) * 2 - 1).contiguous()
    q = E.QuantCtx(sd, pns, B, dev)
    for mode in ("f16x2", "bf16x3"):
        enc = E.VaeEncCtx(sd, B, dev, latent_hw=hw, conv_mode=mode)
        f = enc.encode(img)
        enc_ms = timed(lambda: enc.encode(img, out=f), a.iters)
        quant_ms = timed(lambda: q.encode(f), a.iters)
        tf = encoder_flops(hw * 16) * B / (enc_ms * 1e-3) / 1e12
        print(json.dumps({"img": hw * 16, "B": B, "conv_mode": mode, "encode_ms": round(enc_ms, 3), "quantise_ms": round(quant_ms, 3),
                          "encoder_gflop_per_image": round(encoder_flops(hw * 16) / 1e9, 1), "encode_tflops": round(tf, 1)}))
        enc.close()
    q.close()
