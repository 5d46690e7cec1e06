#!/usr/bin/env python3
"""Teacher-forced VAR.forward timing (the validation pass of sdvar_amd.evaluate): one pass of P images through sdvar_model_begin_rows,
sdvar_embed_teacher and sdvar_stage_forward over all stages (M = L * P rows per GEMM), and sdvar_xent_stats on its logits.
python tools/eval_bench.py [--iters 5]      (cases: d16 and d30 at 256^2 with P = 8, 16, 32, d16 at 512^2 with P = 8; GEMM modes f16x2 and bf16x3;
one JSON line per case: ms per pass, xent_stats us, images/s, algorithmic GFLOP per image and achieved TF/s)"""
import argparse, json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdvar_amd import engine as E
from sdvar_amd.ladder import LADDER_256, LADDER_512, as_ladder
from sdvar_amd.weights import var_state_dict_device


def gflop_per_image(depth, pns, V=4096):
    """Blocks 24 C^2 depth per token, head 2 C V per token, attention 4 C depth sum_s lens[s] cum[s] (QK^T and PV over the visible keys)."""
    lad, C = as_ladder(pns), 64 * depth
    att = sum(l * c for l, c in zip(lad.lens, lad.cum))
    return (24.0 * C * C * depth * lad.L + 2.0 * C * V * lad.L + 4.0 * C * depth * att) / 1e9


ap = argparse.ArgumentParser(); ap.add_argument("--iters", type=int, default=5)
a = ap.parse_args()
dev = torch.device("cuda:0")
torch.set_grad_enabled(False)


def timed(fn, iters):
    for _ in range(2): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(iters): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / iters * 1e3


for depth, pns, Ps in ((16, LADDER_256, (8, 16, 32)), (30, LADDER_256, (8, 16, 32)), (16, LADDER_512, (8,))):
    sd = var_state_dict_device(depth, pns, dev, mode="perf")
    lad = as_ladder(pns)
    for mode in ("f16x2", "bf16x3"):
        for P in Ps:
            ctx = E.ModelCtx(sd, depth, pns, (P + 1) // 2, lad.S, dev, gemm_mode=mode)
            g = torch.Generator(device=dev); g.manual_seed(P)
            labels = torch.randint(0, 1000, (P,), device=dev, generator=g)
            xv = torch.randn(P, lad.L - 1, 32, device=dev, generator=g)
            x = torch.empty(P, lad.L, 64 * depth, device=dev)
            logits = torch.empty(P, lad.L, 4096, device=dev)
            tg = torch.randint(0, 4096, (P, lad.L), device=dev, generator=g)
            sums = torch.zeros(4, dtype=torch.float64, device=dev)

            def one_pass():
                ctx.begin_rows(labels); ctx.embed_teacher(xv, x); ctx.forward(x, 0, lad.S, logits)
            ms = timed(one_pass, a.iters)
            xent_us = timed(lambda: E.xent_stats(logits, tg, pns[-1] ** 2, sums), 20) * 1e3
            gf = gflop_per_image(depth, pns)
            print(json.dumps({"depth": depth, "img": pns[-1] * 16, "P": P, "gemm_mode": mode, "forward_ms_per_pass": round(ms, 2),
                              "xent_stats_us": round(xent_us, 1), "xent_gbps": round(4.0 * P * lad.L * 4096 / (xent_us * 1e-6) / 1e9, 0),
                              "images_per_s": round(P / (ms * 1e-3), 1), "gflop_per_image": round(gf, 1), "tflops": round(gf * P / ms, 1)}), flush=True)
            ctx.close(); del x, logits
            torch.cuda.empty_cache()
    del sd
    torch.cuda.empty_cache()
