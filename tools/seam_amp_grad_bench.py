#!/usr/bin/env python3
"""Time seam.slow_attn_amp_grad (sdvar_op_sdpa_hm_lse + the three launches of csrc/attention_sdpa_h_bwd.hip) against torch's own half-precision
F.scaled_dot_product_attention under autograd and against seam.slow_attn_grad in fp32, in ONE process on the same data.

Shape: teacher forcing of d16 - B 8, H 16, L 680, the ten-stage block-causal mask.  Two operand sets per half dtype:
  mixed  what attn_l2_norm leaves under torch.autocast: q, k fp32 (normalised, q scaled by 4), v half, each a (B, H, L, 64) view of a (B, L, H, 64) leaf;
  half   all three half, views of one (B, L, 3, H, 64) leaf.
Torch's SDPA takes one dtype, so for the mixed set it is handed q.to(dtype), k.to(dtype) inside the timed call (the casts autocast would insert) and a mask cast to the
half dtype once, outside.  Rows: forward under grad, backward alone (one autograd.grad call on a retained graph), forward + backward.

Every figure is the MEDIAN over --reps windows of --iters back-to-back calls, timed with device events; the candidates alternate window by window, so drift of
the machine hits them alike.  min / max of the windows are printed beside the median.  The last line is one JSON object (microseconds).
Run it under a time limit:  timeout 300 python tools/seam_amp_grad_bench.py [--iters 10] [--reps 7] [--dtypes fp16,bf16]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sdvar_amd import seam                 # noqa: E402
from sdvar_amd.ladder import LADDER_256    # noqa: E402
from seam_grad_bench import block_causal, windows          # noqa: E402


def report(title, res, results):
    print(title)
    for k, (med, lo, hi) in res.items():
        print(f"    {k:<44s} {med:9.1f} us  (min {lo:.1f}, max {hi:.1f})")
        results[f"{title} | {k}"] = round(med, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dtypes", default="fp16,bf16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seam_amp_grad_bench: no GPU (there is nothing to time on a CPU)")
    dev, results = torch.device("cuda:0"), {}
    g = torch.Generator(device=dev).manual_seed(0)
    B, H, L = 8, 16, sum(p * p for p in LADDER_256)
    qkv = torch.randn(B, L, 3, H, 64, device=dev, generator=g)
    qkv[:, :, 0] = F.normalize(qkv[:, :, 0], dim=-1) * 4
    qkv[:, :, 1] = F.normalize(qkv[:, :, 1], dim=-1)
    dout32 = torch.randn(B, L, H, 64, device=dev, generator=g).permute(0, 2, 1, 3)            # the layout the caller's .transpose(1, 2).reshape(B, L, C) hands back
    mask = block_causal(LADDER_256, dev)
    leaf32 = qkv.clone().requires_grad_()
    q32, k32, v32 = leaf32.permute(2, 0, 3, 1, 4).unbind(0)

    for name in a.dtypes.split(","):
        dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[name]
        dout, mask_h = dout32.to(dtype), mask.to(dtype)
        lq, lk = (qkv[:, :, i].contiguous().requires_grad_() for i in (0, 1))                 # (B, L, H, 64) fp32
        lv = qkv[:, :, 2].to(dtype).contiguous().requires_grad_()
        mixed = [t.permute(0, 2, 1, 3) for t in (lq, lk, lv)]
        leaf_h = qkv.to(dtype).requires_grad_()
        half = list(leaf_h.permute(2, 0, 3, 1, 4).unbind(0))
        sets = {"mixed": (mixed, [lq, lk, lv]), "half": (half, [leaf_h])}

        fwd, leaves, dos = {}, {}, {}
        for sname, (ops, lv_) in sets.items():
            fwd[f"seam.slow_attn_amp_grad, {sname}"] = lambda ops=ops: seam.slow_attn_amp_grad(*ops, 1.0, attn_mask=mask)
            fwd[f"torch SDPA {name}, {sname}"] = lambda ops=ops: F.scaled_dot_product_attention(ops[0].to(dtype), ops[1].to(dtype), ops[2], attn_mask=mask_h, scale=1.0)
            leaves[f"seam.slow_attn_amp_grad, {sname}"] = leaves[f"torch SDPA {name}, {sname}"] = lv_
        fwd["seam.slow_attn_grad, fp32"] = lambda: seam.slow_attn_grad(q32, k32, v32, 1.0, attn_mask=mask)
        leaves["seam.slow_attn_grad, fp32"] = [leaf32]
        for k in fwd:
            dos[k] = dout32 if k.endswith("fp32") else dout

        # ---- agreement first (torch in half on the GPU is the other candidate, not the oracle: tests/test_gpu_seam_amp_grad.py has float64)
        for sname in sets:
            so, to = fwd[f"seam.slow_attn_amp_grad, {sname}"](), fwd[f"torch SDPA {name}, {sname}"]()
            sg = torch.autograd.grad(so, sets[sname][1], dout)
            tg = torch.autograd.grad(to, sets[sname][1], dout)
            print(f"{name} {sname}: max |seam - torch {name}|: out {(so.float() - to.float()).abs().max().item():.2e}, grads "
                  + ", ".join(f"{(x.float() - y.float()).abs().max().item():.2e}" for x, y in zip(sg, tg)) + f" (max |grad| {max(y.abs().max().item() for y in tg):.2e})")

        report(f"{name}: forward under grad", windows(fwd, a.iters, a.reps), results)
        outs = {k: f() for k, f in fwd.items()}
        report(f"{name}: backward (autograd.grad to the leaves)",
               windows({k: (lambda k=k: torch.autograd.grad(outs[k], leaves[k], dos[k], retain_graph=True)) for k in fwd}, a.iters, a.reps), results)
        del outs
        report(f"{name}: forward + backward",
               windows({k: (lambda k=k, f=f: torch.autograd.grad(f(), leaves[k], dos[k])) for k, f in fwd.items()}, a.iters, a.reps), results)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
