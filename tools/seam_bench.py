#!/usr/bin/env python3
"""Time the operator seam (sdvar_amd/seam.py) against what it replaces in the reference's slots, in ONE process on the same tensors.

  slow_attn        vs torch's fp32 F.scaled_dot_product_attention     B 8, H 16, Lq = Lk = 680 under the ten-stage block-causal mask (teacher forcing)
                                                                      the same shape without a mask (+ the library's older route: contiguous copies of
                                                                      q, k, v and sdvar_op_attention on an fp32 cache)
                                                                      B 16, H 16, 256 queries against 680 cached keys, no mask
  fused_mlp_func   vs F.linear / tanh-GELU / F.linear                 C 1024 (hidden 4096), M = 680 * 8 and M = 64, every GEMM mode
  flash_attn_func  vs torch's SDPA in the same half dtype             fp16 and bf16, (B, L, H, 64) views of one qkv buffer / torch.cat caches, no mask:
                   and seam.slow_attn on fp32 copies of the           B 16, H 16, Lq 256 on Lk 680;  B 16, H 16, Lq 16 on Lk 91 (cached calls);
                   same operands (the only route before the slot)     B 8, H 16, L 680 (self-attention);  B 4, H 30, Lq 1024 on Lk 2240 (512^2)
  slow_attn_amp    vs torch's SDPA in the same half dtype with the    fp16 and bf16, (B, H, L, 64) views of one qkv buffer, attn_l2_norm scaling, ten-stage block-causal mask:
                   same mask, and seam.slow_attn on fp32 copies       B 8, H 16, L 680 with q / k fp32 and v half (what autocast delivers), and with all three half;
                   with the fp32 mask                                 B 16, H 16, Lq 425 on Lk 680 under rows [255:] of the mask (a two-stage verify chunk)

Every figure is the MEDIAN over --reps windows of --iters back-to-back calls, timed with device events; the candidates of one shape alternate window by window, so
drift of the machine hits them alike.  min / max of the windows are printed beside the median.  The last line is one JSON object with every median (microseconds).
python tools/seam_bench.py [--iters 20] [--reps 9] [--rows all|fp32|flash|amp]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdvar_amd import engine as E          # noqa: E402
from sdvar_amd import seam                 # noqa: E402
from sdvar_amd.ladder import LADDER_256    # noqa: E402


def windows(fns, iters, reps):
    """{name: callable} -> {name: (median, min, max)} in microseconds per call."""
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in us.items()}


def report(title, res, results, flops=None):
    print(title)
    for k, (med, lo, hi) in res.items():
        extra = f"  {flops / med * 1e-6:7.1f} TFLOP/s (algorithmic)" if flops else ""
        print(f"    {k:<34s} {med:9.1f} us  (min {lo:.1f}, max {hi:.1f}){extra}")
        results[f"{title} | {k}"] = round(med, 2)


def block_causal(patch_nums, dev):
    d = torch.cat([torch.full((pn * pn,), i) for i, pn in enumerate(patch_nums)]).to(dev)
    return torch.where(d[:, None] >= d[None, :], 0.0, float("-inf")).reshape(1, 1, len(d), len(d)).float().contiguous()


def flash_rows(a, dev, g, results):
    """seam.flash_attn_func on half operands: the reference's (B, L, H, 64) unbind(dim=2) views of one qkv buffer for q (and for k / v in self-attention), contiguous
    torch.cat caches otherwise; against torch's SDPA on the same tensors and seam.slow_attn on fp32 copies (made once, outside the timed region)."""
    for B, H, Lq, Lk in ((16, 16, 256, 680), (16, 16, 16, 91), (8, 16, 680, 680), (4, 30, 1024, 2240)):
        for dtype in (torch.float16, torch.bfloat16):
            qkv = torch.randn(B, Lq, 3, H, 64, device=dev, generator=g).to(dtype)
            q = qkv[:, :, 0]
            if Lq == Lk:
                k, v = qkv[:, :, 1], qkv[:, :, 2]
            else:
                k, v = torch.randn(B, Lk, H, 64, device=dev, generator=g).to(dtype), torch.randn(B, Lk, H, 64, device=dev, generator=g).to(dtype)
            tq, tk, tv = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)                   # (B, H, L, 64) views for the (B, H, L, c) interfaces
            fq, fk, fv = tq.float(), tk.float(), tv.float()
            diff = (seam.flash_attn_func(q, k, v, softmax_scale=0.125).float() - F.scaled_dot_product_attention(tq, tk, tv, scale=0.125).transpose(1, 2).float()).abs().max().item()
            r = windows({"seam.flash_attn_func": lambda: seam.flash_attn_func(q, k, v, softmax_scale=0.125),
                         "torch SDPA same dtype": lambda: F.scaled_dot_product_attention(tq, tk, tv, scale=0.125),
                         "seam.slow_attn on fp32 copies": lambda: seam.slow_attn(fq, fk, fv, 0.125)}, a.iters, a.reps)
            report(f"flash {str(dtype)[6:]} B{B} H{H} Lq{Lq} Lk{Lk} (max |seam - torch| {diff:.1e})", r, results, 4.0 * B * H * Lq * Lk * 64)


def amp_rows(a, dev, g, results):
    """seam.slow_attn_amp on the operands torch.autocast delivers to the slow_attn slot, under the ten-stage block-causal mask: against torch's SDPA on half copies
    with the mask in the half dtype, and seam.slow_attn on fp32 copies with the fp32 mask (all copies made once, outside the timed region).  The unmasked call of
    the same operands gives the masked / unmasked ratio, printed beside the fraction of (128-query, 64-key) tiles the skip map leaves."""
    L = sum(p * p for p in LADDER_256)
    mask = block_causal(LADDER_256, dev)
    for B, H, Lq, mixed in ((8, 16, L, True), (8, 16, L, False), (16, 16, L - 255, True)):
        for dtype in (torch.float16, torch.bfloat16):
            qkv = torch.randn(B, L, 3, H, 64, device=dev, generator=g)
            qkv[:, :, 0] = F.normalize(qkv[:, :, 0], dim=-1) * 4
            qkv[:, :, 1] = F.normalize(qkv[:, :, 1], dim=-1)
            half = qkv.to(dtype)
            fq, fk, fv = qkv.permute(2, 0, 3, 1, 4).unbind(0)
            hq, hk, hv = half.permute(2, 0, 3, 1, 4).unbind(0)
            fq, hq, m = fq[:, :, L - Lq:], hq[:, :, L - Lq:], mask[:, :, L - Lq:, :]
            mh = m.to(dtype)
            q, k = (fq, fk) if mixed else (hq, hk)
            got = seam.slow_attn_amp(q, k, hv, 1.0, attn_mask=m)
            diff = (got.float() - F.scaled_dot_product_attention(hq, hk, hv, attn_mask=mh, scale=1.0).float()).abs().max().item()
            smap = next(e[1] for e in seam._SKIP_MAPS.values() if e[0].data_ptr() == m.data_ptr())
            frac = 1.0 - smap.float().mean().item()
            r = windows({"seam.slow_attn_amp": lambda: seam.slow_attn_amp(q, k, hv, 1.0, attn_mask=m),
                         "seam.slow_attn_amp no mask": lambda: seam.slow_attn_amp(q, k, hv, 1.0),
                         "torch SDPA same dtype, same mask": lambda: F.scaled_dot_product_attention(hq, hk, hv, attn_mask=mh, scale=1.0),
                         "seam.slow_attn on fp32 copies": lambda: seam.slow_attn(fq, fk, fv, 1.0, attn_mask=m)}, a.iters, a.reps)
            title = f"amp {str(dtype)[6:]} B{B} H{H} Lq{Lq} Lk{L} {'q/k fp32, v half' if mixed else 'all half'} (max |seam - torch| {diff:.1e})"
            report(title, r, results, 4.0 * B * H * Lq * L * 64)
            ratio = r["seam.slow_attn_amp"][0] / r["seam.slow_attn_amp no mask"][0]
            print(f"    masked / unmasked time of seam.slow_attn_amp: {ratio:.3f}  (tiles visited: {frac:.3f})")
            results[f"{title} | masked_to_unmasked_ratio"] = round(ratio, 4)
            results[f"{title} | tiles_visited_fraction"] = round(frac, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rows", choices=("all", "fp32", "flash", "amp"), default="all",
                    help="fp32: the slow_attn / fused_mlp_func rows; flash: the flash_attn_func rows; amp: the slow_attn_amp rows")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seam_bench: no GPU (there is nothing to time on a CPU)")
    torch.set_grad_enabled(False)
    dev, lib, results = torch.device("cuda:0"), E.load_library(), {}
    P = lambda t: C.c_void_p(t.data_ptr())
    g = torch.Generator(device=dev).manual_seed(0)
    if a.rows in ("flash", "amp"):
        (flash_rows if a.rows == "flash" else amp_rows)(a, dev, g, results)
        print(json.dumps(results))
        return

    # ---- attention, teacher-forced shape: q, k, v are the reference's views of one (B, L, 3, H, 64) buffer (basic_var.py:93-99), attn_l2_norm scaling
    B, H, L = 8, 16, sum(p * p for p in LADDER_256)
    qkv = torch.randn(B, L, 3, H, 64, device=dev, generator=g)
    qkv[:, :, 0] = F.normalize(qkv[:, :, 0], dim=-1) * 4
    qkv[:, :, 1] = F.normalize(qkv[:, :, 1], dim=-1)
    q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)
    mask = block_causal(LADDER_256, dev)
    flops = 4.0 * B * H * L * L * 64
    diff = (seam.slow_attn(q, k, v, 1.0, attn_mask=mask) - F.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=1.0)).abs().max().item()
    smap = next(iter(seam._SKIP_MAPS.values()))[1]
    frac = 1.0 - smap.float().mean().item()
    print(f"block-causal mask L = {L}: {frac * 100:.1f} % of the (128-query, 64-key) tiles are visited; {(mask == 0).float().mean().item() * 100:.1f} % of the elements are visible; "
          f"max |seam - torch fp32| = {diff:.2e}")
    rm = windows({"seam.slow_attn": lambda: seam.slow_attn(q, k, v, 1.0, attn_mask=mask),
                  "torch SDPA fp32": lambda: F.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=1.0)}, a.iters, a.reps)
    report(f"attention B{B} H{H} L{L} block-causal mask", rm, results, flops)

    qb, vs, st = (C.c_int32 * 1)(0), (C.c_int32 * 1)(L), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    old_out = torch.empty(B, L, H * 64, device=dev)

    def old_route():
        qc, kc, vc = q.contiguous(), k.contiguous(), v.contiguous()
        E._check(lib.sdvar_op_attention(P(qc), P(kc), P(vc), 0, P(old_out), None, 0, 3, B, H, L, L, L, 1, qb, vs, st))
    rn = windows({"seam.slow_attn": lambda: seam.slow_attn(q, k, v, 1.0),
                  "torch SDPA fp32": lambda: F.scaled_dot_product_attention(q, k, v, scale=1.0),
                  "copies + sdvar_op_attention fmt 0": old_route}, a.iters, a.reps)
    report(f"attention B{B} H{H} L{L} no mask", rn, results, flops)
    ratio = rm["seam.slow_attn"][0] / rn["seam.slow_attn"][0]
    print(f"    masked / unmasked time of seam.slow_attn: {ratio:.3f}  (tiles visited: {frac:.3f})")
    results["masked_to_unmasked_ratio"] = round(ratio, 4)
    results["tiles_visited_fraction"] = round(frac, 4)

    # ---- attention, cached call: 256 new queries (views of the qkv buffer) against 680 keys of the concatenated (B, H, L, 64) caches
    B2, Lq = 16, 256
    qkv2 = torch.randn(B2, Lq, 3, H, 64, device=dev, generator=g)
    q2 = qkv2.permute(2, 0, 3, 1, 4)[0]
    k2, v2 = torch.randn(B2, H, L, 64, device=dev, generator=g), torch.randn(B2, H, L, 64, device=dev, generator=g)
    s2 = 0.25 / math.sqrt(64)
    rc = windows({"seam.slow_attn": lambda: seam.slow_attn(q2, k2, v2, s2),
                  "torch SDPA fp32": lambda: F.scaled_dot_product_attention(q2, k2, v2, scale=s2)}, a.iters, a.reps)
    report(f"attention B{B2} H{H} Lq{Lq} Lk{L} no mask", rc, results, 4.0 * B2 * H * Lq * L * 64)

    # ---- fused MLP
    Cw, hid = 1024, 4096
    w1, b1 = torch.randn(hid, Cw, device=dev, generator=g) / math.sqrt(Cw), torch.randn(hid, device=dev, generator=g)
    w2, b2 = torch.randn(Cw, hid, device=dev, generator=g) / math.sqrt(hid), torch.randn(Cw, device=dev, generator=g)
    for M in (L * 8, 64):
        x = torch.randn(M, Cw, device=dev, generator=g)

        def seam_mlp(mode):
            def f():
                seam.configure(gemm_mode=mode)
                return seam.fused_mlp_func(x=x, weight1=w1, weight2=w2, bias1=b1, bias2=b2, activation="gelu_approx", save_pre_act=False, return_residual=False,
                                           checkpoint_lvl=0, heuristic=0, process_group=None)
            return f
        fns = {f"seam.fused_mlp_func {m}": seam_mlp(m) for m in E.GEMM_MODES}
        fns["torch linear/gelu/linear fp32"] = lambda: F.linear(F.gelu(F.linear(x, w1, b1), approximate="tanh"), w2, b2)
        report(f"mlp M{M} C{Cw}", windows(fns, a.iters, a.reps), results, 4.0 * M * Cw * hid)
    seam.configure(gemm_mode=E.DEFAULT_GEMM_MODE)
    if a.rows == "all":
        flash_rows(a, dev, g, results)
        amp_rows(a, dev, g, results)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
