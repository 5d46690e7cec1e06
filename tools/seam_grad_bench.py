#!/usr/bin/env python3
"""Time seam.slow_attn_grad (HIP forward with log-sum-exp + the three backward launches of csrc/attention_sdpa_bwd.hip) against torch's own
F.scaled_dot_product_attention forward and backward, in ONE process on the same tensors.

Shape: teacher forcing of d16 - B 8, H 16, L 680, the ten-stage block-causal mask, q / k / v the reference's views of one (B, L, 3, H, 64) buffer
(basic_var.py:93-99) with attn_l2_norm scaling.  Rows: forward under grad (with the LSE write), backward alone (one autograd.grad call on a retained graph:
sdvar_op_sdpa_bwd plus autograd's dispatch), forward + backward; each for the seam with the skip map, the seam without it (the same mask handed to the C entry
points with skip_map = NULL) and torch.  The inference forward (seam.slow_attn, no LSE) is timed next to them.

Every figure is the MEDIAN over --reps windows of --iters back-to-back calls, timed with device events; the candidates alternate window by window, so drift of
the machine hits them alike.  min / max of the windows are printed beside the median.  Algorithmic work: 2 score-sized products forward (4 B H L^2 64 FLOP), 7
backward (dP, dV, dQ, dK and the score recomputed in both kernels: 14 B H L^2 64), counted WITHOUT the mask.  The last line is one JSON object (microseconds).
python tools/seam_grad_bench.py [--iters 10] [--reps 9]"""
import argparse
import ctypes as C
import json
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


def report(title, res, results, flops):
    print(title)
    for k, (med, lo, hi) in res.items():
        print(f"    {k:<34s} {med:9.1f} us  (min {lo:.1f}, max {hi:.1f})  {flops / med * 1e-6:7.1f} TFLOP/s (algorithmic, mask not counted)")
        results[f"{title} | {k}"] = round(med, 2)


def block_causal(patch_nums, dev):
    d = torch.cat([torch.full((pn * pn,), i) for i, pn in enumerate(patch_nums)]).to(dev)
    return torch.where(d[:, None] >= d[None, :], 0.0, float("-inf")).reshape(1, 1, len(d), len(d)).float().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seam_grad_bench: no GPU (there is nothing to time on a CPU)")
    dev, lib, results = torch.device("cuda:0"), E.load_library(), {}
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    g = torch.Generator(device=dev).manual_seed(0)
    B, H, L = 8, 16, sum(p * p for p in LADDER_256)
    qkv = torch.randn(B, L, 3, H, 64, device=dev, generator=g)
    qkv[:, :, 0] = F.normalize(qkv[:, :, 0], dim=-1) * 4
    qkv[:, :, 1] = F.normalize(qkv[:, :, 1], dim=-1)
    dout = torch.randn(B, L, H, 64, device=dev, generator=g).permute(0, 2, 1, 3)              # the layout the caller's .transpose(1, 2).reshape(B, L, C) hands back
    mask = block_causal(LADDER_256, dev)
    leaf = qkv.clone().requires_grad_()
    q, k, v = leaf.permute(2, 0, 3, 1, 4).unbind(0)

    # ---- agreement first: same inputs, same upstream gradient (fp32 torch on the GPU is the other candidate, not the oracle: tests/test_gpu_seam_grad.py has fp64)
    so = seam.slow_attn_grad(q, k, v, 1.0, attn_mask=mask)
    sg, = torch.autograd.grad(so, leaf, dout)
    to = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=1.0)
    tg, = torch.autograd.grad(to, leaf, dout)
    smap = next(e[1] for e in seam._SKIP_MAPS.values() if e[0].data_ptr() == mask.data_ptr())
    frac = 1.0 - smap.float().mean().item()
    print(f"B{B} H{H} L{L}: {frac * 100:.1f} % of the (128-query, 64-key) tiles are visited; max |seam - torch fp32|: out {(so - to).abs().max().item():.2e}, "
          f"grad {(sg - tg).abs().max().item():.2e} (max |grad| {tg.abs().max().item():.2e})")
    results["tiles_visited_fraction"] = round(frac, 4)

    # ---- the C entry points directly, with and without the skip map (the Python slot always passes the map)
    qd, kd, vd = (t.detach() for t in (q, k, v))
    out, lse, delta = torch.empty(B, L, H, 64, device=dev), torch.empty(B, H, L, device=dev), torch.empty(B * H * L, device=dev)
    dq, dk, dv = (torch.empty(B, L, H, 64, device=dev) for _ in range(3))
    blhc = lambda t: (t.stride(0), t.stride(2), t.stride(1))
    s12 = (C.c_int64 * 12)(*(t.stride(i) for t in (qd, kd, vd) for i in (0, 1, 2)), *blhc(out))
    s24 = (C.c_int64 * 24)(*(t.stride(i) for t in (qd, kd, vd) for i in (0, 1, 2)), *blhc(out), *(dout.stride(i) for i in (0, 1, 2)), *blhc(dq), *blhc(dk), *blhc(dv))
    bstr = (C.c_int64 * 3)(0, 0, mask.stride(2))

    def c_fwd(sm, with_lse=True):
        def f():
            st = E._stream()
            if with_lse:
                E._check(lib.sdvar_op_sdpa_lse(P(qd), P(kd), P(vd), P(out), P(lse), s12, P(mask), 1, bstr, P(sm), B, H, L, L, 64, 1.0, st))
            else:
                E._check(lib.sdvar_op_sdpa(P(qd), P(kd), P(vd), P(out), s12, P(mask), 1, bstr, P(sm), B, H, L, L, 64, 1.0, st))
        return f

    def c_bwd(sm, want=(True, True, True)):
        def f():
            E._check(lib.sdvar_op_sdpa_bwd(P(qd), P(kd), P(vd), P(out), P(dout), P(lse), P(delta), P(dq) if want[0] else None, P(dk) if want[1] else None,
                                           P(dv) if want[2] else None, s24, P(mask), 1, bstr, P(sm), B, H, L, L, 64, 1.0, E._stream()))
        return f
    c_fwd(smap)()
    fl = 4.0 * B * H * L * L * 64
    r = windows({"sdvar_op_sdpa (no LSE), skip map": c_fwd(smap, False), "sdvar_op_sdpa_lse, skip map": c_fwd(smap), "sdvar_op_sdpa_lse, no skip map": c_fwd(None)},
                a.iters, a.reps)
    report("forward, C entry points", r, results, fl)
    rb = windows({"sdvar_op_sdpa_bwd, skip map": c_bwd(smap), "sdvar_op_sdpa_bwd, no skip map": c_bwd(None),
                  "  dq only, skip map": c_bwd(smap, (True, False, False)), "  dk + dv only, skip map": c_bwd(smap, (False, True, True))}, a.iters, a.reps)
    report("backward, C entry points", rb, results, 3.5 * fl)
    ratio = rb["sdvar_op_sdpa_bwd, skip map"][0] / r["sdvar_op_sdpa_lse, skip map"][0]
    print(f"    backward / forward time with the skip map: {ratio:.2f}  (algorithmic work: 3.5)")
    results["backward_to_forward_ratio"] = round(ratio, 3)

    # ---- through autograd, as a trainer sees it
    def seam_fwd():
        return seam.slow_attn_grad(q, k, v, 1.0, attn_mask=mask)

    def torch_fwd():
        return F.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=1.0)
    rf = windows({"seam.slow_attn_grad": seam_fwd, "torch SDPA fp32": torch_fwd}, a.iters, a.reps)
    report("forward under grad (autograd)", rf, results, fl)
    so, to = seam_fwd(), torch_fwd()
    rg = windows({"seam.slow_attn_grad": lambda: torch.autograd.grad(so, leaf, dout, retain_graph=True),
                  "torch SDPA fp32": lambda: torch.autograd.grad(to, leaf, dout, retain_graph=True)}, a.iters, a.reps)
    report("backward (autograd.grad to the qkv leaf)", rg, results, 3.5 * fl)
    rt = windows({"seam.slow_attn_grad": lambda: torch.autograd.grad(seam_fwd(), leaf, dout),
                  "torch SDPA fp32": lambda: torch.autograd.grad(torch_fwd(), leaf, dout)}, a.iters, a.reps)
    report("forward + backward (autograd)", rt, results, 4.5 * fl)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
