#!/usr/bin/env python3
"""Time seam.qk_l2norm (csrc/qknorm_train.hip) against torch's eager chain of the reference's attention between the QKV GEMM and the attention call
(basic_var.py:93-105) in ONE process on the same tensors:

    torch eager   qkv = F.linear(x, W, cat(q_bias, 0, v_bias)).view(B, L, 3, H, 64); q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0);
                  q = F.normalize(q, dim=-1).mul(scale_log.clamp_max(max_log).exp()); k = F.normalize(k, dim=-1)
    seam          q, k, v = seam.qk_l2norm(F.linear(x, W).view(B, L, 3, H, 64), scale_log, max_log, q_bias, v_bias)
    linear alone  F.linear(x, W): the GEMM both candidates contain, for subtraction (its backward: dx and dW from an upstream gradient of qkv's dtype)

The bias add is on both sides - inside torch's GEMM, inside this side's kernel - so the v this side writes because of it is charged to this side.
Cases: the teacher-forcing shape B 8, L 680 at H 16 (d16) and H 30 (d30); float32 ('f32'), and torch.autocast to float16 ('amp16') and bfloat16 ('ampbf16') over
float32 master parameters.  Legs: the forward under grad, the backward alone (autograd.grad on retained graphs, with respect to x, W, the biases and scale_log, for
upstream gradients of q, k and v), forward + backward; and torch.cuda.max_memory_allocated above the resident tensors of one forward + backward.

x and the upstream gradients are --copies distinct buffers each, used round-robin (default: as many as exceed 512 MiB together).  Every figure is the MEDIAN over
--reps windows of --iters back-to-back calls, timed with device events; the candidates alternate window by window, so drift of the machine hits them alike; min / max of
the windows are printed beside the median, and the host time to enqueue one call beside the device time.  Traffic floors of the normalisation alone (no GEMM), with
M = B L rows, C = 64 H and s bytes per element of qkv: forward (3 s + 8 + s) M C (qkv read; q, k float32 and v written), backward (2 s + 8 + s + 3 s) M C (the q and k
slots of qkv, dq, dk, dv read; dqkv written), at 6.3 TB/s.  One JSON line at the end.
python tools/seam_qknorm_bench.py [--iters 100] [--reps 5] [--heads 16 30]"""
import argparse
import itertools
import json
import math
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdvar_amd import engine as E          # noqa: E402
from sdvar_amd import seam                 # noqa: E402

STREAM_RATE = 6.3e12        # bytes / s: the HBM stream rate DESIGN.md section 4d measures against
MAX_LOG = math.log(100.0)
MODES = {"f32": None, "amp16": torch.float16, "ampbf16": torch.bfloat16}


def windows(fns, iters, reps):
    """{name: callable} -> {name: (median, min, max, host)} in microseconds per call; host = the median host-clock time to ENQUEUE one call."""
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us, host = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            e0.record()
            t0 = time.perf_counter()
            for _ in range(iters):
                f()
            t1 = time.perf_counter()
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / iters)
            host[k].append((t1 - t0) * 1e6 / iters)
    return {k: (statistics.median(v), min(v), max(v), statistics.median(host[k])) for k, v in us.items()}


def report(title, res, out, nbytes):
    floor = nbytes / STREAM_RATE * 1e6
    print(f"{title}   (traffic floor of the normalisation alone: {floor:.1f} us)")
    lin = res["linear alone"][0]
    for k, (med, lo, hi, host) in res.items():
        extra = "" if k == "linear alone" else f"  minus the linear: {med - lin:8.1f} us = {(med - lin) / floor:5.1f} floors"
        print(f"    {k:<14s} {med:9.1f} us  (min {lo:.1f}, max {hi:.1f}; host enqueue {host:.1f}){extra}")
        out[f"{title} | {k}"] = {"us": round(med, 2), "min_us": round(lo, 2), "max_us": round(hi, 2), "host_us": round(host, 2)}
    t, s = res["torch eager"][0], res["seam"][0]
    print(f"    torch / seam {t / s:5.2f}x with the GEMM on both sides, {(t - lin) / max(s - lin, 1e-9):5.2f}x with the linear's time taken off both")
    out[f"{title} | torch / seam"] = round(t / s, 3)
    out[f"{title} | torch / seam minus linear"] = round((t - lin) / max(s - lin, 1e-9), 3)
    out[f"{title} | floor_us"] = round(floor, 2)


def peak_above_resident(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    del r
    return torch.cuda.max_memory_allocated() - base


def case(H, mode, a, dev):
    B, L = 8, 680
    M, Cc = B * L, 64 * H
    half = MODES[mode]
    qdt, s = (half, 2) if half else (torch.float32, 4)
    gen = torch.Generator(device=dev).manual_seed(H)
    ncopy = a.copies or (512 * 2 ** 20) // (4 * M * Cc * 4) + 1          # x, gq, gk, gv per copy
    rn = lambda *shape: torch.randn(*shape, device=dev, generator=gen)
    xs = [rn(B, L, Cc).requires_grad_() for _ in range(ncopy)]
    gs = [(rn(B, H, L, 64), rn(B, H, L, 64), rn(B, H, L, 64).to(qdt)) for _ in range(ncopy)]
    gl = [rn(B, L, 3 * Cc).to(qdt) for _ in range(ncopy)]
    W = (rn(3 * Cc, Cc) / Cc ** 0.5).requires_grad_()
    qb, vb = (0.1 * rn(Cc)).requires_grad_(), (0.1 * rn(Cc)).requires_grad_()
    zero = torch.zeros(Cc, device=dev)
    sl = torch.full((1, H, 1, 1), math.log(4.0), device=dev).requires_grad_()
    ring = itertools.cycle(range(ncopy))
    cast = lambda: torch.autocast("cuda", dtype=half or torch.float16, enabled=half is not None)

    def t_fwd(i):
        with cast():
            qkv = F.linear(xs[i], W, torch.cat((qb, zero, vb))).view(B, L, 3, H, 64)
            q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)
            return F.normalize(q, dim=-1).mul(sl.clamp_max(MAX_LOG).exp()), F.normalize(k, dim=-1), v

    def s_fwd(i):
        with cast():
            return seam.qk_l2norm(F.linear(xs[i], W).view(B, L, 3, H, 64), sl.view(H), MAX_LOG, qb, vb)

    def l_fwd(i):
        with cast():
            return F.linear(xs[i], W)

    fwds = {"seam": s_fwd, "torch eager": t_fwd, "linear alone": l_fwd}
    wrt = lambda k, i: (xs[i], W) if k == "linear alone" else (xs[i], W, qb, vb, sl)
    up = lambda k, i: gl[i] if k == "linear alone" else gs[i]
    out = {"case": f"B{B} L{L} H{H} {mode}", "rows": M, "C": Cc, "mode": mode, "buffers_in_rotation": ncopy}

    a_, b_ = s_fwd(0), t_fwd(0)          # agreement first (torch on the GPU is the other candidate, not the oracle: tests/test_gpu_seam_qknorm.py has fp64)
    assert [t.dtype for t in a_] == [t.dtype for t in b_]
    d = [float((x.float() - y.float()).abs().max()) for x, y in zip(a_, b_)]
    print(f"{out['case']}: max |seam - torch|: q {d[0]:.2e}, k {d[1]:.2e}, v {d[2]:.2e}; {ncopy} buffers of each operand in rotation")
    del a_, b_

    f_bytes, b_bytes = (3 * s + 8 + s) * M * Cc, (2 * s + 8 + s + 3 * s) * M * Cc
    report("forward", windows({k: (lambda f=f: f(next(ring))) for k, f in fwds.items()}, a.iters, a.reps), out, f_bytes)
    graphs = {k: [f(i) for i in range(ncopy)] for k, f in fwds.items()}

    def bwd(k):
        def f():
            i = next(ring)
            return torch.autograd.grad(graphs[k][i], wrt(k, i), up(k, i), retain_graph=True)
        return f
    report("backward", windows({k: bwd(k) for k in fwds}, a.iters, a.reps), out, b_bytes)
    del graphs

    def both(k):
        def f():
            i = next(ring)
            return torch.autograd.grad(fwds[k](i), wrt(k, i), up(k, i))
        return f
    report("forward + backward", windows({k: both(k) for k in fwds}, a.iters, a.reps), out, f_bytes + b_bytes)
    out["peak_bytes_above_resident"] = {k: peak_above_resident(both(k)) for k in fwds}
    p = out["peak_bytes_above_resident"]
    print(f"    peak memory above the resident tensors, one forward + backward: seam {p['seam'] / 2 ** 20:.1f} MiB, torch {p['torch eager'] / 2 ** 20:.1f} MiB, "
          f"linear alone {p['linear alone'] / 2 ** 20:.1f} MiB (one float32 (M, C) activation is {4 * M * Cc / 2 ** 20:.1f} MiB)")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--heads", type=int, nargs="+", default=[16, 30])
    ap.add_argument("--modes", nargs="+", default=list(MODES), choices=list(MODES))
    ap.add_argument("--copies", type=int, default=0, help="buffers of each operand in rotation (0: enough to exceed 512 MiB)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seam_qknorm_bench: no GPU (there is nothing to time on a CPU)")
    dev = torch.device("cuda:0")
    E.load_library()
    res = {"cases": []}
    for H in a.heads:
        for mode in a.modes:
            res["cases"].append(case(H, mode, a, dev))
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
