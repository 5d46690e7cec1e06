#!/usr/bin/env python3
"""Time seam.cross_entropy (csrc/xent_train.hip: sdvar_xent_train_fwd / sdvar_xent_train_bwd) against torch's nn.CrossEntropyLoss(label_smoothing=0.1,
reduction='none') forward and backward and, for the forward, against engine.xent_stats - in ONE process on the same tensors.

Cases: the trainer's loss call for d16 256^2 (trainer.py:112): V = 4096, rows = B * 680 for B in 8, 16, 32, eps = 0.1, a random per-row upstream gradient.
Rows of each case: forward (engine call with the lse write; the no-grad seam call; xent_stats; torch under grad, which keeps its log_softmax; torch under no_grad),
backward alone (the engine call with plain and with non-temporal stores; seam and torch through autograd.grad on a retained graph), the same two store flavours
followed by one pass that reads the gradient (its consumer), forward + backward through autograd (seam, torch), and torch.cuda.max_memory_allocated above the
resident tensors across one forward + backward of each path.  Beside each device time stands the host time to enqueue one call.

The logits of one case are --copies distinct buffers used round-robin (default: as many as exceed 512 MiB together), so that no call finds its input in the 256 MiB
Infinity Cache from the call before: the rates are HBM rates at every B.  Every figure is the MEDIAN over --reps windows of --iters back-to-back calls, timed with
device events; the candidates alternate window by window, so drift of the machine hits them alike; min / max of the windows are printed beside the median.
Algorithmic bytes: 4 V per row forward, 8 V per row backward, 12 V forward + backward.  One JSON object per case (microseconds, GB/s, bytes), one line each.
python tools/seam_xent_bench.py [--iters 20] [--reps 9] [--batches 8 16 32]"""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdvar_amd import engine as E          # noqa: E402
from sdvar_amd import seam                 # noqa: E402

STREAM_RATE = 6.3e12        # bytes / s: the HBM stream rate DESIGN.md section 4d measures against


def windows(fns, iters, reps):
    """{name: callable} -> {name: (median, min, max, host)} in microseconds per call; host = the median host-clock time to ENQUEUE one call (no synchronise inside the
    window): where it is close to the device time the row is bound by Python / autograd dispatch, not by the kernels."""
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
    print(title)
    for k, (med, lo, hi, host) in res.items():
        gbs = nbytes / med * 1e-3
        print(f"    {k:<64s} {med:9.1f} us  (min {lo:.1f}, max {hi:.1f}; host enqueue {host:.1f})  {gbs:7.0f} GB/s algorithmic  "
              f"({nbytes / (med * 1e-6) / STREAM_RATE:.2f} of 6.3 TB/s)")
        out[f"{title} | {k}"] = {"us": round(med, 2), "GBps": round(gbs, 1), "host_us": round(host, 2)}


def peak_above_resident(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def case(B, a, dev):
    V, L, eps = 4096, 680, 0.1
    rows = B * L
    gen = torch.Generator(device=dev).manual_seed(B)
    ncopy = a.copies or (512 * 2 ** 20) // (4 * rows * V) + 1
    leaves = [(torch.randn(rows, V, device=dev, generator=gen) * 3).requires_grad_() for _ in range(ncopy)]
    tg = torch.randint(0, V, (rows,), device=dev, generator=gen)
    g = torch.randn(rows, device=dev, generator=gen) / rows
    ring = itertools.cycle(range(ncopy))
    nxt = lambda: leaves[next(ring)]
    tloss = nn.CrossEntropyLoss(label_smoothing=eps, reduction="none")
    out = {"case": f"d16 256^2 B{B}", "rows": rows, "V": V, "label_smoothing": eps, "logits_copies": ncopy}

    # ---- agreement first (fp32 torch on the GPU is the other candidate, not the oracle: tests/test_gpu_seam_xent.py has fp64)
    x = leaves[0]
    sl, tl = seam.cross_entropy(x, tg, eps), tloss(x, tg)
    sg, = torch.autograd.grad(sl, x, g)
    tgr, = torch.autograd.grad(tl, x, g)
    print(f"B{B} rows {rows} V {V}: max |seam - torch fp32|: loss {(sl - tl).abs().max().item():.2e}, grad {(sg - tgr).abs().max().item():.2e} "
          f"(max |grad| {tgr.abs().max().item():.2e}); {ncopy} logits buffers in rotation")
    del sl, tl, sg, tgr

    sums = torch.zeros(4, dtype=torch.float64, device=dev)
    nll = torch.empty(B, L, device=dev)

    def torch_nograd():
        with torch.no_grad():
            return tloss(nxt(), tg)

    rf = windows({"engine.xent_train_fwd (loss + lse)": lambda: E.xent_train_fwd(nxt().detach(), tg, eps),
                  "seam.cross_entropy, no grad (loss only)": lambda: seam.cross_entropy(nxt().detach(), tg, eps),
                  "engine.xent_stats": lambda: E.xent_stats(nxt().detach().view(B, L, V), tg.view(B, L), 0, sums, nll_out=nll),
                  "seam.cross_entropy under grad": lambda: seam.cross_entropy(nxt(), tg, eps),
                  "torch CrossEntropyLoss under grad": lambda: tloss(nxt(), tg),
                  "torch CrossEntropyLoss, no grad": torch_nograd}, a.iters, a.reps)
    report("forward", rf, out, 4.0 * rows * V)

    lses = [E.xent_train_fwd(x.detach(), tg, eps)[1] for x in leaves]
    idx = itertools.cycle(range(ncopy))

    def c_bwd(nt):
        def f():
            i = next(idx)
            return E.xent_train_bwd(leaves[i].detach(), tg, lses[i], g, "none", None, eps, -100, nt_stores=nt)
        return f
    sgraph = [seam.cross_entropy(x, tg, eps) for x in leaves]
    tgraph = [tloss(x, tg) for x in leaves]

    def ag(graphs):
        def f():
            i = next(idx)
            return torch.autograd.grad(graphs[i], leaves[i], g, retain_graph=True)
        return f
    rb = windows({"engine.xent_train_bwd, plain stores": c_bwd(False), "engine.xent_train_bwd, non-temporal stores": c_bwd(True),
                  "seam.cross_entropy (autograd.grad)": ag(sgraph), "torch CrossEntropyLoss (autograd.grad)": ag(tgraph)}, a.iters, a.reps)
    report("backward", rb, out, 8.0 * rows * V)
    # the gradient's consumer reads it right away (the head GEMM's backward in a trainer; here one reduction over it): does the store flavour change what that pass costs?

    def c_bwd_read(nt):
        f = c_bwd(nt)
        return lambda: f().sum()
    rc = windows({"xent_train_bwd plain stores, then a pass reading dlogits": c_bwd_read(False),
                  "xent_train_bwd non-temporal stores, then a pass reading dlogits": c_bwd_read(True)}, a.iters, a.reps)
    report("backward + consumer", rc, out, 12.0 * rows * V)
    del sgraph, tgraph, lses

    def both(fn):
        def f():
            x = nxt()
            return torch.autograd.grad(fn(x, tg), x, g)
        return f
    seam_fn = lambda x, t: seam.cross_entropy(x, t, eps)
    rt = windows({"seam.cross_entropy": both(seam_fn), "torch CrossEntropyLoss": both(tloss)}, a.iters, a.reps)
    report("forward + backward (autograd)", rt, out, 12.0 * rows * V)
    out["peak_bytes_above_resident"] = {"seam.cross_entropy": peak_above_resident(both(seam_fn)), "torch CrossEntropyLoss": peak_above_resident(both(tloss))}
    print(f"    peak memory above the resident tensors, one forward + backward: seam {out['peak_bytes_above_resident']['seam.cross_entropy'] / 2 ** 20:.1f} MiB, "
          f"torch {out['peak_bytes_above_resident']['torch CrossEntropyLoss'] / 2 ** 20:.1f} MiB (the gradient itself is {4 * rows * V / 2 ** 20:.1f} MiB)")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 16, 32])
    ap.add_argument("--copies", type=int, default=0, help="logits buffers in rotation per case (0: enough to exceed 512 MiB)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seam_xent_bench: no GPU (there is nothing to time on a CPU)")
    dev = torch.device("cuda:0")
    E.load_library()
    lines = []
    for B in a.batches:
        lines.append(json.dumps(case(B, a, dev)))
        torch.cuda.empty_cache()
    for ln in lines:
        print(ln)


if __name__ == "__main__":
    main()
