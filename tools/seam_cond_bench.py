#!/usr/bin/env python3
"""Time seam.ada_lin (the conditioning linears Sequential(SiLU, Linear): one kernel forward, two backward, csrc/cond_train.hip) in ONE process on the same tensors against
  - torch:   nn.Sequential(nn.SiLU(), nn.Linear) itself, fp32 or under torch.autocast;
  - parent:  what linears=True did for this module before ada_lin existed - torch's SiLU into seam.linear_grad (fp32: the operator GEMMs of the default mode) or
             seam.linear_amp_grad (autocast), PER STEP: the weight-operand cache is dropped inside every timed call, which is what an optimizer step between calls does.

Shapes: the batch B = 8 and B = 32 at the d16 width (ada_lin 1024 -> 6144, head norm 1024 -> 2048) and the d30 width (1920 -> 11520, 1920 -> 3840), in fp32, fp16 and
bf16.  fp32 cond, fp32 master weight and bias, as the reference's trainer holds them.  Per shape and mode: the forward under grad, the backward alone (one
autograd.grad call on a retained graph: dcond, dW, db) and forward + backward through autograd, then the kernels alone through the C entry points on preallocated
buffers (no Python between the launches but the call itself).  The calls are a few microseconds long, so a window is --iters = 200 back-to-back calls.

The traffic floor: W (N K float32) is read once forward; backward it is read once and dW (N K float32) is written once - 4 N K and 8 N K bytes at the project's
6.3 TB/s stream rate.  "of floor" = floor / measured: the achieved fraction of that rate.  Peak memory of a forward + backward
(torch.cuda.max_memory_allocated above what was allocated before the call) for the three candidates.

seam.ada_lin is timed at every shape by a direct call.  install_cond's bound forward does not hand every one of them to it (seam.cond_serves: above 16 rows only up to
2^23 weights): a case it declines runs nn.Sequential.forward - the parent's path where linears=True is installed - and is marked "not served"; the closing lines list
the served cases that are not faster than the parent's path (there should be none) and, apart, what the direct call does at the declined ones.
W plus dW is at most 177 MB, less than the 256 MiB Infinity Cache: back-to-back calls of a window may find part of W there, so "of floor" is against a floor an
HBM-cold call cannot be assumed to meet.  Through autograd a call of this size is bound by the host (85 - 105 us for 25 - 65 us of kernels) and single windows
scatter by tens of microseconds: the "kernels" lines are the reliable ones.

Every figure is the MEDIAN over --reps windows, timed with device events; candidates alternate window by window.  The last line is one JSON object (microseconds, bytes).
python tools/seam_cond_bench.py [--iters 200] [--reps 9] [--batches 8,32]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdvar_amd import engine as E          # noqa: E402
from sdvar_amd import seam                 # noqa: E402

STREAM_BYTES_PER_US = 6.3e6                # 6.3 TB/s
SHAPES = [("d16 ada_lin", 1024, 6144), ("d16 head", 1024, 2048), ("d30 ada_lin", 1920, 11520), ("d30 head", 1920, 3840)]
MODES = [("fp32", None), ("fp16", torch.float16), ("bf16", torch.bfloat16)]


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
            f()
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in us.items()}


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batches", default="8,32")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seam_cond_bench: no GPU (there is nothing to time on a CPU)")
    dev, lib, results = torch.device("cuda:0"), E.load_library(), {}
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s, scale=1.0: torch.randn(*s, device=dev, generator=g) * scale
    seam.configure(gemm_mode=E.DEFAULT_GEMM_MODE)
    slower_than_torch, slower_than_parent, declined = [], [], {}

    for layer, K, N in SHAPES:
        seq = nn.Sequential(nn.SiLU(), nn.Linear(K, N)).to(dev)
        with torch.no_grad():
            seq[1].weight.copy_(rn(N, K, scale=1 / math.sqrt(K)))
            seq[1].bias.copy_(rn(N))
        W, b = seq[1].weight, seq[1].bias
        for B in [int(v) for v in a.batches.split(",")]:
            c = rn(B, K).requires_grad_()
            leaves = (c, W, b)
            floors = {"forward": 4.0 * N * K / STREAM_BYTES_PER_US, "backward": 8.0 * N * K / STREAM_BYTES_PER_US, "forward + backward": 12.0 * N * K / STREAM_BYTES_PER_US}
            for mname, half in MODES:
                tag = f"{layer} {K}->{N} B{B} {mname}"
                seam.clear_caches()

                def amp(fn, half=half):
                    if half is None:
                        return fn

                    def f():
                        with torch.autocast("cuda", dtype=half):
                            return fn()
                    return f

                def parent():
                    seam._WEIGHT_PLANES.clear()          # per step: an optimizer step has moved the weight on
                    s = torch.nn.functional.silu(c)
                    return seam.linear_grad(s, W, b) if half is None else seam.linear_amp_grad(s, W, b)
                dy = rn(B, N, scale=1e-4) if half is None else rn(B, N).to(half)
                cands = {"seam": amp(lambda: seam.ada_lin(c, W, b)), "torch": amp(lambda: seq(c)), "parent": amp(parent)}
                grads = {k: torch.autograd.grad(f(), leaves, dy) for k, f in cands.items()}
                rel = {k: max(((s_ - t_).abs().max() / t_.abs().max()).item() for s_, t_ in zip(grads[k], grads["torch"])) for k in ("seam", "parent")}
                rf = windows(cands, a.iters, a.reps)
                outs = {k: f() for k, f in cands.items()}
                rb = windows({k: (lambda o=o: torch.autograd.grad(o, leaves, dy, retain_graph=True)) for k, o in outs.items()}, a.iters, a.reps)
                del outs
                rt = windows({k: (lambda f=f: torch.autograd.grad(f(), leaves, dy)) for k, f in cands.items()}, a.iters, a.reps)
                mem = {k: peak_bytes(lambda f=f: torch.autograd.grad(f(), leaves, dy)) for k, f in cands.items()}
                served = seam.cond_serves(B, N, K)
                print(f"{tag}{'' if served else '  [NOT SERVED by install_cond: the direct call]'}: max |x - torch| / max|torch| over the gradients: seam {rel['seam']:.1e}, "
                      f"parent {rel['parent']:.1e}")
                for leg, r in (("forward", rf), ("backward", rb), ("forward + backward", rt)):
                    s_, t_, p_ = r["seam"], r["torch"], r["parent"]
                    print(f"    {leg:<20s} seam {s_[0]:7.1f} us (min {s_[1]:.1f}, max {s_[2]:.1f})   torch {t_[0]:7.1f} us (min {t_[1]:.1f}, max {t_[2]:.1f})   "
                          f"parent, per step {p_[0]:7.1f} us (min {p_[1]:.1f}, max {p_[2]:.1f})   seam / torch {s_[0] / t_[0]:5.2f}   seam / parent {s_[0] / p_[0]:5.2f}   "
                          f"floor {floors[leg]:5.1f} us: seam at {floors[leg] / s_[0] * 100:4.1f} % of 6.3 TB/s")
                    results[f"{tag} | {leg}"] = {"seam": round(s_[0], 1), "torch": round(t_[0], 1), "parent_per_step": round(p_[0], 1), "floor": round(floors[leg], 1)}
                    if s_[0] > t_[0]:
                        slower_than_torch.append(f"{tag} | {leg}")
                    if leg == "forward + backward":
                        if not served:
                            declined[tag] = round(s_[0] / p_[0], 2)
                        elif s_[0] >= p_[0]:
                            slower_than_parent.append(tag)
                print(f"    peak memory, forward + backward: seam {mem['seam'] / 2**20:.1f} MiB, torch {mem['torch'] / 2**20:.1f} MiB, parent {mem['parent'] / 2**20:.1f} MiB")
                results[f"{tag} | peak_bytes"] = mem
                results[f"{tag} | served"] = served

                # ---- the kernels alone, through the C entry points on preallocated buffers
                st, code = E._stream(), 0 if half is None else seam._HALF_DTYPES[half]
                od = torch.float32 if half is None else half
                cd, Wd, bd = c.detach(), W.detach(), b.detach()
                y, dc, dW, db = torch.empty(B, N, dtype=od, device=dev), torch.empty(B, K, device=dev), torch.empty(N, K, device=dev), torch.empty(N, device=dev)
                ws = torch.empty(E.cond_lin_bwd_ws_bytes(B, N, K) // 4, device=dev)
                kern = {"forward": lambda: E._check(lib.sdvar_op_cond_lin_fwd(P(cd), 0, K, P(Wd), 0, P(bd), P(y), code, B, N, K, st)),
                        "backward": lambda: E._check(lib.sdvar_op_cond_lin_bwd(P(dy), P(cd), 0, K, P(Wd), 0, P(dc), P(dW), P(db), P(ws), code, B, N, K, st)),
                        "backward, dW and db only": lambda: E._check(lib.sdvar_op_cond_lin_bwd(P(dy), P(cd), 0, K, P(Wd), 0, None, P(dW), P(db), None, code, B, N, K, st))}
                rk = windows(kern, a.iters, a.reps)
                kfloor = {"forward": floors["forward"], "backward": floors["backward"], "backward, dW and db only": 4.0 * N * K / STREAM_BYTES_PER_US}
                for k, r in rk.items():
                    print(f"    kernels, {k:<26s} {r[0]:7.1f} us (min {r[1]:.1f}, max {r[2]:.1f})   floor {kfloor[k]:5.1f} us: {kfloor[k] / r[0] * 100:4.1f} % of 6.3 TB/s")
                results[f"{tag} | kernels"] = {k: round(r[0], 1) for k, r in rk.items()}
                del grads, y, dc, dW, db, ws
    print("served by install_cond and forward + backward not faster than the parent's path: " + (", ".join(slower_than_parent) or "nowhere"))
    print("not served by install_cond (direct call, forward + backward, seam / parent): " + (", ".join(f"{k} {v:.2f}" for k, v in declined.items()) or "none"))
    print("legs on which torch is faster: " + (", ".join(slower_than_torch) or "none"))
    results["slower_than_parent"], results["slower_than_torch"], results["declined"] = slower_than_parent, slower_than_torch, declined
    seam.clear_caches()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
