#!/usr/bin/env python3
"""Time seam.teacher_embed (the prologue of a teacher-forced training step: one kernel forward; one pass over the gradient plus three small launches backward,
csrc/embed_train.hip) in ONE process on the same tensors against
  - torch:   the prologue as eager torch ops (var.py:225-243: rand, <, where, the class_emb gather, expand + pos_start, word_embed, cat, the lvl_embed gather, + pos_1LC in
             place, the new_ones / matmul dtype probe, .to(main_type)), fp32 or under torch.autocast with the reference's autocast(enabled=False) around the embedding;
  - parent:  the same ops with word_embed through seam.linear_grad - what linears=True did for this prologue before teacher_embed existed - PER STEP: the weight-operand
             cache is dropped inside every timed call, which is what an optimizer step between calls does - and, next to it, with the cache left warm (no step between
             the calls: the operand passes over the weight are not charged), so that the comparison cannot be read as inflated.

Shapes: B = 8 and 32, L = 680 (the 256-pixel ladder), K = 32, C = 1024 (d16) and 1920 (d30), x_BLC leaving in fp32 and in fp16 / bf16.  fp32 features and master
parameters, as the reference's trainer holds them.  Per shape and dtype: the forward under grad, the backward alone (one autograd.grad call on a retained graph: the six
parameter gradients from the gradients of x_BLC and cond_BD), forward + backward through autograd, the peak memory of a forward + backward and the launches per
direction (torch.profiler's kernel events; "n/a" where the profiler gives none), then the kernels alone through the C entry points on preallocated buffers.

The traffic floor: x_BLC (B L C values of the output dtype) is written once forward and its gradient read once backward - at the project's 6.3 TB/s stream rate.
"of floor" = floor / measured.  Parameters, features and the parameter gradients (L C + C K + ... floats) are left out of the floor: at B = 8 they are a third of it,
so the share there is against a floor the call cannot meet.  The buffers of a window (at most 167 MB) fit the 256 MiB Infinity Cache: back-to-back calls may find part
of them there.

Every figure is the MEDIAN over --reps windows, timed with device events; candidates alternate window by window.  The last line is one JSON object (microseconds, bytes).
python tools/seam_embed_bench.py [--iters 50] [--reps 7] [--batches 8,32]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdvar_amd import engine as E          # noqa: E402
from sdvar_amd import seam                 # noqa: E402
from sdvar_amd.ladder import LADDER_256    # noqa: E402

STREAM_BYTES_PER_US = 6.3e6                # 6.3 TB/s
WIDTHS = [("d16", 1024), ("d30", 1920)]
MODES = [("fp32", None), ("fp16", torch.float16), ("bf16", torch.bfloat16)]
K, NUM_CLASSES, RATE = 32, 1000, 0.1


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


def launches(fn):
    """Kernel launches of one call, from torch.profiler; None where it records no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower())
        return n or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", default="8,32")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seam_embed_bench: no GPU (there is nothing to time on a CPU)")
    dev, lib, results = torch.device("cuda:0"), E.load_library(), {}
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s, scale=1.0: torch.randn(*s, device=dev, generator=g) * scale
    seam.configure(gemm_mode=E.DEFAULT_GEMM_MODE)
    pns = tuple(LADDER_256)
    sizes = [p * p for p in pns]
    first_l, L, S, NC1 = sizes[0], sum(sizes), len(pns), NUM_CLASSES + 1
    lvl = torch.cat([torch.full((n,), i, dtype=torch.int64) for i, n in enumerate(sizes)]).view(1, L).to(dev)
    slower_than_torch, slower_than_parent = [], []

    for wname, Cw in WIDTHS:
        leaves = [rn(NC1, Cw, scale=0.02).requires_grad_(), rn(1, first_l, Cw, scale=0.02).requires_grad_(), rn(Cw, K, scale=1 / math.sqrt(K)).requires_grad_(),
                  rn(Cw, scale=0.02).requires_grad_(), rn(S, Cw, scale=0.02).requires_grad_(), rn(1, L, Cw, scale=0.02).requires_grad_()]
        cls, ps, W, b, le, pos = leaves
        for B in [int(v) for v in a.batches.split(",")]:
            label = torch.randint(0, NUM_CLASSES, (B,), device=dev, generator=g)
            xv = rn(B, L - first_l, K)
            for mname, half in MODES:
                tag = f"{wname} C{Cw} B{B} {mname}"
                od = torch.float32 if half is None else half
                el = 4 if half is None else 2
                seam.clear_caches()

                def eager(linear, half=half, od=od):
                    def f():
                        with torch.autocast("cuda", dtype=half or torch.bfloat16, enabled=half is not None):
                            with torch.autocast("cuda", enabled=False):
                                lab = torch.where(torch.rand(B, device=dev) < RATE, NUM_CLASSES, label)
                                sos = cond = cls[lab]
                                sos = sos.unsqueeze(1).expand(B, first_l, -1) + ps.expand(B, first_l, -1)
                                x = torch.cat((sos, linear(xv.float())), dim=1)
                                x += le[lvl[:, :L].expand(B, -1)] + pos[:, :L]
                            t = x.new_ones(8, 8)
                            main = torch.matmul(t, t).dtype
                            return x.to(dtype=main), cond
                    return f

                def parent_linear(t):
                    seam._WEIGHT_PLANES.clear()          # per step: an optimizer step has moved the weight on
                    return seam.linear_grad(t, W, b)

                def ours(od=od):
                    r = torch.rand(B, device=dev)
                    return seam.teacher_embed(label, xv, cls, ps, W, b, le, pos, lvl, tokens=L, drop=(r, RATE), out_dtype=od)

                cands = {"seam": ours, "torch": eager(lambda t: torch.nn.functional.linear(t, W, b)), "parent": eager(parent_linear),
                         "parent_cached": eager(lambda t: seam.linear_grad(t, W, b))}          # the weight-operand cache left warm: no optimizer step between the calls
                gx, gc = (rn(B, L, Cw, scale=1e-3)).to(od), rn(B, Cw, scale=1e-3)
                bwd = lambda out: torch.autograd.grad(out, leaves, (gx, gc), retain_graph=True)
                rf = windows(cands, a.iters, a.reps)
                outs = {k: f() for k, f in cands.items()}
                rb = windows({k: (lambda o=o: bwd(o)) for k, o in outs.items()}, a.iters, a.reps)
                nb = {k: launches(lambda o=o: bwd(o)) for k, o in outs.items()}
                del outs
                rt = windows({k: (lambda f=f: torch.autograd.grad(f(), leaves, (gx, gc))) for k, f in cands.items()}, a.iters, a.reps)
                mem = {k: peak_bytes(lambda f=f: torch.autograd.grad(f(), leaves, (gx, gc))) for k, f in cands.items()}
                nf = {k: launches(f) for k, f in cands.items()}
                floor1 = B * L * Cw * el / STREAM_BYTES_PER_US
                floors = {"forward": floor1, "backward": floor1, "forward + backward": 2 * floor1}
                print(tag)
                for leg, r in (("forward", rf), ("backward", rb), ("forward + backward", rt)):
                    s_, t_, p_, pc = r["seam"], r["torch"], r["parent"], r["parent_cached"]
                    print(f"    {leg:<20s} seam {s_[0]:7.1f} us (min {s_[1]:.1f}, max {s_[2]:.1f})   torch {t_[0]:7.1f} us (min {t_[1]:.1f}, max {t_[2]:.1f})   "
                          f"parent, per step {p_[0]:7.1f} us (min {p_[1]:.1f}, max {p_[2]:.1f}), cache warm {pc[0]:7.1f} us   seam / torch {s_[0] / t_[0]:5.2f}   seam / parent {s_[0] / p_[0]:5.2f}   "
                          f"floor {floors[leg]:5.1f} us: seam at {floors[leg] / s_[0] * 100:4.1f} % of 6.3 TB/s")
                    results[f"{tag} | {leg}"] = {"seam": round(s_[0], 1), "torch": round(t_[0], 1), "parent_per_step": round(p_[0], 1), "parent_cache_warm": round(pc[0], 1), "floor": round(floors[leg], 1)}
                    if s_[0] > t_[0]:
                        slower_than_torch.append(f"{tag} | {leg}")
                    if s_[0] >= min(p_[0], pc[0]):
                        slower_than_parent.append(f"{tag} | {leg}")
                print(f"    peak memory, forward + backward: seam {mem['seam'] / 2**20:.1f} MiB, torch {mem['torch'] / 2**20:.1f} MiB, parent {mem['parent'] / 2**20:.1f} MiB")
                fmt = lambda d: ", ".join(f"{k} {'n/a' if v is None else v}" for k, v in d.items())
                print(f"    launches (the draw of r included), forward: {fmt(nf)};   backward: {fmt(nb)}")
                results[f"{tag} | peak_bytes"], results[f"{tag} | launches"] = mem, {"forward": nf, "backward": nb}

                # ---- the kernels alone, through the C entry points on preallocated buffers
                st, code = E._stream(), E.TRAIN_DTYPES[od]
                d = [t.detach() for t in leaves]
                r = torch.rand(B, device=dev)
                x, cond = torch.empty(B, L, Cw, dtype=od, device=dev), torch.empty(B, Cw, device=dev)
                dcls, dps, dW, db, dl, dpos = (torch.empty_like(t) for t in d)
                ws = torch.empty(E.embed_bwd_ws_bytes(B, L, Cw, K) // 4, device=dev)
                xbs, xrs = xv.stride(0), xv.stride(1)
                kern = {"forward": lambda: E._check(lib.sdvar_op_embed_fwd(P(label), 1, P(r), RATE, P(lvl), P(xv), xbs, xrs, P(d[0]), P(d[1]), P(d[2]), P(d[3]), P(d[4]), P(d[5]), P(x),
                                                                           code, P(cond), B, L, L, first_l, Cw, K, S, NC1, st)),
                        "backward": lambda: E._check(lib.sdvar_op_embed_bwd(P(gx), code, P(gc), P(label), 1, P(r), RATE, P(lvl), P(xv), xbs, xrs, P(d[2]), P(dpos), P(dps), P(dl),
                                                                            P(dcls), P(db), P(dW), None, 0, P(ws), B, L, L, first_l, Cw, K, S, NC1, st)),
                        "backward, dW only": lambda: E._check(lib.sdvar_op_embed_bwd(P(gx), code, None, None, 1, None, RATE, P(lvl), P(xv), xbs, xrs, P(d[2]), None, None, None, None,
                                                                                     None, P(dW), None, 0, P(ws), B, L, L, first_l, Cw, K, S, NC1, st)),
                        "backward, dclass only": lambda: E._check(lib.sdvar_op_embed_bwd(P(gx), code, P(gc), P(label), 1, P(r), RATE, P(lvl), P(xv), xbs, xrs, P(d[2]), None, None, None,
                                                                                         P(dcls), None, None, None, 0, P(ws), B, L, L, first_l, Cw, K, S, NC1, st)),
                        "backward, dpos_1LC only": lambda: E._check(lib.sdvar_op_embed_bwd(P(gx), code, None, None, 1, None, RATE, P(lvl), P(xv), xbs, xrs, P(d[2]), P(dpos), None, None,
                                                                                           None, None, None, None, 0, P(ws), B, L, L, first_l, Cw, K, S, NC1, st))}
                rk = windows(kern, a.iters, a.reps)
                for k, v in rk.items():
                    print(f"    kernels, {k:<26s} {v[0]:7.1f} us (min {v[1]:.1f}, max {v[2]:.1f})   floor {floor1:5.1f} us: {floor1 / v[0] * 100:4.1f} % of 6.3 TB/s")
                results[f"{tag} | kernels"] = {k: round(v[0], 1) for k, v in rk.items()}
                del x, cond, dcls, dps, dW, db, dl, dpos, ws
    print("legs not faster than the parent's path: " + (", ".join(slower_than_parent) or "none"))
    print("legs on which torch is faster: " + (", ".join(slower_than_torch) or "none"))
    results["slower_than_parent"], results["slower_than_torch"] = slower_than_parent, slower_than_torch
    seam.clear_caches()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
