#!/usr/bin/env python3
"""Time seam.fused_mlp_func_grad (the forward's GEMMs, the operand producers of csrc/mlp_bwd.hip and the four backward GEMMs) against torch's own fp32
fc2(gelu_tanh(fc1(x))) under autograd, in ONE process on the same tensors.

Shape: the FFN of d16 under teacher forcing - M = 8 * 680 rows, C = 1024, hidden = 4096.  Per GEMM mode of the seam (engine.GEMM_MODES) and for torch: the inference
forward (seam.fused_mlp_func; torch under no_grad), the forward under grad (fc1 with the bias epilogue + the GELU operand kernel), the backward alone (one
autograd.grad call on a retained graph, all five gradients), forward + backward.  The backward's two halves are then timed apart on preallocated buffers, through the C
entry points: the producers (dy split, dy^T, x^T, GELU backward, column sums, scale kernels) and the four GEMMs; their sum misses only autograd's dispatch and the
allocations.  The GELU operand kernel alone is the price of keeping the nine GEMM kernels untouched in the forward under grad.

Every figure is the MEDIAN over --reps windows of --iters back-to-back calls, timed with device events; the candidates alternate window by window, so drift of the
machine hits them alike.  min / max of the windows are printed beside the median.  Algorithmic work: 4 M C hidden FLOP forward (two GEMMs), 8 M C hidden backward (four).
The last line is one JSON object (microseconds).
python tools/seam_mlp_grad_bench.py [--iters 5] [--reps 9] [--rows 5440]"""
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
        tf = f"{flops / med * 1e-6:7.1f} TFLOP/s (algorithmic)" if flops else ""
        print(f"    {k:<28s} {med:9.1f} us  (min {lo:.1f}, max {hi:.1f})  {tf}")
        results[f"{title} | {k}"] = round(med, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rows", type=int, default=8 * 680)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seam_mlp_grad_bench: no GPU (there is nothing to time on a CPU)")
    dev, lib, results = torch.device("cuda:0"), E.load_library(), {}
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    g = torch.Generator(device=dev).manual_seed(0)
    M, Cw, hid = a.rows, 1024, 4096
    Mp = seam._pad32(M)
    rn = lambda *s, scale=1.0: torch.randn(*s, device=dev, generator=g) * scale
    x, dy = rn(1, M, Cw).requires_grad_(), rn(1, M, Cw, scale=1e-4)
    W1, b1 = rn(hid, Cw, scale=1 / math.sqrt(Cw)).requires_grad_(), rn(hid).requires_grad_()
    W2, b2 = rn(Cw, hid, scale=1 / math.sqrt(hid)).requires_grad_(), rn(Cw).requires_grad_()
    leaves = (x, W1, b1, W2, b2)
    fl = 4.0 * M * Cw * hid

    def torch_fwd():
        return F.linear(F.gelu(F.linear(x, W1, b1), approximate="tanh"), W2, b2)

    def seam_fwd():
        return seam.fused_mlp_func_grad(x, W1, W2, b1, b2)

    def infer(fn):
        def f():
            with torch.no_grad():
                return fn()
        return f

    tg = torch.autograd.grad(torch_fwd(), leaves, dy)
    for mode in E.GEMM_MODES:
        seam.configure(gemm_mode=mode)
        seam.clear_caches()
        sg = torch.autograd.grad(seam_fwd(), leaves, dy)
        rel = [((s_ - t_).abs().max() / t_.abs().max()).item() for s_, t_ in zip(sg, tg)]
        print(f"mode {mode}, M {M} C {Cw} hidden {hid}: max |seam - torch fp32| / max|torch| for dx, dW1, db1, dW2, db2: " + ", ".join(f"{r:.1e}" for r in rel))
        rf = windows({"seam": infer(lambda: seam.fused_mlp_func(x.detach(), W1.detach(), W2.detach(), b1.detach(), b2.detach())), "torch fp32": infer(torch_fwd)}, a.iters, a.reps)
        report(f"{mode}: forward, inference", rf, results, fl)
        rg = windows({"seam": seam_fwd, "torch fp32": torch_fwd}, a.iters, a.reps)
        report(f"{mode}: forward under grad", rg, results, fl)
        so, to = seam_fwd(), torch_fwd()
        rb = windows({"seam": lambda: torch.autograd.grad(so, leaves, dy, retain_graph=True), "torch fp32": lambda: torch.autograd.grad(to, leaves, dy, retain_graph=True)},
                     a.iters, a.reps)
        report(f"{mode}: backward (autograd.grad, five gradients)", rb, results, 2 * fl)
        rt = windows({"seam": lambda: torch.autograd.grad(seam_fwd(), leaves, dy), "torch fp32": lambda: torch.autograd.grad(torch_fwd(), leaves, dy)}, a.iters, a.reps)
        report(f"{mode}: forward + backward", rt, results, 3 * fl)
        del so, to

        # ---- the backward's two halves on preallocated buffers
        fmt, npl, h16 = seam._OPERAND_FORMAT[mode], seam._OPERAND_PLANES[mode], mode == "f16x2"
        el = torch.float32 if mode == "f32" else torch.int16
        op = lambda n: torch.empty(npl, n, dtype=el, device=dev)
        f32 = lambda *s: torch.empty(*s, device=dev)
        xr, dyr = x.detach().view(M, Cw), dy.view(M, Cw)
        pre, dh = rn(M, hid), rn(M, hid, scale=1e-4)
        w2t, s2 = seam._weight_planes_t(W2, mode)
        w1t, s1 = seam._weight_planes_t(W1, mode)
        sdy, sdp = (torch.zeros(4, device=dev), torch.zeros(4, device=dev)) if h16 else (None, None)
        dyo, dyt, xt, dpre, dpre_t, h_t, hp = (dyr if mode == "f32" else op(M * Cw)), op(Cw * Mp), op(Cw * Mp), op(M * hid), op(hid * Mp), op(hid * Mp), op(M * hid)
        part, db1, db2, dx, dw1, dw2 = f32(Mp // 32, hid), f32(hid), f32(Cw), f32(M, Cw), f32(hid, Cw), f32(Cw, hid)
        off = lambda sc, n: None if sc is None else C.c_void_p(sc.data_ptr() + 4 * n)

        def producers():
            st = E._stream()
            E._check(lib.sdvar_op_colsum(P(dyr), Cw, M, Cw, P(db2), st))
            if h16:
                E._check(lib.sdvar_op_split_planes_f16(P(dyr), P(dyo), M, Cw, M * Cw, P(sdy), st))
                E._check(lib.sdvar_op_scale_pair(None, 0, P(sdy), 0, P(s2), st))
                E._check(lib.sdvar_op_scale_pair(P(dh), M * hid, P(sdp), 1, P(s1), st))
            elif mode != "f32":
                E._check(lib.sdvar_op_split_planes(P(dyr), P(dyo), M, Cw, M * Cw, st))
            E._check(lib.sdvar_op_gelu_bwd(P(dh), P(pre), M, hid, fmt, int(h16), P(sdp), P(dpre), M * hid, P(dpre_t), hid * Mp, P(h_t), hid * Mp, P(part), st))
            E._check(lib.sdvar_op_transpose_operand(P(dyr), Cw, M, Cw, fmt, P(dyt), Cw * Mp, P(sdy), st))
            E._check(lib.sdvar_op_transpose_operand(P(xr), Cw, M, Cw, fmt, P(xt), Cw * Mp, None, st))
            E._check(lib.sdvar_op_colsum(P(part), hid, Mp // 32, hid, P(db1), st))

        def gemms():
            seam._gemm_nt(mode, dyo, w2t, off(sdy, 2), dh, M, hid, Cw)
            seam._gemm_nt(mode, dpre, w1t, off(sdp, 2), dx, M, Cw, hid)
            seam._gemm_nt(mode, dyt, h_t, off(sdy, 0), dw2, Cw, hid, Mp)
            seam._gemm_nt(mode, dpre_t, xt, off(sdp, 0), dw1, hid, Cw, Mp)

        def gelu_operand():
            E._check(lib.sdvar_op_gelu_operand(P(pre), M, hid, fmt, int(h16), P(hp), M * hid, E._stream()))
        producers()
        rp = windows({"producers": producers, "four GEMMs": gemms, "GELU operand (forward)": gelu_operand}, a.iters, a.reps)
        report(f"{mode}: backward, halves through the C entry points", rp, results, 0)
        share = rp["producers"][0] / (rp["producers"][0] + rp["four GEMMs"][0])
        print(f"    producers' share of producers + GEMMs: {share * 100:.1f} %;  backward / forward-under-grad time: {rb['seam'][0] / rg['seam'][0]:.2f} (algorithmic: 2)")
        results[f"{mode}: producer_share"] = round(share, 4)
        del w2t, w1t, dyo, dyt, xt, dpre, dpre_t, h_t, hp, pre, dh
    seam.configure(gemm_mode=E.DEFAULT_GEMM_MODE)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
