#!/usr/bin/env python3
"""Time seam.fused_mlp_func_amp / fused_mlp_func_amp_grad (the half GEMM of csrc/gemm_half.hip and the producers of csrc/mlp_half.hip) in ONE process on the same
tensors against (a) torch's own fc2(gelu_tanh(fc1(x))) under torch.autocast - its half GEMMs - and (b) seam.fused_mlp_func_grad in mode f16x2, the fp32-grade route
install_train_amp(ffn=True) takes.

Shape: the FFN of d16 under teacher forcing - M = 8 * 680 rows, C = 1024, hidden = 4096 - with fp32 x, fp32 master weights and biases, as the reference's trainer holds
them; fp16 and bf16.  Per dtype: the inference forward (no_grad), the forward under grad, the backward alone (one autograd.grad call on a retained graph, all five
gradients) and forward + backward.  The backward's halves are then timed apart on preallocated buffers through the C entry points: the producers (dy, dy^T + db2's
partials, x^T, GELU backward, the two column sums), each of the four GEMMs, and the forward's x operand pass and two GEMMs.

Weights: the seam caches the half operands of W1 and W2 (as stored for the forward, transposed for the backward) until the weight is updated in place, so calls on
UNCHANGED weights (inference, gradient accumulation) skip those four passes, while a training loop with one optimizer step per forward + backward pays all four every
step.  torch's autocast casts its weights on every call here (leaving the autocast context clears its cast cache).  Both are timed: "seam half" reuses the cached
operands, "seam half, per step" drops the cache inside every timed call (what an optimizer step between calls does), and the four weight passes are timed alone.

Every figure is the MEDIAN over --reps windows of --iters back-to-back calls, timed with device events; the candidates alternate window by window, so drift of the
machine hits them alike.  min / max of the windows are printed beside the median.  Algorithmic work: 4 M C hidden FLOP forward, 8 M C hidden backward.
The last line is one JSON object (microseconds).
python tools/seam_mlp_amp_bench.py [--iters 5] [--reps 9] [--rows 5440]"""
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
            f()                 # untimed: a candidate that reuses cached weight operands finds them rebuilt after a window of one that drops them
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
        fl = flops.get(k, 0) if isinstance(flops, dict) else flops
        tf = f"{fl / med * 1e-6:7.1f} TFLOP/s (algorithmic)" if fl else ""
        print(f"    {k:<34s} {med:9.1f} us  (min {lo:.1f}, max {hi:.1f})  {tf}")
        results[f"{title} | {k}"] = round(med, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rows", type=int, default=8 * 680)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seam_mlp_amp_bench: no GPU (there is nothing to time on a CPU)")
    dev, lib, results = torch.device("cuda:0"), E.load_library(), {}
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    g = torch.Generator(device=dev).manual_seed(0)
    M, Cw, hid = a.rows, 1024, 4096
    Mp = seam._pad32(M)
    rn = lambda *s, scale=1.0: torch.randn(*s, device=dev, generator=g) * scale
    x = rn(1, M, Cw).requires_grad_()
    W1, b1 = rn(hid, Cw, scale=1 / math.sqrt(Cw)).requires_grad_(), rn(hid).requires_grad_()
    W2, b2 = rn(Cw, hid, scale=1 / math.sqrt(hid)).requires_grad_(), rn(Cw).requires_grad_()
    leaves = (x, W1, b1, W2, b2)
    fl = 4.0 * M * Cw * hid
    seam.configure(gemm_mode="f16x2")

    def infer(fn):
        def f():
            with torch.no_grad():
                return fn()
        return f

    for dtype in (torch.float16, torch.bfloat16):
        name, dt = str(dtype)[6:], seam._HALF_DTYPES[dtype]
        seam.clear_caches()
        dy, dy32 = rn(1, M, Cw).to(dtype), rn(1, M, Cw, scale=1e-4)

        def amp(fn):
            def f():
                with torch.autocast("cuda", dtype=dtype):
                    return fn()
            return f
        torch_fwd = amp(lambda: F.linear(F.gelu(F.linear(x, W1, b1), approximate="tanh"), W2, b2))
        seam_fwd = amp(lambda: seam.fused_mlp_func_amp_grad(x, W1, W2, b1, b2))
        f16x2_fwd = lambda: seam.fused_mlp_func_grad(x, W1, W2, b1, b2)
        tg = torch.autograd.grad(torch_fwd(), leaves, dy)
        sg = torch.autograd.grad(seam_fwd(), leaves, dy)
        rel = [((s_ - t_).abs().max() / t_.abs().max()).item() for s_, t_ in zip(sg, tg)]
        print(f"{name}, M {M} C {Cw} hidden {hid}: max |seam - torch autocast| / max|torch| for dx, dW1, db1, dW2, db2: " + ", ".join(f"{r:.1e}" for r in rel))
        cands = lambda s, t, f: {"seam half": s, "torch autocast": t, "seam f16x2 (fp32 operands)": f}

        def per_step(fn):           # the weights moved on since the last call: every cached operand is rebuilt inside the timed call
            def f():
                seam._WEIGHT_PLANES.clear()
                return fn()
            return f
        rf = windows(cands(infer(seam_fwd), infer(torch_fwd), infer(f16x2_fwd)), a.iters, a.reps)
        report(f"{name}: forward, inference", rf, results, fl)
        rg = windows({**cands(seam_fwd, torch_fwd, f16x2_fwd), "seam half, per step": per_step(seam_fwd)}, a.iters, a.reps)
        report(f"{name}: forward under grad", rg, results, fl)
        so, to, fo = seam_fwd(), torch_fwd(), f16x2_fwd()
        rb = windows({**cands(lambda: torch.autograd.grad(so, leaves, dy, retain_graph=True), lambda: torch.autograd.grad(to, leaves, dy, retain_graph=True),
                              lambda: torch.autograd.grad(fo, leaves, dy32, retain_graph=True)),
                      "seam half, per step": per_step(lambda: torch.autograd.grad(so, leaves, dy, retain_graph=True))}, a.iters, a.reps)
        report(f"{name}: backward (autograd.grad, five gradients)", rb, results, 2 * fl)
        rt = windows({**cands(lambda: torch.autograd.grad(seam_fwd(), leaves, dy), lambda: torch.autograd.grad(torch_fwd(), leaves, dy),
                              lambda: torch.autograd.grad(f16x2_fwd(), leaves, dy32)),
                      "seam half, per step": per_step(lambda: torch.autograd.grad(seam_fwd(), leaves, dy)),
                      "seam f16x2, per step": per_step(lambda: torch.autograd.grad(f16x2_fwd(), leaves, dy32))}, a.iters, a.reps)
        report(f"{name}: forward + backward", rt, results, 3 * fl)
        del so, to, fo

        # ---- the pieces on preallocated buffers, through the C entry points
        op = lambda n: torch.empty(n, dtype=torch.int16, device=dev)
        f32 = lambda *s: torch.empty(*s, device=dev)
        xr, dyr = x.detach().view(M, Cw), dy.view(M, Cw)
        p, dh = rn(M, hid).to(dtype), rn(M, hid)
        w1n, w2n = seam._weight_operand_h(W1, dtype, False), seam._weight_operand_h(W2, dtype, False)
        w1t, w2t = seam._weight_operand_h(W1, dtype, True), seam._weight_operand_h(W2, dtype, True)
        xo, ho, dyo, dyt, xt, dpre, dpre_t, h_t = op(M * Cw), op(M * hid), op(M * Cw), op(Cw * Mp), op(Cw * Mp), op(M * hid), op(hid * Mp), op(hid * Mp)
        part1, part2, db1, db2 = f32(Mp // 32, hid), f32(Mp // 32, Cw), f32(hid), f32(Cw)
        dx, dw1, dw2, y, pbuf = f32(M, Cw), f32(hid, Cw), f32(Cw, hid), torch.empty(M, Cw, dtype=dtype, device=dev), torch.empty(M, hid, dtype=dtype, device=dev)
        b1d, b2d = b1.detach(), b2.detach()

        def producers():
            st = E._stream()
            E._check(lib.sdvar_op_half_operand(P(dyr), dt, Cw, M, Cw, dt, 1, P(dyt), P(part2), st))
            E._check(lib.sdvar_op_colsum(P(part2), Cw, Mp // 32, Cw, P(db2), st))
            E._check(lib.sdvar_op_half_operand(P(dyr), dt, Cw, M, Cw, dt, 0, P(dyo), None, st))
            E._check(lib.sdvar_op_gelu_bwd_h(P(dh), P(p), M, hid, dt, P(dpre), P(dpre_t), P(h_t), P(part1), st))
            E._check(lib.sdvar_op_half_operand(P(xr), 0, Cw, M, Cw, dt, 1, P(xt), None, st))
            E._check(lib.sdvar_op_colsum(P(part1), hid, Mp // 32, hid, P(db1), st))

        def gelu_bwd():
            E._check(lib.sdvar_op_gelu_bwd_h(P(dh), P(p), M, hid, dt, P(dpre), P(dpre_t), P(h_t), P(part1), E._stream()))

        def x_operand():
            E._check(lib.sdvar_op_half_operand(P(xr), 0, Cw, M, Cw, dt, 0, P(xo), None, E._stream()))

        def fc1(keep):
            return lambda: E._check(lib.sdvar_op_gemm_h(P(xo), P(w1n), dt, P(b1d), None, 0, 0, P(ho), P(pbuf) if keep else None, M, hid, Cw, 1, E._stream()))

        def fc2():
            E._check(lib.sdvar_op_gemm_h(P(ho), P(w2n), dt, P(b2d), P(y), dt, Cw, None, None, M, Cw, hid, 0, E._stream()))
        W1d, W2d, wbuf = W1.detach(), W2.detach(), op(hid * Cw)

        def wpass(w, tr):
            return lambda: E._check(lib.sdvar_op_half_operand(P(w), 0, w.shape[1], w.shape[0], w.shape[1], dt, tr, P(wbuf), None, E._stream()))
        wpasses = {"W1 operand (forward)": wpass(W1d, 0), "W2 operand (forward)": wpass(W2d, 0), "W1^T operand (backward)": wpass(W1d, 1), "W2^T operand (backward)": wpass(W2d, 1)}
        gemm = {"dh = dy W2": lambda: seam._gemm_h(dtype, dyo, w2t, None, dh, M, hid, Cw), "dx = dpre W1": lambda: seam._gemm_h(dtype, dpre, w1t, None, dx, M, Cw, hid),
                "dW2 = dy^T h": lambda: seam._gemm_h(dtype, dyt, h_t, None, dw2, Cw, hid, Mp), "dW1 = dpre^T x": lambda: seam._gemm_h(dtype, dpre_t, xt, None, dw1, hid, Cw, Mp)}
        x_operand()
        fc1(True)()
        producers()
        one = 2.0 * M * Cw * hid
        rp = windows({"producers (all six launches)": producers, "GELU backward alone": gelu_bwd, **gemm, "x operand (forward)": x_operand, "fc1 + GELU epilogue": fc1(False),
                      "fc1 + GELU epilogue + p": fc1(True), "fc2": fc2, **wpasses}, a.iters, a.reps)
        report(f"{name}: pieces through the C entry points", rp, results,
               {k: one for k in list(gemm) + ["fc1 + GELU epilogue", "fc1 + GELU epilogue + p", "fc2"]})
        gsum = sum(rp[k][0] for k in gemm)
        share = rp["producers (all six launches)"][0] / (rp["producers (all six launches)"][0] + gsum)
        print(f"    four GEMMs {gsum:.1f} us; producers' share of producers + GEMMs: {share * 100:.1f} %")
        wsum = sum(rp[k][0] for k in wpasses)
        print(f"    four weight-operand passes {wsum:.1f} us per optimizer step")
        results[f"{name}: four_weight_passes"] = round(wsum, 2)
        results[f"{name}: four_gemms"] = round(gsum, 2)
        results[f"{name}: producer_share"] = round(share, 4)
        del w1n, w2n, w1t, w2t, xo, ho, dyo, dyt, xt, dpre, dpre_t, h_t, p, dh
    seam.configure(gemm_mode=E.DEFAULT_GEMM_MODE)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
