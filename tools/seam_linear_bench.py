#!/usr/bin/env python3
"""Time seam.linear_grad / linear_amp_grad (the dense linears: one operator GEMM per product on operands from csrc/linear_train.hip) in ONE process on the same tensors
against torch's own F.linear: fp32 for the fp32 modes (f16x2, bf16x3), under torch.autocast for the half modes (fp16, bf16).

Shapes: the dense linears of a teacher-forced step with B 8, L 680 (M = 5440 rows) at the d16 width (C 1024) and the d30 width (C 1920):
    QKV C -> 3C;  proj C -> C;  head C -> 4096;  word_embed 32 -> C (M 5432, x without grad);  ada_lin C -> 6C (M 8).
fp32 x, fp32 master weight and bias, as the reference's trainer holds them.  Per shape and mode: the forward under grad, the backward alone (one autograd.grad call on
a retained graph, every gradient the layer has) and forward + backward; "per step" drops the seam's weight-operand cache inside every timed call, which is what an
optimizer step between calls does (torch's autocast casts its weights on every call as well).  Peak memory of a forward + backward on both sides
(torch.cuda.max_memory_allocated above what was allocated before the call).

The pieces, through the C entry points on preallocated buffers: the three GEMMs with their TFLOP/s (2 M K N FLOP each), and the operand passes (x operand, the
gradient-operand pass, x^T, the column sum; mode f16x2: the scale's absmax pass) with the bytes they must move and the time those bytes take at the project's
6.3 TB/s stream rate - the traffic floor - and the passes' share of passes + GEMMs.

The decision the backward rests on: the single-pass entries sdvar_op_grad_operands / sdvar_op_grad_operands_h against the sequence of existing entries they replace
(fp32 modes: split + sdvar_op_transpose_operand + sdvar_op_colsum, with mode f16x2's absmax on both sides; half: two sdvar_op_half_operand calls), alternating, at
the QKV and head shapes of d16, in windows of 200 calls (a window of five 20 us calls measures the scheduler).  "faster" = the medians differ by more than the
spread (max - min of the windows) of the old sequence itself.

Every figure is the MEDIAN over --reps windows of --iters back-to-back calls, timed with device events; candidates alternate window by window.
The last line is one JSON object (microseconds, bytes).
python tools/seam_linear_bench.py [--iters 5] [--reps 9] [--widths 1024,1920]"""
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

STREAM_BYTES_PER_US = 6.3e6                # 6.3 TB/s


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


def shapes(Cw, M=5440):
    """(layer, M, K, N, x requires grad)"""
    return [("QKV", M, Cw, 3 * Cw, True), ("proj", M, Cw, Cw, True), ("head", M, Cw, 4096, True), ("word_embed", M - 8, 32, Cw, False), ("ada_lin", 8, Cw, 6 * Cw, True)]


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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--widths", default="1024,1920")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seam_linear_bench: no GPU (there is nothing to time on a CPU)")
    dev, lib, results = torch.device("cuda:0"), E.load_library(), {}
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s, scale=1.0: torch.randn(*s, device=dev, generator=g) * scale
    MODES = [("f16x2", None), ("bf16x3", None), ("fp16", torch.float16), ("bf16", torch.bfloat16)]

    def per_step(fn):
        def f():
            seam._WEIGHT_PLANES.clear()
            return fn()
        return f

    for Cw in [int(w) for w in a.widths.split(",")]:
        for layer, M, K, N, xgrad in shapes(Cw):
            x = rn(M, K).requires_grad_(xgrad)
            W, b = rn(N, K, scale=1 / math.sqrt(K)).requires_grad_(), rn(N).requires_grad_()
            leaves = ((x,) if xgrad else ()) + (W, b)
            fl, Mp = 2.0 * M * K * N, seam._pad32(M)
            for mname, half in MODES:
                tag = f"C{Cw} {layer} {K}->{N} M{M} {mname}"
                seam.clear_caches()
                if half is None:
                    seam.configure(gemm_mode=mname)
                    dy = rn(M, N, scale=1e-4)
                    seam_fwd, torch_fwd = (lambda: seam.linear_grad(x, W, b)), (lambda: F.linear(x, W, b))
                else:
                    dy = rn(M, N).to(half)

                    def amp(fn, half=half):
                        def f():
                            with torch.autocast("cuda", dtype=half):
                                return fn()
                        return f
                    seam_fwd, torch_fwd = amp(lambda: seam.linear_amp_grad(x, W, b)), amp(lambda: F.linear(x, W, b))
                sg, tg = torch.autograd.grad(seam_fwd(), leaves, dy), torch.autograd.grad(torch_fwd(), leaves, dy)
                rel = max(((s_ - t_).abs().max() / t_.abs().max()).item() for s_, t_ in zip(sg, tg))
                rf = windows({"seam": seam_fwd, "torch": torch_fwd}, a.iters, a.reps)
                so, to = seam_fwd(), torch_fwd()
                rb = windows({"seam": lambda: torch.autograd.grad(so, leaves, dy, retain_graph=True),
                              "torch": lambda: torch.autograd.grad(to, leaves, dy, retain_graph=True)}, a.iters, a.reps)
                del so, to
                rt = windows({"seam": lambda: torch.autograd.grad(seam_fwd(), leaves, dy), "torch": lambda: torch.autograd.grad(torch_fwd(), leaves, dy),
                              "seam, per step": per_step(lambda: torch.autograd.grad(seam_fwd(), leaves, dy))}, a.iters, a.reps)
                mem_s = peak_bytes(lambda: torch.autograd.grad(seam_fwd(), leaves, dy))
                mem_t = peak_bytes(lambda: torch.autograd.grad(torch_fwd(), leaves, dy))
                print(f"{tag}: max |seam - torch| / max|torch| over the gradients {rel:.1e}")
                for leg, r, nf in (("forward", rf, 1), ("backward", rb, 2 if xgrad else 1), ("forward + backward", rt, 3 if xgrad else 2)):
                    s_, t_ = r["seam"], r["torch"]
                    extra = f"   per step {r['seam, per step'][0]:8.1f} us" if "seam, per step" in r else ""
                    print(f"    {leg:<20s} seam {s_[0]:8.1f} us (min {s_[1]:.1f}, max {s_[2]:.1f})   torch {t_[0]:8.1f} us (min {t_[1]:.1f}, max {t_[2]:.1f})   "
                          f"seam / torch {s_[0] / t_[0]:5.2f}   seam {nf * fl / s_[0] * 1e-6:6.1f} TFLOP/s (algorithmic){extra}")
                    results[f"{tag} | {leg}"] = {"seam": round(s_[0], 1), "torch": round(t_[0], 1), **({"seam_per_step": round(r["seam, per step"][0], 1)} if extra else {})}
                print(f"    peak memory, forward + backward: seam {mem_s / 2**20:.1f} MiB, torch {mem_t / 2**20:.1f} MiB")
                results[f"{tag} | peak_bytes"] = {"seam": mem_s, "torch": mem_t}

                # ---- the pieces on preallocated buffers
                st = E._stream()
                xr, dyr = x.detach(), dy
                if half is None:
                    npl, fmt, el = seam._OPERAND_PLANES[mname], seam._OPERAND_FORMAT[mname], torch.int16
                    op = lambda n: torch.empty(npl, n, dtype=el, device=dev)
                    wn, swn = seam._weight_planes(W, mname)
                    wt, swt = seam._weight_planes_t(W, mname)
                    xo, dyo, dyt, xt = op(M * K), op(M * N), op(N * Mp), op(K * Mp)
                    sdy = torch.zeros(4, device=dev) if mname == "f16x2" else None
                    part, db, y, dx, dw = torch.empty(Mp // 32, N, device=dev), torch.empty(N, device=dev), torch.empty(M, N, device=dev), torch.empty(M, K, device=dev), torch.empty(N, K, device=dev)
                    off = lambda sc, fl_: None if sc is None else C.c_void_p(sc.data_ptr() + 4 * fl_)
                    split = lib.sdvar_op_split_planes_f16 if mname == "f16x2" else lib.sdvar_op_split_planes
                    x_operand = (lambda: E._check(split(P(xr), P(xo), M, K, M * K, None, st))) if mname == "f16x2" else (lambda: E._check(split(P(xr), P(xo), M, K, M * K, st)))
                    scale = lambda: E._check(lib.sdvar_op_scale_pair(P(dyr), M * N, P(sdy), 0, P(swt), st))
                    grad_pass = lambda: E._check(lib.sdvar_op_grad_operands(P(dyr), N, M, N, fmt, P(sdy), P(dyo), M * N, P(dyt), N * Mp, P(part), st))
                    xt_pass = lambda: E._check(lib.sdvar_op_transpose_operand(P(xr), K, M, K, fmt, P(xt), K * Mp, None, st))
                    gemms = {"forward GEMM": lambda: seam._gemm_nt(mname, xo, wn, P(swn), y, M, N, K, b.detach(), st=st),
                             "dgrad GEMM": lambda: seam._gemm_nt(mname, dyo, wt, off(sdy, 2), dx, M, K, N, st=st),
                             "wgrad GEMM": lambda: seam._gemm_nt(mname, dyt, xt, off(sdy, 0), dw, N, K, Mp, st=st)}
                    eb = 2 * npl                       # bytes per operand element
                    traffic = {"x operand": 4 * M * K + eb * M * K, "gradient-operand pass": 4 * M * N + eb * (M * N + N * Mp) + 4 * (Mp // 32) * N,
                               "x^T": 4 * M * K + eb * K * Mp, "column sum": 4 * (Mp // 32) * N + 4 * N}
                    passes = {"x operand": x_operand, "gradient-operand pass": grad_pass, "x^T": xt_pass}
                    if sdy is not None:
                        passes["dy absmax + scale pair"] = scale
                        traffic["dy absmax + scale pair"] = 4 * M * N
                        scale()
                else:
                    dt = seam._HALF_DTYPES[half]
                    op = lambda n: torch.empty(n, dtype=torch.int16, device=dev)
                    wn, wt = seam._weight_operand_h(W, half, False), seam._weight_operand_h(W, half, True)
                    xo, dyo, dyt, xt = op(M * K), op(M * N), op(N * Mp), op(K * Mp)
                    part, db, y, dx, dw = torch.empty(Mp // 32, N, device=dev), torch.empty(N, device=dev), torch.empty(M, N, dtype=half, device=dev), torch.empty(M, K, device=dev), torch.empty(N, K, device=dev)
                    x_operand = lambda: E._check(lib.sdvar_op_half_operand(P(xr), 0, K, M, K, dt, 0, P(xo), None, st))
                    grad_pass = lambda: E._check(lib.sdvar_op_grad_operands_h(P(dyr), dt, N, M, N, dt, P(dyo), P(dyt), P(part), st))
                    xt_pass = lambda: E._check(lib.sdvar_op_operand_transpose_h(P(xo), M, K, P(xt), st))
                    bd = b.detach()
                    gemms = {"forward GEMM": lambda: seam._gemm_h(half, xo, wn, bd, y, M, N, K), "dgrad GEMM": lambda: seam._gemm_h(half, dyo, wt, None, dx, M, K, N),
                             "wgrad GEMM": lambda: seam._gemm_h(half, dyt, xt, None, dw, N, K, Mp)}
                    traffic = {"x operand": 4 * M * K + 2 * M * K, "gradient-operand pass": 2 * M * N + 2 * (M * N + N * Mp) + 4 * (Mp // 32) * N,
                               "x^T": 2 * M * K + 2 * K * Mp, "column sum": 4 * (Mp // 32) * N + 4 * N}
                    passes = {"x operand": x_operand, "gradient-operand pass": grad_pass, "x^T": xt_pass}
                passes["column sum"] = lambda: E._check(lib.sdvar_op_colsum(P(part), N, Mp // 32, N, P(db), st))
                if not xgrad:
                    gemms.pop("dgrad GEMM")
                x_operand(), grad_pass(), xt_pass()
                rp = windows({**gemms, **passes}, a.iters, a.reps)
                gsum, psum = sum(rp[k][0] for k in gemms), sum(rp[k][0] for k in passes)
                floor = sum(traffic[k] for k in passes) / STREAM_BYTES_PER_US
                for k in gemms:
                    print(f"    {k:<26s} {rp[k][0]:8.1f} us  {fl / rp[k][0] * 1e-6:7.1f} TFLOP/s")
                for k in passes:
                    print(f"    {k:<26s} {rp[k][0]:8.1f} us  traffic floor {traffic[k] / STREAM_BYTES_PER_US:7.1f} us ({traffic[k] / 2**20:.1f} MiB)")
                print(f"    GEMMs {gsum:.1f} us, operand passes {psum:.1f} us (traffic floor {floor:.1f} us): the passes are {psum / (psum + gsum) * 100:.1f} % of passes + GEMMs")
                results[f"{tag} | pieces"] = {**{k: round(rp[k][0], 1) for k in rp}, "gemm_tflops": {k: round(fl / rp[k][0] * 1e-6, 1) for k in gemms},
                                              "passes_floor_us": round(floor, 1), "pass_share": round(psum / (psum + gsum), 4)}

                # ---- the decision: the single pass against the sequence of entries it replaces (QKV and head of d16)
                if Cw == 1024 and layer in ("QKV", "head"):
                    if half is None:
                        want, want_t, sold = op(M * N), op(N * Mp), (torch.zeros(4, device=dev) if mname == "f16x2" else None)

                        def old():
                            if mname == "f16x2":          # the API entry takes the absmax itself when it is handed a scale
                                E._check(lib.sdvar_op_split_planes_f16(P(dyr), P(want), M, N, M * N, P(sold), st))
                                E._check(lib.sdvar_op_scale_pair(None, 0, P(sold), 0, P(swt), st))
                            else:
                                E._check(lib.sdvar_op_split_planes(P(dyr), P(want), M, N, M * N, st))
                            E._check(lib.sdvar_op_transpose_operand(P(dyr), N, M, N, fmt, P(want_t), N * Mp, P(sold), st))
                            E._check(lib.sdvar_op_colsum(P(dyr), N, M, N, P(db), st))

                        def new():
                            if mname == "f16x2":
                                scale()
                            grad_pass()
                            passes["column sum"]()
                    else:
                        want, want_t = op(M * N), op(N * Mp)

                        def old():
                            E._check(lib.sdvar_op_half_operand(P(dyr), dt, N, M, N, dt, 0, P(want), None, st))
                            E._check(lib.sdvar_op_half_operand(P(dyr), dt, N, M, N, dt, 1, P(want_t), P(part), st))

                        def new():
                            grad_pass()
                    old(), new()
                    assert torch.equal(want, dyo) and torch.equal(want_t, dyt), "the single pass does not write the bits of the entries it replaces"
                    # windows of ~200 calls: a window of five 20 us calls measures the clock and the scheduler as much as the kernels
                    rd = windows({"single pass": new, "existing entries": old}, max(a.iters, 200), 2 * a.reps)
                    n_, o_ = rd["single pass"], rd["existing entries"]
                    spread = o_[2] - o_[1]
                    verdict = "FASTER" if o_[0] - n_[0] > spread else "NOT faster"
                    print(f"    decision, dy ({M}, {N}) {mname}: single pass {n_[0]:.1f} us (min {n_[1]:.1f}, max {n_[2]:.1f}); existing entries {o_[0]:.1f} us "
                          f"(min {o_[1]:.1f}, max {o_[2]:.1f}, spread {spread:.1f}): {verdict} by {o_[0] - n_[0]:.1f} us")
                    results[f"{tag} | decision"] = {"single_pass": round(n_[0], 1), "existing": round(o_[0], 1), "existing_spread": round(spread, 1), "faster": verdict == "FASTER"}
                    del want, want_t
                del wn, wt, xo, dyo, dyt, xt, part, y, dx, dw, sg, tg
    seam.configure(gemm_mode=E.DEFAULT_GEMM_MODE)
    seam.clear_caches()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
