#!/usr/bin/env python3
"""Time seam.adaln_modulate and seam.gated_residual (csrc/adaln_train.hip) against torch's eager expressions of the reference's block glue (basic_var.py:157-158,
:174) - `ln_wo_grad(x).mul(scale.add(1)).add_(shift)` and `x + y.mul(gamma)` - in ONE process on the same tensors.

Cases: the teacher-forcing shape B 8, L 680 at C 1024 (d16) and C 1920 (d30), with float32 operands ('f32') and with autocast-fp16 modulation vectors and a half y
('amp16').  The modulation vectors are the unbind(2) views of one (B, 1, 6, C) buffer that requires grad, so the backward includes dscale / dshift / dgamma.
Rows per operator: the forward under grad, the backward alone (autograd.grad on retained graphs), forward + backward; then one whole-block line - two modulations and
two gated adds, forward + backward - with its rate against the traffic floor and torch.cuda.max_memory_allocated above the resident tensors for both paths.  Last, the
modulation forward at M = 4096, C = 1024 beside the inference path's ln_modulate_kernel (7.98 us), with rotating buffers and on one buffer.

x, y and the upstream gradient of a case are --copies distinct buffers each, used round-robin (default: as many as exceed 512 MiB together), so that no call finds its
input in the 256 MiB Infinity Cache from the call before.  Every figure is the MEDIAN over --reps windows of --iters back-to-back calls, timed with device events; the
candidates alternate window by window, so drift of the machine hits them alike; min / max of the windows are printed beside the median, and the host time to enqueue
one call beside the device time.  Traffic floors with M = B L rows: modulation 8 M C bytes forward, 12 M C backward; gated add (8 + s) M C forward and (4 + 2 s) M C
backward for a y of s bytes per element (12 M C each for a float32 y).  One JSON line at the end.
python tools/seam_adaln_bench.py [--iters 500] [--reps 7] [--widths 1024 1920]"""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdvar_amd import engine as E          # noqa: E402
from sdvar_amd import seam                 # noqa: E402

STREAM_RATE = 6.3e12        # bytes / s: the HBM stream rate DESIGN.md section 4d measures against
LN_MODULATE_US = 7.98       # ln_modulate_kernel at M = 4096, C = 1024


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
    print(title)
    base = res.get("torch eager")
    for k, (med, lo, hi, host) in res.items():
        gbs = nbytes / med * 1e-3
        ratio = f"  torch / this {base[0] / med:5.2f}x" if base and k != "torch eager" else ""
        print(f"    {k:<28s} {med:9.1f} us  (min {lo:.1f}, max {hi:.1f}; host enqueue {host:.1f})  {gbs:7.0f} GB/s of the floor's bytes  "
              f"({nbytes / (med * 1e-6) / STREAM_RATE:.2f} of 6.3 TB/s){ratio}")
        out[f"{title} | {k}"] = {"us": round(med, 2), "GBps": round(gbs, 1), "of_stream": round(nbytes / (med * 1e-6) / STREAM_RATE, 3), "host_us": round(host, 2)}
    if base:
        out[f"{title} | torch / seam"] = round(base[0] / res["seam"][0], 3)


def peak_above_resident(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    del r
    return torch.cuda.max_memory_allocated() - base


def case(Cc, mode, a, dev):
    B, L = 8, 680
    M = B * L
    half = torch.float16 if mode == "amp16" else None
    ydt, s = (half, 2) if half else (torch.float32, 4)
    gen = torch.Generator(device=dev).manual_seed(Cc)
    ncopy = a.copies or (512 * 2 ** 20) // (4 * M * Cc) + 1
    rn = lambda *shape: torch.randn(*shape, device=dev, generator=gen)
    xs = [rn(B, L, Cc).requires_grad_() for _ in range(ncopy)]
    ys = [rn(B, L, Cc).to(ydt).requires_grad_() for _ in range(ncopy)]
    gs = [rn(B, L, Cc) for _ in range(ncopy)]
    mod = (rn(B, 1, 6, Cc) * 0.5).to(half or torch.float32).requires_grad_()
    gamma1, gamma2, scale1, scale2, shift1, shift2 = mod.unbind(2)
    ring = itertools.cycle(range(ncopy))
    ln = torch.nn.LayerNorm(Cc, eps=1e-6, elementwise_affine=False)
    t_mod = lambda x, sc, sh: ln(x).mul(sc.add(1)).add_(sh)
    t_gate = lambda x, y, gm: x + y.mul(gm)
    s_mod, s_gate = seam.adaln_modulate, seam.gated_residual
    out = {"case": f"B{B} L{L} C{Cc} {mode}", "rows": M, "C": Cc, "mode": mode, "buffers_in_rotation": ncopy}

    # ---- agreement first (fp32 torch on the GPU is the other candidate, not the oracle: tests/test_gpu_seam_adaln.py has fp64)
    dm = (s_mod(xs[0], scale1, shift1) - t_mod(xs[0], scale1, shift1)).abs().max().item()
    dg = (s_gate(xs[0], ys[0], gamma1) - t_gate(xs[0], ys[0], gamma1)).abs().max().item()
    print(f"{out['case']}: max |seam - torch|: modulation {dm:.2e}, gated add {dg:.2e}; {ncopy} buffers of each operand in rotation")

    floors = {"mod": (8.0 * M * Cc, 12.0 * M * Cc), "gate": ((8.0 + s) * M * Cc, (4.0 + 2 * s) * M * Cc)}
    for op, sfn, tfn in (("mod", s_mod, t_mod), ("gate", s_gate, t_gate)):
        name = "adaln_modulate" if op == "mod" else "gated_residual"
        if op == "mod":
            call = lambda fn: (lambda i: fn(xs[i], scale1, shift1))
            wrt = lambda i: (xs[i], mod)
        else:
            call = lambda fn: (lambda i: fn(xs[i], ys[i], gamma1))
            wrt = lambda i: (xs[i], ys[i], mod)
        fwd = lambda fn: (lambda c=call(fn): c(next(ring)))
        report(f"{name} forward", windows({"seam": fwd(sfn), "torch eager": fwd(tfn)}, a.iters, a.reps), out, floors[op][0])
        graphs = {k: [call(fn)(i) for i in range(ncopy)] for k, fn in (("seam", sfn), ("torch eager", tfn))}

        def bwd(k):
            def f():
                i = next(ring)
                return torch.autograd.grad(graphs[k][i], wrt(i), gs[i], retain_graph=True)
            return f
        report(f"{name} backward", windows({"seam": bwd("seam"), "torch eager": bwd("torch eager")}, a.iters, a.reps), out, floors[op][1])
        del graphs

        def both(fn):
            c = call(fn)

            def f():
                i = next(ring)
                return torch.autograd.grad(c(i), wrt(i), gs[i])
            return f
        report(f"{name} forward + backward", windows({"seam": both(sfn), "torch eager": both(tfn)}, a.iters, a.reps), out, floors[op][0] + floors[op][1])

    # ---- the glue of one block: two modulations and two gated adds (the branch outputs y1, y2 stand for attn / ffn), forward + backward
    def block(mfn, gfn):
        def f():
            i = next(ring)
            j = (i + 1) % ncopy
            x, y1, y2 = xs[i], ys[i], ys[j]
            h1 = mfn(x, scale1, shift1)
            x1 = gfn(x, y1, gamma1)
            h2 = mfn(x1, scale2, shift2)
            x2 = gfn(x1, y2, gamma2)
            return torch.autograd.grad((h1, h2, x2), (x, y1, y2, mod), (gs[i], gs[j], gs[i]))
        return f
    nb = 2 * sum(floors["mod"]) + 2 * sum(floors["gate"])
    report("block glue (2 modulations + 2 gated adds) forward + backward", windows({"seam": block(s_mod, s_gate), "torch eager": block(t_mod, t_gate)}, a.iters, a.reps),
           out, nb)
    out["floor_bytes_block"] = nb
    out["peak_bytes_above_resident"] = {"seam": peak_above_resident(block(s_mod, s_gate)), "torch eager": peak_above_resident(block(t_mod, t_gate))}
    p = out["peak_bytes_above_resident"]
    print(f"    peak memory above the resident tensors, one block forward + backward: seam {p['seam'] / 2 ** 20:.1f} MiB, torch {p['torch eager'] / 2 ** 20:.1f} MiB "
          f"(one activation is {4 * M * Cc / 2 ** 20:.1f} MiB)")
    return out


def ln_modulate_row(a, dev):
    """The modulation forward at the shape DESIGN.md section 4 quotes for the inference path's ln_modulate_kernel: M = 4096 rows, C = 1024."""
    B, L, Cc = 8, 512, 1024
    gen = torch.Generator(device=dev).manual_seed(7)
    ncopy = (512 * 2 ** 20) // (4 * B * L * Cc) + 1
    xs = [torch.randn(B, L, Cc, device=dev, generator=gen) for _ in range(ncopy)]
    mod = torch.randn(B, 1, 6, Cc, device=dev, generator=gen)
    sc, sh = mod[:, :, 2], mod[:, :, 4]
    ring = itertools.cycle(range(ncopy))
    res = windows({"rotating buffers": lambda: E.adaln_fwd(xs[next(ring)], sc, sh), "one buffer": lambda: E.adaln_fwd(xs[0], sc, sh)}, a.iters, a.reps)
    out = {}
    print(f"engine.adaln_fwd at M = 4096, C = 1024 (ln_modulate_kernel of the inference path: {LN_MODULATE_US} us)")
    for k, (med, lo, hi, host) in res.items():
        print(f"    {k:<28s} {med:9.1f} us  (min {lo:.1f}, max {hi:.1f}; host enqueue {host:.1f})")
        out[k] = {"us": round(med, 2), "host_us": round(host, 2)}
    out["ln_modulate_kernel_us"] = LN_MODULATE_US
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--widths", type=int, nargs="+", default=[1024, 1920])
    ap.add_argument("--copies", type=int, default=0, help="buffers of each operand in rotation (0: enough to exceed 512 MiB)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seam_adaln_bench: no GPU (there is nothing to time on a CPU)")
    dev = torch.device("cuda:0")
    E.load_library()
    res = {"cases": []}
    for Cc in a.widths:
        for mode in ("f32", "amp16"):
            res["cases"].append(case(Cc, mode, a, dev))
            torch.cuda.empty_cache()
    res["adaln_fwd_M4096_C1024"] = ln_modulate_row(a, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
