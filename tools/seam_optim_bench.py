#!/usr/bin/env python3
"""Time seam.AdamW (csrc/optim.hip: sdvar_optim_grad_stats / sdvar_optim_adamw_step) against the optimizer step the reference's AmpOptimizer.backward_clip_step issues
(utils/amp_sc.py:39-75: GradScaler.unscale_, clip_grad_norm_, torch.optim.AdamW(fused=True) through GradScaler.step, GradScaler.update) - in ONE process, on tensors of
the parameter shapes of VAR d16 and d30 (sdvar_amd.var.VAR, attn_l2_norm on, built on the meta device: no weights are allocated for the model itself) with random
float32 parameters and gradients, betas (0.9, 0.95), two groups (weight decay 0.05 / 0), grad_clip 2.

Legs (each on its own parameters and state; torch's legs and the seam's legs each share one set of gradients):
  torch full    scaler.unscale_(opt); clip_grad_norm_(params, 2); scaler.step(opt); scaler.update()        - what the reference issues with early clipping
  torch step    torch.optim.AdamW(fused=True).step() alone
  seam unscale  scaler.unscale_(opt); scaler.step(opt); scaler.update() with opt = seam.AdamW(grad_clip=2)   - the reference's flow after seam.install_optimizer
  seam scaler   scaler.step(opt); scaler.update() without unscale_: GradScaler's own inf check still passes over the gradients, the kernel unscales
  seam step     seam.AdamW.step() alone with grad_scale / found_inf set as GradScaler.step sets them
The scale is 1 and, after the warm-up, the clipping coefficient of torch's in-place clip is 1 too, so the gradients keep their values from call to call.  Every figure is
the MEDIAN over --reps windows of --iters back-to-back calls timed with device events; the legs alternate window by window; min / max of the windows stand beside the
median, and the host-clock time to ENQUEUE one call.  The tensors of one leg are far larger than the 256 MiB Infinity Cache: the rates are HBM rates.
Algorithmic bytes per element (N = all parameters): unscale_ 8 (read + write g), clip_grad_norm_ 12 (read; read + write), GradScaler's inf check 8 (torch runs it as an
unscale by 1: read + write g), an AdamW step 28 (read g, p, m, v; write p, m, v), the seam's statistics pass 4.  torch full = 48 N, torch step = 28 N, seam unscale =
40 N, seam scaler = 40 N, seam step = 32 N.  Before the legs the two library calls are timed alone on one table and workspace (engine.optim_grad_stats, 4 N;
engine.optim_adamw_step, 28 N; --engine-only stops after them).
Launches per call are counted with torch.profiler in one extra, untimed call per leg.  One JSON object per model, one line each.
python tools/seam_optim_bench.py [--models d16 d30] [--iters 5] [--reps 7] [--engine-only]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdvar_amd import engine as E          # noqa: E402
from sdvar_amd import seam                 # noqa: E402

STREAM_RATE = 6.3e12        # bytes / s: the HBM stream rate DESIGN.md section 4d measures against
BETAS, CLIP = (0.9, 0.95), 2.0


def model_shapes(depth):
    """(name, shape) of every parameter of VAR at this depth, from the module itself on the meta device."""
    from sdvar_amd.var import VAR
    with torch.device("meta"):
        m = VAR(types.SimpleNamespace(Cvae=32, vocab_size=4096, quantize=None), depth=depth, embed_dim=64 * depth, num_heads=depth, attn_l2_norm=True)
    return [(n, tuple(p.shape)) for n, p in m.named_parameters()]


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


def count_launches(fn):
    """Kernels one call launches, from torch.profiler's device activity; None when the profiler gives no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA") and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower())
        return n or None
    except Exception as exc:          # the timing rows do not depend on this
        print(f"    (launch count unavailable: {type(exc).__name__}: {exc})")
        return None


def make_set(shapes, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.02) for _, s in shapes]
    decay = [p for (n, _), p in zip(shapes, params) if p.dim() >= 2]
    rest = [p for (n, _), p in zip(shapes, params) if p.dim() < 2]
    groups = [dict(params=decay, weight_decay=0.05), dict(params=rest, weight_decay=0.0)]
    return params, groups


def set_grads(params, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3


def case(name, depth, a, dev):
    shapes = model_shapes(depth)
    N = sum(int(torch.Size(s).numel()) for _, s in shapes)
    out = {"case": name, "tensors": len(shapes), "elements": N, "launch_tensors": E.OPTIM_TENSORS_PER_LAUNCH, "chunk": E.OPTIM_CHUNK}
    tparams, tgroups = make_set(shapes, dev, depth)
    sparams, sgroups = make_set(shapes, dev, depth)
    topt = torch.optim.AdamW(tgroups, lr=1e-4, betas=BETAS, fused=True)
    sopt = seam.AdamW(sgroups, lr=1e-4, betas=BETAS, grad_clip=CLIP)
    set_grads(tparams, dev, 1)
    set_grads(sparams, dev, 1)
    tscaler = torch.amp.GradScaler("cuda", init_scale=1.0, growth_interval=10 ** 9)
    sscaler = torch.amp.GradScaler("cuda", init_scale=1.0, growth_interval=10 ** 9)
    for sc in (tscaler, sscaler):
        sc.scale(torch.ones((), device=dev))          # GradScaler creates its scale tensor at the first scale() call
    scale1, noinf = torch.ones((), device=dev), torch.zeros((), device=dev)

    def torch_full():
        tscaler.unscale_(topt)
        torch.nn.utils.clip_grad_norm_(tparams, CLIP)
        tscaler.step(topt)
        tscaler.update()

    def seam_unscale():
        sscaler.unscale_(sopt)
        sscaler.step(sopt)
        sscaler.update()

    def seam_scaler():
        sscaler.step(sopt)
        sscaler.update()

    def seam_step():
        sopt.grad_scale, sopt.found_inf = scale1, noinf
        sopt.step()
        del sopt.grad_scale, sopt.found_inf

    # ---- agreement first: one full step of each side from equal inputs (fp32 torch is the other candidate, not the oracle: tests/test_gpu_seam_optim.py has fp64)
    tnorm = torch.nn.utils.clip_grad_norm_(tparams, CLIP)
    topt.step()
    sopt.step()
    diff = max((p - q).abs().max().item() for p, q in zip(tparams, sparams))
    print(f"{name}: {len(shapes)} tensors, {N / 1e6:.1f} M elements; after one clipped step max |seam - torch fp32| over the parameters {diff:.2e}; "
          f"norm seam {sopt.global_grad_norm.item():.6f} torch {tnorm.item():.6f}")
    set_grads(tparams, dev, 1)          # torch's clip scaled them in place

    # ---- the two library calls on their own (the table and the workspace of one step, reused: the update then runs from the same record every time)
    rows_ = [(p.data_ptr(), p.grad.data_ptr(), sopt.state[p]["exp_avg"].data_ptr(), sopt.state[p]["exp_avg_sq"].data_ptr(), sopt.state[p]["step"].data_ptr(), p.numel(),
              1e-4, 0.05 if p.dim() >= 2 else 0.0) for p in sparams]
    table = E.optim_table(rows_)
    ws = torch.empty(E.optim_ws_bytes([p.numel() for p in sparams]) // 4, dtype=torch.float32, device=dev)
    eng = {"engine.optim_grad_stats (reads g; finalising launches)": (lambda: E.optim_grad_stats(table, None, None, CLIP, BETAS[0], BETAS[1], ws), 4.0),
           "engine.optim_adamw_step (reads g, p, m, v; writes p, m, v)": (lambda: E.optim_adamw_step(table, BETAS[0], BETAS[1], 1e-8, ws), 28.0)}
    eres = windows({k: f for k, (f, _) in eng.items()}, a.iters, a.reps)
    out["engine"] = {}
    for k, (med, lo, hi, host) in eres.items():
        nbytes = eng[k][1] * N
        print(f"    {k:<78s} {med:9.1f} us  (min {lo:.1f}, max {hi:.1f}; host enqueue {host:.1f})  {nbytes / med * 1e-3:6.0f} GB/s algorithmic "
              f"({nbytes / (med * 1e-6) / STREAM_RATE:.2f} of 6.3 TB/s)")
        out["engine"][k] = {"us": round(med, 1), "host_us": round(host, 1), "bytes": nbytes, "of_stream_rate": round(nbytes / (med * 1e-6) / STREAM_RATE, 3)}
    if a.engine_only:
        return out

    legs = {"torch full: unscale_ + clip_grad_norm_ + scaler.step(AdamW fused) + update": (torch_full, 48.0),
            "torch step: AdamW(fused=True).step alone": (topt.step, 28.0),
            "seam unscale: unscale_ + scaler.step(seam.AdamW) + update": (seam_unscale, 40.0),
            "seam scaler: scaler.step(seam.AdamW) + update, no unscale_": (seam_scaler, 40.0),
            "seam step: seam.AdamW.step alone, grad_scale set": (seam_step, 32.0)}
    res = windows({k: f for k, (f, _) in legs.items()}, a.iters, a.reps)
    base = res[next(iter(legs))][0]
    rows = {}
    for k, (med, lo, hi, host) in res.items():
        nbytes = legs[k][1] * N
        print(f"    {k:<78s} {med:9.1f} us  (min {lo:.1f}, max {hi:.1f}; host enqueue {host:.1f})  {nbytes / med * 1e-3:6.0f} GB/s algorithmic "
              f"({nbytes / (med * 1e-6) / STREAM_RATE:.2f} of 6.3 TB/s)  {base / med:5.2f}x torch full")
        rows[k] = {"us": round(med, 1), "min_us": round(lo, 1), "max_us": round(hi, 1), "host_us": round(host, 1), "bytes": nbytes,
                   "of_stream_rate": round(nbytes / (med * 1e-6) / STREAM_RATE, 3), "vs_torch_full": round(base / med, 3)}
    print("    launches per call:")
    for k, (f, _) in legs.items():
        rows[k]["launches"] = count_launches(f)
        print(f"        {k:<78s} {rows[k]['launches']}")
    out["legs"] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["d16", "d30"], choices=["d16", "d20", "d24", "d30"])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--engine-only", action="store_true", help="time the two library calls alone and stop")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seam_optim_bench: no GPU (there is nothing to time on a CPU)")
    dev = torch.device("cuda:0")
    E.load_library()
    lines = []
    for m in a.models:
        lines.append(json.dumps(case(m, int(m[1:]), a, dev)))
        torch.cuda.empty_cache()
    for ln in lines:
        print(ln)


if __name__ == "__main__":
    main()
