#!/usr/bin/env python3
"""What per-image sampling parameters cost, measured in ONE process with the variants alternating ("per-image parameters").

  (a) the four sampler kernels at the P1 step's stage-9 shape (B = 8, l = 256, V = 4096, top_k 900, top_p 0.96, t = 1.5, in-kernel Philox): the scalar entry
      point against the *_rows entry point with the same value in every row.  The scalar entry is timed twice per round ("scalar" and "scalar again"): their
      ratio is the run-to-run spread the other ratios are read against.  With --parent-lib PATH the scalar entry points of another build of the library
      (the parent commit's libsdvar_hip.so) are timed in the same rounds.
  (b) Sampler.plain_ar of the d16 model at B = 8 (no decode): scalar arguments against uniform sequences (the per-image path with equal rows, one table upload
      per call), and scalar again for the spread.
  (c) the same with eight different (cfg, top_k, top_p, seed) sets.

Times come from a host clock around work that ends in a device synchronise; every window is warmed up with what it times.  Needs an MI355X.

    python tools/row_params_bench.py [--rounds 7] [--launches 50] [--steps 10] [--parent-lib PATH] > profiles/row_params_bench.log"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sdvar_amd import engine as E  # noqa: E402
from sdvar_amd.ladder import LADDER_256, as_ladder  # noqa: E402

B, L9, V, T9, TOP_K, TOP_P, SEED = 8, 256, 4096, 1.5, 900, 0.96, 1234
HETERO = dict(cfg=[1.5, 3.0, 0.75, 1.0, 2.0, 4.0, 1.5, 0.0], top_k=[900, 0, 40, 900, 600, 0, 2000, 900], top_p=[0.96, 0.0, 0.5, 0.9, 0.96, 0.95, 0.99, 0.0],
              seed=[11, 12, 13, 14, 15, 16, 17, 18])


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def alternate(variants, rounds, n, warm):
    """variants: [(name, fn)].  Median seconds per call of `rounds` alternating windows of n calls, and max/min over each variant's windows."""
    for _, fn in variants:
        window(fn, warm)
    t = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            window(fn, 1)
            t[name].append(window(fn, n))
    return {k: statistics.median(v) for k, v in t.items()}, max(max(v) / min(v) for v in t.values())


def load_other(path):
    """A second build of the library beside the engine's (dlopen keeps their symbols apart): the prototypes of the entry points it has."""
    lib = C.CDLL(path)
    for name, (res, args) in E._SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def quant_for(lib, dev, sd_v):
    saved = E._lib
    E._lib = lib
    try:
        return E.QuantCtx(sd_v, LADDER_256, B, dev)
    finally:
        E._lib = saved


def kernels(dev, lib, parent, sd_v, rounds, launches):
    g = torch.Generator(device=dev); g.manual_seed(1)
    lg = torch.randn(2 * B, L9, V, device=dev, generator=g) * 2.5
    ids = torch.zeros(B, L9, dtype=torch.int64, device=dev)
    masked = torch.empty(B, L9, V, device=dev)
    counts = torch.zeros(40, dtype=torch.int32, device=dev)
    out = torch.empty(B, L9, V, device=dev)
    h = torch.empty(B, L9, 32, device=dev)
    rows = E.RowParams(B, as_ladder((1, 2)), [T9] * B, [TOP_K] * B, [TOP_P] * B, [SEED] * B, list(range(B)), dev)       # a 2-stage ladder: stage 1 has t = cfg
    fac, img, img_h = rows.fac_ptr(1), rows.img_ptr(), rows.img_host_ptr()
    lens, ts = (C.c_int32 * 1)(L9), (C.c_double * 1)(T9)
    qc = quant_for(lib, dev, sd_v)
    E._check(lib.sdvar_cfg_sample(_p(lg), B, L9, V, T9, TOP_K, TOP_P, None, SEED, 9, 0, _p(ids), L9, _p(masked), _st()))       # the masked logits gumbel_mix reads

    def scalar(l_, q_):
        return {
            "cfg_sample": lambda i: E._check(l_.sdvar_cfg_sample(_p(lg), B, L9, V, T9, TOP_K, TOP_P, None, SEED, 9, 0, _p(ids), L9, None, _st())),
            "verify_accept": lambda i: E._check(l_.sdvar_verify_accept_ex(_p(lg), B, L9, V, 1, lens, ts, _p(ids), L9, 0.5, 0, 0, 0.0, None, _p(counts), None, None, None, _st())),
            "cfg_combine": lambda i: E._check(l_.sdvar_cfg_combine(_p(lg), B, L9, V, 1, lens, ts, _p(out), _st())),
            "gumbel_mix": lambda i: E._check(l_.sdvar_gumbel_mix(q_.h, _p(masked), B, L9, 1.0, 0.0135, None, SEED, 9 | E.GUMBEL_DRAW, 0, _p(h), _st())),
        }
    per_image = {
        "cfg_sample": lambda i: E._check(lib.sdvar_cfg_sample_rows(_p(lg), B, L9, V, fac, img, img_h, B, None, 9, _p(ids), L9, None, _st())),
        "verify_accept": lambda i: E._check(lib.sdvar_verify_accept_rows(_p(lg), B, L9, V, 1, lens, fac, B, _p(ids), L9, 0.5, 0, 0, 0.0, None, _p(counts), None, None, None, _st())),
        "cfg_combine": lambda i: E._check(lib.sdvar_cfg_combine_rows(_p(lg), B, L9, V, 1, lens, fac, B, _p(out), _st())),
        "gumbel_mix": lambda i: E._check(lib.sdvar_gumbel_mix_rows(qc.h, _p(masked), B, L9, 1.0, 0.0135, None, img, B, 9 | E.GUMBEL_DRAW, _p(h), _st())),
    }
    mine = scalar(lib, qc)
    theirs = scalar(parent, quant_for(parent, dev, sd_v)) if parent is not None else None
    print(f"# (a) kernels at B = {B}, l = {L9}, V = {V}, t = {T9}, top_k = {TOP_K}, top_p = {TOP_P}, Philox noise: microseconds per call (entry point, all its launches),")
    print(f"#     median of {rounds} alternating windows of {launches} calls.  spread = largest max/min over a variant's windows; 'again' = the scalar entry timed a second time")
    print(f"{'entry':>14} {'scalar us':>10} {'again us':>10} {'rows us':>10} {'parent us':>10} {'rows/scalar':>12} {'again/scalar':>13} {'scalar/parent':>14} {'spread':>7}")
    for name in ("cfg_sample", "verify_accept", "cfg_combine", "gumbel_mix"):
        var = [("scalar", mine[name]), ("again", mine[name]), ("rows", per_image[name])] + ([("parent", theirs[name])] if theirs else [])
        med, spread = alternate(var, rounds, launches, 5)
        us = {k: v * 1e6 for k, v in med.items()}
        par = f"{us['parent']:>10.1f}" if theirs else f"{'-':>10}"
        rp = f"{us['scalar'] / us['parent']:>14.3f}" if theirs else f"{'-':>14}"
        print(f"{name:>14} {us['scalar']:>10.1f} {us['again']:>10.1f} {us['rows']:>10.1f} {par} {us['rows'] / us['scalar']:>12.3f} {us['again'] / us['scalar']:>13.3f} {rp} {spread:>7.3f}")


def end_to_end(dev, sd_v, rounds, steps, warmup):
    from sdvar_amd.weights import var_state_dict_device
    sd_t = var_state_dict_device(16, LADDER_256, dev, seed=1234)
    tc, qc = E.ModelCtx(sd_t, 16, LADDER_256, B, 1, dev), E.QuantCtx(sd_v, LADDER_256, B, dev)
    smp = E.Sampler(tc, qc)
    labels = (torch.arange(B) % 1000).to(dev)
    scalar = lambda i: smp.plain_ar(labels, 1.5, TOP_K, TOP_P, E.Noise("device", i))
    uniform = lambda i: smp.plain_ar(labels, [1.5] * B, [TOP_K] * B, [TOP_P] * B, E.Noise("device", [i] * B, list(range(B))))
    hetero = lambda i: smp.plain_ar(labels, HETERO["cfg"], HETERO["top_k"], HETERO["top_p"], E.Noise("device", [s + 100 * i for s in HETERO["seed"]]))
    a, b = scalar(3).ids.clone(), uniform(3).ids.clone()
    assert torch.equal(a, b), "uniform sequences must be the scalar call"
    med, spread = alternate([("scalar", scalar), ("again", scalar), ("uniform", uniform), ("hetero", hetero)], rounds, steps, warmup)
    ms = {k: v * 1e3 for k, v in med.items()}
    print(f"# (b), (c) Sampler.plain_ar, d16, B = {B}, no decode: ms per call, median of {rounds} alternating windows of {steps} calls; images/s = B / median")
    print(f"{'arguments':>28} {'ms':>8} {'images/s':>9} {'/ scalar':>9}")
    for k, label in (("scalar", "scalar"), ("again", "scalar again"), ("uniform", "(b) uniform sequences"), ("hetero", "(c) eight parameter sets")):
        print(f"{label:>28} {ms[k]:>8.2f} {B / ms[k] * 1e3:>9.1f} {ms[k] / ms['scalar']:>9.3f}")
    print(f"# spread (largest max/min over a variant's windows): {spread:.3f}")
    print(f"# (c) parameter sets: cfg {HETERO['cfg']} top_k {HETERO['top_k']} top_p {HETERO['top_p']}: images without top-k sort all 4096 entries, images without top-p sort none")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libsdvar_hip.so of the parent commit: its scalar entry points are timed in the same rounds")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("row_params_bench: no GPU - timings are taken on an MI355X only")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    from sdvar_amd.weights import vae_state_dict
    lib = E.load_library()
    parent = load_other(a.parent_lib) if a.parent_lib else None
    sd_v = vae_state_dict(LADDER_256, "perf", 1234, with_encoder=False)
    print(f"# {torch.cuda.get_device_name(dev)}; scalar and per-image sampling parameters alternating in one process" + ("; parent library loaded beside this one" if parent else ""))
    if not a.skip_kernels:
        kernels(dev, lib, parent, sd_v, a.rounds, a.launches)
    if not a.skip_e2e:
        end_to_end(dev, sd_v, a.rounds, a.steps, a.warmup)


if __name__ == "__main__":
    main()
