#!/usr/bin/env python3
"""What masked sampling (VAR.autoregressive_infer_cfg_edit) costs, measured in ONE process with the variants alternating ("masked sampling").

  (a) the sampler launch alone at the last stage's shape (B = 8, l = 256, V = 4096, top_k 900, top_p 0.96, t = 1.5, in-kernel Philox): sdvar_cfg_sample against
      sdvar_cfg_sample_forced with 0 %, 50 %, 75 % and 100 % of the tokens forced (the forced tokens spread at random over images and tokens).
      sdvar_cfg_sample is timed twice per round ("again"): their ratio is the run-to-run spread the other ratios are read against.
  (b) d16, 256^2, B = 8: autoregressive_infer_cfg against autoregressive_infer_cfg_edit with a 25 % hole, its inverse and an all-regenerate mask.
  (c) the parts of an edit call, each timed alone on the same inputs: encode (img_to_idxBl), mask table (mask_tokens), sampler loop (plain_ar with and without the
      mask), decode (fhat_to_img), composite (img_composite, against add_(1).mul_(0.5)).

Times come from a host clock around work that ends in a device synchronise; every window is warmed up with what it times.  Needs an MI355X.

    python tools/edit_bench.py [--rounds 7] [--launches 50] [--steps 5] > profiles/edit_bench.log"""
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
import sdvar_amd  # noqa: E402
from sdvar_amd import engine as E  # noqa: E402
from sdvar_amd.ladder import LADDER_256, as_ladder  # noqa: E402

B, L9, V, T9, TOP_K, TOP_P, SEED, H = 8, 256, 4096, 1.5, 900, 0.96, 1234, 256


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


def kernels(dev, lib, rounds, launches):
    g = torch.Generator(device=dev); g.manual_seed(1)
    lg = torch.randn(2 * B, L9, V, device=dev, generator=g) * 2.5
    ids = torch.zeros(B, L9, dtype=torch.int64, device=dev)
    force = torch.randint(0, V, (B, L9), device=dev, generator=g)
    rs = np.random.Generator(np.random.Philox(key=[1, 2]))

    def table(frac):          # exactly frac of the B * l tokens forced, spread at random
        gen = np.ones(B * L9, np.uint8)
        gen[rs.permutation(B * L9)[:int(round(frac * B * L9))]] = 0
        return torch.from_numpy(gen.reshape(B, L9)).to(dev)
    tabs = {f: table(f) for f in (0.0, 0.5, 0.75, 1.0)}
    plain = lambda i: E._check(lib.sdvar_cfg_sample(_p(lg), B, L9, V, T9, TOP_K, TOP_P, None, SEED, 9, 0, _p(ids), L9, None, _st()))

    def forced(f):
        gen = tabs[f]
        return lambda i: E._check(lib.sdvar_cfg_sample_forced(_p(lg), B, L9, V, T9, TOP_K, TOP_P, None, SEED, 9, 0, _p(ids), L9, None, _p(gen), _p(force), L9, _st()))
    var = [("cfg_sample", plain), ("again", plain)] + [(f"forced {int(100 * f)} %", forced(f)) for f in tabs]
    med, spread = alternate(var, rounds, launches, 5)
    print(f"# (a) the sampler launch at B = {B}, l = {L9}, V = {V}, t = {T9}, top_k = {TOP_K}, top_p = {TOP_P}, Philox noise: microseconds per call,")
    print(f"#     median of {rounds} alternating windows of {launches} calls.  spread = largest max/min over a variant's windows")
    print(f"{'entry':>16} {'us':>9} {'/ cfg_sample':>13}")
    for k, v in med.items():
        print(f"{k:>16} {v * 1e6:>9.1f} {v / med['cfg_sample']:>13.3f}")
    print(f"# spread: {spread:.3f}")


def end_to_end(dev, rounds, steps, warmup):
    vae, var = sdvar_amd.build_vae_var(device=dev, depth=16)
    lad = as_ladder(LADDER_256)
    g = torch.Generator(device=dev); g.manual_seed(2)
    image = (torch.rand(B, 3, H, H, device=dev, generator=g) * 2 - 1).contiguous()
    hole = torch.zeros(H, H, dtype=torch.uint8, device=dev); hole[64:192, 64:192] = 1          # 25 % of the pixels
    masks = {"25 % hole": hole, "its inverse": 1 - hole, "all regenerated": torch.ones_like(hole)}
    labels = (torch.arange(B) % 1000)
    kw = dict(cfg=1.5, top_k=TOP_K, top_p=TOP_P)
    plain = lambda i: var.autoregressive_infer_cfg(B, labels, g_seed=i, **kw)
    variants = [("autoregressive_infer_cfg", plain), ("again", plain)]
    for name, m in masks.items():
        variants.append((f"edit, {name}", (lambda m_: lambda i: var.autoregressive_infer_cfg_edit(image, m_, labels, g_seed=i, **kw))(m)))
    med, spread = alternate(variants, rounds, steps, warmup)
    print(f"# (b) d16, 256^2, B = {B}, image out: ms per call, median of {rounds} alternating windows of {steps} calls; images/s = B / median")
    print(f"{'call':>32} {'ms':>8} {'images/s':>9} {'/ plain':>8}")
    for k, v in med.items():
        print(f"{k:>32} {v * 1e3:>8.2f} {B / v:>9.1f} {v / med['autoregressive_infer_cfg']:>8.3f}")
    print(f"# spread: {spread:.3f}")

    # (c) the parts, on the 25 % hole
    smp = var._sampler
    lab_d = labels.to(dev)
    mask_px = hole[None].expand(B, H, H).contiguous()
    force = torch.cat(vae.img_to_idxBl(image), 1).contiguous()
    gens = {name: E.mask_tokens(m[None].expand(B, H, H).contiguous(), LADDER_256) for name, m in masks.items()}
    f_hat = smp.plain_ar(lab_d, 1.5, TOP_K, TOP_P, E.Noise("device", 1)).f_hat.clone()
    img = vae.fhat_to_img(f_hat)
    parts = [("encode (img_to_idxBl)", lambda i: vae.img_to_idxBl(image)),
             ("mask table (mask_tokens)", lambda i: E.mask_tokens(mask_px, LADDER_256)),
             ("sampler loop, plain", lambda i: smp.plain_ar(lab_d, 1.5, TOP_K, TOP_P, E.Noise("device", i))),
             ("sampler loop, plain again", lambda i: smp.plain_ar(lab_d, 1.5, TOP_K, TOP_P, E.Noise("device", i)))]
    for name, gen in gens.items():
        parts.append((f"sampler loop, {name}", (lambda g_: lambda i: smp.plain_ar(lab_d, 1.5, TOP_K, TOP_P, E.Noise("device", i), force_ids=force, gen=g_, trusted_ids=True))(gen)))
    parts += [("sampler loop, hole, ids checked", lambda i: smp.plain_ar(lab_d, 1.5, TOP_K, TOP_P, E.Noise("device", i), force_ids=force, gen=gens["25 % hole"])),
              ("decode (fhat_to_img)", lambda i: vae.fhat_to_img(f_hat)),
              ("composite (img_composite)", lambda i: E.img_composite(img, image, mask_px)),
              ("clone + add_(1).mul_(0.5)", lambda i: img.clone().add_(1).mul_(0.5))]
    med, spread = alternate(parts, rounds, steps, warmup)
    print(f"# (c) the parts of an edit call, each alone: ms per call, median of {rounds} alternating windows of {steps} calls")
    print(f"{'part':>36} {'ms':>8} {'/ plain loop':>13}")
    for k, v in med.items():
        print(f"{k:>36} {v * 1e3:>8.3f} {v / med['sampler loop, plain']:>13.3f}")
    print(f"# spread: {spread:.3f}")
    print(f"# sampled tokens of {lad.L} per image: " + ", ".join(f"{name} {int(gen[0].sum())}" for name, gen in gens.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("edit_bench: no GPU - timings are taken on an MI355X only")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    lib = E.load_library()
    print(f"# {torch.cuda.get_device_name(dev)}; plain and masked sampling alternating in one process")
    if not a.skip_kernels:
        kernels(dev, lib, a.rounds, a.launches)
    if not a.skip_e2e:
        end_to_end(dev, a.rounds, a.steps, a.warmup)


if __name__ == "__main__":
    main()
