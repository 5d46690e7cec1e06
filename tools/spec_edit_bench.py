#!/usr/bin/env python3
"""What a mask costs in the speculative sampler (SDVAR.sdvar_autoregressive_infer_cfg_parallel_v1_edit), measured in ONE process with the variants alternating
("masked sampling in the speculative loop").  d12 draft -> d16 target, 256^2, B = 8; the hole / hole-inverse / box masks of tests/edit_cases.py.

  (a) the acceptance launch alone at the largest chunk of the P1 step (gamma = 2: stages 8 and 9, 169 + 256 tokens, B = 8, V = 4096, top-1 rule):
      sdvar_verify_accept_ex against sdvar_verify_accept_forced with nothing forced, with the hole's table, and with everything forced.
      sdvar_verify_accept_ex is timed twice per round ("again"): their ratio is the run-to-run spread the other ratios are read against.
  (b) the whole call: the unmasked speculative call and the target's plain autoregressive_infer_cfg_edit against the speculative edit, per mask.
  (c) the acceptance rate per stage under each mask: matched / sampled tokens of the batch, summed over every verification of the stage in `--rate-calls` calls
      (a stage without a sampled token shows "-"), and the calls' mean target calls, forced accepts and final gamma.

Times come from a host clock around work that ends in a device synchronise; every window is warmed up with what it times.  Needs an MI355X.

    python tools/spec_edit_bench.py [--rounds 7] [--launches 50] [--steps 5] > profiles/spec_edit_bench.log"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sdvar_amd  # noqa: E402
from edit_bench import alternate  # noqa: E402
from sdvar_amd import engine as E  # noqa: E402
from sdvar_amd.ladder import LADDER_256, as_ladder  # noqa: E402

B, V, TOP_K, TOP_P, CFG, GAMMA, H = 8, 4096, 900, 0.96, 1.5, 2, 256
MASKS = ("hole", "hole_inverse", "box")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def pixel_masks():
    import edit_cases as EC
    ms = EC.masks(H)
    return {n: ms[n] for n in MASKS}, EC.mask_tokens_np


def kernels(dev, lib, rounds, launches):
    lad = as_ladder(LADDER_256)
    lens = list(lad.lens[-GAMMA:])
    lsum, n = sum(lens), len(lens)
    g = torch.Generator(device=dev); g.manual_seed(1)
    lg = torch.randn(2 * B, lsum, V, device=dev, generator=g) * 2.5
    ids = torch.randint(0, V, (B, lad.L), device=dev, generator=g)
    counts = torch.zeros(40, dtype=torch.int32, device=dev)
    masks, to_tokens = pixel_masks()
    hole = torch.from_numpy(to_tokens(np.stack([masks["hole"]] * B), LADDER_256)).to(dev)
    tabs = {"nothing forced": torch.ones(B, lad.L, dtype=torch.uint8, device=dev), "the hole's table": hole,
            "everything forced": torch.zeros(B, lad.L, dtype=torch.uint8, device=dev)}
    off = lad.begin(lad.S - GAMMA)
    lens_c, ts = (C.c_int32 * n)(*lens), (C.c_double * n)(*[lad.cfg_t(CFG, lad.S - GAMMA + j) for j in range(n)])
    p_ids = C.c_void_p(ids.data_ptr() + 8 * off)
    plain = lambda i: E._check(lib.sdvar_verify_accept_ex(_p(lg), B, lsum, V, n, lens_c, ts, p_ids, lad.L, 0.5, 0, 0, 0.0, None, _p(counts), None, None, None, _st()))

    def forced(gen):
        p_gen = C.c_void_p(gen.data_ptr() + off)
        return lambda i: E._check(lib.sdvar_verify_accept_forced(_p(lg), B, lsum, V, n, lens_c, ts, p_ids, lad.L, 0.5, 0, 0, 0.0, None, _p(counts), None, None, None,
                                                                 p_gen, lad.L, _st()))
    var = [("verify_accept_ex", plain), ("again", plain)] + [(f"forced, {k}", forced(v)) for k, v in tabs.items()]
    med, spread = alternate(var, rounds, launches, 5)
    print(f"# (a) the acceptance launch (memset + match kernel + scan) at B = {B}, stages {lens}, V = {V}, top-1 rule: microseconds per call,")
    print(f"#     median of {rounds} alternating windows of {launches} calls.  spread = largest max/min over a variant's windows")
    print(f"{'entry':>28} {'us':>9} {'/ verify_accept_ex':>19}")
    for k, v in med.items():
        print(f"{k:>28} {v * 1e6:>9.1f} {v / med['verify_accept_ex']:>19.3f}")
    print(f"# spread: {spread:.3f}")
    print(f"# sampled tokens of the chunk's {B * lsum}: " + ", ".join(f"{k} {int(v[:, off:].sum())}" for k, v in tabs.items()))


def end_to_end(dev, rounds, steps, warmup, rate_calls):
    vae, draft, target, sd = sdvar_amd.build_vae_var_speculative_decoding(device=dev, depth_draft=12, depth_target=16)
    lad = as_ladder(LADDER_256)
    g = torch.Generator(device=dev); g.manual_seed(2)
    image = (torch.rand(B, 3, H, H, device=dev, generator=g) * 2 - 1).contiguous()
    masks, to_tokens = pixel_masks()
    masks = {n: torch.from_numpy(m).to(dev) for n, m in masks.items()}
    labels = (torch.arange(B) % 1000)
    kw = dict(cfg=CFG, top_k=TOP_K, top_p=TOP_P)
    spec = lambda i: sd.sdvar_autoregressive_infer_cfg_parallel_v1(B, labels, g_seed=i, gamma=GAMMA, **kw)
    variants = [("speculative, no mask", spec), ("again", spec)]
    for name, m in masks.items():
        variants.append((f"plain edit, {name}", (lambda m_: lambda i: target.autoregressive_infer_cfg_edit(image, m_, labels, g_seed=i, **kw))(m)))
        variants.append((f"speculative edit, {name}", (lambda m_: lambda i: sd.sdvar_autoregressive_infer_cfg_parallel_v1_edit(image, m_, labels, g_seed=i, gamma=GAMMA, **kw))(m)))
    med, spread = alternate(variants, rounds, steps, warmup)
    print(f"# (b) d12 -> d16, 256^2, B = {B}, gamma = {GAMMA}, thr = {sd.match_threshold}, image out: ms per call, median of {rounds} alternating windows of {steps} calls")
    print(f"{'call':>36} {'ms':>8} {'images/s':>9} {'/ spec, no mask':>16} {'/ plain edit':>13}")
    for k, v in med.items():
        pe = med.get(k.replace("speculative edit", "plain edit")) if k.startswith("speculative edit") else None
        print(f"{k:>36} {v * 1e3:>8.2f} {B / v:>9.1f} {v / med['speculative, no mask']:>16.3f} {(f'{v / pe:.3f}' if pe else '-'):>13}")
    print(f"# spread: {spread:.3f}")

    print(f"# (c) acceptance per stage, matched / sampled tokens of the batch over every verification of the stage in {rate_calls} calls (seeds 0 ..); '-' = no sampled token")
    print(f"{'mask':>14} " + " ".join(f"{'s' + str(s):>7}" for s in range(lad.S)) + f" {'target calls':>13} {'forced acc.':>12} {'gamma end':>10} {'sampled/img':>12}")
    runs = [("no mask", lambda i: spec(i))] + [(n, (lambda m_: lambda i: sd.sdvar_autoregressive_infer_cfg_parallel_v1_edit(image, m_, labels, g_seed=i, gamma=GAMMA, **kw))(m))
                                                for n, m in masks.items()]
    for name, fn in runs:
        mt, tt = np.zeros(lad.S, np.int64), np.zeros(lad.S, np.int64)
        calls, forced_acc, gam, sampled = [], [], [], []
        for i in range(rate_calls):
            fn(i)
            st = sd.last_result.stats
            for r in st["rounds"]:
                for j in range(r["g"]):
                    mt[r["stage"] + j] += r["matched"][j]; tt[r["stage"] + j] += r["total"][j]
            calls.append(st["target_calls"]); forced_acc.append(st["forced_accepts"]); gam.append(st["gamma_final"])
            sampled.append(st.get("sampled_tokens", B * lad.L) / B)
        cells = " ".join(f"{(f'{m / t:.3f}' if t else '-'):>7}" for m, t in zip(mt, tt))
        print(f"{name:>14} {cells} {np.mean(calls):>13.1f} {np.mean(forced_acc):>12.1f} {np.mean(gam):>10.1f} {np.mean(sampled):>12.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rate-calls", type=int, default=4)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spec_edit_bench: no GPU - timings are taken on an MI355X only")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    lib = E.load_library()
    print(f"# {torch.cuda.get_device_name(dev)}; masked and unmasked speculative sampling alternating in one process")
    if not a.skip_kernels:
        kernels(dev, lib, a.rounds, a.launches)
    if not a.skip_e2e:
        end_to_end(dev, a.rounds, a.steps, a.warmup, a.rate_calls)


if __name__ == "__main__":
    main()
