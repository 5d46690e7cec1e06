#!/usr/bin/env python3
"""What the decoder's conv mode 'f16' (one fp16 product per convolution, plane_format 6) buys, measured against 'f16x2' in ONE process with the two alternating
("Conv mode f16").

  a. per convolution: every distinct conv_planes shape of the ch = 160 decoder at B = 8, 256^2 (3x3, 1x1, the fused up-sampling phases, with and without residual,
     split and unsplit) through sdvar_op_conv_planes_ex with the decoder's workspace and fused GroupNorm statistics: microseconds per launch in both formats, their
     ratio, and the kernel and K split each took (sdvar_debug_get_conv_plan).
  f. the K-step cost of conv_choose_split for the one-product loop: the shapes of the 16^2 and 32^2 levels timed at every K split the library can make, and, for
     candidate costs, the splits the heuristic (restated here) would choose and what they cost in measured time.
  b. whole decode at B = 8, 256^2 and at B = 2, 512^2: --pairs alternating pairs, every pair printed, and the verdict the mode is held to.
  c. end to end: the P1 step of bench.py (d12 -> d16, B = 8, gamma = 2, threshold 0.5 on random weights, decode of batch i under the sampling of batch i + 1) in
     conv modes f16x2 and f16, the same with gemm_mode 'f16' on top, and plain d16 AR.

Times: (a) and (f) HIP events around a window of launches, (b) and (c) a host clock around work that ends in a device synchronise; every window is warmed up with
the shapes it times.  Needs an MI355X.

    python tools/f16_conv_bench.py [--rounds 5] [--pairs 5] [--steps 10] [--skip-e2e] > profiles/f16_conv_bench.log"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sdvar_amd import engine as E  # noqa: E402

PNS = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
WS_FLOATS = 64 << 20                                           # the decoder's split-K workspace (vae.hip)
# (H, Cin, N, taps, residual, where) - the decoder walk of vae.hip at ch = 160, ch_mult (1, 1, 2, 2, 4), latent 16; taps 4 = the fused up-sampling (output 2H)
SHAPES = [
    (16, 32, 32, 9, 0, "post_quant_conv"), (16, 32, 640, 9, 0, "conv_in"), (16, 640, 640, 9, 0, "res conv1 @16"), (16, 640, 640, 9, 1, "res conv2 @16"),
    (16, 640, 1920, 1, 0, "attn qkv"), (16, 640, 640, 1, 1, "attn proj"), (16, 640, 640, 4, 0, "up 16 -> 32"),
    (32, 640, 320, 9, 0, "res conv1 @32 (first)"), (32, 640, 320, 1, 0, "shortcut @32"), (32, 320, 320, 9, 0, "res conv1 @32"), (32, 320, 320, 9, 1, "res conv2 @32"),
    (32, 320, 320, 4, 0, "up 32 -> 64"),
    (64, 320, 320, 9, 0, "res conv1 @64"), (64, 320, 320, 9, 1, "res conv2 @64"), (64, 320, 320, 4, 0, "up 64 -> 128"),
    (128, 320, 160, 9, 0, "res conv1 @128 (first)"), (128, 320, 160, 1, 0, "shortcut @128"), (128, 160, 160, 9, 0, "res conv1 @128"), (128, 160, 160, 9, 1, "res conv2 @128"),
    (128, 160, 160, 4, 0, "up 128 -> 256"),
    (256, 160, 160, 9, 0, "res conv1 @256"), (256, 160, 160, 9, 1, "res conv2 @256"),
]
KERNEL = {0: "bf16x3", 1: "f16x2", 2: "f16x2-reuse", 3: "hh", 4: "hh-reuse"}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def host_window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def event_window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n                       # microseconds per launch


class Conv:
    """one convolution of the decoder on random operands from the library's producers (format 2 planes: format 6 reads their plane 0)"""

    def __init__(self, lib, dev, B, H, Cin, N, taps, res, g):
        self.lib, self.B, self.H, self.Cin, self.N, self.taps = lib, B, H, Cin, N, taps
        W = H
        self.G = (W + 3 + 15) // 16 * 16
        self.R = B * (H + 2) * (W + 2) + 2 * self.G
        self.M, self.nkt = B * H * W, taps * (Cin // 32)
        x = torch.randn(self.M, Cin, device=dev, generator=g)
        self.xp = torch.zeros(2, Cin // 32, self.R, 32, dtype=torch.int16, device=dev)
        E._check(lib.sdvar_op_vae_prep(_p(x), None, None, None, _p(self.xp), (Cin // 32) * self.R * 32, 2, B, Cin, H, W, 0, 0, self.G, _st()))
        self.wsc = torch.zeros(4, device=dev)
        if taps == 4:
            w = (torch.randn(N, Cin, 3, 3, device=dev, generator=g) / (9 * Cin) ** 0.5).contiguous()
            self.wps = 4 * Cin * N
            weff = torch.zeros(4, N, Cin, 4, device=dev)
            E._check(lib.sdvar_op_upconv_weights(_p(w), _p(weff), N, Cin, _st()))
            tmp = torch.zeros(2, 16 * N * Cin, dtype=torch.int16, device=dev)
            E._check(lib.sdvar_op_split_planes_f16(_p(weff), _p(tmp), 16 * N, Cin, 16 * N * Cin, _p(self.wsc), _st()))
            weff = (weff * self.wsc[0]).contiguous()
            self.wp = torch.zeros(4, 2, self.wps, dtype=torch.int16, device=dev)
            for ph in range(4):
                E._check(lib.sdvar_op_conv_weight_planes(_p(weff[ph]), _p(self.wp[ph]), N, Cin, 4, self.wps, 2, None, _st()))
            self.wstride, self.up = 2 * self.wps, 0
        else:
            k = 3 if taps == 9 else 1
            w = (torch.randn(N, Cin, k, k, device=dev, generator=g) / (taps * Cin) ** 0.5).contiguous()
            self.wps = taps * Cin * N
            self.wp = torch.zeros(2, self.wps, dtype=torch.int16, device=dev)
            E._check(lib.sdvar_op_conv_weight_planes(_p(w), _p(self.wp), N, Cin, taps, self.wps, 2, _p(self.wsc), _st()))
            self.wstride, self.up = 0, -1
        Mo = self.M * (4 if taps == 4 else 1)
        self.bias = torch.randn(N, device=dev, generator=g)
        self.res = torch.randn(Mo, N, device=dev, generator=g) if res else None
        self.out = torch.empty(Mo, N, device=dev)
        self.part = torch.zeros(B * ((H * W) // 256 + 64) * 64 * 4, dtype=torch.float64, device=dev)
        self.stats = torch.zeros(B, 32, 2, device=dev)
        self.done = C.c_int32(-1)
        torch.cuda.synchronize()

    def run(self, pf, ws, force_split=0):
        E._check(self.lib.sdvar_op_conv_planes_ex(_p(self.xp), (self.Cin // 32) * self.R * 32, self.R, self.G, _p(self.wp), self.wps, pf, _p(self.wsc), _p(self.bias),
                                                  _p(self.res), _p(self.out), self.B, self.H, self.H, self.N, self.Cin, self.taps, _p(ws), WS_FLOATS, force_split, self.up,
                                                  self.wstride, _p(self.part), _p(self.stats), C.byref(self.done), _st()))

    def plan(self):
        out4 = (C.c_int32 * 4)()
        E._check(self.lib.sdvar_debug_get_conv_plan(out4))
        return list(out4)


def launches_for(us_guess):
    return 40 if us_guess < 200 else 20 if us_guess < 1000 else 10


def per_conv(lib, dev, B, rounds):
    print(f"# a. per convolution, B = {B}, ch = 160 decoder: microseconds per launch, median of {rounds} alternating windows (HIP events); ratio = f16x2 / f16 (above 1: f16 faster)")
    print(f"{'H':>4} {'Cin':>4} {'N':>5} {'taps':>4} {'res':>3} {'K-steps':>7} {'f16x2 us':>9} {'f16 us':>9} {'ratio':>6} {'f16x2 kernel/split':>18} {'f16 kernel/split':>17}  where")
    g = torch.Generator(device=dev); g.manual_seed(1)
    ws = torch.empty(WS_FLOATS, device=dev)
    slower, tot = [], [0.0, 0.0]
    for H, Cin, N, taps, res, where in SHAPES:
        c = Conv(lib, dev, B, H, Cin, N, taps, res, g)
        for pf in (2, 6):
            for _ in range(3):
                c.run(pf, ws)
        c.run(2, ws); p2 = c.plan(); c.run(6, ws); p6 = c.plan()
        n = launches_for(event_window(lambda: c.run(2, ws), 3))
        ta, tb = [], []
        for _ in range(rounds):
            ta.append(event_window(lambda: c.run(2, ws), n)); tb.append(event_window(lambda: c.run(6, ws), n))
        a, b = statistics.median(ta), statistics.median(tb)
        tot[0] += a; tot[1] += b
        print(f"{H:>4} {Cin:>4} {N:>5} {taps:>4} {res:>3} {c.nkt:>7} {a:>9.1f} {b:>9.1f} {a / b:>6.2f} {KERNEL[p2[0]] + '/' + str(p2[2]):>18} {KERNEL[p6[0]] + '/' + str(p6[2]):>17}  {where}")
        if b > a:
            slower.append((H, Cin, N, taps, res, round(a / b, 3)))
        del c
    print(f"# sum over the distinct shapes (one launch each): f16x2 {tot[0]:.0f} us, f16 {tot[1]:.0f} us")
    print("# one-product kernel slower per launch at:", slower or "no shape")


def choose_split(M, N, nkt, ws_floats, kstep):
    """conv_choose_split of csrc/conv.hip, restated"""
    tiles = -(-M // 256) * -(-N // 160)
    best, bs = 1e30, 1
    split = 1
    while split <= 16 and split <= nkt // 2:
        if split > 1 and (split * M * N > ws_floats or N % 4):
            break
        kps = -(-nkt // split)
        if -(-nkt // kps) == split:
            rounds = (tiles * split + 255) // 256
            cyc = rounds * (kps * kstep + 3000.0)
            if split > 1:
                cyc += 4000.0 + (split + 2) * M * N * 4.0 / 4000.0
            if cyc < best:
                best, bs = cyc, split
        split += 1
    return bs


def fit_kstep(lib, dev, B, rounds):
    print(f"# f. K-step cost of the one-product per-tap loop for conv_choose_split: format 6 at every K split the library can make (forced), B = {B}; us per call (kernel + reduce)")
    g = torch.Generator(device=dev); g.manual_seed(2)
    ws = torch.empty(WS_FLOATS, device=dev)
    table = []
    for H, Cin, N, taps, res, where in SHAPES:
        if H > 32 or taps == 4:
            continue
        c = Conv(lib, dev, B, H, Cin, N, taps, res, g)
        splits = [s for s in range(1, 17) if s <= max(c.nkt // 2, 1) and -(-c.nkt // -(-c.nkt // s)) == s and s * c.M * N <= WS_FLOATS]
        times = {}
        for s in splits:
            for _ in range(3):
                c.run(6, ws, s)
            assert c.plan()[2] == s, (c.plan(), s)
            times[s] = statistics.median(event_window(lambda: c.run(6, ws, s), 20) for _ in range(rounds))
        table.append((c.M, N, c.nkt, times, where))
        print(f"  H {H:>3} {Cin:>4} -> {N:>5} taps {taps} res {res} ({where}): " + " ".join(f"{s}:{t:.1f}" for s, t in times.items()) + f"   best split {min(times, key=times.get)}")
        del c
    best = sum(min(t.values()) for _, _, _, t, _ in table)
    print(f"  sum of the best split per shape: {best:.1f} us")
    print("  cost  -> splits chosen (shape order above), sum of their measured times")
    for k in (300, 400, 500, 600, 700, 800, 900, 1000, 1200, 1500, 2000):
        ch = [choose_split(M, N, nkt, WS_FLOATS, float(k)) for M, N, nkt, _, _ in table]
        tot = sum(t[s] for (_, _, _, t, _), s in zip(table, ch))
        print(f"  {k:>5} -> {ch}  {tot:.1f} us ({tot / best:.3f} of the best)")


def decode_pairs(dev, pairs, iters):
    from sdvar_amd.weights import vae_state_dict
    sd = vae_state_dict(PNS, "stress", 3, with_encoder=False)
    print(f"# b. whole decode, ch = 160: ms per batch, {pairs} alternating pairs of windows of {iters} decodes (2 warm-up decodes per window)")
    for B, latent in ((8, 16), (2, 32)):
        ctxs = {m: E.VaeCtx(sd, B, dev, latent_hw=latent, conv_mode=m) for m in ("f16x2", "f16")}
        f_hat = torch.randn(B, 32, latent, latent, device=dev)
        out = torch.empty(B, 3, 16 * latent, 16 * latent, device=dev)
        t = {"f16x2": [], "f16": []}
        for _ in range(pairs):
            for m in ("f16x2", "f16"):
                host_window(lambda i: ctxs[m].decode(f_hat, out), 2)
                t[m].append(host_window(lambda i: ctxs[m].decode(f_hat, out), iters) * 1e3)
        print(f"  B = {B}, {16 * latent}^2: f16x2 " + " ".join(f"{v:.2f}" for v in t["f16x2"]) + "   f16 " + " ".join(f"{v:.2f}" for v in t["f16"]))
        every = all(b < a for a, b in zip(t["f16x2"], t["f16"]))
        print(f"    medians f16x2 {statistics.median(t['f16x2']):.2f} ms, f16 {statistics.median(t['f16']):.2f} ms, ratio {statistics.median(t['f16x2']) / statistics.median(t['f16']):.3f}; "
              f"f16 faster in every pair: {every}; slowest f16 {max(t['f16']):.2f} {'<' if max(t['f16']) < min(t['f16x2']) else '>='} fastest f16x2 {min(t['f16x2']):.2f}")
        for c in ctxs.values():
            c.close()


def end_to_end(dev, rounds, steps, warmup):
    from sdvar_amd.ladder import LADDER_256, as_ladder
    from sdvar_amd.vqvae import VQVAE
    from sdvar_amd.weights import vae_state_dict, var_state_dict_device
    pns, B, CFG, lad = LADDER_256, 8, 1.5, as_ladder(LADDER_256)
    sd_d, sd_t = var_state_dict_device(12, pns, dev, seed=1234), var_state_dict_device(16, pns, dev, seed=1234)
    sd_v = vae_state_dict(pns, "perf", 1234, with_encoder=False)
    vaes = {}
    for cm in ("f16x2", "f16"):                                            # one VQVAE per conv mode: switching VQVAE.conv_mode would rebuild the context at every window
        v = VQVAE(vocab_size=4096, z_channels=32, ch=160, v_patch_nums=pns, with_encoder=False)
        v.load_state_dict(sd_v); v = v.to(dev); v.conv_mode = cm
        vaes[cm] = v
    labels = (torch.arange(B) % 1000).to(dev)
    main, dec = torch.cuda.current_stream(), torch.cuda.Stream(device=dev)
    fh = [torch.zeros(B, 32, lad.HW, lad.HW, device=dev) for _ in range(2)]
    done, state = [None, None], {"i": 0}

    def with_decode(res, vae):                                             # bench.py's step: the decode of batch i on a second stream, under the sampling of batch i + 1
        j = state["i"] & 1; state["i"] += 1
        if done[j] is not None:
            main.wait_event(done[j])
        fh[j].copy_(res.f_hat)
        ready = torch.cuda.Event(); ready.record(main)
        dec.wait_event(ready)
        with torch.cuda.stream(dec):
            vae.fhat_to_img(fh[j]).add_(1).mul_(0.5)
            done[j] = torch.cuda.Event(); done[j].record(dec)

    qc = E.QuantCtx(sd_v, pns, B, dev)
    samplers, keep = {}, []
    for gm in ("f16x2", "f16"):
        dc, tc = E.ModelCtx(sd_d, 12, pns, B, 1, dev, gemm_mode=gm), E.ModelCtx(sd_t, 16, pns, B, 2, dev, gemm_mode=gm)
        samplers[gm] = (E.Sampler(tc, qc, dc), E.Sampler(tc, qc))
        keep.append((dc, tc))

    def p1(gm, cm):
        return lambda i: with_decode(samplers[gm][0].spec_decode(labels, CFG, 2, 900, 0.96, E.Noise("device", i), thr=0.5), vaes[cm])

    def plain(gm, cm):
        return lambda i: with_decode(samplers[gm][1].plain_ar(labels, CFG, 900, 0.96, E.Noise("device", i)), vaes[cm])
    rows = [("P1 step (d12 -> d16, B = 8, decode), gemm f16x2", p1, "f16x2"), ("P1 step (d12 -> d16, B = 8, decode), gemm f16", p1, "f16"),
            ("plain d16 AR (B = 8, decode), gemm f16x2", plain, "f16x2")]
    print(f"# c. end to end: ms per step, median of {rounds} alternating windows of {steps} steps ({warmup} warm-up steps per case); ratio = conv f16x2 / conv f16")
    print(f"{'workload':>50} {'conv f16x2 ms':>14} {'conv f16 ms':>12} {'ratio':>6}   spread")
    for name, mk, gm in rows:
        fns = {cm: mk(gm, cm) for cm in ("f16x2", "f16")}
        t = {cm: [] for cm in fns}
        for cm, fn in fns.items():
            host_window(fn, warmup)
        for _ in range(rounds):
            for cm, fn in fns.items():
                host_window(fn, 1)
                t[cm].append(host_window(fn, steps))
        med = {k: statistics.median(v) * 1e3 for k, v in t.items()}
        spread = max(max(v) / min(v) for v in t.values())
        print(f"{name:>50} {med['f16x2']:>14.2f} {med['f16']:>12.2f} {med['f16x2'] / med['f16']:>6.3f}   {spread:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-conv", action="store_true")
    ap.add_argument("--skip-fit", action="store_true")
    ap.add_argument("--skip-decode", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("f16_conv_bench: no GPU - timings are taken on an MI355X only")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    lib = E.load_library()
    print(f"# {torch.cuda.get_device_name(dev)}; conv modes f16x2 (plane_format 2) and f16 (plane_format 6) alternating in one process")
    if not a.skip_conv:
        per_conv(lib, dev, a.batch, a.rounds)
    if not a.skip_fit:
        fit_kstep(lib, dev, a.batch, a.rounds)
    if not a.skip_decode:
        decode_pairs(dev, a.pairs, a.iters)
    if not a.skip_e2e:
        end_to_end(dev, a.rounds, a.steps, a.warmup)


if __name__ == "__main__":
    main()
