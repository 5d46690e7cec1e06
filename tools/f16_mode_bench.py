#!/usr/bin/env python3
"""What the engine's GEMM mode 'f16' buys, measured against 'f16x2' in ONE process with the two alternating ("GEMM mode f16").

  1. per GEMM: the f16x2 launch (sdvar_op_gemm_f16x2: planner's tile, K split and reduce) against the half kernel on the same operands' high planes
     (sdvar_op_gemm_h_ex), for the engine's (N, K, epilogue) at C = 768 / 1024 / 1920 and M in {256 .. 5440}.  Eight weight copies are rotated so that a launch finds
     its weights outside L2 as inside a model pass (more than the 256 MB of the memory-side cache at the wide shapes, less at the narrow ones: stated per row).
     Prints the table and the smallest M from which the half kernel is not slower at ANY of the shapes - the default of the variant `h16_min_m`.
  2. end to end, each in f16x2 and in f16 at the --min-m values of h16_min_m (the first is the library's default): the P1 step of bench.py (d12 -> d16, B = 8, gamma = 2, acceptance threshold 0.5 on
     random weights = every round rejected: the worst case; VQVAE decode of batch i overlapped with the sampling of batch i + 1), plain AR of the d16 target with
     the same decode, and a teacher-forced d16 pass over 32 images (eval_ep's forward).

Times come from a host clock around work that ends in a device synchronise; every window is warmed up with the shapes it times.  Needs an MI355X.

    python tools/f16_mode_bench.py [--rounds 5] [--steps 10] [--skip-e2e] > profiles/f16_mode_bench.log"""
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

MS = (256, 576, 1024, 1600, 2704, 4096, 5440)
WIDTHS = (768, 1024, 1920)
NCOPY = 8


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def shapes(Cw, V=4096):
    return [("qkv", 3 * Cw, Cw, 0), ("proj", Cw, Cw, 2), ("fc1", 4 * Cw, Cw, 1), ("fc2", Cw, 4 * Cw, 2), ("head", V, Cw, 0)]


def planes(lib, x, scaled):
    rows, K = x.shape
    p = torch.empty(2, K // 32, rows, 32, dtype=torch.int16, device=x.device)
    sc = torch.zeros(4, device=x.device) if scaled else None
    E._check(lib.sdvar_op_split_planes_f16(_p(x), _p(p), rows, K, rows * K, _p(sc), _st()))
    return p, sc


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def per_gemm(lib, dev, rounds, launches):
    print(f"# 1. per GEMM: microseconds per launch, median of {rounds} alternating windows of {launches} launches over {NCOPY} rotating weight copies; ratio = f16x2 / half")
    print(f"{'C':>5} {'gemm':>5} {'N':>5} {'K':>5} {'M':>5} {'f16x2 us':>9} {'half us':>9} {'ratio':>6} {'half TFLOP/s':>12} {'f16x2 kernel':>12} {'weights MB':>10}")
    g = torch.Generator(device=dev); g.manual_seed(1)
    slower = {}                                                            # M -> [(C, gemm, ratio)] where the half kernel lost
    for Cw in WIDTHS:
        for name, N, K, epi in shapes(Cw):
            Ws = [planes(lib, torch.randn(N, K, device=dev, generator=g) * K ** -0.5, True) for _ in range(NCOPY)]
            bias = torch.randn(N, device=dev, generator=g)
            for M in MS:
                Xp, _ = planes(lib, torch.randn(M, K, device=dev, generator=g), False)
                rpg = 680 if M >= 680 else M
                gate = torch.randn((M + rpg - 1) // rpg, 2 * N, device=dev, generator=g) * 0.1
                out = torch.zeros(M, N, device=dev) if epi != 1 else None
                outp = torch.empty(2, N // 32, M, 32, dtype=torch.int16, device=dev) if epi == 1 else None
                res, gt = (out, gate) if epi == 2 else (None, None)

                def x2(i):
                    Wp, sc = Ws[i % NCOPY]
                    E._check(lib.sdvar_op_gemm_f16x2(_p(Xp), M * K, _p(Wp), N * K, _p(sc), _p(bias), _p(out), N, _p(outp), M * N, M, N, K, epi, _p(res), N, _p(gt), rpg, 2 * N, _st()))

                def half(i):
                    Wp, sc = Ws[i % NCOPY]
                    E._check(lib.sdvar_op_gemm_h_ex(_p(Xp), _p(Wp), 1, C.c_void_p(sc.data_ptr() + 4), _p(bias), _p(out), N, _p(outp), None, _p(res), N, _p(gt), rpg, 2 * N,
                                                    M, N, K, epi, _st()))
                window(x2, NCOPY); kern = E.last_gemm_cfg(); window(half, NCOPY)
                ta, tb = [], []
                for _ in range(rounds):
                    ta.append(window(x2, launches)); tb.append(window(half, launches))
                a, b = statistics.median(ta) * 1e6, statistics.median(tb) * 1e6
                print(f"{Cw:>5} {name:>5} {N:>5} {K:>5} {M:>5} {a:>9.1f} {b:>9.1f} {a / b:>6.2f} {2.0 * M * N * K / b * 1e-6:>12.0f} {str(kern['bm']) + '/' + str(kern['split']):>12} "
                      f"{NCOPY * N * K * 4 / 2 ** 20:>10.0f}")
                if b > a:
                    slower.setdefault(M, []).append((Cw, name, round(a / b, 3)))
            del Ws
    ok = [M for M in MS if all(m not in slower for m in MS if m >= M)]
    print("# half kernel slower at:", {m: v for m, v in sorted(slower.items())} or "no shape")
    print(f"# smallest M of the list from which the half kernel is not slower at any shape: {ok[0] if ok else 'none'}")
    return ok[0] if ok else None


def end_to_end(dev, rounds, steps, warmup, min_ms):
    from sdvar_amd.ladder import LADDER_256, as_ladder
    from sdvar_amd.vqvae import VQVAE
    from sdvar_amd.weights import vae_state_dict, var_state_dict_device
    pns, B, CFG, lad = LADDER_256, 8, 1.5, as_ladder(LADDER_256)
    sd_d, sd_t = var_state_dict_device(12, pns, dev, seed=1234), var_state_dict_device(16, pns, dev, seed=1234)
    sd_v = vae_state_dict(pns, "perf", 1234, with_encoder=False)
    vae = VQVAE(vocab_size=4096, z_channels=32, ch=160, v_patch_nums=pns, with_encoder=False)
    vae.load_state_dict(sd_v); vae = vae.to(dev)
    labels = (torch.arange(B) % 1000).to(dev)
    main, dec = torch.cuda.current_stream(), torch.cuda.Stream(device=dev)
    fh = [torch.zeros(B, 32, lad.HW, lad.HW, device=dev) for _ in range(2)]
    done, state = [None, None], {"i": 0}

    def with_decode(res):                                                  # bench.py's step: the decode of batch i on a second stream, under the sampling of batch i + 1
        j = state["i"] & 1; state["i"] += 1
        if done[j] is not None:
            main.wait_event(done[j])
        fh[j].copy_(res.f_hat)
        ready = torch.cuda.Event(); ready.record(main)
        dec.wait_event(ready)
        with torch.cuda.stream(dec):
            vae.fhat_to_img(fh[j]).add_(1).mul_(0.5)
            done[j] = torch.cuda.Event(); done[j].record(dec)

    runs, keep = {}, []
    for mode in ("f16x2", "f16"):
        dc, tc = E.ModelCtx(sd_d, 12, pns, B, 1, dev, gemm_mode=mode), E.ModelCtx(sd_t, 16, pns, B, 2, dev, gemm_mode=mode)
        qc = E.QuantCtx(sd_v, pns, B, dev)
        sp, pl = E.Sampler(tc, qc, dc), E.Sampler(tc, qc)
        tf = E.ModelCtx(sd_t, 16, pns, 16, lad.S, dev, gemm_mode=mode)
        xv, lab32 = torch.randn(32, lad.L - 1, 32, device=dev), (torch.arange(32) % 1000).to(dev)
        xb, lg = torch.empty(32, lad.L, 1024, device=dev), torch.empty(32, lad.L, 4096, device=dev)

        def p1(i, sp=sp):
            with_decode(sp.spec_decode(labels, CFG, 2, 900, 0.96, E.Noise("device", i), thr=0.5))

        def plain(i, pl=pl):
            with_decode(pl.plain_ar(labels, CFG, 900, 0.96, E.Noise("device", i)))

        def teach(i, tf=tf, xv=xv, lab32=lab32, xb=xb, lg=lg):
            tf.begin_rows(lab32); tf.embed_teacher(xv, xb); tf.forward(xb, 0, lad.S, lg); tf.kv_set_len(0)
        runs[mode] = dict(p1=p1, plain=plain, teach=teach)
        keep.append((dc, tc, qc, tf))
    cases = [("f16x2", "f16x2", None)] + [(f"f16 @ {m}", "f16", m) for m in min_ms]
    print(f"# 2. end to end: ms per step, median of {rounds} alternating windows of {steps} steps ({warmup} warm-up steps per case, one more after every switch of h16_min_m)")
    print("# ratio = f16x2 / f16: above 1 the f16 mode is faster")
    names = dict(p1="P1 step (d12 -> d16, B = 8, decode)", plain="plain d16 AR (B = 8, decode)", teach="teacher forcing d16, 32 images")
    print(f"{'workload':>36} " + " ".join(f"{c[0] + ' ms':>16}" for c in cases) + " " + " ".join(f"{'ratio ' + c[0][4:]:>14}" for c in cases[1:]) + "   spread")

    def switch(c):
        if c[2] is not None:
            E.set_variant("h16_min_m", c[2])
    for wl in ("p1", "plain", "teach"):
        t = {c[0]: [] for c in cases}
        for c in cases:
            switch(c); window(runs[c[1]][wl], warmup)
        for _ in range(rounds):
            for c in cases:
                switch(c); window(runs[c[1]][wl], 1)
                t[c[0]].append(window(runs[c[1]][wl], steps))
        med = {k: statistics.median(v) * 1e3 for k, v in t.items()}
        spread = max(max(v) / min(v) for v in t.values())
        print(f"{names[wl]:>36} " + " ".join(f"{med[c[0]]:>16.2f}" for c in cases) + " " + " ".join(f"{med['f16x2'] / med[c[0]]:>14.3f}" for c in cases[1:]) + f"   {spread:.3f}")
    E.set_variant("h16_min_m", -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-m", type=int, nargs="+", default=[2704, 1600, 1024, 576], help="h16_min_m values of the end-to-end runs in mode f16")
    ap.add_argument("--skip-gemm", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("f16_mode_bench: no GPU - timings are taken on an MI355X only")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    lib = E.load_library()
    print(f"# {torch.cuda.get_device_name(dev)}; GEMM modes f16x2 and f16 alternating in one process")
    if not a.skip_gemm:
        per_gemm(lib, dev, a.rounds, a.launches)
    if not a.skip_e2e:
        end_to_end(dev, a.rounds, a.steps, a.warmup, a.min_m)


if __name__ == "__main__":
    main()
