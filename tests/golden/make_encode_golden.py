#!/usr/bin/env python3
"""Generate tests/golden/encode_*.npz by running the REFERENCE VQVAE image side (imported from /root/reference, CPU) on seeded weights.

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_encode_golden.py
The reference never travels to the GPU box; only the .npz outputs (data) are committed.  Cases: 256^2 B = 2 and 512^2 B = 1, the
full-width VQVAE (ch = 160) with the 'perf' init of sdvar_amd.weights.vae_state_dict, loaded into models.VQVAE with strict=True.

Test images are procedural: a few low-frequency sinusoids plus noise, quantised to uint8 and stored as uint8; x = u8 / 127.5 - 1.

Recorded per case: f = quant_conv(encoder(x)); the ids of every scale (img_to_idxBl); f_hat after scales PER_SCALE and the final f_hat
(f_to_idxBl_or_fhat(to_fhat=True)); idxBl_to_var_input; at 256^2 image 0 of img_to_reconstructed_img(last_one=True); and the fp64
top-2 distance margin of every row along the reference's own chain.

Margin threshold.  The GPU test compares f within F_TOL (max abs).  A row z of a scale is an area average of f_rest, so |dz|_inf <= F_TOL
and |dz|_2 <= sqrt(Cvae) F_TOL.  The distance to code e is |z|^2 + |e|^2 - 2 z.e, so |dd| <= 2 |z - e| |dz|_2 for one code; the GAP
d_2 - d_1 between the two nearest codes is linear in z (the |z|^2 terms cancel): d_2 - d_1 = |e_2|^2 - |e_1|^2 - 2 z.(e_2 - e_1), so it moves by
exactly |2 dz.(e_2 - e_1)| <= 2 |e_1 - e_2| sqrt(Cvae) F_TOL.  A case is written only if every row's gap is at least SAFETY times that bound;
then no f within F_TOL can flip an id, and the chain of scales stays the reference's.  Seeds are tried in order.
The cases have 679 (256^2) / 2240 (512^2) rows per image against 4096 random codes and their smallest relative gaps are ~1e-5 .. 1e-6
(gap / (|z|^2 + mean |e|^2); recorded in `min_rel_margin_per_scale`), so the 10x margin over a 1e-4 tolerance on f that one would like is
out of reach: F_TOL = F_REL max(1, max |f|) with F_REL = 1e-5 (the measured GPU error of f is 4e-6 .. 1.2e-5 at max |f| 1.3 .. 2.4) and SAFETY = 1
against a worst case that assumes the whole error vector of z aligned with e_1 - e_2 (a random error is ~sqrt(Cvae) smaller).  `f_tol` records
the case's F_TOL, `margin_safety` min gap / bound (>= 1).
"""
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")

import models as ref_models                      # noqa: E402  (the reference)
from sdvar_amd.ladder import LADDER_256, LADDER_512   # noqa: E402
from sdvar_amd.weights import vae_state_dict     # noqa: E402

torch.set_grad_enabled(False)
torch.set_num_threads(8)
F_REL = 1e-5
SAFETY = 1.0
PER_SCALE = (0, 4, 8)


def test_images(seed: int, B: int, H: int) -> np.ndarray:
    """(B, 3, H, H) uint8: sinusoids of 1..4 periods per side with random phases and amplitudes, plus Gaussian noise."""
    g = np.random.Generator(np.random.Philox(key=[seed, 777]))
    yy, xx = np.meshgrid(np.arange(H) / H, np.arange(H) / H, indexing="ij")
    out = np.zeros((B, 3, H, H), dtype=np.float64)
    for b in range(B):
        for c in range(3):
            v = np.full((H, H), 0.5)
            for _ in range(4):
                fy, fx = g.integers(0, 5, size=2)
                v += g.uniform(0.05, 0.2) * np.sin(2 * np.pi * (fy * yy + fx * xx) + g.uniform(0, 2 * np.pi))
            out[b, c] = v + g.normal(0, 0.04, size=(H, H))
    return np.clip(np.rint(out * 255.0), 0, 255).astype(np.uint8)


def margin_bound_ok(vae, rows_margins, f_tol):
    """(ok, smallest gap / bound over all rows) for the threshold of the module docstring."""
    worst = math.inf
    for gap, _, de in rows_margins:
        bound = 2.0 * de * math.sqrt(vae.Cvae) * f_tol
        worst = min(worst, float((gap / (SAFETY * bound)).min()))
    return worst >= 1.0, worst


def build_case(pns, B, wseed, iseed):
    from torch_ref_encode import f_to_idxBl_or_fhat_torch
    from sdvar_amd.vqvae import VQVAE as OurVQVAE
    sd = vae_state_dict(pns, "perf", wseed, with_encoder=True)
    vae = ref_models.VQVAE(vocab_size=4096, z_channels=32, ch=160, test_mode=True, share_quant_resi=4, v_patch_nums=pns)
    vae.load_state_dict(sd, strict=True)
    H = pns[-1] * 16
    u8 = test_images(iseed, B, H)
    x = torch.from_numpy(u8).float() / 127.5 - 1.0
    t0 = time.time()
    f = vae.quant_conv(vae.encoder(x))
    ids = vae.img_to_idxBl(x)
    fh = vae.quantize.f_to_idxBl_or_fhat(f, to_fhat=True)
    var_in = vae.quantize.idxBl_to_var_input(ids)
    # the fp64 margins along the reference's chain: the restatement reproduces its ids (checked), so its rows are the reference's rows
    ours = OurVQVAE(vocab_size=4096, z_channels=32, ch=160, v_patch_nums=pns)
    ours.load_state_dict(sd, strict=True)
    rows = []
    ids_t = f_to_idxBl_or_fhat_torch(ours, f, False, margins=rows)
    assert all(torch.equal(a, b) for a, b in zip(ids, ids_t)), "torch restatement ids differ from the reference"
    f_tol = F_REL * max(1.0, float(f.abs().max()))
    ok, worst = margin_bound_ok(vae, rows, f_tol)
    rel = [float((gap / s).min()) for gap, s, _ in rows]
    out = dict(patch_nums=np.array(pns), wseed=np.array(wseed), iseed=np.array(iseed), img_u8=u8, f=f.numpy(),
               ids=torch.cat(ids, 1).numpy(), f_hat=fh[-1].numpy(), per_scale=np.array(PER_SCALE),
               f_hat_per_scale=np.stack([fh[s].numpy() for s in PER_SCALE]), var_input=var_in.numpy(),
               rel_margin=np.concatenate([gap / s for gap, s, _ in rows]).astype(np.float32), min_rel_margin_per_scale=np.array(rel),
               f_tol=np.array(f_tol), margin_safety=np.array(worst))
    if H == 256:
        out["recon0"] = vae.img_to_reconstructed_img(x[:1], last_one=True)[0].numpy()
    print(f"[encode golden] {H}^2 B={B} wseed {wseed} iseed {iseed}: {time.time() - t0:.1f}s |f| max {f.abs().max():.3f}, "
          f"min rel margin per scale {' '.join(f'{m:.1e}' for m in rel)}, gap / bound {worst:.2f}")
    return ok, out


def save(name, out, parts):
    """name.npz + name.<part>.npz (tests/conftest.py golden_parts), each under 1 MiB."""
    main = {k: v for k, v in out.items() if not any(k in p for p in parts.values())}
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **main)
    parts = {p: keys for p, keys in parts.items() if any(k in out for k in keys)}
    for pname, keys in parts.items():
        np.savez_compressed(os.path.join(OUT, f"{name}.{pname}.npz"), **{k: out[k] for k in keys if k in out})
    for f in [name + ".npz"] + [f"{name}.{p}.npz" for p in parts]:
        sz = os.path.getsize(os.path.join(OUT, f))
        assert sz < 1 << 20, f"{f}: {sz} bytes"


def main():
    for pns, B, name in ((LADDER_256, 2, "encode_256"), (LADDER_512, 1, "encode_512")):
        for trial in range(40):
            ok, out = build_case(pns, B, 1234 + trial, 10 + trial)
            if ok:
                break
        else:
            raise SystemExit(f"{name}: no seed with every top-2 margin above the threshold")
        save(name, out, {"img": ("img_u8",), "recon": ("recon0",)})


if __name__ == "__main__":
    main()
