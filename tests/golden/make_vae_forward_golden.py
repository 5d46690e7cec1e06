#!/usr/bin/env python3
"""Generate tests/golden/vae_forward_256*.npz by running the REFERENCE VQVAE.forward (imported from /root/reference, CPU) on seeded weights.

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_vae_forward_golden.py
The reference never travels to the GPU box; only the .npz outputs (data) are committed.

The case is encode_256 of make_encode_golden.py again (same wseed / iseed, B = 2, ch = 160, its images): that case's ids are proven stable
within its f_tol, and this generator asserts that the reference's ids are encode_256's.  What is new is VQVAE.forward(x, ret_usages=True)
in eval mode (vqvae.py:56-59, quant.py:52-104):

  * ema_vocab_hit_SV is loaded with a seeded array, uniform in [0, 2 margin], margin = world (B H W) / V * 0.08 = 0.01 (quant.py:100); nothing is
    written if an entry lies within 1e-6 of the margin, so the fp32 comparison cannot fall either way (seeds are tried in order from EMA_SEED).
  * tdist.get_world_size() (quant.py:100) needs a process group: a single-rank gloo group on a file store (local, no network).

Recorded: vq_loss; usages; the straight-through f_hat (quant.py:98); rec of image 0, unclamped, and the number of its values outside [-1, 1];
the ema array; mse64[s], the fp64 mean of (f_hat_s - f)^2 over the reference's f_to_idxBl_or_fhat(to_fhat=True); the bincount of every scale's ids.
The reference's fp32 vq_loss must agree with (1 + beta) / S * sum mse64 to 1e-5 relative (asserted).
"""
import os
import sys
import tempfile
import time

import numpy as np
import torch
import torch.distributed as tdist

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")

import models as ref_models                      # noqa: E402  (the reference)
from sdvar_amd.weights import vae_state_dict     # noqa: E402

torch.set_grad_enabled(False)
torch.set_num_threads(8)
EMA_SEED = 4242
V, BETA = 4096, 0.25


def main():
    enc = dict(np.load(os.path.join(OUT, "encode_256.npz"), allow_pickle=False))
    enc.update(np.load(os.path.join(OUT, "encode_256.img.npz"), allow_pickle=False))
    pns = tuple(int(p) for p in enc["patch_nums"])
    wseed, iseed = int(enc["wseed"]), int(enc["iseed"])
    S = len(pns)
    sd = vae_state_dict(pns, "perf", wseed, with_encoder=True)
    vae = ref_models.VQVAE(vocab_size=V, z_channels=32, ch=160, beta=BETA, test_mode=True, share_quant_resi=4, v_patch_nums=pns)
    vae.load_state_dict(sd, strict=True)
    vae.eval()
    x = torch.from_numpy(enc["img_u8"]).float() / 127.5 - 1.0
    B, HW = x.shape[0], pns[-1]

    margin = 1 * (B * HW * HW) / V * 0.08
    # S V = 40960 draws over a range of 0.02 put ~4 entries within 1e-6 of the margin on average: seeds are tried in order, as make_encode_golden.py does
    for ema_seed in range(EMA_SEED, EMA_SEED + 2000):
        g = np.random.Generator(np.random.Philox(key=[ema_seed, 99]))
        ema = g.uniform(0.0, 2.0 * margin, size=(S, V)).astype(np.float32)
        if np.abs(ema.astype(np.float64) - margin).min() > 1e-6:
            break
    else:
        raise SystemExit("no ema seed keeps every entry 1e-6 away from the margin: nothing written")
    vae.quantize.ema_vocab_hit_SV.copy_(torch.from_numpy(ema))

    os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
    store_dir = tempfile.mkdtemp()
    tdist.init_process_group("gloo", store=tdist.FileStore(os.path.join(store_dir, "store"), 1), rank=0, world_size=1)
    assert tdist.get_world_size() == 1

    seen = {}
    hook = vae.quantize.register_forward_hook(lambda m, args, out: seen.update(f=args[0].clone(), f_hat=out[0].clone()))
    t0 = time.time()
    rec, usages, vq_loss = vae(x, ret_usages=True)
    hook.remove()
    f, f_st = seen["f"], seen["f_hat"]
    assert np.array_equal(f.numpy(), enc["f"]), "the reference's f differs from encode_256's"

    ids = vae.img_to_idxBl(x)
    assert np.array_equal(torch.cat(ids, 1).numpy(), enc["ids"]), "the reference's ids differ from encode_256's"
    hits = np.stack([np.bincount(t.reshape(-1).numpy(), minlength=V) for t in ids]).astype(np.int32)
    assert [int(h.sum()) for h in hits] == [B * p * p for p in pns]

    fh = vae.quantize.f_to_idxBl_or_fhat(f, to_fhat=True)
    mse64 = np.array([float(((t.double() - f.double()) ** 2).mean()) for t in fh])
    want = (1.0 + BETA) / S * float(mse64.sum())
    rel = abs(float(vq_loss) - want) / want
    assert rel <= 1e-5, f"vq_loss {float(vq_loss)} vs (1 + beta) / S sum mse64 {want}: rel {rel:.2e}"
    want_usage = [float((ema[s] >= np.float32(margin)).mean()) * 100 for s in range(S)]
    assert np.allclose(usages, want_usage, rtol=0, atol=1e-9), (usages, want_usage)
    # the straight-through value is not the accumulator itself
    assert not torch.equal(f_st, fh[-1]) and torch.equal(f_st, (fh[-1] - f) + f)

    rec0 = rec[0].numpy()
    out = dict(patch_nums=np.array(pns), wseed=np.array(wseed), iseed=np.array(iseed), beta=np.array(BETA), ema_seed=np.array(ema_seed),
               margin=np.array(margin), vq_loss=np.array(float(vq_loss)), usages=np.array(usages, dtype=np.float64), f_hat_st=f_st.numpy(),
               ema=ema, mse64=mse64, hits=hits, rec0_outside=np.array(int((np.abs(rec0) > 1).sum())))
    np.savez_compressed(os.path.join(OUT, "vae_forward_256.npz"), **out)
    np.savez_compressed(os.path.join(OUT, "vae_forward_256.rec.npz"), rec0=rec0)
    for fn in ("vae_forward_256.npz", "vae_forward_256.rec.npz"):
        sz = os.path.getsize(os.path.join(OUT, fn))
        assert sz < 1 << 20, f"{fn}: {sz} bytes"
        print(f"[vae forward golden] {fn}: {sz} bytes")
    print(f"[vae forward golden] {time.time() - t0:.1f}s vq_loss {float(vq_loss):.6f} (rel. to fp64 {rel:.1e}), usages {' '.join(f'{u:.2f}' for u in usages)}, "
          f"|rec0| max {np.abs(rec0).max():.3f}, {int(out['rec0_outside'])} values outside [-1, 1], mse64 {' '.join(f'{m:.3e}' for m in mse64)}")
    tdist.destroy_process_group()


if __name__ == "__main__":
    main()
