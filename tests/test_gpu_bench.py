"""bench.py's plain run in a fresh process: the headline fields of its result line, the extras left to --full, and --dump-outputs holding exactly what
the timed path returned in its last step (recomputed here with the same weights, labels and noise seed)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_bench_plain_run_and_dump(dev, tmp_path):
    B, steps, warmup = 2, 2, 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--batch", str(B),
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["steps"] == steps and out["warmup"] == warmup and out["unit"] == "images/s" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0 and out["value"] > 0 and out["metric"].startswith("images/s") and out["dtype"].startswith("f32")
    assert not {"modes", "roofline", "cpu_baseline", "images_per_s_no_decode"} & set(out)          # measured with --full only
    got = {n: np.load(tmp_path / f"{n}.npy") for n in ("images", "ids", "f_hat")}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["images"].shape == (B, 3, 256, 256) and got["ids"].shape == (B, 680) and got["f_hat"].shape == (B, 32, 16, 16)

    from sdvar_amd import engine as E
    from sdvar_amd.ladder import LADDER_256
    from sdvar_amd.vqvae import VQVAE
    from sdvar_amd.weights import vae_state_dict, var_state_dict_device
    torch.set_grad_enabled(False)
    pns = LADDER_256
    sd_v = vae_state_dict(pns, "perf", 1234, with_encoder=False)
    vae = VQVAE(vocab_size=4096, z_channels=32, ch=160, v_patch_nums=pns, with_encoder=False)
    vae.load_state_dict(sd_v); vae = vae.to(dev)
    dc = E.ModelCtx(var_state_dict_device(12, pns, dev, seed=1234), 12, pns, B, 1, dev)
    tc = E.ModelCtx(var_state_dict_device(16, pns, dev, seed=1234), 16, pns, B, 2, dev)
    qc = E.QuantCtx(sd_v, pns, B, dev)
    try:
        res = E.Sampler(tc, qc, dc).spec_decode(torch.arange(B, device=dev), 1.5, 2, 900, 0.96, E.Noise("device", 1000 + steps - 1), thr=0.5, run_ahead=True)
        img = vae.fhat_to_img(res.f_hat).add_(1).mul_(0.5)
        torch.cuda.synchronize()
        assert np.array_equal(got["ids"], res.ids.float().cpu().numpy())
        assert np.array_equal(got["f_hat"], res.f_hat.cpu().numpy())
        assert np.abs(got["images"] - img.cpu().numpy()).max() < 1e-5
    finally:
        dc.close(); tc.close(); qc.close(); torch.cuda.empty_cache()
