"""GPU: the masked sampler loop (Sampler.plain_ar(force_ids, gen)) and the public call VAR.autoregressive_infer_cfg_edit.
The yardstick is the masked oracle loop of tests/edit_cases.py (orc.plain_ar's loop with ids = where(gen, sampled, force_ids)), run once per image with that
image's noise stream; the seeds were picked on the CPU so that no sampled token is within MIN_MARGIN of a tie (tests/test_edit_host.py), so ids are compared
bit for bit with no token excused.  The d4 `stress` model on LADDER_256, B <= 3; the public call on a ch = 32 VQVAE with its encoder."""
import numpy as np
import pytest
import torch

import edit_cases as EC
import sampler_hard_cases as H
from conftest import state_dicts
from oracle import var_oracle as orc
from sdvar_amd import engine as E
from sdvar_amd.ladder import LADDER_256

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
LAD = EC.LAD
FHAT_TOL, IMG_TOL = 1e-4, 1e-4          # the project's bars (tests/test_gpu_e2e.py, tests/test_gpu_vae_encode.py)
PLAIN = (1.5, 900, 0.96)


@pytest.fixture(scope="module")
def models(dev):
    sd4, sdv = state_dicts(EC.DEPTH, LADDER_256)
    ctxs = {mode: E.ModelCtx(sd4, EC.DEPTH, LADDER_256, 3, 1, dev, gemm_mode=mode) for mode in (None, "bf16x3")}
    qc = E.QuantCtx(sdv, LADDER_256, 3, dev)
    yield dict(sdv=sdv, default=E.Sampler(ctxs[None], qc), bf16x3=E.Sampler(ctxs["bf16x3"], qc))
    for c in ctxs.values():
        c.close()
    qc.close()


def _snap(res):
    return res.ids.clone(), res.f_hat.clone()


# ------------------------------------------------------------------------------------------------ the engine loop
def test_all_ones_gen_is_the_unmasked_call(dev, models):
    smp, lab = models["default"], torch.tensor(EC.LABELS3, device=dev)
    ids0, f0 = _snap(smp.plain_ar(lab, *PLAIN, E.Noise("device", 31)))
    ones = torch.ones(3, LAD.L, dtype=torch.uint8, device=dev)
    ids1, f1 = _snap(smp.plain_ar(lab, *PLAIN, E.Noise("device", 31), force_ids=EC.random_ids(3).to(dev), gen=ones))
    assert torch.equal(ids0, ids1) and torch.equal(H.bits(f0), H.bits(f1))
    ids2, f2 = _snap(smp.plain_ar(lab, [1.5] * 3, [900] * 3, [0.96] * 3, E.Noise("device", [31] * 3, [0, 1, 2]), force_ids=EC.random_ids(3).to(dev), gen=ones))
    assert torch.equal(ids0, ids2) and torch.equal(H.bits(f0), H.bits(f2))                          # ... through the rows entry point too


def test_all_zeros_gen_forces_every_token(dev, models):
    smp, lab = models["default"], torch.tensor(EC.LABELS3, device=dev)
    force = EC.random_ids(3)
    res = smp.plain_ar(lab, *PLAIN, E.Noise("device", 31), force_ids=force.to(dev), gen=torch.zeros(3, LAD.L, dtype=torch.uint8, device=dev))
    assert torch.equal(res.ids.cpu(), force)
    want = EC.accumulate_ids(orc.OracleQuant(models["sdv"], LADDER_256), force)
    err = float((res.f_hat.cpu() - want).abs().max())
    print("all-forced f_hat max|diff| vs the oracle's accumulation:", err)
    assert err <= FHAT_TOL


def _against_oracle(res, case, what):
    ids, f_hat = res.ids.cpu(), res.f_hat.cpu()
    gen, force = EC.gen_table(), EC.random_ids(3)
    for b, im in enumerate(case):
        tr = EC.oracle_run(im, b)
        assert torch.equal(ids[b:b + 1], tr.ids), f"{what}: image {b} ({im.mask}): ids differ from the masked oracle loop"
        assert torch.equal(ids[b][gen[b] == 0], force[b][gen[b] == 0])
        err = float((f_hat[b] - tr.f_hat[0]).abs().max())
        print(f"{what}: image {b} ({im.mask}) f_hat max|diff| {err:.3g}")
        assert err <= FHAT_TOL, f"{what}: image {b}: f_hat off by {err}"


@pytest.mark.parametrize("mode", ["default", "bf16x3"])
def test_three_masks_in_one_batch_are_the_masked_oracle_per_image(dev, models, mode):
    """Hole, its inverse and a thin strip, random forced ids; one seed, image b at noise index b."""
    smp, lab = models[mode], torch.tensor(EC.LABELS3, device=dev)
    gen, force = EC.gen_table().to(dev), EC.random_ids(3).to(dev)
    res = smp.plain_ar(lab, *PLAIN, E.Noise("host", EC.SCALAR_SEED), force_ids=force, gen=gen)
    _against_oracle(res, EC.SCALAR, f"{mode} host noise")
    ids, f = _snap(res)
    res2 = smp.plain_ar(lab, *PLAIN, E.Noise("device", EC.SCALAR_SEED), force_ids=force, gen=gen)               # the in-kernel Philox stream: the same draws
    assert torch.equal(res2.ids, ids) and torch.equal(H.bits(res2.f_hat), H.bits(f))
    res3 = smp.plain_ar(lab, *PLAIN, E.Noise("device", EC.SCALAR_SEED), force_ids=force, gen=gen)               # a repeat is bit-identical
    assert torch.equal(res3.ids, ids) and torch.equal(H.bits(res3.f_hat), H.bits(f))
    assert res.stats["target_calls"] == LAD.S and smp.t.kv_len() == 0


def test_per_image_parameters_with_masks_take_the_rows_entry_point(dev, models):
    smp, lab = models["default"], torch.tensor([im.label for im in EC.ROWS], device=dev)
    gen, force = EC.gen_table().to(dev), EC.random_ids(3).to(dev)
    cfg, top_k, top_p, seeds = ([getattr(im, k) for im in EC.ROWS] for k in ("cfg", "top_k", "top_p", "seed"))
    assert E.RowParams.build(3, LAD, cfg, top_k, top_p, E.Noise("host", seeds)) is not None
    res = smp.plain_ar(lab, cfg, top_k, top_p, E.Noise("host", seeds), force_ids=force, gen=gen)
    _against_oracle(res, EC.ROWS, "rows")
    ids = res.ids.clone()
    assert torch.equal(smp.plain_ar(lab, cfg, top_k, top_p, E.Noise("device", seeds), force_ids=force, gen=gen).ids, ids)


def test_masked_call_refusals(dev, models):
    smp, lab = models["default"], torch.tensor(EC.LABELS3, device=dev)
    gen, force = EC.gen_table().to(dev), EC.random_ids(3).to(dev)
    noise = E.Noise("device", 1)
    before = smp.ids.clone()
    with pytest.raises(E.SdvarError, match="more_smooth"):
        smp.plain_ar(lab, *PLAIN, noise, more_smooth=True, force_ids=force, gen=gen)
    for bad_id in (-1, EC.V):
        bad = force.clone(); bad[1, 77] = bad_id
        with pytest.raises(E.SdvarError, match="force_ids"):
            smp.plain_ar(lab, *PLAIN, noise, force_ids=bad, gen=gen)
    with pytest.raises(E.SdvarError, match="go together"):
        smp.plain_ar(lab, *PLAIN, noise, gen=gen)
    with pytest.raises(E.SdvarError, match="gen"):
        smp.plain_ar(lab, *PLAIN, noise, force_ids=force, gen=gen.to(torch.int64))
    with pytest.raises(E.SdvarError, match="force_ids has shape"):
        smp.plain_ar(lab, *PLAIN, noise, force_ids=force[:2], gen=gen)
    with pytest.raises(E.SdvarError, match="gen is on cpu"):
        smp.plain_ar(lab, *PLAIN, noise, force_ids=force, gen=gen.cpu())
    torch.cuda.synchronize()
    assert torch.equal(smp.ids, before) and smp.t.kv_len() == 0                                          # nothing ran


# ------------------------------------------------------------------------------------------------ the public call
@pytest.fixture(scope="module")
def pub(dev):
    vae, var = EC.build_var(dev)
    return dict(vae=vae, var=var, image=EC.sample_image(3).to(dev))


def _unit(x):
    return x.add(1).mul(0.5)


def test_edit_composite_keeps_the_bits_outside_the_mask(dev, pub):
    vae, var, image = pub["vae"], pub["var"], pub["image"][:2].contiguous()
    hole = torch.from_numpy(EC.masks()["hole"]).to(dev)
    out = var.autoregressive_infer_cfg_edit(image, hole.bool(), 3, g_seed=1, cfg=1.5, top_k=900, top_p=0.96)          # a 2-D bool mask serves both images
    res = var.last_result
    assert out.shape == (2, 3, 256, 256) and out.dtype == torch.float32
    m = (hole != 0)[None, None].expand_as(out)
    assert torch.equal(H.bits(out[~m].cpu()), H.bits(_unit(image)[~m].cpu())), "a kept pixel is not the input's"
    plain = _unit(vae.fhat_to_img(res.f_hat.clone()))
    assert torch.equal(H.bits(out[m].cpu()), H.bits(plain[m].cpu())), "a regenerated pixel is not the plain decode of f_hat"
    want_gen = torch.from_numpy(EC.mask_tokens_np(EC.masks()["hole"], LADDER_256)).expand(2, -1)
    assert res.gen.dtype == torch.uint8 and torch.equal(res.gen.cpu(), want_gen)
    own = torch.cat(vae.img_to_idxBl(image), 1)
    keep = res.gen == 0
    assert torch.equal(res.ids[keep], own[keep]) and res.ids.shape == (2, LAD.L)
    assert res.stats["target_calls"] == LAD.S
    out2 = var.autoregressive_infer_cfg_edit(image, hole, 3, g_seed=1, cfg=1.5, top_k=900, top_p=0.96)               # uint8, and a repeat: the same bits
    assert torch.equal(H.bits(out2.cpu()), H.bits(out.cpu()))


def test_edit_with_nothing_to_regenerate_is_the_reconstruction(dev, pub):
    vae, var, image = pub["vae"], pub["var"], pub["image"][:1].contiguous()
    out = var.autoregressive_infer_cfg_edit(image, torch.zeros(1, 1, 256, 256, dtype=torch.bool, device=dev), 3, g_seed=1, composite=False)
    want = _unit(vae.idxBl_to_img(vae.img_to_idxBl(image), same_shape=True, last_one=True))
    err = float((out - want).abs().max())
    print("all-kept edit vs idxBl_to_img(img_to_idxBl(image)): max|diff|", err)
    assert err <= IMG_TOL
    assert int(var.last_result.gen.sum()) == 0


def test_class_edit_in_a_box_changes_the_box_only(dev, pub):
    """B = 3, one (B, 1, H, H) uint8 mask per image (the box, the strip, the box), another label, per-image cfg / top_k / top_p / seeds."""
    var, image = pub["var"], pub["image"]
    ms = EC.masks()
    mask = torch.from_numpy(np.stack([ms["box"], ms["strip"], ms["box"]])[:, None]).to(dev)
    out = var.autoregressive_infer_cfg_edit(image, mask, torch.tensor([977, 3, 500]), g_seed=[5, 6, 7], cfg=[1.5, 3.0, 0.75], top_k=[900, 0, 40], top_p=[0.96, 0.0, 0.5])
    assert out.shape == (3, 3, 256, 256) and bool(torch.isfinite(out).all()) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    m = (mask != 0).expand_as(out)
    inp = _unit(image)
    assert torch.equal(H.bits(out[~m].cpu()), H.bits(inp[~m].cpu()))
    for b in range(3):
        assert bool((out[b][m[b]] != inp[b][m[b]]).any()), f"image {b}: nothing changed inside its mask"
    assert torch.equal(var.last_result.gen.cpu(), torch.from_numpy(EC.mask_tokens_np(mask[:, 0].cpu().numpy(), LADDER_256)))


def test_edit_refusals(dev, pub):
    var, image = pub["var"], pub["image"][:2].contiguous()
    mask = torch.zeros(2, 256, 256, dtype=torch.bool, device=dev)
    with pytest.raises(E.SdvarError, match="more_smooth"):
        var.autoregressive_infer_cfg_edit(image, mask, 3, more_smooth=True)
    with pytest.raises(E.SdvarError, match="image is on cpu"):
        var.autoregressive_infer_cfg_edit(image.cpu(), mask, 3)
    with pytest.raises(E.SdvarError, match="mask is on cpu"):
        var.autoregressive_infer_cfg_edit(image, mask.cpu(), 3)
    with pytest.raises(E.SdvarError, match="image must be"):
        var.autoregressive_infer_cfg_edit(image.double(), mask, 3)
    with pytest.raises(E.SdvarError, match="image must be"):
        var.autoregressive_infer_cfg_edit(image[:, :2], mask, 3)
    with pytest.raises(E.SdvarError, match="image is 128 x 128"):
        var.autoregressive_infer_cfg_edit(image[:, :, :128, :128], mask[:, :128, :128], 3)
    with pytest.raises(E.SdvarError, match="mask must be"):
        var.autoregressive_infer_cfg_edit(image, mask.float(), 3)
    with pytest.raises(E.SdvarError, match="mask has shape"):
        var.autoregressive_infer_cfg_edit(image, mask[:1], 3)
    with pytest.raises(E.SdvarError, match="image: a batch of 70000"):
        var.autoregressive_infer_cfg_edit(image[:1].expand(70000, 3, 256, 256), mask[0], 3)
    with pytest.raises(E.SdvarError, match="top_k"):
        var.autoregressive_infer_cfg_edit(image, mask, 3, g_seed=1, top_k=[900, 0, 1])
    with pytest.raises(E.SdvarError, match="label_B"):
        var.autoregressive_infer_cfg_edit(image, mask, None, g_seed=[1, 2])
    vae2, var2 = EC.build_var(dev, with_encoder=False)
    with pytest.raises(E.SdvarError, match="with_encoder=False"):
        var2.autoregressive_infer_cfg_edit(image, mask, 3)
