"""VQVAE.forward on the GPU (vqvae.py:56-59, quant.py:52-104): the statistics of the quantiser chain (sdvar_quant_encode_stats), the unclamped decode
(sdvar_vae_decode_raw), the image error sums (sdvar_img_err_stats), and the public path - VQVAE.forward, Quantizer.forward, evaluate.eval_vae - against
the reference fixture of tests/golden/make_vae_forward_golden.py, in both convolution operand formats."""
import numpy as np
import pytest
import torch

from conftest import golden_parts, rnd

pytestmark = pytest.mark.gpu
MODES = ["f16x2", "bf16x3"]
LADDER_SMALL = (1, 2, 4)
_MEMO = {}


# ------------------------------------------------------------------------------------------------------------- 1. encode_stats against encode
def _quant(dev, pns, V, B):
    from sdvar_amd import engine as E
    from sdvar_amd.weights import vae_state_dict
    sd = vae_state_dict(pns, "stress", 21, V=V, Cvae=32, ch=32, with_encoder=False)
    return E.QuantCtx(sd, pns, B, dev), sd


def _check_stats(ctx, f, pns, V):
    B = f.shape[0]
    ids, f_hat, ps = ctx.encode(f, per_scale=True)
    ids2, f_hat2, ps2, hits, sqerr, f_st = ctx.encode_stats(f, per_scale=True, straight_through=True)
    assert torch.equal(ids2, ids) and torch.equal(f_hat2, f_hat) and torch.equal(ps2, ps)                # the same chain: the same bits
    assert hits.dtype == torch.int32 and tuple(hits.shape) == (len(pns), V) and sqerr.dtype == torch.float64 and tuple(sqerr.shape) == (len(pns),)
    off = 0
    for s, pn in enumerate(pns):
        want = torch.bincount(ids2[:, off:off + pn * pn].reshape(-1), minlength=V)                       # quant.py:77
        assert torch.equal(hits[s].long(), want) and int(hits[s].sum()) == B * pn * pn
        off += pn * pn
        ref = ((ps2[s].double() - f.double()) ** 2).sum().item()
        got = sqerr[s].item()
        print(f"scale {s}: sqerr {got:.9e} fp64 {ref:.9e} |diff| {abs(got - ref):.1e}")
        assert abs(got - ref) <= 1e-6 * ref                  # one fp32 rounding per difference (2^-24), doubled by the square: 1.2e-7
    assert torch.equal(f_st, (f_hat2 - f) + f)                                                           # quant.py:98, as written
    again = ctx.encode_stats(f, per_scale=False, straight_through=False)
    assert again[2] is None and again[5] is None and torch.equal(again[3], hits)
    assert torch.equal(again[4], sqerr)                                                                  # fixed-order reduction: bit-identical
    return ids2, hits


@pytest.mark.parametrize("variant", ["plain", "x1000", "one_code"])
def test_encode_stats_small(dev, variant):
    """Ladder (1, 2, 4), V = 64, B = 3: odd batch, 16-pixel planes, one workgroup per statistics pass; large residuals; every row on one code."""
    ctx, sd = _quant(dev, LADDER_SMALL, 64, 3)
    f = rnd(31, (3, 32, 4, 4)).to(dev)
    if variant == "x1000":
        f = f * 1e3
    if variant == "one_code":
        f = sd["quantize.embedding.weight"][7].to(dev).view(1, 32, 1, 1).expand(3, 32, 4, 4).contiguous()
    ids, hits = _check_stats(ctx, f, LADDER_SMALL, 64)
    if variant == "one_code":                                # scale 0: every image's single row lands in the same bin (contended atomics still count exactly)
        assert int(hits[0].max()) == 3 and int((hits[0] > 0).sum()) == 1


def test_encode_stats_ladder_256(dev):
    """LADDER_256, V = 4096, B = 2: 16384 elements -> 16 workgroups per statistics pass, ten scales, 1360 ids."""
    from sdvar_amd.ladder import LADDER_256
    ctx, _ = _quant(dev, LADDER_256, 4096, 2)
    _check_stats(ctx, rnd(32, (2, 32, 16, 16)).to(dev), LADDER_256, 4096)


# ------------------------------------------------------------------------------------------------------------- 2. raw decode
@pytest.mark.parametrize("cm", MODES)
def test_raw_decode_is_the_decode_without_the_clamp(dev, cm):
    from sdvar_amd import engine as E
    from sdvar_amd.vqvae import VQVAE
    from sdvar_amd.weights import vae_state_dict
    from torch_ref import fhat_to_img_torch
    pns = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
    sd = vae_state_dict(pns, "stress", 5, V=64, Cvae=32, ch=32, with_encoder=False)
    vae = VQVAE(vocab_size=64, z_channels=32, ch=32, v_patch_nums=pns, with_encoder=False)
    vae.load_state_dict(sd)
    vae = vae.to(dev)
    ctx = E.VaeCtx(sd, 2, dev, latent_hw=16, conv_mode=cm)
    f_hat = rnd(6, (2, 32, 16, 16), 3.0).to(dev)             # scaled: about an eighth of the outputs leave [-1, 1]
    raw = ctx.decode_raw(f_hat)
    got = ctx.decode(f_hat)
    print(f"{cm}: max|raw| {raw.abs().max().item():.3f}, {(raw.abs() > 1).float().mean().item():.3f} outside")
    assert raw.abs().max().item() > 1
    assert torch.equal(raw.clamp(-1, 1), got)
    assert torch.equal(ctx.decode(f_hat, clamp=False), raw)
    err = (got - fhat_to_img_torch(vae, f_hat.clone())).abs().max().item()
    assert err <= 1e-4, err                                  # the tolerance of test_gpu_vae.py


# ------------------------------------------------------------------------------------------------------------- 3. image error statistics
@pytest.mark.parametrize("n", [1, 4097, 2 * 3 * 256 * 256])
def test_img_err_stats(dev, n):
    from sdvar_amd import engine as E
    a, b = rnd(41, (n,)).to(dev), rnd(42, (n,)).to(dev)
    d = a.double() - b.double()
    ref = (d.abs().sum().item(), (d * d).sum().item())
    sums = torch.full((2,), 123.0, dtype=torch.float64, device=dev)
    E.img_err_stats(a, b, sums)                              # overwrites
    first = sums.clone()
    for k in range(2):
        print(f"n {n} sum[{k}]: {sums[k].item():.12e} fp64 {ref[k]:.12e}")
        assert abs(sums[k].item() - ref[k]) <= 1e-6 * ref[k]
    E.img_err_stats(a, b, sums, accumulate=True)             # adds: s + s is exact
    assert torch.equal(sums, 2 * first)
    E.img_err_stats(a, b, sums)
    assert torch.equal(sums, first)                          # bit-identical repeat
    if n > 1:                                                # a pointer that is not 16-byte aligned takes the scalar loads
        a1, b1 = a[1:], b[1:]
        d1 = a1.double() - b1.double()
        E.img_err_stats(a1, b1, sums)
        assert abs(sums[0].item() - d1.abs().sum().item()) <= 1e-6 * d1.abs().sum().item()
        assert abs(sums[1].item() - (d1 * d1).sum().item()) <= 1e-6 * (d1 * d1).sum().item()


# ------------------------------------------------------------------------------------------------------------- 4. / 5. the public path
def _model(dev):
    from sdvar_amd.vqvae import VQVAE
    from sdvar_amd.weights import vae_state_dict
    g, e = golden_parts("vae_forward_256"), golden_parts("encode_256")
    pns = tuple(int(p) for p in g["patch_nums"])
    assert int(g["wseed"]) == int(e["wseed"]) and int(g["iseed"]) == int(e["iseed"])
    if "sd" not in _MEMO:
        sd = dict(vae_state_dict(pns, "perf", int(g["wseed"]), with_encoder=True))
        sd["quantize.ema_vocab_hit_SV"] = torch.from_numpy(g["ema"])
        _MEMO["sd"] = sd
    vae = VQVAE(vocab_size=4096, ch=160, v_patch_nums=pns, beta=float(g["beta"])).to(dev)
    vae.load_state_dict(dict(_MEMO["sd"]), strict=True)
    x = (torch.from_numpy(e["img_u8"]).float() / 127.5 - 1.0).to(dev)
    return g, e, vae, x


@pytest.mark.parametrize("mode", MODES)
def test_forward_matches_reference(dev, monkeypatch, mode):
    monkeypatch.setenv("SDVAR_CONV_MODE", mode)
    g, e, vae, x = _model(dev)
    rec, usages, vq_loss = vae(x, ret_usages=True)
    S, beta = len(g["patch_nums"]), float(g["beta"])
    assert len(usages) == S and np.abs(np.array(usages) - g["usages"]).max() <= 1e-9
    assert vq_loss.dim() == 0 and vq_loss.dtype == torch.float32 and vq_loss.is_cuda
    f_st, usages_q, loss_q = vae.quantize(vae.img_to_f(x), ret_usages=True)
    assert usages_q == usages and torch.equal(loss_q, vq_loss)
    err_f = (f_st.cpu() - torch.from_numpy(g["f_hat_st"])).abs().max().item()
    want = float(g["vq_loss"])
    # Cauchy-Schwarz on the MSE when f_hat moves by at most 1e-5 per element, plus the reference's own fp32 summation error
    tol = (1 + beta) / S * float(np.sum(2 * np.sqrt(g["mse64"]) * 1e-5 + 1e-10)) + 1e-5 * want
    err_r = (rec[0].cpu() - torch.from_numpy(g["rec0"])).abs().max().item()
    print(f"{mode}: straight-through f_hat max|diff| {err_f:.2e}; vq_loss {vq_loss.item():.8f} vs {want:.8f} (tolerance {tol:.1e}); rec0 max|diff| {err_r:.2e}, "
          f"max|rec| {rec.abs().max().item():.3f}")
    assert err_f <= 1e-5                                     # the tolerance test_gpu_vae_encode.py gives f_hat
    assert abs(vq_loss.item() - want) <= tol
    assert err_r <= 1e-4                                     # the tolerance test_gpu_vae_encode.py gives recon0
    assert rec.shape == x.shape and rec.abs().max().item() > 1                                            # unclamped (the fixture has values outside [-1, 1])
    assert int(g["rec0_outside"]) > 0
    rec2, none, loss2 = vae(x, ret_usages=False)
    assert none is None and torch.equal(rec2, rec) and torch.equal(loss2, vq_loss)
    assert torch.equal(rec.clamp(-1, 1), vae.fhat_to_img(f_st))                                  # the clamped decode of the same f_hat


@pytest.mark.parametrize("mode", MODES)
def test_eval_vae(dev, monkeypatch, mode):
    from sdvar_amd import evaluate
    from sdvar_amd.engine import SdvarError
    monkeypatch.setenv("SDVAR_CONV_MODE", mode)
    g, e, vae, x = _model(dev)
    loader = [(x.cpu(), torch.zeros(2, dtype=torch.int64)), (x[:1], torch.zeros(1, dtype=torch.int64, device=dev))]
    rec_mse, rec_l1, vq_loss, usage_S, tot, seconds = evaluate.eval_vae(vae, loader)
    l1 = l2 = vq = 0.0
    n = 0
    ids = []
    for xb, _ in loader:
        xb = xb.to(dev)
        rec, _, loss = vae(xb)
        d = rec.double() - xb.double()
        l1 += d.abs().sum().item(); l2 += (d * d).sum().item(); n += d.numel()
        vq += loss.double().item() * xb.shape[0]
        ids.append(torch.cat(vae.img_to_idxBl(xb), 1))
    ids = torch.cat(ids, 0)
    print(f"{mode}: rec_mse {rec_mse:.9e} ({l2 / n:.9e}) rec_l1 {rec_l1:.9e} ({l1 / n:.9e}) vq_loss {vq_loss:.9e} ({vq / 3:.9e}) usage {usage_S}")
    assert tot == 3 and seconds >= 0
    assert abs(rec_mse - l2 / n) <= 1e-6 * (l2 / n) and abs(rec_l1 - l1 / n) <= 1e-6 * (l1 / n) and abs(vq_loss - vq / 3) <= 1e-6 * (vq / 3)
    off, want = 0, []
    for pn in (int(p) for p in g["patch_nums"]):
        hit = torch.bincount(ids[:, off:off + pn * pn].reshape(-1), minlength=4096)
        want.append(int((hit > 0).sum()) * 100.0 / 4096)
        off += pn * pn
    assert usage_S == want
    assert not vae.training
    with pytest.raises(SdvarError, match="no images"):
        evaluate.eval_vae(vae, [])
