"""GPU: the opt-in decoder mode conv_mode "f16" (one fp16 product per convolution) against an fp16-operand oracle.

Model: ch = 32, 'stress' init, B = 2, latent 16, the UNCLAMPED image (decode_raw).  On the CPU, tests/torch_ref.decoder_torch is the fp32 reference and
conv_f16_cases.decoder_f16_oracle the same walk with every convolution but conv_out taken on fp16(clamp(x)) and fp16(w S) / S (the up-sampling convolutions as four
phase weight sets under one scale).  e_ref = max |oracle - fp32| is what one fp16 product per convolution costs on this model; the HIP mode is held to the GEMM
tier's rule (tests/test_gpu_f16_mode.py): max |HIP f16 - fp32| <= 2 e_ref.  max |HIP f16 - oracle| is printed, not bounded.
Measured on MI355X: e_ref 4.34e-3 (the CPU of that machine; 4.88e-3 on another CPU), max |HIP f16 - fp32| 5.25e-3 (mean 5.8e-4), max |HIP f16 - oracle| 4.55e-3,
max |raw| 3.59; the f16x2 context in the same process 6.1e-6."""
import ctypes as C

import pytest
import torch

import conv_f16_cases as H
from conftest import rnd
from sdvar_amd import engine as E
from sdvar_amd.vqvae import VQVAE
from sdvar_amd.weights import vae_state_dict
from torch_ref import _conv, decoder_torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

PNS = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
B, LATENT, SEED = 2, 16, 11
_MEMO = {}


def _setup():
    """model, f_hat and both CPU references: built once, never modified"""
    if not _MEMO:
        sd = vae_state_dict(PNS, "stress", SEED, V=64, Cvae=32, ch=32, with_encoder=False)
        vae = VQVAE(vocab_size=64, z_channels=32, ch=32, v_patch_nums=PNS, with_encoder=False)
        vae.load_state_dict(sd)
        f_hat = rnd(SEED + 1, (B, 32, LATENT, LATENT), 1.5)
        ref = decoder_torch(vae.decoder, _conv(vae.post_quant_conv, f_hat.clone()))
        orc = H.decoder_f16_oracle(vae, f_hat.clone())
        _MEMO.update(sd=sd, vae=vae, f_hat=f_hat, ref=ref, orc=orc)
    return _MEMO


def _last_kernel(lib):
    out4 = (C.c_int32 * 4)()
    E._check(lib.sdvar_debug_get_conv_plan(out4))
    return out4[0]


def test_decoder_f16_within_twice_the_oracle_error(dev):
    m = _setup()
    lib = E.load_library()
    ref, orc, f_hat = m["ref"], m["orc"], m["f_hat"].to(dev)
    e_ref = (orc - ref).abs().max().item()
    assert e_ref > 0
    ctx = E.VaeCtx(m["sd"], B, dev, latent_hw=LATENT, conv_mode="f16")
    assert ctx.conv_mode == "f16" and ctx.desc.plane_format == H.PF_HH
    got = ctx.decode_raw(f_hat)
    assert _last_kernel(lib) in (3, 4)
    again = ctx.decode_raw(f_hat)
    assert got.shape == ref.shape == (B, 3, 256, 256)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, again), "two decodes of one f_hat differ"
    e_hip, e_orc = (got.cpu() - ref).abs().max().item(), (got.cpu() - orc).abs().max().item()
    print(f"conv_mode f16 accuracy: e_ref {e_ref:.3e}, max|HIP f16 - fp32| {e_hip:.3e}, max|HIP f16 - oracle| {e_orc:.3e}, mean|HIP f16 - fp32| "
          f"{(got.cpu() - ref).abs().mean().item():.3e}, max|raw| {ref.abs().max().item():.3e}")
    # the mode is not the default in disguise: an f16x2 context in the same process stays fp32-accurate, before and after, and takes the three-product kernels
    ctx2 = E.VaeCtx(m["sd"], B, dev, latent_hw=LATENT, conv_mode="f16x2")
    got2 = ctx2.decode_raw(f_hat)
    assert _last_kernel(lib) in (1, 2)
    e2 = (got2.cpu() - ref).abs().max().item()
    print(f"conv_mode f16x2 in the same process: max|HIP - fp32| {e2:.3e}")
    assert e2 <= 1e-4, e2
    assert torch.equal(ctx.decode_raw(f_hat), got), "the f16 decode changed after an f16x2 context ran"
    assert not torch.equal(got, got2)
    assert e_hip <= 2 * e_ref, (e_hip, e_ref)
    ctx.close(); ctx2.close()


def test_vqvae_conv_mode_switch(dev, monkeypatch):
    """through the public class: conv_mode = "f16" changes fhat_to_img's bits, None restores the default's exactly; the clamped image stays within 2 e_ref too"""
    monkeypatch.delenv("SDVAR_CONV_MODE", raising=False)
    m = _setup()
    vae = VQVAE(vocab_size=64, z_channels=32, ch=32, v_patch_nums=PNS, with_encoder=False)
    vae.load_state_dict(m["sd"])
    vae = vae.to(dev)
    f_hat = m["f_hat"].to(dev)
    assert vae.conv_mode is None
    base = vae.fhat_to_img(f_hat).clone()
    assert vae._hip_ctx.conv_mode == "f16x2"
    vae.conv_mode = "f16"
    half = vae.fhat_to_img(f_hat).clone()
    assert vae._hip_ctx.conv_mode == "f16" and _last_kernel(E.load_library()) in (3, 4)
    assert not torch.equal(half, base)
    e_ref = (m["orc"] - m["ref"]).abs().max().item()
    assert (half.cpu() - m["ref"].clamp(-1, 1)).abs().max().item() <= 2 * e_ref
    vae.conv_mode = None
    back = vae.fhat_to_img(f_hat)
    assert vae._hip_ctx.conv_mode == "f16x2" and torch.equal(back, base)
    vae.conv_mode = "f16x2"                                   # the same mode by name: the context stays
    ctx = vae._hip_ctx
    assert torch.equal(vae.fhat_to_img(f_hat), base) and vae._hip_ctx is ctx
    vae.refresh_hip()


def test_env_selects_f16_for_decoders(dev, monkeypatch):
    m = _setup()
    monkeypatch.setenv("SDVAR_CONV_MODE", "f16")
    ctx = E.VaeCtx(m["sd"], B, dev, latent_hw=LATENT)
    assert ctx.conv_mode == "f16" and ctx.desc.plane_format == H.PF_HH
    ctx.close()


def test_encoder_create_rejects_the_format(dev):
    """sdvar_vae_enc_create keeps rejecting plane_format 6 (the Python layer never sends it)"""
    lib = E.load_library()
    d = E._VaeDesc()
    d.ch, d.z_channels, d.n_mult, d.num_res_blocks, d.max_batch, d.latent_hw, d.plane_format = 32, 32, 5, 2, 1, 16, H.PF_HH
    for i, mult in enumerate((1, 1, 2, 2, 4)):
        d.ch_mult[i] = mult
    h = C.c_void_p()
    assert lib.sdvar_vae_enc_create(C.byref(d), C.byref(h)) != 0 and not h
    assert "plane_format 6" in lib.sdvar_last_error().decode()
