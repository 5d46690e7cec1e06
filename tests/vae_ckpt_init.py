"""Checkpoint-like VQVAE inits, derived from weights.vae_state_dict(..., "stress"), and their fp64 references on the CPU: the decoder's for the whole-decoder test
of tests/test_gpu_vae_kernels.py (below), the encoder's for tests/test_gpu_vae_encode_fp64.py (checkpoint_like_encoder_state_dict, at the end of this file).

The "stress" init sets every GroupNorm to the identity affine and every conv bias to 0.02, with zero-mean fan-in-normalised weights: every GroupNorm input then has
a group mean near 0 and a spread near 1, the one regime where a one-pass variance cannot fail and a gamma / beta mix-up does not show.  Here:
  - GroupNorm gamma ~ U(0.5, 1.5), beta ~ N(0, 0.5); conv biases ~ N(0, 0.2);
  - the convolutions that write the residual stream (conv_in, each resblock's conv2, the attention's proj_out, the upsample conv) get a per-group bias offset,
    set in one fp32 calibration pass on the given input so that the stream each of them leaves has |mean| / std between 10 and 30 in every group (signs mixed):
    the GroupNorms that read the stream (norm1, the attention's norm, norm_out) see those ratios;
  - conv_out's weight is scaled so that its output (before the bias) has 99 % of its values within +-0.6: the clamp at +-1 leaves the image readable.
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F

PNS = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
CH_MULT = (1, 1, 2, 2, 4)
NRB = 2


def _group_targets():
    g = torch.arange(32, dtype=torch.float64)
    r = 10.0 + 20.0 * ((g * 7) % 32) / 31.0                   # 10 .. 30, spread over the groups
    s = torch.where((g // 2) % 2 == 0, 1.0, -1.0)
    return s * r


def checkpoint_like_state_dict(f_hat, ch=160, seed=11):
    """f_hat (B, 32, h, w) float32 on the CPU -> decoder state_dict (float32) as described above."""
    from sdvar_amd.weights import vae_state_dict
    sd = OrderedDict((k, v.clone()) for k, v in vae_state_dict(PNS, "stress", seed, V=64, Cvae=32, ch=ch, with_encoder=False).items())
    gen = torch.Generator().manual_seed(seed + 1000)
    for k in sd:
        if not k.startswith(("decoder.", "post_quant_conv.")) or sd[k].dim() != 1:
            continue
        mod = k.rsplit(".", 2)[-2]
        if mod.startswith("norm"):
            sd[k] = (torch.rand(sd[k].shape, generator=gen) + 0.5) if k.endswith(".weight") else torch.randn(sd[k].shape, generator=gen) * 0.5
        else:
            sd[k] = torch.randn(sd[k].shape, generator=gen) * 0.2
    targets = _group_targets()

    def conv(name, x, pad):
        return F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], padding=pad)

    def gn(name, x):
        return F.group_norm(x, 32, sd[name + ".weight"], sd[name + ".bias"], eps=1e-6)

    def write(name, x):
        """x: the stream the conv `name` just wrote (its bias included): shift its bias per channel so that every channel of group g has the mean t_g s_g, s_g^2
        the group's within-channel variance - the group then has |mean| / std = |t_g|, and the spread stays that of the pixels (channel means that differ
        inside a group would add to it, and grow through every convolution that reads the stream)"""
        B, Cc = x.shape[:2]
        xc = x.double().transpose(0, 1).reshape(Cc, -1)
        s = xc.var(-1, unbiased=False).reshape(32, -1).mean(-1).sqrt()
        delta = ((targets * s).repeat_interleave(Cc // 32) - xc.mean(-1)).float()
        sd[name + ".bias"] = (sd[name + ".bias"] + delta).float()
        return x + delta[None, :, None, None]

    def res(p, x):
        h = conv(p + ".conv1", F.silu(gn(p + ".norm1", x)), 1)
        h = conv(p + ".conv2", F.silu(gn(p + ".norm2", h)), 1)
        sc = conv(p + ".nin_shortcut", x, 0) if p + ".nin_shortcut.weight" in sd else x
        return write(p + ".conv2", sc + h)

    def attn(p, x):
        B, Cc, H, W = x.shape
        q, k, v = conv(p + ".qkv", gn(p + ".norm", x), 0).reshape(B, 3, Cc, H * W).unbind(1)
        w = torch.softmax(torch.bmm(q.transpose(1, 2), k) * Cc ** -0.5, dim=2)
        h = torch.bmm(v, w.transpose(1, 2)).view(B, Cc, H, W)
        return write(p + ".proj_out", x + conv(p + ".proj_out", h, 0))

    with torch.no_grad():
        x = write("decoder.conv_in", conv("decoder.conv_in", conv("post_quant_conv", f_hat, 1), 1))
        x = res("decoder.mid.block_2", attn("decoder.mid.attn_1", res("decoder.mid.block_1", x)))
        for lv in reversed(range(len(CH_MULT))):
            for ib in range(NRB + 1):
                x = res(f"decoder.up.{lv}.block.{ib}", x)
                if lv == len(CH_MULT) - 1:
                    x = attn(f"decoder.up.{lv}.attn.{ib}", x)
            if lv != 0:
                x = write(f"decoder.up.{lv}.upsample.conv", conv(f"decoder.up.{lv}.upsample.conv", F.interpolate(x, scale_factor=2, mode="nearest"), 1))
        y = F.conv2d(F.silu(gn("decoder.norm_out", x)), sd["decoder.conv_out.weight"], padding=1)
        sd["decoder.conv_out.weight"] = (sd["decoder.conv_out.weight"] * (0.6 / torch.quantile(y.abs().flatten()[::7], 0.99))).float()
    return sd


def reference_fp64(sd, f_hat, ch=160):
    """The fp64 decode on the CPU (tests/torch_ref.py on a .double() copy of the module): the image before the clamp, and the largest |mean| / std of a group at each
    GroupNorm (in call order) from the fp64 intermediates."""
    import torch_ref as TR
    from sdvar_amd.vqvae import VQVAE
    vae = VQVAE(vocab_size=64, z_channels=32, ch=ch, v_patch_nums=PNS, with_encoder=False)
    vae.load_state_dict(sd)
    vae = vae.double()
    ratios = []
    orig = TR._gn

    def gn_rec(m, x):
        xg = x.reshape(x.shape[0], 32, -1)
        ratios.append((xg.mean(-1).abs() / xg.std(-1, unbiased=False)).max().item())
        return orig(m, x)

    TR._gn = gn_rec
    try:
        with torch.no_grad():
            y = TR.decoder_torch(vae.decoder, TR._conv(vae.post_quant_conv, f_hat.double()))
    finally:
        TR._gn = orig
    return y, ratios


# ---------------------------------------------------------------------------------------------------- the encoder (image -> f)
def checkpoint_like_encoder_state_dict(img, ch=160, seed=23, V=4096, patch_nums=PNS, share_quant_resi=4):
    """img (B, 3, H, H) float32 on the CPU in [-1, 1] -> a whole VQVAE state_dict (float32) whose encoder half is checkpoint-like in the sense of this file's header:
      - GroupNorm gamma ~ U(0.5, 1.5), beta ~ N(0, 0.5); conv biases ~ N(0, 0.2) (encoder.* and quant_conv);
      - the convolutions that write the encoder's residual stream (encoder.conv_in, each resblock's conv2, each attention's proj_out, each downsample.conv) get
        a per-channel bias offset, set in one fp32 calibration pass on img so that every group of the stream each of them leaves has |mean| / std between 10 and
        30 (signs mixed): norm1 of the next resblock, the attention's norm, norm_out and - unnormalised - the Downsample2x convolution read those streams;
      - quant_conv is scaled so that f has a per-pixel spread of 1 around per-channel offsets ~ U(-3, 3) (a few units), then shrunk if needed so that
        max|f| <= 10.
    The decoder, the codebook (N(0, 1)) and the Phi convolutions stay those of the stress init."""
    from sdvar_amd.weights import vae_state_dict
    sd = OrderedDict((k, v.clone()) for k, v in vae_state_dict(tuple(patch_nums), "stress", seed, V=V, Cvae=32, ch=ch, with_encoder=True,
                                                                share_quant_resi=share_quant_resi).items())
    gen = torch.Generator().manual_seed(seed + 2000)
    for k in sd:
        if not k.startswith(("encoder.", "quant_conv.")) or sd[k].dim() != 1:
            continue
        mod = k.rsplit(".", 2)[-2]
        if mod.startswith("norm"):
            sd[k] = (torch.rand(sd[k].shape, generator=gen) + 0.5) if k.endswith(".weight") else torch.randn(sd[k].shape, generator=gen) * 0.5
        else:
            sd[k] = torch.randn(sd[k].shape, generator=gen) * 0.2
    targets = _group_targets()

    def conv(name, x, pad, stride=1):
        return F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], stride=stride, padding=pad)

    def gn(name, x):
        return F.group_norm(x, 32, sd[name + ".weight"], sd[name + ".bias"], eps=1e-6)

    def write(name, x):                                          # as in checkpoint_like_state_dict
        Cc = x.shape[1]
        xc = x.double().transpose(0, 1).reshape(Cc, -1)
        s = xc.var(-1, unbiased=False).reshape(32, -1).mean(-1).sqrt()
        delta = ((targets * s).repeat_interleave(Cc // 32) - xc.mean(-1)).float()
        sd[name + ".bias"] = (sd[name + ".bias"] + delta).float()
        return x + delta[None, :, None, None]

    def res(p, x):
        h = conv(p + ".conv1", F.silu(gn(p + ".norm1", x)), 1)
        h = conv(p + ".conv2", F.silu(gn(p + ".norm2", h)), 1)
        sc = conv(p + ".nin_shortcut", x, 0) if p + ".nin_shortcut.weight" in sd else x
        return write(p + ".conv2", sc + h)

    def attn(p, x):
        B, Cc, H, W = x.shape
        q, k, v = conv(p + ".qkv", gn(p + ".norm", x), 0).reshape(B, 3, Cc, H * W).unbind(1)
        w = torch.softmax(torch.bmm(q.transpose(1, 2), k) * Cc ** -0.5, dim=2)
        h = torch.bmm(v, w.transpose(1, 2)).view(B, Cc, H, W)
        return write(p + ".proj_out", x + conv(p + ".proj_out", h, 0))

    nlv = len(CH_MULT)
    with torch.no_grad():
        x = write("encoder.conv_in", conv("encoder.conv_in", img, 1))
        for lv in range(nlv):
            for ib in range(NRB):
                x = res(f"encoder.down.{lv}.block.{ib}", x)
                if lv == nlv - 1:
                    x = attn(f"encoder.down.{lv}.attn.{ib}", x)
            if lv != nlv - 1:
                p = f"encoder.down.{lv}.downsample.conv"
                x = write(p, conv(p, F.pad(x, (0, 1, 0, 1)), 0, stride=2))
        x = res("encoder.mid.block_2", attn("encoder.mid.attn_1", res("encoder.mid.block_1", x)))
        h = conv("encoder.conv_out", F.silu(gn("encoder.norm_out", x)), 1)
        y0 = F.conv2d(h, sd["quant_conv.weight"], padding=1)
        y0c = y0.transpose(0, 1).reshape(y0.shape[1], -1)
        sd["quant_conv.weight"] = (sd["quant_conv.weight"] / y0c.std(-1).mean()).float()
        off = (torch.rand(y0.shape[1], generator=gen) * 6 - 3)
        sd["quant_conv.bias"] = (off - y0c.mean(-1) / y0c.std(-1).mean()).float()
        f = conv("quant_conv", h, 1)
        shrink = min(1.0, 9.5 / f.abs().max().item())
        sd["quant_conv.weight"] = (sd["quant_conv.weight"] * shrink).float()
        sd["quant_conv.bias"] = (sd["quant_conv.bias"] * shrink).float()
    return sd


def encoder_model(sd, ch=160, patch_nums=PNS, share_quant_resi=4):
    """The parameter container of sd (float32, on the CPU)"""
    from sdvar_amd.vqvae import VQVAE
    vae = VQVAE(vocab_size=sd["quantize.embedding.weight"].shape[0], z_channels=32, ch=ch, v_patch_nums=tuple(patch_nums), share_quant_resi=share_quant_resi)
    vae.load_state_dict(sd)
    return vae


def encoder_reference_fp64(sd, img, ch=160, patch_nums=PNS, share_quant_resi=4):
    """The fp64 encode on the CPU (tests/torch_ref_encode.img_to_f_torch on a .double() copy of the module): f, and the largest |mean| / std of a group at each
    GroupNorm (in call order) from the fp64 intermediates."""
    import torch_ref as TR
    import torch_ref_encode as TE
    vae = encoder_model(sd, ch, patch_nums, share_quant_resi).double()
    ratios = []
    orig = TR._gn

    def gn_rec(m, x):
        xg = x.reshape(x.shape[0], 32, -1)
        ratios.append((xg.mean(-1).abs() / xg.std(-1, unbiased=False)).max().item())
        return orig(m, x)

    TR._gn = TE._gn = gn_rec                                     # torch_ref_encode holds its own name for norm_out's call
    try:
        f = TE.img_to_f_torch(vae, img.double())
    finally:
        TR._gn = TE._gn = orig
    return f, ratios
