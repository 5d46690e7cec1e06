"""References for the one-product convolution format (plane_format 6, conv_mode "f16"): f16x2 planes, X plane 0 times W plane 0 and nothing else.  Imports
without a GPU; builds on tests/conv_exact_cases.py, which it does not modify.

hh_ref(c, res): the float64 convolution of x plane 0 with w plane 0 of an f16x2 case, divided by the weight scale, + bias (+ res).  On 'int' cases the low planes
are zero and this is the float64 conv2d; on 'dense' and 'sparse' cases it differs from the three-product reference wherever an hl or lh term is non-zero, so a
kernel that keeps one of them - or reads plane 1 at all - cannot pass.  prove_exact_hh(c) shows that every partial sum of that product is exact in fp32.

decoder_f16_oracle(vae, f_hat): tests/torch_ref.decoder_torch with every convolution except conv_out taken on fp16-rounded operands, as the library packs them."""
import math

import torch
import torch.nn.functional as F

import conv_exact_cases as X
from gemm_exact_cases import weight_scale

PF_HH = 6                                   # include/sdvar_hip.h: plane_format of sdvar_op_conv_planes(_ex) and sdvar_vae_desc
F16_MAX = 65504.0


def int_cases():
    """the INT_SHAPES the one-product format takes (N % 4 == 0), and a 1x1 convolution of ONE K-step (INT_SHAPES starts at two)"""
    return [c for c in X.int_cases() if c.N % 4 == 0] + [X.case("int", None, 2, 3, 5, 32, 48, 1, "prep")]


def split_plane_cases():
    return X.split_plane_cases(2)


def hh_base(c, absolute=False):
    xs, ws = c.x_planes(2), c.w_planes(2)
    t = c._conv(xs[0].abs(), ws[0].abs()) if absolute else c._conv(xs[0], ws[0])
    return t / c.scale(2)


_REFS = {}


def hh_ref(c, res):
    """float64 (B, N, Ho, Wo), cached and never modified"""
    key = (c.id, bool(res))
    if key not in _REFS:
        r = hh_base(c) + c.bias.double()[None, :, None, None]
        if res:
            r = r + c.res.double()
        _REFS[key] = r
    return _REFS[key]


def prove_exact_hh(c):
    """(bound of every partial sum, grain, bits) of the plane-0 product, as conv_exact_cases.prove_exact does for the products of a format"""
    xs, ws = c.x_planes(2), c.w_planes(2)
    e = min(0, X.grain_log2(xs[0]) + X.grain_log2(ws[0]) - int(math.log2(c.scale(2))))
    bound = float(hh_base(c, absolute=True).max()) + float(c.bias.abs().max()) + (float(c.res.abs().max()) if c.res is not None else 0.0)
    return bound, 2.0 ** e, math.log2(bound / 2.0 ** e)


def expected_kernel(c, reuse, split):
    """out[0] of sdvar_debug_get_conv_plan in format 6: 4 where the tap-reuse rule of the header holds (the rule of format 2 with "conv_pp" 2), else 3"""
    return 4 if X.tap_reuse_eligible(c, 2, 2, reuse, split) else 3


# ---------------------------------------------------------------------------------------------------------------- the decoder on fp16-rounded operands
def _h(t):
    return t.clamp(-F16_MAX, F16_MAX).half().float()


def _wq(w):
    S = weight_scale(w)
    return (w * S).half().float() / S


def _conv16(m, x):
    return F.conv2d(_h(x), _wq(m.weight), m.bias, m.stride, m.padding)


def _upconv16(m, x):
    """Upsample2x as the library runs it: four 2x2 phase convolutions on the input grid, the four phase weight sets rounded under ONE scale"""
    w = m.weight
    N = w.shape[0]
    weff = X.upconv_weff(w.float().cpu()).to(w.device)                 # (4, N, Cin, 2, 2)
    S = weight_scale(weff)
    wq = ((weff * S).half().float() / S).reshape(4 * N, w.shape[1], 2, 2)
    B, _, H, W = x.shape
    full = F.conv2d(F.pad(_h(x), (1, 1, 1, 1)), wq)                     # (B, 4N, H + 1, W + 1)
    out = x.new_zeros(B, N, 2 * H, 2 * W)
    for py in range(2):
        for px in range(2):
            ph = 2 * py + px
            out[:, :, py::2, px::2] = full[:, ph * N:(ph + 1) * N, py:py + H, px:px + W]
    return out + m.bias[None, :, None, None]


def _gn(m, x):
    return F.group_norm(x, m.num_groups, m.weight, m.bias, m.eps)


def _res16(b, x):
    h = _conv16(b.conv1, F.silu(_gn(b.norm1, x)))
    h = _conv16(b.conv2, F.silu(_gn(b.norm2, h)))
    sc = x if isinstance(b.nin_shortcut, torch.nn.Identity) else _conv16(b.nin_shortcut, x)
    return sc + h


def _attn16(a, x):
    B, C, H, W = x.shape
    q, k, v = _conv16(a.qkv, _gn(a.norm, x)).reshape(B, 3, C, H * W).unbind(1)
    w = torch.bmm(q.transpose(1, 2), k).mul_(C ** -0.5).softmax(dim=2)
    h = torch.bmm(v, w.transpose(1, 2)).view(B, C, H, W)
    return x + _conv16(a.proj_out, h)


@torch.no_grad()
def decoder_f16_oracle(vae, f_hat):
    """the unclamped image: torch_ref.decoder_torch(vae.decoder, post_quant_conv(f_hat)) with fp16-operand convolutions everywhere but conv_out (fp32)"""
    dec = vae.decoder
    h = _conv16(dec.conv_in, _conv16(vae.post_quant_conv, f_hat))
    h = _res16(dec.mid.block_2, _attn16(dec.mid.attn_1, _res16(dec.mid.block_1, h)))
    for lv in reversed(range(len(dec.up))):
        up = dec.up[lv]
        for ib, blk in enumerate(up.block):
            h = _res16(blk, h)
            if len(up.attn):
                h = _attn16(up.attn[ib], h)
        if lv != 0:
            h = _upconv16(up.upsample.conv, h)
    m = dec.conv_out
    return F.conv2d(F.silu(_gn(dec.norm_out, h)), m.weight, m.bias, m.stride, m.padding)
