"""PyTorch restatement of the VQVAE image side, used ONLY by tests and tools (never imported by sdvar_amd/).

`img_to_f_torch(vae, img)`: quant_conv(encoder(img)) (/root/reference/models/vqvae.py:66, models/basic_vae.py:99-161);
`f_to_idxBl_or_fhat_torch(vae, f, to_fhat)`: the multi-scale residual quantisation (models/quant.py:135-166, using_znorm=False);
`idxBl_to_var_input_torch(vae, ids)`: the teacher-forcing input (quant.py:169-184).  They read the parameters of an
`sdvar_amd.vqvae.VQVAE`, whose modules are parameter containers without forward().
"""
import torch
import torch.nn.functional as F

from sdvar_amd.ladder import phi_index
from torch_ref import _attn, _conv, _gn, _res


@torch.no_grad()
def encoder_torch(enc, x):                             # basic_vae.py:144-161
    h = _conv(enc.conv_in, x)
    for lv, dn in enumerate(enc.down):
        for ib, blk in enumerate(dn.block):
            h = _res(blk, h)
            if len(dn.attn):
                h = _attn(dn.attn[ib], h)
        if lv != len(enc.down) - 1:
            h = _conv(dn.downsample.conv, F.pad(h, (0, 1, 0, 1)))          # Downsample2x: pad right / bottom, 3x3 stride 2
    h = _res(enc.mid.block_2, _attn(enc.mid.attn_1, _res(enc.mid.block_1, h)))
    return _conv(enc.conv_out, F.silu(_gn(enc.norm_out, h)))


@torch.no_grad()
def img_to_f_torch(vae, img):                          # vqvae.py:66
    return _conv(vae.quant_conv, encoder_torch(vae.encoder, img))


def _phis(q):
    qr = q.quant_resi
    if hasattr(qr, "qresi"):
        return [qr.qresi]
    return list(qr.qresi_ls) if hasattr(qr, "qresi_ls") else list(qr)


def _phi(q, si, S, h):                                 # Phi (quant.py:199-206) chosen as quant.py:218-226
    phis = _phis(q)
    m = phis[phi_index(si, S, len(phis))] if len(phis) > 1 else phis[0]
    return h.mul(0.5) + _conv(m, h).mul_(0.5)


@torch.no_grad()
def f_to_idxBl_or_fhat_torch(vae, f, to_fhat, v_patch_nums=None, margins=None):     # quant.py:135-166
    """margins (list or None): receives per scale, for every row, the fp64 gap between the two smallest distances, |z|^2 + mean |e|^2, and
    |e_1 - e_2| of the two nearest codes (the gap is linear in z with gradient 2 (e_2 - e_1))."""
    q = vae.quantize
    pns = tuple(v_patch_nums or q.v_patch_nums)
    B, C, H, W = f.shape
    E = q.embedding.weight.data
    f_rest, f_hat, out = f.clone(), torch.zeros_like(f), []
    SN = len(pns)
    for si, pn in enumerate(pns):
        z = (F.interpolate(f_rest, size=(pn, pn), mode="area") if si != SN - 1 else f_rest).permute(0, 2, 3, 1).reshape(-1, C)
        d = torch.sum(z.square(), dim=1, keepdim=True) + torch.sum(E.square(), dim=1, keepdim=False)
        d.addmm_(z, E.T, alpha=-2, beta=1)
        idx = torch.argmin(d, dim=1)
        if margins is not None:
            z64, e64 = z.double(), E.double()
            d64 = (z64 * z64).sum(1, keepdim=True) + (e64 * e64).sum(1) - 2 * z64 @ e64.T
            two = d64.topk(2, dim=1, largest=False)
            de = (e64[two.indices[:, 0]] - e64[two.indices[:, 1]]).norm(dim=1)
            margins.append(((two.values[:, 1] - two.values[:, 0]).numpy(), ((z64 * z64).sum(1) + (e64 * e64).sum(1).mean()).numpy(), de.numpy()))
        hb = E[idx.view(B, pn, pn)].permute(0, 3, 1, 2)
        h = F.interpolate(hb, size=(H, W), mode="bicubic") if si != SN - 1 else hb.contiguous()
        h = _phi(q, si, SN, h)
        f_hat.add_(h)
        f_rest.sub_(h)
        out.append(f_hat.clone() if to_fhat else idx.reshape(B, pn * pn))
    return out


@torch.no_grad()
def idxBl_to_var_input_torch(vae, ids):                # quant.py:169-184
    q = vae.quantize
    pns, C = q.v_patch_nums, q.Cvae
    B, H, SN = ids[0].shape[0], pns[-1], len(pns)
    E = q.embedding.weight.data
    f_hat, nxt = torch.zeros(B, C, H, H, dtype=E.dtype), []                # a .double() model keeps the whole chain in fp64
    for si in range(SN - 1):
        h = F.interpolate(E[ids[si]].transpose(1, 2).reshape(B, C, pns[si], pns[si]), size=(H, H), mode="bicubic")
        f_hat.add_(_phi(q, si, SN, h))
        nxt.append(F.interpolate(f_hat, size=(pns[si + 1], pns[si + 1]), mode="area").view(B, C, -1).transpose(1, 2))
    return torch.cat(nxt, dim=1)
