"""VQVAE parameter container with the reference's state_dict layout.

The quantizer tensors (codebook, shared Phi convs) feed sdvar_amd/csrc/quant.hip; the conv decoder `fhat_to_img`
(/root/reference/models/vqvae.py:62-63, models/basic_vae.py:163-226) runs as hand-written HIP
(csrc/conv.hip, csrc/vae.hip) through engine.VaeCtx.  The nn.Module tree below exists for the parameter names only - they follow
the upstream checkpoint `vae_ch160v4096z32.pth` so it loads unchanged.  There is no torch math in this package
(the PyTorch decoder the GPU parity tests compare against lives in tests/torch_ref.py), and no nn.Module class below defines a forward() of its own:
VQVAE.forward / VectorQuantizer2.forward (vqvae.py:56-59, quant.py:52-104: reconstruction, VQ loss, codebook usage; eval mode) is a sequence of HIP calls
that the two container classes inherit from the plain mixins _VaeForward and _QuantizerForward, so tests/test_abi.py's rule that the nn.Module classes
here stay parameter containers keeps holding, and its scan for torch arithmetic covers the mixins like every other line of the package.

The image side (vqvae.py:65-90, quant.py:107-184: img_to_idxBl, img_to_reconstructed_img, idxBl_to_img, embed_to_img,
f_to_idxBl_or_fhat, embed_to_fhat, idxBl_to_var_input) runs on HIP as well: the encoder + quant_conv through engine.VaeEncCtx
(csrc/vae.hip), the multi-scale residual quantisation through engine.QuantCtx.encode (csrc/quant.hip).  GPU tensors only.  Not supported
(SdvarError): using_znorm=True, non-square (ph, pw) patch tuples, all_to_max_scale=False, a VQVAE built with with_encoder=False.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import numpy as np
import torch
import torch.distributed as tdist
import torch.nn as nn


def _gn(c): return nn.GroupNorm(32, c, eps=1e-6, affine=True)


class _Res(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.norm1, self.conv1 = _gn(cin), nn.Conv2d(cin, cout, 3, 1, 1)
        self.norm2, self.conv2 = _gn(cout), nn.Conv2d(cout, cout, 3, 1, 1)
        self.nin_shortcut = nn.Conv2d(cin, cout, 1) if cin != cout else nn.Identity()


class _Attn(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.C = c
        self.norm, self.qkv, self.proj_out = _gn(c), nn.Conv2d(c, 3 * c, 1), nn.Conv2d(c, c, 1)


class _Up(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, 1, 1)


class _Down(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, 2, 0)


class Decoder(nn.Module):
    def __init__(self, ch, ch_mult, nrb, z):
        super().__init__()
        nres = len(ch_mult)
        bi = ch * ch_mult[-1]
        self.conv_in = nn.Conv2d(z, bi, 3, 1, 1)
        self.mid = nn.Module()
        self.mid.block_1, self.mid.attn_1, self.mid.block_2 = _Res(bi, bi), _Attn(bi), _Res(bi, bi)
        self.up = nn.ModuleList()
        for lv in reversed(range(nres)):
            bo = ch * ch_mult[lv]
            up = nn.Module()
            up.block, up.attn = nn.ModuleList(), nn.ModuleList()
            for _ in range(nrb + 1):
                up.block.append(_Res(bi, bo)); bi = bo
                if lv == nres - 1:
                    up.attn.append(_Attn(bi))
            if lv != 0:
                up.upsample = _Up(bi)
            self.up.insert(0, up)
        self.norm_out, self.conv_out = _gn(bi), nn.Conv2d(bi, 3, 3, 1, 1)


class Encoder(nn.Module):
    """Parameters only (state_dict names); the arithmetic is engine.VaeEncCtx (csrc/vae.hip)."""
    def __init__(self, ch, ch_mult, nrb, z):
        super().__init__()
        nres = len(ch_mult)
        self.conv_in = nn.Conv2d(3, ch, 3, 1, 1)
        in_mult = (1,) + tuple(ch_mult)
        self.down = nn.ModuleList()
        bi = ch
        for lv in range(nres):
            bi, bo = ch * in_mult[lv], ch * ch_mult[lv]
            dn = nn.Module()
            dn.block, dn.attn = nn.ModuleList(), nn.ModuleList()
            for _ in range(nrb):
                dn.block.append(_Res(bi, bo)); bi = bo
                if lv == nres - 1:
                    dn.attn.append(_Attn(bi))
            if lv != nres - 1:
                dn.downsample = _Down(bi)
            self.down.append(dn)
        self.mid = nn.Module()
        self.mid.block_1, self.mid.attn_1, self.mid.block_2 = _Res(bi, bi), _Attn(bi), _Res(bi, bi)
        self.norm_out, self.conv_out = _gn(bi), nn.Conv2d(bi, z, 3, 1, 1)


class _PhiList(nn.Module):          # PhiPartiallyShared (quant.py:219-229): quant_resi.qresi_ls.<k>
    def __init__(self, n, c):
        super().__init__()
        self.qresi_ls = nn.ModuleList([nn.Conv2d(c, c, 3, 1, 1) for _ in range(n)])


class _PhiOne(nn.Module):           # PhiShared (quant.py:209-216): quant_resi.qresi
    def __init__(self, c):
        super().__init__()
        self.qresi = nn.Conv2d(c, c, 3, 1, 1)


def _refuse_forward(mod: nn.Module, t: torch.Tensor, what: str):
    """forward() runs in eval mode on GPU tensors without autograd; anything else is an error, never a torch fall-back."""
    from . import engine as E
    if mod.training:
        raise E.SdvarError(f"{what}: the module is in training mode; the HIP forward is the reference's eval branch (no EMA update, no backward): call .eval() first")
    if t.requires_grad and torch.is_grad_enabled():
        raise E.SdvarError(f"{what}: the input requires grad but no backward exists for the HIP kernels; detach it or run under torch.no_grad()")
    if not t.is_cuda:
        raise E.SdvarError(f"{what} runs on HIP and needs GPU tensors")


class _QuantizerForward:
    """VectorQuantizer2.forward (quant.py:52-104) in eval mode on HIP: engine.QuantCtx.encode_stats (csrc/quant.hip)."""

    def forward(self, f_BChw: torch.Tensor, ret_usages=False):
        """-> (f_hat, usages, mean_vq_loss): f_hat the straight-through (f_hat - f) + f of quant.py:98; usages None or per scale the percentage of
        codes whose ema_vocab_hit_SV entry reaches the reference's margin (world size 1 without a process group); mean_vq_loss a 0-dim fp32 tensor,
        (1/S) sum_s (beta + 1) mse(f_hat_s, f) - without autograd the two terms of quant.py:95 are one number."""
        f_st, usages, loss, _ = self._forward_hip(f_BChw, ret_usages)
        return f_st, usages, torch.tensor(loss, dtype=torch.float32, device=f_st.device)

    def _forward_hip(self, f_BChw: torch.Tensor, ret_usages: bool):
        """forward() with the loss as a python float (float64 arithmetic on the S sums) and the (S, V) int32 hit counts of this batch."""
        _refuse_forward(self, f_BChw, "Quantizer.forward")
        f = f_BChw.detach()
        if f.dtype != torch.float32:
            f = f.float()                                                                             # quant.py:54
        pns = self._ladder(None)
        if f.dim() != 4 or f.shape[1] != self.Cvae or f.shape[2] != pns[-1] or f.shape[3] != pns[-1]:
            raise self._err(f"Quantizer.forward: f of shape {tuple(f.shape)}: expected (B, {self.Cvae}, {pns[-1]}, {pns[-1]})")
        ctx = self._ctx(f.device, f.shape[0], pns)
        with torch.no_grad(), torch.cuda.device(f.device):
            _, _, _, hits, sqerr, f_st = ctx.encode_stats(f, straight_through=True)
        numel = f.numel()
        loss = sum((self.beta + 1.0) * (v / numel) for v in sqerr.cpu().tolist()) / len(pns)        # quant.py:95-97
        usages = self._usages(numel // f.shape[1]) if ret_usages else None
        return f_st, usages, loss, hits

    def _usages(self, n_rows: int) -> List[float]:
        """quant.py:100-102 on the host, for a batch of n_rows = B H W rows: per scale the percentage of codes whose ema_vocab_hit_SV entry reaches the margin."""
        world = tdist.get_world_size() if tdist.is_available() and tdist.is_initialized() else 1
        margin = world * n_rows / self.vocab_size * 0.08
        ema = self.ema_vocab_hit_SV.detach().to(dtype=torch.float32).cpu().numpy()
        # torch compares the fp32 buffer with the scalar rounded to fp32 and takes the mean in fp32
        return [float(np.float32(np.count_nonzero(row >= np.float32(margin))) / np.float32(self.vocab_size)) * 100 for row in ema]


class Quantizer(_QuantizerForward, nn.Module):
    """quantize.* tensors of the checkpoint (models/quant.py:15-43) in the layout `share_quant_resi` selects there (quant.py:27-32): 0 = one Phi per scale
    (PhiNonShared, an nn.ModuleList: quant_resi.<k>), 1 = one Phi for all (PhiShared), >= 2 = partially shared.  The arithmetic lives in csrc/quant.hip."""
    def __init__(self, vocab_size, Cvae, v_patch_nums, share_quant_resi=4, using_znorm=False, beta: float = 0.25):
        super().__init__()
        self.vocab_size, self.Cvae, self.v_patch_nums = vocab_size, Cvae, tuple(v_patch_nums)
        self.using_znorm = bool(using_znorm)
        self.beta = float(beta)             # commitment weight (quant.py:18, 38): enters forward()'s mean_vq_loss
        self._hip_q = None
        if share_quant_resi == 0:
            self.quant_resi = nn.ModuleList([nn.Conv2d(Cvae, Cvae, 3, 1, 1) for _ in range(len(v_patch_nums))])
        elif share_quant_resi == 1:
            self.quant_resi = _PhiOne(Cvae)
        else:
            self.quant_resi = _PhiList(share_quant_resi, Cvae)
        self.register_buffer("ema_vocab_hit_SV", torch.zeros(len(v_patch_nums), vocab_size))
        self.embedding = nn.Embedding(vocab_size, Cvae)

    # ------------------------------------------------------------------------------------------- image side on HIP (quant.py:107-184)
    def _err(self, msg):
        from . import engine as E
        return E.SdvarError(msg)

    def _ladder(self, v_patch_nums) -> tuple:
        out = []
        for pn in (v_patch_nums or self.v_patch_nums):
            if not isinstance(pn, int):
                ph, pw = pn
                if ph != pw:
                    raise self._err(f"Quantizer: non-square patch ({ph}, {pw}) is not supported (square ladders only)")
                pn = ph
            out.append(int(pn))
        return tuple(out)

    def _ctx(self, device, B: int, pns: tuple):
        from . import engine as E
        if self.using_znorm:
            raise self._err("Quantizer: using_znorm=True is not supported on HIP (the released checkpoint uses the L2 distance)")
        ctx = self._hip_q
        if ctx is None or ctx.device != device or ctx.max_batch < B or tuple(ctx.lad.patch_nums) != pns:
            if ctx is not None:
                ctx.close()
            ctx = self._hip_q = E.QuantCtx(self.state_dict(), pns, B, device, prefix="")
        return ctx

    def refresh_hip(self):
        """Drop the HIP quantizer's binding (call after changing the codebook or the Phi convolutions in place)."""
        if self._hip_q is not None:
            self._hip_q.close()
        self._hip_q = None

    def _need_gpu(self, t: torch.Tensor, what: str):
        if not t.is_cuda:
            raise self._err(f"Quantizer.{what} runs on HIP and needs GPU tensors")

    @torch.no_grad()
    def f_to_idxBl_or_fhat(self, f_BChw: torch.Tensor, to_fhat: bool, v_patch_nums=None) -> List[torch.Tensor]:       # quant.py:135-166
        """Multi-scale residual quantisation of f (B, Cvae, H, W): per scale the (B, pn^2) int64 ids, or (to_fhat) f_hat after that scale."""
        self._need_gpu(f_BChw, "f_to_idxBl_or_fhat")
        pns = self._ladder(v_patch_nums)
        B, _, H, W = f_BChw.shape
        if pns[-1] != H or pns[-1] != W:
            raise self._err(f"Quantizer.f_to_idxBl_or_fhat: last patch {pns[-1]} != (H={H}, W={W})")
        ctx = self._ctx(f_BChw.device, B, pns)
        ids, _, per_scale = ctx.encode(f_BChw, per_scale=to_fhat)
        if to_fhat:
            return [per_scale[si] for si in range(len(pns))]
        return [ids[:, ctx.lad.begin(si):ctx.lad.cum[si]].contiguous() for si in range(len(pns))]

    @torch.no_grad()
    def embed_to_fhat(self, ms_h_BChw: List[torch.Tensor], all_to_max_scale=True, last_one=False) -> Union[List[torch.Tensor], torch.Tensor]:   # quant.py:98-123
        if not all_to_max_scale:
            raise self._err("Quantizer.embed_to_fhat: all_to_max_scale=False (experimental in the reference) is not supported")
        self._need_gpu(ms_h_BChw[0], "embed_to_fhat")
        pns = self.v_patch_nums
        B, dev = ms_h_BChw[0].shape[0], ms_h_BChw[0].device
        ctx = self._ctx(dev, B, pns)
        H = pns[-1]
        f_hat = torch.zeros(B, self.Cvae, H, H, device=dev, dtype=torch.float32)
        out = []
        for si, pn in enumerate(pns):
            h = ms_h_BChw[si]
            if tuple(h.shape) != (B, self.Cvae, pn, pn):
                raise self._err(f"Quantizer.embed_to_fhat: scale {si} has shape {tuple(h.shape)}, expected {(B, self.Cvae, pn, pn)}")
            h_rows = h.to(dtype=torch.float32).permute(0, 2, 3, 1).contiguous()               # (B, pn^2, Cvae) rows
            nxt = torch.empty(B, pns[si + 1] ** 2, self.Cvae, device=dev) if si < len(pns) - 1 else None
            ctx.next_h(si, h_rows, f_hat, nxt, B)
            if not last_one:
                out.append(f_hat.clone())
        return f_hat if last_one else out

    def _ids_fhat(self, ms_idx_Bl: List[torch.Tensor], keep: bool, want_nxt: bool):
        """f_hat from per-scale ids (quant_next): the list of f_hat after every scale (keep) and / or the next-scale inputs (want_nxt)."""
        self._need_gpu(ms_idx_Bl[0], "idxBl")
        pns = self.v_patch_nums
        B, dev = ms_idx_Bl[0].shape[0], ms_idx_Bl[0].device
        ctx = self._ctx(dev, B, pns)
        f_hat = torch.zeros(B, self.Cvae, pns[-1], pns[-1], device=dev, dtype=torch.float32)
        fs, nxts = [], []
        n = len(ms_idx_Bl) if keep else len(pns) - 1
        for si in range(n):
            ids = ms_idx_Bl[si].to(dtype=torch.int64).contiguous()
            if tuple(ids.shape) != (B, pns[si] ** 2):
                raise self._err(f"Quantizer: ids of scale {si} have shape {tuple(ids.shape)}, expected {(B, pns[si] ** 2)}")
            nxt = torch.empty(B, pns[si + 1] ** 2, self.Cvae, device=dev) if si < len(pns) - 1 else None
            ctx.next(si, ids, pns[si] ** 2, f_hat, nxt, B)
            if keep:
                fs.append(f_hat.clone())
            if want_nxt:
                nxts.append(nxt)
        return fs, nxts

    @torch.no_grad()
    def idxBl_to_var_input(self, gt_ms_idx_Bl: List[torch.Tensor]) -> Optional[torch.Tensor]:     # quant.py:169-184
        """Teacher-forcing input: area_down(f_hat, pn_{s+1}) after scales 0 .. S-2, concatenated -> (B, L - pn_0^2, Cvae)."""
        if len(self.v_patch_nums) < 2:
            return None
        _, nxts = self._ids_fhat(gt_ms_idx_Bl, keep=False, want_nxt=True)
        return torch.cat(nxts, dim=1)


class _VaeForward:
    """VQVAE.forward (vqvae.py:56-59) on HIP: encoder -> Quantizer.forward -> decoder without the clamp."""

    def forward(self, inp: torch.Tensor, ret_usages=False):
        """-> (rec, usages, vq_loss): rec (B, 3, H, W) the UNCLAMPED reconstruction of inp (B, 3, H, W) in [-1, 1]; usages / vq_loss as Quantizer.forward."""
        rec, usages, loss, _ = self._forward_hip(inp, ret_usages)
        return rec, usages, torch.tensor(loss, dtype=torch.float32, device=rec.device)

    def _forward_hip(self, inp: torch.Tensor, ret_usages: bool):
        _refuse_forward(self, inp, "VQVAE.forward")
        with torch.no_grad():
            f_st, usages, loss, hits = self.quantize._forward_hip(self.img_to_f(inp.detach()), ret_usages)
            return self._decode(f_st, clamp=False), usages, loss, hits


class VQVAE(_VaeForward, nn.Module):
    def __init__(self, vocab_size=4096, z_channels=32, ch=128, share_quant_resi=4, v_patch_nums: Sequence[int] = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16),
                 test_mode=True, with_encoder=True, using_znorm=False, beta: float = 0.25, **_unused):
        super().__init__()
        self.V = self.vocab_size = vocab_size
        self.Cvae = z_channels
        ch_mult, nrb = (1, 1, 2, 2, 4), 2
        self._ch_mult, self._nrb, self._hip_ctx, self._hip_enc = ch_mult, nrb, None, None
        self.conv_mode: Optional[str] = None        # arithmetic of the decoder's convolutions (engine.CONV_MODES; None = SDVAR_CONV_MODE / the engine default); 'f16' = the
                                                    # opt-in one-product fp16 tier: not fp32-accurate.  The encoder never takes it
        self.with_encoder = bool(with_encoder)
        if with_encoder:
            self.encoder = Encoder(ch, ch_mult, nrb, z_channels)
        self.decoder = Decoder(ch, ch_mult, nrb, z_channels)
        self.downsample = 2 ** (len(ch_mult) - 1)
        self.quantize = Quantizer(vocab_size, z_channels, v_patch_nums, share_quant_resi, using_znorm, beta=beta)
        self.quant_conv = nn.Conv2d(z_channels, z_channels, 3, 1, 1)
        self.post_quant_conv = nn.Conv2d(z_channels, z_channels, 3, 1, 1)
        if test_mode:
            self.eval()
            for p in self.parameters():
                p.requires_grad_(False)

    @torch.no_grad()
    def fhat_to_img(self, f_hat: torch.Tensor) -> torch.Tensor:      # vqvae.py:62-63
        """(B, Cvae, h, w) -> (B, 3, 16h, 16w) in [-1, 1] on the HIP decoder.  GPU tensors only: there is no CPU path."""
        return self._decode(f_hat, clamp=True)

    def _decode(self, f_hat: torch.Tensor, clamp: bool) -> torch.Tensor:
        from . import engine as E
        if not f_hat.is_cuda:
            raise E.SdvarError("VQVAE: decoding (fhat_to_img, forward) runs on the HIP decoder and needs a GPU tensor (tests/torch_ref.py holds the PyTorch test reference)")
        B, hw = f_hat.shape[0], f_hat.shape[-1]
        ctx, mode = self._hip_ctx, E.resolve_conv_mode(self.conv_mode)
        if ctx is None or ctx.device != f_hat.device or ctx.max_batch < B or ctx.latent_hw != hw or ctx.conv_mode != mode:
            if ctx is not None:
                ctx.close()
            sd = {k: v for k, v in self.state_dict().items() if k.startswith(("decoder.", "post_quant_conv."))}
            ctx = self._hip_ctx = E.VaeCtx(sd, B, f_hat.device, latent_hw=hw, ch_mult=self._ch_mult, num_res_blocks=self._nrb, conv_mode=mode)
        return ctx.decode(f_hat, clamp=clamp)

    @torch.no_grad()
    def img_to_f(self, img: torch.Tensor) -> torch.Tensor:
        """quant_conv(encoder(img)) (vqvae.py:66): (B, 3, H, W) in [-1, 1] -> (B, Cvae, H/16, W/16) on the HIP encoder."""
        from . import engine as E
        if not self.with_encoder:
            raise E.SdvarError("VQVAE: built with with_encoder=False, so it cannot encode images")
        if not img.is_cuda:
            raise E.SdvarError("VQVAE image encoding runs on the HIP encoder and needs a GPU tensor (tests/torch_ref_encode.py holds the PyTorch test reference)")
        B, H, W = img.shape[0], img.shape[-2], img.shape[-1]
        if img.dim() != 4 or img.shape[1] != 3 or H != W or H % self.downsample:
            raise E.SdvarError(f"VQVAE: image of shape {tuple(img.shape)}: expected (B, 3, H, H) with H a multiple of {self.downsample}")
        hw = H // self.downsample
        ctx = self._hip_enc
        if ctx is None or ctx.device != img.device or ctx.max_batch < B or ctx.latent_hw != hw:
            if ctx is not None:
                ctx.close()
            sd = {k: v for k, v in self.state_dict().items() if k.startswith(("encoder.", "quant_conv."))}
            ctx = self._hip_enc = E.VaeEncCtx(sd, B, img.device, latent_hw=hw, ch_mult=self._ch_mult, num_res_blocks=self._nrb)
        return ctx.encode(img)

    @torch.no_grad()
    def img_to_idxBl(self, inp_img_no_grad: torch.Tensor, v_patch_nums=None) -> List[torch.Tensor]:           # vqvae.py:65-67
        return self.quantize.f_to_idxBl_or_fhat(self.img_to_f(inp_img_no_grad), to_fhat=False, v_patch_nums=v_patch_nums)

    @torch.no_grad()
    def idxBl_to_img(self, ms_idx_Bl: List[torch.Tensor], same_shape: bool, last_one=False) -> Union[List[torch.Tensor], torch.Tensor]:   # vqvae.py:69-76
        if not same_shape:
            raise self.quantize._err("VQVAE.idxBl_to_img: same_shape=False (all_to_max_scale=False, experimental in the reference) is not supported")
        fs, _ = self.quantize._ids_fhat(ms_idx_Bl, keep=True, want_nxt=False)
        return self.fhat_to_img(fs[-1]) if last_one else [self.fhat_to_img(f) for f in fs]

    @torch.no_grad()
    def embed_to_img(self, ms_h_BChw: List[torch.Tensor], all_to_max_scale: bool, last_one=False) -> Union[List[torch.Tensor], torch.Tensor]:   # vqvae.py:78-82
        fs = self.quantize.embed_to_fhat(ms_h_BChw, all_to_max_scale=all_to_max_scale, last_one=last_one)
        return self.fhat_to_img(fs) if last_one else [self.fhat_to_img(f) for f in fs]

    @torch.no_grad()
    def img_to_reconstructed_img(self, x: torch.Tensor, v_patch_nums=None, last_one=False) -> Union[List[torch.Tensor], torch.Tensor]:   # vqvae.py:84-90
        fs = self.quantize.f_to_idxBl_or_fhat(self.img_to_f(x), to_fhat=True, v_patch_nums=v_patch_nums)
        return self.fhat_to_img(fs[-1]) if last_one else [self.fhat_to_img(f) for f in fs]

    def refresh_hip(self):
        """Drop the HIP copies of the weights (decoder, encoder, quantizer; call after changing parameters in place)."""
        if self._hip_ctx is not None:
            self._hip_ctx.close()
        if self._hip_enc is not None:
            self._hip_enc.close()
        self._hip_ctx = self._hip_enc = None
        self.quantize.refresh_hip()

    def load_state_dict(self, state_dict, strict=True, assign=False):  # vqvae.py:92-95
        key = "quantize.ema_vocab_hit_SV"
        if key in state_dict and state_dict[key].shape[0] != self.quantize.ema_vocab_hit_SV.shape[0]:
            state_dict[key] = self.quantize.ema_vocab_hit_SV
        self.refresh_hip()
        return super().load_state_dict(state_dict, strict=strict, assign=assign)
