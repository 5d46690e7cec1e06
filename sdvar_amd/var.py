"""Host-side mirror of the reference's `models.var` API for the sampling path: VAR and SDVAR.

Same constructor arguments, attribute names, sampler signatures and state_dict keys as
/root/reference/models/var.py:22-215 (VAR) and :535-1383 (SDVAR), so existing callers and upstream checkpoints work
unchanged - but the modules here only HOLD parameters; every sampler call runs on the gfx950 kernels through
sdvar_amd.engine (C ABI).  VAR.forward is the teacher-forced pass of var.py:217-259 for scoring (validation loss and
accuracy, sdvar_amd.evaluate); it returns logits without an autograd graph.  Training (backward, dropout, progressive
training) is outside the scope table.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn

from . import engine as E
from .ladder import as_ladder
from .vqvae import VQVAE

# images per pass of VAR.forward (M = L * TF_PASS_IMAGES rows per GEMM), from tools/eval_bench.py: at 256^2 a d16 pass
# runs 915 / 1012 / 1119 images/s at 8 / 16 / 32 images (f16x2), d30 195 / 201 / 203
TF_PASS_IMAGES = 32
# images per call of autoregressive_infer_cfg_edit: the sampler kernels put the image index on the grid's y axis (65535 at the most)
MAX_EDIT_BATCH = 65535


class _SelfAttention(nn.Module):                   # parameter names of basic_var.py:58-87
    def __init__(self, C, H, attn_l2_norm=True):
        super().__init__()
        self.num_heads, self.head_dim, self.attn_l2_norm = H, C // H, attn_l2_norm
        if attn_l2_norm:                                # basic_var.py:66-72: otherwise plain scaled dot-product attention, scale 0.25 / sqrt(head_dim)
            self.scale_mul_1H11 = nn.Parameter(torch.full((1, H, 1, 1), 4.0).log())
        self.mat_qkv = nn.Linear(C, 3 * C, bias=False)
        self.q_bias, self.v_bias = nn.Parameter(torch.zeros(C)), nn.Parameter(torch.zeros(C))
        self.register_buffer("zero_k_bias", torch.zeros(C))
        self.proj = nn.Linear(C, C)
        self.caching = False
        self._owner = None

    def kv_caching(self, enable: bool):             # basic_var.py:87: toggling resets the cache
        self.caching = enable
        if self._owner is not None:
            self._owner()._kv_reset()


class _FFN(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(C, 4 * C), nn.Linear(4 * C, C)


class _Block(nn.Module):
    def __init__(self, C, H, shared_aln=False, attn_l2_norm=True):
        super().__init__()
        self.attn, self.ffn = _SelfAttention(C, H, attn_l2_norm), _FFN(C)
        self.shared_aln = shared_aln
        if shared_aln:                                                   # basic_var.py:143-144
            self.ada_gss = nn.Parameter(torch.randn(1, 1, 6, C) / C ** 0.5)
        else:
            self.ada_lin = nn.Sequential(nn.SiLU(inplace=False), nn.Linear(C, 6 * C))


class _HeadNorm(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.ada_lin = nn.Sequential(nn.SiLU(inplace=False), nn.Linear(C, 2 * C))


class VAR(nn.Module):
    def __init__(self, vae_local: VQVAE, num_classes=1000, depth=16, embed_dim=1024, num_heads=16, mlp_ratio=4., drop_rate=0.,
                 attn_drop_rate=0., drop_path_rate=0., norm_eps=1e-6, shared_aln=False, cond_drop_rate=0.1, attn_l2_norm=False,
                 patch_nums=(1, 2, 3, 4, 5, 6, 8, 10, 13, 16), flash_if_available=True, fused_if_available=True):
        super().__init__()
        assert embed_dim % num_heads == 0
        if embed_dim != 64 * num_heads or num_heads != depth or mlp_ratio != 4.:
            raise NotImplementedError("the HIP path assumes head_dim 64, heads == depth, mlp_ratio 4 (models/__init__.py:26-27)")
        self.Cvae, self.V = vae_local.Cvae, vae_local.vocab_size
        self.depth, self.C, self.D, self.num_heads = depth, embed_dim, embed_dim, num_heads
        self.patch_nums: Tuple[int] = tuple(patch_nums)
        lad = as_ladder(patch_nums)
        self.L, self.first_l = lad.L, lad.lens[0]
        self.begin_ends = [(lad.begin(s), lad.cum[s]) for s in range(lad.S)]
        self.num_stages_minus_1 = lad.S - 1
        self.num_classes = num_classes
        self.cond_drop_rate = cond_drop_rate
        self.drop_rate, self.attn_drop_rate, self.drop_path_rate = drop_rate, attn_drop_rate, drop_path_rate
        self.prog_si = -1                           # progressive training is not supported (quant.py:42: "prog_si always -1")
        self.vae_proxy, self.vae_quant_proxy = (vae_local,), (vae_local.quantize,)
        C = embed_dim
        self.word_embed = nn.Linear(self.Cvae, C)
        self.class_emb = nn.Embedding(num_classes + 1, C)
        self.pos_start = nn.Parameter(torch.zeros(1, self.first_l, C))
        self.pos_1LC = nn.Parameter(torch.zeros(1, self.L, C))
        self.lvl_embed = nn.Embedding(lad.S, C)
        self.shared_aln = bool(shared_aln)
        self.shared_ada_lin = nn.Sequential(nn.SiLU(inplace=False), nn.Linear(C, 6 * C)) if shared_aln else nn.Identity()   # var.py:81
        self.attn_l2_norm = bool(attn_l2_norm)
        self.blocks = nn.ModuleList([_Block(C, num_heads, shared_aln, self.attn_l2_norm) for _ in range(depth)])
        lvl = torch.cat([torch.full((n,), i, dtype=torch.int64) for i, n in enumerate(lad.lens)]).view(1, self.L)
        self.register_buffer("lvl_1L", lvl)
        d = lvl.view(1, self.L, 1)
        self.register_buffer("attn_bias_for_masking", torch.where(d >= d.transpose(1, 2), 0., -torch.inf).reshape(1, 1, self.L, self.L).contiguous())
        self.head_nm = _HeadNorm(C)
        self.head = nn.Linear(C, self.V)
        self.rng = torch.Generator(device="cpu")
        import weakref
        for b in self.blocks:
            b.attn._owner = weakref.ref(self)
        self._ctx: Optional[E.ModelCtx] = None
        self._sampler: Optional[E.Sampler] = None
        self._quant: Optional[E.QuantCtx] = None
        self._tf_ctx: Optional[E.ModelCtx] = None   # VAR.forward's own model object (teacher forcing): the sampler's context stays untouched
        self.tf_pass_images = TF_PASS_IMAGES
        self.tf_gemm_mode: Optional[str] = None     # GEMM arithmetic of VAR.forward (engine.ENGINE_GEMM_MODES; None = the engine default)
        self.gemm_mode: Optional[str] = None        # GEMM arithmetic of the sampler's model object (engine.ENGINE_GEMM_MODES; None = the engine default); 'f16' = the opt-in
                                                    # fp16 tier for the large stages: not fp32-accurate, sampled ids differ from the reference's
        self.noise_kind = "device"                  # 'device' | 'host' | 'torch' (sdvar_amd.engine.Noise)
        self.last_result: Optional[E.SampleResult] = None

    # ---- engine plumbing ---------------------------------------------------------------------------------------
    def _device(self):
        return self.lvl_1L.device

    def _kv_reset(self):
        if self._ctx is not None and self._ctx.kv_len() > 0:
            self._ctx.kv_set_len(0)

    def invalidate_engine(self):
        """Call after changing parameters in place (load_state_dict does it automatically)."""
        self._ctx = self._sampler = self._quant = self._tf_ctx = None

    def load_state_dict(self, *a, **kw):
        out = super().load_state_dict(*a, **kw)
        self.invalidate_engine()
        return out

    def _apply(self, fn, *a, **kw):                 # .to()/.cuda() move the tensors the engine points at
        self.invalidate_engine()
        return super()._apply(fn, *a, **kw)

    def engine_ctx(self, max_batch: int, max_chunk: int = 1) -> E.ModelCtx:
        dev = self._device()
        if dev.type != "cuda":
            raise E.SdvarError("the sampler runs on an MI355X: move the model to a cuda (HIP) device; there is no CPU path")
        c = self._ctx
        if c is None or c.max_batch < max_batch or c.max_chunk < max_chunk or c.device != dev or c.gemm_mode != (self.gemm_mode or c.gemm_mode):
            if c is not None:
                c.close()
            self._ctx = E.ModelCtx(self.state_dict(), self.depth, self.patch_nums, max_batch, max_chunk, dev, self.num_classes, gemm_mode=self.gemm_mode)
            self._sampler = None
        return self._ctx

    def quant_ctx(self, max_batch: int) -> E.QuantCtx:
        q = self._quant
        if q is None or q.lad.patch_nums != self.patch_nums or q.device != self._device() or q.max_batch < max_batch:
            if q is not None:                                  # a larger batch than the cached quantizer was sized for: rebuild it
                q.close()
                self._sampler = None
            sd = {"quantize." + k: v for k, v in self.vae_quant_proxy[0].state_dict().items()}
            self._quant = E.QuantCtx(sd, self.patch_nums, max(max_batch, 1), self._device())
        return self._quant

    def _labels(self, B, label_B, rng):             # var.py:147-150
        dev = self._device()
        if label_B is None:
            p = torch.full((1, self.num_classes), 1.0 / self.num_classes)
            label_B = torch.multinomial(p, num_samples=B, replacement=True, generator=rng).reshape(B)
        elif isinstance(label_B, int):
            label_B = torch.full((B,), fill_value=self.num_classes if label_B < 0 else label_B)
        label_B = label_B.to(device=dev, dtype=torch.int64).contiguous()
        assert label_B.shape == (B,)
        return label_B

    def _noise(self, g_seed, image_offset=0) -> E.Noise:
        seed = int(torch.seed() & 0x7FFFFFFFFFFFFFFF) if g_seed is None else E._as_rows("g_seed", g_seed, int)
        if self.noise_kind == "torch":
            return E.Noise("torch", seed, generator=self.rng if g_seed is not None else None)
        return E.Noise(self.noise_kind, seed, image_offset)

    # ---- the sampler (var.py:127-215) ----------------------------------------------------------------------------
    @torch.no_grad()
    def autoregressive_infer_cfg(self, B: int, label_B: Optional[Union[int, torch.LongTensor]], g_seed: Optional[int] = None, cfg=1.5,
                                 top_k=0, top_p=0.0, more_smooth=False) -> torch.Tensor:
        """var.py:127-215.  An extension of the reference's call: `cfg`, `top_k`, `top_p` and `g_seed` each also take a length-B sequence, numpy array or
        tensor - image b is then sampled with its own values, and with a sequence of seeds it draws what a B = 1 call with g_seed = g_seed[b] draws
        (INTEGRATION.md section 3).  A wrong length, or a sequence of seeds with label_B=None (the label draw needs one generator), raises SdvarError."""
        g_seed = _seed_arg(g_seed, B, label_B)
        if g_seed is None or isinstance(g_seed, list):
            rng = None
        else:
            self.rng.manual_seed(g_seed); rng = self.rng
        _row_lengths(B, cfg=cfg, top_k=top_k, top_p=top_p)
        labels = self._labels(B, label_B, rng)
        ctx = self.engine_ctx(B, 1)
        qc = self.quant_ctx(ctx.max_batch)
        if self._sampler is None or self._sampler.t is not ctx or self._sampler.q is not qc:
            self._sampler = E.Sampler(ctx, qc)
        res = self._sampler.plain_ar(labels, cfg, top_k, top_p, self._noise(g_seed), more_smooth=bool(more_smooth))   # more_smooth: var.py:206-208
        self.last_result = res
        return self.vae_proxy[0].fhat_to_img(res.f_hat.clone()).add_(1).mul_(0.5)

    # ---- masked sampling: in-painting, out-painting, class-conditional editing (an extension; the reference has no such call) -------------
    @torch.no_grad()
    def autoregressive_infer_cfg_edit(self, image: torch.Tensor, mask: torch.Tensor, label_B: Optional[Union[int, torch.LongTensor]], g_seed: Optional[int] = None,
                                      cfg=1.5, top_k=0, top_p=0.0, composite: bool = True, more_smooth: bool = False) -> torch.Tensor:
        """Regenerate the masked region of `image` under `label_B` and keep the rest: (B, 3, H, H) in [0, 1].
        image: (B, 3, H, H) fp32 GPU tensor in [-1, 1] (what VQVAE.img_to_idxBl takes), H = 16 * patch_nums[-1].  mask: (B, H, H), (B, 1, H, H) or (H, H) bool /
        uint8 GPU tensor, non-zero = regenerate; a 2-D mask serves every image.  label_B, g_seed, cfg, top_k, top_p: as autoregressive_infer_cfg takes them,
        per-image sequences included.  The image is encoded to its multi-scale ids; at every scale the tokens whose window (the pixels area interpolation
        averages into them) is at least half masked are sampled and the others keep the image's own id (engine.mask_tokens, Sampler.plain_ar(force_ids, gen));
        the result is decoded and, with composite=True, the pixels outside the mask are put back: they are then the bits of image.add(1).mul(0.5).  With
        composite=False the decoder's output is returned as it is, and kept pixels move (the decoder's receptive field, the bicubic up-sampling of coarse
        tokens).  more_smooth=True raises SdvarError (the gumbel mix of a forced token is undefined).  last_result additionally carries `gen`, the (B, L) table."""
        who = "autoregressive_infer_cfg_edit"
        vae = self.vae_proxy[0]
        B, H = _edit_args(who, self, image, mask, more_smooth)
        g_seed = _seed_arg(g_seed, B, label_B)
        if g_seed is None or isinstance(g_seed, list):
            rng = None
        else:
            self.rng.manual_seed(g_seed); rng = self.rng
        _row_lengths(B, cfg=cfg, top_k=top_k, top_p=top_p)
        labels = self._labels(B, label_B, rng)
        image, mask_px = _edit_operands(image, mask, B, H)
        try:
            ctx = self.engine_ctx(B, 1)
            qc = self.quant_ctx(ctx.max_batch)
            if self._sampler is None or self._sampler.t is not ctx or self._sampler.q is not qc:
                self._sampler = E.Sampler(ctx, qc)
        except torch.cuda.OutOfMemoryError as e:
            self.invalidate_engine()
            raise E.SdvarError(f"{who}: image: the sampler contexts cannot be built for a batch of {B} images: {e}") from None
        force_ids = torch.cat(vae.img_to_idxBl(image, v_patch_nums=self.patch_nums), dim=1).contiguous()                     # (B, L): the image's own ids, stage s at [begin(s), begin(s) + pn_s^2)
        gen = E.mask_tokens(mask_px, self.patch_nums)
        res = self._sampler.plain_ar(labels, cfg, top_k, top_p, self._noise(g_seed), force_ids=force_ids, gen=gen, trusted_ids=True)
        res.gen = gen
        self.last_result = res
        out = vae.fhat_to_img(res.f_hat.clone())
        if composite:
            return E.img_composite(out, image, mask_px, out=out)
        return out.add_(1).mul_(0.5)

    @torch.no_grad()
    def autoregressive_infer_cfg_sd_helper1(self, B: int, current_step: int, step: int, next_token_map, f_hat, rng, sos, lvl_pos, cfg=1.5, top_k=0, top_p=0.0,
                                            more_smooth=False):
        """var.py:319-443: `step` stages of the sampler from stage `current_step`, from a handed-in (next_token_map, f_hat) and the conditioning rows `sos`
        (2B, C) of SDVAR.init_param; returns (input_token_history, f_hat_history, logits_history, token_id_history) as the reference builds them.  `lvl_pos`
        is the model's own table (init_param hands it back unchanged, var.py:598): it is checked for shape and otherwise taken from the bound weights.
        `rng`: a CPU torch.Generator (the reference's stream on this host), an engine.Noise, or None (device Philox, fresh seed)."""
        S = len(self.patch_nums)
        E.scalar_arg("autoregressive_infer_cfg_sd_helper1", cfg=cfg, top_k=top_k, top_p=top_p)
        assert 0 <= current_step < S and step >= 1
        assert sos.shape == (2 * B, self.C), tuple(sos.shape)
        assert lvl_pos is None or tuple(lvl_pos.shape[-2:]) == (self.L, self.C), tuple(lvl_pos.shape)
        dev = self._device()
        ctx = self.engine_ctx(B, 1)
        qc = self.quant_ctx(ctx.max_batch)
        if self._sampler is None or self._sampler.t is not ctx or self._sampler.q is not qc:
            self._sampler = E.Sampler(ctx, qc)
        if isinstance(rng, E.Noise):
            noise = rng
        elif rng is not None:
            noise = E.Noise("torch", 0, generator=rng)
        else:
            noise = self._noise(None)
        if not (f_hat.is_cuda and f_hat.dtype == torch.float32 and f_hat.is_contiguous()):
            raise E.SdvarError("autoregressive_infer_cfg_sd_helper1: f_hat must be a contiguous fp32 GPU tensor (it is updated in place, quant.py:191)")
        nm = None if (next_token_map is None or current_step == 0) else next_token_map.to(dev)
        return self._sampler.resume_ar(sos.to(device=dev, dtype=torch.float32).contiguous(), current_step, step, nm, f_hat, cfg, top_k, top_p, noise,
                                       more_smooth=bool(more_smooth))

    def tf_ctx(self, images: int) -> E.ModelCtx:
        """The model object of VAR.forward: passes of up to `images` unpaired rows over all S stages at once (max_batch = ceil(images / 2),
        max_chunk = S).  A second weight-plane copy beside the sampler's, so sampling state is never disturbed."""
        dev, S = self._device(), len(self.patch_nums)
        c, mb = self._tf_ctx, (images + 1) // 2
        if c is None or c.max_batch < mb or c.device != dev or c.gemm_mode != (self.tf_gemm_mode or c.gemm_mode):
            if c is not None:
                c.close()
            self._tf_ctx = c = E.ModelCtx(self.state_dict(), self.depth, self.patch_nums, mb, S, dev, self.num_classes, gemm_mode=self.tf_gemm_mode)
        return c

    @torch.no_grad()
    def forward(self, label_B: torch.LongTensor, x_BLCv_wo_first_l: torch.Tensor) -> torch.Tensor:
        """Teacher-forced logits (var.py:217-259): label_B (B,) int64, x_BLCv_wo_first_l (B, L-1, Cvae) fp32 (VectorQuantizer2.idxBl_to_var_input)
        -> logits (B, L, V) fp32 on the model's device.  Token 0 is (class_emb[label'] + pos_start) + lvl_pos[0], token t >= 1 is
        word_embed(x[:, t-1]) + lvl_pos[t]; every block runs under the block-causal mask, then head(head_nm(x, cond)).

        Condition dropout as in the reference, in eval mode too: label' = where(torch.rand(B, device=label_B.device) < cond_drop_rate,
        num_classes, label_B) - one draw from that device's global generator, even at rate 0.  Set `cond_drop_rate = 0` for deterministic
        validation numbers.  The returned logits carry NO autograd graph (no backward on the HIP path).  Images run in passes of at most
        `tf_pass_images` rows, each through sdvar_model_begin_rows / sdvar_embed_teacher / sdvar_stage_forward over all stages.

        Raises SdvarError for prog_si != -1, for training mode with a non-zero drop_rate / attn_drop_rate / drop_path_rate (the HIP path has no
        dropout: call .eval()), for wrong shapes or dtypes, and for CPU tensors."""
        if self.prog_si != -1:
            raise E.SdvarError(f"VAR.forward: prog_si={self.prog_si}: progressive training is not supported (prog_si must be -1)")
        if self.training and (self.drop_rate or self.attn_drop_rate or self.drop_path_rate):
            raise E.SdvarError("VAR.forward: the module is in training mode with dropout (drop_rate / attn_drop_rate / drop_path_rate), which the HIP "
                               "path does not apply: call .eval() first")
        if not isinstance(label_B, torch.Tensor) or label_B.dim() != 1 or label_B.dtype not in (torch.int64, torch.int32):
            raise E.SdvarError(f"VAR.forward: label_B must be a (B,) integer tensor, got {getattr(label_B, 'shape', type(label_B))}")
        B, Lm1 = label_B.shape[0], self.L - self.first_l
        x = x_BLCv_wo_first_l
        if B < 1 or not isinstance(x, torch.Tensor) or tuple(x.shape) != (B, Lm1, self.Cvae) or not x.is_floating_point():
            raise E.SdvarError(f"VAR.forward: x_BLCv_wo_first_l must be a float ({B}, {Lm1}, {self.Cvae}) tensor, got {tuple(getattr(x, 'shape', ()))}")
        dev = self._device()
        if dev.type != "cuda" or not label_B.is_cuda or not x.is_cuda:
            raise E.SdvarError("VAR.forward runs on an MI355X: the model, label_B and x_BLCv_wo_first_l must be on a cuda (HIP) device; there is no CPU path")
        drop = torch.rand(B, device=label_B.device) < self.cond_drop_rate            # var.py:231, the reference's single draw
        labels = label_B.to(torch.int64).masked_fill(drop, self.num_classes).to(dev).contiguous()
        xv = x.to(device=dev, dtype=torch.float32).contiguous()
        P = max(1, int(self.tf_pass_images))
        ctx = self.tf_ctx(min(B, P))
        L, C = self.L, self.C
        out = torch.empty(B, L, self.V, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            xb = torch.empty(min(B, P), L, C, device=dev, dtype=torch.float32)
            for lo in range(0, B, P):
                n = min(P, B - lo)
                ctx.begin_rows(labels[lo:lo + n])
                ctx.embed_teacher(xv[lo:lo + n], xb[:n])
                ctx.forward(xb[:n], 0, len(self.patch_nums), out[lo:lo + n])
        return out

    def init_weights(self, init_adaln=0.5, init_adaln_gamma=1e-5, init_head=0.02, init_std=0.02, conv_std_or_gain=0.02, seed: int = 1234):
        """Distributions of var.py:261-311 drawn from a seeded generator (sdvar_amd.weights 'perf' init): trunc-normal(init_std; < 0 =
        sqrt(1/C/3)) Linear / Embedding / positional tensors, head x init_head, head_nm and the adaLN scale/shift rows x init_adaln, the
        adaLN gamma rows x init_adaln_gamma, proj / fc2 / sqrt(2 depth), zero biases.  conv_std_or_gain only concerns convolutions, of
        which a VAR has none (var.py:275)."""
        from .weights import var_state_dict
        sd = var_state_dict(self.depth, self.patch_nums, "perf", seed, V=self.V, Cvae=self.Cvae, num_classes=self.num_classes, shared_aln=self.shared_aln, attn_l2_norm=self.attn_l2_norm,
                            init_adaln=init_adaln, init_adaln_gamma=init_adaln_gamma, init_head=init_head, init_std=init_std)
        self.load_state_dict({k: v.to(self._device()) for k, v in sd.items()})


try:                                                     # optional: only the from_pretrained / save_pretrained conveniences need it
    from huggingface_hub import PyTorchModelHubMixin as _HubMixin
except Exception:                                        # pragma: no cover - huggingface_hub not installed
    class _HubMixin:                                     # type: ignore[no-redef]
        pass


class VARHF(VAR, _HubMixin):
    """models/var.py:513-533: VAR that builds its own VQVAE from `vae_kwargs` and carries the Hugging Face hub mixin
    (`VARHF.from_pretrained(local_dir)` loads a `config.json` + weights directory; there is no network on the GPU boxes)."""

    def __init__(self, vae_kwargs, num_classes=1000, depth=16, embed_dim=1024, num_heads=16, mlp_ratio=4., drop_rate=0., attn_drop_rate=0.,
                 drop_path_rate=0., norm_eps=1e-6, shared_aln=False, cond_drop_rate=0.1, attn_l2_norm=False,
                 patch_nums=(1, 2, 3, 4, 5, 6, 8, 10, 13, 16), flash_if_available=True, fused_if_available=True):
        super().__init__(vae_local=VQVAE(**vae_kwargs), num_classes=num_classes, depth=depth, embed_dim=embed_dim, num_heads=num_heads,
                         mlp_ratio=mlp_ratio, drop_rate=drop_rate, attn_drop_rate=attn_drop_rate, drop_path_rate=drop_path_rate, norm_eps=norm_eps,
                         shared_aln=shared_aln, cond_drop_rate=cond_drop_rate, attn_l2_norm=attn_l2_norm, patch_nums=patch_nums,
                         flash_if_available=flash_if_available, fused_if_available=fused_if_available)


def _edit_args(who: str, model: "VAR", image, mask, more_smooth: bool):
    """The argument contract of the edit calls (VAR.autoregressive_infer_cfg_edit, SDVAR.sdvar_autoregressive_infer_cfg_parallel_v1_edit), checked before anything
    is built or launched; `model` is the VAR whose VQVAE encodes the image.  Returns (B, H)."""
    if more_smooth:
        raise E.SdvarError(f"{who}: more_smooth=True is not supported with a mask: the gumbel mix of a forced token is undefined")
    vae = model.vae_proxy[0]
    if not getattr(vae, "with_encoder", False):
        raise E.SdvarError(f"{who}: image: the VQVAE was built with with_encoder=False, so it cannot encode the image to edit")
    H = vae.downsample * model.patch_nums[-1]
    if not isinstance(image, torch.Tensor) or image.dim() != 4 or image.shape[0] < 1 or image.shape[1] != 3 or image.dtype != torch.float32:
        what = f"{tuple(image.shape)} {image.dtype}" if isinstance(image, torch.Tensor) else type(image).__name__
        raise E.SdvarError(f"{who}: image must be a (B, 3, H, H) float32 tensor in [-1, 1], got {what}")
    B = int(image.shape[0])
    if tuple(image.shape[2:]) != (H, H):
        raise E.SdvarError(f"{who}: image is {image.shape[2]} x {image.shape[3]}, but the ladder {model.patch_nums} generates {H} x {H} images")
    if B > MAX_EDIT_BATCH:
        raise E.SdvarError(f"{who}: image: a batch of {B} images is more than the sampler contexts can be built for ({MAX_EDIT_BATCH})")
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8):
        what = f"{mask.dtype}" if isinstance(mask, torch.Tensor) else type(mask).__name__
        raise E.SdvarError(f"{who}: mask must be a bool or uint8 tensor (non-zero = regenerate), got {what}")
    if tuple(mask.shape) not in ((B, H, H), (B, 1, H, H), (H, H)):
        raise E.SdvarError(f"{who}: mask has shape {tuple(mask.shape)}, expected {(B, H, H)}, {(B, 1, H, H)} or {(H, H)}")
    dev = model._device()
    for name, t in (("image", image), ("mask", mask)):
        if not t.is_cuda or t.device != dev:
            raise E.SdvarError(f"{who}: {name} is on {t.device}, the model on {dev}: masked sampling runs on the GPU and there is no CPU path")
    return B, H


def _edit_operands(image: torch.Tensor, mask: torch.Tensor, B: int, H: int):
    """(image, mask_px): the dense image and the (B, H, H) uint8 pixel mask the kernels take."""
    mask_px = (mask.expand(B, H, H) if mask.dim() == 2 else mask.reshape(B, H, H)).contiguous()
    if mask_px.dtype == torch.bool:
        mask_px = mask_px.view(torch.uint8)                      # a bool tensor is one byte per element, 0 / 1
    return image.contiguous(), mask_px


def _seed_arg(g_seed, B: int, label_B):
    """g_seed as the samplers take it: None, one int, or a list of B ints (per-image seeds; they need explicit labels)."""
    if g_seed is None:
        return None
    g_seed = E._as_rows("g_seed", g_seed, int)
    if isinstance(g_seed, list):
        if len(g_seed) != B:
            raise E.SdvarError(f"g_seed: {len(g_seed)} entries for a batch of {B} images")
        if label_B is None:
            raise E.SdvarError("g_seed: a sequence of seeds needs label_B: the label draw of label_B=None takes one generator")
    return g_seed


def _row_lengths(B: int, **named):
    for name, v in named.items():
        v = E._as_rows(name, v, float)
        if isinstance(v, list) and len(v) != B:
            raise E.SdvarError(f"{name}: {len(v)} entries for a batch of {B} images")


class SDVAR(nn.Module):
    """Speculative draft -> verify sampler over a (draft, target) VAR pair (models/var.py:535-1383)."""

    def __init__(self, draft_model: VAR, target_model: VAR, similarity_thresh: float = 0.8):
        super().__init__()
        self.draft_model, self.target_model = draft_model, target_model
        self.similarity_thresh = similarity_thresh     # stored and never read, as in the reference (var.py:546)
        self.match_threshold = 0.5                      # the constant of var.py:1215
        self.match_rule = E.MatchRule()                 # advanced_token_matching's rule (var.py:1229-1243); the default is the reference's fall-back
        self.noise_kind = "device"
        self.accept_scope = "shard"
        self._sampler: Optional[E.Sampler] = None
        self.last_result: Optional[E.SampleResult] = None

    # ---- the reference's helper methods (var.py:580-601, 871-1282), each a thin call into the engine --------------
    def init_param(self, model: VAR, B: int, label_B):
        """var.py:580-601 -> (sos, cond_BD, cond_BD_or_gss, lvl_pos, first_token_map, first_f_hat), computed by
        sdvar_model_begin on the device."""
        labels = model._labels(B, label_B, None)
        ctx = model.engine_ctx(B, 1)
        with torch.cuda.device(ctx.device):
            ctx.begin(labels)
            cond, lvl_pos, first = ctx.export_prologue()
        f_hat = cond.new_zeros(B, model.Cvae, model.patch_nums[-1], model.patch_nums[-1])
        return cond, cond, cond, lvl_pos, first, f_hat

    def _get_sampler(self, B: int, chunk: int) -> E.Sampler:
        d, t = self.draft_model, self.target_model
        assert d.patch_nums == t.patch_nums                                   # var.py:877
        dc, tc = d.engine_ctx(B, 1), t.engine_ctx(B, max(chunk, 1))
        qc = t.quant_ctx(max(tc.max_batch, dc.max_batch))
        s = self._sampler
        if s is None or s.t is not tc or s.d is not dc or s.q is not qc:
            self._sampler = E.Sampler(tc, qc, dc)
        return self._sampler

    def _prepare(self, B: int, label_B, g_seed: Optional[int], chunk: int, rng: Optional[torch.Generator] = None):
        """Labels, sampler objects and the noise source of one call (var.py:641-656, 880-902)."""
        t = self.target_model
        g_seed = _seed_arg(g_seed, B, label_B)
        if g_seed is not None and rng is None and not isinstance(g_seed, list):
            rng = torch.Generator(device="cpu"); rng.manual_seed(g_seed)      # var.py:882-887
        labels = t._labels(B, label_B, rng)
        smp = self._get_sampler(B, chunk)
        seed = int(torch.seed() & 0x7FFFFFFFFFFFFFFF) if g_seed is None else g_seed
        noise = E.Noise("torch", seed, generator=rng) if self.noise_kind == "torch" else E.Noise(self.noise_kind, seed)
        return labels, smp, noise

    def _initialize_inference_state(self, B: int, label_B, g_seed: Optional[int], cfg: float, gamma: int) -> E.SpecState:
        """var.py:871-947.  The returned state carries the reference's field names (current_stage, gamma, total_stages,
        accept_count, target_calls, patch_nums, cfg, top_k, top_p, draft_f_hat, target_f_hat)."""
        E.scalar_arg("_initialize_inference_state", g_seed=g_seed, cfg=cfg)
        labels, smp, noise = self._prepare(B, label_B, g_seed, gamma)
        st = smp.spec_begin(labels, cfg, gamma, 0, 0.0, noise, thr=self.match_threshold, match=self.match_rule)   # top_k / top_p set by the caller (var.py:937-938)
        st.accept_scope = self.accept_scope
        return st

    def draft_generate_batch(self, state: E.SpecState, B: int):
        """var.py:949-1024 -> list of g token tensors (B, pn^2) int64 for stages current_stage .. current_stage+g-1."""
        smp, lad = state.sampler, state.sampler.lad
        _mask_free("draft_generate_batch", state)
        if state.rows is None:                      # a state begun with scalars samples with the scalars it carries now (var.py:937-938 sets top_k / top_p on it)
            E.scalar_arg("draft_generate_batch", cfg=state.cfg, top_k=state.top_k, top_p=state.top_p)
        g = smp.spec_draft(state)
        cur = state.current_stage
        return [smp.ids[:B, lad.begin(cur + j):lad.begin(cur + j) + lad.lens[cur + j]].clone() for j in range(g)]

    def target_verify_batch(self, draft_tokens, state: E.SpecState, B: int):
        """var.py:1026-1070 -> (list of per-stage CFG logits (B, pn^2, V), gamma).  The verified stages are the ones the last
        draft_generate_batch produced (their next-scale inputs were built while drafting)."""
        if not draft_tokens:
            return [], 0
        assert len(draft_tokens) == state.g, "target_verify_batch verifies the stages of the last draft_generate_batch"
        _mask_free("target_verify_batch", state)
        if state.rows is None:
            E.scalar_arg("target_verify_batch", cfg=state.cfg)
        smp, lad, cur = state.sampler, state.sampler.lad, state.current_stage
        lg = smp.spec_verify_forward(state)
        lens = [lad.lens[cur + j] for j in range(state.g)]
        with torch.cuda.device(lg.device):                                                           # var.py:1062-1067 (csrc/sampler.hip cfg_combine_kernel)
            out = E.cfg_combine(lg, B, lens, lg.shape[-1], state.chunk_ts(cur, state.g), rows=state.rows, s0=cur)      # a state begun with per-image tables: every image's own factor
        return out, state.g

    def _match(self, draft_tokens, target_logits, B: int, rule: E.MatchRule, draft_logits=None):
        if not draft_tokens or not target_logits or len(draft_tokens) != len(target_logits):
            return 0, None
        dev = target_logits[0].device
        lens = [int(t.shape[1]) for t in draft_tokens]
        ids = torch.cat([t.to(dev) for t in draft_tokens], 1).contiguous()
        lg = torch.cat(target_logits, 1)
        lg2 = torch.cat([lg, lg], 0).contiguous()          # t = 0 makes the kernel's CFG the identity on the first B rows
        dl = None
        if rule.rule == "kl":
            if draft_logits is None or len(draft_logits) != len(draft_tokens):
                raise ValueError("the KL rule compares distributions: pass the draft's CFG logits per stage (draft_logits=[(B, pn^2, V), ...])")
            dl = torch.cat([torch.cat([d, d], 0).reshape(-1) for d in draft_logits]).to(dev).contiguous()     # stage j as (2B, l_j, V)
        counts = torch.zeros(40, dtype=torch.int32, device=dev)
        match = torch.zeros(B, ids.shape[1], dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            E.verify_accept(lg2, B, lens, lg.shape[-1], [0.0] * len(lens), ids, 0, ids.shape[1], self.match_threshold, counts, rule=rule, draft_logits=dl,
                            match_out=match)
        return int(counts[16].item()), match

    def basic_token_matching(self, draft_tokens, target_logits, state, B: int) -> int:
        """var.py:1160-1227 on arbitrary (tokens, CFG logits) lists: leading stages whose batch match rate is >= 0.5."""
        return self._match(draft_tokens, target_logits, B, E.MatchRule())[0]

    def advanced_token_matching(self, draft_tokens, target_logits, state, B: int, draft_logits=None) -> int:
        """var.py:1229-1243.  The reference's body is a stub that returns basic_token_matching; with the default `self.match_rule` this does
        the same.  Setting `self.match_rule = MatchRule('topk', top_k=k)` / `MatchRule('kl', kl_thr=x)` switches on the rules its docstring
        lists (top-k membership, KL threshold); `token_level=True` (partial acceptance) acts in the sampling loop, see
        sdvar_amd.engine.Sampler.spec_correct.  The per-token verdicts of the last call are kept in `self.last_match`."""
        n, self.last_match = self._match(draft_tokens, target_logits, B, self.match_rule, draft_logits)
        return n

    def update_state_with_accepted_tokens(self, draft_tokens, accept_length: int, state: E.SpecState, B: int):
        """var.py:1245-1282 (+ the stage advance of var.py:1349-1350 and the KV rollback the reference lacks)."""
        _mask_free("update_state_with_accepted_tokens", state)
        state.sampler.spec_commit(state, max(int(accept_length), 0))

    @torch.no_grad()
    def sdvar_autoregressive_infer_cfg_parallel_v1(self, B: int, label_B: Optional[Union[int, torch.LongTensor]] = None, g_seed: Optional[int] = None,
                                                   cfg: float = 1.5, gamma: int = 2, top_k: int = 0, top_p: float = 0.0, more_smooth: bool = False) -> torch.Tensor:
        """var.py:1284-1383 with the resolved semantics of SURVEY.md App. C.1: ONE call of engine.Sampler.spec_decode, i.e. the loop the
        step-wise helpers above spell out, with the verifier running behind / ahead of the draft where the policy allows it (same tokens,
        same counters: tests/test_gpu_e2e.py).  more_smooth is accepted and, exactly as in the reference, has no effect on this path
        (var.py:1315 stores it, draft_generate_batch var.py:949-1024 never reads it)."""
        t = self.target_model
        _row_lengths(B, cfg=cfg, top_k=top_k, top_p=top_p)
        labels, smp, noise = self._prepare(B, label_B, g_seed, gamma)
        res = smp.spec_decode(labels, cfg, gamma, top_k, top_p, noise, thr=self.match_threshold, run_ahead=True, accept_scope=self.accept_scope,
                              match=self.match_rule)
        self.last_result = res
        return t.vae_proxy[0].fhat_to_img(res.f_hat.clone()).add_(1).mul_(0.5)

    # ---- masked sampling at draft -> verify speed (an extension; the reference has no such call) ----------------------------------------
    @torch.no_grad()
    def sdvar_autoregressive_infer_cfg_parallel_v1_edit(self, image: torch.Tensor, mask: torch.Tensor, label_B: Optional[Union[int, torch.LongTensor]],
                                                        g_seed: Optional[int] = None, cfg=1.5, gamma: int = 2, top_k=0, top_p=0.0, composite: bool = True,
                                                        more_smooth: bool = False) -> torch.Tensor:
        """VAR.autoregressive_infer_cfg_edit through the speculative loop: regenerate the masked region of `image` under `label_B` and keep the rest, (B, 3, H, H)
        in [0, 1].  The arguments are those of VAR.autoregressive_infer_cfg_edit (same checks, same messages) plus `gamma`; cfg / top_k / top_p / g_seed may be
        per-image sequences; more_smooth=True raises SdvarError.  The image is encoded by the target's VQVAE, engine.mask_tokens turns the pixel mask into the
        (B, L) token table, and Sampler.spec_decode(force_ids=, gen=) runs the draft -> verify loop in which both models see the image's own ids at the kept
        tokens and only the sampled tokens are verified: the acceptance rate of a stage is matched / sampled tokens of the batch, and a stage without a sampled
        token is accepted.  With composite=True the kept pixels are the bits of image.add(1).mul(0.5).  last_result carries `gen`."""
        who = "sdvar_autoregressive_infer_cfg_parallel_v1_edit"
        t = self.target_model
        vae = t.vae_proxy[0]
        B, H = _edit_args(who, t, image, mask, more_smooth)
        _row_lengths(B, cfg=cfg, top_k=top_k, top_p=top_p)
        image, mask_px = _edit_operands(image, mask, B, H)
        try:
            labels, smp, noise = self._prepare(B, label_B, g_seed, gamma)
        except torch.cuda.OutOfMemoryError as e:
            t.invalidate_engine(); self.draft_model.invalidate_engine()
            self._sampler = None
            raise E.SdvarError(f"{who}: image: the sampler contexts cannot be built for a batch of {B} images: {e}") from None
        force_ids = torch.cat(vae.img_to_idxBl(image, v_patch_nums=t.patch_nums), dim=1).contiguous()          # (B, L): the image's own ids
        gen = E.mask_tokens(mask_px, t.patch_nums)
        res = smp.spec_decode(labels, cfg, gamma, top_k, top_p, noise, thr=self.match_threshold, run_ahead=True, accept_scope=self.accept_scope,
                              match=self.match_rule, force_ids=force_ids, gen=gen, trusted_ids=True)
        res.gen = gen
        self.last_result = res
        out = vae.fhat_to_img(res.f_hat.clone())
        if composite:
            return E.img_composite(out, image, mask_px, out=out)
        return out.add_(1).mul_(0.5)

    @torch.no_grad()
    def sdvar_autoregressive_infer_cfg_sd_test3(self, B: int, label_B: Optional[Union[int, torch.LongTensor]], g_seed: Optional[int] = None, cfg: float = 1.5,
                                                top_k: int = 0, top_p: float = 0.0, more_smooth: bool = False, entry_num: int = 10, sd_mask: int = 0) -> torch.Tensor:
        """var.py:604-865: the draft samples stages 0 .. entry_num-1, the target continues from the shared f_hat.  One generator, the target
        model's (var.py:641-642); labels as in var.py:647-656.  All six sd_mask values are built (engine.Sampler.handoff;
        1, 2, 4, 5 run the prefill under the explicit block-wise masks of var.py:557-578)."""
        t = self.target_model
        E.scalar_arg("sdvar_autoregressive_infer_cfg_sd_test3", g_seed=g_seed, cfg=cfg, top_k=top_k, top_p=top_p)
        rng = None
        if g_seed is not None:
            t.rng.manual_seed(g_seed); rng = t.rng
        S = len(t.patch_nums)
        labels, smp, noise = self._prepare(B, label_B, g_seed, entry_num + 1 if (sd_mask != 0 and entry_num < S) else 1, rng=rng)
        res = smp.handoff(labels, cfg, top_k, top_p, noise, entry_num, sd_mask, more_smooth=bool(more_smooth))
        self.last_result = res
        return t.vae_proxy[0].fhat_to_img(res.f_hat.clone()).add_(1).mul_(0.5)


def _mask_free(who: str, state: E.SpecState):
    if state.forced is not None:
        raise E.SdvarError(f"{who}: the step-wise helpers take no mask (force_ids / gen): run Sampler.spec_decode or sdvar_autoregressive_infer_cfg_parallel_v1_edit")


def _factory_checks(patch_nums: Sequence[int]):
    if len(patch_nums) > E.MAX_STAGES:
        raise NotImplementedError(f"ladders longer than {E.MAX_STAGES} stages are not supported")


def build_vae_var(device, patch_nums=(1, 2, 3, 4, 5, 6, 8, 10, 13, 16), V=4096, Cvae=32, ch=160, share_quant_resi=4, num_classes=1000, depth=16,
                  shared_aln=False, attn_l2_norm=True, flash_if_available=True, fused_if_available=True, init_adaln=0.5, init_adaln_gamma=1e-5,
                  init_head=0.02, init_std=-1):
    """models/__init__.py:16-46 (same arguments and return value)."""
    _factory_checks(patch_nums)
    vae = VQVAE(vocab_size=V, z_channels=Cvae, ch=ch, test_mode=True, share_quant_resi=share_quant_resi, v_patch_nums=patch_nums).to(device)
    var = VAR(vae_local=vae, num_classes=num_classes, depth=depth, embed_dim=depth * 64, num_heads=depth, drop_rate=0., attn_drop_rate=0.,
              drop_path_rate=0.1 * depth / 24, norm_eps=1e-6, shared_aln=shared_aln, cond_drop_rate=0.1, attn_l2_norm=attn_l2_norm,
              patch_nums=patch_nums, flash_if_available=flash_if_available, fused_if_available=fused_if_available).to(device)
    var.init_weights(init_adaln=init_adaln, init_adaln_gamma=init_adaln_gamma, init_head=init_head, init_std=init_std)
    _init_vae(vae)
    return vae, var


def build_vae_var_speculative_decoding(device, patch_nums=(1, 2, 3, 4, 5, 6, 8, 10, 13, 16), V=4096, Cvae=32, ch=160, share_quant_resi=4,
                                       num_classes=1000, depth_draft=16, depth_target=30, shared_aln=False, attn_l2_norm=True,
                                       flash_if_available=True, fused_if_available=True, init_adaln=0.5, init_adaln_gamma=1e-5, init_head=0.02,
                                       init_std=-1, similarity_thresh=0.8):
    """models/__init__.py:51-97 (same arguments; returns (vae, draft, target, sd_var); one VQVAE shared by both models)."""
    _factory_checks(patch_nums)
    vae = VQVAE(vocab_size=V, z_channels=Cvae, ch=ch, test_mode=True, share_quant_resi=share_quant_resi, v_patch_nums=patch_nums).to(device)
    models = []
    for depth in (depth_draft, depth_target):
        m = VAR(vae_local=vae, num_classes=num_classes, depth=depth, embed_dim=depth * 64, num_heads=depth, drop_path_rate=0.1 * depth / 24,
                shared_aln=shared_aln, attn_l2_norm=attn_l2_norm, patch_nums=patch_nums, flash_if_available=flash_if_available,
                fused_if_available=fused_if_available).to(device)
        m.init_weights(init_adaln=init_adaln, init_adaln_gamma=init_adaln_gamma, init_head=init_head, init_std=init_std)
        models.append(m)
    _init_vae(vae)
    return vae, models[0], models[1], SDVAR(models[0], models[1], similarity_thresh)


def _init_vae(vae: VQVAE, seed: int = 1234):
    """The reference leaves the VQVAE uninitialised when no checkpoint is loaded; give it the seeded
    'perf' init so random-weight runs are finite and reproducible."""
    from .weights import vae_state_dict
    dev = next(vae.parameters()).device
    sd = vae_state_dict(vae.quantize.v_patch_nums, "perf", seed, V=vae.vocab_size, Cvae=vae.Cvae, ch=vae.decoder.conv_out.in_channels,
                        with_encoder=hasattr(vae, "encoder"))
    vae.load_state_dict({k: v.to(dev) for k, v in sd.items()})
