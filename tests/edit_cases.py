"""Shared inputs of the masked-sampling tests (tests/test_edit_host.py, tests/test_gpu_edit_kernels.py, tests/test_gpu_edit.py).  A plain helper module.

  * `mask_tokens_np`: the numpy restatement of the pixel mask -> token table rule of sdvar_mask_tokens (include/sdvar_hip.h): token (i, j) of a stage with
    side pn owns pixel rows [floor(i H / pn), ceil((i + 1) H / pn)) and the same span of columns, and is sampled iff 2 * (set pixels) >= (pixels).
  * `masks(H)`: the pixel masks, by name, at any image size (the 256^2 coordinates scaled by H / 256).
  * the masked oracle loop: oracle.var_oracle.plain_ar's loop from the oracle's own parts, with ids = where(gen, sampled, force_ids) after sampling and
    the tie margins collected over the sampled tokens only.  The reference has no masked sampler; this restatement is the yardstick.
  * the seeds: picked on the CPU the way tests/row_params_cases.py picks its own - the first seed from its start value whose masked oracle run keeps
    every sampled token at least MIN_MARGIN away from a tie, so the GPU ids must equal the oracle's with no token excused.  `pick_seeds()` recomputes them;
    test_edit_host.py checks the committed ones.
The d4 `stress` model on LADDER_256; one image of the oracle costs about 2.5 s of CPU, every run is cached with conftest.oracle_memo."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Sequence

import numpy as np
import torch

from conftest import oracle_memo, state_dicts
from oracle import var_oracle as orc
from sdvar_amd.ladder import LADDER_256, as_ladder
from sdvar_amd.noise import exponential_noise

MIN_MARGIN = 1e-3          # tests/golden/make_golden.py
DEPTH = 4
LAD = as_ladder(LADDER_256)
V = 4096


# ------------------------------------------------------------------------------------------------ the mask rule
def windows(H: int, pn: int):
    """[(lo, hi)] of the pn tokens along one axis: [floor(i H / pn), ceil((i + 1) H / pn))."""
    return [((i * H) // pn, -((-(i + 1) * H) // pn)) for i in range(pn)]


def mask_tokens_np(mask_px: np.ndarray, patch_nums: Sequence[int]) -> np.ndarray:
    """mask_px (B, H, H) or (H, H), non-zero = regenerate -> gen (B, L) uint8.  Integer arithmetic on a summed-area table."""
    m = np.asarray(mask_px)
    m = (m[None] if m.ndim == 2 else m) != 0
    B, H, W = m.shape
    assert H == W
    sat = np.zeros((B, H + 1, H + 1), np.int64)
    sat[:, 1:, 1:] = m.astype(np.int64).cumsum(1).cumsum(2)
    out = []
    for pn in patch_nums:
        win = windows(H, int(pn))
        g = np.zeros((B, pn, pn), np.uint8)
        for i, (y0, y1) in enumerate(win):
            for j, (x0, x1) in enumerate(win):
                n_set = sat[:, y1, x1] - sat[:, y0, x1] - sat[:, y1, x0] + sat[:, y0, x0]
                g[:, i, j] = 2 * n_set >= (y1 - y0) * (x1 - x0)
        out.append(g.reshape(B, pn * pn))
    return np.concatenate(out, 1)


def stage_counts(gen_row: np.ndarray, patch_nums: Sequence[int] = LADDER_256) -> List[int]:
    out, o = [], 0
    for pn in patch_nums:
        out.append(int(gen_row[o:o + pn * pn].sum())); o += pn * pn
    return out


# ------------------------------------------------------------------------------------------------ the masks
HOLE = (70, 56, 100, 110)                  # (y, x, height, width) at 256^2: rows 70 .. 169, columns 56 .. 165
HOLE_COUNTS = [0, 0, 1, 3, 4, 6, 9, 16, 25, 47]                 # sampled tokens per stage of LADDER_256 at 256^2
HOLE_INVERSE_COUNTS = [1, 4, 8, 13, 21, 30, 55, 84, 144, 214]


def masks(H: int = 256) -> Dict[str, np.ndarray]:
    """name -> (H, H) uint8, 1 = regenerate.  Coordinates are those of the 256^2 masks times H / 256 (H a multiple of 256)."""
    assert H % 256 == 0
    k = H // 256
    z = lambda: np.zeros((H, H), np.uint8)
    y, x, h, w = (v * k for v in HOLE)
    hole = z(); hole[y:y + h, x:x + w] = 1
    strip = z(); strip[:, 131 * k:131 * k + 9 * k] = 1                    # thin vertical strip: narrower than every coarse token
    box = z(); box[64 * k:192 * k, 64 * k:192 * k] = 1                   # 25 % of the image, aligned to the finest tokens
    pixel = z(); pixel[H // 3, H // 5] = 1
    half = z(); half[:, :H // 2 + 8 * k] = 1                             # a half-plane whose edge cuts the 16-wide tokens of the last stage in two: exact ties
    speckle = (np.random.Generator(np.random.Philox(key=[H, 77])).integers(0, 256, size=(H, H)) < 128).astype(np.uint8) * 255      # non-zero, not 1
    return {"hole": hole, "hole_inverse": (1 - hole).astype(np.uint8), "strip": strip, "box": box, "empty": z(), "full": z() + 1, "pixel": pixel,
            "half_plane": half, "speckle": speckle}


def random_ids(B: int, seed: int = 5) -> torch.Tensor:
    """(B, L) int64 in [0, V): the forced ids of the engine tests (any ids do: the sampler conditions on them through the quantiser)."""
    return torch.from_numpy(np.random.Generator(np.random.Philox(key=[seed, 99])).integers(0, V, size=(B, LAD.L)))


# ------------------------------------------------------------------------------------------------ the masked oracle loop
@dataclass
class MaskedTrace:
    ids: torch.Tensor              # (B, L)
    f_hat: torch.Tensor            # (B, Cvae, HW, HW)
    margins: List[float]           # per stage: min relative top-2 gap of p / q over the SAMPLED tokens (inf where a stage samples none)


def noise_of(seed: int, index: int = 0):
    """The oracle's noise source of one image: the Philox stream with key `seed` at image counter `index` (the call is B = 1)."""
    return orc.array_noise(lambda d, B_, l, V_: exponential_noise(seed, d, B_, l, V_, index))


def masked_plain_ar(model: orc.OracleVAR, quant: orc.OracleQuant, label_B: torch.Tensor, cfg: float, top_k: int, top_p: float, noise, gen: torch.Tensor,
                    force_ids: torch.Tensor) -> MaskedTrace:
    """orc.plain_ar's loop (var.py:127-215 up to the decode) with forced tokens: after sampling, ids = where(gen, sampled, force_ids)."""
    B, S = label_B.shape[0], model.S
    cond, lvl_pos, x = model.prologue(label_B)
    f_hat = torch.zeros(B, model.Cvae, model.patch_nums[-1], model.patch_nums[-1])
    model.kv_reset()
    all_ids, margins = [], []
    for si, pn in enumerate(model.patch_nums):
        l, beg = pn * pn, LAD.begin(si)
        logits = model.forward(x, cond, si, 1)
        cl = orc.cfg_combine(logits, B, cfg * (si / (S - 1)))
        q = noise(si, B, l, cl.shape[-1])
        sampled, masked = orc.sample_topk_topp(cl, top_k, top_p, q)
        g = gen[:, beg:beg + l] != 0
        ids = torch.where(g, sampled, force_ids[:, beg:beg + l])
        ratio = masked.softmax(dim=-1).view(-1, cl.shape[-1]) / q.view(-1, cl.shape[-1])           # sample_topk_topp's own tie detector, kept per token
        top2 = ratio.topk(2, dim=-1)[0]
        gap = ((top2[:, 0] - top2[:, 1]) / top2[:, 0]).view(B, l)
        margins.append(float(gap[g].min()) if bool(g.any()) else float("inf"))
        all_ids.append(ids)
        f_hat, nxt = quant.next_input(si, f_hat, quant.embed_ids(ids, pn))
        if si != S - 1:
            x = model.embed_next(nxt, lvl_pos, si + 1)
    model.kv_reset()
    return MaskedTrace(torch.cat(all_ids, 1), f_hat, margins)


def accumulate_ids(quant: orc.OracleQuant, ids: torch.Tensor) -> torch.Tensor:
    """f_hat of given ids (B, L): the oracle's quantiser accumulation alone (quant.py:187-196)."""
    f_hat = torch.zeros(ids.shape[0], quant.codebook.shape[1], LADDER_256[-1], LADDER_256[-1])
    for si, pn in enumerate(LADDER_256):
        f_hat, _ = quant.next_input(si, f_hat, quant.embed_ids(ids[:, LAD.begin(si):LAD.cum[si]], pn))
    return f_hat


# ------------------------------------------------------------------------------------------------ the cases and their seeds
@dataclass(frozen=True)
class EditImage:
    mask: str                      # name in masks(256)
    label: int
    cfg: float
    top_k: int
    top_p: float
    seed: int
    index: int                     # Philox image counter


MASKS3 = ("hole", "hole_inverse", "strip")
LABELS3 = (3, 977, 500)
# one scalar call, B = 3: one seed, image b draws at image counter b
SCALAR_START = 400
SCALAR_SEED = 405
SCALAR = tuple(EditImage(m, lab, 1.5, 900, 0.96, SCALAR_SEED, b) for b, (m, lab) in enumerate(zip(MASKS3, LABELS3)))
# the per-image call: three (cfg, top_k, top_p, seed) sets (image 1 with top-k and top-p off), image counter 0 each
ROWS_START = (500, 600, 700)
ROWS_SEEDS = (500, 601, 700)
ROWS = tuple(EditImage(m, lab, c, k, p, s, 0) for m, lab, (c, k, p), s in zip(MASKS3, LABELS3, ((1.5, 900, 0.96), (3.0, 0, 0.0), (0.75, 40, 0.5)), ROWS_SEEDS))


def gen_table(names: Sequence[str] = MASKS3, H: int = 256) -> torch.Tensor:
    ms = masks(H)
    return torch.from_numpy(mask_tokens_np(np.stack([ms[n] for n in names]), LADDER_256))


def _oracles():
    sd4, sdv = state_dicts(DEPTH, LADDER_256)
    return oracle_memo(("edit_oracles",), lambda: (orc.OracleVAR(sd4, DEPTH, LADDER_256), orc.OracleQuant(sdv, LADDER_256)))


def oracle_run(img: EditImage, b: int, seed=None) -> MaskedTrace:
    """Image `b` of a three-image case alone (B = 1): its mask's table, row b of random_ids(3), its own noise stream.  Cached."""
    seed = img.seed if seed is None else seed

    def run():
        model, quant = _oracles()
        gen = gen_table((img.mask,))
        return masked_plain_ar(model, quant, torch.tensor([img.label]), img.cfg, img.top_k, img.top_p, noise_of(seed, img.index), gen, random_ids(3)[b:b + 1])
    return oracle_memo(("edit_run", img.mask, img.label, img.cfg, img.top_k, img.top_p, seed, img.index, b), run)


def build_var(dev=None, with_encoder: bool = True):
    """The public pair of the tests: the d4 `stress` VAR over a ch = 32 VQVAE (with its encoder unless asked otherwise); on `dev`, or on the CPU (argument checks)."""
    from sdvar_amd.var import VAR
    from sdvar_amd.vqvae import VQVAE
    from sdvar_amd.weights import vae_state_dict
    vae = VQVAE(vocab_size=V, z_channels=32, ch=32, v_patch_nums=LADDER_256, with_encoder=with_encoder)
    vae.load_state_dict(vae_state_dict(LADDER_256, "stress", ch=32, with_encoder=with_encoder))
    var = VAR(vae_local=vae, depth=DEPTH, embed_dim=64 * DEPTH, num_heads=DEPTH, attn_l2_norm=True, patch_nums=LADDER_256)
    var.load_state_dict(state_dicts(DEPTH, LADDER_256)[0])
    if dev is not None:
        vae, var = vae.to(dev), var.to(dev)
    return vae, var


def sample_image(B: int, H: int = 256, seed: int = 11) -> torch.Tensor:
    """(B, 3, H, H) fp32 in [-1, 1]: smooth waves plus a little noise (numpy Philox: portable)."""
    g = np.random.Generator(np.random.Philox(key=[seed, 4242]))
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="ij")
    out = np.empty((B, 3, H, H), np.float32)
    for b in range(B):
        for c in range(3):
            fy, fx, ph = g.uniform(0.01, 0.08), g.uniform(0.01, 0.08), g.uniform(0, 6.28)
            out[b, c] = 0.8 * np.sin(fy * yy + fx * xx + ph) + 0.1 * g.standard_normal(size=(H, H), dtype=np.float32)
    return torch.from_numpy(np.clip(out, -1.0, 1.0).astype(np.float32))




def pick_seeds(tries: int = 40):
    """(scalar seed, rows seeds): the first seeds from their start values whose masked oracle runs keep every sampled token >= MIN_MARGIN from a tie."""
    for seed in range(SCALAR_START, SCALAR_START + tries):
        if all(min(oracle_run(im, b, seed).margins) >= MIN_MARGIN for b, im in enumerate(SCALAR)):
            scalar = seed
            break
    else:
        raise RuntimeError(f"no scalar seed with margin >= {MIN_MARGIN}")
    rows = []
    for b, (im, start) in enumerate(zip(ROWS, ROWS_START)):
        for seed in range(start, start + tries):
            if min(oracle_run(im, b, seed).margins) >= MIN_MARGIN:
                rows.append(seed)
                break
        else:
            raise RuntimeError(f"no seed with margin >= {MIN_MARGIN} for {im}")
    return scalar, tuple(rows)
