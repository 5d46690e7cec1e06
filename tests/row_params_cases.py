"""Parameter sets of the per-image sampling tests (tests/test_row_params_host.py, tests/test_gpu_row_params.py).  A plain helper module.

Three images of one batch, each with its own (label, cfg, top_k, top_p, seed); image 1 has top-k and top-p off.  The d4 `stress` model on LADDER_256.
The seeds were picked on the CPU the way tests/golden/make_golden.py's pick_seed does: the first seed from `SEED_START[i]` on whose oracle run of
that image alone (B = 1, Philox key = seed, image counter 0) keeps every sampled token at least MIN_MARGIN away from a tie - so the GPU ids of every
image must equal the oracle's, no token excused.  `pick_seeds()` recomputes them; test_row_params_host.py checks the committed ones."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from oracle import var_oracle as orc
from sdvar_amd.noise import exponential_noise

MIN_MARGIN = 1e-3          # tests/golden/make_golden.py
DEPTH = 4


@dataclass(frozen=True)
class ImageSet:
    label: int
    cfg: float
    top_k: int
    top_p: float
    seed: int


SEED_START = (100, 200, 300)
SETS = (ImageSet(3, 1.5, 900, 0.96, 100), ImageSet(977, 3.0, 0, 0.0, 200), ImageSet(500, 0.75, 40, 0.5, 302))


def noise_of(seed: int, index: int = 0):
    """The oracle's noise source of one image: the Philox stream with key `seed` at image counter `index` (the call is B = 1)."""
    return orc.array_noise(lambda d, B_, l, V_: exponential_noise(seed, d, B_, l, V_, index))


def oracle_run(model, quant, s: ImageSet, seed=None, keep: bool = False, more_smooth: bool = False):
    return orc.plain_ar(model, quant, torch.tensor([s.label]), s.cfg, s.top_k, s.top_p, noise_of(s.seed if seed is None else seed), keep=keep,
                        more_smooth=more_smooth)


def pick_seeds(model, quant, tries: int = 60):
    out = []
    for s, start in zip(SETS, SEED_START):
        for seed in range(start, start + tries):
            if min(oracle_run(model, quant, s, seed).margins) >= MIN_MARGIN:
                out.append(seed)
                break
        else:
            raise RuntimeError(f"no seed with margin >= {MIN_MARGIN} for {s}")
    return out
