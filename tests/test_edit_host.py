"""Host side of masked sampling (no GPU): the numpy restatement of the mask rule against hand-counted cases, the committed seeds of tests/edit_cases.py
against their rule, the argument errors of the new wrappers that need no GPU, and the ABI with the new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import edit_cases as EC
from conftest import ROOT
from sdvar_amd import engine as E
from sdvar_amd.ladder import LADDER_256

EDIT_SYMBOLS = ("sdvar_cfg_sample_forced", "sdvar_cfg_sample_rows_forced", "sdvar_mask_tokens", "sdvar_img_composite")


# ------------------------------------------------------------------------------------------------ the mask rule
def _counts(name, H=256):
    return EC.stage_counts(EC.mask_tokens_np(EC.masks(H)[name], LADDER_256)[0])


def test_hole_and_its_inverse_give_the_quoted_counts():
    assert _counts("hole") == EC.HOLE_COUNTS == [0, 0, 1, 3, 4, 6, 9, 16, 25, 47]                    # a small hole keeps the coarse tokens of the image
    assert _counts("hole_inverse") == EC.HOLE_INVERSE_COUNTS == [1, 4, 8, 13, 21, 30, 55, 84, 144, 214]
    full = [pn * pn for pn in LADDER_256]
    both = [a + b - f for a, b, f in zip(EC.HOLE_COUNTS, EC.HOLE_INVERSE_COUNTS, full)]
    assert both == [0] * 9 + [5]                      # five tokens of the last stage are exact ties: sampled under the mask AND under its inverse
    assert _counts("hole", 512) == EC.HOLE_COUNTS     # the same mask at twice the size: every window doubles, every ratio stays


def test_empty_full_and_single_pixel():
    assert _counts("empty") == [0] * 10
    assert _counts("full") == [pn * pn for pn in LADDER_256]
    assert _counts("pixel") == [0] * 10               # one pixel is never half of a 16 x 16 window
    m = np.zeros((16, 16), np.uint8); m[5, 9] = 1     # ... but it is all of a 1 x 1 window: a stage as fine as the pixels samples exactly that token
    g = EC.mask_tokens_np(m, (1, 2, 16))[0]
    assert g[:5].tolist() == [0] * 5 and g[5:].reshape(16, 16).nonzero()[0].tolist() == [5] and g[5:].reshape(16, 16).nonzero()[1].tolist() == [9]
    m = np.zeros((16, 16), np.uint8); m[5, 9] = 200   # any non-zero value is "set"
    assert np.array_equal(EC.mask_tokens_np(m, (1, 2, 16))[0], g)


def test_overlapping_windows_and_ties_by_hand():
    """H = 4, pn = 3: the windows along one axis are [0, 2), [1, 3), [2, 4) - they overlap.  Column 1 set: the 2 x 2 windows of token columns 0 and 1 hold
    2 set pixels of 4, a tie, which is sampled; token column 2 holds none."""
    assert EC.windows(4, 3) == [(0, 2), (1, 3), (2, 4)]
    m = np.zeros((4, 4), np.uint8); m[:, 1] = 1
    assert EC.mask_tokens_np(m, (3,))[0].reshape(3, 3).tolist() == [[1, 1, 0]] * 3
    m[0, 1] = 0                                        # one pixel fewer: the two top windows fall below half
    assert EC.mask_tokens_np(m, (3,))[0].reshape(3, 3).tolist() == [[0, 0, 0], [1, 1, 0], [1, 1, 0]]
    assert EC.windows(256, 13)[6] == (118, 138) and EC.windows(256, 5)[2] == (102, 154)


def test_half_plane_ties():
    """Columns [0, 136) set at 256^2.  Counted by hand per stage (token columns sampled x pn): the 16-wide tokens of the last stage at columns [128, 144)
    hold 8 set columns of 16 - an exact tie, sampled; pn = 13's window [118, 138) holds 18 of 20, pn = 5's [102, 154) 34 of 52, pn = 3's [85, 171) 51 of 86;
    pn = 8's [128, 160) holds 8 of 32 and is kept."""
    assert _counts("half_plane") == [1, 2 * 1, 3 * 2, 4 * 2, 5 * 3, 6 * 3, 8 * 4, 10 * 5, 13 * 7, 16 * 9]
    g = EC.mask_tokens_np(EC.masks()["half_plane"], LADDER_256)[0][-256:].reshape(16, 16)
    assert g[:, 8].all() and not g[:, 9].any()
    shifted = EC.masks()["half_plane"].copy(); shifted[:, 135] = 0                     # one column short of the tie
    assert not EC.mask_tokens_np(shifted, LADDER_256)[0][-256:].reshape(16, 16)[:, 8].any()


def test_batched_masks_are_the_single_masks():
    ms = EC.masks()
    names = ("hole", "strip", "speckle")
    g3 = EC.mask_tokens_np(np.stack([ms[n] for n in names]), LADDER_256)
    assert g3.shape == (3, EC.LAD.L) and g3.dtype == np.uint8
    for b, n in enumerate(names):
        assert np.array_equal(g3[b], EC.mask_tokens_np(ms[n], LADDER_256)[0])


# ------------------------------------------------------------------------------------------------ the seeds
def test_committed_seeds_are_the_first_with_every_sampled_token_clear_of_a_tie():
    """No token may be excused: every sampled token of every oracle run the GPU tests compare against is at least MIN_MARGIN from a tie."""
    scalar, rows = EC.pick_seeds()
    assert scalar == EC.SCALAR_SEED and rows == EC.ROWS_SEEDS
    for case in (EC.SCALAR, EC.ROWS):
        for b, im in enumerate(case):
            tr = EC.oracle_run(im, b)
            assert min(tr.margins) >= EC.MIN_MARGIN, (im, tr.margins)
            gen = EC.gen_table((im.mask,))[0]
            assert torch.equal(tr.ids[0][gen == 0], EC.random_ids(3)[b][gen == 0])          # the loop forces what it is told to
            assert int(gen.sum()) > 0
    assert EC.stage_counts(EC.gen_table()[0].numpy()) == EC.HOLE_COUNTS


# ------------------------------------------------------------------------------------------------ argument errors that need no GPU
def test_wrappers_refuse_bad_operands_by_name():
    z8, zf = torch.zeros(1, 16, 16, dtype=torch.uint8), torch.zeros(1, 3, 16, 16)
    with pytest.raises(E.SdvarError, match="mask_px"):
        E.mask_tokens(z8, (1, 2, 4))                                      # a CPU tensor
    with pytest.raises(E.SdvarError, match="mask_px"):
        E.mask_tokens(torch.zeros(1, 16, 8, dtype=torch.uint8), (1, 2))   # not square
    with pytest.raises(E.SdvarError, match="patch_nums"):
        E.mask_tokens(z8, (1, 2, 32))                                     # a stage finer than the pixels
    with pytest.raises(E.SdvarError, match="patch_nums"):
        E.mask_tokens(z8, ())
    with pytest.raises(E.SdvarError, match="gen_img"):
        E.img_composite(zf, zf, z8)
    with pytest.raises(E.SdvarError, match="gen_img"):
        E.img_composite(torch.zeros(3, 16, 16), zf, z8)
    lg, ids = torch.zeros(2, 4, 8), torch.zeros(1, 4, dtype=torch.int64)
    gen = torch.ones(1, 4, dtype=torch.uint8)
    with pytest.raises(E.SdvarError, match="logits"):
        E.cfg_sample_forced(lg, 1, 4, 8, 0.5, 0, 0.0, None, 0, 0, 0, ids, 0, 4, gen, ids, 0, 4)
    with pytest.raises(E.SdvarError, match="V = 6"):
        E.cfg_sample_forced(lg, 1, 4, 6, 0.5, 0, 0.0, None, 0, 0, 0, ids, 0, 4, gen, ids, 0, 4)
    with pytest.raises(E.SdvarError, match="stride"):
        E.cfg_sample_forced(lg, 1, 4, 8, 0.5, 0, 0.0, None, 0, 0, 0, ids, 2, 4, gen, ids, 0, 4)          # 4 tokens at offset 2 in rows of 4
    with pytest.raises(E.SdvarError, match="logits"):
        E.cfg_sample_rows_forced(lg, 1, 4, 8, None, 0, None, 0, ids, 0, 4, gen, ids, 0, 4)


def test_library_refuses_null_operands_before_any_gpu_call():
    lib = E.load_library()
    one = (C.c_int32 * 1)(1)
    assert lib.sdvar_mask_tokens(None, 1, 16, 1, one, None, None) == 1 and b"mask_tokens" in lib.sdvar_last_error()
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    assert lib.sdvar_mask_tokens(p, 1, 16, 0, one, p, None) == 1 and b"stages" in lib.sdvar_last_error()
    bad = (C.c_int32 * 2)(1, 17)
    assert lib.sdvar_mask_tokens(p, 1, 16, 2, bad, p, None) == 1 and b"patch_nums[1]" in lib.sdvar_last_error()
    assert lib.sdvar_img_composite(None, None, None, 1, 3, 16, None, None) == 1 and b"img_composite" in lib.sdvar_last_error()
    assert lib.sdvar_img_composite(p, p, p, 0, 3, 16, p, None) == 1 and b"img_composite" in lib.sdvar_last_error()
    assert lib.sdvar_cfg_sample_forced(p, 1, 4, 8, 0.5, 0, 0.0, None, 0, 0, 0, p, 4, None, None, None, 4, None) == 1 and b"cfg_sample_forced" in lib.sdvar_last_error()
    assert lib.sdvar_cfg_sample_rows_forced(p, 1, 4, 8, p, p, p, 1, None, 0, p, 4, None, None, p, 4, None) == 1 and b"cfg_sample_rows_forced" in lib.sdvar_last_error()


def test_public_method_refuses_by_argument_name_without_a_gpu():
    """Every check of VAR.autoregressive_infer_cfg_edit comes before the first launch: a CPU model reaches them all."""
    vae, var = EC.build_var(None)
    img, mask = torch.zeros(2, 3, 256, 256), torch.zeros(2, 256, 256, dtype=torch.bool)
    with pytest.raises(E.SdvarError, match="more_smooth"):
        var.autoregressive_infer_cfg_edit(img, mask, 3, more_smooth=True)
    for bad in (torch.zeros(2, 1, 256, 256), torch.zeros(3, 256, 256), torch.zeros(2, 3, 256, 256, dtype=torch.float64), "no tensor"):
        with pytest.raises(E.SdvarError, match="image must be"):
            var.autoregressive_infer_cfg_edit(bad, mask, 3)
    with pytest.raises(E.SdvarError, match="image is 512 x 512"):
        var.autoregressive_infer_cfg_edit(torch.zeros(1, 3, 512, 512), torch.zeros(512, 512, dtype=torch.bool), 3)
    with pytest.raises(E.SdvarError, match="image: a batch of 70000"):
        var.autoregressive_infer_cfg_edit(torch.zeros(1, 3, 256, 256).expand(70000, 3, 256, 256), torch.zeros(256, 256, dtype=torch.bool), 3)
    with pytest.raises(E.SdvarError, match="mask must be"):
        var.autoregressive_infer_cfg_edit(img, torch.zeros(2, 256, 256), 3)                       # a float mask
    for bad in (torch.zeros(3, 256, 256, dtype=torch.bool), torch.zeros(2, 128, 128, dtype=torch.uint8), torch.zeros(2, 3, 256, 256, dtype=torch.bool)):
        with pytest.raises(E.SdvarError, match="mask has shape"):
            var.autoregressive_infer_cfg_edit(img, bad, 3)
    with pytest.raises(E.SdvarError, match="image is on cpu"):
        var.autoregressive_infer_cfg_edit(img, mask, 3)
    vae2, var2 = EC.build_var(None, with_encoder=False)
    with pytest.raises(E.SdvarError, match="with_encoder=False"):
        var2.autoregressive_infer_cfg_edit(img, mask, 3)


# ------------------------------------------------------------------------------------------------ the ABI
def test_abi_is_additive_and_bound():
    lib = E.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdvar_hip.h")).read(), flags=re.S)
    for s in EDIT_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), f"{s} is not declared in include/sdvar_hip.h"
        assert hasattr(lib, s) and s in E._SIGNATURES
    n_args = lambda s: len(E._SIGNATURES[s][1])
    assert n_args("sdvar_cfg_sample_forced") == n_args("sdvar_cfg_sample") + 3               # the twins' lists plus gen, force_ids, force_stride
    assert n_args("sdvar_cfg_sample_rows_forced") == n_args("sdvar_cfg_sample_rows") + 3
    assert lib.sdvar_abi_version() == 5 == E.ABI_VERSION
    assert all(callable(getattr(E, f)) for f in ("cfg_sample_forced", "cfg_sample_rows_forced", "mask_tokens", "img_composite"))
    import inspect
    sig = inspect.signature(E.Sampler.plain_ar).parameters
    assert sig["force_ids"].default is None and sig["gen"].default is None and sig["trusted_ids"].default is False
    from sdvar_amd.var import SDVAR, VAR
    assert "mask" in inspect.signature(VAR.autoregressive_infer_cfg_edit).parameters
    assert "mask" not in inspect.signature(SDVAR.sdvar_autoregressive_infer_cfg_parallel_v1).parameters
