"""Host side of masked sampling in the speculative sampler (no GPU): the masked oracle loop of tests/spec_edit_cases.py against orc.spec_decode, its committed
seeds against their rule (no sampled token near a sampling tie, no top-1 verdict near a flip), the zero-total rule of dist.leading_accepted, the new symbols, and
the argument refusals of the public call, which all come before the first launch."""
import inspect
import os
import re

import pytest
import torch

import edit_cases as EC
import spec_edit_cases as SC
from conftest import ROOT
from oracle import var_oracle as orc
from sdvar_amd import dist as D
from sdvar_amd import engine as E

torch.set_grad_enabled(False)
NEW_SYMBOLS = ("sdvar_verify_accept_forced", "sdvar_verify_accept_rows_forced")


def test_all_ones_masked_oracle_is_the_oracles_spec_decode():
    d, t, q = SC.oracles()
    lab, ones = torch.tensor(EC.LABELS3), torch.ones(SC.B, SC.LAD.L, dtype=torch.uint8)
    seed = SC.CASES["g2_t5"].seed
    a = orc.spec_decode(d, t, q, lab, *SC.PLAIN[:1], 2, *SC.PLAIN[1:], SC.noise_fn(seed), thr=0.5)
    b = SC.masked_spec_decode(d, t, q, lab, SC.PLAIN[0], 2, SC.PLAIN[1], SC.PLAIN[2], SC.noise_fn(seed), ones, EC.random_ids(SC.B), 0.5)
    assert torch.equal(torch.cat(a.ids, 1), b.ids) and torch.equal(a.f_hat, b.f_hat)
    assert b.stats.pop("sampled_tokens") == SC.B * SC.LAD.L
    assert a.stats == b.stats and len(a.stats["rounds"]) >= 5


def test_committed_seeds_keep_every_sampled_token_and_every_verdict_clear():
    """No token may be excused: in every oracle run the GPU tests compare against, each sampled token is at least MIN_MARGIN from a sampling tie, and no top-1
    verdict is within the same relative margin of flipping."""
    force = EC.random_ids(SC.B)
    for name, c in SC.CASES.items():
        gen = EC.gen_table(c.masks)
        tr = SC.oracle_run(name)
        print(name, "sampling margin", min(tr.margins), "verdict margin", min(tr.vmargins))
        assert min(tr.margins) >= EC.MIN_MARGIN, (name, tr.margins)
        assert min(tr.vmargins) >= EC.MIN_MARGIN, (name, tr.vmargins)
        assert torch.equal(tr.ids[gen == 0], force[gen == 0])                      # the loop forces what it is told to
        assert tr.stats["sampled_tokens"] == int(gen.sum()) == sum(sum(r["total"][:r["n_accept"]]) for r in tr.stats["rounds"])
        assert all(r["total"][j] <= SC.B * SC.LAD.lens[r["stage"] + j] for r in tr.stats["rounds"] for j in range(r["g"]))


def test_leading_accepted_takes_a_stage_without_sampled_tokens():
    assert D.leading_accepted([0, 0, 3], [0, 0, 4], 0.5) == 3
    assert D.leading_accepted([0, 1, 0], [0, 4, 0], 0.5) == 1                    # stop at the first failure: the empty stage behind it is not reached
    assert D.leading_accepted([2, 0], [4, 0], 0.5) == 2
    assert D.leading_accepted([0], [0], 2.0) == 1
    assert D.leading_accepted([1, 4], [4, 4], 0.5) == 0                          # the unmasked rule is unchanged
    assert D.global_accept([0, 2], [0, 4], 0.5, torch.device("cpu"))[0] == 2     # one process: the local decision


def test_new_symbols_are_additive_and_bound():
    lib = E.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdvar_hip.h")).read(), flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), f"{s} is not declared in include/sdvar_hip.h"
        assert hasattr(lib, s) and s in E._SIGNATURES
    n_args = lambda s: len(E._SIGNATURES[s][1])
    assert n_args("sdvar_verify_accept_forced") == n_args("sdvar_verify_accept_ex") + 2          # the twins' lists plus gen, gen_stride
    assert n_args("sdvar_verify_accept_rows_forced") == n_args("sdvar_verify_accept_rows") + 2
    assert lib.sdvar_abi_version() == 5 == E.ABI_VERSION
    p = inspect.signature(E.verify_accept).parameters
    assert p["gen"].default is None and p["gen_off"].default == 0 and p["gen_stride"].default == 0
    for fn in (E.Sampler.spec_begin, E.Sampler.spec_decode):
        p = inspect.signature(fn).parameters
        assert p["force_ids"].default is None and p["gen"].default is None and p["trusted_ids"].default is False
    from sdvar_amd.var import SDVAR, VAR
    a = inspect.signature(VAR.autoregressive_infer_cfg_edit).parameters
    b = inspect.signature(SDVAR.sdvar_autoregressive_infer_cfg_parallel_v1_edit).parameters
    assert [k for k in b if k != "gamma"] == list(a) and b["gamma"].default == 2 and b["composite"].default is True
    assert "mask" not in inspect.signature(SDVAR.sdvar_autoregressive_infer_cfg_parallel_v1).parameters


def test_library_refuses_null_gen_before_any_gpu_call():
    import ctypes as C
    lib = E.load_library()
    buf = C.create_string_buffer(256)
    p = C.cast(buf, C.c_void_p)
    one, t = (C.c_int32 * 1)(4), (C.c_double * 1)(0.0)
    assert lib.sdvar_verify_accept_forced(p, 1, 4, 8, 1, one, t, p, 4, 0.5, 0, 0, 0.0, None, p, None, None, None, None, 4, None) == 1
    assert b"verify_accept_forced" in lib.sdvar_last_error()
    assert lib.sdvar_verify_accept_rows_forced(p, 1, 4, 8, 1, one, p, 1, p, 4, 0.5, 0, 0, 0.0, None, p, None, None, None, None, 4, None) == 1
    assert b"verify_accept_rows_forced" in lib.sdvar_last_error()
    assert lib.sdvar_verify_accept_forced(p, 1, 4, 8, 1, one, t, p, 4, 0.5, 0, 0, 0.0, None, p, None, None, None, p, 3, None) == 1          # gen_stride below lsum
    assert b"gen_stride" in lib.sdvar_last_error()


def test_public_spec_edit_refuses_by_argument_name_without_a_gpu():
    """Every check of SDVAR.sdvar_autoregressive_infer_cfg_parallel_v1_edit comes before the first launch, and carries the texts of VAR.autoregressive_infer_cfg_edit."""
    from sdvar_amd.var import SDVAR
    vae, var = EC.build_var(None)
    sd = SDVAR(var, var)
    call = sd.sdvar_autoregressive_infer_cfg_parallel_v1_edit
    img, mask = torch.zeros(2, 3, 256, 256), torch.zeros(2, 256, 256, dtype=torch.bool)
    with pytest.raises(E.SdvarError, match="sdvar_autoregressive_infer_cfg_parallel_v1_edit: more_smooth"):
        call(img, mask, 3, more_smooth=True)
    for bad in (torch.zeros(2, 1, 256, 256), torch.zeros(3, 256, 256), torch.zeros(2, 3, 256, 256, dtype=torch.float64), "no tensor"):
        with pytest.raises(E.SdvarError, match="image must be"):
            call(bad, mask, 3)
    with pytest.raises(E.SdvarError, match="image is 512 x 512"):
        call(torch.zeros(1, 3, 512, 512), torch.zeros(512, 512, dtype=torch.bool), 3)
    with pytest.raises(E.SdvarError, match="image: a batch of 70000"):
        call(torch.zeros(1, 3, 256, 256).expand(70000, 3, 256, 256), torch.zeros(256, 256, dtype=torch.bool), 3)
    with pytest.raises(E.SdvarError, match="mask must be"):
        call(img, torch.zeros(2, 256, 256), 3)
    for bad in (torch.zeros(3, 256, 256, dtype=torch.bool), torch.zeros(2, 128, 128, dtype=torch.uint8), torch.zeros(2, 3, 256, 256, dtype=torch.bool)):
        with pytest.raises(E.SdvarError, match="mask has shape"):
            call(img, bad, 3)
    with pytest.raises(E.SdvarError, match="image is on cpu"):
        call(img, mask, 3)
    vae2, var2 = EC.build_var(None, with_encoder=False)
    with pytest.raises(E.SdvarError, match="with_encoder=False"):
        SDVAR(var2, var2).sdvar_autoregressive_infer_cfg_parallel_v1_edit(img, mask, 3)
    # the one message of the unmasked contract is unchanged
    with pytest.raises(E.SdvarError, match="^autoregressive_infer_cfg_edit: more_smooth=True is not supported with a mask"):
        var.autoregressive_infer_cfg_edit(img, mask, 3, more_smooth=True)
