"""GPU: masked sampling in the speculative sampler - Sampler.spec_decode(force_ids, gen) and SDVAR.sdvar_autoregressive_infer_cfg_parallel_v1_edit.
The yardstick is the masked oracle loop of tests/spec_edit_cases.py (orc.spec_decode's loop with forced tokens, counts over sampled tokens, zero-total stages
accepted); its seeds were picked on the CPU so that no sampled token is near a sampling tie and no verdict near a flip (tests/test_spec_edit_host.py), so ids
and the rounds' counters are compared with no token excused.  The d4 draft -> d6 target `stress` pair on LADDER_256, B = 3; the public call on a ch = 32 VQVAE
with its encoder."""
import numpy as np
import pytest
import torch

import edit_cases as EC
import sampler_hard_cases as H
import spec_edit_cases as SC
from conftest import state_dicts
from oracle import var_oracle as orc
from sdvar_amd import engine as E
from sdvar_amd.ladder import LADDER_256

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
LAD = EC.LAD
FHAT_TOL = 1e-4          # the project's bar (tests/test_gpu_edit.py)
PLAIN = SC.PLAIN
ROUND_KEYS = ("stage", "g", "matched", "total", "n_accept", "forced")


@pytest.fixture(scope="module")
def models(dev):
    sd4, sdv = state_dicts(SC.DRAFT_DEPTH, LADDER_256)
    sd6, _ = state_dicts(SC.TARGET_DEPTH, LADDER_256)
    ctxs, out = [], dict(sdv=sdv)
    qc = E.QuantCtx(sdv, LADDER_256, 3, dev)
    for mode in (None, "bf16x3"):
        c4, c6 = E.ModelCtx(sd4, SC.DRAFT_DEPTH, LADDER_256, 3, 1, dev, gemm_mode=mode), E.ModelCtx(sd6, SC.TARGET_DEPTH, LADDER_256, 3, 2, dev, gemm_mode=mode)
        ctxs += [c4, c6]
        out["default" if mode is None else mode] = E.Sampler(c6, qc, c4)
    yield out
    for c in ctxs:
        c.close()
    qc.close()


def _lab(dev):
    return torch.tensor(EC.LABELS3, device=dev)


def _snap(res):
    return res.ids.clone(), res.f_hat.clone(), {k: (list(v) if k == "rounds" else v) for k, v in res.stats.items()}


def _strip(st, *more):
    return {k: v for k, v in st.items() if k not in ("discarded_speculative_rounds",) + more}


def _rounds(st):
    return [{k: r[k] for k in ROUND_KEYS} for r in st["rounds"]]


def _noise(kind, seed):
    return E.Noise(kind, list(seed) if isinstance(seed, tuple) else seed)


def _run_case(smp, dev, name, kind="host", run_ahead=True):
    c = SC.CASES[name]
    lab = torch.tensor(EC.LABELS3, device=dev)
    return smp.spec_decode(lab, SC.as_list(c.cfg), c.gamma, SC.as_list(c.top_k), SC.as_list(c.top_p), _noise(kind, c.seed), thr=c.thr, run_ahead=run_ahead,
                           match=c.match(E), force_ids=EC.random_ids(3).to(dev), gen=EC.gen_table(c.masks).to(dev))


def _against_oracle(res, name, what):
    tr = SC.oracle_run(name)
    gen, force = EC.gen_table(SC.CASES[name].masks), EC.random_ids(3)
    ids = res.ids.cpu()
    assert torch.equal(ids, tr.ids), f"{what}: ids differ from the masked oracle loop at {(ids != tr.ids).nonzero()[:5].tolist()}"
    assert torch.equal(ids[gen == 0], force[gen == 0])
    err = float((res.f_hat.cpu() - tr.f_hat).abs().max())
    print(f"{what}: f_hat max|diff| {err:.3g}; rounds {[(r['stage'], r['g'], r['matched'], r['total'], r['n_accept'], r['forced']) for r in res.stats['rounds']]}")
    assert err <= FHAT_TOL, f"{what}: f_hat off by {err}"
    assert _rounds(res.stats) == _rounds(tr.stats), f"{what}: rounds differ\n got  {_rounds(res.stats)}\n want {_rounds(tr.stats)}"
    assert _strip(res.stats, "rounds") == _strip(tr.stats, "rounds")


# ------------------------------------------------------------------------------------------------ gen all ones / all zeros
@pytest.mark.parametrize("run_ahead", [True, False])
@pytest.mark.parametrize("gamma,thr", [(2, 0.5), (2, 0.0)])
def test_all_ones_gen_is_the_unmasked_spec_decode(dev, models, run_ahead, gamma, thr):
    smp, lab = models["default"], _lab(dev)
    ids0, f0, st0 = _snap(smp.spec_decode(lab, *PLAIN[:1], gamma, *PLAIN[1:], E.Noise("device", 31), thr=thr, run_ahead=run_ahead))
    ones = torch.ones(3, LAD.L, dtype=torch.uint8, device=dev)
    ids1, f1, st1 = _snap(smp.spec_decode(lab, *PLAIN[:1], gamma, *PLAIN[1:], E.Noise("device", 31), thr=thr, run_ahead=run_ahead, force_ids=EC.random_ids(3).to(dev),
                                          gen=ones))
    assert torch.equal(ids0, ids1) and torch.equal(H.bits(f0), H.bits(f1))
    assert st1.pop("sampled_tokens") == 3 * LAD.L and "sampled_tokens" not in st0
    assert st0 == st1
    rows = ([PLAIN[0]] * 3, gamma, [PLAIN[1]] * 3, [PLAIN[2]] * 3, E.Noise("device", [31] * 3, [0, 1, 2]))          # ... through the rows entry points too
    ids2, f2, st2 = _snap(smp.spec_decode(lab, *rows, thr=thr, run_ahead=run_ahead, force_ids=EC.random_ids(3).to(dev), gen=ones))
    st2.pop("sampled_tokens")
    assert torch.equal(ids0, ids2) and torch.equal(H.bits(f0), H.bits(f2)) and st0 == st2


@pytest.mark.parametrize("gamma", [1, 2])
def test_all_zeros_gen_forces_every_token_and_accepts_every_stage(dev, models, gamma):
    smp, force = models["default"], EC.random_ids(3)
    zeros = torch.zeros(3, LAD.L, dtype=torch.uint8, device=dev)
    res = smp.spec_decode(_lab(dev), *PLAIN[:1], gamma, *PLAIN[1:], E.Noise("device", 31), thr=0.5, force_ids=force.to(dev), gen=zeros)
    assert torch.equal(res.ids.cpu(), force)
    st = res.stats
    assert st["target_calls"] == -(-LAD.S // gamma) and st["gamma_final"] == gamma and st["forced_accepts"] == 0 and st["sampled_tokens"] == 0
    assert all(r["n_accept"] == r["g"] and not r["forced"] and not any(r["total"]) and not any(r["matched"]) for r in st["rounds"])
    want = EC.accumulate_ids(orc.OracleQuant(models["sdv"], LADDER_256), force)
    err = float((res.f_hat.cpu() - want).abs().max())
    print("all-forced f_hat max|diff| vs the oracle's accumulation:", err)
    assert err <= FHAT_TOL
    assert smp.t.kv_len() == 0 and smp.d.kv_len() == 0


# ------------------------------------------------------------------------------------------------ against the masked oracle
@pytest.mark.parametrize("mode", ["default", "bf16x3"])
@pytest.mark.parametrize("name", ["g1_t0", "g2_t0", "g1_t5", "g2_t5"])
def test_three_masks_in_one_batch_are_the_masked_oracle(dev, models, mode, name):
    """Hole, its inverse and a thin strip, random forced ids; one seed, image b at noise index b; gamma in {1, 2}, thr in {0.0, 0.5}."""
    _against_oracle(_run_case(models[mode], dev, name), name, f"{mode} {name}")


def test_stages_without_a_sampled_token_are_accepted_and_the_next_round_rolled_back(dev, models):
    """Three small holes: stages 0 and 1 hold no sampled token, the round is accepted in full; the next one fails."""
    res = _run_case(models["default"], dev, "holes")
    _against_oracle(res, "holes", "holes")
    r = res.stats["rounds"]
    assert r[0]["total"] == [0, 0] and r[0]["n_accept"] == 2 and not r[0]["forced"]


def test_top_k_rule_counts_sampled_tokens_only(dev, models):
    """The two random-weight models never agree on a top-1 token; under top-k membership at half the vocabulary about half the sampled tokens match."""
    res = _run_case(models["default"], dev, "topk")
    _against_oracle(res, "topk", "topk")
    assert sum(sum(r["matched"]) for r in res.stats["rounds"]) > 50 and any(not r["forced"] and r["n_accept"] for r in res.stats["rounds"])


def test_token_level_correction_under_a_mask(dev, models):
    res = _run_case(models["default"], dev, "token_level")
    _against_oracle(res, "token_level", "token_level")
    assert res.stats["corrected_tokens"] <= res.stats["sampled_tokens"] and res.stats["corrected_stages"] >= 1


def test_per_image_parameters_under_masks_take_the_rows_entry_points(dev, models):
    c = SC.CASES["rows"]
    assert E.RowParams.build(3, LAD, list(c.cfg), list(c.top_k), list(c.top_p), _noise("host", c.seed)) is not None
    res = _run_case(models["default"], dev, "rows")
    _against_oracle(res, "rows", "rows")
    ids = res.ids.clone()
    assert torch.equal(_run_case(models["default"], dev, "rows", kind="device").ids, ids)


def test_device_noise_reproduces_host_noise_and_a_repeat_is_bit_identical(dev, models):
    smp = models["default"]
    ids, f, st = _snap(_run_case(smp, dev, "g2_t5", kind="host"))
    for _ in range(2):
        ids2, f2, st2 = _snap(_run_case(smp, dev, "g2_t5", kind="device"))
        assert torch.equal(ids2, ids) and torch.equal(H.bits(f2), H.bits(f)) and st2 == st


# ------------------------------------------------------------------------------------------------ run-ahead against lock-step
def test_run_ahead_equals_lock_step_on_all_three_paths(dev, models, monkeypatch):
    """holes: a lock-step first round, accepted in full -> the optimistic path, whose round fails and is rolled back -> gamma 1 -> the run-ahead tail.
    g2_t0: every round accepted, the optimistic path to the end.  g2_t5: the first round fails at once, the run-ahead tail from stage 0."""
    smp = models["default"]
    taken = dict(optimistic=0, run_ahead=0, lock_step=0)
    for key, attr in (("optimistic", "_spec_optimistic"), ("run_ahead", "_spec_run_ahead"), ("lock_step", "spec_accept")):
        fn = getattr(smp, attr)
        monkeypatch.setattr(smp, attr, (lambda f, k: lambda *a, **kw: (taken.__setitem__(k, taken[k] + 1), f(*a, **kw))[1])(fn, key))
    for name in ("holes", "g2_t0", "g2_t5"):
        before = dict(taken)
        ids_a, f_a, st_a = _snap(_run_case(smp, dev, name, kind="device", run_ahead=True))
        used = {k: taken[k] - before[k] for k in taken}
        ids_b, f_b, st_b = _snap(_run_case(smp, dev, name, kind="device", run_ahead=False))
        print(name, "paths taken with run_ahead=True:", used)
        assert torch.equal(ids_a, ids_b) and torch.equal(H.bits(f_a), H.bits(f_b)), name
        assert _strip(st_a) == _strip(st_b), name
        if name == "holes":
            assert used == dict(optimistic=1, run_ahead=1, lock_step=1) and st_a.get("discarded_speculative_rounds", 0) == 1
        assert smp.t.kv_len() == 0 and smp.d.kv_len() == 0
    assert taken["optimistic"] >= 2 and taken["run_ahead"] >= 2


# ------------------------------------------------------------------------------------------------ refusals
def test_masked_spec_decode_refusals_leave_the_sampler_untouched(dev, models):
    smp, lab = models["default"], _lab(dev)
    gen, force = EC.gen_table().to(dev), EC.random_ids(3).to(dev)
    noise = E.Noise("device", 1)
    torch.cuda.synchronize()
    before = smp.ids.clone()
    call = lambda **kw: smp.spec_decode(lab, *PLAIN[:1], 2, *PLAIN[1:], noise, **kw)
    for bad_id in (-1, EC.V):
        bad = force.clone(); bad[1, 77] = bad_id
        with pytest.raises(E.SdvarError, match="spec_decode: force_ids holds ids outside"):
            call(force_ids=bad, gen=gen)
    with pytest.raises(E.SdvarError, match="go together"):
        call(gen=gen)
    with pytest.raises(E.SdvarError, match="go together"):
        smp.spec_begin(lab, PLAIN[0], 2, PLAIN[1], PLAIN[2], noise, force_ids=force)
    with pytest.raises(E.SdvarError, match="gen"):
        call(force_ids=force, gen=gen.to(torch.int64))
    with pytest.raises(E.SdvarError, match="force_ids has shape"):
        call(force_ids=force[:2], gen=gen)
    with pytest.raises(E.SdvarError, match="gen is on cpu"):
        call(force_ids=force, gen=gen.cpu())
    with pytest.raises(E.SdvarError, match="handoff"):
        smp.handoff(lab, *PLAIN, noise, 3, force_ids=force, gen=gen)
    torch.cuda.synchronize()
    assert torch.equal(smp.ids, before) and smp.t.kv_len() == 0 and smp.d.kv_len() == 0          # nothing ran
    from sdvar_amd.var import SDVAR
    st = smp.spec_begin(lab, PLAIN[0], 2, PLAIN[1], PLAIN[2], noise, force_ids=force, gen=gen)          # the step-wise helpers take no mask
    with pytest.raises(E.SdvarError, match="draft_generate_batch: the step-wise helpers take no mask"):
        SDVAR.draft_generate_batch(None, st, 3)
    smp.spec_end(st)


# ------------------------------------------------------------------------------------------------ the public call
@pytest.fixture(scope="module")
def pub(dev):
    from sdvar_amd.var import SDVAR, VAR
    vae, draft = EC.build_var(dev)
    target = VAR(vae_local=vae, depth=SC.TARGET_DEPTH, embed_dim=64 * SC.TARGET_DEPTH, num_heads=SC.TARGET_DEPTH, attn_l2_norm=True, patch_nums=LADDER_256)
    target.load_state_dict(state_dicts(SC.TARGET_DEPTH, LADDER_256)[0])
    target = target.to(dev)
    return dict(vae=vae, sd=SDVAR(draft, target), image=EC.sample_image(3).to(dev))


def _unit(x):
    return x.add(1).mul(0.5)


def test_spec_edit_composite_keeps_the_bits_outside_the_mask(dev, pub):
    vae, sd, image = pub["vae"], pub["sd"], pub["image"][:2].contiguous()
    hole = torch.from_numpy(EC.masks()["hole"]).to(dev)
    out = sd.sdvar_autoregressive_infer_cfg_parallel_v1_edit(image, hole.bool(), 3, g_seed=1, cfg=1.5, gamma=2, top_k=900, top_p=0.96)
    res = sd.last_result
    assert out.shape == (2, 3, 256, 256) and out.dtype == torch.float32
    m = (hole != 0)[None, None].expand_as(out)
    assert torch.equal(H.bits(out[~m].cpu()), H.bits(_unit(image)[~m].cpu())), "a kept pixel is not the input's"
    plain = _unit(vae.fhat_to_img(res.f_hat.clone()))
    assert torch.equal(H.bits(out[m].cpu()), H.bits(plain[m].cpu())), "a regenerated pixel is not the plain decode of f_hat"
    want_gen = torch.from_numpy(EC.mask_tokens_np(EC.masks()["hole"], LADDER_256)).expand(2, -1)
    assert res.gen.dtype == torch.uint8 and torch.equal(res.gen.cpu(), want_gen)
    own = torch.cat(vae.img_to_idxBl(image), 1)
    keep = res.gen == 0
    assert torch.equal(res.ids[keep], own[keep]) and res.ids.shape == (2, LAD.L)
    st = res.stats
    assert st["sampled_tokens"] == int(want_gen.sum()) and st["rounds"][0]["total"] == [0, 0] and st["rounds"][0]["n_accept"] == 2
    out2 = sd.sdvar_autoregressive_infer_cfg_parallel_v1_edit(image, hole, 3, g_seed=1, cfg=1.5, gamma=2, top_k=900, top_p=0.96)          # uint8, and a repeat
    assert torch.equal(H.bits(out2.cpu()), H.bits(out.cpu()))


def test_spec_edit_per_image_arguments_and_refusals(dev, pub):
    sd, image = pub["sd"], pub["image"]
    ms = EC.masks()
    mask = torch.from_numpy(np.stack([ms["box"], ms["strip"], ms["box"]])[:, None]).to(dev)
    out = sd.sdvar_autoregressive_infer_cfg_parallel_v1_edit(image, mask, torch.tensor([977, 3, 500]), g_seed=[5, 6, 7], cfg=[1.5, 3.0, 0.75], gamma=2,
                                                             top_k=[900, 0, 40], top_p=[0.96, 0.0, 0.5])
    assert out.shape == (3, 3, 256, 256) and bool(torch.isfinite(out).all())
    m = (mask != 0).expand_as(out)
    assert torch.equal(H.bits(out[~m].cpu()), H.bits(_unit(image)[~m].cpu()))
    assert torch.equal(sd.last_result.gen.cpu(), torch.from_numpy(EC.mask_tokens_np(mask[:, 0].cpu().numpy(), LADDER_256)))
    raw = sd.sdvar_autoregressive_infer_cfg_parallel_v1_edit(image, mask, torch.tensor([977, 3, 500]), g_seed=[5, 6, 7], cfg=[1.5, 3.0, 0.75], gamma=2,
                                                             top_k=[900, 0, 40], top_p=[0.96, 0.0, 0.5], composite=False)
    assert torch.equal(H.bits(raw[m].cpu()), H.bits(out[m].cpu())) and not torch.equal(raw[~m], out[~m])          # without the composite the kept pixels move
    with pytest.raises(E.SdvarError, match="more_smooth"):
        sd.sdvar_autoregressive_infer_cfg_parallel_v1_edit(image, mask, 3, more_smooth=True)
    with pytest.raises(E.SdvarError, match="mask is on cpu"):
        sd.sdvar_autoregressive_infer_cfg_parallel_v1_edit(image, mask.cpu(), 3)
    with pytest.raises(E.SdvarError, match="top_k"):
        sd.sdvar_autoregressive_infer_cfg_parallel_v1_edit(image, mask, 3, g_seed=1, top_k=[900, 0])
    with pytest.raises(E.SdvarError, match="label_B"):
        sd.sdvar_autoregressive_infer_cfg_parallel_v1_edit(image, mask, None, g_seed=[1, 2, 3])
