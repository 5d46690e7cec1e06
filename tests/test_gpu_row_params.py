"""GPU: per-image sampling parameters.  The *_rows kernels of csrc/sampler.hip against their scalar twins, bit for bit (a batch whose images carry the
parameters of different cases == the scalar launch of each case), and the sampler loops built on them: uniform sequences are the scalar call, a
heterogeneous batch equals the CPU oracle run once per image with B = 1, the speculative loop's verify step uses every image's own CFG factor.
Inputs come from tests/sampler_hard_cases.py (shared, cached references) and tests/row_params_cases.py (the seeds, picked on the CPU)."""
import numpy as np
import pytest
import torch

import row_params_cases as RC
import sampler_hard_cases as H
from conftest import state_dicts
from oracle import var_oracle as orc
from sdvar_amd import engine as E
from sdvar_amd.ladder import LADDER_256, as_ladder

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
LAD = as_ladder(LADDER_256)
LOGIT_TOL, FHAT_TOL = 1e-3, 1e-4          # the project's bars (tests/test_gpu_e2e.py)


def _tables(dev, ts, top_k=None, top_p=None, seeds=None, index=None):
    """RowParams from explicit per-(stage, image) t: ts (n, B) or (B,)."""
    ts = np.atleast_2d(np.asarray(ts, np.float64))
    n, B = ts.shape
    fac = np.stack([(1.0 + ts).astype(np.float32), ts.astype(np.float32)], -1)
    img = np.zeros(B, E.ROW_IMAGE_DTYPE)
    top_p = [0.0] * B if top_p is None else top_p
    img["top_k"] = [0] * B if top_k is None else top_k
    img["use_top_p"] = [1 if p > 0.0 else 0 for p in top_p]
    img["top_p_thr"] = [np.float32(1.0 - p) for p in top_p]
    seeds = [0] * B if seeds is None else seeds
    img["seed_lo"], img["seed_hi"] = [s & 0xFFFFFFFF for s in seeds], [s >> 32 for s in seeds]
    img["index"] = [0] * B if index is None else index
    return E.RowParams.from_tables(fac, img, dev)


class _Guarded:
    """A device tensor inside a larger buffer of sentinels: whatever a kernel writes outside its output is seen."""

    def __init__(self, dev, shape, dtype, fill, pad=64):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev)
        self.view = self.buf[pad:pad + n].view(*shape)
        self.fill, self.pad, self.n = fill, pad, n

    def intact(self):
        return bool((self.buf[:self.pad] == self.fill).all()) and bool((self.buf[self.pad + self.n:] == self.fill).all())


# ------------------------------------------------------------------------------------------------ 1. cfg_sample_rows
SAMPLE_GROUPS = {
    "v4096": ["b1024", "b1025", "g4096_k40", "g4096_none", "g4096_p_near0_full", "g4096_kV", "heavy4096_k900", "inf4096_full"],
    "v1000": [c.name for c in H.V1000 if c.l == 16],
    "v8": [c.name for c in H.SMALL_V if c.V == 8],
    "v4": [c.name for c in H.SMALL_V if c.V == 4],
}
STRIDE, OFF = 23, 4            # ids land at ids[b * STRIDE + OFF + tok]: the columns around them are guards


def _stack(names, sl=slice(None), imgs=slice(None)):
    refs = [H.reference(n) for n in names]
    V = refs[0]["case"].V
    assert all(r["case"].V == V and r["case"].l == 16 and r["case"].B == 2 for r in refs)
    cond = torch.cat([r["logits"][:2][imgs, sl] for r in refs], 0)
    unc = torch.cat([r["logits"][2:][imgs, sl] for r in refs], 0)
    q = torch.cat([r["q"].view(2, 16, V)[imgs, sl] for r in refs], 0)
    per = cond.shape[0] // len(refs)
    return refs, torch.cat([cond, unc], 0).contiguous(), q.contiguous(), per


def _scalar_sample(dev, c, lg, q, seed=0, draw=0, off=0):
    B, l = lg.shape[0] // 2, lg.shape[1]
    ids = torch.full((B, l), -7, dtype=torch.int64, device=dev); dbg = torch.full((B, l, c.V), 123.0, device=dev)
    E.cfg_sample(lg.to(dev).contiguous(), B, l, c.V, c.t, c.top_k, c.top_p, None if q is None else q.reshape(B * l, c.V).to(dev).contiguous(), seed, draw, off, ids, 0, l, dbg)
    return ids.cpu(), dbg.cpu()


def _rows_sample_equals_scalar(dev, names, philox, sl=slice(None), imgs=slice(None)):
    refs, lg, q, per = _stack(names, sl, imgs)
    B, l, V = lg.shape[0] // 2, lg.shape[1], lg.shape[2]
    cs = [r["case"] for r in refs]
    seed_of, off_of, draw = (lambda i: 4321 + 1000003 * i + (i << 33)), (lambda i: 3 + 5 * i), 6
    rows = _tables(dev, [c.t for c in cs for _ in range(per)], [c.top_k for c in cs for _ in range(per)], [c.top_p for c in cs for _ in range(per)],
                   [seed_of(i) for i in range(len(cs)) for _ in range(per)], [off_of(i) + j for i in range(len(cs)) for j in range(per)])
    ids = _Guarded(dev, (B, STRIDE), torch.int64, -7)
    dbg = _Guarded(dev, (B, l, V), torch.float32, 123.0)
    E.cfg_sample_rows(lg.to(dev), B, l, V, rows, 0, None if philox else q.reshape(B * l, V).to(dev), draw, ids.view, OFF, STRIDE, dbg.view)
    got_ids, got_dbg = ids.view.cpu(), dbg.view.cpu()
    assert ids.intact() and dbg.intact()
    assert bool((got_ids[:, :OFF] == -7).all()) and bool((got_ids[:, OFF + l:] == -7).all())
    paths = set()
    for i, (c, r) in enumerate(zip(cs, refs)):
        lo = per * i
        one = torch.cat([lg[lo:lo + per], lg[B + lo:B + lo + per]], 0)
        want_ids, want_dbg = _scalar_sample(dev, c, one, None if philox else q[lo:lo + per], seed_of(i), draw, off_of(i))
        assert torch.equal(H.bits(got_dbg[lo:lo + per]), H.bits(want_dbg)), f"{c.name}: masked logits differ from the scalar launch"
        assert torch.equal(got_ids[lo:lo + per, OFF:OFF + l], want_ids), f"{c.name}: ids differ from the scalar launch"
        if c.top_p > 0:                           # survivors of the top-k filter: what the kernel's choice of sort depends on
            paths |= {"compact" if int(x) <= 1024 else "full" for x in r["n_topk"]}
    return paths


@pytest.mark.parametrize("philox", [False, True], ids=["explicit_q", "philox"])
@pytest.mark.parametrize("group", list(SAMPLE_GROUPS))
def test_cfg_sample_rows_is_the_scalar_kernel(dev, group, philox):
    """Images of several cases in one launch, each with its case's (t, top_k, top_p) - and, with in-kernel Philox, its case's seed and counter."""
    names = SAMPLE_GROUPS[group]
    cs = [H.BY_NAME[n] for n in names]
    if group != "v4":                             # a top-k-off, a top-p-off and a both-off image in the batch (the V = 4 cases all use top-p)
        assert any(c.top_k == 0 and c.top_p > 0 for c in cs) and any(c.top_p == 0 and c.top_k > 0 for c in cs) and any(c.top_k == 0 and c.top_p == 0 for c in cs)
    paths = _rows_sample_equals_scalar(dev, names, philox)
    if group == "v4096":
        assert {"b1024", "b1025"} <= set(names) and paths == {"compact", "full"}          # both sort paths in one launch


@pytest.mark.parametrize("philox", [False, True], ids=["explicit_q", "philox"])
def test_cfg_sample_rows_one_token_and_one_image(dev, philox):
    _rows_sample_equals_scalar(dev, ["b1025", "g4096_none", "b1024"], philox, sl=slice(5, 6))                 # l = 1
    _rows_sample_equals_scalar(dev, ["g1000_k40"], philox, imgs=slice(1, 2))                                   # B = 1
    _rows_sample_equals_scalar(dev, ["g8_full"], philox, sl=slice(0, 1), imgs=slice(0, 1))                    # B = 1, l = 1


# ------------------------------------------------------------------------------------------------ 2. verify_accept_rows, cfg_combine_rows
RULES = [E.MatchRule(), E.MatchRule("topk", top_k=5), E.MatchRule("kl", kl_thr=0.5)]
CHUNK_LENS = [1, 4, 9]


def _verify(dev, B, V, lens, lg, ids, dl, thr, rule, ts=None, rows=None):
    lsum = sum(lens)
    counts = _Guarded(dev, (40,), torch.int32, -5)
    match = _Guarded(dev, (B, lsum), torch.uint8, 9)
    corr = _Guarded(dev, (B, lsum), torch.int64, -9); am = _Guarded(dev, (B, lsum), torch.int64, -9)
    E.verify_accept(lg.to(dev).contiguous(), B, lens, V, ts, ids.to(dev).contiguous(), 0, lsum, thr, counts.view, argmax_out=am.view, rule=rule,
                    draft_logits=None if dl is None else dl.to(dev).contiguous(), match_out=match.view, corrected_out=corr.view, rows=rows)
    assert counts.intact() and match.intact() and corr.intact() and am.intact()
    return counts.view.cpu().tolist(), match.view.cpu(), corr.view.cpu(), am.view.cpu()


def _image(x, b, B):
    return torch.stack([x[b], x[B + b]], 0)


def _rows_verify_equals_scalar(dev, B, V, lens, tl, idl, dll, ts, thr, rule):
    """tl / dll: per stage (2B, l_j, V) target / draft logits, idl per stage (B, l_j); ts (n, B).  The rows call on the batch against the scalar call on
    every image alone."""
    n = len(lens)
    rows = _tables(dev, ts)
    lg, ids = torch.cat(tl, 1), torch.cat(idl, 1)
    kl = rule.rule == "kl"
    dl = torch.cat([d.reshape(-1) for d in dll]) if kl else None
    c, match, corr, am = _verify(dev, B, V, lens, lg, ids, dl, thr, rule, rows=rows)
    outs = E.cfg_combine(lg.to(dev).contiguous(), B, lens, V, None, rows=rows)
    matched = [0] * n
    for b in range(B):
        dl_b = torch.cat([_image(d, b, B).reshape(-1) for d in dll]) if kl else None
        tb = [float(ts[j][b]) for j in range(n)]
        c1, m1, k1, a1 = _verify(dev, 1, V, lens, _image(lg, b, B), ids[b:b + 1], dl_b, thr, rule, ts=tb)
        assert torch.equal(am[b:b + 1], a1) and torch.equal(match[b:b + 1], m1) and torch.equal(corr[b:b + 1], k1), f"image {b}"
        matched = [x + y for x, y in zip(matched, c1[:n])]
        one = E.cfg_combine(_image(lg, b, B).to(dev).contiguous(), 1, lens, V, tb)
        for j in range(n):
            assert torch.equal(H.bits(outs[j][b:b + 1].cpu()), H.bits(one[j].cpu())), f"cfg_combine_rows: image {b}, stage {j}"
    assert c[:n] == matched and c[17:17 + n] == [B * l for l in lens]
    assert c[16] == H.scan_expect(lens, matched, thr, B)
    return c, matched


@pytest.mark.parametrize("rule", RULES, ids=[r.rule for r in RULES])
@pytest.mark.parametrize("V", [1000, 4096])
def test_verify_and_combine_rows_per_stage_and_image_factor(dev, V, rule):
    B, lens = 3, CHUNK_LENS
    g = np.random.Generator(np.random.Philox(key=[V, 77 + rule.code]))
    tl = [torch.from_numpy(g.standard_normal(size=(2 * B, l, V), dtype=np.float32) * np.float32(2)) for l in lens]
    dll = [t + torch.from_numpy(g.standard_normal(size=(2 * B, l, V), dtype=np.float32) * np.float32(0.5)) for t, l in zip(tl, lens)]
    ts = np.array([[0.0, 0.37, 1.5], [0.5, 2.25, 0.1], [3.0, 0.0, 0.83]])          # a different t per (stage, image)
    idl = []
    for j, l in enumerate(lens):                 # draft ids: the image's own CFG argmax on some tokens, its second best or a random id on the others
        ids = torch.from_numpy(g.integers(0, V, size=(B, l)))
        for b in range(B):
            cl = orc.cfg_combine(_image(tl[j], b, B), 1, float(ts[j][b]))[0]
            top2 = cl.topk(2, dim=-1)[1]
            for tok in range(l):
                r = (tok + b + j) % 3
                if r < 2:
                    ids[b, tok] = top2[tok, r]
        idl.append(ids)
    for thr in (0.5, 0.3):
        c, matched = _rows_verify_equals_scalar(dev, B, V, lens, tl, idl, dll, ts, thr, rule)
    if rule.rule == "top1":
        assert 0 < sum(matched) < B * sum(lens)                                      # some tokens match, some do not


@pytest.mark.parametrize("V", [1000, 4096])
def test_verify_rows_on_the_argmax_tie_rows(dev, V):
    """The duplicated maxima of argmax_tie_case stay ties under every image's own factor (the uncond half is zero): smallest index wins, per image."""
    vc = H.argmax_tie_case(V)
    ts = np.array([[0.0, 1.5], [0.75, 0.0]])
    _rows_verify_equals_scalar(dev, vc.B, V, vc.lens, vc.logits, vc.ids, None, ts, 0.5, E.MatchRule())
    rows = _tables(dev, ts)
    am = _verify(dev, vc.B, V, vc.lens, torch.cat(vc.logits, 1), torch.cat(vc.ids, 1), None, 0.5, E.MatchRule(), rows=rows)[3]
    assert torch.equal(am, vc.expect_argmax)


def test_verify_rows_topk_and_kl_tie_builders(dev):
    vc = H.topk_tie_case(1000)
    ts = np.array([[1.0, 0.5], [0.5, 1.0]])
    for k in (3, 4, 5):
        _rows_verify_equals_scalar(dev, vc.B, vc.V, vc.lens, vc.logits, vc.ids, None, ts, 0.5, E.MatchRule("topk", top_k=k))
    vk = H.kl_case(1000)
    for thr in H.KL_THRESHOLDS:
        _rows_verify_equals_scalar(dev, vk.B, vk.V, vk.lens, vk.logits, vk.ids, vk.draft, np.array([[0.0, 0.4], [1.1, 0.0]]), 0.5, E.MatchRule("kl", kl_thr=thr))


# ------------------------------------------------------------------------------------------------ 3. gumbel_mix_rows
def _quant_ctx(dev, codebook, B):
    Cv = codebook.shape[1]
    sd = {"quantize.embedding.weight": codebook, "quantize.quant_resi.qresi.weight": torch.zeros(Cv, Cv, 3, 3), "quantize.quant_resi.qresi.bias": torch.zeros(Cv)}
    return E.QuantCtx(sd, (1, 2), B, dev)


@pytest.mark.parametrize("name", ["k1024_V4096_Cv32_r1_tau0.0135", "inf_V4096_Cv32_r0_tau0.27", "inf_V1000_Cv33_r1_tau0.005", "gauss_V1000_Cv8_r1_tau0.0135"])
def test_gumbel_mix_rows_per_image_key_and_counter(dev, name):
    gi = H.gumbel_inputs(name)
    gc, c = gi["case"], gi["sampler_case"]
    B, l, V = c.B, c.l, c.V
    qc = _quant_ctx(dev, gi["codebook"], B)
    masked = gi["masked"].to(dev).contiguous()
    seeds, index, draw = [77 + (5 << 32), 2**63 + 9], [3, 0], 4 | E.GUMBEL_DRAW
    rows = _tables(dev, [0.0] * B, seeds=seeds, index=index)
    for e in (None, gi["e"].to(dev).contiguous()):
        h = _Guarded(dev, (B, l, gc.Cv), torch.float32, 77.0)
        qc.gumbel_mix_rows(masked, B, l, gc.ratio, gc.tau, e, rows, draw, h.view)
        assert h.intact()
        for b in range(B):
            h1 = torch.full((1, l, gc.Cv), 77.0, device=dev)
            qc.gumbel_mix(masked[b:b + 1].contiguous(), 1, l, gc.ratio, gc.tau, None if e is None else e[b:b + 1].contiguous(), seeds[b], draw, index[b], h1)
            assert torch.equal(H.bits(h.view[b:b + 1].cpu()), H.bits(h1.cpu())), f"image {b}"
    qc.close()


# ------------------------------------------------------------------------------------------------ the sampler loops
@pytest.fixture(scope="module")
def models(dev):
    """d4 (plain AR, and the draft) and d6 (target, chunks of 2 stages) `stress` models on LADDER_256, B <= 3; one quantiser."""
    sd4, sdv = state_dicts(4, LADDER_256)
    sd6, _ = state_dicts(6, LADDER_256)
    c4, c6, qc = E.ModelCtx(sd4, 4, LADDER_256, 3, 1, dev), E.ModelCtx(sd6, 6, LADDER_256, 3, 2, dev), E.QuantCtx(sdv, LADDER_256, 3, dev)
    yield dict(sd4=sd4, sdv=sdv, ar=E.Sampler(c4, qc), spec=E.Sampler(c6, qc, c4))
    c4.close(); c6.close(); qc.close()


def _snap(res):
    return res.ids.clone(), res.f_hat.clone(), res.stats


LABELS = [s.label for s in RC.SETS]


# ---- 4. uniform sequences are the scalar call
@pytest.mark.parametrize("more_smooth", [False, True])
def test_uniform_sequences_are_the_scalar_plain_ar(dev, models, more_smooth):
    B, (c, k, p, s) = 3, (1.5, 900, 0.96, 31)
    lab = torch.tensor(LABELS, device=dev)
    ids0, f0, st0 = _snap(models["ar"].plain_ar(lab, c, k, p, E.Noise("device", s), more_smooth=more_smooth))
    ids1, f1, st1 = _snap(models["ar"].plain_ar(lab, [c] * B, [k] * B, [p] * B, E.Noise("device", [s] * B, [0, 1, 2]), more_smooth=more_smooth))
    assert torch.equal(ids0, ids1) and torch.equal(H.bits(f0), H.bits(f1)) and st0 == st1


@pytest.mark.parametrize("run_ahead", [True, False])
def test_uniform_sequences_are_the_scalar_spec_decode(dev, models, run_ahead):
    B, (c, k, p, s) = 3, (1.5, 900, 0.96, 31)
    lab = torch.tensor(LABELS, device=dev)
    ids0, f0, st0 = _snap(models["spec"].spec_decode(lab, c, 2, k, p, E.Noise("device", s), run_ahead=run_ahead))
    ids1, f1, st1 = _snap(models["spec"].spec_decode(lab, [c] * B, 2, [k] * B, [p] * B, E.Noise("device", [s] * B, [0, 1, 2]), run_ahead=run_ahead))
    assert torch.equal(ids0, ids1) and torch.equal(H.bits(f0), H.bits(f1)) and st0 == st1
    assert st0["rounds"] and st0["target_calls"] >= 5


# ---- 5. a heterogeneous batch against the oracle, one image at a time
@pytest.fixture(scope="module")
def oracle_runs(models):
    m, q = orc.OracleVAR(models["sd4"], RC.DEPTH, LADDER_256), orc.OracleQuant(models["sdv"], LADDER_256)
    return [RC.oracle_run(m, q, s, keep=True) for s in RC.SETS]


def _hetero(order):
    sets = [RC.SETS[i] for i in order]
    return ([s.label for s in sets], [s.cfg for s in sets], [s.top_k for s in sets], [s.top_p for s in sets], [s.seed for s in sets])


def test_heterogeneous_plain_ar_is_the_oracle_per_image(dev, models, oracle_runs):
    B = 3
    lab, cfg, top_k, top_p, seeds = _hetero([0, 1, 2])
    res = models["ar"].plain_ar(torch.tensor(lab, device=dev), cfg, top_k, top_p, E.Noise("host", seeds), trace=True)
    ids, f_hat = res.ids.cpu(), res.f_hat.cpu()
    for b, tr in enumerate(oracle_runs):
        assert torch.equal(ids[b:b + 1], torch.cat(tr.ids, 1)), f"image {b}: ids differ from the oracle's B = 1 run"
        for s in range(LAD.S):
            got = res.trace["logits"][s].cpu()
            err = max(float((got[b] - tr.logits[s][0]).abs().max()), float((got[B + b] - tr.logits[s][1]).abs().max()))
            assert err <= LOGIT_TOL, f"image {b} stage {s}: logits off by {err}"
        err = float((f_hat[b] - tr.f_hat[0]).abs().max())
        assert err <= FHAT_TOL, f"image {b}: f_hat off by {err}"
    # the batch an image lands in does not matter: another order, and the in-kernel Philox stream
    order = [2, 0, 1]
    lab2, cfg2, k2, p2, s2 = _hetero(order)
    for kind in ("host", "device"):
        ids2 = models["ar"].plain_ar(torch.tensor(lab2, device=dev), cfg2, k2, p2, E.Noise(kind, s2)).ids.cpu()
        for pos, i in enumerate(order):
            assert torch.equal(ids2[pos], ids[i]), f"{kind} noise: image {i} at position {pos}"


def test_one_image_alone_through_the_public_api(dev, models, oracle_runs):
    """VAR.autoregressive_infer_cfg: the heterogeneous batch with sequences, and image 2 alone at B = 1 with its scalars: the same ids for that image."""
    from sdvar_amd.var import VAR
    from sdvar_amd.vqvae import VQVAE
    vae = VQVAE(vocab_size=4096, z_channels=32, ch=160, v_patch_nums=LADDER_256, with_encoder=False)
    vae.load_state_dict(models["sdv"])
    var = VAR(vae_local=vae, depth=4, embed_dim=256, num_heads=4, attn_l2_norm=True, patch_nums=LADDER_256)
    var.load_state_dict(models["sd4"])
    vae, var = vae.to(dev), var.to(dev)
    var.noise_kind = "host"
    lab, cfg, top_k, top_p, seeds = _hetero([0, 1, 2])
    img = var.autoregressive_infer_cfg(3, torch.tensor(lab), g_seed=seeds, cfg=cfg, top_k=torch.tensor(top_k), top_p=np.array(top_p))
    ids3 = var.last_result.ids.cpu().clone()
    assert img.shape == (3, 3, 256, 256) and torch.isfinite(img).all()
    assert set(var.last_result.stats) >= {"target_calls", "draft_stage_calls", "forced_accepts", "accepted_tokens"} and var.last_result.stats["target_calls"] == LAD.S
    for b, tr in enumerate(oracle_runs):
        assert torch.equal(ids3[b:b + 1], torch.cat(tr.ids, 1)), b
    s = RC.SETS[2]
    var.autoregressive_infer_cfg(1, torch.tensor([s.label]), g_seed=s.seed, cfg=s.cfg, top_k=s.top_k, top_p=s.top_p)
    assert torch.equal(var.last_result.ids.cpu()[0], ids3[2])
    with pytest.raises(E.SdvarError, match="label_B"):
        var.autoregressive_infer_cfg(3, None, g_seed=seeds)
    with pytest.raises(E.SdvarError, match="top_k"):
        var.autoregressive_infer_cfg(3, torch.tensor(lab), g_seed=1, top_k=[900, 0])


def test_heterogeneous_more_smooth_plain_ar(dev, models):
    """more_smooth=True with per-image parameters, at the bar of tests/test_gpu_samplers.py::test_more_smooth_plain_ar: every stage's sampling + soft mix +
    f_hat update recomputed by the oracle from the HIP path's own logits of that stage, one image at a time."""
    B = 3
    lab, cfg, top_k, top_p, seeds = _hetero([0, 1, 2])
    res = models["ar"].plain_ar(torch.tensor(lab, device=dev), cfg, top_k, top_p, E.Noise("host", seeds), trace=True, more_smooth=True)
    ids, f_hat = res.ids.cpu(), res.f_hat.cpu()
    assert torch.isfinite(f_hat).all()
    oq = orc.OracleQuant(models["sdv"], LADDER_256)
    for b, st in enumerate(RC.SETS):
        nfn, f = RC.noise_of(st.seed), torch.zeros(1, 32, 16, 16)
        for s, pn in enumerate(LADDER_256):
            cl = orc.cfg_combine(_image(res.trace["logits"][s].cpu(), b, B), 1, LAD.cfg_t(st.cfg, s))
            ids_o, h = orc._stage_features(oq, cl, pn, st.top_k, st.top_p, nfn, s, True, s / (LAD.S - 1), None)
            assert torch.equal(ids_o, ids[b:b + 1, LAD.begin(s):LAD.cum[s]]), (b, s)
            f, _ = oq.next_input(s, f, h)
        assert (f[0] - f_hat[b]).abs().max().item() <= 2e-3 * max(1.0, f.abs().max().item()), b


# ---- 6. the speculative loop verifies every image with its own factor
def test_heterogeneous_spec_decode_verifies_with_each_images_factor(dev, models):
    B = 3
    lab, cfg, top_k, top_p, seeds = _hetero([0, 1, 2])
    labels = torch.tensor(lab, device=dev)
    res = models["spec"].spec_decode(labels, cfg, 2, top_k, top_p, E.Noise("device", seeds), trace=True)
    ids, f_hat, stats = res.ids.cpu().clone(), res.f_hat.clone(), res.stats
    rounds = stats["rounds"]
    assert len(rounds) == len(res.trace["target_logits"]) >= 5
    for rd, (cur, g, lg), drafted in zip(rounds, res.trace["target_logits"], res.trace["draft_ids"]):
        assert rd["stage"] == cur and rd["g"] == g
        lg, drafted, off, matched = lg.cpu(), drafted.cpu(), 0, []
        for j in range(g):
            s, l, m = cur + j, LAD.lens[cur + j], 0
            for b in range(B):
                t = LAD.cfg_t(cfg[b], s)           # torch fp32 with the kernel's arithmetic: float32(1 + t) * cond and float32(t) * uncond rounded, then a subtraction
                cl = float(np.float32(1.0 + t)) * lg[b, off:off + l] - float(np.float32(t)) * lg[B + b, off:off + l]
                top2 = cl.topk(2, dim=-1)[0]
                assert bool((top2[:, 0] > top2[:, 1]).all()), "a tied argmax: the comparison would be ill-posed"
                m += int((cl.argmax(-1) == drafted[b, off:off + l]).sum())
            matched.append(m); off += l
        assert matched == rd["matched"], (cur, matched, rd["matched"])
        n_acc = H.scan_expect([LAD.lens[cur + j] for j in range(g)], matched, 0.5, B)
        assert rd["n_accept"] == (1 if rd["forced"] else n_acc) and (not rd["forced"] or n_acc == 0)
    assert len({tuple(r["matched"]) for r in rounds}) > 1
    res2 = models["spec"].spec_decode(labels, cfg, 2, top_k, top_p, E.Noise("device", seeds), run_ahead=True)
    assert torch.equal(res2.ids.cpu(), ids) and torch.equal(H.bits(res2.f_hat), H.bits(f_hat))
    strip = lambda st: {k: v for k, v in st.items() if k != "discarded_speculative_rounds"}
    assert strip(res2.stats) == strip(stats)


def test_target_verify_batch_uses_the_states_table(dev, models):
    """A state begun with per-image parameters carries the table: SDVAR.target_verify_batch hands back every image's CFG logits under its own factor."""
    from sdvar_amd.var import SDVAR
    sd, smp, B, V = SDVAR(None, None), models["spec"], 3, 4096
    lab, cfg, top_k, top_p, seeds = _hetero([0, 1, 2])
    st = smp.spec_begin(torch.tensor(lab, device=dev), cfg, 2, top_k, top_p, E.Noise("device", seeds))
    for _ in range(2):                                  # stages 0-1, then the next round (whatever was accepted)
        cur = st.current_stage
        toks = sd.draft_generate_batch(st, B)
        outs, g = sd.target_verify_batch(toks, st, B)
        lsum = sum(st.glen)
        lg, off = smp.logits_t[:2 * B * lsum * V].view(2 * B, lsum, V).cpu(), 0
        for j in range(g):
            l = st.glen[j]
            assert outs[j].shape == (B, l, V)
            for b in range(B):
                t = LAD.cfg_t(cfg[b], cur + j)
                want = float(np.float32(1.0 + t)) * lg[b, off:off + l] - float(np.float32(t)) * lg[B + b, off:off + l]
                assert torch.equal(H.bits(outs[j][b].cpu()), H.bits(want)), (cur, j, b)
            off += l
        sd.update_state_with_accepted_tokens(toks, 1, st, B)
    smp.spec_end(st)


# ---- 7. refusals
def test_out_of_scope_paths_refuse_sequences_before_launching(dev, models):
    import sdvar_amd
    smp, lab = models["spec"], torch.tensor(LABELS, device=dev)
    before = smp.ids.clone()
    with pytest.raises(E.SdvarError, match="cfg"):
        smp.handoff(lab, [1.5, 1.0, 2.0], 900, 0.96, E.Noise("device", 1), 3)
    with pytest.raises(E.SdvarError, match="per-image seeds"):
        smp.handoff(lab, 1.5, 900, 0.96, E.Noise("device", [1, 2, 3]), 3)
    with pytest.raises(E.SdvarError, match="top_p"):
        models["ar"].resume_ar(torch.zeros(6, 256, device=dev), 0, 1, None, torch.zeros(3, 32, 16, 16, device=dev), 1.5, 900, [0.9, 0.9, 0.9], E.Noise("device", 1))
    with pytest.raises(E.SdvarError, match="top_k"):                                   # a wrong length
        smp.spec_decode(lab, 1.5, 2, [900, 0], 0.96, E.Noise("device", 1))
    with pytest.raises(E.SdvarError, match="entries"):
        models["ar"].plain_ar(lab, 1.5, 900, 0.96, E.Noise("device", [1, 2]))
    with pytest.raises(E.SdvarError, match="top_k"):
        models["ar"].plain_ar(lab, 1.5, [900, -1, 0], 0.96, E.Noise("device", 1))
    torch.cuda.synchronize()
    assert torch.equal(smp.ids, before) and smp.t.kv_len() == 0 and smp.d.kv_len() == 0          # nothing ran
    vae, d, t, sd = sdvar_amd.build_vae_var_speculative_decoding(device=dev, depth_draft=2, depth_target=2)
    with pytest.raises(E.SdvarError, match="cfg"):
        sd._initialize_inference_state(2, 5, 1, [1.5, 2.0], 2)
    with pytest.raises(E.SdvarError, match="g_seed"):
        sd._initialize_inference_state(2, 5, [1, 2], 1.5, 2)
    st = sd._initialize_inference_state(2, 5, 1, 1.5, 2)
    st.top_k, st.top_p = [900, 0], 0.96
    with pytest.raises(E.SdvarError, match="top_k"):
        sd.draft_generate_batch(st, 2)
    st.top_k = 900
    toks = sd.draft_generate_batch(st, 2)
    st.cfg = [1.5, 2.0]
    with pytest.raises(E.SdvarError, match="cfg"):
        sd.target_verify_batch(toks, st, 2)
    st.sampler.spec_end(st)
    with pytest.raises(E.SdvarError, match="cfg"):
        sd.sdvar_autoregressive_infer_cfg_sd_test3(2, 5, g_seed=1, cfg=(1.5, 2.0), entry_num=3)
    with pytest.raises(E.SdvarError, match="top_p"):
        d.autoregressive_infer_cfg_sd_helper1(2, 0, 1, None, torch.zeros(2, 32, 16, 16, device=dev), None, torch.zeros(4, 128, device=dev), None, top_p=[0.5, 0.5])
