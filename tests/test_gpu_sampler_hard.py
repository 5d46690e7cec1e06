"""GPU: the five kernels of csrc/sampler.hip on hard inputs - ties at both cuts, peaked and heavy-tailed rows, rows holding -inf, zeros of both signs,
the 1024 / 1025 survivor boundary between the compact and the full sort, V < 4096 - against the two references of tests/sampler_hard_cases.py (R1: the
torch-fp32 oracle; R2: float64 with the kernel's documented (value, index) tie rule) and float64 statements of the KL rule and the gumbel mix.
tests/test_sampler_hard_host.py checks the references against each other and fixes the seeds.

Conventions pinned here:
  ties        equal values are ordered by index in the top-p sort, the lowest indices are removed first.  The oracle (torch.sort, not stable) agrees with
              that in the NUMBER kept and the kept VALUES only; which of several equal entries survives is compared with R2.
  zero sign   -0.0 and +0.0 are one value in the sort key; the stored logits keep their bits.
  KL rule     0 * log 0 = 0: entries masked to -inf in the target contribute nothing (kernel and oracle; the oracle used to return NaN there).
Out of scope: NaN or +inf logits, rows that are all -inf (torch's softmax and the kernel both return NaN ids / probabilities there; nothing is pinned).

Measured on an MI355X (each case prints its figures; run with -s): one set-ambiguous row in all 60 sampler cases (g4096_p_near1), no draw-ambiguous row.
gumbel_mix: kernel error / torch-fp32 oracle error against float64 is 0.995-1.00 on nine of the ten cases with an error above 1e-9 (largest error 2.15e-5 at
tau = 0.005, V = 1000, Cv = 33; the oracle's own is 2.15e-5) and 1.89 on the tenth (1.8e-7 against 9.4e-8, 400 times under the floor); the bar is 4x.
Sensitivity (scratch builds of the library, this file run once against each): `x[i] <= kth` in the top-k filter fails 18 tests, the compact sort without its
"last entry always kept" guard fails 1, the verify kernel's argmax tie-break reversed fails 3, the library before the zero-sign change fails 5."""
import ctypes as C

import numpy as np
import pytest
import torch

import sampler_hard_cases as H
from oracle import var_oracle as orc
from sdvar_amd import engine as E

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ cfg_sample
def _run_sampler(dev, ref):
    c = ref["case"]
    ids = torch.full((c.B, c.l), -7, dtype=torch.int64, device=dev)
    dbg = torch.full((c.B, c.l, c.V), 123.0, device=dev)
    E.cfg_sample(ref["logits"].to(dev).contiguous(), c.B, c.l, c.V, c.t, c.top_k, c.top_p, ref["q"].to(dev).contiguous(), 0, 0, 0, ids, 0, c.l, dbg)
    return ids.cpu().reshape(-1), dbg.cpu().reshape(-1, c.V)


def _check_sampler_case(dev, name):
    ref = H.reference(name)
    c = ref["case"]
    ids, dbg = _run_sampler(dev, ref)
    m1, q = ref["masked1"], ref["q"]
    amb, tie = ref["set_ambiguous"], ref["tie"]
    gap = H.draw_gap(dbg, q)                                  # of the kernel's own surviving set
    damb = gap <= H.AMBIG_DRAW
    path = "none" if c.top_p <= 0 else ("compact" if int(ref["n_topk"].max()) <= 1024 else ("full" if int(ref["n_topk"].min()) > 1024 else "both"))
    print(f"{name}: rows {c.rows} set-ambiguous {int(amb.sum())} (cap {c.set_cap}) draw-ambiguous {int(damb.sum())} (cap {c.draw_cap}) tied {int(tie.sum())} "
          f"sort path {path} survivors before top-p {int(ref['n_topk'].min())}..{int(ref['n_topk'].max())} kept {int(ref['n_keep'].min())}..{int(ref['n_keep'].max())}")
    assert int(amb.sum()) <= c.set_cap and int(damb.sum()) <= c.draw_cap
    assert not torch.isnan(dbg).any()
    kept = dbg > H.NEG_INF
    # the stored values are the CFG logits' bits or -inf: no fma contraction on the heavy tails, zero signs kept
    assert torch.equal(H.bits(dbg)[kept], H.bits(ref["cfg"].reshape(-1, c.V))[kept]), "a kept logit is not the torch-fp32 CFG value"
    clean = ~tie
    assert torch.equal(H.bits(dbg[clean]), H.bits(m1[clean])), "masked logits differ from the oracle's on rows without ties"
    assert torch.equal(kept.sum(-1), (m1 > H.NEG_INF).sum(-1)), "number kept differs from the oracle's"
    assert torch.equal(H.sorted_kept(dbg), H.sorted_kept(m1)), "kept values differ from the oracle's"
    assert torch.equal(kept[~amb], ref["keep"][~amb]), "surviving set differs from the (value, index) rule"
    own = (dbg.softmax(-1) / q).argmax(-1)                    # torch fp32 on the kernel's own masked logits: the draw, separated from the set
    assert torch.equal(ids[~damb], own[~damb]), "draw differs from argmax(softmax(masked) / q)"
    same = kept.eq(m1 > H.NEG_INF).all(-1) & ~damb
    assert torch.equal(ids[same], ref["ids1"].reshape(-1)[same]), "ids differ from the oracle's where the sets agree"
    return ref, ids, dbg


@pytest.mark.parametrize("name", [c.name for c in H.RANDOM_4096])
def test_cfg_sample_random_rows_v4096(dev, name):
    ref, _, dbg = _check_sampler_case(dev, name)
    if name in ("b1024", "b1025"):        # the two sides of the threshold between the compact and the full sort: the count the kernel branches on,
        c = ref["case"]                   # from the kernel itself (the same rows with top-p off leave exactly the top-k survivors in dbg)
        assert bool((ref["n_topk"] == c.top_k).all())
        ids = torch.zeros(c.B, c.l, dtype=torch.int64, device=dev); after_k = torch.empty(c.B, c.l, c.V, device=dev)
        E.cfg_sample(ref["logits"].to(dev).contiguous(), c.B, c.l, c.V, c.t, c.top_k, 0.0, ref["q"].to(dev).contiguous(), 0, 0, 0, ids, 0, c.l, after_k)
        assert bool(((after_k > H.NEG_INF).sum(-1) == c.top_k).all())


@pytest.mark.parametrize("name", [c.name for c in H.CONSTRUCTED_4096])
def test_cfg_sample_constructed_rows_v4096(dev, name):
    _check_sampler_case(dev, name)


@pytest.mark.parametrize("name", [c.name for c in H.V1000])
def test_cfg_sample_v1000(dev, name):
    _check_sampler_case(dev, name)


@pytest.mark.parametrize("name", [c.name for c in H.SMALL_V])
def test_cfg_sample_v8_v4(dev, name):
    _check_sampler_case(dev, name)


@pytest.mark.parametrize("name", ["g1000_k900", "inf1000_full", "g8_full", "quant8_kV"])
def test_cfg_sample_device_noise_small_vocab(dev, name):
    """q = None (in-kernel Philox) == the explicit-noise mode fed by sdvar_op_noise_fill, at V = 1000 and V = 8."""
    ref = H.reference(name)
    c = ref["case"]
    lib = E.load_library()
    q = torch.empty(c.rows, c.V, device=dev)
    E._check(lib.sdvar_op_noise_fill(C.c_void_p(q.data_ptr()), c.B, c.l, c.V, 4321, 6, 3, _st()))
    lg = ref["logits"].to(dev).contiguous()
    a = torch.zeros(c.B, c.l, dtype=torch.int64, device=dev); b = torch.zeros_like(a)
    da = torch.empty(c.B, c.l, c.V, device=dev); db = torch.empty_like(da)
    E.cfg_sample(lg, c.B, c.l, c.V, c.t, c.top_k, c.top_p, None, 4321, 6, 3, a, 0, c.l, da)
    E.cfg_sample(lg, c.B, c.l, c.V, c.t, c.top_k, c.top_p, q, 0, 0, 0, b, 0, c.l, db)
    assert torch.equal(a, b) and torch.equal(H.bits(da), H.bits(db))


def test_cfg_sample_ids_offset_and_stride_v8(dev):
    ref = H.reference("g8_full")
    c = ref["case"]
    stride, off = 41, 9
    buf = torch.full((c.B, stride), -99, dtype=torch.int64, device=dev)
    E.cfg_sample(ref["logits"].to(dev).contiguous(), c.B, c.l, c.V, c.t, c.top_k, c.top_p, ref["q"].to(dev).contiguous(), 0, 0, 0, buf, off, stride)
    out = buf.cpu()
    assert torch.equal(out[:, off:off + c.l], ref["ids1"])
    assert bool((out[:, :off] == -99).all()) and bool((out[:, off + c.l:] == -99).all())


# ------------------------------------------------------------------------------------------------ verify_accept, cfg_combine
def _run_verify(dev, vc, thr, rule=None):
    lens, lsum = list(vc.lens), sum(vc.lens)
    lg = torch.cat(vc.logits, 1).to(dev).contiguous()
    ids = torch.cat(vc.ids, 1).to(dev).contiguous()
    dl = torch.cat([d.reshape(-1) for d in vc.draft]).to(dev).contiguous() if vc.draft is not None else None
    counts = torch.full((40,), -5, dtype=torch.int32, device=dev)
    match = torch.full((vc.B, lsum), 9, dtype=torch.uint8, device=dev)
    corr = torch.full((vc.B, lsum), -9, dtype=torch.int64, device=dev); am = torch.full_like(corr, -9)
    E.verify_accept(lg, vc.B, lens, vc.V, vc.ts, ids, 0, lsum, thr, counts, argmax_out=am, rule=rule, draft_logits=dl, match_out=match, corrected_out=corr)
    return counts.cpu().tolist(), match.cpu().bool(), corr.cpu(), am.cpu()


def _check_vs_oracle(vc, thr, rule, out):
    c, match, corr, am = out
    n = len(vc.lens)
    orule = orc.MatchRule(rule.rule, rule.top_k, rule.kl_thr) if rule is not None else orc.MatchRule()
    n_o, matched_o, total_o, masks_o, corr_o = orc.accept_scan_ex(vc.ids, vc.cfg(), thr, orule, vc.cfg("draft") if vc.draft is not None else None)
    assert torch.equal(am, torch.cat([x.argmax(-1) for x in vc.cfg()], 1)), "argmax"
    assert torch.equal(match, torch.cat(masks_o, 1)), "per-token verdict"
    assert torch.equal(corr, torch.cat(corr_o, 1)), "corrected ids"
    assert c[:n] == matched_o and c[16] == n_o and c[17:17 + n] == total_o, (c, matched_o, n_o, total_o)
    return n_o, matched_o


@pytest.mark.parametrize("V", [4096, 1000, 8])
def test_verify_argmax_ties_smallest_index_wins(dev, V):
    """The maximum duplicated across lanes, across a thread's chunks and across waves; an all-equal row; a -inf row with one finite entry."""
    vc = H.argmax_tie_case(V)
    out = _run_verify(dev, vc, 0.5)
    assert torch.equal(out[3], vc.expect_argmax)
    n_o, matched_o = _check_vs_oracle(vc, 0.5, None, out)
    assert matched_o == [6, 3]                       # stage 0: tokens 0-2 of both images; stage 1: token 6 of image 0, token 7 of both
    out_k = _run_verify(dev, vc, 0.5, E.MatchRule("topk", top_k=1))          # top_k = 1 counts strictly-higher entries: both holders of the maximum match
    _check_vs_oracle(vc, 0.5, E.MatchRule("topk", top_k=1), out_k)
    assert bool(out_k[1].all())


@pytest.mark.parametrize("top_k", [1, 3, 4, 5, 9, 1000, 1005])
def test_verify_topk_rule_ties_at_the_draft_score(dev, top_k):
    """Six entries tied at the draft token's score with three strictly above: the rule holds iff top_k > 3.  Quantised halves whose per-stage t cancels into
    exact ties.  top_k = 1, top_k >= V."""
    vc = H.topk_tie_case(1000)
    rule = E.MatchRule("topk", top_k=top_k)
    out = _run_verify(dev, vc, 0.5, rule)
    _check_vs_oracle(vc, 0.5, rule, out)
    ctl = torch.cat([out[1][:, :2], out[1][:, 4:6]], 1)
    assert bool(ctl.all()) if top_k > H.TOPK_TIE_ABOVE else not bool(ctl.any())
    if top_k >= vc.V:
        assert bool(out[1].all())


@pytest.mark.parametrize("rule", [E.MatchRule(), E.MatchRule("topk", top_k=5), E.MatchRule("topk", top_k=2000)])
def test_verify_out_of_range_draft_ids(dev, rule):
    """Draft ids -1 and V: no match under any rule, corrected = the target's argmax, nothing dereferenced; the in-range tokens as the oracle says."""
    vc = H.topk_tie_case(1000, oob=True)
    c, match, corr, am = _run_verify(dev, vc, 0.5, rule)
    cls = vc.cfg()
    am_o = torch.cat([x.argmax(-1) for x in cls], 1)
    ids = torch.cat(vc.ids, 1)
    oob = (ids < 0) | (ids >= vc.V)
    assert int(oob.sum()) == 8
    orule = orc.MatchRule(rule.rule, rule.top_k)
    m_o = torch.cat([orc.token_matches(i.clamp(0, vc.V - 1), x, orule) for i, x in zip(vc.ids, cls)], 1) & ~oob
    assert torch.equal(am, am_o) and torch.equal(match, m_o) and not bool(match[oob].any())
    assert torch.equal(corr, torch.where(m_o, ids, am_o))
    assert c[:2] == [int(m_o[:, :4].sum()), int(m_o[:, 4:].sum())] and c[17:19] == [8, 8]


@pytest.mark.parametrize("V", [1000, 8])
def test_verify_kl_rule(dev, V):
    """KL(target || draft) in float64 with 0 * log 0 = 0: shared -inf entries, a draft -inf under a finite target (never a match), a peaked target;
    identical logits at kl_thr = 0 (every token matches)."""
    vc = H.kl_case(V)
    kl = torch.cat([H.kl_ref(a, b) for a, b in zip(vc.cfg(), vc.cfg("draft"))], 1)
    for thr in H.KL_THRESHOLDS:
        rule = E.MatchRule("kl", kl_thr=thr)
        out = _run_verify(dev, vc, 0.5, rule)
        _check_vs_oracle(vc, 0.5, rule, out)
        assert torch.equal(out[1], kl <= float(np.float32(thr)))
        assert not bool(out[1][:, 2].any()) and bool(out[1][:, 4].all())        # stage 1: token 0 has KL = +inf, token 2 has KL = 0
    vi = H.kl_case(V, identical=True)
    rule = E.MatchRule("kl", kl_thr=0.0)
    out = _run_verify(dev, vi, 1.0, rule)
    _check_vs_oracle(vi, 1.0, rule, out)
    assert bool(out[1].all()) and out[0][16] == 2


@pytest.mark.parametrize("thr,n_expect", list(H.SCAN_16))
def test_accept_scan_16_stages(dev, thr, n_expect):
    """n_chunk = 16, totals 1, 2, 3, 7 and 10: the float32 rate against the double threshold decides; the counts of every stage are filled although
    n_accept stops at the first failure."""
    vc = H.scan_case(H.SCAN_LENS, H.SCAN_MATCHED)
    out = _run_verify(dev, vc, thr)
    _check_vs_oracle(vc, thr, None, out)
    c = out[0]
    assert c[:16] == list(H.SCAN_MATCHED) and c[17:33] == list(H.SCAN_LENS) and c[16] == n_expect


@pytest.mark.parametrize("thr,n_expect", list(H.SCAN_3))
def test_accept_scan_rate_rounds_down(dev, thr, n_expect):
    """7 of 10 is 0.699999988 in float32: below the double 0.7, equal to float32(0.7)."""
    vc = H.scan_case(H.SCAN_3_LENS, H.SCAN_3_MATCHED)
    out = _run_verify(dev, vc, thr)
    _check_vs_oracle(vc, thr, None, out)
    assert out[0][16] == n_expect and out[0][:3] == list(H.SCAN_3_MATCHED)


def test_verify_accept_rejects_17_stages(dev):
    lens = [1] * 17
    lg = torch.zeros(2, 17, 8, device=dev); ids = torch.zeros(1, 17, dtype=torch.int64, device=dev)
    counts = torch.zeros(40, dtype=torch.int32, device=dev)
    with pytest.raises(E.SdvarError):
        E.verify_accept(lg, 1, lens, 8, [0.0] * 17, ids, 0, 17, 0.5, counts)


def test_cfg_combine_heavy_tails_v1000(dev):
    vc = H.combine_case()
    outs = E.cfg_combine(torch.cat(vc.logits, 1).to(dev).contiguous(), vc.B, vc.lens, vc.V, vc.ts)
    for j, (o, ref) in enumerate(zip(outs, vc.cfg())):
        assert torch.equal(H.bits(o.cpu()), H.bits(ref)), f"stage {j}"


# ------------------------------------------------------------------------------------------------ gumbel_mix
def _quant_ctx(dev, codebook, B):
    """A quantiser context around an arbitrary (V, Cv) codebook: gumbel_mix reads only the codebook, the Phi convolution is a placeholder."""
    Cv = codebook.shape[1]
    sd = {"quantize.embedding.weight": codebook, "quantize.quant_resi.qresi.weight": torch.zeros(Cv, Cv, 3, 3), "quantize.quant_resi.qresi.bias": torch.zeros(Cv)}
    return E.QuantCtx(sd, (1, 2), B, dev)


@pytest.mark.parametrize("name", [g.name for g in H.GUMBEL_CASES])
def test_gumbel_mix_vs_float64(dev, name):
    gi = H.gumbel_inputs(name)
    gc, c = gi["case"], gi["sampler_case"]
    qc = _quant_ctx(dev, gi["codebook"], c.B)
    buf = torch.full((c.rows * gc.Cv + 64,), 77.0, device=dev)                # h with a sentinel tail: Cv = 33 and 8 are no multiple of the kernel's 32 channels
    h = buf[:c.rows * gc.Cv].view(c.B, c.l, gc.Cv)
    qc.gumbel_mix(gi["masked"].to(dev).contiguous(), c.B, c.l, gc.ratio, gc.tau, gi["e"].to(dev).contiguous(), 0, 0, 0, h)
    assert bool((buf[c.rows * gc.Cv:] == 77.0).all())
    h = h.cpu()
    qc.close()
    err, bar = float((h.double() - gi["h64"]).abs().max()), H.gumbel_bar(gi)
    ratio = err / gi["err_oracle"] if max(err, gi["err_oracle"]) > 1e-9 else float("nan")
    print(f"{name}: kernel error {err:.3g} oracle error {gi['err_oracle']:.3g} ratio {ratio:.3g} bar {bar:.3g}")
    assert torch.isfinite(h).all() and err <= bar, (err, bar)
    one = (gi["n_finite"] == 1)
    if bool(one.any()):                   # p is exactly 1 on the survivor: h is that codebook row, bit for bit
        rows = gi["codebook"][gi["masked"].argmax(-1)]
        assert torch.equal(H.bits(h[one]), H.bits(rows[one]))
    if name.startswith("one_"):
        assert bool(one.all())
