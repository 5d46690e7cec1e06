"""CPU: the two references of tests/sampler_hard_cases.py against each other, on every case the GPU battery (tests/test_gpu_sampler_hard.py) runs.

R1 (the torch-fp32 oracle) and R2 (float64, stable (value, index) order) must agree wherever the operation is well defined: the same surviving set on rows
without ties at either cut, the same number and values kept on every row.  The seeds of the cases are chosen here so that the references alone stay within
the ambiguity caps (set-ambiguous rows: 5 % of a random-continuous case, 0 of a constructed one; draw-ambiguous rows: 1 %); the GPU test asserts the same
caps and never excludes more.  Also here: the KL rule's float64 statement against the oracle, the distance of every token's KL from the thresholds used,
and the accept scan's float32-rate known answers."""
import numpy as np
import pytest
import torch

import sampler_hard_cases as H
from oracle import var_oracle as orc

torch.set_grad_enabled(False)


@pytest.mark.parametrize("name", [c.name for c in H.ALL_CASES])
def test_references_agree(name):
    ref = H.reference(name)
    c = ref["case"]
    m1, m2 = ref["masked1"], ref["masked"]
    amb, tie = ref["set_ambiguous"], ref["tie"]
    print(f"{name}: rows {c.rows} set-ambiguous {int(amb.sum())} (cap {c.set_cap}) draw-ambiguous {int(ref['draw_ambiguous'].sum())} (cap {c.draw_cap}) "
          f"tied {int(tie.sum())} min margin {float(ref['margin'].min()):.3g} min gap {float(ref['gap'].min()):.3g} "
          f"survivors before top-p {int(ref['n_topk'].min())}..{int(ref['n_topk'].max())} kept {int(ref['n_keep'].min())}..{int(ref['n_keep'].max())}")
    assert int(amb.sum()) <= c.set_cap
    assert int(ref["draw_ambiguous"].sum()) <= c.draw_cap
    assert not torch.isnan(ref["cfg"]).any() and not torch.isposinf(ref["cfg"]).any() and bool((ref["n_keep"] >= 1).all())
    clean = ~tie & ~amb
    assert torch.equal(H.bits(m1[clean]), H.bits(m2[clean])), "surviving sets differ on rows without ties"
    assert torch.equal((m1 > H.NEG_INF).sum(-1), ref["n_keep"]), "number kept"
    assert torch.equal(H.sorted_kept(m1), H.sorted_kept(m2)), "kept values"
    ok = (m1 > H.NEG_INF).eq(ref["keep"]).all(-1) & ~ref["draw_ambiguous"]
    ids2 = (m2.double().softmax(-1) / ref["q"].double()).argmax(-1)
    assert torch.equal(ref["ids1"].reshape(-1)[ok], ids2[ok]), "draw differs where the sets agree"


def test_families_hit_what_they_are_built_for():
    """The constructions do what the battery relies on: the survivor counts that select the sort path, the ties, the zero signs, the one-survivor rows."""
    n = lambda name: H.reference(name)["n_topk"]
    assert bool((n("b1024") == 1024).all()) and bool((n("b1025") == 1025).all())                       # both sides of the compact / full threshold
    assert bool((n("ties900_full") == 1100).all()) and bool((n("ties900_compact") == 1000).all())
    assert bool((n("zeros4096_compact") == 949).all()) and bool((n("zeros4096_full") == 1800).all()) and bool((n("zeros1000") == 950).all())
    assert bool((n("inf1000_k900") == 667).all()) and bool((n("equal4096_k900") == 4096).all())
    for name in ("peak4096_k900", "peak4096_full", "peak1000_k900", "peak4_k900", "g4096_p_near0_compact", "g4096_p_near0_full", "g4096_k1", "peak8_k1"):
        assert bool((H.reference(name)["n_keep"] == 1).all()), name
    for name in ("zeros4096_compact", "zeros4096_full", "zeros4096_nok", "zeros1000", "zeros8"):
        ref = H.reference(name)
        cl, keep = ref["cfg"].reshape(-1, ref["case"].V), ref["keep"]
        zero, neg = cl == 0, H.bits(cl) == H.bits(torch.tensor([-0.0]))
        assert bool(ref["tie"].all()), name
        # zeros of both signs on both sides of the top-p cut: the cut falls inside the run of zeros
        assert bool(((zero & keep).any(-1) & (zero & ~keep).any(-1)).all()) and bool((neg.any(-1) & (zero & ~neg).any(-1)).all()), name
    for name in ("quant4096_k900", "quant1000_k900", "ties900_full", "ties900_compact", "equal4096_full"):
        assert float(H.reference(name)["tie"].float().mean()) >= 0.9, name
    # R1's unstable sort really does pick other survivors among equal values than the (value, index) rule: a naive "equal to the oracle" check would fail
    differs = sum(int((~(H.reference(nm)["masked1"] > H.NEG_INF).eq(H.reference(nm)["keep"]).all(-1)).sum()) for nm in ("quant4096_k900", "equal4096_full"))
    assert differs > 0


def test_inf_in_both_halves_is_nan_in_the_reference_arithmetic():
    """Why the `inf` family masks the cond half only: -inf at the same place of both halves gives NaN CFG logits for every t, NaN is out of scope."""
    lg = torch.tensor([[[1.0, -np.inf]], [[0.5, -np.inf]]])
    for t in (0.0, 1.5):
        assert bool(torch.isnan(orc.cfg_combine(lg, 1, t)[0, 0, 1]))
    lg[1, 0, 1] = 0.25
    for t in (0.0, 1.5):
        assert float(orc.cfg_combine(lg, 1, t)[0, 0, 1]) == H.NEG_INF


# ------------------------------------------------------------------------------------------------ KL rule, accept scan
@pytest.mark.parametrize("V", [1000, 8])
def test_kl_oracle_is_the_float64_rule_with_zero_log_zero(V):
    """orc.token_matches('kl') == (float64 KL with 0 * log 0 = 0) <= float32(kl_thr), also where both distributions carry the same -inf entries; and no
    token's KL lies within 1e-4 * max(1, KL) of a threshold the GPU test uses (cap 0), so the kernel's float32 inputs to exp / log cannot decide."""
    vc = H.kl_case(V)
    for cl_t, cl_d, ids in zip(vc.cfg(), vc.cfg("draft"), vc.ids):
        kl = H.kl_ref(cl_t, cl_d)
        assert not torch.isnan(kl).any()
        for thr in H.KL_THRESHOLDS:
            fin = torch.isfinite(kl)
            assert bool(((kl[fin] - thr).abs() > 1e-4 * kl[fin].clamp(min=1.0)).all()), (thr, kl)
            assert torch.equal(orc.token_matches(ids, cl_t, orc.MatchRule("kl", kl_thr=thr), cl_d), kl <= float(np.float32(thr)))
    kl1 = H.kl_ref(vc.cfg()[1], vc.cfg("draft")[1])
    assert bool(torch.isposinf(kl1[:, 0]).all()) and bool((kl1[:, 2] == 0).all()) and bool((kl1[:, 1] > 0).all())
    vi = H.kl_case(V, identical=True)
    for cl_t, cl_d, ids in zip(vi.cfg(), vi.cfg("draft"), vi.ids):
        assert bool(torch.isneginf(cl_t).any()) and bool((H.kl_ref(cl_t, cl_d) == 0).all())
        assert bool(orc.token_matches(ids, cl_t, orc.MatchRule("kl", kl_thr=0.0), cl_d).all())


def test_accept_scan_float32_rate_known_answers():
    """The oracle's scan on the constructed counts: float32 rates against double thresholds, as the reference's `.float().mean() >= thr` does."""
    assert float(np.float32(1) / np.float32(10)) > 0.1 and float(np.float32(1) / np.float32(3)) > 1.0 / 3.0 and float(np.float32(7) / np.float32(10)) < 0.7
    for lens, matched, table in ((H.SCAN_LENS, H.SCAN_MATCHED, H.SCAN_16), (H.SCAN_3_LENS, H.SCAN_3_MATCHED, H.SCAN_3)):
        vc = H.scan_case(lens, matched)
        for thr, n_expect in table:
            n, m, tot, _, _ = orc.accept_scan_ex(vc.ids, vc.cfg(), thr, orc.MatchRule())
            assert m == list(matched) and tot == list(lens)
            assert n == n_expect == H.scan_expect(lens, matched, thr), (thr, n)


def test_verify_constructions():
    for V in (4096, 1000, 8):
        vc = H.argmax_tie_case(V)
        cl = torch.cat(vc.cfg(), 1)
        assert torch.equal(cl.argmax(-1), vc.expect_argmax)
        assert bool(((cl == cl.amax(-1, keepdim=True)).sum(-1)[:, :6] == 2).all())
    vc = H.topk_tie_case(1000)
    for cl, ids in zip(vc.cfg(), vc.ids):
        xd = cl.gather(-1, ids.unsqueeze(-1))
        assert bool(((cl > xd).sum(-1)[:, :2] == H.TOPK_TIE_ABOVE).all()) and bool(((cl == xd).sum(-1)[:, :2] == 6).all())
        assert bool(((cl == xd).sum(-1)[:, 2:] > 1).all()), "the quantised rows must tie at the draft token's score"


@pytest.mark.parametrize("name", [g.name for g in H.GUMBEL_CASES])
def test_gumbel_reference_inputs(name):
    gi = H.gumbel_inputs(name)
    gc = gi["case"]
    print(f"{name}: oracle fp32 error vs float64 {gi['err_oracle']:.3g} bar {H.gumbel_bar(gi):.3g} finite entries {int(gi['n_finite'].min())}..{int(gi['n_finite'].max())}")
    assert torch.isfinite(gi["h64"]).all() and torch.isfinite(gi["h_oracle"]).all()
    if gc.name.startswith("one_"):
        assert bool((gi["n_finite"] == 1).all())
    if gc.name.startswith("k1024_"):
        assert bool((gi["n_finite"] == 1024).all())
