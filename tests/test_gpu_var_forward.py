"""Teacher-forced VAR.forward and the validation statistics on the GPU: parity with the reference fixtures of tests/golden/make_tf_golden.py in
every GEMM mode, eval_ep end to end from images, a full-width d16 pass against the CPU oracle, condition dropout, sdvar_xent_stats against
torch, multi-pass batching, and the sampler's independence from the teacher-forcing context."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden, golden_parts, state_dicts

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
LOGIT_TOL = 1e-3          # BASELINE.json north_star: "within 1e-3 on logits"
MODES = ["f16x2", "bf16x3", "f32"]
TF_CASES = ["tf_d4_256_stress", "tf_d4_256_uncond", "tf_d4_512_stress", "tf_d4_256_sharedaln", "tf_d4_256_nol2"]
_MEMO = {}


def _var(dev, g, mode=None, sd=None, strict=True):
    from sdvar_amd import VAR, VQVAE
    pns, depth = tuple(int(p) for p in g["patch_nums"]), int(g["depth"])
    sa, l2 = bool(g["shared_aln"]), bool(g["attn_l2_norm"])
    if sd is None:
        sd, _ = state_dicts(depth, pns, "stress", int(g["wseed"]), vae=False, shared_aln=sa, attn_l2_norm=l2)
    vae = VQVAE(vocab_size=4096, ch=32, with_encoder=False, v_patch_nums=pns)
    m = VAR(vae, depth=depth, embed_dim=64 * depth, num_heads=depth, patch_nums=pns, shared_aln=sa, attn_l2_norm=l2, cond_drop_rate=0.0,
            drop_path_rate=0.1 * depth / 24)
    m.load_state_dict(sd, strict=strict)
    m = m.to(dev).eval()
    m.tf_gemm_mode = mode
    return m


def _inputs(dev, g, B=None):
    e = golden(str(g["encode"]))
    B = len(g["labels"]) if B is None else B
    return torch.from_numpy(g["labels"]).to(dev), torch.from_numpy(e["var_input"][:B]).to(dev)


def _cols(lg, idx):
    return np.take_along_axis(lg, idx.astype(np.int64), -1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", TF_CASES)
def test_forward_matches_reference(dev, mode, name):
    from sdvar_amd import engine as E
    g = golden(name)
    m = _var(dev, g, mode)
    labels, xv = _inputs(dev, g)
    out = m(labels, xv)
    B = labels.shape[0]
    assert tuple(out.shape) == (B, m.L, m.V) and out.dtype == torch.float32 and out.device == dev and not out.requires_grad
    assert m._tf_ctx.gemm_mode == mode and m._ctx is None                  # its own model object; the sampler's is never built
    lg = out.cpu().numpy()
    errs = dict(top=np.abs(_cols(lg, g["top_idx"]) - g["top_val"]).max(), rand=np.abs(_cols(lg, g["rand_idx"]) - g["rand_val"]).max(),
                rows=np.abs(np.stack([lg[b, t] for b, t in g["rows_bt"]]) - g["rows"]).max(),
                lse=np.abs(torch.logsumexp(out.double(), -1).cpu().numpy() - g["lse"]).max())
    print(name, mode, {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) <= LOGIT_TOL, errs
    safe = g["margin"] > 2 * LOGIT_TOL
    assert safe.mean() > 0.9
    am = torch.empty(B, m.L, dtype=torch.int64, device=dev)
    nll = torch.empty(B, m.L, dtype=torch.float32, device=dev)
    gt = torch.from_numpy(golden(str(g["encode"]))["ids"][:B]).to(dev)
    E.xent_stats(out, gt, m.patch_nums[-1] ** 2, torch.zeros(4, dtype=torch.float64, device=dev), nll_out=nll, argmax_out=am)
    assert np.array_equal(am.cpu().numpy()[safe], g["argmax"].astype(np.int64)[safe])
    assert np.abs(nll.cpu().numpy() - g["nll"]).max() <= 2 * LOGIT_TOL


@pytest.mark.parametrize("mode", ["f16x2", "bf16x3"])
def test_eval_ep_end_to_end(dev, mode):
    from sdvar_amd.evaluate import eval_ep
    from sdvar_amd.vqvae import VQVAE
    from sdvar_amd.weights import vae_state_dict
    g, ge = golden("tf_d4_256_stress"), golden_parts("encode_256")
    pns = tuple(int(p) for p in ge["patch_nums"])
    vae = VQVAE(vocab_size=4096, ch=160, v_patch_nums=pns).to(dev)
    vae.load_state_dict(vae_state_dict(pns, "perf", int(ge["wseed"]), with_encoder=True), strict=True)
    m = _var(dev, g, mode)
    m.train()                                                               # eval_ep switches to eval mode and back
    x = torch.from_numpy(ge["img_u8"]).float() / 127.5 - 1.0
    labels = torch.from_numpy(g["labels"])
    L_mean, L_tail, acc_mean, acc_tail, tot, sec = eval_ep(m, vae, [(x[i:i + 1], labels[i:i + 1]) for i in range(2)])
    assert m.training and tot == 2 and sec > 0
    want = g["stats"]
    print(mode, "eval_ep", (L_mean, L_tail, acc_mean, acc_tail), "reference", want.tolist())
    assert abs(L_mean - want[0]) <= 1e-3 and abs(L_tail - want[1]) <= 1e-3
    L, last_l = m.L, pns[-1] ** 2
    unsafe = int((g["margin"] <= 2 * LOGIT_TOL).sum()); unsafe_tail = int((g["margin"][:, -last_l:] <= 2 * LOGIT_TOL).sum())
    assert abs(round(acc_mean * L * tot / 100) - round(want[2] * L * tot / 100)) <= unsafe
    assert abs(round(acc_tail * last_l * tot / 100) - round(want[3] * last_l * tot / 100)) <= unsafe_tail


def test_fullwidth_d16_vs_oracle(dev):
    """d16 (C = 1024), 256^2, B = 2, stress init drawn on the device, all ten stages in one pass vs OracleVAR on the CPU."""
    from oracle import var_oracle as orc
    from sdvar_amd.ladder import LADDER_256
    from sdvar_amd.weights import var_state_dict_device
    from torch_ref_tf import tf_logits
    pns = LADDER_256
    sd = var_state_dict_device(16, pns, dev, mode="stress")
    g = dict(patch_nums=np.array(pns), depth=np.array(16), shared_aln=np.array(0), attn_l2_norm=np.array(1), labels=np.array([3, 977]),
             encode=np.array("encode_256"))
    m = _var(dev, g, None, sd=sd, strict=False)                           # the device init has no buffers; the constructor's are the reference's
    labels, xv = _inputs(dev, g)
    lg = m(labels, xv).cpu()
    if "d16" not in _MEMO:
        _MEMO["d16"] = tf_logits(orc.OracleVAR({k: v.cpu() for k, v in sd.items()}, 16, pns), labels.cpu(), xv.cpu())
    ref = _MEMO["d16"]
    top = ref.topk(8, dim=-1).indices
    rnd_idx = torch.from_numpy(np.random.Generator(np.random.Philox(key=[16, 5])).integers(0, m.V, size=(2, m.L, 8)))
    errs = [(lg.gather(-1, i) - ref.gather(-1, i)).abs().max().item() for i in (top, rnd_idx)]
    print("d16 full width: top-8 / random columns max|diff|", errs)
    assert max(errs) <= LOGIT_TOL


def test_condition_dropout(dev):
    g = golden("tf_d4_256_stress")
    m = _var(dev, g)
    _, xv2 = _inputs(dev, g)
    B = 8
    xv = xv2[torch.arange(B) % 2].contiguous()
    labels = torch.tensor([3, 977, 5, 6, 7, 8, 9, 10], device=dev)
    m.cond_drop_rate = 1.0
    a = m(labels, xv)
    m.cond_drop_rate = 0.0
    b = m(torch.full_like(labels, m.num_classes), xv)
    assert (a - b).abs().max().item() <= 1e-6
    seed = next(s for s in range(100) if (lambda u: 0 < int(u.sum()) < B)(torch.rand(B, generator=torch.Generator(dev).manual_seed(s), device=dev) < 0.5))
    m.cond_drop_rate = 0.5
    torch.manual_seed(seed)
    st0 = torch.cuda.get_rng_state(dev)
    c = m(labels, xv)
    st1 = torch.cuda.get_rng_state(dev)
    torch.cuda.set_rng_state(st0, dev)
    drop = torch.rand(B, device=dev) < 0.5
    assert torch.equal(torch.cuda.get_rng_state(dev), st1)               # forward drew exactly one rand(B)
    assert 0 < int(drop.sum()) < B
    m.cond_drop_rate = 0.0
    d = m(torch.where(drop, torch.full_like(labels, m.num_classes), labels), xv)
    assert (c - d).abs().max().item() <= 1e-6
    st2 = torch.cuda.get_rng_state(dev)
    m(labels, xv)                                                         # rate 0 still draws once (the reference's torch.rand(B))
    st3 = torch.cuda.get_rng_state(dev)
    torch.cuda.set_rng_state(st2, dev); torch.rand(B, device=dev)
    assert torch.equal(torch.cuda.get_rng_state(dev), st3) and not torch.equal(st2, st3)


def test_xent_stats_against_torch(dev):
    from sdvar_amd import engine as E
    B, L, V, tail = 3, 680, 4096, 256
    gen = torch.Generator().manual_seed(11)
    lg = torch.randn(B, L, V, generator=gen) * 3
    lg[0, 30:40, 17] = 50.0; lg[0, 30:40, 4000] = 50.0; lg[0, 30:40, 3] = 50.0     # ties at the maximum: lowest index wins
    lg[0, 41, :] = 1.25                                                                # a constant row
    lg[1, 5:25, ::3] = -float("inf")                                                   # -inf entries
    lg[1, 26, 1:] = -float("inf")                                                      # a row with one finite logit
    lg[2, 100:140] *= 1e4                                                              # rows scaled x 1e4
    tg = torch.randint(0, V, (B, L), generator=gen)
    tg[:, ::3] = lg.argmax(-1)[:, ::3]                                                 # a third of the tokens correct
    tg[1, 5:25] = 1                                                                    # finite targets in the -inf rows (index 1 is not a multiple of 3)
    tg[1, 26] = 0
    lgd, tgd = lg.to(dev), tg.to(dev)
    sums, nll, am = torch.zeros(4, dtype=torch.float64, device=dev), torch.empty(B, L, device=dev), torch.empty(B, L, dtype=torch.int64, device=dev)
    E.xent_stats(lgd, tgd, tail, sums, nll_out=nll, argmax_out=am)
    ref = F.cross_entropy(lg.double().view(-1, V), tg.view(-1), reduction="none").view(B, L)
    rel = ((nll.cpu().double() - ref).abs() / ref.abs().clamp_min(1.0)).max().item()
    assert rel <= 1e-5, rel
    assert torch.equal(am.cpu(), lg.argmax(-1))
    assert am[0, 30].item() == 3 and am[0, 41].item() == 0
    n64 = nll.cpu().double()
    cor = (am.cpu() == tg).double()
    want = torch.stack([n64.sum(), n64[:, -tail:].sum(), cor.sum(), cor[:, -tail:].sum()])
    s = sums.cpu()
    assert torch.equal(s[2:], want[2:]) and s[2].item() >= B * L // 3 - 40       # the -inf rows moved 7 of the argmax targets
    assert ((s[:2] - want[:2]).abs() / want[:2].abs()).max().item() <= 1e-12
    s2, nll2, am2 = torch.zeros_like(sums), torch.empty_like(nll), torch.empty_like(am)
    E.xent_stats(lgd, tgd, tail, s2, nll_out=nll2, argmax_out=am2)
    assert torch.equal(s2, sums) and torch.equal(nll2, nll) and torch.equal(am2, am)           # bit-identical runs
    E.xent_stats(lgd, tgd, tail, s2, accumulate=True)
    assert torch.equal(s2, sums + sums)
    bad = tgd.clone(); bad[0, 0] = V + 5; bad[2, L - 1] = -1
    E.xent_stats(lgd, bad, tail, s2, nll_out=nll2, argmax_out=am2)
    assert torch.isnan(nll2[0, 0]) and torch.isnan(nll2[2, L - 1]) and torch.isnan(s2[0]) and torch.isnan(s2[1])
    assert torch.equal(am2, am) and torch.isfinite(nll2[1]).all()


def xent_bound_c(V):
    """c of |nll_hip - nll_64| <= c 2^-24 max(1, |lse|, |x_t|) for sdvar_xent_stats (csrc/xent.hip), from its operation count, first order, u = 2^-24.
    The kernel forms s = sum_v exp(x_v - m), lse = m + log s, nll = lse - x_t.  Relative error of s (s >= 1, it holds the maximum's exp(0)), in units of u:
      10      the subtractions x_v - m: u |x_v - m| on each exponent, weighted by the term's share of s: sum_v p_v |x_v - m| <= ln V <= 10 for V <= 16384
       2      expf, 1 ulp = 2 u on every term
      R + 8   additions a term passes through: 2 inside its float4, at most R = ceil(V / 256) down its lane's running sum, 6 in the butterfly
      3 R + 2 the rescaling s <- s expf(m_old - m_new) of a lane's running sum, at most once per round: expf (2 u) and the product (u); its exponent's own
              rounding is weighted by what survives the rescaling, sum_j d_j exp(-(d_j + d_j+1 + ...)) <= 2
      26      six butterfly merges: both sides' expf and product (3 u), the sum (u), the exponents' roundings (<= 2 over all levels)
    That relative error of s is an absolute one of log s.  Then, in units of u max(1, |lse|, |x_t|):
      20      logf, 1 ulp of |log s| <= ln V <= 10 (not bounded by |lse| when m < 0): 2 u x 10
       3      m + log s (u |lse|), lse - x_t (u |nll| <= u (|lse| + |x_t|))
    c = 71 + 4 R."""
    return 71 + 4 * ((V + 255) // 256)


@pytest.mark.parametrize("V", [4, 1000, 4096, 16384])
@pytest.mark.parametrize("B,L,tail", [(1, 5, 0), (3, 7, 7), (2, 681, 3)])
def test_xent_stats_shapes_and_confident_rows(dev, V, B, L, tail):
    """sdvar_xent_stats against fp64 F.cross_entropy: V = 4 (one float4, 63 idle lanes), 1000 (a ragged last round of the 64 lanes), 4096, 16384 (64 rounds);
    B L = 5, 21, 1362 (none a multiple of the 4 rows per workgroup); tail = 0, tail = L and a short tail.  Every third row is confident: its target is the
    maximum at about +30 over logits of magnitude 30 and nll is about 1e-4 - the kernel computes (m + log s) - x_t, so its error there is absolute, a few
    ulp of 30.  Bound: xent_bound_c above (derived, not measured); torch's own float cross_entropy on the CPU must meet it on the same inputs."""
    from sdvar_amd import engine as E
    gen = torch.Generator().manual_seed(V + 7 * L)
    lg = torch.randn(B, L, V, generator=gen) * 3
    tg = torch.randint(0, V, (B, L), generator=gen)
    conf = torch.zeros(B, L, dtype=torch.bool)
    conf.view(-1)[::3] = True
    # confident rows: the target at 30, the V - 1 others around 30 - ln(1e4) - ln(V - 1), so that sum_{v != t} exp(x_v - 30) ~ 1e-4
    lo = 30.0 - np.log(1e4) - np.log(V - 1) + 0.3 * torch.randn(B, L, V, generator=gen)
    lg[conf] = lo[conf]
    lg.view(-1, V)[conf.view(-1), tg.view(-1)[conf.view(-1)]] = 30.0
    lgd, tgd = lg.to(dev), tg.to(dev)
    sums, nll, am = torch.zeros(4, dtype=torch.float64, device=dev), torch.empty(B, L, device=dev), torch.empty(B, L, dtype=torch.int64, device=dev)
    E.xent_stats(lgd, tgd, tail, sums, nll_out=nll, argmax_out=am)
    ref = F.cross_entropy(lg.double().view(-1, V), tg.view(-1), reduction="none").view(B, L)
    assert 0.5e-4 <= ref[conf].min().item() and ref[conf].max().item() <= 2e-4
    lse = torch.logsumexp(lg.double(), -1)
    xt = lg.double().gather(-1, tg.unsqueeze(-1)).squeeze(-1)
    bound = xent_bound_c(V) * 2.0 ** -24 * torch.maximum(torch.ones_like(lse), torch.maximum(lse.abs(), xt.abs()))
    err = (nll.cpu().double() - ref).abs()
    cpu32 = (F.cross_entropy(lg.view(-1, V), tg.view(-1), reduction="none").view(B, L).double() - ref).abs()
    print(f"xent V={V} B L={B * L} tail={tail}: max|err| {err.max().item():.2e} (confident rows {err[conf].max().item():.2e}; torch float on the CPU {cpu32.max().item():.2e}; "
          f"bound {bound.min().item():.2e} .. {bound.max().item():.2e})")
    assert (cpu32 <= bound).all()
    assert (err <= bound).all(), (err / bound).max().item()
    assert torch.equal(am.cpu(), lg.argmax(-1))
    n64 = nll.cpu().double()
    cor = (am.cpu() == tg).double()
    want = torch.stack([n64.sum(), n64[:, L - tail:].sum(), cor.sum(), cor[:, L - tail:].sum()])
    s = sums.cpu()
    assert torch.equal(s[2:], want[2:]) and s[2].item() >= conf.sum().item()
    assert ((s[:2] - want[:2]).abs() <= 1e-12 * want[:2].abs()).all()
    assert tail > 0 or (s[1].item() == 0.0 and s[3].item() == 0.0)
    assert tail < L or torch.equal(s[0::2], s[1::2])


def test_batching_over_passes(dev):
    g = golden("tf_d4_256_stress")
    m = _var(dev, g)
    P = m.tf_pass_images
    B = P + 1
    _, xv2 = _inputs(dev, g)
    xv = xv2[torch.arange(B) % 2].contiguous()
    labels = (torch.arange(B, device=dev) * 61) % 1001
    out = m(labels, xv)
    assert m._tf_ctx.max_batch == (P + 1) // 2
    worst = max((out[i] - m(labels[i:i + 1], xv[i:i + 1])[0]).abs().max().item() for i in range(B))
    assert worst <= LOGIT_TOL, worst


def test_sampling_unaffected_by_forward(dev):
    from sdvar_amd.weights import vae_state_dict
    g = golden("tf_d4_256_stress")
    m = _var(dev, g)
    pns = m.patch_nums
    vae = m.vae_proxy[0]
    vae.load_state_dict(vae_state_dict(pns, "stress", ch=32, with_encoder=False), strict=False)
    vae.to(dev)
    labels, xv = _inputs(dev, g)
    img1 = m.autoregressive_infer_cfg(2, labels, g_seed=5).clone(); ids1 = m.last_result.ids.clone()
    m(labels, xv)
    img2 = m.autoregressive_infer_cfg(2, labels, g_seed=5).clone(); ids2 = m.last_result.ids.clone()
    assert torch.equal(ids1, ids2) and torch.equal(img1, img2)
