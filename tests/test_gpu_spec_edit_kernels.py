"""GPU: the acceptance launches with forced tokens (sdvar_verify_accept_forced / sdvar_verify_accept_rows_forced, csrc/sampler.hip) against a numpy
restatement, every output inside guard canaries.  B = 2, chunks of stage lengths (1, 4, 9) and (4,), V = 12 (most lanes hold only padding) and V = 4096.
The logits are small integers, tie-free per row after the CFG combine (cond in multiples of 4, uncond in {0, 1}, t in {0, 0.5, 1}: every product and difference
is exact in fp32), so every verdict is exact; one case holds an exact argmax tie (the smallest index wins).  A forced token must add nothing to any counter, read
as match 1 / corrected = the draft id / argmax -1 in the optional outputs, and a stage without a sampled token must be accepted."""
import numpy as np
import pytest
import torch

from sdvar_amd import engine as E

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
B = 2
IDS_STRIDE, IDS_OFF = 31, 5          # draft ids at ids[b * IDS_STRIDE + IDS_OFF + tok]
GEN_STRIDE, GEN_OFF = 23, 2          # gen at gen[b * GEN_STRIDE + GEN_OFF + tok]: another stride than the ids'
SENT = -7
RULES = {"top1": E.MatchRule(), "topk": E.MatchRule("topk", top_k=3), "kl": E.MatchRule("kl", kl_thr=0.5)}
T_STAGE = (0.0, 0.5, 1.0)            # scalar launches: t of stage j of the chunk
T_IMAGE = ((0.0, 1.0), (0.5, 0.0), (1.0, 0.5))          # rows launches: t of (stage j, image b)


class _Guarded:
    """A device tensor inside a larger buffer of sentinels: whatever a kernel writes outside its output is seen."""

    def __init__(self, dev, shape, dtype, fill, pad=64):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev)
        self.view = self.buf[pad:pad + n].view(*shape)
        self.fill, self.pad, self.n = fill, pad, n

    def intact(self):
        return bool((self.buf[:self.pad] == self.fill).all()) and bool((self.buf[self.pad + self.n:] == self.fill).all())


# ------------------------------------------------------------------------------------------------ inputs
def _stage_of(lens):
    return np.concatenate([np.full(l, j) for j, l in enumerate(lens)])


def _factors(lens, rows):
    """(n, B, 2) float32 {float32(1 + t), float32(t)} of (stage j, image b)."""
    t = np.array([[T_IMAGE[j][b] if rows else T_STAGE[j] for b in range(B)] for j in range(len(lens))], np.float64)
    return np.stack([(1.0 + t).astype(np.float32), t.astype(np.float32)], -1), t


def _combine(lg, lens, fac):
    """x (B, lsum, V) float32 = fl(fl(opt * cond) - fl(t * uncond))."""
    st = _stage_of(lens)
    opt, tt = fac[st][..., 0].T[:, :, None], fac[st][..., 1].T[:, :, None]          # (B, lsum, 1)
    return ((opt * lg[:B]).astype(np.float32) - (tt * lg[B:]).astype(np.float32)).astype(np.float32)


def _logits(V, lsum, key, tie=False):
    g = np.random.Generator(np.random.Philox(key=[V, key]))
    cond = np.stack([g.permutation(V) for _ in range(B * lsum)]).reshape(B, lsum, V).astype(np.float32) * 4.0
    unc = g.integers(0, 2, size=(B, lsum, V)).astype(np.float32)
    if tie:          # rows (b, 0): the two best entries of cond made equal, uncond zero there: an exact tie of the CFG logits whatever t is
        for b in range(B):
            order = np.argsort(-cond[b, 0])
            cond[b, 0, order[1]] = cond[b, 0, order[0]]
            unc[b, 0, order[:2]] = 0.0
    return np.concatenate([cond, unc]).astype(np.float32)


def _draft_ids(x):
    """(tok + b) % 3 == 0: the argmax (smallest index on a tie); 1: the second best (a top-k match, a top-1 miss); 2: the worst entry."""
    Bn, lsum, V = x.shape
    order = np.argsort(-x, axis=-1, kind="stable")
    ids = np.empty((Bn, lsum), np.int64)
    for b in range(Bn):
        for i in range(lsum):
            ids[b, i] = order[b, i, (0, 1, V - 1)[(i + b) % 3]]
    return ids


def _draft_logits(lg, lens):
    """The KL rule's draft logits, stage j as (2B, l_j, V) at element offset 2 B V qbeg_j: the target's own rows where (tok + b) is even (KL exactly 0), the
    rows reversed along V elsewhere (the draft's peak sits on the target's worst entry: KL in the thousands)."""
    lsum, V = lg.shape[1], lg.shape[2]
    d = lg.copy()
    for b in range(B):
        for i in range(lsum):
            if (i + b) % 2:
                d[b, i] = lg[b, i, ::-1]; d[B + b, i] = lg[B + b, i, ::-1]
    out, off = [], 0
    for l in lens:
        out.append(d[:, off:off + l].reshape(-1)); off += l
    return np.concatenate(out), d


def _reference(lg, ids, gen, lens, fac, thr, rule, dl_full=None):
    """numpy restatement of the forced launches: (counts (40,), argmax, match, corrected)."""
    x = _combine(lg, lens, fac)
    Bn, lsum, V = x.shape
    st = _stage_of(lens)
    am = np.argmax(x, -1)                                                        # the first maximum: the smallest index
    if rule.rule == "top1":
        m = am == ids
    elif rule.rule == "topk":
        xd = np.take_along_axis(x, ids[..., None], -1)
        m = (x > xd).sum(-1) < rule.top_k
    else:
        xdr = _combine(dl_full, lens, fac).astype(np.float64)
        x64 = x.astype(np.float64)
        lt = x64 - x64.max(-1, keepdims=True); lt -= np.log(np.exp(lt).sum(-1, keepdims=True))
        ld = xdr - xdr.max(-1, keepdims=True); ld -= np.log(np.exp(ld).sum(-1, keepdims=True))
        p = np.exp(lt)
        m = np.where(p > 0, p * (lt - ld), 0.0).sum(-1) <= float(np.float32(rule.kl_thr))
    g = gen != 0
    counts = np.zeros(40, np.int32)
    for j in range(len(lens)):
        counts[j] = int((m & g)[:, st == j].sum()); counts[17 + j] = int(g[:, st == j].sum())
    n, alive = 0, True
    for j in range(len(lens)):
        ok = counts[17 + j] == 0 or float(np.float32(counts[j]) / np.float32(counts[17 + j])) >= thr
        if alive and ok:
            n += 1
        else:
            alive = False
    counts[16] = n
    return counts, np.where(g, am, -1), np.where(g, m, True).astype(np.uint8), np.where(g & ~m, am, ids)


def _patterns(lens):
    lsum, st = sum(lens), _stage_of(lens)
    alt = ((np.arange(lsum)[None] + np.arange(B)[:, None]) % 2).astype(np.uint8)          # every token index sampled in one image and forced in the other
    out = {"ones": np.ones((B, lsum), np.uint8), "zeros": np.zeros((B, lsum), np.uint8), "alternating": alt * 200}          # any non-zero byte means "sampled"
    one = np.ones((B, lsum), np.uint8); one[1] = 0
    out["image_forced"] = one
    if len(lens) > 1:
        for name, j in (("empty_front", 0), ("empty_middle", 1), ("empty_back", len(lens) - 1)):
            g = np.ones((B, lsum), np.uint8); g[:, st == j] = 0
            g[0, (st != j).nonzero()[0][::3]] = 0                               # ... and some forced tokens in the stages that keep sampled ones
            out[name] = g
    return out


def _launch(dev, lg, ids, lens, fac, t, rows, thr, rule, gen=None, dl=None):
    """One launch, forced (gen (B, lsum) given) or the unforced twin; every output in canaries.  Returns host (counts, argmax, match, corrected)."""
    lsum, V = lg.shape[1], lg.shape[2]
    counts = _Guarded(dev, (40,), torch.int32, SENT)
    am = _Guarded(dev, (B, lsum), torch.int64, SENT); mo = _Guarded(dev, (B, lsum), torch.uint8, 99); co = _Guarded(dev, (B, lsum), torch.int64, SENT)
    idt = torch.full((B, IDS_STRIDE), -(2 ** 40), dtype=torch.int64)               # an id no vocabulary holds around the chunk: reading it instead would show
    idt[:, IDS_OFF:IDS_OFF + lsum] = torch.from_numpy(ids)
    idt = idt.to(dev)
    tab = None
    if rows:
        img = np.zeros(B, E.ROW_IMAGE_DTYPE)
        tab = E.RowParams.from_tables(fac, img, dev)
    kw = {}
    if gen is not None:
        gt = torch.zeros(B, GEN_STRIDE, dtype=torch.uint8)
        gt[:, GEN_OFF:GEN_OFF + lsum] = torch.from_numpy(gen)
        gt[:, :GEN_OFF] = torch.from_numpy(1 - (gen[:, :1] != 0)).expand(B, GEN_OFF)          # the neighbours say the opposite of the first token
        kw = dict(gen=gt.to(dev), gen_off=GEN_OFF, gen_stride=GEN_STRIDE)
    dld = None if dl is None else torch.from_numpy(dl).to(dev)
    E.verify_accept(torch.from_numpy(lg).to(dev), B, list(lens), V, [float(x) for x in t[:, 0]], idt, IDS_OFF, IDS_STRIDE, thr, counts.view, argmax_out=am.view,
                    rule=rule, draft_logits=dld, match_out=mo.view, corrected_out=co.view, rows=tab, s0=0, **kw)
    torch.cuda.synchronize()
    assert counts.intact() and am.intact() and mo.intact() and co.intact(), "a guard byte around an output was written"
    return counts.view.cpu().numpy(), am.view.cpu().numpy(), mo.view.cpu().numpy(), co.view.cpu().numpy()


def _case(V, lens, rows, tie=False):
    lg = _logits(V, sum(lens), 10 * len(lens) + int(rows), tie)
    fac, t = _factors(lens, rows)
    ids = _draft_ids(_combine(lg, lens, fac))
    dl, dl_full = _draft_logits(lg, lens)
    return lg, fac, t, ids, dl, dl_full


def _same(got, want, what):
    for name, g, w in zip(("counts", "argmax_out", "match_out", "corrected_out"), got, want):
        assert np.array_equal(g, w), f"{what}: {name} differs\n got  {g}\n want {w}"


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("rows", [False, True], ids=["scalar", "rows"])
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("lens", [(1, 4, 9), (4,)], ids=["chunk149", "chunk4"])
@pytest.mark.parametrize("V", [12, 4096])
def test_forced_launch_is_the_numpy_restatement(dev, V, lens, rule, rows):
    """Every gen pattern (a stage with no sampled token in front of, between and after stages with some; one image fully forced; all ones; all zeros) at two
    thresholds: counters, n_accept and the three optional outputs, forced positions included."""
    lg, fac, t, ids, dl, dl_full = _case(V, lens, rows)
    r = RULES[rule]
    for pname, gen in _patterns(lens).items():
        for thr in (0.5, 0.3):
            want = _reference(lg, ids, gen, lens, fac, thr, r, dl_full)
            got = _launch(dev, lg, ids, lens, fac, t, rows, thr, r, gen, dl if rule == "kl" else None)
            _same(got, want, f"V={V} lens={lens} {rule} {pname} thr={thr}")
            f = gen == 0
            assert (got[1][f] == -1).all() and (got[2][f] == 1).all() and np.array_equal(got[3][f], ids[f])
    if len(lens) > 1 and rule == "top1":                                     # the patterns do what their names say
        c = _reference(lg, ids, _patterns(lens)["empty_middle"], lens, fac, 0.3, r)[0]
        assert c[18] == 0 and c[17] > 0 and c[19] > 0


@pytest.mark.parametrize("rows", [False, True], ids=["scalar", "rows"])
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("V", [12, 4096])
def test_all_ones_gen_is_the_unforced_entry_point(dev, V, rule, rows):
    lens = (1, 4, 9)
    lg, fac, t, ids, dl, _ = _case(V, lens, rows)
    r, d = RULES[rule], (dl if rule == "kl" else None)
    for thr in (0.0, 0.3, 0.5, 2.0):
        base = _launch(dev, lg, ids, lens, fac, t, rows, thr, r, None, d)
        ones = _launch(dev, lg, ids, lens, fac, t, rows, thr, r, np.ones((B, sum(lens)), np.uint8), d)
        _same(ones, base, f"V={V} {rule} thr={thr}")
        assert list(base[0][17:20]) == [B * l for l in lens]
    again = _launch(dev, lg, ids, lens, fac, t, rows, 2.0, r, np.ones((B, sum(lens)), np.uint8), d)
    _same(again, ones, "a repeat")                                            # integer counters: bit-identical


@pytest.mark.parametrize("rows", [False, True], ids=["scalar", "rows"])
@pytest.mark.parametrize("lens", [(1, 4, 9), (4,)], ids=["chunk149", "chunk4"])
def test_all_zeros_gen_accepts_every_stage_at_any_threshold(dev, lens, rows):
    lg, fac, t, ids, _, _ = _case(12, lens, rows)
    c, am, mo, co = _launch(dev, lg, ids, lens, fac, t, rows, 2.0, RULES["top1"], np.zeros((B, sum(lens)), np.uint8))
    assert c[16] == len(lens) and not c[:16].any() and not c[17:].any()
    assert (am == -1).all() and (mo == 1).all() and np.array_equal(co, ids)


@pytest.mark.parametrize("rows", [False, True], ids=["scalar", "rows"])
@pytest.mark.parametrize("V", [12, 4096])
def test_exact_argmax_tie_takes_the_smallest_index(dev, V, rows):
    lens = (1, 4, 9)
    lg, fac, t, ids, _, _ = _case(V, lens, rows, tie=True)
    x = _combine(lg, lens, fac)
    for b in range(B):
        top = np.sort(x[b, 0])[-2:]
        assert top[0] == top[1], "the constructed tie is gone"
    lo = np.argmax(x[:, 0], -1)
    hi = np.array([np.flatnonzero(x[b, 0] == x[b, 0].max())[1] for b in range(B)])
    assert (lo < hi).all()
    ids = ids.copy(); ids[0, 0], ids[1, 0] = lo[0], hi[1]                        # image 0 drafts the smaller index (a match), image 1 the larger (a miss)
    gen = np.ones((B, sum(lens)), np.uint8); gen[:, 3::4] = 0
    want = _reference(lg, ids, gen, lens, fac, 0.5, RULES["top1"])
    got = _launch(dev, lg, ids, lens, fac, t, rows, 0.5, RULES["top1"], gen)
    _same(got, want, f"tie V={V}")
    assert got[0][0] == 1 and got[0][17] == 2 and got[2][0, 0] == 1 and got[2][1, 0] == 0 and got[3][1, 0] == lo[1] and got[1][1, 0] == lo[1]


def test_wrapper_refuses_a_gen_table_that_does_not_fit(dev):
    lens = (4,)
    lg, fac, t, ids, _, _ = _case(12, lens, False)
    counts = torch.zeros(40, dtype=torch.int32, device=dev)
    idt = torch.zeros(B, 4, dtype=torch.int64, device=dev)
    lgd = torch.from_numpy(lg).to(dev)
    with pytest.raises(E.SdvarError, match="stride"):
        E.verify_accept(lgd, B, list(lens), 12, [0.0], idt, 0, 4, 0.5, counts, gen=torch.ones(B, 4, dtype=torch.uint8, device=dev), gen_off=2, gen_stride=4)
    with pytest.raises(E.SdvarError, match="gen"):
        E.verify_accept(lgd, B, list(lens), 12, [0.0], idt, 0, 4, 0.5, counts, gen=torch.ones(B, 4, dtype=torch.int64, device=dev), gen_off=0, gen_stride=4)
    with pytest.raises(E.SdvarError, match="gen"):
        E.verify_accept(lgd, B, list(lens), 12, [0.0], idt, 0, 4, 0.5, counts, gen=torch.ones(1, 4, dtype=torch.uint8, device=dev), gen_off=0, gen_stride=4)
    with pytest.raises(E.SdvarError, match="gen is on cpu"):
        E.verify_accept(lgd, B, list(lens), 12, [0.0], idt, 0, 4, 0.5, counts, gen=torch.ones(B, 4, dtype=torch.uint8), gen_off=0, gen_stride=4)
