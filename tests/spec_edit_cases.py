"""Shared inputs of the masked speculative-sampling tests (tests/test_spec_edit_host.py, tests/test_gpu_spec_edit_kernels.py, tests/test_gpu_spec_edit.py).
A plain helper module.

  * `masked_spec_decode`: the yardstick.  oracle.var_oracle.spec_decode's loop from the oracle's own parts, with
      - ids = where(gen, sampled, force_ids) after each draft sampling,
      - match masks and counts over the SAMPLED tokens only (a forced token is no draft prediction),
      - a stage without a sampled token accepted, every other stage by float32(matched) / float32(sampled) >= thr,
      - corrected ids equal to the forced ids at forced positions,
      - stats["sampled_tokens"], and corrected_tokens over sampled tokens.
    cfg / top_k / top_p may be per-image lists (the CFG factors rounded as the engine's tables round them).  With gen all ones and scalar parameters it is
    orc.spec_decode bit for bit (tests/test_spec_edit_host.py).  The reference has no masked sampler.
  * two kinds of margin are collected so that the GPU ids can be compared with no token excused:
      margins   per draft sampling: the smallest relative top-2 gap of p / q over the sampled tokens (a sampling tie),
      vmargins  per verification: over the sampled tokens whose draft id is the target's best or second-best CFG logit, the relative gap between those two
                logits - the only tokens whose top-1 verdict a rounding error could flip.
  * the cases and their seeds: the d4 draft -> d6 target `stress` pair on LADDER_256, B = 3, the masks / labels / forced ids of tests/edit_cases.py.  Each
    case's seed is the first from its start value whose run keeps both margins >= edit_cases.MIN_MARGIN; `pick_seeds()` recomputes them.
One oracle run costs 10 - 20 s of CPU; every run is cached with conftest.oracle_memo."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

import edit_cases as EC
from conftest import oracle_memo, state_dicts
from oracle import var_oracle as orc
from sdvar_amd.ladder import LADDER_256
from sdvar_amd.noise import exponential_noise

LAD = EC.LAD
DRAFT_DEPTH, TARGET_DEPTH = 4, 6
B = 3
PLAIN = (1.5, 900, 0.96)


@dataclass
class SpecTrace:
    ids: torch.Tensor              # (B, L)
    f_hat: torch.Tensor
    stats: Dict[str, object]
    margins: List[float] = field(default_factory=list)
    vmargins: List[float] = field(default_factory=list)


def _rows(v, n):
    return list(v) if isinstance(v, (list, tuple)) else [v] * n


def _cfg_combine(logits_2B: torch.Tensor, nB: int, ts: Sequence[float]) -> torch.Tensor:
    """var.py:199-200 per image: float32(1 + t_b) * cond - float32(t_b) * uncond, the two roundings of torch's scalar ops (and of the engine's factor table)."""
    opt = torch.tensor([np.float32(1.0 + t) for t in ts]).view(nB, 1, 1)
    tt = torch.tensor([np.float32(t) for t in ts]).view(nB, 1, 1)
    return opt * logits_2B[:nB] - tt * logits_2B[nB:]


def _sample(cl, top_k, top_p, q, g):
    """Per-image top-k / top-p sampling; (ids, the smallest relative top-2 gap of p / q over the tokens with g set, inf without any)."""
    nB, l, V = cl.shape
    q = q.view(nB, l, V)
    ids, masked = [], []
    for b in range(nB):
        i, m = orc.sample_topk_topp(cl[b:b + 1], top_k[b], top_p[b], q[b:b + 1])
        ids.append(i); masked.append(m)
    ids, masked = torch.cat(ids), torch.cat(masked)
    ratio = masked.softmax(dim=-1).view(-1, V) / q.view(-1, V)
    top2 = ratio.topk(2, dim=-1)[0]
    gap = ((top2[:, 0] - top2[:, 1]) / top2[:, 0]).view(nB, l)
    return ids, (float(gap[g].min()) if bool(g.any()) else float("inf"))


def _verdict_margin(ids, cl, g) -> float:
    top2v, top2i = cl.topk(2, dim=-1)
    near = g & ((ids == top2i[..., 0]) | (ids == top2i[..., 1]))
    if not bool(near.any()):
        return float("inf")
    gap = (top2v[..., 0] - top2v[..., 1]) / top2v[..., 0].abs().clamp_min(1e-30)
    return float(gap[near].min())


def _verdict_margin_topk(ids, cl, g, k: int) -> float:
    """The top-k rule holds iff fewer than k entries score strictly above the draft token.  A token that holds flips once the (k + 1)-th largest entry passes it, a
    token that does not once it passes the k-th largest: the gap to that entry, relative to the row's largest |logit| (the draft token's own score is near 0 at
    mid-rank), over the sampled tokens."""
    xd = cl.gather(-1, ids.unsqueeze(-1)).squeeze(-1)
    rank = (cl > xd.unsqueeze(-1)).sum(-1)
    srt = cl.sort(dim=-1, descending=True)[0]
    gap = torch.where(rank < k, xd - srt[..., k], srt[..., k - 1] - xd)
    return float((gap / cl.abs().amax(-1))[g].min()) if bool(g.any()) else float("inf")


def masked_spec_decode(draft: orc.OracleVAR, target: orc.OracleVAR, quant: orc.OracleQuant, label_B: torch.Tensor, cfg, gamma: int, top_k, top_p, noise,
                       gen: torch.Tensor, force_ids: torch.Tensor, thr: float = 0.5, match: Optional[orc.MatchRule] = None) -> SpecTrace:
    nB, S, pns = label_B.shape[0], draft.S, draft.patch_nums
    cfgs, tks, tps = _rows(cfg, nB), _rows(top_k, nB), _rows(top_p, nB)
    ts = lambda s: [c * (s / (S - 1)) for c in cfgs]
    gen = gen != 0
    d_cond, d_lvl, d_x = draft.prologue(label_B)
    t_cond, t_lvl, t_x = target.prologue(label_B)
    f_acc = torch.zeros(nB, draft.Cvae, pns[-1], pns[-1])
    draft.kv_reset(); target.kv_reset()
    cur, draw = 0, 0
    rule = match or orc.MatchRule()
    tr = SpecTrace(None, None, None)
    ids_acc: List[torch.Tensor] = []
    st = dict(target_calls=0, draft_stage_calls=0, forced_accepts=0, accepted_tokens=0, rounds=[], gamma_final=gamma)
    while cur < S:
        g = min(gamma, S - cur)
        ids_r, fh_r, dx_r, tx_r, dcl_r, gen_r = [], [], [d_x], [t_x], [], []
        f = f_acc
        for j in range(g):
            s = cur + j
            l, beg = pns[s] ** 2, LAD.begin(s)
            lg = draft.forward(dx_r[j], d_cond, s, 1)
            st["draft_stage_calls"] += 1
            cl = _cfg_combine(lg, nB, ts(s))
            gs = gen[:, beg:beg + l]
            sampled, mg = _sample(cl, tks, tps, noise(draw, nB, l, draft.V), gs); draw += 1
            tr.margins.append(mg)
            ids = torch.where(gs, sampled, force_ids[:, beg:beg + l])
            ids_r.append(ids); dcl_r.append(cl); gen_r.append(gs)
            f, nxt = quant.next_input(s, f, quant.embed_ids(ids, pns[s]))
            fh_r.append(f)
            if s + 1 < S:
                dx_r.append(draft.embed_next(nxt, d_lvl, s + 1)); tx_r.append(target.embed_next(nxt, t_lvl, s + 1))
        tl = target.forward(torch.cat(tx_r[:g], dim=1), t_cond, cur, g)
        st["target_calls"] += 1
        matched, total, corrected, n_acc, alive, off = [], [], [], 0, True, 0
        for j in range(g):
            n = pns[cur + j] ** 2
            cl = _cfg_combine(tl[:, off:off + n], nB, ts(cur + j)); off += n
            m = orc.token_matches(ids_r[j], cl, rule, dcl_r[j]) & gen_r[j]
            if rule.rule == "top1":
                tr.vmargins.append(_verdict_margin(ids_r[j], cl, gen_r[j]))
            elif rule.rule == "topk":
                tr.vmargins.append(_verdict_margin_topk(ids_r[j], cl, gen_r[j], rule.top_k))
            corrected.append(torch.where(gen_r[j] & ~m, torch.argmax(cl, dim=-1), ids_r[j]))
            matched.append(int(m.sum())); total.append(int(gen_r[j].sum()))
            ok = total[j] == 0 or float(np.float32(matched[j]) / np.float32(total[j])) >= thr
            if alive and ok:
                n_acc += 1
            else:
                alive = False
        forced, acc_tok = False, None
        if n_acc < g and rule.token_level:
            j = n_acc
            acc_tok = sum(pns[cur + i] ** 2 for i in range(j)) + matched[j]
            st["corrected_tokens"] = st.get("corrected_tokens", 0) + total[j] - matched[j]
            st["corrected_stages"] = st.get("corrected_stages", 0) + 1
            ids_r[j] = corrected[j]
            fh_r[j], nxt = quant.next_input(cur + j, f_acc if j == 0 else fh_r[j - 1], quant.embed_ids(ids_r[j], pns[cur + j]))
            if cur + j + 1 < S:
                dx, tx = draft.embed_next(nxt, d_lvl, cur + j + 1), target.embed_next(nxt, t_lvl, cur + j + 1)
                if len(dx_r) > j + 1:
                    dx_r[j + 1], tx_r[j + 1] = dx, tx
                else:
                    dx_r.append(dx); tx_r.append(tx)
            n_acc = j + 1
        elif n_acc == 0:
            if gamma > 1:
                gamma -= 1
            else:
                n_acc, forced = 1, True
                st["forced_accepts"] += 1
        st["rounds"].append(dict(stage=cur, g=g, matched=matched, total=total, n_accept=n_acc, forced=forced))
        if n_acc > 0:
            f_acc = fh_r[n_acc - 1]
            ids_acc.extend(ids_r[:n_acc])
            if not forced:
                st["accepted_tokens"] += sum(pns[cur + j] ** 2 for j in range(n_acc)) if acc_tok is None else acc_tok
            cur += n_acc
            if cur < S:
                d_x, t_x = dx_r[n_acc], tx_r[n_acc]
        keep_len = draft.begin(cur) if cur < S else draft.L
        draft.kv_truncate(keep_len); target.kv_truncate(keep_len)
    st["gamma_final"] = gamma
    st["sampled_tokens"] = int(gen.sum())
    draft.kv_reset(); target.kv_reset()
    tr.ids, tr.f_hat, tr.stats = torch.cat(ids_acc, 1), f_acc, st
    return tr


# ------------------------------------------------------------------------------------------------ the cases and their seeds
@dataclass(frozen=True)
class SpecCase:
    gamma: int
    thr: float
    start: int                     # where pick_seeds() starts looking
    seed: object                   # the committed seed: an int (image b at Philox image counter b), or one per image (each at counter 0)
    token_level: bool = False
    cfg: object = PLAIN[0]
    top_k: object = PLAIN[1]
    top_p: object = PLAIN[2]
    masks: tuple = EC.MASKS3       # names in edit_cases.masks(256), one per image
    rule: str = "top1"
    rule_k: int = 1

    def match(self, mod=orc):
        """The case's MatchRule, the oracle's or (mod = sdvar_amd.engine) the engine's."""
        return mod.MatchRule(rule=self.rule, top_k=self.rule_k, token_level=self.token_level)

    @property
    def rows(self) -> bool:
        return isinstance(self.seed, tuple)


ROW_PARAMS = dict(cfg=(1.5, 3.0, 0.75), top_k=(900, 0, 40), top_p=(0.96, 0.0, 0.5))          # image 1 with top-k and top-p off
CASES: Dict[str, SpecCase] = {
    "g1_t0": SpecCase(1, 0.0, 1000, 1000),
    "g2_t0": SpecCase(2, 0.0, 1100, 1100),
    "g1_t5": SpecCase(1, 0.5, 1200, 1200),
    "g2_t5": SpecCase(2, 0.5, 1300, 1300),
    "token_level": SpecCase(2, 0.5, 1400, 1400, token_level=True),
    "rows": SpecCase(2, 0.5, 1500, (1501, 2501, 3501), **ROW_PARAMS),
    # three small holes: stages 0 and 1 hold no sampled token in any image, so the first round is accepted in full without a single verdict, and the next one is not
    "holes": SpecCase(2, 0.5, 1600, 1600, masks=("hole", "hole", "hole")),
    # the two random-weight models never agree on a top-1 token; under the top-k membership rule at half the vocabulary about half the sampled tokens match,
    # so stages pass and fail by their sampled tokens' rate (three small holes: with few sampled tokens a seed exists that keeps every verdict clear of the
    # dense mid-rank boundary)
    "topk": SpecCase(2, 0.5, 1700, 1705, rule="topk", rule_k=2048, masks=("hole", "hole", "hole")),
}


def case_seed(c: SpecCase, k: int):
    """The k-th candidate seed of a case (k = 0: its start value); a per-image case moves its three seeds together."""
    return tuple(c.start + k + 1000 * b for b in range(B)) if c.rows else c.start + k


def noise_fn(seed):
    if isinstance(seed, tuple):
        return orc.array_noise(lambda d, B_, l, V_: np.concatenate([exponential_noise(s, d, 1, l, V_, 0) for s in seed]))
    return orc.array_noise(lambda d, B_, l, V_: exponential_noise(seed, d, B_, l, V_, 0))


def oracles():
    sd4, sdv = state_dicts(DRAFT_DEPTH, LADDER_256)
    sd6, _ = state_dicts(TARGET_DEPTH, LADDER_256)
    return oracle_memo(("spec_edit_oracles",), lambda: (orc.OracleVAR(sd4, DRAFT_DEPTH, LADDER_256), orc.OracleVAR(sd6, TARGET_DEPTH, LADDER_256),
                                                        orc.OracleQuant(sdv, LADDER_256)))


def as_list(v):
    return list(v) if isinstance(v, tuple) else v


def oracle_run(name: str, seed=None) -> SpecTrace:
    c = CASES[name]
    seed = c.seed if seed is None else seed

    def run():
        d, t, q = oracles()
        return masked_spec_decode(d, t, q, torch.tensor(EC.LABELS3), as_list(c.cfg), c.gamma, as_list(c.top_k), as_list(c.top_p), noise_fn(seed), EC.gen_table(c.masks),
                                  EC.random_ids(B), c.thr, c.match())
    return oracle_memo(("spec_edit_run", name, seed), run)


def clear(tr: SpecTrace) -> bool:
    return min(tr.margins) >= EC.MIN_MARGIN and min(tr.vmargins) >= EC.MIN_MARGIN


def pick_seeds(tries: int = 40, names: Sequence[str] = tuple(CASES)) -> Dict[str, object]:
    out = {}
    for name in names:
        for k in range(tries):
            if clear(oracle_run(name, case_seed(CASES[name], k))):
                out[name] = case_seed(CASES[name], k)
                break
        else:
            raise RuntimeError(f"no seed with both margins >= {EC.MIN_MARGIN} for {name}")
    return out
