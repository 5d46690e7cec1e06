"""Hard inputs and references for the sampler and acceptance kernels of csrc/sampler.hip (cfg_sample, gumbel_mix, verify_match + accept_scan,
cfg_combine).  A plain helper module: tests/test_sampler_hard_host.py checks the references against each other on the CPU, tests/test_gpu_sampler_hard.py
checks the kernels against them.  Every input is generated from a seed (numpy Philox); nothing here touches a GPU.

Two references for cfg_sample:
  R1  oracle.var_oracle.sample_topk_topp on orc.cfg_combine: the reference's arithmetic in torch fp32.  Its torch.sort is not stable, so WHICH of several
      equal values survives the top-p cut is an accident of torch's sort; only the number kept and the kept values are meaningful on a tied row.
  R2  `r2` below, float64: top-k by value, ascending stable sort (equal values go by index; -0.0 and +0.0 count as equal in the ordering only), softmax and
      running sum in float64, entry removed iff cumsum <= float32(1 - top_p), last entry always kept.  This is the kernel's documented rule.
A row is set-ambiguous when its top-p margin (min over the sorted positions but the last of |cumsum - thr|) is <= 8 * 2^-24: the kernel and torch round each
probability, the row sum and the running sum to float32 on values <= 1 (each rounding <= 2^-24), 8 is the margin over these three.  A row is draw-ambiguous
when the relative gap between the two largest p/q is <= 1e-5.

One deviation from a literal reading of "-inf at the same places in the cond and uncond halves": (1+t)*(-inf) - t*(-inf) is NaN for every t (and 0*(-inf) is
NaN at t = 0), in torch as in the kernel, and NaN logits are out of scope.  The `inf` family therefore puts its -inf into the cond half only, which is what
makes the CFG logits -inf (test_sampler_hard_host.py pins the NaN statement)."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from oracle import var_oracle as orc
from sdvar_amd.noise import exponential_noise

AMBIG_SET = 8 * 2.0 ** -24
AMBIG_DRAW = 1e-5
NEG_INF = float("-inf")
CONSTRUCTED = ("peak", "quant", "equal", "zeros", "ties")          # families whose set-ambiguity cap is 0 (so is every top_k = 1 case)


@dataclass(frozen=True)
class Case:
    name: str
    family: str            # gauss | peak | heavy | quant | equal | inf | zeros | bound | ties
    V: int
    t: float
    top_k: int
    top_p: float
    seed: int
    B: int = 2
    l: int = 16
    param: Optional[Tuple[int, int]] = None

    @property
    def rows(self) -> int:
        return self.B * self.l

    @property
    def set_cap(self) -> int:
        """Most set-ambiguous rows the case may hold: 0 for constructed families, 5 % of the rows for random-continuous ones."""
        return 0 if (self.family in CONSTRUCTED or self.top_k == 1) else int(0.05 * self.rows)

    @property
    def draw_cap(self) -> int:
        return int(0.01 * self.rows)


def _c(name, family, V, t, top_k, top_p, seed, l=16, param=None):
    return Case(name, family, V, t, top_k, top_p, seed, 2, l, param)


RANDOM_4096 = [
    _c("g4096_k900", "gauss", 4096, 1.5, 900, 0.96, 1, l=32),
    _c("g4096_full", "gauss", 4096, 0.0, 0, 0.9, 2, l=32),
    _c("g4096_kV", "gauss", 4096, 1.5, 4096, 0.5, 3),
    _c("g4096_k40", "gauss", 4096, 0.0, 40, 0.0, 4),
    _c("g4096_none", "gauss", 4096, 1.5, 0, 0.0, 5),
    _c("g4096_k1", "gauss", 4096, 1.5, 1, 0.96, 6),
    _c("g4096_p_near1", "gauss", 4096, 0.0, 900, 0.999, 7, l=32),              # t = 0: at t = 1.5 the lowest survivors' probabilities are below the margin itself
    _c("g4096_p_near0_compact", "gauss", 4096, 0.0, 900, 1e-8, 8, l=32),      # thr rounds to 1.0f: only the "last entry always kept" rule leaves a token
    _c("g4096_p_near0_full", "gauss", 4096, 1.5, 0, 1e-8, 9),
    _c("heavy4096_k900", "heavy", 4096, 1.5, 900, 0.96, 10),
    _c("heavy4096_full", "heavy", 4096, 1.5, 0, 0.9, 11),
    _c("heavy4096_t0", "heavy", 4096, 0.0, 900, 0.96, 12),
    _c("inf4096_k900", "inf", 4096, 1.5, 900, 0.96, 13),
    _c("inf4096_full", "inf", 4096, 0.0, 0, 0.9, 14),
    _c("b1024", "bound", 4096, 0.0, 1024, 0.96, 15),
    _c("b1025", "bound", 4096, 1.5, 1025, 0.96, 16),
]
CONSTRUCTED_4096 = [
    _c("peak4096_k900", "peak", 4096, 1.5, 900, 0.96, 21),
    _c("peak4096_k1", "peak", 4096, 0.0, 1, 0.96, 22),
    _c("peak4096_full", "peak", 4096, 1.5, 0, 0.9, 23),
    _c("quant4096_k900", "quant", 4096, 0.0, 900, 0.96, 24),
    _c("quant4096_full", "quant", 4096, 1.5, 0, 0.9, 25),
    _c("quant4096_k40", "quant", 4096, 1.5, 40, 0.0, 26),
    _c("quant4096_kV", "quant", 4096, 0.0, 4096, 0.5, 27),
    _c("equal4096_full", "equal", 4096, 0.0, 0, 0.96, 28),
    _c("equal4096_k900", "equal", 4096, 1.5, 900, 0.96, 29),
    _c("zeros4096_compact", "zeros", 4096, 0.0, 900, 0.96, 30, param=(499, 450)),       # (positives, zeros): the 900th value is a zero, 949 survivors
    _c("zeros4096_full", "zeros", 4096, 0.0, 900, 0.96, 31, param=(600, 1200)),         # 1800 survivors: the full sort
    _c("zeros4096_nok", "zeros", 4096, 0.0, 0, 0.9, 32, param=(600, 1200)),
    _c("ties900_full", "ties", 4096, 0.0, 900, 0.96, 35, param=(850, 1100)),            # ranks 850..1099 tied at the 900th value: 1100 survivors
    _c("ties900_compact", "ties", 4096, 0.0, 900, 0.96, 34, param=(880, 1000)),         # 1000 survivors: ties in the compact sort
]
V1000 = [
    _c("g1000_k900", "gauss", 1000, 1.5, 900, 0.96, 41, l=32),
    _c("g1000_full", "gauss", 1000, 0.0, 0, 0.9, 42, l=32),
    _c("g1000_none", "gauss", 1000, 1.5, 0, 0.0, 43),
    _c("g1000_k40", "gauss", 1000, 0.0, 40, 0.0, 44),
    _c("heavy1000_kV", "heavy", 1000, 1.5, 1000, 0.5, 45),
    _c("heavy1000_k900", "heavy", 1000, 1.5, 900, 0.96, 46),
    _c("inf1000_full", "inf", 1000, 0.0, 0, 0.9, 47),
    _c("inf1000_k900", "inf", 1000, 1.5, 900, 0.96, 48),                                 # 667 finite entries < top_k: the k-th value is -inf
    _c("peak1000_k1", "peak", 1000, 1.5, 1, 0.96, 49),
    _c("peak1000_k900", "peak", 1000, 0.0, 900, 0.96, 50),
    _c("quant1000_k900", "quant", 1000, 1.5, 900, 0.96, 51),
    _c("quant1000_k40", "quant", 1000, 0.0, 40, 0.0, 52),
    _c("equal1000", "equal", 1000, 0.0, 0, 0.9005, 53),                                  # 0.96 / 0.9 would sit on the threshold (40 * 0.001): margin 5e-4 here
    _c("zeros1000", "zeros", 1000, 0.0, 900, 0.96, 54, param=(700, 250)),
]
SMALL_V = [
    _c("g8_full", "gauss", 8, 1.5, 0, 0.9, 61),
    _c("g8_k900", "gauss", 8, 0.0, 900, 0.96, 62),                                       # top_k > V: no top-k
    _c("g8_none", "gauss", 8, 1.5, 0, 0.0, 63),
    _c("quant8_kV", "quant", 8, 0.0, 8, 0.5, 64),
    _c("quant8_k40", "quant", 8, 1.5, 40, 0.0, 65),
    _c("equal8", "equal", 8, 0.0, 0, 0.55, 66),
    _c("peak8_k1", "peak", 8, 1.5, 1, 0.96, 67),
    _c("inf8_full", "inf", 8, 1.5, 0, 0.9, 68),
    _c("zeros8", "zeros", 8, 0.0, 8, 0.5, 69, param=(1, 6)),
    _c("heavy8_full", "heavy", 8, 1.5, 0, 0.9, 70),
    _c("g4_full", "gauss", 4, 1.5, 0, 0.9, 71),
    _c("g4_k1", "gauss", 4, 0.0, 1, 0.96, 72),
    _c("quant4_kV", "quant", 4, 0.0, 4, 0.5, 73),
    _c("equal4", "equal", 4, 0.0, 0, 0.6, 74),
    _c("peak4_k900", "peak", 4, 1.5, 900, 0.96, 75),
    _c("inf4_full", "inf", 4, 0.0, 0, 0.9, 76),
]
GROUPS = {"random4096": RANDOM_4096, "constructed4096": CONSTRUCTED_4096, "v1000": V1000, "small": SMALL_V}
ALL_CASES = [c for g in GROUPS.values() for c in g]
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES) and all(len(g) <= 16 for g in GROUPS.values()) and all(32 <= c.rows <= 128 for c in ALL_CASES)


# ------------------------------------------------------------------------------------------------ row generators
def _rng(seed: int, stream: int = 7001):
    return np.random.Generator(np.random.Philox(key=[seed, stream]))


def _distinct(a: np.ndarray) -> np.ndarray:
    """Make the values of every row of a (R, V) float32 array pairwise distinct, moving a duplicate up to the next float."""
    a = a.copy()
    for r in range(a.shape[0]):
        order = np.argsort(a[r], kind="stable")
        s = a[r][order]
        while True:
            dup = np.nonzero(s[1:] <= s[:-1])[0]
            if dup.size == 0:
                break
            s[dup + 1] = np.nextafter(s[dup], np.float32(np.inf))
        a[r][order] = s
    return a


def make_logits(c: Case) -> torch.Tensor:
    """The raw (2B, l, V) float32 logits of a case (cond half first)."""
    g, B, l, V = _rng(c.seed), c.B, c.l, c.V
    R = B * l
    gauss = lambda scale: (g.standard_normal(size=(2 * B, l, V), dtype=np.float32) * np.float32(scale))
    if c.family == "gauss":
        lg = gauss(2.5)
    elif c.family == "peak":                   # unit-scale rows: the +25 entry then holds all but ~1e-5 of the mass at t = 0 and t = 1.5 alike
        lg = gauss(1.0)
        j = g.integers(0, V, size=(B, l))
        for h in (0, B):
            np.put_along_axis(lg[h:h + B], j[..., None], np.take_along_axis(lg[h:h + B], j[..., None], -1) + np.float32(25), -1)
    elif c.family == "heavy":
        lg = np.clip(g.standard_cauchy(size=(2 * B, l, V)) * 2.0, -1e4, 1e4).astype(np.float32)
    elif c.family == "quant":                  # multiples of 0.5 in both halves: the CFG values are exact multiples of 0.25, tied in dozens
        lg = (np.round(gauss(2.5) * 2) / 2).astype(np.float32)
    elif c.family == "equal":
        lg = np.full((2 * B, l, V), 1.25, dtype=np.float32)
    elif c.family == "inf":                    # a third of every cond row at -inf (see the module docstring for why not the uncond row as well)
        lg = gauss(2.5)
        for r in range(R):
            lg[:B].reshape(R, V)[r, g.permutation(V)[:max(1, V // 3)]] = -np.inf
    elif c.family == "zeros":                  # t = 0 over a +0.0 uncond half keeps the cond bits: positives, zeros of both signs, far negatives
        n_pos, n_zero = c.param
        rows = np.empty((R, V), dtype=np.float32)
        for r in range(R):
            v = np.concatenate([g.uniform(0.1, 1.0, n_pos), np.zeros(n_zero), -np.abs(g.standard_normal(V - n_pos - n_zero)) - 8.0]).astype(np.float32)
            sign = g.integers(0, 2, n_zero).astype(bool)
            sign[:2] = (True, False)
            v[n_pos:n_pos + n_zero][sign] = np.float32(-0.0)
            rows[r] = v[g.permutation(V)]
        lg = np.concatenate([rows.reshape(B, l, V), np.zeros((B, l, V), dtype=np.float32)], 0)
    elif c.family == "bound":                  # pairwise distinct cond values; at t != 0 the host test checks that no tie arose at the k-th CFG value
        lg = gauss(2.5)
        lg[:B] = _distinct(lg[:B].reshape(R, V)).reshape(B, l, V)
        if c.t == 0.0:
            lg[B:] = 0.0
    elif c.family == "ties":                   # ranks lo .. hi-1 of every row set to the value at rank 899 (the 900th largest)
        lo, hi = c.param
        rows = _distinct(gauss(2.5)[:B].reshape(R, V))
        order = np.argsort(-rows, axis=-1, kind="stable")
        for r in range(R):
            rows[r, order[r, lo:hi]] = rows[r, order[r, 899]]
        lg = np.concatenate([rows.reshape(B, l, V), np.zeros((B, l, V), dtype=np.float32)], 0)
    else:
        raise ValueError(c.family)
    return torch.from_numpy(np.ascontiguousarray(lg))


def make_noise(c: Case) -> torch.Tensor:
    """(B*l, V) Exp(1) noise of the case: the portable Philox stream."""
    return torch.from_numpy(exponential_noise(1000 + c.seed, c.seed, c.B, c.l, c.V)).view(-1, c.V)


# ------------------------------------------------------------------------------------------------ references for cfg_sample
def r1(c: Case, lg: torch.Tensor, q: torch.Tensor):
    """(cfg logits, ids, masked logits) of the torch-fp32 oracle.  The kernel reads top_k >= V as "no top-k"; torch.topk raises there."""
    cl = orc.cfg_combine(lg, c.B, c.t)
    ids, masked = orc.sample_topk_topp(cl, min(c.top_k, c.V), c.top_p, q)
    return cl, ids, masked


def draw_gap(masked: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """Per row: relative gap between the two largest p/q, p = softmax of the masked logits in float64."""
    V = masked.shape[-1]
    ratio = masked.reshape(-1, V).double().softmax(-1) / q.reshape(-1, V).double()
    top2 = ratio.topk(2, dim=-1)[0]
    return (top2[:, 0] - top2[:, 1]) / top2[:, 0]


def r2(cl: torch.Tensor, top_k: int, top_p: float, q: torch.Tensor) -> dict:
    """The float64 restatement with the (value, index) tie rule, from the fp32 CFG logits `cl` (B, l, V).  Per row (R = B*l):
    keep (R, V) bool, masked (R, V) fp32 (the input bits where kept), n_keep, n_topk (finite entries before top-p), margin (a), gap (b), tie (bool:
    several entries at the k-th value, or the top-p cut falls between equal values)."""
    V = cl.shape[-1]
    x32 = cl.reshape(-1, V)
    x = x32.double()
    R = x.shape[0]
    keep = x > NEG_INF
    tie = torch.zeros(R, dtype=torch.bool)
    if 0 < top_k < V:
        kth = x.topk(top_k, dim=-1)[0][:, -1:]
        tie = ((x == kth).sum(-1) > 1) & (kth[:, 0] > NEG_INF)
        keep = keep & (x >= kth)
    n_topk = keep.sum(-1)
    margin = torch.full((R,), float("inf"), dtype=torch.float64)
    if top_p > 0:
        xm = torch.where(keep, x, torch.full_like(x, NEG_INF))
        s, idx = torch.sort(xm + 0.0, dim=-1, descending=False, stable=True)          # + 0.0: -0.0 sorts as +0.0, so equal zeros go by index
        cum = s.softmax(-1).cumsum(-1)
        thr = float(np.float32(1.0 - top_p))
        rm_s = cum <= thr
        rm_s[:, -1] = False
        if V > 1:
            margin = (cum[:, :-1] - thr).abs().amin(-1)
        n_rm = rm_s.sum(-1)                                                            # the running sum is monotone: the removed entries are a prefix
        assert bool((rm_s.long().cumsum(-1)[torch.arange(R), (n_rm - 1).clamp(min=0)] == n_rm).all())
        last_rm = s[torch.arange(R), (n_rm - 1).clamp(min=0)]
        first_kept = s[torch.arange(R), n_rm]
        tie = tie | ((n_rm > 0) & (last_rm == first_kept) & (first_kept > NEG_INF))
        keep = keep & ~torch.zeros_like(rm_s).scatter_(1, idx, rm_s)
    masked = torch.where(keep, x32, torch.full_like(x32, NEG_INF))
    return {"keep": keep, "masked": masked, "n_keep": keep.sum(-1), "n_topk": n_topk, "margin": margin, "gap": draw_gap(masked, q), "tie": tie}


def sorted_kept(masked: torch.Tensor) -> torch.Tensor:
    """Rows sorted ascending (-inf first): equal between two maskings iff they keep the same number of entries and the same values."""
    return masked.reshape(-1, masked.shape[-1]).sort(-1)[0]


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    """Inputs and both references of a case, computed once per process and shared (callers must not modify the tensors)."""
    c = BY_NAME[name]
    lg, q = make_logits(c), make_noise(c)
    cl, ids1, masked1 = r1(c, lg, q)
    out = {"case": c, "logits": lg, "q": q, "cfg": cl, "ids1": ids1, "masked1": masked1.reshape(-1, c.V)}
    out.update(r2(cl, c.top_k, c.top_p, q))
    out["set_ambiguous"] = out["margin"] <= AMBIG_SET
    out["draw_ambiguous"] = out["gap"] <= AMBIG_DRAW
    return out


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ verify_accept: rules and scan
def kl_ref(cfg_t: torch.Tensor, cfg_d: torch.Tensor) -> torch.Tensor:
    """KL(softmax target || softmax draft) per token in float64 with 0 * log 0 = 0: entries of target probability 0 contribute nothing,
    a draft probability of 0 under a positive target probability makes the divergence +inf."""
    lt, ld = cfg_t.double().log_softmax(-1), cfg_d.double().log_softmax(-1)
    p = lt.exp()
    return torch.where(p > 0, p * (lt - ld), torch.zeros_like(p)).sum(-1)


@dataclass
class VerifyCase:
    name: str
    B: int
    V: int
    lens: List[int]
    ts: List[float]
    logits: List[torch.Tensor]                     # per stage (2B, l_j, V) target logits
    ids: List[torch.Tensor]                        # per stage (B, l_j) int64 draft ids
    draft: Optional[List[torch.Tensor]] = None     # per stage (2B, l_j, V) draft logits (KL rule)
    expect_argmax: Optional[torch.Tensor] = None   # (B, lsum) where the construction fixes it

    def cfg(self, which="logits"):
        return [orc.cfg_combine(x, self.B, t) for x, t in zip(getattr(self, which), self.ts)]


def tie_pairs(V: int):
    """Index pairs that hold the duplicated maximum: different lanes of one wave, different 1024-entry chunks of one thread, different waves."""
    return {4096: [(5, 4095), (1023, 1024), (3, 4)], 1000: [(5, 999), (255, 256), (3, 4)], 8: [(0, 7), (5, 6), (3, 4)]}[V]


def argmax_tie_case(V: int) -> VerifyCase:
    """B = 2, two stages of 4 tokens, t = 0 over a zero uncond half (the CFG logits are the cond bits).  Tokens 0-2: the maximum duplicated at one pair each,
    draft = the smaller index (match); tokens 3-5: the same pairs, draft = the larger index (no match); token 6: all-equal row, draft 0 for image 0 and 1 for
    image 1; token 7: -inf everywhere but at V - 1."""
    g, B = _rng(900 + V), 2
    cond = g.standard_normal(size=(B, 8, V), dtype=np.float32) * np.float32(2)
    ids = np.zeros((B, 8), dtype=np.int64)
    am = np.zeros((B, 8), dtype=np.int64)
    for b in range(B):
        for k, (i, j) in enumerate(tie_pairs(V) * 2):
            cond[b, k, [i, j]] = cond[b, k].max() + np.float32(1.0)
            ids[b, k], am[b, k] = (i if k < 3 else j), i
        cond[b, 6] = np.float32(0.75); ids[b, 6] = b; am[b, 6] = 0
        cond[b, 7] = -np.inf; cond[b, 7, V - 1] = np.float32(-3.0); ids[b, 7] = V - 1; am[b, 7] = V - 1
    lg = torch.from_numpy(np.concatenate([cond, np.zeros_like(cond)], 0))
    idt = torch.from_numpy(ids)
    return VerifyCase(f"argmax_ties_V{V}", B, V, [4, 4], [0.0, 0.0], [lg[:, :4].contiguous(), lg[:, 4:].contiguous()], [idt[:, :4], idt[:, 4:]],
                      expect_argmax=torch.from_numpy(am))


TOPK_TIE_ABOVE = 3          # entries strictly above the draft token's score on the controlled rows of topk_tie_case


def topk_tie_case(V: int = 1000, oob: bool = False) -> VerifyCase:
    """B = 2, stages of 4 tokens at t = 1.0 and t = 0.5.  Tokens 0-1 of each stage: a zero uncond half, ranks 3..8 of the row tied (six entries, three strictly
    above them), draft = one of the tied entries: the rule holds iff top_k > 3.  Tokens 2-3: both halves multiples of 0.5, so (1+t)*c - t*u cancels into exact
    ties; draft = an entry of the first tied group at rank >= 4 of the CFG row.  oob: the draft ids of token 1 and token 3 of every stage are -1 and V."""
    g, B, ts = _rng(950 + V), 2, [1.0, 0.5]
    lgs, idl = [], []
    for t in ts:
        lg = g.standard_normal(size=(2 * B, 4, V), dtype=np.float32) * np.float32(2)
        lg[:, 2:] = np.round(lg[:, 2:] * 2) / 2
        lg[B:, :2] = 0.0
        ids = np.zeros((B, 4), dtype=np.int64)
        for b in range(B):
            for k in (0, 1):
                order = np.argsort(-lg[b, k], kind="stable")
                lg[b, k, order[3:9]] = lg[b, k, order[3]]
                ids[b, k] = order[3 + 2 * k + b]
        lgt = torch.from_numpy(lg)
        cl = orc.cfg_combine(lgt, B, t)
        ids_t = torch.from_numpy(ids)
        sv, si = cl[:, 2:].sort(dim=-1, descending=True, stable=True)
        first_tied = ((sv[..., 4:-1] == sv[..., 5:]).int().argmax(-1) + 4).unsqueeze(-1)          # first rank >= 4 that ties with the next one
        ids_t[:, 2:] = si.gather(-1, first_tied + torch.tensor([0, 1]).view(1, 2, 1)).squeeze(-1)   # token 2: its first entry, token 3: its second
        if oob:
            ids_t[:, 1], ids_t[:, 3] = -1, V
        lgs.append(lgt); idl.append(ids_t)
    return VerifyCase(f"topk_ties_V{V}" + ("_oob" if oob else ""), B, V, [4, 4], ts, lgs, idl)


def kl_case(V: int = 1000, identical: bool = False) -> VerifyCase:
    """B = 2, stages of 2 and 3 tokens, t = 0 over a zero uncond half.  identical: the draft logits are the target's bits, every second token top-50 masked
    (shared -inf entries).  Otherwise per (stage, token):
      (0,0) draft = target + noise                      (0,1) both top-50 masked at the same places, draft = target + noise there
      (1,0) draft -inf at 5 places where the target is finite: KL = +inf
      (1,1) peaked target (+25 at one entry), draft = target + noise       (1,2) shared -inf entries and identical values: KL = 0"""
    g, B, lens = _rng(970 + V), 2, [2, 3]
    tl, dl = [], []
    for s, n in enumerate(lens):
        t = g.standard_normal(size=(B, n, V), dtype=np.float32) * np.float32(2)
        noise = g.standard_normal(size=(B, n, V), dtype=np.float32) * np.float32(0.6)
        kth = np.sort(t, -1)[..., V - min(50, V // 2)][..., None]
        masked = np.where(t < kth, np.float32(-np.inf), t)
        if identical:
            t[:, 1::2] = masked[:, 1::2]
            d = t.copy()
        elif s == 0:
            t[:, 1] = masked[:, 1]
            d = t + noise                                                   # -inf + noise stays -inf
        else:
            t[:, 1, 7 % V] += np.float32(25)
            t[:, 2] = masked[:, 2]
            d = t + noise
            d[:, 2] = t[:, 2]
            d[:, 0, 3:8] = -np.inf
        z = np.zeros_like(t)
        tl.append(torch.from_numpy(np.concatenate([t, z], 0))); dl.append(torch.from_numpy(np.concatenate([d, z], 0)))
    ids = [x[:B].argmax(-1) for x in dl]
    return VerifyCase(f"kl_V{V}" + ("_identical" if identical else ""), B, V, lens, [0.0, 0.0], tl, ids, draft=dl)


KL_THRESHOLDS = (0.05, 0.5, 5.0)      # test_sampler_hard_host.py checks that no token's fp64 KL lies within 1e-4 * max(1, KL) of any of them

SCAN_LENS = (1, 1, 2, 3, 1, 7, 10, 1, 1, 2, 3, 1, 1, 10, 1, 1)
SCAN_MATCHED = (1, 1, 2, 1, 1, 3, 1, 1, 1, 0, 3, 1, 1, 7, 1, 1)
F32_THIRD = float(np.float32(1.0 / 3.0))
# (threshold, leading stages accepted): the rate is float32(matched) / float32(total) promoted to double, against the double threshold.
#   0.1   float32(1/10) = 0.100000001490 >= 0.1, so the 10-token stage passes and the scan stops at stage 9 (0 of 2)
#   1/3   float32(1/3) = 0.333333343267 >= 1/3, so stage 3 passes; stage 6 (0.1) fails
#   float32(1/3) as a double: stage 3 passes at equality
#   3/7   float32(3/7) = 0.428571432829 >= 3/7: stages 0-2 pass, stage 3 (1/3) fails
SCAN_16 = ((0.0, 16), (1.5, 0), (0.1, 9), (1.0 / 3.0, 6), (F32_THIRD, 6), (3.0 / 7.0, 3))
SCAN_3_LENS, SCAN_3_MATCHED = (10, 7, 3), (7, 3, 1)
F32_SEVEN_TENTHS = float(np.float32(0.7))
# float32(7/10) = 0.699999988079 < 0.7 (a double rate would pass); against float32(0.7) it passes at equality and stage 1 (3/7) fails.
# 0.25: all three stages pass (0.7, 3/7, 1/3).
SCAN_3 = ((0.7, 0), (F32_SEVEN_TENTHS, 1), (0.25, 3))


def scan_case(lens, matched, V: int = 8) -> VerifyCase:
    """B = 1 (so the token totals are the stage lengths: 3, 7 and 10 among them), top-1 rule at t = 0: the first matched[j] tokens of stage j carry the target's
    argmax, the others argmax + 1."""
    g = _rng(990 + len(lens))
    lgs, ids = [], []
    for n, m in zip(lens, matched):
        cond = g.standard_normal(size=(1, n, V), dtype=np.float32)
        lg = torch.from_numpy(np.concatenate([cond, np.zeros_like(cond)], 0))
        am = lg[:1].argmax(-1)
        am[:, m:] = (am[:, m:] + 1) % V
        lgs.append(lg); ids.append(am)
    return VerifyCase(f"scan_{len(lens)}", 1, V, list(lens), [0.0] * len(lens), lgs, ids)


def scan_expect(lens, matched, thr: float, B: int = 1) -> int:
    n = 0
    for l, m in zip(lens, matched):
        if float(np.float32(m) / np.float32(B * l)) >= thr:
            n += 1
        else:
            break
    return n


def combine_case() -> VerifyCase:
    """Heavy-tailed rows (Cauchy x 2 clamped to +-1e4) at V = 1000, three stages with their own t: products up to 2.5e4 whose difference an fma would round
    differently from torch's two roundings."""
    g, B, V, lens = _rng(999), 2, 1000, [3, 5, 8]
    lgs = [torch.from_numpy(np.clip(g.standard_cauchy(size=(2 * B, n, V)) * 2.0, -1e4, 1e4).astype(np.float32)) for n in lens]
    return VerifyCase("combine_heavy", B, V, lens, [0.3, 1.5, 0.0], lgs, [torch.zeros(B, n, dtype=torch.int64) for n in lens])


# ------------------------------------------------------------------------------------------------ gumbel_mix
@dataclass(frozen=True)
class GumbelCase:
    name: str
    src: str               # sampler case whose logits and noise provide `masked`
    kind: str              # 'r1' = the oracle's masked logits of that case, 'topk' = top-k only (exactly top_k survivors on the b1024 rows)
    Cv: int
    ratio: float
    tau: float


_TAUS = ((0.0, 0.27), (1.0, 0.0135), (1.0, 0.005))
GUMBEL_CASES = ([GumbelCase(f"one_V4096_Cv32_r{r:g}_tau{tau:g}", "peak4096_k900", "r1", 32, r, tau) for r, tau in _TAUS]
                + [GumbelCase(f"k1024_V4096_Cv32_r{r:g}_tau{tau:g}", "b1024", "topk", 32, r, tau) for r, tau in _TAUS]
                + [GumbelCase(f"inf_V4096_Cv32_r{r:g}_tau{tau:g}", "inf4096_k900", "r1", 32, r, tau) for r, tau in _TAUS]
                + [GumbelCase("inf_V1000_Cv33_r1_tau0.005", "inf1000_full", "r1", 33, 1.0, 0.005),
                   GumbelCase("one_V1000_Cv33_r0_tau0.27", "peak1000_k900", "r1", 33, 0.0, 0.27),
                   GumbelCase("gauss_V1000_Cv8_r1_tau0.0135", "g1000_k900", "r1", 8, 1.0, 0.0135),
                   GumbelCase("inf_V8_Cv8_r0_tau0.005", "inf8_full", "r1", 8, 0.0, 0.005),
                   GumbelCase("one_V8_Cv33_r0_tau0.27", "peak8_k1", "r1", 33, 0.0, 0.27),
                   GumbelCase("gauss_V8_Cv32_r1_tau0.0135", "g8_full", "r1", 32, 1.0, 0.0135),
                   GumbelCase("gauss_V8_Cv8_r1_tau0.005", "g8_full", "r1", 8, 1.0, 0.005)])
assert len(GUMBEL_CASES) <= 16
GUMBEL_FLOOR = 2e-5


@functools.lru_cache(maxsize=None)
def gumbel_inputs(name: str) -> dict:
    """masked (B, l, V), e (B, l, V), codebook (V, Cv), the float64 result h64 (B, l, Cv), the torch-fp32 oracle's result and its error against h64."""
    gc = next(g for g in GUMBEL_CASES if g.name == name)
    ref = reference(gc.src)
    c = ref["case"]
    if gc.kind == "topk":
        masked = orc.sample_topk_topp(ref["cfg"], c.top_k, 0.0, ref["q"])[1]
    else:
        masked = ref["masked1"].reshape(c.B, c.l, c.V)
    e = torch.from_numpy(exponential_noise(2000 + c.seed, c.seed | orc.GUMBEL_DRAW, c.B, c.l, c.V))
    cb = torch.from_numpy(_rng(c.seed, 7002).standard_normal(size=(c.V, gc.Cv), dtype=np.float32))
    y = (masked.double() * (1.0 + gc.ratio) - e.double().log()) / gc.tau
    h64 = y.softmax(-1) @ cb.double()
    h_o = orc.gumbel_mix(masked, gc.ratio, e, cb, tau=gc.tau)
    return {"case": gc, "sampler_case": c, "masked": masked.contiguous(), "e": e, "codebook": cb, "h64": h64, "h_oracle": h_o,
            "err_oracle": float((h_o.double() - h64).abs().max()), "n_finite": (masked > NEG_INF).sum(-1)}


def gumbel_bar(gi: dict) -> float:
    """4 x the torch-fp32 oracle's own error against float64 (the margin the backward-attention battery gave its fp32 reference), floored at the golden
    test's bar 2e-5 * max(1, max|codebook|)."""
    return max(4.0 * gi["err_oracle"], GUMBEL_FLOOR * max(1.0, float(gi["codebook"].abs().max())))
