"""Hard inputs, float64 references and per-element bars for the three kernel families every sampled token passes through in every transformer block:
ln_modulate (csrc/elementwise.hip), qk_norm_append (same file, five cache formats) and sdvar_op_attention (csrc/attention.hip, attention_bf16x3.hip,
attention_f16x2.hip).  A plain helper module: tests/test_block_hard_host.py checks the cases and the bars on the CPU, tests/test_gpu_block_hard.py checks the
kernels against them.  Every input comes from a seed (conftest.rnd, numpy Philox); nothing here touches a GPU, and no reference uses
F.scaled_dot_product_attention, F.layer_norm or F.normalize: softmax, mean / variance and the L2 norm are written out in float64 on the fp32 inputs the kernel receives.

Attention bar, per output element (i, d), cache format f:
    tol = eps_f * sum_j p_ij |v_jd|  +  phi_f * 2^-25 * (1 + sum_{j visible to i} |v_jd|)
    eps_f = 2e-5 + c_f * max_ij(|q_i| |k_j|) * 2^-22        (the maximum is taken per (row, head))
  2e-5 is the project's bar for every fp32-accurate kernel; the second term of eps_f is the error of the exponent: c_f = 1 for formats 0, 1, 2 (exact operands, the
  fp32 rounding of a 64-term dot product), c_f = 4 for formats 3 and 4 (Q split to 2^-22 per element, K too in format 3, added over the channels in the worst case,
  with a factor of 2 left for the fp32 accumulation).  phi_f = 1 for formats 3 and 4, else 0: the absolute floor of the two-plane fp16 split - fp16's subnormal
  spacing 2^-24 halved by rounding, once per softmax weight and once for V.  The floor is conservative: the kernel's deferred running maximum keeps P at or above
  exp(s - rowmax), the value assumed here.  For formats 1 and 4 the reference uses the fp16-rounded K and V the cache holds.

LayerNorm bar, per element:
    tol = 2e-5 * max(1, |ref|) + (1 + |scale|) * (max_row|x| / sqrt(var + 1e-6)) * 2^-22
  The second term is what an fp32 mean costs on a row whose offset dwarfs its spread: the mean carries a rounding error of max|x| 2^-24 or so, which the
  normalisation divides by sigma and the modulation multiplies by (1 + scale).  No fp32 LayerNorm avoids it.

Each attention case also has a plain fp32 evaluation (`attn_fp32`) and an emulation of the operand format (`attn_emulate`: Q, K, V and P split as the format
splits them, the plane products the kernel keeps, float64 accumulation, the true row maximum as the softmax reference); each LayerNorm case a plain fp32
two-pass evaluation (`ln_fp32`).  test_block_hard_host.py holds them to a fraction of the bar, which is what makes the bar a statement about the format and
not about one kernel."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch

from conftest import rnd

FORMATS = (0, 1, 2, 3, 4)
LN100_F32 = float(np.float32(math.log(100.0)))          # the reference's float32 clamp of scale_mul (basic_var.py:104)
L2E = 1.4426950408889634
DEFER_NATS = 6.0 * math.log(2.0)                        # ATT_DEFER of attention_f16x2.hip in nats: 4.159
F16_MAX = 65504.0
D = 64


def unit(t: torch.Tensor) -> torch.Tensor:
    return t / t.norm(dim=-1, keepdim=True)


def key_perm(n: int) -> torch.Tensor:
    """Format 2 stores V^T with bits 2 and 3 of the key position swapped inside every 16 keys (an involution): key j lives at position key_perm[j]."""
    return torch.tensor([(p & ~12) | ((p & 4) << 1) | ((p & 8) >> 1) for p in range(n)], dtype=torch.long)


# ------------------------------------------------------------------------------------------------------------------ operand splits (host)
def split3(t: torch.Tensor):
    """Exact 3-way truncation split of fp32 into bf16 planes (common.h split3): list of three fp32 tensors whose sum is t."""
    out, rest = [], t.clone()
    for _ in range(3):
        hi = (rest.view(torch.int32) & -65536).view(torch.float32)
        out.append(hi)
        rest = rest - hi
    return out


def split3_bits(t: torch.Tensor) -> torch.Tensor:
    return torch.stack([(p.view(torch.int32) >> 16).to(torch.int16) for p in split3(t)])


def split2h(t: torch.Tensor):
    """fp32 -> (h, l) fp16 planes as common.h split2h: saturate at +-65504, h = fp16(x) to nearest even, l = fp16(x - h)."""
    x = t.clamp(-F16_MAX, F16_MAX)
    h = x.half()
    return h, (x - h.float()).half()


def f16x2_plane_tol(ref: torch.Tensor) -> torch.Tensor:
    """The two-plane rule: 2^-21.9 relative while the low plane is a normal fp16 number, 2^-24.9 absolute below."""
    return torch.maximum(ref.abs() * 2.0 ** -21.9, torch.full_like(ref, 2.0 ** -24.9))


# ------------------------------------------------------------------------------------------------------------------ attention cases
@dataclass(frozen=True, eq=False)
class AttnCase:
    name: str
    q: torch.Tensor            # (R, H, l, 64) fp32, what sdvar_op_attention receives
    k: torch.Tensor            # (R, H, Ktot, 64) fp32, before the cache format rounds it
    v: torch.Tensor
    qbeg: Tuple[int, ...]
    vis: Tuple[int, ...]

    @property
    def R(self): return self.q.shape[0]
    @property
    def H(self): return self.q.shape[1]
    @property
    def l(self): return self.q.shape[2]
    @property
    def Ktot(self): return self.k.shape[2]
    @property
    def Lp(self): return (self.Ktot + 5 + 63) // 64 * 64          # always leaves rows [Ktot, Lp) behind the valid keys

    def visible(self) -> torch.Tensor:
        """(l, Ktot) bool: queries >= qbeg[j] see keys < vis[j]."""
        m = torch.zeros(self.l, self.Ktot, dtype=torch.bool)
        for j, b in enumerate(self.qbeg):
            e = self.qbeg[j + 1] if j + 1 < len(self.qbeg) else self.l
            m[b:e, :self.vis[j]] = True
        return m


def _benign(seed, R, H, l, Ktot, qbeg, vis, name):
    q = unit(rnd(seed, (R, H, l, D))) * 4.0
    return AttnCase(name, q, unit(rnd(seed + 1, (R, H, Ktot, D))), rnd(seed + 2, (R, H, Ktot, D)), tuple(qbeg), tuple(vis))


def _a1(last: bool) -> AttnCase:
    """Diffuse tail: one key carries 60 to 98 % of a row's mass (heads = three mass levels), ~700 keys 8 to 12 nats below it carry the rest."""
    R, H, l, Ktot = 1, 3, 40, 700
    q0, k, v = unit(rnd(101, (R, H, l, D))), unit(rnd(102, (R, H, Ktot, D))), rnd(103, (R, H, Ktot, D))
    kd = Ktot - 5 if last else 5                                 # tile 0 or the last tile
    k[:, :, kd] = unit(q0.mean(2))
    q = unit(0.3 * q0 + k[:, :, kd:kd + 1]) * torch.tensor([8.0, 10.0, 12.0]).view(1, 3, 1, 1)
    return AttnCase("A1_last" if last else "A1_first", q, k, v, (0,), (Ktot,))


A2_STEPS = (4.0, 4.3)          # nats per tile, head 0 / head 1: one on each side of DEFER_NATS
A2_TILES = 20
A2_Q = 8.0
A2_RISING = 13                 # the one query of A2_one that sees the staircase


def _a2(kind: str) -> AttnCase:
    """Staircases: every key of a 32-key tile has the same score, tiles differ by `step` nats (keys are multiples of one unit vector u, not unit vectors).
    asc / desc: every query along u, query i scaled by 1 + i / (100 l), so the steps spread over 1 % and stay on their side of 4.159.
    one: ONLY query 13 lies along u; the others are orthogonal to it (scores of +-1 against an orthogonal noise component of the keys)."""
    R, H, l, Ktot = 1, 2, 40, 32 * A2_TILES
    u = unit(rnd(111, (D,)))
    t = torch.arange(A2_TILES, dtype=torch.float32)
    if kind == "desc":
        t = A2_TILES - 1 - t
    k = torch.zeros(R, H, Ktot, D)
    for h, step in enumerate(A2_STEPS):
        k[0, h] = (t * (step / A2_Q)).repeat_interleave(32)[:, None] * u
    if kind == "one":
        w = rnd(112, (R, H, l, D)); w = w - (w @ u)[..., None] * u
        q = A2_Q * unit(w)
        q[:, :, A2_RISING] = A2_Q * u
        n = rnd(113, (R, H, Ktot, D)); n = n - (n @ u)[..., None] * u
        k = k + unit(n)
    else:
        g = A2_Q * (1.0 + torch.arange(l, dtype=torch.float32) / (100.0 * l))
        q = (g[:, None] * u).expand(R, H, l, D).contiguous()
    return AttnCase("A2_" + kind, q, k, rnd(114, (R, H, Ktot, D)), (0,), (Ktot,))


def _a3() -> AttnCase:
    """Clamp scale: |q| = 100 (the ln 100 clamp of scale_mul), unit keys.  Queries 0..15 are sign vectors / 8 (norm exactly 1, so a copied key scores exactly 100
    and a negated one exactly -100 in any arithmetic); keys 10..17 copy queries 0..7, keys 100..107 negate queries 8..15, keys 108..111 negate queries 0..3;
    key 200 sits at 0.97 of query 20 (which has no copy), key 201 at 0.97 of query 0 (which has one)."""
    R, H, l, Ktot = 1, 2, 40, 300
    uq, k, v = unit(rnd(121, (R, H, l, D))), unit(rnd(122, (R, H, Ktot, D))), rnd(123, (R, H, Ktot, D))
    uq[:, :, :16] = torch.sign(rnd(124, (R, H, 16, D))) / 8.0
    k[:, :, 10:18] = uq[:, :, 0:8]
    k[:, :, 100:108] = -uq[:, :, 8:16]
    k[:, :, 108:112] = -uq[:, :, 0:4]
    for kidx, qi in ((200, 20), (201, 0)):
        a = uq[:, :, qi]
        w = k[:, :, kidx] - (k[:, :, kidx] * a).sum(-1, keepdim=True) * a
        k[:, :, kidx] = unit(0.97 * a + math.sqrt(1 - 0.97 ** 2) * unit(w))
    return AttnCase("A3_clamp", uq * 100.0, k, v, (0,), (Ktot,))


A4_HOT = (7, 40)


def _a4() -> AttnCase:
    """V dynamic range: channels 7 and 40 reach |v| = 6e4 (below 65504), every 16th key row is scaled by 1e-4, key row 33 is exactly zero."""
    c = _benign(131, 1, 2, 40, 300, (0,), (300,), "A4_vrange")
    v = c.v.clone()
    v[:, :, ::16] *= 1e-4
    v[:, :, 33] = 0.0
    for ch in A4_HOT:
        v[..., ch] *= 6e4 / v[..., ch].abs().max()
    return AttnCase(c.name, c.q, c.k, v, c.qbeg, c.vis)


A6_QBEG = (0, 1, 5, 14, 30, 55, 91, 128, 129, 160, 200, 256, 290, 300, 330, 350)
A6_VIS = (1, 5, 14, 31, 32, 33, 64, 95, 96, 97, 161, 256, 257, 300, 351, 400)
A6_L = 380


def _a6() -> AttnCase:
    """One call with the 16 stages the kernels take: boundaries inside the first wave (1, 5, 14, 30), at queries 128 and 256, a single-query stage [128, 129),
    vis at 32 k - 1, 32 k and 32 k + 1, vis[0] = 1."""
    return _benign(141, 1, 2, A6_L, A6_VIS[-1], A6_QBEG, A6_VIS, "A6_stages16")


A7_KTOT = (31, 32, 33, 63, 64, 65, 96, 97)
A7_L = (1, 31, 32, 33, 127, 128, 129, 130, 255, 256, 257)
A7_PREFIX = 40


def _a7k(Ktot: int) -> AttnCase:
    """17 queries in two stages; the first sees Ktot - 1 keys, the second Ktot: both sides of every tile edge."""
    return _benign(150 + Ktot, 1, 2, 17, Ktot, (0, 9), (Ktot - 1, Ktot), f"A7_K{Ktot}")


def _a7l(l: int) -> AttnCase:
    Ktot = A7_PREFIX + l
    qbeg, vis = ((0,), (Ktot,)) if l < 2 else ((0, l // 2), (A7_PREFIX + l // 2, Ktot))
    return _benign(400 + l, 1, 2, l, Ktot, qbeg, vis, f"A7_l{l}")


_BUILDERS = {"A1_first": lambda: _a1(False), "A1_last": lambda: _a1(True), "A2_asc": lambda: _a2("asc"), "A2_desc": lambda: _a2("desc"),
             "A2_one": lambda: _a2("one"), "A3_clamp": _a3, "A4_vrange": _a4, "A6_stages16": _a6}
_BUILDERS.update({f"A7_K{K}": functools.partial(_a7k, K) for K in A7_KTOT})
_BUILDERS.update({f"A7_l{l}": functools.partial(_a7l, l) for l in A7_L})
HARD_ATTN = ("A1_first", "A1_last", "A2_asc", "A2_desc", "A2_one", "A3_clamp", "A4_vrange")       # A1 .. A4: also run with operand-plane outputs
STALE_ATTN = ("A1_first", "A6_stages16")                                                          # A5: run twice, zero tail / stale tail
EDGE_ATTN = tuple(f"A7_K{K}" for K in A7_KTOT) + tuple(f"A7_l{l}" for l in A7_L)
ALL_ATTN = HARD_ATTN + ("A6_stages16",) + EDGE_ATTN


@functools.lru_cache(maxsize=None)
def attn_case(name: str) -> AttnCase:
    return _BUILDERS[name]()


def held_kv(c: AttnCase, fmt: int):
    """K and V as the reference takes them: the fp16-rounded values for formats 1 and 4 (what the cache holds), the fp32 values otherwise."""
    if fmt in (1, 4):
        return c.k.clamp(-F16_MAX, F16_MAX).half().float(), c.v.clamp(-F16_MAX, F16_MAX).half().float()
    return c.k, c.v


def pack_cache(c: AttnCase, fmt: int, stale: bool = False):
    """(kc, vc) CPU tensors in the layout of cache format `fmt` with Lp rows per (row, head).  Rows [Ktot, Lp) are zero, or with `stale` the largest finite
    leftovers a rolled-back cursor can leave: +-65504 in every plane (formats 3, 4), +-3e38 in every plane (format 2), NaN for formats 0 and 1 (which never
    read past Ktot)."""
    R, H, Ktot, Lp = c.R, c.H, c.Ktot, c.Lp
    sign = 1.0 - 2.0 * ((torch.arange(Lp - Ktot)[:, None] + torch.arange(D)[None, :]) % 2).float()          # (tail, 64) of +-1
    if fmt in (0, 1):
        dt = torch.float32 if fmt == 0 else torch.float16
        kc = torch.zeros(R, H, Lp, D, dtype=dt); vc = torch.zeros(R, H, Lp, D, dtype=dt)
        kc[:, :, :Ktot] = c.k.to(dt); vc[:, :, :Ktot] = c.v.to(dt)
        if stale:
            kc[:, :, Ktot:] = float("nan"); vc[:, :, Ktot:] = float("nan")
        return kc, vc
    if fmt == 2:
        kc = torch.zeros(R, H, 3, Lp, D, dtype=torch.int16); vc = torch.zeros(R, H, 3, D, Lp, dtype=torch.int16)
        perm = key_perm(Lp)
        kc[:, :, :, :Ktot] = split3_bits(c.k).permute(1, 2, 0, 3, 4)
        vc[:, :, :, :, perm[:Ktot]] = split3_bits(c.v).permute(1, 2, 0, 4, 3)
        if stale:
            big = (sign * 3e38).bfloat16().view(torch.int16)
            kc[:, :, :, Ktot:] = big
            vc[:, :, :, :, perm[Ktot:]] = big.t()
        return kc, vc
    NP = 2 if fmt == 3 else 1
    kc = torch.zeros(R, H, NP, Lp, D, dtype=torch.int16); vc = torch.zeros(R, H, NP, Lp, D, dtype=torch.int16)
    kc[:, :, :, :Ktot] = torch.stack(split2h(c.k)[:NP]).view(torch.int16).permute(1, 2, 0, 3, 4)
    vc[:, :, :, :Ktot] = torch.stack(split2h(c.v)[:NP]).view(torch.int16).permute(1, 2, 0, 3, 4)
    if stale:
        big = (sign * F16_MAX).half().view(torch.int16)
        kc[:, :, :, Ktot:] = big; vc[:, :, :, Ktot:] = big
    return kc, vc


def _layout(o: torch.Tensor) -> torch.Tensor:
    """(R, H, l, 64) -> the kernel's (R, l, H * 64)."""
    R, H, l, _ = o.shape
    return o.transpose(1, 2).reshape(R, l, H * D)


def _softmax64(s: torch.Tensor) -> torch.Tensor:
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def attn_ref_of(c: AttnCase, fmt: int):
    """(ref, tol), both (R, l, H * 64) float64: the float64 attention on the fp32 inputs and the per-element bar of the module docstring."""
    kh, vh = held_kv(c, fmt)
    vis = c.visible()
    s = (c.q.double() @ kh.double().transpose(-1, -2)).masked_fill(~vis, -math.inf)
    p = _softmax64(s)
    ref = p @ vh.double()
    spv = p @ vh.double().abs()
    vsum = 1.0 + vis.double() @ vh.double().abs()
    qk = c.q.double().norm(dim=-1).amax(-1) * kh.double().norm(dim=-1).amax(-1)                  # (R, H): max_ij |q_i| |k_j|
    eps = 2e-5 + (4.0 if fmt >= 3 else 1.0) * qk * 2.0 ** -22
    tol = eps[..., None, None] * spv + (2.0 ** -25 * vsum if fmt >= 3 else 0.0)
    return _layout(ref), _layout(tol)


@functools.lru_cache(maxsize=None)
def attn_ref(name: str, fmt: int):
    """attn_ref_of a named case, computed once per session and shared by every test that needs it (callers must not modify it)."""
    return attn_ref_of(attn_case(name), fmt)


def attn_probs(name: str, fmt: int = 0):
    """(scores, probabilities) in float64, (R, H, l, Ktot): what the host test reads the cases' properties from."""
    c = attn_case(name)
    kh, _ = held_kv(c, fmt)
    s = (c.q.double() @ kh.double().transpose(-1, -2)).masked_fill(~c.visible(), -math.inf)
    return s, _softmax64(s)


def attn_fp32(name: str, fmt: int) -> torch.Tensor:
    """Plain fp32 evaluation: fp32 scores, fp32 softmax, fp32 P V."""
    c = attn_case(name)
    kh, vh = held_kv(c, fmt)
    s = (c.q @ kh.transpose(-1, -2)).masked_fill(~c.visible(), -math.inf)
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return _layout((e / e.sum(-1, keepdim=True)) @ vh).double()


def _planes(t: torch.Tensor, fmt: int, cache_side: bool):
    """The operand planes of format `fmt` as float64 tensors, and per plane its order (a product is kept when the orders add up to <= the format's budget)."""
    if fmt == 2:
        return [p.double() for p in split3(t)]
    if fmt == 3 or (fmt == 4 and not cache_side):
        h, l = split2h(t)
        return [h.double(), l.double()]
    if fmt == 4:
        return [t.clamp(-F16_MAX, F16_MAX).half().double()]
    return [t.double()]


def _kept_products(a, b, fmt: int):
    """sum of the plane products the kernels keep: all with i + j <= 2 of 3 x 3 (bf16x3: six of nine), i + j <= 1 of 2 x 2 (f16x2: three of four; two of two
    when the cache side has one plane), the single product otherwise.  `a` and `b` are lists of matrices; b is transposed by the caller."""
    budget = 2 if fmt == 2 else 1
    return sum(x @ y for i, x in enumerate(a) for j, y in enumerate(b) if i + j <= budget)


def attn_emulate(name: str, fmt: int, drop_p_low: bool = False) -> torch.Tensor:
    """The operand format's own arithmetic with float64 accumulation: scores from the kept plane products of Q and K, rounded to fp32 once; p = 2^(s log2 e - M) in
    fp32 against the true row maximum; P split like every other operand; O from the kept products of P and V; the row sum from the unsplit fp32 p.
    drop_p_low emulates the SDVAR_ATTN_P1 experiment of attention_f16x2.hip (P without its low plane) - the host test shows that the bar refuses it."""
    c = attn_case(name)
    kf = held_kv(c, fmt)[0] if fmt in (1, 4) else c.k
    vf = held_kv(c, fmt)[1] if fmt in (1, 4) else c.v
    qp, kp = _planes(c.q, fmt, False), [p.transpose(-1, -2) for p in _planes(kf, fmt, True)]
    s = _kept_products(qp, kp, fmt).float().masked_fill(~c.visible(), -math.inf)
    m = s.max(-1, keepdim=True).values * np.float32(L2E)
    p = torch.exp2(s * np.float32(L2E) - m)
    pp = _planes(p, fmt, False)
    if drop_p_low:
        pp = pp[:1]
    o = _kept_products(pp, _planes(vf, fmt, True), fmt) / p.double().sum(-1, keepdim=True)
    return _layout(o)


def worst(err: torch.Tensor, tol: torch.Tensor):
    """(max err / tol, flat index of that element)."""
    ratio = err / tol
    i = int(torch.argmax(ratio))
    return float(ratio.flatten()[i]), i


# ------------------------------------------------------------------------------------------------------------------ LayerNorm cases
LN_WIDTHS = (64, 260, 1024, 1028, 2048, 2060, 2304, 3072)       # three instantiations (C <= 1024 / 2048 / 3072), both lane maps (C % 8), each upper edge
LN_FAMILIES = ("hot3", "one3e4", "off1e2", "off1e3", "off1e4", "off1e3_tight", "tiny1e-4", "tiny1e-6", "const", "zero", "gauss", "const_generic")
LN_EXACT_ROWS = ("const", "zero")                               # output == shift exactly
LN_GROUPS = ("rnd", "minus1", "pm30")                           # modulation of an image group: N(0,1) scale, scale == -1 exactly, scale = +-30
LN_CONST = 3.5            # short significand: C * 3.5 and every partial sum of it are exact in fp32 in any order, so mean == x exactly
LN_CONST_GENERIC = 3.7    # a generic constant's fp32 row sum is not exact: held to the bar, not to equality


@dataclass(frozen=True, eq=False)
class LnCase:
    name: str
    rows: int
    C: int
    rpi: int
    x: torch.Tensor            # (rows, C)
    mod: torch.Tensor          # (groups, mod_stride): scale at [2C, 3C), shift at [4C, 5C) of each group's row, as the adaLN buffer
    row_family: Tuple[str, ...]
    group_family: Tuple[str, ...]

    @property
    def mod_stride(self): return self.mod.shape[1]
    @property
    def scale(self): return self.mod[:, 2 * self.C:3 * self.C].repeat_interleave(self.rpi, 0)[:self.rows]
    @property
    def shift(self): return self.mod[:, 4 * self.C:5 * self.C].repeat_interleave(self.rpi, 0)[:self.rows]
    @property
    def planes(self): return self.C % 32 == 0


def _ln_row(fam: str, seed: int, C: int) -> torch.Tensor:
    g = rnd(seed, (C,))
    if fam == "hot3":
        g[[3, C // 2 + 1, C - 2]] *= 1e3
    elif fam == "one3e4":
        g[C // 3] = 3e4
    elif fam in ("off1e2", "off1e3", "off1e4"):
        g = g + float(fam[3:])
    elif fam == "off1e3_tight":
        g = g * 1e-2 + 1e3
    elif fam == "tiny1e-4":
        g = g * 1e-4
    elif fam == "tiny1e-6":
        g = g * 1e-6
    elif fam == "const":
        g = torch.full((C,), LN_CONST)
    elif fam == "const_generic":
        g = torch.full((C,), LN_CONST_GENERIC)
    elif fam == "zero":
        g = torch.zeros(C)
    else:
        g = g * 2.0 + 0.3
    return g


LN_SHAPES = tuple((C, 41, 7, 0, 0) for C in LN_WIDTHS) + tuple(
    (C, rows, rpi, foff, goff) for C in (260, 2304) for rows, rpi, foff, goff in ((1, 1, 4, 1), (5, 7, 0, 2), (5, 5, 5, 1), (41, 1, 3, 0), (41, 41, 7, 2)))


@functools.lru_cache(maxsize=None)
def ln_case(C: int, rows: int, rpi: int, foff: int = 0, goff: int = 0) -> LnCase:
    """Row i is of family (i + foff) % 12, image group g of family (g + goff) % 3; mod_stride = 6 C + 8 (larger than the 6 C of a dense adaLN buffer)."""
    G = (rows + rpi - 1) // rpi
    seed = 1000 + 7 * C + 3 * rows + rpi
    rf = tuple(LN_FAMILIES[(i + foff) % len(LN_FAMILIES)] for i in range(rows))
    gf = tuple(LN_GROUPS[(g + goff) % len(LN_GROUPS)] for g in range(G))
    x = torch.stack([_ln_row(f, seed + 1 + i, C) for i, f in enumerate(rf)])
    mod = rnd(seed, (G, 6 * C + 8))
    for g, f in enumerate(gf):
        if f == "minus1":
            mod[g, 2 * C:3 * C] = -1.0
        elif f == "pm30":
            mod[g, 2 * C:3 * C] = 30.0 * torch.sign(mod[g, 2 * C:3 * C])
    return LnCase(f"C{C}_r{rows}_i{rpi}", rows, C, rpi, x, mod, rf, gf)


def ln_ref(c: LnCase):
    """(ref, tol, max|x| / sigma per row), float64."""
    x, sc, sh = c.x.double(), c.scale.double(), c.shift.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    sig = torch.sqrt(var + 1e-6)
    ref = (x - mean) / sig * (1.0 + sc) + sh
    spread = x.abs().amax(-1, keepdim=True) / sig
    tol = 2e-5 * ref.abs().clamp_min(1.0) + (1.0 + sc.abs()) * spread * 2.0 ** -22
    return ref, tol, spread.squeeze(-1)


def ln_exact_mask(c: LnCase) -> torch.Tensor:
    """(rows,) bool: rows whose output must equal `shift` bit for bit - constant and all-zero rows, and every row of a group with scale == -1."""
    g = torch.arange(c.rows) // c.rpi
    return torch.tensor([c.row_family[i] in LN_EXACT_ROWS or c.group_family[int(g[i])] == "minus1" for i in range(c.rows)])


def ln_fp32(c: LnCase, one_pass: bool = False, serial: bool = False) -> torch.Tensor:
    """Plain fp32 evaluation in two passes (mean, then the squared deviations) with numpy's float32 sum, which adds pairwise in blocks - the error growth of any
    tree-shaped sum, a wave reduction included.  serial: strictly left to right instead (numpy cumsum); its mean drifts by sqrt(C) roundings and it misses the
    bar on the offset rows from C = 2048 on (3.4 x at C = 2304), so the bar also says that a row must not be summed by one thread.
    one_pass: the E[x^2] - mean^2 form that the bar must refuse on the offset rows."""
    x = c.x.numpy()
    f = np.float32
    total = (lambda a: np.cumsum(a, axis=1, dtype=f)[:, -1:]) if serial else (lambda a: a.sum(axis=1, keepdims=True, dtype=f))
    mean = (total(x) / f(c.C)).astype(f)
    if one_pass:
        var = np.maximum((total(x * x) / f(c.C) - mean * mean).astype(f), f(0))
    else:
        d = (x - mean).astype(f)
        var = (total(d * d) / f(c.C)).astype(f)
    rstd = (f(1) / np.sqrt(var + f(1e-6))).astype(f)
    out = ((x - mean) * rstd) * (c.scale.numpy() + f(1)) + c.shift.numpy()
    return torch.from_numpy(out.astype(f)).double()


# ------------------------------------------------------------------------------------------------------------------ QK-norm append
SAMPLER_POS0 = (0, 1, 5, 14, 30, 55, 91, 155, 255, 424)         # the cursor positions of the 256^2 ladder
SAMPLER_LENS = (1, 4, 9, 16, 25, 36, 64, 100, 169, 256)
SAMPLER_LP = 704
SAMPLER_REDO = (6, 7)                                           # a rejected round: stages 6 and 7 appended again over the old rows


def qkv_split(qkv: torch.Tensor, R: int, l: int, H: int):
    """(R * l, 3 H 64) -> q, k, v as (R, H, l, 64) views of the GEMM output the kernel reads."""
    return qkv.view(R, l, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)


def qk_ref(qkv: torch.Tensor, scale_mul, R: int, l: int, H: int):
    """float64 reference of qk_norm_append from the fp32 qkv: (q_out, k, v, q magnitude) with q magnitude = the expected length of each q vector
    (the bar is 2e-5 of it).  scale_mul None: attn_l2_norm = False, q * 2^-5 and k raw."""
    q, k, v = (t.double() for t in qkv_split(qkv, R, l, H))
    if scale_mul is None:
        return q * 2.0 ** -5, k, v, (q * 2.0 ** -5).norm(dim=-1, keepdim=True)
    sm = torch.exp(scale_mul.double().clamp_max(LN100_F32)).view(1, H, 1, 1)
    qn = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12) * sm
    kn = k / k.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return qn, kn, v, qn.norm(dim=-1, keepdim=True)


def k_norm_fp32(qkv: torch.Tensor, scale_mul, R: int, l: int, H: int) -> torch.Tensor:
    """The fp32-normalised k (raw k without scale_mul) whose .half() formats 1 and 4 hold, up to rare one-ulp differences."""
    k = qkv_split(qkv, R, l, H)[1]
    return k if scale_mul is None else k / k.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def qk_edge_inputs(seed: int, R: int, l: int, H: int, extremes: bool) -> torch.Tensor:
    """qkv (R * l, 3 H 64) with, on row 0 .. 4 of every image (where l allows): an all-zero q AND an all-zero k on the same (row, head); one-hot q and k;
    and with `extremes` q and k of magnitude 1e-15 per element (norm below F.normalize's eps) and 1e15 (the squares stay normal in fp32); a v channel at 6e4."""
    C = H * D
    qkv = rnd(seed, (R * l, 3 * C))
    t = qkv.view(R, l, 3, H, D)
    t[:, 0, 0:2, 0] = 0.0
    if l > 1:
        t[:, 1, 0:2, H - 1] = 0.0; t[:, 1, 0, H - 1, 5] = -2.5; t[:, 1, 1, H - 1, 63] = 0.75
    if extremes and l > 3:
        t[:, 2, 0:2, 0] *= 1e-15
        t[:, 3, 0:2, H - 1] *= 1e15
    t[:, :, 2, :, 9] = 6e4 * torch.sign(t[:, :, 2, :, 9])
    return qkv


def decode_cache(kc: torch.Tensor, vc: torch.Tensor, fmt: int):
    """CPU copies of a cache in format `fmt` -> (K, V) in key order as raw bits, (R, H, planes, Lp, 64): equality of two decodes is equality of every bit of the
    caches, and a slice along the key axis selects exactly the storage of those keys (format 2's V^T is un-transposed and un-permuted)."""
    if fmt == 0:
        return kc.view(torch.int32).unsqueeze(2), vc.view(torch.int32).unsqueeze(2)
    if fmt == 1:
        return kc.view(torch.int16).unsqueeze(2), vc.view(torch.int16).unsqueeze(2)
    if fmt == 2:
        return kc, vc[..., key_perm(vc.shape[-1])].transpose(-1, -2)
    return kc, vc


def cache_values(bits: torch.Tensor, fmt: int) -> torch.Tensor:
    """decoded bits -> float64 values (R, H, Lp, 64): the sum of the planes."""
    if fmt == 0:
        return bits.view(torch.float32).double().sum(2)
    if fmt == 2:
        return (bits.to(torch.int32) << 16).view(torch.float32).double().sum(2)
    return bits.contiguous().view(torch.float16).double().sum(2)


def empty_cache(fmt: int, R: int, H: int, Lp: int, seed: int):
    """A cache full of finite leftovers (what a rolled-back cursor leaves behind), never zeros: every untouched bit is recognisable."""
    shape = {0: (R, H, Lp, D), 1: (R, H, Lp, D), 2: (R, H, 3, Lp, D), 3: (R, H, 2, Lp, D), 4: (R, H, 1, Lp, D)}[fmt]
    g = [rnd(seed + i, shape, 3.0) for i in range(2)]
    if fmt == 0:
        return g[0], g[1]
    if fmt == 1:
        return g[0].half(), g[1].half()
    if fmt == 2:
        return g[0].bfloat16().view(torch.int16), g[1].bfloat16().view(torch.int16).transpose(-1, -2).contiguous()
    return g[0].half().view(torch.int16), g[1].half().view(torch.int16)
