"""Inputs, float64 references and per-element error bounds for seam.teacher_embed (tests/test_gpu_seam_embed.py, tests/test_seam_embed_host.py).  Everything here is
CPU work from fixed seeds.

The bound.  An output element is a sum of n terms t_1 .. t_n formed in float32.  Each product enters its sum through one fmaf (no rounding of its own) and every addition
rounds once, so whatever the order of the additions the computed value is sum_i t_i (1 + d_i) with |d_i| <= (1 + u)^(n - 1) - 1, u = 2^-24: to first order
|err| <= (n - 1) u sum_i |t_i|.  The tests allow 1.01 (n + 1) u sum_i |t_i|: two further roundings (torch's GEMM may round a product before adding it; the widening
of a half gradient is exact) and 1 % for the second-order terms, which stay below that for n u < 0.01, n < 1.6e5 - asserted below.  sum_i |t_i| is evaluated in float64
from the same inputs by running the same linear maps on absolute values.  A half output adds half an ulp of the half format at |exact|; a half upstream gradient is
rounded BEFORE either side reads it, so it adds nothing.  An element with no terms (a stage beyond `tokens`, a class no image selects) must be exactly 0."""
from __future__ import annotations

import math

import torch

U = 2.0 ** -24
F32, F64 = torch.float32, torch.float64
NC1 = 6
GRADS = ("xv", "class_emb", "pos_start", "word_w", "word_b", "lvl_emb", "pos_1LC")
PARAMS = ("class_emb", "pos_start", "word_w", "word_b", "lvl_emb", "pos_1LC")


def ladder(pns):
    """(first_l, L, lvl (1, L) int64, begin_ends) of a patch-number ladder."""
    lens = [p * p for p in pns]
    lvl = torch.cat([torch.full((n,), i, dtype=torch.int64) for i, n in enumerate(lens)]).view(1, -1)
    ends, cur = [], 0
    for n in lens:
        ends.append((cur, cur + n)); cur += n
    return lens[0], cur, lvl, ends


def _draw(gen, shape, kind):
    if kind == "int":
        return torch.randint(-3, 4, shape, generator=gen).to(F32)
    x = torch.randn(shape, generator=gen)
    if kind == "heavy":          # a few entries 32 times the rest (their products 2^10 times): single terms dominate the sums, which cancel badly; a float16 x stays finite
        x = x * torch.where(torch.rand(shape, generator=gen) < 0.03, 32.0, 1.0)
    return x


def make(pns, B, C, K, T=None, seed=0, kind="normal", labels="random", gdtype=F32, rate=0.25):
    """One case: CPU tensors in the dtypes the operator takes.  kind: 'normal', 'heavy' (heavy-tailed) or 'int' (small integers: every sum is exact in float32).  labels:
    'random' (repeats are likely: NC1 = 6) or 'same' (every image on one label).  xv is a slice of a longer tensor (two spare rows), as the reference hands it over."""
    first_l, L, lvl, ends = ladder(pns)
    T = L if T is None else T
    gen = torch.Generator().manual_seed(1000 + seed)
    c = dict(pns=tuple(pns), B=B, C=C, K=K, T=T, L=L, S=len(pns), first_l=first_l, lvl=lvl, begin_ends=ends, kind=kind, rate=rate)
    c["label"] = torch.randint(0, NC1 - 1, (B,), generator=gen) if labels == "random" else torch.full((B,), 2, dtype=torch.int64)
    c["r"] = torch.rand(B, generator=gen)
    c["xv_long"] = _draw(gen, (B, L - first_l + 2, K), kind)
    c["xv"] = c["xv_long"][:, :L - first_l]
    for name, shape in (("class_emb", (NC1, C)), ("pos_start", (1, first_l, C)), ("word_w", (C, K)), ("word_b", (C,)), ("lvl_emb", (len(pns), C)), ("pos_1LC", (1, L, C))):
        c[name] = _draw(gen, shape, kind)
    c["g"] = _draw(gen, (B, T, C), kind).to(gdtype)
    c["gc"] = _draw(gen, (B, C), kind)
    return c


def effective_labels(c, drop=True):
    if not drop:
        return c["label"]
    return torch.where(c["r"] < c["rate"], NC1 - 1, c["label"])          # a float32 tensor against a Python number: a float32 comparison


def _forward(c, j, xv, p, dt):
    """The reference expression of var.py:227-232 in dtype dt on the tensors given."""
    first_l, T = c["first_l"], c["T"]
    cond = p["class_emb"][j]
    sos = cond.unsqueeze(1).expand(-1, first_l, -1) + p["pos_start"].expand(c["B"], first_l, -1)
    x = sos if T == first_l else torch.cat((sos, xv[:, :T - first_l] @ p["word_w"].t() + p["word_b"]), dim=1)
    return x + (p["lvl_emb"][c["lvl"][0, :T]].unsqueeze(0) + p["pos_1LC"][:, :T]), cond


def run(c, dt=F64, drop=True, absolute=False, with_g=True, with_gc=True):
    """(x, cond, {gradient name: tensor}) in dtype dt through torch's autograd on the CPU.  absolute=True: the same maps on |inputs| - the sum of |terms| per element."""
    f = (lambda t: t.to(dt).abs()) if absolute else (lambda t: t.to(dt))
    with torch.enable_grad():          # grad mode is process-wide state and other test modules switch it off
        p = {n: f(c[n]).clone().requires_grad_(True) for n in PARAMS}
        xv = f(c["xv"]).clone().requires_grad_(True)
        x, cond = _forward(c, effective_labels(c, drop), xv, p, dt)
        loss = 0
        if with_g:
            loss = loss + (x * f(c["g"])).sum()          # a half g is widened exactly
        if with_gc:
            loss = loss + (cond * f(c["gc"])).sum()
        grads = torch.autograd.grad(loss, [xv] + [p[n] for n in PARAMS], allow_unused=True)
    named = {n: (torch.zeros_like(t) if gr is None else gr) for n, gr, t in zip(GRADS, grads, [xv] + [p[n] for n in PARAMS])}
    return x.detach(), cond.detach(), named


def term_counts(c, drop=True, with_gc=True):
    """n per element: how many terms are added into it (scalars where it is the same for every element of a tensor; per row where it differs)."""
    B, T, K, C, first_l, S = c["B"], c["T"], c["K"], c["C"], c["first_l"], c["S"]
    j = effective_labels(c, drop)
    per_class = torch.bincount(j, minlength=NC1).to(F64) * (first_l + (1 if with_gc else 0))
    per_stage = torch.bincount(c["lvl"][0, :T], minlength=S).to(F64) * B
    nx = torch.cat((torch.full((first_l,), 4.0, dtype=F64), torch.full((T - first_l,), K + 3.0, dtype=F64))).view(1, T, 1)
    return dict(x=nx, cond=0.0, xv=float(C), class_emb=per_class.view(NC1, 1), pos_start=float(B), word_w=float(B * (T - first_l)), word_b=float(B * (T - first_l)),
                lvl_emb=per_stage.view(S, 1), pos_1LC=float(B))


def half_ulp(exact: torch.Tensor, dtype) -> torch.Tensor:
    """Half a unit in the last place of `dtype` (float16 / bfloat16) at |exact|; 0 for float32."""
    if dtype == F32:
        return torch.zeros_like(exact)
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(exact.abs().clamp_min(2.0 ** emin))).clamp_min(emin)
    return 0.5 * torch.pow(torch.tensor(2.0, dtype=F64), e - mant)


def bounds(c, drop=True, out_dtype=F32, with_g=True, with_gc=True):
    """(reference, bound) dictionaries over 'x', 'cond' and the gradient names, float64."""
    x, cond, gr = run(c, F64, drop, False, with_g, with_gc)
    ax, _, agr = run(c, F64, drop, True, with_g, with_gc)
    n = term_counts(c, drop, with_gc)
    assert max(float(torch.as_tensor(v).max()) for v in n.values()) * U < 0.01, "the first-order bound needs n u << 1"
    ref = dict(x=x, cond=cond, **gr)
    bnd = dict(x=1.01 * (n["x"] + 1) * U * ax + half_ulp(x, out_dtype), cond=torch.zeros_like(cond))
    for name in GRADS:
        nn = torch.as_tensor(n[name], dtype=F64)
        bnd[name] = 1.01 * torch.where(nn > 0, nn + 1, nn) * U * agr[name]
    return ref, bnd


def worst(got: torch.Tensor, ref: torch.Tensor, bnd: torch.Tensor):
    """(largest err / bound over the elements with a positive bound, whether every element with a zero bound is exact)."""
    err = (got.detach().to("cpu", F64) - ref).abs()
    pos = bnd > 0
    ratio = float((err[pos] / bnd[pos]).max()) if pos.any() else 0.0
    return ratio, bool((err[~pos] == 0).all()), bool(torch.isfinite(err).all())


def assert_integer_case_is_exact(c, drop=True):
    """An 'int' case cannot pass by accident: every sum of |terms| stays below 2^24, so each partial sum in any order is an integer float32 holds exactly."""
    ax, _, agr = run(c, F64, drop, True)
    top = max([float(ax.max())] + [float(t.max()) for t in agr.values()])
    assert top < 2 ** 24, f"integer case overflows the exact range: {top}"
    return top


def assert_torch_float32_meets_bounds(c, drop=True):
    """The sanity check of the bound: torch's own float32 autograd on the CPU stays inside it on the same inputs."""
    ref, bnd = bounds(c, drop)
    c32 = dict(c, g=c["g"].float())
    x, cond, gr = run(c32, F32, drop)
    got = dict(x=x, cond=cond, **gr)
    out = {}
    for name in ref:
        ratio, zeros_ok, finite = worst(got[name], ref[name], bnd[name])
        assert finite and zeros_ok and ratio <= 1.0, f"torch float32 misses the bound on {name}: err / bound = {ratio}"
        out[name] = ratio
    return out


def to_device(c, dev):
    d = dict(c)
    for k, v in c.items():
        if isinstance(v, torch.Tensor):
            d[k] = v.to(dev)
    d["xv"] = d["xv_long"][:, :c["L"] - c["first_l"]]          # again a slice, read in place
    return d


def params_of(c, requires_grad=True):
    return [c[n].clone().requires_grad_(requires_grad) for n in PARAMS]
