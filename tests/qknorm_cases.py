"""Inputs, fp64 references and error bounds shared by test_gpu_seam_qknorm.py and test_seam_qknorm_host.py (seam.qk_l2norm, csrc/qknorm_train.hip).

Inputs: qkv (B, L, 3, H, 64) whose q and k heads cycle over FAMILIES by (row, head) - N(0, 1); one channel at 1e4 beside 1e-3; every channel at +-6e4, the edge of
fp16's range; 1e-20 N(0, 1) (fp32 only: a norm below eps; a half qkv gets N(0, 1) there); an all-zero head - the v heads N(0, 1); biases N(0, 1); scale_log with heads
below, exactly at and above max_log = float32(log 100).  Upstream gradients: N(0, 1) with one row x 65536, one zero row and one row x -65536 (the gradient of a float16 v:
x 16, since 65536 N(0, 1) is no float16 number).  A half qkv is rounded first and the reference starts from the rounded values.

Reference: the torch chain of basic_var.py:93-105 in float64 on the CPU, with the bias added in full precision to the given qkv.

Bounds, first order in u = 2^-24, from the kernels' operation counts.  With x the widened (and biased) head, n = max(|x|, eps), xh = x / n, s = exp(min(scale_log, max_log)):
  * the bias add: one rounding per element (C_B = 1; counted for k too, which has none).
  * n: the sum of squares has non-negative terms of one rounding each (the product) under a chain of at most 4 + 4 additions (the lane's four products, four cross-lane
    levels), and x itself carries C_B twice in its square: relative (1 + 8 + 2 C_B) u on the sum, halved by the root, then the root's own rounding:
    C_N = (9 + 2 C_B) / 2 + 1 = 6.5.
  * s: expf within its documented 1 ulp = 2 u (the min is exact): C_S = 2.
  * xh = x / n: C_X = C_B + C_N + 1 = 8.5.   q = xh s: C_Q = C_X + C_S + 1 = 11.5.   k = xh: C_X.
    A head below eps gives x / eps (float32(1e-12) is off 1e-12 by less than u): fewer roundings than the counts above.
  * dx_j = (s / n) (g_j - xh_j dot), dot = sum_i xh_i g_i, A = sum_i |xh_i g_i|:
      dot: terms of C_X + 1 under a chain of 8 additions:                       |d dot| <= (C_X + 9) u A
      xh_j dot: C_X + 1 relative, plus |xh_j| |d dot|
      the subtraction, s / n (C_S + C_N + 1) and the last product:              C_F = C_N + C_S + 3 = 11.5 relative to |dx_j|
    tol_dx = u [ (s / n) ((C_X + 1) |xh_j dot| + |xh_j| (C_X + 9) A) + C_F |dx_j| ];  below eps dx = (s g) / eps: 5 roundings <= C_F.
  * column sums over (b, l): a term passes through at most `depth` additions: 8 rows per wave, 3 to add the waves, ceil(parts / 4) partial rows per slice of pass 2 and 3
    to add the slices, parts = B ceil(L / 32).  dq_bias: the terms' own tol_dx plus depth u sum|dx_q|; dv_bias: exact terms, depth u sum|dv|;
    dscale_log: terms g q of C_Q + 1, depth + 6 (the six wave levels over a head's 64 column sums).
  * one rounding to the output's dtype (2^-24 / 2^-11 / 2^-8 relative; fp16 also half its smallest subnormal; fp32 outputs: 2^-150 for the subnormal range).  Where the
    reference rounded to the output's dtype is +-inf the result must be that inf.
Nothing here was fitted to a kernel's output.  The condition that keeps the bounds honest is asserted by both test files: torch's float32 autograd ON THE CPU, on the
same inputs, meets every one of them."""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F

from conftest import rnd

U = 2.0 ** -24
EPS = 1e-12
CHUNK = 32                                     # engine.TRAIN_CHUNK, asserted equal by the host test
MAX_LOG = float(torch.log(torch.tensor(100.0)))          # the reference's max_scale_mul: a float32 number
HEADS = (1, 3, 4, 16, 30, 48)
SHAPES = tuple((H, B, L) for H in HEADS for B, L in ((1, 1), (2, 5), (3, 41))) + ((16, 2, 681),)        # (2, 681): 22 chunks per image
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
FAMILIES = ("normal", "hot", "edge", "tiny", "zero")
ROUND = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
C_B, C_S = 1.0, 2.0
C_N = (9.0 + 2.0 * C_B) / 2.0 + 1.0
C_X = C_B + C_N + 1.0
C_Q = C_X + C_S + 1.0
C_F = C_N + C_S + 3.0


def _k(H: int) -> int:
    return HEADS.index(H) if H in HEADS else 0


def families(H: int, B: int, L: int, slot: int):
    """Family of head h of row r in slot 0 (q) / 1 (k): cycled over (row, head), shifted by the index of H and by 2 for k, so that the small shapes cover every family in
    both slots between them."""
    k = _k(H) + 2 * slot
    return [[FAMILIES[(r * H + h + k) % len(FAMILIES)] for h in range(H)] for r in range(B * L)]


@functools.lru_cache(maxsize=None)
def case(H: int, B: int, L: int, dtype=torch.float32):
    """(qkv (B, L, 3, H, 64) in dtype, q_bias (64 H), v_bias (64 H), scale_log (H)), all but qkv float32."""
    seed = 9000 + 11 * H + 3 * L + B
    qkv = rnd(seed, (B * L, 3, H, 64))
    sign = torch.sign(rnd(seed + 1, (B * L, 3, H, 64)))
    for slot in (0, 1):
        fam = families(H, B, L, slot)
        for r in range(B * L):
            for h in range(H):
                f = fam[r][h]
                if f == "hot":
                    qkv[r, slot, h] = 1e-3 * sign[r, slot, h]
                    qkv[r, slot, h, (7 * r + 3 * h) % 64] = 1e4
                elif f == "edge":
                    qkv[r, slot, h] = 6e4 * sign[r, slot, h]
                elif f == "tiny" and dtype == torch.float32:
                    qkv[r, slot, h] *= 1e-20
                elif f == "zero":
                    qkv[r, slot, h] = 0.0
    scale_log = 1.0 + 0.5 * rnd(seed + 2, (H,))
    for h in range(min(H, 3)):          # head h: at / above / below max_log, rotated by the index of H
        kind = (h + _k(H)) % 3
        scale_log[h] = (MAX_LOG, MAX_LOG + 0.75, 1.25)[kind]
    return qkv.view(B, L, 3, H, 64).to(dtype).contiguous(), rnd(seed + 3, (64 * H,)), rnd(seed + 4, (64 * H,)), scale_log


@functools.lru_cache(maxsize=None)
def upstream(H: int, B: int, L: int, dtype=torch.float32):
    """(gq, gk fp32, gv in dtype), each (B, L, H, 64): N(0, 1); row 0 x big, the middle row zero, the last row x -big (fewer rows: as many of the three as fit, in that
    order).  big = 65536; 16 for a float16 gv."""
    out = []
    n = B * L
    for i, dt in enumerate((torch.float32, torch.float32, dtype)):
        big = 16.0 if dt == torch.float16 else 65536.0
        g = rnd(4242 + 64 * H + 5 * L + B + 1000 * i, (n, H, 64))
        g[0] *= big
        if n >= 3:
            g[n // 2] = 0.0
        if n >= 2:
            g[n - 1] *= -big
        out.append(g.view(B, L, H, 64).to(dt).contiguous())
    return tuple(out)


def _chain(qkv, scale_log, q_bias, v_bias, dtype):
    """The reference's chain in `dtype` on the CPU -> leaves and (q, k, v), each (B, L, H, 64)."""
    H = qkv.shape[3]
    x = qkv.detach().to(dtype).clone().requires_grad_(True)
    sl = scale_log.detach().to(dtype).clone().requires_grad_(True)
    qb = None if q_bias is None else q_bias.detach().to(dtype).clone().requires_grad_(True)
    vb = None if v_bias is None else v_bias.detach().to(dtype).clone().requires_grad_(True)
    xq, xk, xv = x.unbind(2)
    if qb is not None:
        xq = xq + qb.view(H, 64)
    if vb is not None:
        xv = xv + vb.view(H, 64)
    s = sl.clamp_max(MAX_LOG).exp().view(H, 1)
    return (x, sl, qb, vb), (F.normalize(xq, dim=-1).mul(s), F.normalize(xk, dim=-1), xv)


def _run(qkv, scale_log, q_bias, v_bias, grads, dtype):
    """{q, k, v, dqkv, dscale_log, dq_bias, dv_bias} of torch's autograd in `dtype` on the CPU (the bias gradients None without the bias)."""
    with torch.enable_grad():
        leaves, outs = _chain(qkv, scale_log, q_bias, v_bias, dtype)
        res = dict(zip(("q", "k", "v"), (o.detach() for o in outs)))
        if grads is not None:
            ins = [t for t in leaves if t is not None]
            got = list(torch.autograd.grad(outs, ins, [g.to(dtype) for g in grads]))
            for name, t in zip(("dqkv", "dscale_log", "dq_bias", "dv_bias"), leaves):
                res[name] = None if t is None else got.pop(0)
    return res


def ref64(qkv, scale_log, q_bias, v_bias, grads=None):
    return _run(qkv, scale_log, q_bias, v_bias, grads, torch.float64)


def torch32(qkv, scale_log, q_bias, v_bias, grads=None):
    return _run(qkv.float(), scale_log, q_bias, v_bias, grads, torch.float32)


def sum_depth(B: int, L: int) -> int:
    parts = math.ceil(L / CHUNK) * B
    return CHUNK // 4 + 3 + math.ceil(parts / 4) + 3


def _rounded(tol0: torch.Tensor, ref: torch.Tensor, dtype) -> torch.Tensor:
    r = ROUND[dtype]
    return tol0 * (1.0 + r) + r * ref.abs() + (2.0 ** -25 if dtype == torch.float16 else 2.0 ** -150 if dtype == torch.float32 else 0.0)


def fwd_bounds(ref, dtype, v_bias: bool = True):
    """(tol_q, tol_k, tol_v): q and k are float32 results whose last rounding is the last counted operation; v, written only with a v_bias, is the float32 sum (one
    rounding) rounded once more to qkv's dtype when that is a half - without a v_bias it is a view of qkv: exact."""
    tv = C_B * U * ref["v"].abs()
    if not v_bias:
        tv = torch.zeros_like(tv)
    elif dtype != torch.float32:
        tv = _rounded(tv, ref["v"], dtype)
    return C_Q * U * ref["q"].abs() + 2.0 ** -150, C_X * U * ref["k"].abs() + 2.0 ** -150, tv


def bwd_bounds(qkv, scale_log, q_bias, grads, ref, dtype):
    """{dqkv, dscale_log, dq_bias, dv_bias} -> bound, in the shapes of the gradients; ref = ref64's dict."""
    B, L, _, H, _ = qkv.shape
    x = qkv.double()
    gq, gk, gv = (g.double() for g in grads)
    s = scale_log.double().clamp_max(MAX_LOG).exp().view(H, 1)
    depth = sum_depth(B, L)

    def dx_tol(xs, g, sc, dx):
        nrm = xs.norm(dim=-1, keepdim=True)
        n = nrm.clamp_min(EPS)
        xh = xs / n
        dot = (xh * g).sum(-1, keepdim=True)
        A = (xh * g).abs().sum(-1, keepdim=True)
        return U * ((sc / n) * ((C_X + 1) * (xh * dot).abs() + xh.abs() * (C_X + 9) * A) + C_F * dx.abs())

    xq = x[:, :, 0] + (0.0 if q_bias is None else q_bias.double().view(H, 64))
    dxq, dxk = ref["dqkv"][:, :, 0], ref["dqkv"][:, :, 1]
    tq0, tk0 = dx_tol(xq, gq, s, dxq), dx_tol(x[:, :, 1], gk, torch.ones_like(s), dxk)
    tol = {"dqkv": torch.stack((_rounded(tq0, dxq, dtype), _rounded(tk0, dxk, dtype), torch.zeros_like(gv)), 2)}
    if dtype == torch.float32:          # the last rounding of a float32 result is the last counted operation, not one more
        tol["dqkv"] = torch.stack((tq0 + 2.0 ** -150, tk0 + 2.0 ** -150, torch.zeros_like(gv)), 2)
    gate = (scale_log.double() <= MAX_LOG).double()
    tol["dscale_log"] = gate * (C_Q + 1 + depth + 6) * U * (gq * ref["q"]).abs().sum((0, 1, 3)) + 2.0 ** -150
    tol["dq_bias"] = (tq0 + depth * U * dxq.abs()).sum((0, 1)).reshape(-1) + 2.0 ** -150
    tol["dv_bias"] = (depth * U * gv.abs()).sum((0, 1)).reshape(-1) + 2.0 ** -150
    return tol


@functools.lru_cache(maxsize=None)
def full(H: int, B: int, L: int, dtype, bias: bool):
    """Everything the tests of one case share, computed once and left unchanged: inputs (qkv, q_bias, v_bias, scale_log; the biases None without), upstream gradients,
    the float64 reference, torch's float32 run and every bound."""
    qkv, qb, vb, sl = case(H, B, L, dtype)
    if not bias:
        qb = vb = None
    g = upstream(H, B, L, dtype)
    ref = ref64(qkv, sl, qb, vb, g)
    tol = dict(zip(("q", "k", "v"), fwd_bounds(ref, dtype, bias)))
    tol.update(bwd_bounds(qkv, sl, qb, g, ref, dtype))
    return {"in": (qkv, qb, vb, sl), "g": g, "ref": ref, "t32": torch32(qkv, sl, qb, vb, g), "tol": tol}


def assert_torch32_meets_the_bounds(c, tag: str) -> None:
    """The honesty condition of the module docstring, on one case of full()."""
    for name, t in c["tol"].items():
        if c["ref"][name] is not None:
            assert worst(f"{name} torch float32 CPU {tag}", c["t32"][name], c["ref"][name], t) <= 1.0, (name, tag)


def worst(name: str, got: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor, dtype=torch.float32) -> float:
    """Print and return the worst err / bound ratio over EVERY element (0 / 0 counts as 0: an exact result under a zero bound).  Where the reference rounded to `dtype` is
    +-inf the result must be that inf (ratio 0 when it is, inf when not); any other non-finite result counts as inf.  The caller asserts the return value."""
    got = got.detach().double().cpu().reshape(ref.shape)
    ref_r = ref.to(dtype).double()
    inf_ref = torch.isinf(ref_r)
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    ratio = torch.where(~torch.isfinite(got), torch.full_like(err, float("inf")), ratio)
    ratio = torch.where(inf_ref, torch.where(got == ref_r, torch.zeros_like(err), torch.full_like(err, float("inf"))), ratio)
    w = float(ratio.max())
    i = int(ratio.argmax())
    print(f"  {name}: worst err/bound {w:.3f} (got {float(got.flatten()[i]):.6e}, ref {float(ref.flatten()[i]):.6e}, bound {float(tol.flatten()[i]):.3e}; "
          f"{int(inf_ref.sum())} of {ref.numel()} elements are inf in {dtype})")
    return w
