"""Inputs, fp64 references and error bounds shared by test_gpu_seam_adaln.py and test_seam_adaln_host.py (seam.adaln_modulate / seam.gated_residual,
csrc/adaln_train.hip).

Inputs: rows of block_hard_cases.LN_FAMILIES (hot channels, offsets 1e2 - 1e4, tiny, constant and zero rows), modulation groups LN_GROUPS (N(0,1) scale, scale == -1,
scale = +-30) laid out as the reference's (B, 1, 6, C) adaLN buffer: gamma = [:, :, 0], scale = [:, :, 2], shift = [:, :, 4] are strided views (batch stride 6 C).
Upstream gradients: N(0,1) with one row x 65536, one zero row and one row x -65536.

Forward bar: the project's LayerNorm bar, 2e-5 max(1, |ref|) + (1 + |scale|) (max_row|x| / sqrt(var + 1e-6)) 2^-22.

Backward bounds, first order in u = 2^-24, from the kernels' operation counts.  D = 4 ceil(C / 256) + 6 is the longest chain of additions in a row sum (the values a lane
holds, then six wave levels).  With sigma = sqrt(var + eps), rstd = 1 / sigma, xhat = (x - mean) rstd, a = g (1 + scale):
  * rstd: the variance is a sum of non-negative terms of 3 roundings each ((x - mean), the square) -> relative (D + 3) u, the division by C and the + eps one each, halved
    by the root, then the root and the reciprocal: c_r = (D + 5) / 2 + 2.
  * xhat: the subtraction, the product and rstd: c_x = c_r + 2 relative - plus the ABSOLUTE error the fp32 mean costs: a row sum of values near 1e4 is off by a few ulps
    of max|x|, every x - mean moves by that amount and xhat by E = (max|x| / sigma) 2^-22, the factor of the forward bar.  The variance sees it in second order only.
  * dx_j = rstd ((a_j - m1) - xhat_j m2), m1 = mean(a), m2 = mean(a xhat):
      a_j carries 2 roundings (1 + scale, the product), then two subtractions, the product with rstd and rstd itself:            (5 + c_r) u rstd |a_j|
      m1: the terms' 2, the sum's D, the division, then the same four:                                                         (D + 7 + c_r) u rstd mean|a|
      m2: terms of 2 + c_x + 1, the sum's D, the division; then xhat_j's own c_x, the product, one subtraction, rstd:    (2 c_x + D + 7 + c_r) u rstd |xhat_j| mean|a xhat|
      the mean's E enters through xhat_j (times m2) and through every term of m2 (times xhat_j):                     rstd E (mean|a xhat| + |xhat_j| mean|a|)
  * column sums over l (and b): a term passes through at most `depth` additions: 8 rows per wave, 3 to add the waves, ceil(parts / 4) partial rows per slice of pass 2 and 3
    to add the slices (parts = ceil(L / 32), times B when the operand has one row).  dscale: terms g xhat of (c_x + 1) u each and |g| E absolute; dshift: exact terms g;
    dgamma: terms g y of one rounding and the factor row_scale[b] of one more.  Then one rounding to the operand's dtype (2^-24 / 2^-11 / 2^-8 relative; fp16 also half its
    smallest subnormal).
Nothing here was fitted to a kernel's output.  The condition that keeps the bounds honest is asserted by both test files: torch's float32 autograd ON THE CPU, on the
same inputs, meets every one of them."""
from __future__ import annotations

import functools
import math

import torch

from block_hard_cases import LN_EXACT_ROWS, LN_FAMILIES, LN_GROUPS, _ln_row
from conftest import rnd

U = 2.0 ** -24
EPS = 1e-6
CHUNK = 32                                     # engine.TRAIN_CHUNK, asserted equal by the host test
WIDTHS = (64, 260, 1024, 1028, 2048, 3072)     # each instantiation (C <= 1024 / 2048 / 3072), its upper edge, C % 8 != 0
SHAPES = tuple((C, B, L) for C in WIDTHS for B, L in ((1, 1), (2, 5), (3, 41))) + ((1024, 2, 681),)        # no L is a multiple of 4 or 32; (2, 681): 22 chunks per image
BWD_CASES = tuple(s + (False,) for s in SHAPES) + tuple((C, 3, 41, True) for C in WIDTHS)          # one_row: (1, 1, C) operands, summed over the images too
ROUND = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


@functools.lru_cache(maxsize=None)
def case(C: int, B: int, L: int):
    """(x (B, L, C), mod (B, 1, 6, C), row families, group families).  Row i of the B * L rows is of family (i + k) % 12 and image b of group (b + k) % 3, k = the
    index of C among WIDTHS, so that the small shapes cover every family and group between them."""
    k = WIDTHS.index(C) if C in WIDTHS else 0
    seed = 5000 + 7 * C + 3 * L + B
    fam = tuple(LN_FAMILIES[(i + k) % len(LN_FAMILIES)] for i in range(B * L))
    grp = tuple(LN_GROUPS[(b + k) % len(LN_GROUPS)] for b in range(B))
    x = torch.stack([_ln_row(f, seed + 1 + i, C) for i, f in enumerate(fam)]).view(B, L, C).contiguous()
    mod = rnd(seed, (B, 1, 6, C))
    for b, f in enumerate(grp):
        if f == "minus1":
            mod[b, 0, 2] = -1.0
        elif f == "pm30":
            mod[b, 0, 2] = 30.0 * torch.sign(mod[b, 0, 2])
    return x, mod, fam, grp


@functools.lru_cache(maxsize=None)
def upstream(C: int, B: int, L: int, big: float = 65536.0) -> torch.Tensor:
    """N(0, 1) of shape (B, L, C); row 0 x big, the middle row zero, the last row x -big (fewer rows: as many of the three as fit, in that order)."""
    g = rnd(777 + C + 5 * L + B, (B * L, C))
    n = B * L
    g[0] *= big
    if n >= 3:
        g[n // 2] = 0.0
    if n >= 2:
        g[n - 1] *= -big
    return g.view(B, L, C).contiguous()


def exact_rows(fam, grp, B: int, L: int) -> torch.Tensor:
    """(B, L) bool: rows whose output must equal shift bit for bit: constant-3.5 and zero rows, and every row of an image with scale == -1."""
    return torch.tensor([[fam[b * L + l] in LN_EXACT_ROWS or grp[b] == "minus1" for l in range(L)] for b in range(B)])


def _b(v: torch.Tensor, C: int) -> torch.Tensor:
    """A modulation vector (B, 1, C) / (1, 1, C) / (B, C) as it broadcasts against (B, L, C)."""
    return v.reshape(-1, 1, C)


def _stats(x64: torch.Tensor):
    mean = x64.mean(-1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(-1, keepdim=True)
    sig = torch.sqrt(var + EPS)
    return mean, sig, x64.abs().amax(-1, keepdim=True) / sig


def fwd_ref(x, scale, shift):
    """(ref, tol), float64, from the inputs as given (after any half rounding)."""
    C = x.shape[-1]
    x64, sc, sh = x.double(), _b(scale.double(), C), _b(shift.double(), C)
    mean, sig, spread = _stats(x64)
    ref = (x64 - mean) / sig * (1.0 + sc) + sh
    return ref, 2e-5 * ref.abs().clamp_min(1.0) + (1.0 + sc.abs()) * spread * 2.0 ** -22


def _autograd(x, scale, shift, g, dtype):
    """Autograd of torch's own expression ln(x).mul(scale.add(1)).add(shift) in `dtype` on the CPU -> (h, dx, dscale, dshift), the gradients in the operands' shapes."""
    C = x.shape[-1]
    with torch.enable_grad():
        xl, sl, hl = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, scale, shift))
        h = torch.nn.functional.layer_norm(xl, (C,), eps=EPS).mul(_b(sl, C).add(1)).add(_b(hl, C))
        return (h.detach(),) + torch.autograd.grad(h, (xl, sl, hl), g.to(dtype))


def bwd_ref(x, scale, shift, g):
    return _autograd(x, scale, shift, g, torch.float64)


def bwd_torch32(x, scale, shift, g):
    return _autograd(x.float(), scale.float(), shift.float(), g.float(), torch.float32)


def sum_depth(B: int, L: int, rows_out: int) -> int:
    parts = math.ceil(L / CHUNK) * (B if rows_out == 1 else 1)
    return CHUNK // 4 + 3 + math.ceil(parts / 4) + 3


def _rounded(tol0: torch.Tensor, ref: torch.Tensor, dtype) -> torch.Tensor:
    r = ROUND[dtype]
    return tol0 * (1.0 + r) + r * ref.abs() + (2.0 ** -25 if dtype == torch.float16 else 0.0)


def _over(t: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """(B, C) per-image sums -> the operand's shape (summed over the images when it has one row)."""
    return (t.sum(0, keepdim=True) if like.shape[0] == 1 else t).reshape(like.shape)


def bwd_bounds(x, scale, shift, g, refs):
    """(tol_dx, tol_dscale, tol_dshift) in the shapes of the gradients; refs = bwd_ref's (dx, dscale, dshift)."""
    B, L, C = x.shape
    x64, g64, s1 = x.double(), g.double(), 1.0 + _b(scale.double(), C)
    mean, sig, spread = _stats(x64)
    rstd, xh, a = 1.0 / sig, (x64 - mean) / sig, g64 * s1
    E = spread * 2.0 ** -22
    D = 4 * math.ceil(C / 256) + 6
    c_r = (D + 5) / 2 + 2
    c_x = c_r + 2
    ma, max_ = a.abs().mean(-1, keepdim=True), (a * xh).abs().mean(-1, keepdim=True)
    tol_dx = U * rstd * ((5 + c_r) * a.abs() + (D + 7 + c_r) * ma + (2 * c_x + D + 7 + c_r) * xh.abs() * max_) + rstd * E * (max_ + xh.abs() * ma)
    ds_img = (sum_depth(B, L, scale.shape[0]) + c_x + 1) * U * (g64 * xh).abs().sum(1) + (g64.abs() * E).sum(1)
    dh_img = sum_depth(B, L, shift.shape[0]) * U * g64.abs().sum(1)
    return tol_dx, _rounded(_over(ds_img, scale), refs[1], scale.dtype), _rounded(_over(dh_img, shift), refs[2], shift.dtype)


def gate_ref(x, y, gamma, row_scale, g):
    """fp64 (out, dy, dgamma) and their bounds (tol_out, tol_dy, tol_dgamma).  out = x + (y gamma) r: two products and a sum, one rounding each; dy = (g gamma) r: two
    roundings and the one to y's dtype; dgamma: see the module docstring."""
    B, L, C = x.shape
    x64, y64, g64, gm = x.double(), y.double(), g.double(), _b(gamma.double(), C)
    r = torch.ones(B, dtype=torch.float64) if row_scale is None else row_scale.double()
    r3 = r.view(B, 1, 1)
    t = y64 * gm * r3
    out = x64 + t
    tol_out = U * (out.abs() + 2.0 * t.abs()) * (1.0 + 4 * U)
    dy = g64 * gm * r3
    tol_dy = _rounded(2.0 * U * dy.abs(), dy, y.dtype)
    per_img = (g64 * y64).sum(1) * r.view(B, 1)
    dgamma = _over(per_img, gamma)
    tol_dg = _rounded(_over((sum_depth(B, L, gamma.shape[0]) + 2) * U * (g64 * y64).abs().sum(1) * r.view(B, 1), gamma), dgamma, gamma.dtype)
    return (out, dy, dgamma), (tol_out, tol_dy, tol_dg)


def gate_torch32(x, y, gamma, row_scale, g):
    """torch's float32 autograd on the CPU of x + (y * gamma) * row_scale -> (out, dy, dgamma)."""
    B, L, C = x.shape
    with torch.enable_grad():
        yl, gl = (t.detach().float().clone().requires_grad_(True) for t in (y, gamma))
        t = yl * _b(gl, C)
        if row_scale is not None:
            t = t * row_scale.float().view(B, 1, 1)
        out = x.float() + t
        return (out.detach(),) + torch.autograd.grad(out, (yl, gl), g.float())


def worst(name: str, got: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor) -> float:
    """Print and return the worst err / bound ratio over EVERY element (0 / 0 counts as 0: an exact result under a zero bound); the caller asserts it."""
    err = (got.detach().double().cpu().reshape(ref.shape) - ref).abs()
    bad = ~torch.isfinite(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    ratio = torch.where(bad, torch.full_like(err, float("inf")), ratio)
    w = float(ratio.max())
    i = int(ratio.argmax())
    print(f"  {name}: worst err/bound {w:.3f} (|err| {float(err.flatten()[i]):.3e}, bound {float(tol.flatten()[i]):.3e}, ref {float(ref.flatten()[i]):.3e})")
    return w
