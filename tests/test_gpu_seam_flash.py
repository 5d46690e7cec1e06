"""seam.flash_attn_func on the GPU (csrc/attention_sdpa_h.hip) against torch's SDPA in float64 on the CPU, on the operands already rounded to the half dtype.

err = max |got - ref|, u = 2^-11 (fp16) / 2^-8 (bf16).  Every case must meet BOTH bars:
  (a) derived worst case:  err <= u (max|ref| + max|v|) + [fp16 only] Lk 2^-25 max|v| + 2e-5 max(1, max|ref|)
      (one RNE rounding of the output: u |out|; RNE rounding of each p against an fp32 row sum: <= u max|v|; p below fp16's normal range loses at most 2^-25
      absolute each; the last term is the project's fp32 attention slack);
  (b) against the reference implementation:  err <= 2 e_torch + 2e-5, e_torch = the error against the same float64 result of torch's CPU SDPA run in the same
      half dtype on the same operands (a CPU emulation of the kernel's arithmetic contract measured 0.8-1.25 x e_torch at these shapes).
Each case prints err, e_torch and both bars."""
import ctypes as C
import math
import types

import pytest
import torch
import torch.nn.functional as F

from conftest import rnd
from sdvar_amd import engine as E
from sdvar_amd import seam

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
B0, H0 = 2, 3


def _u(dtype):
    return 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8


def _sdpa_blhc(q, k, v, scale):
    """torch SDPA on (B, L, H, c) CPU operands in their own dtype; returns (B, Lq, H, c)."""
    return F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), scale=scale).transpose(1, 2)


def _check(label, got, q, k, v, scale, dtype):
    """q, k, v: the CPU half operands (any strides).  got: the GPU result."""
    assert got.dtype == dtype and tuple(got.shape) == tuple(q.shape) and got.is_contiguous()
    ref = _sdpa_blhc(q.double(), k.double(), v.double(), scale)
    e_torch = (_sdpa_blhc(q, k, v, scale).double() - ref).abs().max().item()
    err = (got.cpu().double() - ref).abs().max().item()
    u, Lk = _u(dtype), k.shape[1]
    mref, mv = ref.abs().max().item(), v.double().abs().max().item()
    bar_a = u * (mref + mv) + (Lk * 2.0 ** -25 * mv if dtype == torch.float16 else 0.0) + 2e-5 * max(1.0, mref)
    bar_b = 2 * e_torch + 2e-5
    print(f"{label} {str(dtype)[6:]} Lq={q.shape[1]} Lk={Lk}: err {err:.3e}  e_torch {e_torch:.3e}  bar(a) {bar_a:.3e}  bar(b) {bar_b:.3e}")
    assert math.isfinite(err)
    assert err <= bar_a, f"{label}: err {err:.3e} > bar (a) {bar_a:.3e}"
    assert err <= bar_b, f"{label}: err {err:.3e} > bar (b) {bar_b:.3e} (e_torch {e_torch:.3e})"
    return err


def _shared(seed, L, dtype, B=B0, H=H0, norm=None):
    """One (B, L, 3, H, 64) CPU buffer in the half dtype, as the reference's qkv projection leaves it.  norm = m: q <- normalize(q) m, k <- normalize(k) (in fp32,
    before the rounding to the half dtype)."""
    buf = rnd(seed, (B, L, 3, H, 64))
    if norm is not None:
        buf[:, :, 0] = F.normalize(buf[:, :, 0], dim=-1) * norm
        buf[:, :, 1] = F.normalize(buf[:, :, 1], dim=-1)
    return buf.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_raw_views_across_a_query_block(dev, dtype):
    buf = _shared(11, 200, dtype)
    g = buf.to(dev)
    q, k, v = buf.unbind(dim=2)
    gq, gk, gv = g.unbind(dim=2)
    scale = 0.25 / 8
    got = seam.flash_attn_func(gq[:, :130], gk, gv, softmax_scale=scale)
    _check("views", got, q[:, :130], k, v, scale, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_normalised_small_stage_in_the_shared_buffer(dev, dtype):
    buf = _shared(12, 37, dtype, norm=4.0)
    g = buf.to(dev)
    gq, gk, gv = g.unbind(dim=2)
    assert not gq.is_contiguous() and not gk.is_contiguous() and not gv.is_contiguous()
    got = seam.flash_attn_func(gq, gk, gv, softmax_scale=1.0)
    q, k, v = buf.unbind(dim=2)
    _check("l2norm-37", got, q, k, v, 1.0, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cached_call(dev, dtype):
    q = _shared(13, 16, dtype)[:, :, 0]
    k, v = rnd(14, (B0, 91, H0, 64)).to(dtype), rnd(15, (B0, 91, H0, 64)).to(dtype)
    gq = _shared(13, 16, dtype).to(dev)[:, :, 0]
    assert not gq.is_contiguous()
    got = seam.flash_attn_func(gq, k.to(dev), v.to(dev), softmax_scale=0.125)
    _check("cached", got, q, k, v, 0.125, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Lq, Lk", [(1, 1), (5, 63), (5, 64), (5, 65)])
def test_tails(dev, dtype, Lq, Lk):
    q, k, v = rnd(16, (B0, Lq, H0, 64)).to(dtype), rnd(17, (B0, Lk, H0, 64)).to(dtype), rnd(18, (B0, Lk, H0, 64)).to(dtype)
    got = seam.flash_attn_func(q.to(dev), k.to(dev), v.to(dev), softmax_scale=0.125)
    _check("tail", got, q, k, v, 0.125, dtype)
    if (Lq, Lk) == (1, 1):
        assert torch.equal(got.cpu(), v)                     # softmax over one key is exactly 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_default_scale_is_one_over_sqrt_64(dev, dtype):
    g = _shared(19, 70, dtype).to(dev)
    gq, gk, gv = g.unbind(dim=2)
    assert torch.equal(seam.flash_attn_func(gq, gk, gv), seam.flash_attn_func(gq, gk, gv, softmax_scale=0.125))
    assert not torch.equal(seam.flash_attn_func(gq, gk, gv), seam.flash_attn_func(gq, gk, gv, softmax_scale=0.25))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mul, Lq, Lk", [(50.0, 130, 680), (100.0, 16, 680)])
def test_large_scores(dev, dtype, mul, Lq, Lk):
    """attn_l2_norm operands at the top of the reference's range: scale_mul is clamped at 100 (basic_var.py:71, 101)."""
    q = (F.normalize(rnd(20, (B0, Lq, H0, 64)), dim=-1) * mul).to(dtype)
    k = F.normalize(rnd(21, (B0, Lk, H0, 64)), dim=-1).to(dtype)
    v = rnd(22, (B0, Lk, H0, 64)).to(dtype)
    got = seam.flash_attn_func(q.to(dev), k.to(dev), v.to(dev), softmax_scale=1.0)
    _check(f"large x{mul:g}", got, q, k, v, 1.0, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cached_loop_over_the_ladder(dev, dtype):
    """The cached sampling loop: stage si brings pn^2 new tokens, the caches grow along the token axis, the new queries attend to everything cached so far."""
    B, H = 2, 2
    ck = cv = gk = gv = None
    for si, pn in enumerate((1, 2, 3, 4, 5, 6, 8, 10, 13, 16)):
        n = pn * pn
        q, k, v = (rnd(100 + 3 * si + j, (B, n, H, 64)).to(dtype) for j in range(3))
        ck, cv = (k, v) if ck is None else (torch.cat((ck, k), dim=1), torch.cat((cv, v), dim=1))
        gk, gv = (k.to(dev), v.to(dev)) if gk is None else (torch.cat((gk, k.to(dev)), dim=1), torch.cat((gv, v.to(dev)), dim=1))
        got = seam.flash_attn_func(q.to(dev), gk, gv, softmax_scale=0.125)
        _check(f"stage {si}", got, q, ck, cv, 0.125, dtype)
    assert ck.shape[1] == 680


@pytest.mark.parametrize("dtype", DTYPES)
def test_512_launch(dev, dtype):
    q, k, v = rnd(23, (1, 1024, 2, 64)).to(dtype), rnd(24, (1, 2240, 2, 64)).to(dtype), rnd(25, (1, 2240, 2, 64)).to(dtype)
    got = seam.flash_attn_func(q.to(dev), k.to(dev), v.to(dev), softmax_scale=0.125)
    _check("512^2", got, q, k, v, 0.125, dtype)


class _SelfAttention(torch.nn.Module):
    """A small re-enactment, written for this test, of how the reference's self-attention reaches the flash slot (basic_var.py:93-113): one qkv buffer, fp32 l2
    normalisation of q and k with a per-head multiplier, token-axis caches, operands cast to the projection's dtype, result viewed as (B, L, C)."""
    def __init__(self, ns, heads, dtype):
        super().__init__()
        self.ns, self.heads, self.dtype, self.using_flash = ns, heads, dtype, False
        C_ = heads * 64
        self.w = torch.nn.Parameter(rnd(31, (3 * C_, C_), 1.0 / math.sqrt(C_)), requires_grad=False)
        self.bias = torch.nn.Parameter(rnd(32, (3 * C_,), 0.1), requires_grad=False)
        self.scale_mul_1H11 = torch.nn.Parameter(torch.full((1, heads, 1, 1), 4.0).log(), requires_grad=False)
        self.cached_k = self.cached_v = None
        self.calls = []

    def forward(self, x):
        B, L, C_ = x.shape
        qkv = F.linear(x.to(self.dtype), self.w.to(self.dtype), self.bias.to(self.dtype)).view(B, L, 3, self.heads, 64)
        main_type = qkv.dtype
        assert self.using_flash and main_type != torch.float32
        q, k, v = qkv.unbind(dim=2)
        scale_mul = self.scale_mul_1H11.clamp_max(math.log(100)).exp().transpose(1, 2)
        q = F.normalize(q.float(), dim=-1).mul(scale_mul)
        k = F.normalize(k.float(), dim=-1)
        if self.cached_k is None:
            self.cached_k, self.cached_v = k, v
        else:
            k = self.cached_k = torch.cat((self.cached_k, k), dim=1)
            v = self.cached_v = torch.cat((self.cached_v, v), dim=1)
        ops = (q.to(dtype=main_type), k.to(dtype=main_type), v.to(dtype=main_type))
        out = self.ns.flash_attn_func(*ops, dropout_p=0.0, softmax_scale=1.0)
        self.calls.append((ops, out))
        return out.view(B, L, C_)


@pytest.mark.parametrize("dtype", DTYPES)
def test_reenactment_of_the_reference_call(dev, dtype):
    ns = types.SimpleNamespace(flash_attn_func=None)
    attn = _SelfAttention(ns, H0, dtype).to(dev)
    seam.enable_flash(ns, attn)
    assert ns.flash_attn_func is seam.flash_attn_func and attn.using_flash is True
    with torch.no_grad():
        for si, L in enumerate((4, 9)):
            y = attn(rnd(33 + si, (B0, L, H0 * 64)).to(dev))
            assert tuple(y.shape) == (B0, L, H0 * 64) and y.dtype == dtype
    for si, ((q, k, v), out) in enumerate(attn.calls):
        _check(f"re-enactment call {si}", out, q.cpu(), k.cpu(), v.cpu(), 1.0, dtype)
    assert attn.calls[1][0][1].shape[1] == 13


# ---------------------------------------------------------------------------------------------------------------- properties

@pytest.mark.parametrize("dtype", DTYPES)
def test_p_is_rounded_to_nearest(dev, dtype):
    """v == 1: the output is sum(round(p)) / sum(p).  Round-to-nearest leaves it at 1 within one output rounding; truncating p (cvt_pkrtz, a 16-bit shift) biases
    every row down by about u (fp16 emulation: mean -4.9e-4 = -2^-11)."""
    g = _shared(41, 200, dtype).to(dev)
    gq, gk, _ = g.unbind(dim=2)
    ones = torch.ones(B0, 200, H0, 64, dtype=dtype, device=dev)
    out = seam.flash_attn_func(gq[:, :130], gk, ones, softmax_scale=0.125).double()
    lo, hi, mean = out.min().item() - 1, out.max().item() - 1, (out - 1).mean().item()
    print(f"v=1 {str(dtype)[6:]}: min-1 {lo:.3e} max-1 {hi:.3e} mean-1 {mean:.3e}")
    below, above, bias = (2.0 ** -11, 2.0 ** -10, -2.0 ** -13) if dtype == torch.float16 else (2.0 ** -8, 2.0 ** -7, -2.0 ** -10)
    assert lo >= -below and hi <= above
    assert mean >= bias


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_invariance_and_determinism(dev, dtype):
    g = _shared(42, 150, dtype).to(dev)
    gq, gk, gv = g.unbind(dim=2)
    gq = gq[:, :70]
    a = seam.flash_attn_func(gq, gk, gv, softmax_scale=0.125)
    b = seam.flash_attn_func(gq.contiguous(), gk.contiguous(), gv.contiguous(), softmax_scale=0.125)
    c = seam.flash_attn_func(gq, gk, gv, softmax_scale=0.125)
    # a (B, H, L, 64) cache seen through a transpose, and an operand that breaks the alignment rule (copied once)
    d = seam.flash_attn_func(gq, gk.transpose(1, 2).contiguous().transpose(1, 2), gv, softmax_scale=0.125)
    odd = torch.empty(gq.numel() + 4, dtype=dtype, device=dev)[4:].view(gq.shape).copy_(gq)
    assert odd.data_ptr() % 16 != 0
    e = seam.flash_attn_func(odd, gk, gv, softmax_scale=0.125)
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d) and torch.equal(a, e)
    assert a.dtype == dtype and tuple(a.shape) == (B0, 70, H0, 64) and a.is_contiguous()


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_stray_stores(dev, dtype):
    """Rows past Lq of the last query block are never stored: sdvar_op_sdpa_h with Lq = 37 into a 64-row buffer."""
    Lq, Lk, rows = 37, 50, 64
    g = _shared(43, Lk, dtype).to(dev)
    gq, gk, gv = g.unbind(dim=2)
    gq = gq[:, :Lq]
    want = seam.flash_attn_func(gq, gk, gv, softmax_scale=0.125)
    sentinel = -1024.0                   # exact in both dtypes
    out = torch.full((B0, rows, H0, 64), sentinel, dtype=dtype, device=dev)
    strides = (C.c_int64 * 12)(*(t.stride(i) for t in (gq, gk, gv, out) for i in (0, 2, 1)))
    p = lambda t: C.c_void_p(t.data_ptr())
    E._check(E.load_library().sdvar_op_sdpa_h(p(gq), p(gk), p(gv), p(out), strides, 1 if dtype == torch.float16 else 2, B0, H0, Lq, Lk, 64, 0.125, E._stream()))
    torch.cuda.synchronize()
    assert torch.equal(out[:, :Lq], want)
    assert (out[:, Lq:] == sentinel).all()
