"""seam.slow_attn_amp / memory_efficient_attention_amp / install_amp on the GPU (sdvar_op_sdpa_hm, csrc/attention_sdpa_h.hip): masked attention on the half and
mixed operands torch.autocast delivers, against torch's SDPA in float64 on the CPU on the operands AS THE KERNEL SEES THEM (fp32 q / k rounded to the half dtype
with .to(dtype) first; the mask keeps its own values).

err = max |got - ref|, u = 2^-11 (fp16) / 2^-8 (bf16).  Every case must meet the two bars of test_gpu_seam_flash.py:
  (a) err <= u (max|ref| + max|v|) + [fp16 only] Lk 2^-25 max|v| + 2e-5 max(1, max|ref|);
  (b) err <= 2 e_torch + 2e-5, e_torch = the error against the same float64 result of torch's CPU SDPA run in the half dtype with the same mask.
Finite bias values stay within +-4, so the fp32 addition of the bias stays inside the 2e-5 slack.  (A CPU emulation of the contract at L = 55 under the five-stage
mask measured fp16 5.2e-4 against e_torch 5.0e-4 and bar (a) 3.7e-3; bf16 equal to e_torch.)  Each case prints err, e_torch and both bars."""
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
NEG = float("-inf")
LADDER5, LADDER10 = (1, 2, 3, 4, 5), (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)


def _u(dtype):
    return 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8


def block_causal(patch_nums):
    """models/var.py:108-113: a query of stage i sees the keys of stages <= i.  (1, 1, L, L) fp32, 0 / -inf."""
    d = torch.cat([torch.full((pn * pn,), i) for i, pn in enumerate(patch_nums)])
    return torch.where(d[:, None] >= d[None, :], 0.0, NEG).reshape(1, 1, len(d), len(d)).float()


def block_diagonal(L=130, cut=64):
    """Rows >= cut see only keys >= cut, rows < cut only keys < cut: the first visited tile is fully masked for the rows >= cut, and every row has a key."""
    r = torch.arange(L)
    return torch.where((r[:, None] >= cut) == (r[None, :] >= cut), 0.0, NEG).reshape(1, 1, L, L).float()


def _sdpa(q, k, v, scale, mask):
    return F.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=scale)


def _check(label, got, q, k, v, scale, mask, dtype, rows=None):
    """q, k, v: CPU operands (B, H, L, 64) as passed to the slot (fp32 or half); mask: the CPU mask as passed (or None).  got: the GPU result (B, H, Lq, 64).
    rows: the query rows to compare (default all)."""
    assert got.dtype == dtype and tuple(got.shape) == tuple(q.shape)
    qh, kh, vh = q.to(dtype), k.to(dtype), v.to(dtype)
    m64 = None if mask is None else (mask if mask.dtype == torch.bool else mask.double())
    ref = _sdpa(qh.double(), kh.double(), vh.double(), scale, m64)
    tor = _sdpa(qh, kh, vh, scale, mask).double()                  # the same mask, in its own dtype
    g = got.cpu().double()
    if rows is not None:
        ref, tor, g = ref[:, :, rows], tor[:, :, rows], g[:, :, rows]
    e_torch = (tor - ref).abs().max().item()
    err = (g - ref).abs().max().item()
    u, Lk = _u(dtype), k.shape[2]
    mref, mv = ref.abs().max().item(), vh.double().abs().max().item()
    bar_a = u * (mref + mv) + (Lk * 2.0 ** -25 * mv if dtype == torch.float16 else 0.0) + 2e-5 * max(1.0, mref)
    bar_b = 2 * e_torch + 2e-5
    print(f"{label} {str(dtype)[6:]} Lq={q.shape[2]} Lk={Lk}: err {err:.3e}  e_torch {e_torch:.3e}  bar(a) {bar_a:.3e}  bar(b) {bar_b:.3e}")
    assert math.isfinite(err), f"{label}: err {err}"
    assert err <= bar_a, f"{label}: err {err:.3e} > bar (a) {bar_a:.3e}"
    assert err <= bar_b, f"{label}: err {err:.3e} > bar (b) {bar_b:.3e} (e_torch {e_torch:.3e})"
    return err


def _buffer(seed, L, B=B0, H=H0, norm=None):
    """One (B, L, 3, H, 64) fp32 CPU buffer.  norm = m: q <- normalize(q) m, k <- normalize(k), as attn_l2_norm leaves them."""
    buf = rnd(seed, (B, L, 3, H, 64))
    if norm is not None:
        buf[:, :, 0] = F.normalize(buf[:, :, 0], dim=-1) * norm
        buf[:, :, 1] = F.normalize(buf[:, :, 1], dim=-1)
    return buf


def _split(buf):
    """(q, k, v) as (B, H, L, 64) views of a (B, L, 3, H, 64) buffer: the reference's non-flash layout (basic_var.py:99)."""
    return buf.permute(2, 0, 3, 1, 4).unbind(0)


def _views(seed, L, B=B0, H=H0, norm=None):
    return _split(_buffer(seed, L, B, H, norm))


def _dev_views(ops, dtypes, dev):
    """Each operand cast to its dtype on the CPU, moved to the GPU with its strides kept (a permuted view of a dense (B, L, H, 64) tensor)."""
    out = []
    for t, dt in zip(ops, dtypes):
        out.append(t.permute(0, 2, 1, 3).contiguous().to(dt).to(dev).permute(0, 2, 1, 3))
    return out


def _mixed_mask(Lq=130, Lk=150):
    """fp32 (1, 1, Lq, Lk): finite values within +-4 mixed with -inf; key 0 stays visible for every row."""
    m = rnd(70, (1, 1, Lq, Lk)).clamp(-4, 4)
    hole = rnd(71, (1, 1, Lq, Lk)) > 0.3
    hole[..., 0] = False
    return m.masked_fill(hole, NEG)


_p = lambda t: None if t is None else C.c_void_p(t.data_ptr())


def _raw(q, k, v, out, dtype, mask=None, kind=0, smap=None, scale=1.0):
    """sdvar_op_sdpa_hm on (B, H, L, 64) device tensors; mask (mb, mh, Lq, Lk) with key stride 1 (uint8 for a keep-mask)."""
    B, H, Lq, _ = q.shape
    strides = (C.c_int64 * 12)(*(t.stride(i) for t in (q, k, v, out) for i in (0, 1, 2)))
    bstr = None if mask is None else (C.c_int64 * 3)(*(0 if n == 1 else s for n, s in zip(mask.shape[:3], mask.stride()[:3])))
    E._check(E.load_library().sdvar_op_sdpa_hm(_p(q), _p(k), _p(v), _p(out), strides, 1 if dtype == torch.float16 else 2, int(q.dtype == torch.float32),
                                               int(k.dtype == torch.float32), _p(mask), kind, bstr, _p(smap), B, H, Lq, k.shape[2], 64, scale, E._stream()))
    torch.cuda.synchronize()
    return out


def _raw_skip_map(mask, kind, Lq, Lk):
    smap = torch.full((((Lq + 127) // 128) * ((Lk + 63) // 64),), 7, dtype=torch.uint8, device=mask.device)
    bstr = (C.c_int64 * 3)(*(0 if n == 1 else s for n, s in zip(mask.shape[:3], mask.stride()[:3])))
    E._check(E.load_library().sdvar_op_sdpa_skip_map(_p(mask), kind, bstr, mask.shape[0], mask.shape[1], Lq, Lk, _p(smap), E._stream()))
    torch.cuda.synchronize()
    return smap


def _host_skip_map(mask, Lq, Lk):
    """1 where the (128-query, 64-key) tile is masked in every batch / head slice of the CPU mask."""
    vis = (mask != NEG) if mask.dtype != torch.bool else mask
    vis = vis.reshape(-1, Lq, Lk).any(0)
    return [[int(not vis[qb * 128:(qb + 1) * 128, kt * 64:(kt + 1) * 64].any()) for kt in range((Lk + 63) // 64)] for qb in range((Lq + 127) // 128)]


def _cached_skip_map(mask_dev):
    return next(e[1] for e in seam._SKIP_MAPS.values() if e[0].data_ptr() == mask_dev.data_ptr() and e[0].shape[-2:] == mask_dev.shape[-2:]).cpu()


# ----------------------------------------------------------------------------------------------------------------- cases 1-3

@pytest.mark.parametrize("dtype", DTYPES)
def test_five_stage_mask_l2_normalised_mixed_operands(dev, dtype):
    """Case 1 (+ 3): q / k fp32 and l2-normalised x 4, v half, L = 55: permuted views of one buffer and contiguous tensors, bit-identical; fp32 q / k in the kernel
    equal q.to(dtype) / k.to(dtype) passed as half, bit for bit."""
    m = block_causal(LADDER5)
    buf = _buffer(51, 55, norm=4.0)
    q, k, v = _split(buf)
    (gq, gk, _), (_, _, gv) = _split(buf.to(dev)), _split(buf.to(dtype).to(dev))          # q / k views of the fp32 buffer, v of its half copy
    assert not gq.is_contiguous() and not gk.is_contiguous() and not gv.is_contiguous()
    md = m.to(dev)
    got = seam.slow_attn_amp(gq, gk, gv, 1, attn_mask=md)
    assert got.dtype == dtype and got.permute(0, 2, 1, 3).is_contiguous()
    _check("five-stage", got, q, k, v, 1.0, m, dtype)
    assert torch.equal(got, seam.slow_attn_amp(gq.contiguous(), gk.contiguous(), gv.contiguous(), 1, attn_mask=md))
    assert torch.equal(got, seam.slow_attn_amp(gq.to(dtype), gk, gv, 1, attn_mask=md))
    assert torch.equal(got, seam.slow_attn_amp(gq, gk.to(dtype), gv, 1, attn_mask=md))
    assert torch.equal(got, seam.slow_attn_amp(gq.to(dtype), gk.to(dtype), gv, 1, attn_mask=md))
    assert _cached_skip_map(md).tolist() == [0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_blocks_three_tiles_every_operand_mix(dev, dtype):
    """Cases 2 + 3: Lq 130 on Lk 150, an fp32 mask of finite values and -inf; q-only-fp32, k-only-fp32, both, neither: each within the bars, all four the same bits
    (the in-kernel rounding is round-to-nearest-even, the bits of .to(dtype))."""
    m = _mixed_mask()
    q, k, v = _views(52, 150)
    q = q[:, :, :130]
    md = m.to(dev)
    scale = 0.125
    outs = []
    for qd, kd in ((torch.float32, dtype), (dtype, torch.float32), (torch.float32, torch.float32), (dtype, dtype)):
        gq, gk, gv = _dev_views((q, k, v), (qd, kd, dtype), dev)
        outs.append(seam.slow_attn_amp(gq, gk, gv, scale, attn_mask=md))
        _check(f"mixed q {str(qd)[6:]} k {str(kd)[6:]}", outs[-1], q, k, v, scale, m, dtype)
    assert all(torch.equal(outs[0], o) for o in outs[1:])


# ----------------------------------------------------------------------------------------------------------------- cases 4-6

@pytest.mark.parametrize("dtype", DTYPES)
def test_first_visited_tile_fully_masked_for_some_rows(dev, dtype):
    """Cases 4 + 6: block-diagonal mask at L = 130.  Rows 64..127 share their workgroup with rows 0..63, so tile 0 is visited and is all -inf for them: their
    running maximum is still -inf after it.  Finite, within the bars, and the same bits with and without the skip map."""
    m = block_diagonal()
    q, k, v = _views(53, 130)
    gq, gk, gv = _dev_views((q, k, v), (torch.float32, dtype, dtype), dev)
    md = m.to(dev)
    got = seam.slow_attn_amp(gq, gk, gv, 0.125, attn_mask=md)
    assert torch.isfinite(got).all()
    _check("block-diagonal", got, q, k, v, 0.125, m, dtype)
    smap = _raw_skip_map(md, 1, 130, 130)
    assert smap.cpu().reshape(2, 3).tolist() == _host_skip_map(m, 130, 130) == [[0, 0, 0], [1, 0, 0]]
    for sm in (smap, None):
        out = torch.zeros(B0, 130, H0, 64, dtype=dtype, device=dev).permute(0, 2, 1, 3)
        assert torch.equal(_raw(gq, gk, gv, out, dtype, md, 1, sm, 0.125), got)


@pytest.fixture(scope="module")
def ten_stage():
    m = block_causal(LADDER10)
    q, k, v = _views(54, 680, B=1, H=2, norm=4.0)
    return m, q, k, v


@pytest.mark.parametrize("dtype", DTYPES)
def test_ten_stage_mask_and_its_verify_chunk(dev, dtype, ten_stage):
    """Cases 5 + 6: L = 680 under the ten-stage mask, and rows [255:] of the same mask as a verify chunk (Lq 425 on Lk 680; the bias view starts 255 rows into its
    buffer).  The skip map used equals a host-computed one; the result is the same bits with the map and without."""
    m, q, k, v = ten_stage
    md = m.to(dev)
    gq, gk, gv = _dev_views((q, k, v), (torch.float32, torch.float32, dtype), dev)
    got = seam.slow_attn_amp(gq, gk, gv, 1.0, attn_mask=md)
    _check("ten-stage", got, q, k, v, 1.0, m, dtype)
    host = _host_skip_map(m, 680, 680)
    assert _cached_skip_map(md).reshape(6, 11).tolist() == host and sum(map(sum, host)) == 16
    out = torch.zeros(1, 680, 2, 64, dtype=dtype, device=dev).permute(0, 2, 1, 3)
    assert torch.equal(_raw(gq, gk, gv, out, dtype, md, 1, None, 1.0), got)
    # the verify chunk
    ms, msd = m[:, :, 255:, :], md[:, :, 255:, :]
    assert msd.data_ptr() != md.data_ptr()
    got2 = seam.slow_attn_amp(gq[:, :, 255:], gk, gv, 1.0, attn_mask=msd)
    _check("verify chunk", got2, q[:, :, 255:], k, v, 1.0, ms, dtype)
    host2 = _host_skip_map(ms, 425, 680)
    assert _cached_skip_map(msd).reshape(4, 11).tolist() == host2 and sum(map(sum, host2)) > 0
    out2 = torch.zeros(1, 425, 2, 64, dtype=dtype, device=dev).permute(0, 2, 1, 3)
    assert torch.equal(_raw(gq[:, :, 255:], gk, gv, out2, dtype, msd, 1, None, 1.0), got2)


# ----------------------------------------------------------------------------------------------------------------- cases 7-9

@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_kinds_agree(dev, dtype):
    """Case 7: a bool keep-mask, the fp32 0 / -inf mask and the same mask in the half dtype give the same bits, on aligned rows (vector loads) and on a sliced view
    with odd row starts (element loads); a finite half bias matches its .float() copy bit for bit."""
    q, k, v = _views(55, 150)
    q = q[:, :, :130]
    gq, gk, gv = _dev_views((q, k, v), (torch.float32, dtype, dtype), dev)
    big = block_causal(LADDER10)[:, :, :152, :152].contiguous().to(dev)          # rows of 152 elements: 16-byte aligned in all three formats
    big_keep, big_half = big == 0, big.to(dtype)
    for label, cut in (("aligned", (slice(14, 144), slice(0, 150))), ("sliced", (slice(15, 145), slice(1, 151)))):
        md, mk, mh = (t[:, :, cut[0], cut[1]] for t in (big, big_keep, big_half))
        assert tuple(md.shape) == (1, 1, 130, 150) and md.stride() == mk.stride() == mh.stride() and md.stride(2) == 152
        a = seam.slow_attn_amp(gq, gk, gv, 0.125, attn_mask=md)
        b = seam.slow_attn_amp(gq, gk, gv, 0.125, attn_mask=mk)
        c = seam.slow_attn_amp(gq, gk, gv, 0.125, attn_mask=mh)
        assert torch.equal(a, b) and torch.equal(a, c), label
        _check(f"kinds {label}", a, q, k, v, 0.125, md.cpu(), dtype)
    fin = _mixed_mask().to(dtype)
    fd = fin.to(dev)
    a = seam.slow_attn_amp(gq, gk, gv, 0.125, attn_mask=fd)
    assert torch.equal(a, seam.slow_attn_amp(gq, gk, gv, 0.125, attn_mask=fd.float()))
    _check("half bias", a, q, k, v, 0.125, fin.float(), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_per_head_bias_keeps_the_tile_one_head_needs(dev, dtype):
    """Case 8: a (1, H, Lq, Lk) bias in which heads 0 and 1 mask every key >= 64 and head 2 masks nothing: tiles 1 and 2 are needed by head 2 only."""
    L = 130
    m = torch.zeros(1, H0, L, L)
    m[:, :2, :, 64:] = NEG
    q, k, v = _views(56, L)
    gq, gk, gv = _dev_views((q, k, v), (dtype, torch.float32, dtype), dev)
    md = m.to(dev)
    got = seam.slow_attn_amp(gq, gk, gv, 0.125, attn_mask=md)
    _check("per-head", got, q, k, v, 0.125, m, dtype)
    for h in range(H0):
        _check(f"per-head h{h}", got[:, h:h + 1], q[:, h:h + 1], k[:, h:h + 1], v[:, h:h + 1], 0.125, m[:, h:h + 1], dtype)
    assert _cached_skip_map(md).tolist() == [0] * 6


@pytest.mark.parametrize("dtype", DTYPES)
def test_expanded_half_bias_through_the_xformers_slot(dev, dtype):
    """Case 9: what basic_var.py:115 passes: q, k, v (B, L, H, 64) and attn_bias.to(dtype).expand(B, H, -1, -1) with batch and head strides 0."""
    m = block_causal(LADDER5)
    q, k, v = _views(57, 55, norm=4.0)
    gq, gk, gv = _dev_views((q, k, v), (dtype, dtype, dtype), dev)
    mh = m.to(dev).to(dtype)
    bias = mh.expand(B0, H0, -1, -1)
    assert bias.stride()[:2] == (0, 0)
    got = seam.memory_efficient_attention_amp(gq.transpose(1, 2), gk.transpose(1, 2), gv.transpose(1, 2), attn_bias=bias, scale=1.0)
    assert tuple(got.shape) == (B0, 55, H0, 64) and got.is_contiguous() and got.dtype == dtype
    assert torch.equal(got.transpose(1, 2), seam.slow_attn_amp(gq, gk, gv, 1.0, attn_mask=mh))
    assert any(e[0].data_ptr() == mh.data_ptr() and e[0].stride()[:2] == (0, 0) for e in seam._SKIP_MAPS.values())          # read through its strides
    _check("expanded bias", got.transpose(1, 2), q, k, v, 1.0, m, dtype)
    # the default scale of the slot is 1 / sqrt(64)
    assert torch.equal(seam.memory_efficient_attention_amp(gq.transpose(1, 2), gk.transpose(1, 2), gv.transpose(1, 2), attn_bias=bias),
                       seam.memory_efficient_attention_amp(gq.transpose(1, 2), gk.transpose(1, 2), gv.transpose(1, 2), attn_bias=bias, scale=0.125))


# --------------------------------------------------------------------------------------------------------------- cases 10-13

@pytest.mark.parametrize("dtype", DTYPES)
def test_large_scores_masked(dev, dtype):
    """Case 10: q normalised x 100, the clamp of scale_mul (basic_var.py:71, 102)."""
    m = _mixed_mask()
    q, k, v = _views(58, 150, norm=100.0)
    q = q[:, :, :130]
    gq, gk, gv = _dev_views((q, k, v), (torch.float32, torch.float32, dtype), dev)
    _check("large x100", seam.slow_attn_amp(gq, gk, gv, 1.0, attn_mask=m.to(dev)), q, k, v, 1.0, m, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dispatch(dev, dtype):
    """Case 11: all-fp32 operands are seam.slow_attn (same bits, fp32 result); all-half operands without a mask are seam.flash_attn_func's launch (same bits)."""
    m = block_causal(LADDER5).to(dev)
    q, k, v = _views(59, 55)
    fq, fk, fv = _dev_views((q, k, v), (torch.float32,) * 3, dev)
    a = seam.slow_attn_amp(fq, fk, fv, 0.125, attn_mask=m)
    assert a.dtype == torch.float32 and torch.equal(a, seam.slow_attn(fq, fk, fv, 0.125, attn_mask=m))
    hq, hk, hv = _dev_views((q, k, v), (dtype,) * 3, dev)
    b = seam.slow_attn_amp(hq, hk, hv, 0.125)
    assert b.dtype == dtype
    assert torch.equal(b.transpose(1, 2), seam.flash_attn_func(hq.transpose(1, 2), hk.transpose(1, 2), hv.transpose(1, 2), softmax_scale=0.125))
    # mixed operands without a mask: the rounding happens in the kernel, the arithmetic is the flash kernel's
    assert torch.equal(b, seam.slow_attn_amp(fq, fk, hv, 0.125))
    _check("no mask, mixed", seam.slow_attn_amp(fq, hk, hv, 0.125), q, k, v, 0.125, None, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_fully_masked_row(dev, dtype):
    """Case 12: row 9 has no key.  Its value is not asserted; every other row is within the bars."""
    m = block_causal(LADDER5).clone()
    m[:, :, 9, :] = NEG
    q, k, v = _views(60, 55)
    gq, gk, gv = _dev_views((q, k, v), (torch.float32, torch.float32, dtype), dev)
    got = seam.slow_attn_amp(gq, gk, gv, 0.125, attn_mask=m.to(dev))
    torch.cuda.synchronize()
    _check("masked row", got, q, k, v, 0.125, m, dtype, rows=[r for r in range(55) if r != 9])


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_stray_stores(dev, dtype):
    """Case 13: Lq = 37 rows written into a 64-row output carved from the middle of a sentinel-filled buffer: rows past Lq and the bytes around the output stay
    untouched, and repeated calls give the same bits."""
    Lq, Lk, rows, pad = 37, 55, 64, 256
    m = block_causal(LADDER5)[:, :, :Lq, :].contiguous()
    q, k, v = _views(61, Lk)
    gq, gk, gv = _dev_views((q[:, :, :Lq], k, v), (torch.float32, torch.float32, dtype), dev)
    md = m.to(dev)
    want = seam.slow_attn_amp(gq, gk, gv, 0.125, attn_mask=md)
    _check("sentinel", want, q[:, :, :Lq], k, v, 0.125, m, dtype)
    sentinel = -1024.0                   # exact in both dtypes
    n = B0 * rows * H0 * 64
    flat = torch.full((pad + n + pad,), sentinel, dtype=dtype, device=dev)
    out = flat[pad:pad + n].view(B0, rows, H0, 64).permute(0, 2, 1, 3)
    assert out.data_ptr() % 16 == 0
    smap = _raw_skip_map(md, 1, Lq, Lk)
    for _ in range(2):
        _raw(gq, gk, gv, out, dtype, md, 1, smap, 0.125)
        assert torch.equal(out[:, :, :Lq], want)
        assert (out[:, :, Lq:] == sentinel).all() and (flat[:pad] == sentinel).all() and (flat[pad + n:] == sentinel).all()


# --------------------------------------------------------------------------------------------------------------------- case 14

class _SelfAttention(torch.nn.Module):
    """A small re-enactment, written for this test, of how the reference's self-attention reaches the slow_attn slot (basic_var.py:93-117) when it runs under
    torch.autocast: one qkv projection, the non-flash (B, H, L, c) layout, l2 normalisation of q and k with an fp32 per-head multiplier, caches concatenated along
    dim 2, the mask passed on as it is, the result viewed as (B, L, C)."""
    def __init__(self, ns, heads):
        super().__init__()
        self.ns, self.heads = ns, heads
        C_ = heads * 64
        self.w = torch.nn.Parameter(rnd(31, (3 * C_, C_), 1.0 / math.sqrt(C_)), requires_grad=False)
        self.bias = torch.nn.Parameter(rnd(32, (3 * C_,), 0.1), requires_grad=False)
        self.scale_mul_1H11 = torch.nn.Parameter(torch.full((1, heads, 1, 1), 4.0).log(), requires_grad=False)
        self.caching, self.cached_k, self.cached_v = False, None, None
        self.calls = []

    def kv_caching(self, enable):
        self.caching, self.cached_k, self.cached_v = enable, None, None

    def forward(self, x, attn_bias):
        B, L, C_ = x.shape
        qkv = F.linear(x, self.w, self.bias).view(B, L, 3, self.heads, 64)
        q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(dim=0)
        scale_mul = self.scale_mul_1H11.clamp_max(math.log(100)).exp()
        q = F.normalize(q, dim=-1).mul(scale_mul)
        k = F.normalize(k, dim=-1)
        if self.caching:
            if self.cached_k is None:
                self.cached_k, self.cached_v = k, v
            else:
                k = self.cached_k = torch.cat((self.cached_k, k), dim=2)
                v = self.cached_v = torch.cat((self.cached_v, v), dim=2)
        out = self.ns.slow_attn(query=q, key=k, value=v, scale=1, attn_mask=attn_bias, dropout_p=0.0)
        self.calls.append(((q, k, v), attn_bias, out))
        return out.transpose(1, 2).reshape(B, L, C_), qkv.dtype


@pytest.mark.parametrize("dtype", DTYPES)
def test_reenactment_under_autocast(dev, dtype):
    ns = types.SimpleNamespace(slow_attn=None, fused_mlp_func=None, flash_attn_func=None)
    attn = _SelfAttention(ns, H0).to(dev)
    seam.install_amp(ns, attn)
    assert ns.slow_attn is seam.slow_attn_amp
    m5 = block_causal(LADDER5).to(dev)
    m9 = torch.zeros(1, 1, 9, 14)
    m9[:, :, :4, 9:] = NEG
    m9[:, :, :, 2] = NEG
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        y, main_type = attn(rnd(33, (B0, 55, H0 * 64)).to(dev), m5)                 # the teacher-forced pass
        assert main_type == dtype and y.dtype == dtype and tuple(y.shape) == (B0, 55, H0 * 64)
        attn.kv_caching(True)
        for si, L in enumerate((1, 4)):                                             # two cached, unmasked steps
            y, _ = attn(rnd(34 + si, (B0, L, H0 * 64)).to(dev), None)
            assert y.dtype == dtype and tuple(y.shape) == (B0, L, H0 * 64)
        y, _ = attn(rnd(36, (B0, 9, H0 * 64)).to(dev), m9.to(dev))                  # a masked cached call: Lq 9 on Lk 14
        assert y.dtype == dtype
    assert len(attn.calls) == 4 and attn.calls[3][0][1].shape[2] == 14
    for ci, ((q, k, v), bias, out) in enumerate(attn.calls):
        print(f"call {ci}: query {q.dtype} key {k.dtype} value {v.dtype} mask {None if bias is None else bias.dtype}")
        assert v.dtype == dtype and q.dtype == torch.float32 and k.dtype in (torch.float32, dtype) and out.dtype == dtype
        _check(f"re-enactment call {ci}", out, q.cpu(), k.cpu(), v.cpu(), 1.0, None if bias is None else bias.cpu(), dtype)
