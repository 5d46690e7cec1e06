"""sdvar_amd.seam on the GPU: slow_attn / memory_efficient_attention / fused_mlp_func against torch in float64 on the CPU.

Bar of every attention case: the project's attention bar err <= 2e-5 * max(1, max|ref|) (torch's own fp32 SDPA stays below 1.2e-6 on these inputs on the CPU),
except the large-score case, whose bar is 4x the error torch's fp32 SDPA makes on the same inputs (computed here).  Unless stated otherwise q, k, v are the
reference's views of ONE (B, L, 3, H, 64) buffer (basic_var.py:93-99): permuted, never contiguous."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rnd
from sdvar_amd import engine as E
from sdvar_amd import seam

pytestmark = pytest.mark.gpu
NEG = float("-inf")
LADDER10 = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)


def _views(seed, B, L, H, dev):
    """-> (q, k, v) device views (B, H, L, 64) of one (B, L, 3, H, 64) buffer, and the same on the CPU."""
    qkv = rnd(seed, (B, L, 3, H, 64))
    return qkv.to(dev).permute(2, 0, 3, 1, 4).unbind(0), qkv.permute(2, 0, 3, 1, 4).unbind(0)


def _ref(q, k, v, scale, mask=None):
    m = None if mask is None else (mask if mask.dtype == torch.bool else mask.double())
    return F.scaled_dot_product_attention(q.double(), k.double(), v.double(), attn_mask=m, scale=scale)


def _check(got, ref, rows=None, bar=None):
    got = got.cpu().double()
    assert got.shape == ref.shape
    if rows is not None:
        got, ref = got[:, :, rows], ref[:, :, rows]
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    lim = 2e-5 * max(1.0, ref.abs().max().item()) if bar is None else bar
    print(f"err {err:.3e} bar {lim:.3e}")
    assert err <= lim, (err, lim)


def block_causal(patch_nums):
    """models/var.py:108-113: a query of stage i sees the keys of stages <= i.  (1, 1, L, L) fp32, 0 / -inf."""
    d = torch.cat([torch.full((pn * pn,), i) for i, pn in enumerate(patch_nums)])
    return torch.where(d[:, None] >= d[None, :], 0.0, NEG).reshape(1, 1, len(d), len(d)).float()


# ------------------------------------------------------------------------------------------------------------------ no mask
def test_no_mask_l2_normalised(dev):
    qkv = rnd(1, (2, 37, 3, 2, 64))
    qkv[:, :, 0] = F.normalize(qkv[:, :, 0], dim=-1) * 4                    # q as attn_l2_norm leaves it (basic_var.py:104), still inside the shared buffer
    q, k, v = qkv.to(dev).permute(2, 0, 3, 1, 4).unbind(0)
    assert not q.is_contiguous() and not k.is_contiguous()
    _check(seam.slow_attn(q, k, v, 1), _ref(*qkv.permute(2, 0, 3, 1, 4).unbind(0), 1.0))


def test_no_mask_raw_inputs_uneven_lengths(dev):
    (q, k, v), (qc, kc, vc) = _views(2, 2, 200, 2, dev)
    s = 0.25 / math.sqrt(64)
    _check(seam.slow_attn(q[:, :, :130], k, v, s), _ref(qc[:, :, :130], kc, vc, s))


def test_cached_call_contiguous_kv(dev):
    (q, _, _), (qc, _, _) = _views(3, 2, 16, 2, dev)
    kc, vc = rnd(4, (2, 2, 91, 64)), rnd(5, (2, 2, 91, 64))             # the concatenated caches: contiguous (B, H, Lk, 64)
    _check(seam.slow_attn(q, kc.to(dev), vc.to(dev), 1.0), _ref(qc, kc, vc, 1.0))


def test_single_token(dev):
    (q, k, v), (qc, kc, vc) = _views(6, 2, 1, 2, dev)
    _check(seam.slow_attn(q, k, v, 0.5), _ref(qc, kc, vc, 0.5))


# ------------------------------------------------------------------------------------------------------------------ block-causal masks
@pytest.fixture(scope="module")
def mask680(dev):
    m = block_causal(LADDER10)
    return m, m.to(dev)


def test_block_causal_five_stages(dev):
    m = block_causal((1, 2, 3, 4, 5))
    (q, k, v), (qc, kc, vc) = _views(7, 2, 55, 2, dev)
    _check(seam.slow_attn(q, k, v, 1.0, attn_mask=m.to(dev)), _ref(qc, kc, vc, 1.0, m))


def test_block_causal_ten_stages(dev, mask680):
    m, md = mask680
    (q, k, v), (qc, kc, vc) = _views(8, 1, 680, 2, dev)
    _check(seam.slow_attn(q, k, v, 1.0, attn_mask=md), _ref(qc, kc, vc, 1.0, m))
    smap = next(e[1] for e in seam._SKIP_MAPS.values() if e[0].data_ptr() == md.data_ptr()).cpu().reshape(6, 11)
    # stage boundaries 0 1 5 14 30 55 91 155 255 424 680: queries 0..127 see keys < 155, so key tiles 3.. are skipped for them; the last block sees everything
    assert smap[0].tolist() == [0, 0, 0] + [1] * 8 and smap[1].tolist() == smap[2].tolist() == [0] * 7 + [1] * 4 and smap[3:].sum() == 0


def test_block_causal_sliced_view(dev, mask680):
    m, md = mask680
    ms, msd = m[:, :, :424, :424], md[:, :, :424, :424]
    assert not msd.is_contiguous()
    (q, k, v), (qc, kc, vc) = _views(9, 1, 424, 2, dev)
    _check(seam.slow_attn(q, k, v, 1.0, attn_mask=msd), _ref(qc, kc, vc, 1.0, ms))


# ------------------------------------------------------------------------------------------------------------------ finite bias, -inf handling
def _finite_bias(variant):
    b = rnd(10, (2, 2, 70, 130), 3.0)
    b[..., 64:128] = NEG                               # a whole key tile masked for every batch and head: skipped
    if variant >= 1:                                   # the -inf running-max case: row 5's first tile is all -inf while the other rows of its workgroup need it
        b[:, :, 5, :] = NEG
        b[:, :, 5, 77] = 0.75
    if variant >= 2:
        b[:, :, 9, :] = NEG                            # a fully masked row: value outside the contract
    return b


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_finite_bias_with_masked_tile(dev, variant):
    b = _finite_bias(variant)
    bd = b.to(dev)
    (q, k, v), (qc, kc, vc) = _views(11, 2, 130, 2, dev)
    got = seam.slow_attn(q[:, :, :70], k, v, 1.0, attn_mask=bd)             # must not raise
    torch.cuda.synchronize()
    rows = [r for r in range(70) if r != 9] if variant == 2 else None
    _check(got, _ref(qc[:, :, :70], kc, vc, 1.0, b), rows=rows)
    smap = next(e[1] for e in seam._SKIP_MAPS.values() if e[0].data_ptr() == bd.data_ptr()).cpu().tolist()
    assert smap == [0, 1 if variant == 0 else 0, 0]                    # key 77 of row 5 keeps tile 1 alive in variants 1 and 2


def test_bool_mask(dev):
    g = torch.Generator().manual_seed(12)
    keep = torch.rand(1, 1, 70, 130, generator=g) < 0.4
    keep[..., 0] = True
    keep[..., 64:128] &= False                         # one tile fully masked
    (q, k, v), (qc, kc, vc) = _views(13, 2, 130, 2, dev)
    _check(seam.slow_attn(q[:, :, :70], k, v, 1.0, attn_mask=keep.to(dev)), _ref(qc[:, :, :70], kc, vc, 1.0, keep))


def test_per_head_bias_skip_map_is_per_mask_not_per_head(dev):
    b = rnd(14, (1, 2, 70, 130), 2.0)
    b[:, 0, :, 0:64] = NEG                             # head 0 never sees tile 0, head 1 never sees tile 1: neither may be skipped
    b[:, 1, :, 64:128] = NEG
    bd = b.to(dev)
    (q, k, v), (qc, kc, vc) = _views(15, 2, 130, 2, dev)
    _check(seam.slow_attn(q[:, :, :70], k, v, 1.0, attn_mask=bd), _ref(qc[:, :, :70], kc, vc, 1.0, b))
    smap = next(e[1] for e in seam._SKIP_MAPS.values() if e[0].data_ptr() == bd.data_ptr()).cpu().tolist()
    assert smap == [0, 0, 0]


# ------------------------------------------------------------------------------------------------------------------ large scores
@pytest.mark.parametrize("k_normalised", [True, False])
def test_large_scores(dev, k_normalised):
    (q, k, v), (qc, kc, vc) = _views(16, 2, 130, 2, dev)
    qc = F.normalize(qc, dim=-1) * 50
    kc = F.normalize(kc, dim=-1) if k_normalised else kc
    ref = _ref(qc, kc, vc, 1.0)
    torch_err = (F.scaled_dot_product_attention(qc, kc, vc, scale=1.0).double() - ref).abs().max().item()
    _check(seam.slow_attn(qc.to(dev), kc.to(dev), v, 1.0), ref, bar=4 * torch_err)


# ------------------------------------------------------------------------------------------------------------------ the other slots
def test_memory_efficient_attention_equals_slow_attn_bitwise(dev, mask680):
    qkv = rnd(17, (2, 70, 3, 2, 64)).to(dev)
    q, k, v = qkv.unbind(2)                                                  # BLHc, as basic_var.py:98
    m = mask680[1][:, :, :70, :70]
    s = 0.25 / math.sqrt(64)
    for mask in (None, m.expand(2, 2, -1, -1)):
        a = seam.memory_efficient_attention(q, k, v, attn_bias=mask, p=0.0, scale=s)
        b = seam.slow_attn(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), s, attn_mask=mask)
        assert a.shape == (2, 70, 2, 64) and torch.equal(a, b.transpose(1, 2))
    d = seam.memory_efficient_attention(q, k, v)                             # default scale 1 / sqrt(64)
    _check(d.transpose(1, 2), _ref(*(t.cpu().transpose(1, 2) for t in (q, k, v)), 0.125))


@pytest.mark.parametrize("mode", E.GEMM_MODES)
@pytest.mark.parametrize("rows", [5, 130])
def test_fused_mlp_func(dev, mode, rows):
    C_, hid = 128, 512
    fc1, fc2 = torch.nn.Linear(C_, hid), torch.nn.Linear(hid, C_)
    with torch.no_grad():
        fc1.weight.copy_(rnd(20, (hid, C_), 1 / math.sqrt(C_))); fc1.bias.copy_(rnd(21, (hid,)))
        fc2.weight.copy_(rnd(22, (C_, hid), 1 / math.sqrt(hid))); fc2.bias.copy_(rnd(23, (C_,)))
    x = rnd(24, (1, rows, C_))
    r0 = F.linear(F.gelu(F.linear(x.double(), fc1.weight.double(), fc1.bias.double()), approximate="tanh"), fc2.weight.double(), fc2.bias.double()).detach()
    fc1, fc2, xd = fc1.to(dev), fc2.to(dev), x.to(dev)
    seam.configure(gemm_mode=mode)
    try:
        with torch.no_grad():
            call = lambda: seam.fused_mlp_func(x=xd, weight1=fc1.weight, weight2=fc2.weight, bias1=fc1.bias, bias2=fc2.bias, activation='gelu_approx', save_pre_act=False,
                                               return_residual=False, checkpoint_lvl=0, heuristic=0, process_group=None)          # basic_var.py:46-50
            got0 = call()
            assert got0.shape == (1, rows, C_)
            err = (got0.cpu().double() - r0).abs().max().item()
            assert err <= 2e-5 * max(1.0, r0.abs().max().item()), err
            fc1.weight.mul_(-0.5)                                            # in place: same storage, _version bumped -> the cached planes must not be reused
            fc1_cpu_w = fc1.weight.cpu()
            got1 = call()
            r1 = F.linear(F.gelu(F.linear(x.double(), fc1_cpu_w.double(), fc1.bias.cpu().double()), approximate="tanh"), fc2.weight.cpu().double(), fc2.bias.cpu().double())
            assert not torch.equal(got0, got1)
            err = (got1.cpu().double() - r1).abs().max().item()
            assert err <= 2e-5 * max(1.0, r1.abs().max().item()), err
    finally:
        seam.configure(gemm_mode=E.DEFAULT_GEMM_MODE)


def test_slot_call_as_the_reference_makes_it(dev, mask680):
    """basic_var.py:93-117 with the teacher-forcing mask slice of var.py:234."""
    B, L, H = 2, 91, 2
    C_ = H * 64
    m, md = mask680
    qkv = rnd(30, (B, L, 3, H, 64))
    q, k, v = qkv.to(dev).view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4).unbind(dim=0)
    s = 0.25 / math.sqrt(64)
    attn_bias = md[:, :, :L, :L]
    oup = seam.slow_attn(query=q, key=k, value=v, scale=s, attn_mask=attn_bias, dropout_p=0.0).transpose(1, 2).reshape(B, L, C_)
    assert oup.is_contiguous() and oup.shape == (B, L, C_)
    qc, kc, vc = qkv.permute(2, 0, 3, 1, 4).unbind(0)
    ref = _ref(qc, kc, vc, s, m[:, :, :L, :L]).transpose(1, 2).reshape(B, L, C_)
    err = (oup.cpu().double() - ref).abs().max().item()
    assert err <= 2e-5 * max(1.0, ref.abs().max().item()), err


# ------------------------------------------------------------------------------------------------------------------ the copy-once rule
@pytest.mark.parametrize("which", [0, 1, 2])
def test_dense_fp32_operand_at_a_misaligned_address_is_copied_once(dev, which):
    """A dense fp32 q / k / v one element into a flat buffer (address % 16 == 4) meets the stride rule and misses the address rule: it is copied once, and the
    output and all three gradients have the bits of the run on aligned copies.  70 keys: one full 64-key tile and a partial one."""
    g = torch.Generator().manual_seed(40)
    keep = torch.rand(1, 1, 70, 70, generator=g) < 0.5
    keep[..., 0] = True
    md = keep.to(dev)
    aligned = [rnd(41 + i, (1, 2, 70, 64)).to(dev) for i in range(3)]
    dout = rnd(44, (1, 2, 70, 64)).to(dev)
    n = aligned[which].numel()
    flat = torch.zeros(n + 4, device=dev)
    odd = flat[1:1 + n].view(1, 2, 70, 64)
    odd.copy_(aligned[which])
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 4 and all(t.data_ptr() % 16 == 0 for t in aligned)
    operands = [odd if i == which else t for i, t in enumerate(aligned)]
    with torch.no_grad():
        assert torch.equal(seam.slow_attn(*operands, 0.125, attn_mask=md), seam.slow_attn(*aligned, 0.125, attn_mask=md))
    runs = []
    for ops in (operands, aligned):
        with torch.enable_grad():
            leaves = [t.detach().requires_grad_() for t in ops]
            assert leaves[which].data_ptr() == ops[which].data_ptr()
            out = seam.slow_attn_grad(*leaves, 0.125, attn_mask=md)
            runs.append((out.detach(),) + torch.autograd.grad(out, leaves, dout))
    for a, b in zip(*runs):
        assert torch.isfinite(a).all() and torch.equal(a, b)
