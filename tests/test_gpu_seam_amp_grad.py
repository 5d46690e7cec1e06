"""seam.slow_attn_amp_grad / memory_efficient_attention_amp_grad / flash_attn_func_grad / install_train_amp on the GPU (sdvar_op_sdpa_hm_lse + sdvar_op_sdpa_h_bwd,
csrc/attention_sdpa_h_bwd.hip): the attention of a model trained under torch.autocast, forward AND backward, against torch's SDPA in float64 on the CPU on the
operands AS THE KERNEL SEES THEM (fp32 q / k rounded to the half dtype with .to(dtype) first; the mask in its own values; dout in the half dtype).

e_torch = the error against that float64 result of torch's CPU SDPA autograd run in the half dtype on the same operands.  Bar, for out, dq, dk, dv separately, with
u = 2^-11 (fp16) / 2^-8 (bf16):
    err <= 2 e_torch + u max|ref| + 2e-5 max(1, max|ref|)
(the middle term is the one final rounding and also covers the unrounded fp32 gradients; the last is the project's fp32 attention bar).  A CPU emulation of the
kernels' arithmetic contract on these shapes stayed at err / bar <= 0.37.  Every case runs for fp16 and bf16 and prints err, e_torch, the bar and max|ref|.
Every query row of every case has at least one visible key.
Measured on an MI355X, the largest err / bar per output over the cases of the issue: out 0.30 (bf16, uneven lengths, all half: err 8.0e-4 = e_torch), dq 0.34 (fp16,
per-head bias, all half: 1.03e-3 against e_torch 9.3e-4), dk 0.34 (fp16, cached shape, all half: 1.01e-2 at max|ref| 18.5, e_torch 1.00e-2), dv 0.30 (fp16, cached
shape: 1.6e-3 = e_torch); the 2^11-scaled dout 0.15 - 0.24; the single token's dq / dk 2.5e-6 / 3.6e-6 absolute; the qkv weight gradient of the reference-style
call 0.27 (fp16, through the GradScaler step) / 0.34 (bf16); lse 1.2e-6 at max|ref| 9.7 (bar 1.9e-4)."""
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
VARIANTS = ["half", "mixed"]            # all three operands half | q, k fp32 next to a half v (attn_l2_norm under autocast)
NEG = float("-inf")
LADDER5, LADDER10 = (1, 2, 3, 4, 5), (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
NAMES = ("out", "dq", "dk", "dv")
_REFS = {}


def _u(dtype):
    return 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8


def block_causal(patch_nums):
    """models/var.py:108-113: a query of stage i sees the keys of stages <= i.  (1, 1, L, L) fp32, 0 / -inf."""
    d = torch.cat([torch.full((pn * pn,), i) for i, pn in enumerate(patch_nums)])
    return torch.where(d[:, None] >= d[None, :], 0.0, NEG).reshape(1, 1, len(d), len(d)).float()


def _mixed_mask(Lq=130, Lk=150):
    """fp32 (1, 1, Lq, Lk): finite values within +-4 mixed with -inf; key 0 stays visible for every row (the construction of test_gpu_seam_amp.py)."""
    m = rnd(70, (1, 1, Lq, Lk)).clamp(-4, 4)
    hole = rnd(71, (1, 1, Lq, Lk)) > 0.3
    hole[..., 0] = False
    return m.masked_fill(hole, NEG)


@pytest.fixture(autouse=True)
def _grad_mode_on():
    """Grad mode is process-wide state and other test modules of the suite switch it off; these tests are about autograd."""
    with torch.enable_grad():
        yield


@pytest.fixture(scope="module")
def mask680(dev):
    m = block_causal(LADDER10)
    return m, m.to(dev)


def _sdpa_grads(q, k, v, scale, mask, dout):
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    out = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=scale)
    out.backward(dout)
    return [t.double() for t in (out.detach(), q.grad, k.grad, v.grad)]


def _refs(key, ops, scale, mask, dout, dtype):
    """ops: fp32 CPU (B, H, L, 64) q, k, v; mask: the CPU mask as passed (or None); dout: CPU, half.  -> (float64 reference, e_torch) for out, dq, dk, dv;
    computed once per key (the all-half and the mixed variant of a case see the same rounded operands, so they share it)."""
    if key not in _REFS:
        qh, kh, vh = (t.to(dtype) for t in ops)
        m64 = None if mask is None else (mask if mask.dtype == torch.bool else mask.double())
        ref = _sdpa_grads(qh.double(), kh.double(), vh.double(), scale, m64, dout.double())
        tor = _sdpa_grads(qh, kh, vh, scale, mask, dout)
        _REFS[key] = (ref, [(t - r).abs().max().item() for t, r in zip(tor, ref)])
    return _REFS[key]


def _close(label, name, got, ref, e_torch, dtype):
    g = got.detach().cpu().double()
    assert g.shape == ref.shape, (label, name, g.shape, ref.shape)
    mref = ref.abs().max().item()
    err = (g - ref).abs().max().item()
    bar = 2 * e_torch + _u(dtype) * mref + 2e-5 * max(1.0, mref)
    print(f"{label} {str(dtype)[6:]} {name}: err {err:.3e}  e_torch {e_torch:.3e}  bar {bar:.3e}  max|ref| {mref:.3e}  err/bar {err / bar:.2f}")
    assert math.isfinite(err), f"{label} {name}: err {err}"
    assert err <= bar, f"{label} {name}: err {err:.3e} > bar {bar:.3e} (e_torch {e_torch:.3e}, max|ref| {mref:.3e})"


def _inputs(seed, B, H, Lq, Lk, norm=None):
    """fp32 CPU q (B, H, Lq, 64), k, v (B, H, Lk, 64).  norm = m: q <- normalize(q) m, k <- normalize(k), as attn_l2_norm leaves them."""
    q, k, v = rnd(seed, (B, H, Lq, 64)), rnd(seed + 1, (B, H, Lk, 64)), rnd(seed + 2, (B, H, Lk, 64))
    if norm is not None:
        q, k = F.normalize(q, dim=-1) * norm, F.normalize(k, dim=-1)
    return q, k, v


def _blhc_leaf(t, dt, dev):
    """A (B, L, H, 64) leaf on the GPU holding t (B, H, L, 64) in dtype dt, and its (B, H, L, 64) view."""
    leaf = t.permute(0, 2, 1, 3).contiguous().to(dt).to(dev).requires_grad_()
    return leaf, leaf.permute(0, 2, 1, 3)


def _case(dev, label, dtype, variant, seed, B, H, Lq, Lk, scale, mask=None, mask_dev=None, norm=None, layout="blhc", dout_scale=1.0, call=None):
    """One forward + backward through seam.slow_attn_amp_grad (or `call`) against the float64 reference.
    layout: 'blhc' - separate (B, L, H, 64) leaves, passed as permuted views (what autocast's normalised q / k and the unbound v look like);
            'shared' - views of ONE (B, Lk, 3, H, 64) half leaf, the first Lq rows as queries (variant 'half' only);
            'cache' - q a permuted view, k / v separate contiguous (B, H, Lk, 64) leaves."""
    ops = _inputs(seed, B, H, Lq, Lk, norm)
    dout = (rnd(seed + 9, (B, H, Lq, 64)) * dout_scale).to(dtype)
    ref, e_torch = _refs((label, dtype), ops, scale, mask, dout, dtype)
    dts = (dtype, dtype, dtype) if variant == "half" else (torch.float32, torch.float32, dtype)
    if layout == "shared":
        assert variant == "half" and Lq <= Lk
        qpad = torch.cat([ops[0], rnd(seed + 3, (B, H, Lk - Lq, 64))], dim=2)
        leaf = torch.stack([t.permute(0, 2, 1, 3) for t in (qpad, ops[1], ops[2])], dim=2).to(dtype).to(dev).requires_grad_()     # (B, Lk, 3, H, 64)
        q, k, v = leaf.permute(2, 0, 3, 1, 4).unbind(0)
        q = q[:, :, :Lq]
        assert not q.is_contiguous() and not k.is_contiguous()
    elif layout == "cache":
        lq, q = _blhc_leaf(ops[0], dts[0], dev)
        k, v = (t.to(dt).to(dev).requires_grad_() for t, dt in zip(ops[1:], dts[1:]))
    else:
        (lq, q), (lk, k), (lv, v) = (_blhc_leaf(t, dt, dev) for t, dt in zip(ops, dts))
    md = mask_dev if mask_dev is not None else (None if mask is None else mask.to(dev))
    out = (call or seam.slow_attn_amp_grad)(q, k, v, scale, attn_mask=md)
    assert out.requires_grad and out.dtype == dtype and out.shape == (B, H, Lq, 64)
    out.backward(dout.to(dev))
    if layout == "shared":
        g = leaf.grad.permute(2, 0, 3, 1, 4)
        assert leaf.grad.dtype == dtype
        assert not g[0][:, :, Lq:].any()                    # the query rows that never entered the attention: exactly zero
        grads = (g[0][:, :, :Lq], g[1], g[2])
    elif layout == "cache":
        grads = (lq.grad.permute(0, 2, 1, 3), k.grad, v.grad)
        assert k.grad.shape == (B, H, Lk, 64)
    else:
        grads = tuple(l.grad.permute(0, 2, 1, 3) for l in (lq, lk, lv))
    for g_, dt in zip(grads, dts):
        assert g_.dtype == dt                               # each gradient in its operand's own dtype
    for name, got, r, e in zip(NAMES, (out,) + grads, ref, e_torch):
        _close(f"{label}/{variant}", name, got, r, e, dtype)
    return out.detach(), grads


# ------------------------------------------------------------------------------------------------------------------ the cases of the issue
@pytest.mark.parametrize("dtype", DTYPES)
def test_five_stage_mask_mixed_operands(dev, dtype):
    """Case 1: -inf inside a visited tile, a mixed-dtype gradient (dq, dk fp32; dv half)."""
    _case(dev, "five-stage", dtype, "mixed", 201, 2, 2, 55, 55, 1.0, mask=block_causal(LADDER5), norm=4.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_five_stage_mask_one_half_leaf(dev, dtype):
    """Case 2: the same data, all three half and views of ONE (B, L, 3, H, 64) leaf."""
    _case(dev, "five-stage", dtype, "half", 201, 2, 2, 55, 55, 1.0, mask=block_causal(LADDER5), norm=4.0, layout="shared")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_mask_raw_inputs_uneven_lengths(dev, dtype, variant):
    """Case 3: tails in both kernels and an unused part of a 128-block; with a shared leaf the query rows >= Lq of the leaf's grad are exactly zero."""
    _case(dev, "uneven", dtype, variant, 210, 2, 2, 130, 200, 0.25 / 8, layout="shared" if variant == "half" else "blhc")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_cached_shape_separate_leaves(dev, dtype, variant):
    """Case 4: Lq 16, Lk 91, separate contiguous (B, H, Lk, 64) k / v leaves."""
    _case(dev, "cached", dtype, variant, 220, 2, 2, 16, 91, 1.0, layout="cache")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_single_token(dev, dtype, variant):
    """Case 5: P = 1, dS = 0: dv == dout to rounding; dq and dk are ~0 in float64, so they are held to the absolute floor of the bar only."""
    _, grads = _case(dev, "single", dtype, variant, 230, 2, 2, 1, 1, 0.5)
    dout = (rnd(239, (2, 2, 1, 64))).to(dtype)
    assert torch.equal(grads[2].cpu(), dout)               # P rounds to exactly 1


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("half_mask", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_mask(dev, dtype, half_mask, variant):
    """Case 6: finite values within +-4 mixed with -inf, 130 x 150, as fp32 and as an additive mask in the half dtype (kind 3)."""
    m = _mixed_mask()
    if half_mask:
        m = m.to(dtype)
    _case(dev, "mixed-mask-h" if half_mask else "mixed-mask", dtype, variant, 240, 2, 2, 130, 150, 0.125, mask=m)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_bool_mask(dev, dtype, variant):
    """Case 7: a bool keep-mask 91 x 91 at density 0.4 with column 0 kept."""
    g = torch.Generator().manual_seed(111)
    keep = torch.rand(1, 1, 91, 91, generator=g) < 0.4
    keep[..., 0] = True
    _case(dev, "bool", dtype, variant, 250, 2, 2, 91, 91, 1.0, mask=keep, norm=4.0)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_per_head_bias_with_masked_tiles(dev, dtype, variant):
    """Case 8: a per-head finite bias; head 0 has the (128-query, 64-key) tile (1, 1) fully masked, head 1 the tile (1, 0), both the tile (1, 2).  Only the last may
    be skipped: a tile one head masks is still visited for the other (where it is -inf inside a visited tile for the first)."""
    b = rnd(260, (1, 2, 256, 192), 2.0).clamp(-4, 4)
    b[:, 0, 128:256, 64:128] = NEG
    b[:, 1, 128:256, 0:64] = NEG
    b[:, :, 128:256, 128:192] = NEG
    bd = b.to(dev)
    seam.clear_caches()
    _case(dev, "per-head", dtype, variant, 261, 1, 2, 256, 192, 0.125, mask=b, mask_dev=bd)
    smap = next(e[1] for e in seam._SKIP_MAPS.values() if e[0].data_ptr() == bd.data_ptr()).cpu().tolist()
    assert smap == [0, 0, 0, 0, 0, 1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_ten_stage_mask(dev, mask680, dtype):
    """Case 9: the teacher-forcing shape of a d16 model, one batch row, two heads; attn_l2_norm operands (q, k fp32; v half)."""
    m, md = mask680
    seam.clear_caches()
    _case(dev, "ten-stage", dtype, "mixed", 270, 1, 2, 680, 680, 1.0, mask=m, mask_dev=md, norm=4.0)
    smap = next(e[1] for e in seam._SKIP_MAPS.values() if e[0].data_ptr() == md.data_ptr()).cpu().reshape(6, 11)
    # stage boundaries 0 1 5 14 30 55 91 155 255 424 680: queries 0..127 see keys < 155, so key tiles 3.. are skipped for them; the last block sees everything
    assert smap[0].tolist() == [0, 0, 0] + [1] * 8 and smap[1].tolist() == smap[2].tolist() == [0] * 7 + [1] * 4 and smap[3:].sum() == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_ten_stage_mask_sliced_view(dev, mask680, dtype):
    """Case 9, second half: the [:, :, :424, :424] view of the mask, read in place; all three operands views of one half leaf."""
    m, md = mask680
    ms, msd = m[:, :, :424, :424], md[:, :, :424, :424]
    assert not msd.is_contiguous()
    _case(dev, "ten-stage-sliced", dtype, "half", 275, 1, 2, 424, 424, 1.0, mask=ms, mask_dev=msd, norm=4.0, layout="shared")


def test_grad_scaler_sized_dout_fp16(dev):
    """Case 10: dout scaled by 2^11 on the shape of case 1.  The same bar: it is relative, since e_torch scales with dout."""
    _case(dev, "five-stage-scaled", torch.float16, "mixed", 201, 2, 2, 55, 55, 1.0, mask=block_causal(LADDER5), norm=4.0, dout_scale=2.0 ** 11)


# ------------------------------------------------------------------------------------------------------------------ properties
def _leaf_run(dev, dtype, seed, L, mask=None, grad=(True, True, True), B=2, H=2, mixed=True, dout=None, fn=None):
    """Separate (B, H, L, 64) leaves (q, k fp32 when mixed) with the chosen requires_grad -> (out, grads)."""
    dts = (torch.float32, torch.float32, dtype) if mixed else (dtype,) * 3
    ts = [rnd(seed + i, (B, H, L, 64)).to(dt).to(dev).requires_grad_(g) for i, (g, dt) in enumerate(zip(grad, dts))]
    out = (fn or seam.slow_attn_amp_grad)(*ts, 0.125, attn_mask=mask)
    out.backward(rnd(seed + 7, (B, H, L, 64)).to(dtype).to(dev) if dout is None else dout)
    return out.detach(), [t.grad for t in ts]


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_under_grad_equals_slow_attn_amp_bitwise(dev, mask680, dtype):
    for mixed, m in ((True, mask680[1][:, :, :91, :91]), (False, mask680[1][:, :, :91, :91]), (True, None), (False, None)):      # (False, None): flash's kernel
        dts = (torch.float32, torch.float32, dtype) if mixed else (dtype,) * 3
        ts = [rnd(300 + i, (2, 2, 91, 64)).to(dt).to(dev) for i, dt in enumerate(dts)]
        with torch.no_grad():
            plain = seam.slow_attn_amp(*ts, 0.125, attn_mask=m)
            nograd = seam.slow_attn_amp_grad(*(t.clone().requires_grad_() for t in ts), 0.125, attn_mask=m)
        assert not nograd.requires_grad and torch.equal(plain, nograd)
        frozen = seam.slow_attn_amp_grad(*ts, 0.125, attn_mask=m)            # grad mode on, nothing requires grad: the twin's launch
        assert not frozen.requires_grad and torch.equal(plain, frozen)
        under = seam.slow_attn_amp_grad(*(t.clone().requires_grad_() for t in ts), 0.125, attn_mask=m)
        assert under.requires_grad and under.dtype == dtype and torch.equal(plain, under.detach())


@pytest.mark.parametrize("dtype", DTYPES)
def test_three_fp32_operands_take_the_fp32_path(dev, dtype):
    ts = [rnd(310 + i, (2, 2, 55, 64)).to(dev).requires_grad_() for i in range(3)]
    m = block_causal(LADDER5).to(dev)
    a = seam.slow_attn_amp_grad(*ts, 0.125, attn_mask=m)
    a.backward(torch.ones_like(a))
    ga = [t.grad.clone() for t in ts]
    for t in ts:
        t.grad = None
    b = seam.slow_attn_grad(*ts, 0.125, attn_mask=m)
    b.backward(torch.ones_like(b))
    assert a.dtype == torch.float32 and torch.equal(a, b) and all(torch.equal(x, t.grad) for x, t in zip(ga, ts))


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_twins_give_the_same_bits(dev, mask680, dtype):
    """memory_efficient_attention_amp_grad (masked, mixed) and flash_attn_func_grad (no mask, all half) against slow_attn_amp_grad on the same data."""
    B, L, H = 2, 91, 2
    s = 0.25 / math.sqrt(64)
    dout = rnd(327, (B, L, H, 64)).to(dtype).to(dev)
    bias = mask680[1][:, :, :L, :L].expand(B, H, -1, -1)                    # stride-0 batch and head
    mk = lambda i, dt: rnd(320 + i, (B, L, H, 64)).to(dt).to(dev).requires_grad_()
    for mixed, twin in ((True, "mea"), (False, "flash")):
        dts = (torch.float32, torch.float32, dtype) if mixed else (dtype,) * 3
        la, lb = [mk(i, dt) for i, dt in enumerate(dts)], [mk(i, dt) for i, dt in enumerate(dts)]
        if twin == "mea":
            a = seam.memory_efficient_attention_amp_grad(*la, attn_bias=bias, p=0.0, scale=s)
            b = seam.slow_attn_amp_grad(*(t.permute(0, 2, 1, 3) for t in lb), s, attn_mask=bias)
        else:
            a = seam.flash_attn_func_grad(*la, dropout_p=0.0, softmax_scale=s)
            with torch.no_grad():
                assert torch.equal(a.detach(), seam.flash_attn_func(*(t.detach() for t in la), softmax_scale=s))
            b = seam.slow_attn_amp_grad(*(t.permute(0, 2, 1, 3) for t in lb), s)
        assert a.shape == (B, L, H, 64) and a.requires_grad
        a.backward(dout)
        b.backward(dout.transpose(1, 2))
        assert torch.equal(a, b.transpose(1, 2))
        for x, y, dt in zip(la, lb, dts):
            assert x.grad.dtype == dt and x.grad.is_contiguous() and torch.equal(x.grad, y.grad) and x.grad.abs().max() > 0


@pytest.mark.parametrize("L", [55, 680])
@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_is_deterministic(dev, mask680, dtype, L):
    B = 2 if L == 55 else 1
    m = mask680[1][:, :, :L, :L] if L == 680 else block_causal(LADDER5).to(dev)
    o1, g1 = _leaf_run(dev, dtype, 330, L, m, B=B)
    o2, g2 = _leaf_run(dev, dtype, 330, L, m, B=B)
    assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    assert all(torch.isfinite(a).all() and a.abs().max() > 0 for a in g1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_partial_gradients_equal_the_full_run_bitwise(dev, mask680, dtype):
    m = mask680[1][:, :, :91, :91]
    _, full = _leaf_run(dev, dtype, 340, 91, m)
    _, only_q = _leaf_run(dev, dtype, 340, 91, m, grad=(True, False, False))
    assert only_q[1] is None and only_q[2] is None and torch.equal(only_q[0], full[0])
    _, kv = _leaf_run(dev, dtype, 340, 91, m, grad=(False, True, True))
    assert kv[0] is None and torch.equal(kv[1], full[1]) and torch.equal(kv[2], full[2])


@pytest.mark.parametrize("dtype", DTYPES)
def test_second_backward_raises_torch_error(dev, dtype):
    ts = [rnd(350 + i, (2, 2, 55, 64)).to(dtype).to(dev).requires_grad_() for i in range(3)]
    loss = seam.slow_attn_amp_grad(*ts, 0.125).float().sum()
    loss.backward()
    with pytest.raises(RuntimeError):
        loss.backward()
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
def test_misaligned_dout_gives_the_aligned_bits(dev, mask680, dtype):
    B, H, L = 2, 2, 55
    m = block_causal(LADDER5).to(dev)
    d = rnd(367, (B, H, L, 64)).to(dtype).to(dev)
    flat = torch.zeros(d.numel() + 8, dtype=dtype, device=dev)
    mis = flat[1:1 + d.numel()].view(B, H, L, 64)
    mis.copy_(d)
    assert mis.data_ptr() % 16 != 0 and mis.is_contiguous()
    _, ga = _leaf_run(dev, dtype, 360, L, m, dout=d)
    _, gb = _leaf_run(dev, dtype, 360, L, m, dout=mis)
    assert all(torch.equal(a, b) for a, b in zip(ga, gb))


@pytest.mark.parametrize("dtype", DTYPES)
def test_wrong_dout_dtype_raises(dev, dtype):
    """Autograd itself casts a mismatched gradient before it reaches a Function, so the check is reached by calling the backward on the graph node directly."""
    ts = [rnd(370 + i, (1, 16, 2, 64)).to(dtype).to(dev).requires_grad_() for i in range(3)]
    out = seam.memory_efficient_attention_amp_grad(*ts)                      # BLHc: the function's own output, so out.grad_fn is its context
    with pytest.raises(E.SdvarError, match="memory_efficient_attention_amp_grad.*gradient of the output"):
        seam._SdpaFn.backward(out.grad_fn, torch.zeros(1, 16, 2, 64, device=dev))


# ------------------------------------------------------------------------------------------------------------------ the C entries
_p = lambda t: None if t is None else C.c_void_p(t.data_ptr())


def _raw(q, k, v, dtype, dout=None, mask=None, kind=0, smap=None, scale=1.0, want=(True, True, True), lse_pad=0):
    """sdvar_op_sdpa_hm_lse, then (with dout) sdvar_op_sdpa_h_bwd, on (B, H, L, 64) device tensors -> (out, lse buffer, dq, dk, dv)."""
    B, H, Lq, _ = q.shape
    Lk = k.shape[2]
    lib, code = E.load_library(), 1 if dtype == torch.float16 else 2
    qf, kf = int(q.dtype == torch.float32), int(k.dtype == torch.float32)
    out = torch.empty(B, H, Lq, 64, dtype=dtype, device=q.device)
    lse = torch.full((B * H * Lq + lse_pad,), -12345.0, device=q.device)
    bstr = None if mask is None else (C.c_int64 * 3)(*(0 if n == 1 else s for n, s in zip(mask.shape[:3], mask.stride()[:3])))
    s12 = (C.c_int64 * 12)(*(t.stride(i) for t in (q, k, v, out) for i in (0, 1, 2)))
    E._check(lib.sdvar_op_sdpa_hm_lse(_p(q), _p(k), _p(v), _p(out), _p(lse), s12, code, qf, kf, _p(mask), kind, bstr, _p(smap), B, H, Lq, Lk, 64, scale, E._stream()))
    grads = [None, None, None]
    if dout is not None:
        grads = [torch.zeros_like(t) if w else None for t, w in zip((q, k, v), want)]
        delta = torch.empty(B * H * Lq, device=q.device)
        st = lambda t: (0, 0, 0) if t is None else tuple(t.stride(i) for i in (0, 1, 2))
        s24 = (C.c_int64 * 24)(*(x for t in (q, k, v, out, dout, *grads) for x in st(t)))
        E._check(lib.sdvar_op_sdpa_h_bwd(_p(q), _p(k), _p(v), _p(out), _p(dout), _p(lse), _p(delta), *(_p(g) for g in grads), s24, code, qf, kf, _p(mask), kind, bstr,
                                         _p(smap), B, H, Lq, Lk, 64, scale, E._stream()))
    torch.cuda.synchronize()
    return (out, lse, *grads)


def _skip_map(mask, kind, Lq, Lk):
    smap = torch.full((((Lq + 127) // 128) * ((Lk + 63) // 64),), 7, dtype=torch.uint8, device=mask.device)
    bstr = (C.c_int64 * 3)(*(0 if n == 1 else s for n, s in zip(mask.shape[:3], mask.stride()[:3])))
    E._check(E.load_library().sdvar_op_sdpa_skip_map(_p(mask), kind, bstr, mask.shape[0], mask.shape[1], Lq, Lk, _p(smap), E._stream()))
    return smap


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_lse_matches_logsumexp_and_rows_past_lq_stay_untouched(dev, dtype, masked):
    B, H, Lq, Lk, PAD = 2, 2, 130, 200, 64
    s = 0.25
    q, k, v = rnd(400, (B, H, Lq, 64)), rnd(401, (B, H, Lk, 64)), rnd(402, (B, H, Lk, 64))
    bias = None
    if masked:                                              # five-stage style: a query of stage i sees the keys of stages <= i
        dq_ = torch.bucketize(torch.arange(Lq), torch.tensor([1, 5, 14, 30, 55]), right=True)
        dk_ = torch.bucketize(torch.arange(Lk), torch.tensor([1, 5, 14, 30, 55]), right=True)
        bias = torch.where(dq_[:, None] >= dk_[None, :], 0.0, NEG).reshape(1, 1, Lq, Lk).float()
    scores = s * q.to(dtype).double() @ k.to(dtype).double().transpose(-1, -2) + (0 if bias is None else bias.double())
    ref = torch.logsumexp(scores, dim=-1)
    # masked: fp32 q / k rounded in the kernel; unmasked: three half operands (the case sdvar_op_sdpa_h serves in the inference slot)
    qd, kd = (q.to(dev), k.to(dev)) if masked else (q.to(dtype).to(dev), k.to(dtype).to(dev))
    vd = v.to(dtype).to(dev)
    bd = None if bias is None else bias.to(dev)
    out, lse, *_ = _raw(qd, kd, vd, dtype, mask=bd, kind=int(masked), scale=s, lse_pad=PAD)
    assert (lse[B * H * Lq:] == -12345.0).all()             # rows past Lq of the last query block are never written
    got = lse[:B * H * Lq].reshape(B, H, Lq).cpu().double()
    err, lim = (got - ref).abs().max().item(), 2e-5 * max(1.0, ref.abs().max().item())
    print(f"lse {str(dtype)[6:]} masked={masked}: err {err:.3e} bar {lim:.3e} max|ref| {ref.abs().max().item():.3e}")
    assert err <= lim
    with torch.no_grad():
        assert torch.equal(out, seam.slow_attn_amp(qd, kd, vd, s, attn_mask=bd))


@pytest.mark.parametrize("dtype", DTYPES)
def test_c_entry_null_gradients_and_skip_map_change_no_bit(dev, mask680, dtype):
    B, H, L = 1, 2, 424
    m = mask680[1][:, :, :L, :L]
    q, k = (F.normalize(rnd(410 + i, (B, H, L, 64)), dim=-1).to(dev) for i in range(2))
    v, dout = (rnd(412 + i, (B, H, L, 64)).to(dtype).to(dev) for i in range(2))
    smap = _skip_map(m, 1, L, L)
    assert smap.cpu().reshape(4, 7)[0].tolist() == [0, 0, 0, 1, 1, 1, 1]
    full = _raw(q, k, v, dtype, dout, m, 1, smap)
    assert all(torch.isfinite(t).all() and t.abs().max() > 0 for t in (full[0], *full[2:]))
    bare = _raw(q, k, v, dtype, dout, m, 1, None)
    assert all(torch.equal(a, b) for a, b in zip(full, bare))
    only_q = _raw(q, k, v, dtype, dout, m, 1, smap, want=(True, False, False))
    assert only_q[3] is None and only_q[4] is None and torch.equal(only_q[2], full[2])
    kv = _raw(q, k, v, dtype, dout, m, 1, smap, want=(False, True, True))
    assert kv[2] is None and torch.equal(kv[3], full[3]) and torch.equal(kv[4], full[4])
    only_v = _raw(q, k, v, dtype, dout, m, 1, smap, want=(False, False, True))
    assert torch.equal(only_v[4], full[4])


# ------------------------------------------------------------------------------------------------------------------ the call as the reference makes it
@pytest.mark.parametrize("ffn", [False, True])
def test_install_train_amp_slots(dev, ffn):
    mod = types.SimpleNamespace(slow_attn=None, flash_attn_func=None, fused_mlp_func=None)
    seam.install_train_amp(mod, None, ffn=ffn)
    assert mod.slow_attn is seam.slow_attn_amp_grad and mod.flash_attn_func is seam.flash_attn_func_grad
    assert mod.fused_mlp_func is (seam.fused_mlp_func_grad if ffn else None)
    if ffn:             # the FFN slot under autocast: fp32 operands run (the reference's FFN input is fp32 under autocast), a half x raises
        x, w1, w2 = rnd(500, (4, 64)).to(dev), rnd(501, (128, 64), 0.1).to(dev).requires_grad_(), rnd(502, (64, 128), 0.1).to(dev)
        with torch.autocast("cuda", torch.bfloat16):
            y = mod.fused_mlp_func(x, w1, w2)
            assert y.dtype == torch.float32 and y.requires_grad
            with pytest.raises(E.SdvarError, match="fused_mlp_func_grad.*float32"):
                mod.fused_mlp_func(x.half(), w1, w2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_call_as_the_reference_makes_it_under_autocast(dev, mask680, dtype):
    """basic_var.py:93-117 under torch.autocast with attn_l2_norm: a half qkv from a linear layer, F.normalize on q / k (fp32 under autocast), the fp32 mask slice,
    .transpose(1, 2).reshape, a loss, .backward() - for fp16 through a GradScaler step.  The linear layer's weight gradient against the same chain in float64 (from the
    weights and input as autocast rounds them); e_torch = the chain on the CPU in the half dtype."""
    B, L, H = 2, 91, 2
    C_ = H * 64
    m, md = mask680
    x0, w0, r0 = rnd(510, (B, L, C_)), rnd(511, (3 * C_, C_), 1 / math.sqrt(C_)), rnd(512, (B, L, C_))
    mod = types.SimpleNamespace()
    seam.install_train_amp(mod)

    def chain(x, w, r, attn, mask, lo, hi):
        """lo: the dtype of the linear layer and of v; hi: the dtype F.normalize returns."""
        qkv = F.linear(x.to(lo), w.to(lo)).view(B, L, 3, H, 64)
        q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(dim=0)
        q, k = F.normalize(q.to(hi), dim=-1) * 4, F.normalize(k.to(hi), dim=-1)
        oup = attn(q, k, v, mask[:, :, :L, :L]).transpose(1, 2).reshape(B, L, C_)
        return (oup.to(hi) * r.to(hi)).sum()

    def torch_attn(lo):
        return lambda q, k, v, mk: F.scaled_dot_product_attention(q.to(lo), k.to(lo), v, attn_mask=mk.double() if lo == torch.float64 else mk, scale=1.0)

    wr = w0.to(dtype).double().requires_grad_()
    chain(x0.to(dtype).double(), wr, r0, torch_attn(torch.float64), m, torch.float64, torch.float64).backward()
    wt = w0.clone().requires_grad_()
    chain(x0, wt, r0, torch_attn(dtype), m, dtype, torch.float32).backward()
    e_torch = (wt.grad.double() - wr.grad).abs().max().item()

    seen = []
    def slot(q, k, v, mk):
        seen.append((q.dtype, k.dtype, v.dtype))
        return mod.slow_attn(query=q, key=k, value=v, scale=1.0, attn_mask=mk, dropout_p=0.0)

    wd, xd, rd = w0.to(dev).requires_grad_(), x0.to(dev), r0.to(dev)
    opt = torch.optim.SGD([wd], lr=0.0)
    with torch.autocast("cuda", dtype):
        qkv = F.linear(xd, wd).view(B, L, 3, H, 64)
        q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(dim=0)
        q, k = F.normalize(q, dim=-1) * 4, F.normalize(k, dim=-1)
        oup = slot(q, k, v, md[:, :, :L, :L]).transpose(1, 2).reshape(B, L, C_)
        loss = (oup.float() * rd).sum()
    assert seen == [(torch.float32, torch.float32, dtype)]
    if dtype == torch.float16:
        scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 11)
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        scaler.step(opt)
        scaler.update()
        assert scaler.get_scale() == 2.0 ** 11             # no inf / nan was found: the step was taken
    else:
        loss.backward()
    assert wd.grad.dtype == torch.float32
    _close("reference call", "d qkv weight", wd.grad, wr.grad, e_torch, dtype)
