"""seam.slow_attn_grad / memory_efficient_attention_grad on the GPU (sdvar_op_sdpa_lse + sdvar_op_sdpa_bwd, csrc/attention_sdpa_bwd.hip) against torch's
scaled_dot_product_attention forward AND backward in float64 on the CPU, from the same rnd(...) inputs and the same upstream gradient.

Bar of every gradient (dq, dk, dv each): the project's attention bar err <= 2e-5 * max(1, max|ref|).  Torch's own fp32 autograd on the CPU stays at or below
2.5e-6 * max(1, max|ref|) on these shapes with randn inputs and a randn upstream gradient, so the bar leaves 8x headroom over the reference's own fp32 error.
Unless stated otherwise q, k, v are the reference's views of ONE (B, L, 3, H, 64) leaf buffer (basic_var.py:93-99) and the gradient compared is the leaf's .grad,
split into its q / k / v parts.  Every query row of every case has at least one visible key.  Every test prints the errors it measured.
Measured on an MI355X: the largest error relative to max(1, max|ref|) is 3.9e-6 (dq under the sliced ten-stage mask, 1.23e-4 at max|ref| 31.3; torch's fp32 autograd on the
CPU makes 1.19e-4 there); dk <= 2.8e-6, dv <= 1.4e-6, lse 1.4e-6 absolute at max|ref| 9.1; the single-token dq / dk are 2.8e-6 / 2.7e-6 absolute."""
import ctypes as C
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
NAMES = ("dq", "dk", "dv")


def block_causal(patch_nums):
    """models/var.py:108-113: a query of stage i sees the keys of stages <= i.  (1, 1, L, L) fp32, 0 / -inf."""
    d = torch.cat([torch.full((pn * pn,), i) for i, pn in enumerate(patch_nums)])
    return torch.where(d[:, None] >= d[None, :], 0.0, NEG).reshape(1, 1, len(d), len(d)).float()


@pytest.fixture(autouse=True)
def _grad_mode_on():
    """Grad mode is process-wide state and other test modules of the suite switch it off; these tests are about autograd."""
    with torch.enable_grad():
        yield


@pytest.fixture(scope="module")
def mask680(dev):
    m = block_causal(LADDER10)
    return m, m.to(dev)


def _close(name, got, ref):
    got = got.cpu().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), name
    err = (got - ref).abs().max().item()
    lim = 2e-5 * max(1.0, ref.abs().max().item())
    print(f"{name}: err {err:.3e} bar {lim:.3e} max|ref| {ref.abs().max().item():.3e}")
    assert err <= lim, (name, err, lim)


def _ref_grads(q, k, v, scale, mask, dout):
    """fp64 SDPA forward and backward on the CPU; q, k, v (B, H, L, 64) fp32 CPU tensors -> (out, dq, dk, dv) in float64."""
    q, k, v = (t.detach().double().requires_grad_() for t in (q, k, v))
    m = None if mask is None else (mask if mask.dtype == torch.bool else mask.double())
    out = F.scaled_dot_product_attention(q, k, v, attn_mask=m, scale=scale)
    out.backward(dout.double())
    return out.detach(), q.grad, k.grad, v.grad


def _shared_leaf_case(dev, seed, B, L, H, scale, mask=None, Lq=None, prep=None, call=None):
    """q, k, v = views of one (B, L, 3, H, 64) leaf; the first Lq query rows enter the attention.  Checks out and the leaf's gradient; returns the leaf's .grad."""
    Lq = L if Lq is None else Lq
    qkv = rnd(seed, (B, L, 3, H, 64))
    if prep is not None:
        prep(qkv)
    dout = rnd(seed + 1000, (B, H, Lq, 64))
    qc, kc, vc = qkv.permute(2, 0, 3, 1, 4).unbind(0)
    ro, rq, rk, rv = _ref_grads(qc[:, :, :Lq], kc, vc, scale, mask, dout)
    leaf = qkv.to(dev).requires_grad_()
    q, k, v = leaf.permute(2, 0, 3, 1, 4).unbind(0)
    assert not q.is_contiguous() and not k.is_contiguous()
    md = None if mask is None else mask.to(dev)
    out = (call or seam.slow_attn_grad)(q[:, :, :Lq], k, v, scale, attn_mask=md)
    assert out.requires_grad and out.shape == (B, H, Lq, 64)
    _close("out", out.detach(), ro)
    out.backward(dout.to(dev))
    g = leaf.grad.permute(2, 0, 3, 1, 4)
    _close("dq", g[0][:, :, :Lq], rq)
    if Lq < L:
        assert not g[0][:, :, Lq:].any()                    # the query rows that never entered the attention
    _close("dk", g[1], rk)
    _close("dv", g[2], rv)
    return leaf.grad


# ------------------------------------------------------------------------------------------------------------------ no mask
def test_grad_no_mask_l2_normalised(dev):
    def prep(qkv):
        qkv[:, :, 0] = F.normalize(qkv[:, :, 0], dim=-1) * 4
        qkv[:, :, 1] = F.normalize(qkv[:, :, 1], dim=-1)
    _shared_leaf_case(dev, 101, 2, 37, 2, 1.0, prep=prep)


def test_grad_no_mask_raw_inputs_uneven_lengths(dev):
    _shared_leaf_case(dev, 102, 2, 200, 2, 0.25 / 8, Lq=130)


def test_grad_single_token(dev):
    """P = 1, dS = 0: dq and dk are ~1e-15 in fp64, so only the absolute floor of the bar is checked for them; dv = dout."""
    _shared_leaf_case(dev, 103, 2, 1, 2, 0.5)


def test_grad_cached_shape_separate_leaves(dev):
    B, H, Lq, Lk = 2, 2, 16, 91
    qkv = rnd(104, (B, Lq, 3, H, 64))
    kc, vc = rnd(105, (B, H, Lk, 64)), rnd(106, (B, H, Lk, 64))             # the concatenated caches: contiguous (B, H, Lk, 64)
    dout = rnd(107, (B, H, Lq, 64))
    qc = qkv.permute(2, 0, 3, 1, 4)[0]
    _, rq, rk, rv = _ref_grads(qc, kc, vc, 1.0, None, dout)
    leaf = qkv.to(dev).requires_grad_()
    k, v = kc.to(dev).requires_grad_(), vc.to(dev).requires_grad_()
    seam.slow_attn_grad(leaf.permute(2, 0, 3, 1, 4)[0], k, v, 1.0).backward(dout.to(dev))
    g = leaf.grad.permute(2, 0, 3, 1, 4)
    _close("dq", g[0], rq)
    assert not g[1].any() and not g[2].any()
    _close("dk", k.grad, rk)
    _close("dv", v.grad, rv)
    assert k.grad.shape == (B, H, Lk, 64) and k.grad.stride() != g[0].stride()


# ------------------------------------------------------------------------------------------------------------------ masks
def test_grad_block_causal_five_stages(dev):
    """-inf entries inside a visited tile; raw scores reach about +-30."""
    _shared_leaf_case(dev, 108, 2, 55, 2, 1.0, mask=block_causal((1, 2, 3, 4, 5)))


def test_grad_block_causal_ten_stages(dev, mask680):
    m, md = mask680
    seam.clear_caches()
    _shared_leaf_case(dev, 109, 1, 680, 2, 1.0, mask=m, call=lambda q, k, v, s, attn_mask: seam.slow_attn_grad(q, k, v, s, attn_mask=md))
    smap = next(e[1] for e in seam._SKIP_MAPS.values() if e[0].data_ptr() == md.data_ptr()).cpu().reshape(6, 11)
    # stage boundaries 0 1 5 14 30 55 91 155 255 424 680: queries 0..127 see keys < 155, so key tiles 3.. are skipped for them; the last block sees everything
    assert smap[0].tolist() == [0, 0, 0] + [1] * 8 and smap[1].tolist() == smap[2].tolist() == [0] * 7 + [1] * 4 and smap[3:].sum() == 0


def test_grad_block_causal_sliced_view(dev, mask680):
    m, md = mask680
    ms, msd = m[:, :, :424, :424], md[:, :, :424, :424]
    assert not msd.is_contiguous()
    _shared_leaf_case(dev, 110, 1, 424, 2, 1.0, mask=ms, call=lambda q, k, v, s, attn_mask: seam.slow_attn_grad(q, k, v, s, attn_mask=msd))


def test_grad_bool_mask(dev):
    g = torch.Generator().manual_seed(111)
    keep = torch.rand(1, 1, 91, 91, generator=g) < 0.4
    keep[..., 0] = True                                    # every row keeps a key
    _shared_leaf_case(dev, 112, 2, 91, 2, 1.0, mask=keep)


def test_grad_finite_per_head_bias_with_masked_tile(dev):
    b = rnd(113, (1, 2, 256, 128), 2.0)
    b[:, :, 128:256, 64:128] = NEG                          # one whole 128 x 64 tile masked for both heads: skipped in both walks
    qkv = rnd(114, (1, 256, 3, 2, 64))
    dout = rnd(115, (1, 2, 256, 64))
    qc, kc, vc = qkv.permute(2, 0, 3, 1, 4).unbind(0)
    _, rq, rk, rv = _ref_grads(qc, kc[:, :, :128], vc[:, :, :128], 0.125, b, dout)
    leaf, bd = qkv.to(dev).requires_grad_(), b.to(dev)
    q, k, v = leaf.permute(2, 0, 3, 1, 4).unbind(0)
    seam.slow_attn_grad(q, k[:, :, :128], v[:, :, :128], 0.125, attn_mask=bd).backward(dout.to(dev))
    g = leaf.grad.permute(2, 0, 3, 1, 4)
    _close("dq", g[0], rq)
    _close("dk", g[1][:, :, :128], rk)
    _close("dv", g[2][:, :, :128], rv)
    smap = next(e[1] for e in seam._SKIP_MAPS.values() if e[0].data_ptr() == bd.data_ptr()).cpu().tolist()
    assert smap == [0, 0, 0, 1]


def test_grad_memory_efficient_attention_equals_slow_attn_bitwise(dev, mask680):
    B, L, H = 2, 91, 2
    qkv = rnd(116, (B, L, 3, H, 64))
    dout = rnd(117, (B, L, H, 64))
    s = 0.25 / math.sqrt(64)
    bias = mask680[1][:, :, :L, :L].expand(B, H, -1, -1)                    # stride-0 batch and head
    assert bias.stride(0) == 0 and bias.stride(1) == 0
    la, lb = qkv.to(dev).requires_grad_(), qkv.to(dev).requires_grad_()
    q, k, v = la.unbind(2)                                                   # BLHc, as basic_var.py:98
    a = seam.memory_efficient_attention_grad(q, k, v, attn_bias=bias, p=0.0, scale=s)
    assert a.shape == (B, L, H, 64)
    a.backward(dout.to(dev))
    q, k, v = lb.permute(2, 0, 3, 1, 4).unbind(0)
    b = seam.slow_attn_grad(q, k, v, s, attn_mask=bias)
    b.backward(dout.to(dev).transpose(1, 2))
    assert torch.equal(a, b.transpose(1, 2)) and torch.equal(la.grad, lb.grad)
    qc, kc, vc = qkv.permute(2, 0, 3, 1, 4).unbind(0)
    _, rq, rk, rv = _ref_grads(qc, kc, vc, s, mask680[0][:, :, :L, :L], dout.transpose(1, 2))
    for name, got, ref in zip(NAMES, la.grad.permute(2, 0, 3, 1, 4), (rq, rk, rv)):
        _close(name, got, ref)


# ------------------------------------------------------------------------------------------------------------------ properties
def _leaf_run(dev, seed, L, mask=None, grad=(True, True, True), B=2, H=2):
    """Separate q, k, v leaves (B, H, L, 64) with the chosen requires_grad; -> (out, grads)."""
    ts = [rnd(seed + i, (B, H, L, 64)).to(dev).requires_grad_(g) for i, g in enumerate(grad)]
    out = seam.slow_attn_grad(*ts, 0.125, attn_mask=mask)
    out.backward(rnd(seed + 7, (B, H, L, 64)).to(dev))
    return out.detach(), [t.grad for t in ts]


def test_forward_under_grad_equals_slow_attn_bitwise(dev, mask680):
    m = mask680[1][:, :, :91, :91]
    ts = [rnd(120 + i, (2, 2, 91, 64)).to(dev) for i in range(3)]
    with torch.no_grad():
        plain = seam.slow_attn(*ts, 0.125, attn_mask=m)
        nograd = seam.slow_attn_grad(*(t.clone().requires_grad_() for t in ts), 0.125, attn_mask=m)
    assert not nograd.requires_grad and torch.equal(plain, nograd)
    frozen = seam.slow_attn_grad(*ts, 0.125, attn_mask=m)                    # grad mode on, nothing requires grad: the twin's launch
    assert not frozen.requires_grad and torch.equal(plain, frozen)
    under = seam.slow_attn_grad(*(t.clone().requires_grad_() for t in ts), 0.125, attn_mask=m)
    assert under.requires_grad and torch.equal(plain, under.detach())


@pytest.mark.parametrize("L", [91, 680])
def test_backward_is_deterministic(dev, mask680, L):
    B = 2 if L == 91 else 1
    m = mask680[1][:, :, :L, :L]
    o1, g1 = _leaf_run(dev, 130, L, m, B=B)
    o2, g2 = _leaf_run(dev, 130, L, m, B=B)
    assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    assert all(torch.isfinite(a).all() and a.abs().max() > 0 for a in g1)


def test_partial_gradients_equal_the_full_run_bitwise(dev, mask680):
    m = mask680[1][:, :, :91, :91]
    _, full = _leaf_run(dev, 140, 91, m)
    _, only_q = _leaf_run(dev, 140, 91, m, grad=(True, False, False))
    assert only_q[1] is None and only_q[2] is None and torch.equal(only_q[0], full[0])
    _, only_v = _leaf_run(dev, 140, 91, m, grad=(False, False, True))
    assert only_v[0] is None and only_v[1] is None and torch.equal(only_v[2], full[2])


def test_second_backward_raises_torch_error(dev):
    ts = [rnd(150 + i, (2, 2, 91, 64)).to(dev).requires_grad_() for i in range(3)]
    loss = seam.slow_attn_grad(*ts, 0.125).sum()                             # .sum(): the upstream gradient is an expanded (stride-0) tensor, copied once
    loss.backward()
    with pytest.raises(RuntimeError):
        loss.backward()
    torch.cuda.synchronize()


def test_call_as_the_reference_makes_it(dev, mask680):
    """basic_var.py:93-117 with the teacher-forcing mask slice of var.py:234, then the projection and a scalar loss; the gradients of the qkv weight and of the
    input against the same graph in fp64 on the CPU."""
    B, L, H = 2, 91, 2
    C_ = H * 64
    m, md = mask680
    s = 0.25 / math.sqrt(64)
    x0, w0, p0 = rnd(160, (B, L, C_)), rnd(161, (3 * C_, C_), 1 / math.sqrt(C_)), rnd(162, (C_, C_), 1 / math.sqrt(C_))

    def graph(x, w, pw, attn, mask):
        qkv = F.linear(x, w).view(B, L, 3, H, 64)
        q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(dim=0)
        oup = attn(q, k, v, mask[:, :, :L, :L]).transpose(1, 2).reshape(B, L, C_)
        return F.linear(oup, pw).sum()

    xr, wr = x0.double().requires_grad_(), w0.double().requires_grad_()
    graph(xr, wr, p0.double(), lambda q, k, v, mk: F.scaled_dot_product_attention(q, k, v, attn_mask=mk.double(), scale=s), m).backward()
    xd, wd = x0.to(dev).requires_grad_(), w0.to(dev).requires_grad_()
    graph(xd, wd, p0.to(dev), lambda q, k, v, mk: seam.slow_attn_grad(query=q, key=k, value=v, scale=s, attn_mask=mk, dropout_p=0.0), md).backward()
    _close("d qkv weight", wd.grad, wr.grad)
    _close("d input", xd.grad, xr.grad)


# ------------------------------------------------------------------------------------------------------------------ the log-sum-exp rows
@pytest.mark.parametrize("masked", [False, True])
def test_lse_matches_logsumexp_and_rows_past_lq_stay_untouched(dev, masked):
    B, H, Lq, Lk, PAD = 2, 2, 130, 200, 64
    s = 0.25
    q, k, v = rnd(170, (B, H, Lq, 64)), rnd(171, (B, H, Lk, 64)), rnd(172, (B, H, Lk, 64))
    bias = None
    if masked:                                              # five-stage style: stage boundaries over the keys, a query of stage i sees the keys of stages <= i
        dq_ = torch.bucketize(torch.arange(Lq), torch.tensor([1, 5, 14, 30, 55]), right=True)
        dk_ = torch.bucketize(torch.arange(Lk), torch.tensor([1, 5, 14, 30, 55]), right=True)
        bias = torch.where(dq_[:, None] >= dk_[None, :], 0.0, NEG).reshape(1, 1, Lq, Lk).float()
    scores = s * q.double() @ k.double().transpose(-1, -2) + (0 if bias is None else bias.double())
    ref = torch.logsumexp(scores, dim=-1)
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    out = torch.empty(B, Lq, H, 64, device=dev)
    SENT = -12345.0
    lse = torch.full((B * H * Lq + PAD,), SENT, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    strides = (C.c_int64 * 12)(*(t.stride(i) for t in (qd, kd, vd) for i in (0, 1, 2)), out.stride(0), out.stride(2), out.stride(1))
    bd = None if bias is None else bias.to(dev)
    bstr = None if bias is None else (C.c_int64 * 3)(0, 0, bd.stride(2))
    E._check(E.load_library().sdvar_op_sdpa_lse(p(qd), p(kd), p(vd), p(out), p(lse), strides, p(bd), 0 if bias is None else 1, bstr, None, B, H, Lq, Lk, 64, s,
                                                E._stream()))
    torch.cuda.synchronize()
    assert (lse[B * H * Lq:] == SENT).all()                  # rows >= Lq of the last query block are never written
    _close("lse", lse[:B * H * Lq].reshape(B, H, Lq), ref)
    with torch.no_grad():
        assert torch.equal(out.permute(0, 2, 1, 3), seam.slow_attn(qd, kd, vd, s, attn_mask=bd))
