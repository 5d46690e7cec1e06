"""The seam's backward attention kernels (sdvar_op_sdpa_lse + sdvar_op_sdpa_bwd, csrc/attention_sdpa_bwd.hip) on hard inputs, length tails and layouts, against torch's
scaled_dot_product_attention forward AND backward in float64 on the CPU (test_gpu_seam_grad._ref_grads: the same inputs, the same upstream gradient).

Bar, unless a test says otherwise: the project's attention bar err <= 2e-5 * max(1, max|ref|) for out, lse, dq, dk and dv each (test_gpu_seam_grad._close).  The
large-score tests cannot use it (fp32 itself does not reach it there): each tensor's bar is LARGE_MULT = 4 times the error torch's own fp32 CPU autograd makes on the
same inputs against fp64, computed in the test.  No bar comes from the kernels under test.  Before any launch every test asserts on the CPU that every query row
has a visible key and that the fp64 reference is finite; no row and no case is excluded from a comparison.  Every test prints what it measured.

Measured on an MI355X, largest error relative to the bar over the whole file: out 0.10 (6.4e-6 at max|ref| 3.3), dq 0.11 (6.7e-6 at 3.0), dk 0.27 (5.4e-6 absolute at
(Lq, Lk) = (129, 1), where P = 1, dS = 0 and the fp64 gradient is 1e-15; 0.07 elsewhere), dv 0.07 (5.0e-6 at 3.6), lse 0.02 (5.4e-6 at max|ref| 12.8), delta 0.02 (1.7e-6
at 4.0).  Large scores, error as a multiple of torch's fp32 error (bar 4): out <= 1.01, dq <= 1.18 (the dominant-key case, 6.3e-6 against 5.3e-6), dk <= 1.05 (2.7e-4
against 2.5e-4 at max|ref| 123, mul 50 with k normalised), dv <= 1.04; at mul 100 with raw k the kernels make 0.66 - 0.78 of torch's error (dk 4.7e-3 against 7.0e-3 at
max|ref| 192).  The battery exposed no error in the kernels or in seam.py.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from conftest import rnd
from sdvar_amd import engine as E
from sdvar_amd import seam
from test_gpu_seam_grad import LADDER10, NEG, _close, _ref_grads, block_causal

pytestmark = pytest.mark.gpu
NAMES = ("out", "dq", "dk", "dv")
SENT = -12345.0
PAD = 4096
LARGE_MULT = 4.0
TAILS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129)


@pytest.fixture(autouse=True)
def _grad_mode_on():
    """Grad mode is process-wide state and other test modules of the suite switch it off; these tests are about autograd."""
    with torch.enable_grad():
        yield


# ------------------------------------------------------------------------------------------------------------------ helpers
def _additive(mask):
    """A bool keep-mask or an additive mask as a float64 additive bias."""
    return torch.where(mask, 0.0, NEG).double() if mask.dtype == torch.bool else mask.double()


def _in_contract(mask, *refs):
    """Asserted on the CPU before any launch: every query row has a visible key, the fp64 reference is finite everywhere."""
    if mask is not None:
        visible = mask if mask.dtype == torch.bool else mask != NEG
        assert visible.any(dim=-1).all(), "a query row with every key masked"
    for r in refs:
        assert torch.isfinite(r).all()


def _ref_lse(q, k, scale, mask):
    s = scale * q.double() @ k.double().transpose(-1, -2)
    return torch.logsumexp(s if mask is None else s + _additive(mask), dim=-1)


def _seam_run(dev, q, k, v, dout, scale, mask=None, grad=(True, True, True)):
    """Separate (B, H, L, 64) leaves through seam.slow_attn_grad; mask already on the device.  -> (out, [dq, dk, dv]) (None where not asked for)."""
    ts = [t.to(dev).requires_grad_(g) for t, g in zip((q, k, v), grad)]
    out = seam.slow_attn_grad(*ts, scale, attn_mask=mask)
    out.backward(dout if dout.is_cuda else dout.to(dev))
    return out.detach(), [t.grad for t in ts]


def _close_all(out, grads, refs):
    for name, got, ref in zip(NAMES, (out, *grads), refs):
        _close(name, got, ref)


def _equal_all(a, b):
    return all(torch.equal(x, y) for x, y in zip((a[0], *a[1]), (b[0], *b[1])))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _blh(t):
    """(batch, head, token) element strides of a (B, L, H, 64)-shaped tensor."""
    return (0, 0, 0) if t is None else (t.stride(0), t.stride(2), t.stride(1))


def _bias_args(mask):
    """A 4-D device mask as the ABI takes it: (tensor the kernel reads, kind, strides with 0 where it broadcasts)."""
    if mask is None:
        return None, 0, None
    m = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    assert m.dim() == 4 and m.stride(3) == 1
    return m, 2 if mask.dtype == torch.bool else 1, (C.c_int64 * 3)(*(0 if n == 1 else s for n, s in zip(m.shape[:3], m.stride()[:3])))


def _raw_map(m, kind, bstr, Lq, Lk):
    smap = torch.empty(((Lq + 127) // 128) * ((Lk + 63) // 64), dtype=torch.uint8, device=m.device)
    E._check(E.load_library().sdvar_op_sdpa_skip_map(_p(m), kind, bstr, 1 if bstr[0] == 0 else m.shape[0], 1 if bstr[1] == 0 else m.shape[1], Lq, Lk, _p(smap), E._stream()))
    return smap


def _raw_forward(q, k, v, scale, bias=(None, 0, None), smap=None):
    """sdvar_op_sdpa_lse on (B, H, L, 64) device operands -> out (B, Lq, H, 64), lse (B, H, Lq)."""
    B, H, Lq, Lk = *q.shape[:3], k.shape[2]
    out = torch.empty(B, Lq, H, 64, device=q.device)
    lse = torch.empty(B, H, Lq, device=q.device)
    strides = (C.c_int64 * 12)(*(t.stride(i) for t in (q, k, v) for i in (0, 1, 2)), *_blh(out))
    m, kind, bstr = bias
    E._check(E.load_library().sdvar_op_sdpa_lse(_p(q), _p(k), _p(v), _p(out), _p(lse), strides, _p(m), kind, bstr, _p(smap), B, H, Lq, Lk, 64, scale, E._stream()))
    torch.cuda.synchronize()
    return out, lse


def _raw_backward(q, k, v, out, dout, lse, delta, dq, dk, dv, scale, bias=(None, 0, None), smap=None):
    """sdvar_op_sdpa_bwd; out, dout, dq, dk, dv are (B, L, H, 64)-shaped tensors of any strides (dq / dk / dv may be None), delta B*H*Lq floats."""
    B, H, Lq, Lk = *q.shape[:3], k.shape[2]
    assert dout.shape == (B, Lq, H, 64) and delta.numel() == B * H * Lq
    assert dq is None or dq.shape == (B, Lq, H, 64)
    assert all(t is None or t.shape == (B, Lk, H, 64) for t in (dk, dv))
    strides = (C.c_int64 * 24)(*(t.stride(i) for t in (q, k, v) for i in (0, 1, 2)), *_blh(out), *_blh(dout), *_blh(dq), *_blh(dk), *_blh(dv))
    m, kind, bstr = bias
    E._check(E.load_library().sdvar_op_sdpa_bwd(_p(q), _p(k), _p(v), _p(out), _p(dout), _p(lse), _p(delta), _p(dq), _p(dk), _p(dv), strides, _p(m), kind, bstr, _p(smap),
                                                B, H, Lq, Lk, 64, scale, E._stream()))
    torch.cuda.synchronize()


def _raw_run(q, k, v, dout, scale, bias=(None, 0, None), smap=None):
    """Forward + backward into fresh dense buffers -> (out, lse, dq, dk, dv), gradients (B, L, H, 64)."""
    B, H, Lq, Lk = *q.shape[:3], k.shape[2]
    out, lse = _raw_forward(q, k, v, scale, bias, smap)
    dq, dk, dv = (torch.empty(B, L, H, 64, device=q.device) for L in (Lq, Lk, Lk))
    _raw_backward(q, k, v, out, dout, lse, torch.empty(B * H * Lq, device=q.device), dq, dk, dv, scale, bias, smap)
    return out, lse, dq, dk, dv


def _map_of(mask_dev):
    """The skip map seam cached for this device mask."""
    return next(e[1] for e in seam._SKIP_MAPS.values() if e[0].data_ptr() == mask_dev.data_ptr()).cpu()


# ------------------------------------------------------------------------------------------------------------------ 1. large scores
def _f32_grads(q, k, v, scale, dout):
    """Torch's own fp32 SDPA forward and backward on the CPU: the yardstick of the large-score bars."""
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    out = F.scaled_dot_product_attention(q, k, v, scale=scale)
    out.backward(dout)
    return out.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("mul,k_normalised,dominant", [(50, True, False), (50, False, False), (100, True, False), (100, False, False), (50, True, True)])
def test_large_scores(dev, mul, k_normalised, dominant):
    """|s| reaches mul (k normalised) or several hundred (raw k, |k| ~ 8) at scale 1: P = exp2((s - lse) log2 e) is recomputed in both backward walks in an accumulation
    order of their own.  dominant: key 129 (the last tile's tail) is query 3's own direction, so that row's softmax is near one-hot and its dS a cancellation."""
    B, H, L = 2, 3, 130
    q = F.normalize(rnd(201, (B, H, L, 64)), dim=-1) * mul
    k = F.normalize(rnd(202, (B, H, L, 64)), dim=-1) if k_normalised else rnd(202, (B, H, L, 64))
    v, dout = rnd(203, (B, H, L, 64)), rnd(204, (B, H, L, 64))
    if dominant:
        k[:, :, 129] = q[:, :, 3] / 50
    refs = _ref_grads(q, k, v, 1.0, None, dout)
    _in_contract(None, *refs)
    if dominant:
        p3 = torch.softmax(q[:, :, 3:4].double() @ k.double().transpose(-1, -2), dim=-1)[..., 129]
        assert p3.min() > 0.99                              # the row IS near one-hot
    f32 = _f32_grads(q, k, v, 1.0, dout)
    out, grads = _seam_run(dev, q, k, v, dout, 1.0)
    worst = []
    for name, got, f, ref in zip(NAMES, (out, *grads), f32, refs):
        got = got.cpu().double()
        assert got.shape == ref.shape and torch.isfinite(got).all(), name
        terr, err = (f.double() - ref).abs().max().item(), (got - ref).abs().max().item()
        assert terr > 0
        print(f"{name}: err {err:.3e} torch-fp32 err {terr:.3e} ratio {err / terr:.2f} max|ref| {ref.abs().max().item():.3e}")
        if err > LARGE_MULT * terr:
            worst.append((name, err, terr))
    assert not worst, worst


# ------------------------------------------------------------------------------------------------------------------ 2. -inf inside visited tiles, finite lse
def test_masked_tile_inside_visited_blocks_per_batch_bias(dev):
    """A per-batch per-head finite bias.  Rows 40..63 see nothing in key tile 0 while their workgroup visits it; row 5 sees keys 77 and 129 only (batch 0: 129 only);
    batch 0 alone loses keys 64..127, so no tile may be skipped."""
    B, H, Lq, Lk, s = 3, 3, 70, 130, 0.125
    b = rnd(210, (B, H, Lq, Lk), 3.0)
    b[:, :, 40:64, :64] = NEG
    b[:, :, 5, :] = NEG
    b[:, :, 5, 77] = 0.75
    b[:, :, 5, 129] = -1.0
    b[0, :, :, 64:128] = NEG
    q, k, v, dout = rnd(211, (B, H, Lq, 64)), rnd(212, (B, H, Lk, 64)), rnd(213, (B, H, Lk, 64)), rnd(214, (B, H, Lq, 64))
    refs = _ref_grads(q, k, v, s, b, dout)
    rl = _ref_lse(q, k, s, b)
    _in_contract(b, *refs, rl)
    bd = b.to(dev)
    seam.clear_caches()
    out, grads = _seam_run(dev, q, k, v, dout, s, bd)
    assert _map_of(bd).tolist() == [0, 0, 0]
    _close_all(out, grads, refs)
    bias = _bias_args(bd)
    smap = _raw_map(*bias, Lq, Lk)
    assert not smap.any()
    o2, lse = _raw_forward(q.to(dev), k.to(dev), v.to(dev), s, bias, smap)
    _close("lse", lse, rl)
    assert torch.equal(o2.permute(0, 2, 1, 3), out)


# ------------------------------------------------------------------------------------------------------------------ 3. row-broadcast and per-batch masks
@pytest.mark.parametrize("kind", ["fp32", "bool"])
def test_key_padding_mask_per_batch(dev, kind):
    """(B, 1, 1, Lk): bias strides (Lk, 0, 0).  Batch 1 loses the whole first key tile and batch 2 the whole second, per batch only: neither may be skipped."""
    B, H, Lq, Lk, s = 3, 3, 70, 130, 0.125
    keep = torch.ones(B, 1, 1, Lk, dtype=torch.bool)
    keep[0, ..., 100:] = False
    keep[1, ..., :64] = False
    keep[2, ..., 64:128] = False
    m = keep if kind == "bool" else torch.where(keep, 0.0, NEG).float()
    q, k, v, dout = rnd(220, (B, H, Lq, 64)), rnd(221, (B, H, Lk, 64)), rnd(222, (B, H, Lk, 64)), rnd(223, (B, H, Lq, 64))
    refs = _ref_grads(q, k, v, s, m, dout)
    _in_contract(m, *refs)
    md = m.to(dev)
    seam.clear_caches()
    narrow = _seam_run(dev, q, k, v, dout, s, md)
    assert _map_of(md).tolist() == [0, 0, 0]
    wide_mask = md.expand(B, H, Lq, Lk)
    assert wide_mask.stride() == (Lk, 0, 0, 1)
    wide = _seam_run(dev, q, k, v, dout, s, wide_mask)
    assert _equal_all(narrow, wide)
    _close_all(*narrow, refs)
    _close_all(*wide, refs)
    other = torch.where(keep, 0.0, NEG).float() if kind == "bool" else keep           # the same pattern as the other mask kind: the same bits
    assert _equal_all(narrow, _seam_run(dev, q, k, v, dout, s, other.to(dev)))


# ------------------------------------------------------------------------------------------------------------------ 4. mask kinds and load paths
def _mask_copies(m, dev):
    """Device copies of one (1, 1, Lq, Lk) fp32 0 / -inf mask: bool and fp32 with 16-byte-aligned rows (the vector loads), fp32 at an address % 16 == 4 with the
    same row stride, fp32 with an odd row stride (both: the element loads)."""
    Lq, Lk = m.shape[2:]
    if m.is_contiguous():                                                   # a dense mask: pad the rows to a multiple of 4 so that the vector path exists at all
        rs, rows = (Lk + 3) // 4 * 4, Lq
    else:                                                                   # a slice of a larger mask: keep its row stride
        rs, rows = m.stride(2), Lq
    def place(buf, off, stride):
        t = buf[off:off + rows * stride].view(rows, stride)[:, :Lk]
        t.copy_(m[0, 0])
        return t[None, None]
    aligned = place(torch.empty(rows * rs, device=dev), 0, rs)
    shifted = place(torch.empty(rows * rs + 1, device=dev), 1, rs)
    odd = place(torch.empty(rows * (Lk + 1 + Lk % 2), device=dev), 0, Lk + 1 + Lk % 2)
    keep = torch.zeros(rows * rs, dtype=torch.bool, device=dev).view(rows, rs)[:, :Lk][None, None]
    keep.copy_(aligned == 0)
    assert aligned.data_ptr() % 16 == 0 and aligned.stride(2) % 4 == 0 and keep.data_ptr() % 4 == 0 and keep.stride(2) % 4 == 0
    assert shifted.data_ptr() % 16 == 4 and shifted.stride(2) == aligned.stride(2)
    assert odd.stride(2) % 2 == 1
    assert all(torch.equal(t.cpu(), m) for t in (aligned, shifted, odd))
    return keep, aligned, shifted, odd


@pytest.mark.parametrize("which", ["five_stages", "ten_stages_sliced_424"])
def test_mask_kinds_and_bias_load_paths_agree_bitwise(dev, which):
    B, H, s = 2, 3, 0.125
    m = block_causal((1, 2, 3, 4, 5)) if which == "five_stages" else block_causal(LADDER10)[:, :, :424, :424]
    L = m.shape[2]
    q, k, v, dout = (rnd(230 + i, (B, H, L, 64)) for i in range(4))
    refs = _ref_grads(q, k, v, s, m, dout)
    _in_contract(m, *refs)
    keep, aligned, shifted, odd = _mask_copies(m, dev)
    base = _seam_run(dev, q, k, v, dout, s, aligned)
    _close_all(*base, refs)
    for name, other in (("bool", keep), ("shifted", shifted), ("odd", odd)):
        assert _equal_all(base, _seam_run(dev, q, k, v, dout, s, other)), name


# ------------------------------------------------------------------------------------------------------------------ 5. skipping changes no bit
@pytest.mark.parametrize("which", ["ten_stages", "finite_bias"])
def test_skip_map_changes_no_bit(dev, which):
    if which == "ten_stages":
        B, H, Lq, Lk, s = 1, 2, 680, 680, 0.125
        m = block_causal(LADDER10)
    else:
        B, H, Lq, Lk, s = 2, 2, 256, 128, 0.125
        m = rnd(240, (1, H, Lq, Lk), 3.0)
        m[:, :, 128:256, 64:128] = NEG                      # one whole 128 x 64 tile masked for both heads
    q, k, v, dout = rnd(241, (B, H, Lq, 64)), rnd(242, (B, H, Lk, 64)), rnd(243, (B, H, Lk, 64)), rnd(244, (B, Lq, H, 64))
    refs = _ref_grads(q, k, v, s, m, dout.transpose(1, 2))
    rl = _ref_lse(q, k, s, m)
    _in_contract(m, *refs, rl)
    qd, kd, vd, gd, md = (t.to(dev) for t in (q, k, v, dout, m))
    bias = _bias_args(md)
    smap = _raw_map(*bias, Lq, Lk)
    assert (smap == 0).any() and (smap == 1).any() and ((smap == 0) | (smap == 1)).all()
    print(f"skip map: {int(smap.sum())} of {smap.numel()} tiles skipped")
    with_map = _raw_run(qd, kd, vd, gd, s, bias, smap)
    without = _raw_run(qd, kd, vd, gd, s, bias, None)
    for name, a, b in zip(("out", "lse", "dq", "dk", "dv"), with_map, without):
        assert torch.equal(a, b), name
    out, lse, dq, dk, dv = with_map
    _close("lse", lse, rl)
    _close_all(out.permute(0, 2, 1, 3), [t.permute(0, 2, 1, 3) for t in (dq, dk, dv)], refs)


# ------------------------------------------------------------------------------------------------------------------ 6. strided gradient outputs, stray stores
class _Case6:
    B, H, Lq, Lk, s = 2, 3, 70, 130, 0.125

    def __init__(self, dev, masked):
        B, H, Lq, Lk = self.B, self.H, self.Lq, self.Lk
        self.mask = None
        if masked:
            self.mask = torch.rand(1, 1, Lq, Lk, generator=torch.Generator().manual_seed(250)) < 0.4
            self.mask[..., 0] = True
        q, k, v, dout = rnd(251, (B, H, Lq, 64)), rnd(252, (B, H, Lk, 64)), rnd(253, (B, H, Lk, 64)), rnd(254, (B, Lq, H, 64))
        self.cpu = (q, k, v, dout)
        self.refs = _ref_grads(q, k, v, self.s, self.mask, dout.transpose(1, 2))
        self.ref_delta = (dout.transpose(1, 2).double() * self.refs[0]).sum(-1)
        _in_contract(self.mask, *self.refs, self.ref_delta)
        self.q, self.k, self.v, self.dout = (t.to(dev) for t in self.cpu)
        self.bias = _bias_args(None if self.mask is None else self.mask.to(dev))
        self.smap = None if self.mask is None else _raw_map(*self.bias, Lq, Lk)
        self.out, self.lse = _raw_forward(self.q, self.k, self.v, self.s, self.bias, self.smap)

    def backward(self, delta, dq, dk, dv):
        _raw_backward(self.q, self.k, self.v, self.out, self.dout, self.lse, delta, dq, dk, dv, self.s, self.bias, self.smap)


@pytest.fixture(scope="module", params=[False, True], ids=["no_mask", "bool_mask"])
def case6(dev, request):
    with torch.enable_grad():                               # set up before the function-scoped _grad_mode_on; the fp64 reference needs autograd
        return _Case6(dev, request.param)


def _padded(shape, dev):
    """A dense tensor of `shape` with PAD floats of sentinel before and after it; everything starts as the sentinel.  -> (whole buffer, the tensor)."""
    n = int(torch.Size(shape).numel())
    buf = torch.full((n + 2 * PAD,), SENT, device=dev)
    return buf, buf[PAD:PAD + n].view(shape)


def _padding_intact(buf):
    return bool((buf[:PAD] == SENT).all() and (buf[-PAD:] == SENT).all())


def test_gradients_into_one_qkv_buffer(dev, case6):
    """(a) dq, dk, dv are the three slices of ONE (B, Lk, 3, H, 64) buffer, the layout of the reference's qkv activation; dq covers its first Lq token rows only."""
    c = case6
    G = torch.full((c.B, c.Lk, 3, c.H, 64), SENT, device=dev)
    dq, dk, dv = G[:, :c.Lq, 0], G[:, :, 1], G[:, :, 2]
    assert dq.stride() == dk.stride() == (c.Lk * 3 * c.H * 64, 3 * c.H * 64, 64, 1) and not dk.is_contiguous()
    c.backward(torch.empty(c.B * c.H * c.Lq, device=dev), dq, dk, dv)
    _close_all(c.out.permute(0, 2, 1, 3), [t.permute(0, 2, 1, 3) for t in (dq, dk, dv)], c.refs)
    assert (G[:, c.Lq:, 0] == SENT).all()                   # the rows of the dq slice that no query addresses
    assert (G[:, :c.Lq] != SENT).all()


def test_dense_gradients_leave_their_surroundings_alone(dev, case6):
    """(b) sentinel padding around dq, dk, dv and delta; delta = sum(dout * out) against fp64.  (c) an absent gradient changes no bit of the others and is not written."""
    c = case6
    shapes = ((c.B * c.H * c.Lq,), (c.B, c.Lq, c.H, 64), (c.B, c.Lk, c.H, 64), (c.B, c.Lk, c.H, 64))
    bufs, (delta, dq, dk, dv) = zip(*(_padded(s, dev) for s in shapes))
    c.backward(delta, dq, dk, dv)
    assert all(_padding_intact(b) for b in bufs)
    _close("delta", delta.view(c.B, c.H, c.Lq), c.ref_delta)
    _close_all(c.out.permute(0, 2, 1, 3), [t.permute(0, 2, 1, 3) for t in (dq, dk, dv)], c.refs)
    full = [t.clone() for t in (dq, dk, dv)]
    for absent in range(3):
        for b in bufs:
            b.fill_(SENT)
        args = [dq, dk, dv]
        args[absent] = None
        c.backward(delta, *args)
        assert all(_padding_intact(b) for b in bufs)
        for i, (t, f) in enumerate(zip((dq, dk, dv), full)):
            assert (t == SENT).all() if i == absent else torch.equal(t, f), (absent, i)
    q, k, v, dout = c.cpu
    _, only_k = _seam_run(dev, q, k, v, dout.transpose(1, 2), c.s, None if c.mask is None else c.mask.to(dev), grad=(False, True, False))
    assert only_k[0] is None and only_k[2] is None and torch.equal(only_k[1], full[1].permute(0, 2, 1, 3))


# ------------------------------------------------------------------------------------------------------------------ 7. length tails
@pytest.fixture(scope="module")
def tail_operands():
    return tuple(rnd(260 + i, (1, 3, 129, 64)) for i in range(4))


def _tail_pair(dev, ops, Lq, Lk, mask):
    """One (Lq, Lk) pair at B 1, H 3, scale 0.125 -> {tensor: err / (2e-5 * max(1, max|ref|))}."""
    q, k, v, dout = ops[0][:, :, :Lq], ops[1][:, :, :Lk], ops[2][:, :, :Lk], ops[3][:, :, :Lq]
    refs = _ref_grads(q, k, v, 0.125, mask, dout)
    _in_contract(mask, *refs)
    out, grads = _seam_run(dev, q, k, v, dout, 0.125, None if mask is None else mask.to(dev))
    rel = {}
    for name, got, ref in zip(NAMES, (out, *grads), refs):
        got = got.cpu().double()
        assert got.shape == ref.shape and torch.isfinite(got).all(), (name, Lq, Lk)
        rel[name] = (got - ref).abs().max().item() / (2e-5 * max(1.0, ref.abs().max().item()))
    return rel


def _tail_report(results):
    worst = {n: max((r[n], pair) for pair, r in results.items()) for n in NAMES}
    print("worst err / bar: " + ", ".join(f"{n} {w:.3f} at (Lq, Lk) = {pair}" for n, (w, pair) in worst.items()))
    bad = {pair: r for pair, r in results.items() if max(r.values()) > 1.0}
    assert not bad, ("worst", max(worst.values()), "all failing pairs", bad)


@pytest.mark.parametrize("Lq", TAILS)
def test_length_tails_no_mask(dev, tail_operands, Lq):
    """Lq and Lk independently just below, at and just above the wave (32), the tile (64) and the workgroup (128)."""
    _tail_report({(Lq, Lk): _tail_pair(dev, tail_operands, Lq, Lk, None) for Lk in TAILS})


@pytest.mark.parametrize("leg", ["diagonal", "Lk_129"])
def test_length_tails_bool_mask(dev, tail_operands, leg):
    results = {}
    for Lq in TAILS:
        Lk = Lq if leg == "diagonal" else 129
        keep = torch.rand(1, 1, Lq, Lk, generator=torch.Generator().manual_seed(270 + Lq)) < 0.4
        keep[..., 0] = True
        results[(Lq, Lk)] = _tail_pair(dev, tail_operands, Lq, Lk, keep)
    _tail_report(results)


# ------------------------------------------------------------------------------------------------------------------ 8. upstream-gradient layouts, the map cache
def test_upstream_gradient_layouts_give_the_dense_bits(dev):
    B, H, L, s = 2, 3, 91, 0.125
    q, k, v = (rnd(280 + i, (B, H, L, 64)) for i in range(3))
    m = block_causal(LADDER10)[:, :, :L, :L].to(dev)
    g = rnd(283, (B, L, H, 64)).to(dev)
    transposed = g.transpose(1, 2)                                           # (B, H, L, 64) view of a (B, L, H, 64) buffer
    shifted = torch.empty(B * H * L * 64 + 1, device=dev)[1:].view(B, H, L, 64)
    shifted.copy_(transposed)
    row = rnd(284, (B, H, 1, 64)).to(dev)
    expanded = row.expand(B, H, L, 64)
    assert not transposed.is_contiguous() and shifted.data_ptr() % 16 == 4 and expanded.stride(2) == 0
    for name, view in (("transposed", transposed), ("shifted", shifted), ("expanded", expanded)):
        dense = view.clone(memory_format=torch.contiguous_format)           # not .contiguous(): the shifted view is dense already and would come back as itself
        assert dense.data_ptr() % 16 == 0 and dense.is_contiguous() and torch.equal(dense, view)
        a, b = _seam_run(dev, q, k, v, view, s, m), _seam_run(dev, q, k, v, dense, s, m)
        assert _equal_all(a, b), name
        if name != "shifted":                                                # the same values as `transposed`
            _close_all(*a, _ref_grads(q, k, v, s, m.cpu(), view.cpu()))


def test_backward_after_its_skip_map_left_the_cache(dev):
    """Nine forwards with nine masks: the first map leaves seam._SKIP_MAPS (8 entries) before any backward runs; the graph keeps its own."""
    B, H, L, s, N = 2, 2, 91, 0.125, 9
    assert N > seam._SKIP_MAPS_MAX
    q, k, v, dout = (rnd(290 + i, (B, H, L, 64)) for i in range(4))
    masks = []
    for i in range(N):
        keep = torch.rand(1, 1, L, L, generator=torch.Generator().manual_seed(295 + i)) < 0.4
        keep[..., 0] = True
        if i % 2 == 0:
            keep[..., 64:] = False                           # every other mask has a skipped tile: the maps differ, so another mask's map would show
        masks.append(keep)
    refs = [_ref_grads(q, k, v, s, m, dout) for m in masks]
    for m, r in zip(masks, refs):
        _in_contract(m, *r)
    assert len({m.numpy().tobytes() for m in masks}) == N
    seam.clear_caches()
    md = [m.to(dev) for m in masks]
    gd = dout.to(dev)
    graphs = []
    for m in md:
        ts = [t.to(dev).requires_grad_() for t in (q, k, v)]
        graphs.append((ts, seam.slow_attn_grad(*ts, s, attn_mask=m)))
    assert len(seam._SKIP_MAPS) == seam._SKIP_MAPS_MAX and not any(e[0].data_ptr() == md[0].data_ptr() for e in seam._SKIP_MAPS.values())
    results = []
    for (ts, out), r in zip(graphs, refs):
        out.backward(gd)
        results.append((out.detach(), [t.grad for t in ts]))
        _close_all(*results[-1], r)
    assert _equal_all(results[0], _seam_run(dev, q, k, v, gd, s, md[0]))


def test_mask_mutated_between_forward_and_backward_raises(dev):
    B, H, L, s = 2, 2, 91, 0.125
    m = block_causal(LADDER10)[:, :, :L, :L].contiguous().to(dev)
    ts = [rnd(300 + i, (B, H, L, 64)).to(dev).requires_grad_() for i in range(3)]
    out = seam.slow_attn_grad(*ts, s, attn_mask=m)
    m[..., 1, 0] = NEG                                      # in place: the saved mask's version moves
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.backward(rnd(303, (B, H, L, 64)).to(dev))
    torch.cuda.synchronize()
    assert all(t.grad is None for t in ts)                  # raised on reading the saved tensors, before any launch


def test_mask_mutated_between_forwards_gets_a_new_skip_map(dev):
    B, H, L, s = 2, 2, 130, 0.125
    m = torch.zeros(1, 1, L, L)
    m[..., 64:128] = NEG
    q, k, v, dout = (rnd(310 + i, (B, H, L, 64)) for i in range(4))
    md = m.to(dev)
    seam.clear_caches()
    for step in range(2):
        refs = _ref_grads(q, k, v, s, m, dout)
        _in_contract(m, *refs)
        _close_all(*_seam_run(dev, q, k, v, dout, s, md), refs)
        smap = next(e[1] for key, e in seam._SKIP_MAPS.items() if key[0] == md.data_ptr() and key[1] == md._version).cpu().tolist()
        assert smap == ([0, 1, 0, 0, 1, 0] if step == 0 else [0] * 6)
        m[..., 64:128] = rnd(314, (L, 64))                  # the same in-place edit on both copies: the masked tiles become visible
        md[..., 64:128] = m[..., 64:128].to(dev)
    assert len(seam._SKIP_MAPS) == 2
