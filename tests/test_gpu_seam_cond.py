"""seam.ada_lin (csrc/cond_train.hip) and install_cond on the GPU: silu(cond) W^T + b and its three gradients against float64, the bit contracts, and the installers.

Reference: float64 forward and backward on the CPU on the operands as the kernel sees them - in the half modes c, s = silu(c) and W after their roundings (s: torch's
float32 SiLU rounded once to the half dtype), b in its float32 value, dy in half; dc is formed from the UNROUNDED sum over n.  Bars (the project's own):
    fp32:          err <= 2e-5 max|ref|                                                                    (tests/test_gpu_seam_linear.py)
    fp16 / bf16:   err <= 2 e_torch + u max|ref| + 2e-5 max(1, max|ref|),  u = 2^-11 / 2^-8
e_torch = the error, against the float64 result, of torch's CPU autograd in the half dtype on the same Sequential(SiLU, Linear); it is asserted finite.  Every test
prints err / bar for y, dc, dW and db.

Constants of the kernels and the sizes around them that CASES covers (M, K, N):
    rows per pass: forward 8, 16 (more rows: passes of 16); backward 8, 16, 32 (more: a launch per 32 rows for dc, one of 64 for dW)   M = 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64
    forward slab 16 rows, 4 per wave                                                         N = 8, 16, 24
    backward slab 64 rows; 4 slices of slabs in the second pass                              N = 56, 64, 72, 320, 328
    K chunk 256 (forward; backward for M <= 16), 128 (backward, M > 16)                      K = 248, 256, 264 at M <= 16 and M = 17, 63, 64; 120, 128, 136 at M = 17, 31 - 33
    second backward pass: 64 quads of (m, k) per workgroup                                   M K / 4 = 62 (31 x 8), 64 (32 x 8), 66 (33 x 8)

Largest err / bar on an MI355X (one run): fp32 y 0.007, dc 0.013, dW 0.018, db 0.013 (at (8, 128, 768), (8, 128, 256), (63, 264, 16), (64, 40, 200)); half y 0.31
((63, 264, 16) fp16), dc 0.32 ((64, 40, 200) fp16), dW 0.25 (half weight, bf16), db 0.00; y and dc sit at e_torch, the rounding of the result itself.  Hard inputs: 0.011
in fp32 (dc), 0.31 in half (y, bf16).  Through the installers: 0.78 in fp32 (paired.1.weight: a gradient of 3e-7 that is a cancelling sum over every activation; the
ada_lin weights themselves 0.04 - 0.3), 0.54 under autocast (block.attn.q_bias, bf16).  DESIGN.md 4p."""
import ctypes as C
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import rnd
from sdvar_amd import engine as E
from sdvar_amd import seam
import seam_cond_model as CM
import seam_linear_model as SM

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
ARITH = [None, F16, BF16]
IDS = ["fp32", "fp16", "bf16"]
NAMES = ("y", "dc", "dW", "db")
_REFS = {}
# (M, K, N): the issue's cases, then one size below, at and above every constant of the kernels (the table in the docstring)
CASES = [(1, 8, 8), (8, 128, 768), (8, 128, 256), (3, 72, 24), (16, 264, 1544), (64, 40, 200), (33, 1032, 8),
         (7, 248, 56), (8, 256, 64), (9, 264, 72), (15, 120, 8), (16, 128, 16), (17, 136, 24), (31, 8, 320), (32, 8, 328), (33, 8, 64),
         (33, 120, 56), (33, 128, 64), (33, 136, 72), (63, 264, 16), (64, 256, 24), (31, 120, 56), (32, 128, 64), (17, 248, 16), (16, 256, 72)]
SPECIALS = [0.0, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0]


def _u(dtype):
    return 2.0 ** -11 if dtype == F16 else 2.0 ** -8


@pytest.fixture(autouse=True)
def _state():
    """Grad mode is process-wide state and other test modules switch it off; the caches are put back."""
    with torch.enable_grad():
        yield
    seam.clear_caches()


def _inputs(M, K, N, half, bias=True, hard=False, dy_scale=1.0, cshape=None, seed=None):
    """fp32 CPU c, W, b (representable in `half` when given; W is left to the kernel's own rounding) and dy (fp32, or `half`)."""
    seed = seed if seed is not None else 1000 + 7 * M + 3 * K + N
    c = rnd(seed, cshape or (M, K), 2.0)
    if hard:
        sp = SPECIALS + ([1e-30, -1e-30] if half is None else [])
        c.view(-1, K)[:, :len(sp)] = torch.tensor(sp)
    w = rnd(seed + 1, (N, K), K ** -0.5)
    b = rnd(seed + 2, (N,), 0.5) if bias else None
    dy = rnd(seed + 3, tuple(c.shape[:-1]) + (N,)) * dy_scale
    if half is None:
        return c, w, b, dy
    return c.to(half).float(), w, None if b is None else b.to(half).float(), dy.to(half)


def _ref64(c, w, b, dy, half):
    K, N = c.shape[-1], w.shape[0]
    c2, dy64 = c.reshape(-1, K).double(), dy.reshape(-1, N).double()
    sg = torch.sigmoid(c2)
    s = c2 * sg
    if half is not None:
        s = F.silu(c.reshape(-1, K).float()).to(half).double()          # s as the kernel sees it: the float32 SiLU rounded once
        w = w.to(half)
    w64 = w.double()
    y = s @ w64.T + (0 if b is None else b.double())
    dc = (dy64 @ w64) * (sg * (1 + c2 * (1 - sg)))                        # the sum over n is NOT rounded before the derivative
    return [y.view(dy.shape), dc.view(c.shape), dy64.T @ s, None if b is None else dy64.sum(0)]


def _torch_half(c, w, b, dy, half):
    K, N = c.shape[-1], w.shape[0]
    seq = nn.Sequential(nn.SiLU(), nn.Linear(K, N, bias=b is not None)).to(half)
    with torch.no_grad():
        seq[1].weight.copy_(w.to(half))
        if b is not None:
            seq[1].bias.copy_(b.to(half))
    cc = c.to(half).requires_grad_()
    seq(cc).backward(dy)
    y = seq(cc).detach()
    return [y.double(), cc.grad.double(), seq[1].weight.grad.double(), None if b is None else seq[1].bias.grad.double()]


def _refs(key, ops, half):
    """(float64 reference, e_torch) for NAMES, computed once per key and never modified; e_torch is None in fp32."""
    if key not in _REFS:
        ref = _ref64(*ops, half)
        if half is None:
            _REFS[key] = (ref, None)
        else:
            tor = _torch_half(*ops, half)
            _REFS[key] = (ref, [None if r is None else (t - r).abs().max().item() for t, r in zip(tor, ref)])
    return _REFS[key]


def _close(label, name, got, ref, half=None, e_torch=None):
    g = got.detach().cpu().double()
    assert g.shape == ref.shape, (label, name, g.shape, ref.shape)
    assert torch.isfinite(g).all(), f"{label} {name}: non-finite values"
    mref, err = ref.abs().max().item(), (g - ref).abs().max().item()
    if half is None:
        bar = 2e-5 * mref
        print(f"{label} fp32 {name}: err {err:.3e}  bar {bar:.3e}  max|ref| {mref:.3e}  err/bar {err / bar if bar else 0.0:.3f}")
    else:
        assert math.isfinite(e_torch) and math.isfinite(mref), f"{label} {name}: e_torch {e_torch}, max|ref| {mref}: an infinite bar hides everything"
        bar = 2 * e_torch + _u(half) * mref + 2e-5 * max(1.0, mref)
        print(f"{label} {str(half)[6:]} {name}: err {err:.3e}  e_torch {e_torch:.3e}  bar {bar:.3e}  max|ref| {mref:.3e}  err/bar {err / bar:.3f}")
    assert err <= bar, f"{label} {name}: err {err:.3e} > bar {bar:.3e} (max|ref| {mref:.3e})"


def _leaves(ops, dev, half, cdt=None, wdt=F32, grad=(True, True, True)):
    c, w, b, dy = ops
    cdt = cdt or (half or F32)
    return [c.to(cdt).to(dev).requires_grad_(grad[0]), w.to(wdt).to(dev).requires_grad_(grad[1]), None if b is None else b.to(dev).requires_grad_(grad[2])], dy.to(dev)


def _run(leaves, dy, autocast=None, fn=None):
    """One forward + backward through seam.ada_lin; returns (y, dc, dW, db)."""
    for t in leaves:
        if t is not None:
            t.grad = None
    with torch.autocast("cuda", dtype=autocast or F16, enabled=autocast is not None):
        y = (fn or seam.ada_lin)(*leaves)
    y.backward(dy)
    return (y.detach(),) + tuple(None if t is None or t.grad is None else t.grad.clone() for t in leaves)


def _check_all(label, got, ref, half, e_torch):
    for i, name in enumerate(NAMES):
        if ref[i] is not None:
            _close(label, name, got[i], ref[i], half, None if e_torch is None else e_torch[i])


# ------------------------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("half", ARITH, ids=IDS)
@pytest.mark.parametrize("M,K,N", CASES)
def test_vs_fp64(dev, M, K, N, half):
    ops = _inputs(M, K, N, half)
    ref, e_torch = _refs((M, K, N, half), ops, half)
    leaves, dy = _leaves(ops, dev, half)
    got = _run(leaves, dy)
    assert got[0].dtype == (half or F32) and got[1].dtype == (half or F32) and got[2].dtype == F32 and got[3].dtype == F32
    _check_all(f"({M}, {K}, {N})", got, ref, half, e_torch)


@pytest.mark.parametrize("half", [F16, BF16], ids=IDS[1:])
def test_fp32_cond_under_autocast_gives_half_and_fp32_grads(dev, half):
    """The head norm's case: a float32 cond under autocast; y is half, dc float32, dW unrounded float32."""
    M, K, N = 8, 128, 256
    ops = _inputs(M, K, N, half)
    ref, e_torch = _refs((M, K, N, half), ops, half)
    leaves, dy = _leaves(ops, dev, half, cdt=F32)
    got = _run(leaves, dy, autocast=half)
    assert got[0].dtype == half and got[1].dtype == F32 and got[2].dtype == F32
    _check_all("fp32 cond under autocast", got, ref, half, e_torch)
    # the same operands with a half cond: the same s, so y and dW have the same bits
    leaves_h, _ = _leaves(ops, dev, half)
    got_h = _run(leaves_h, dy)
    assert torch.equal(got[0], got_h[0]) and torch.equal(got[2], got_h[2]) and torch.equal(got[3], got_h[3])


@pytest.mark.parametrize("half", [F16, BF16], ids=IDS[1:])
def test_half_weight_vs_fp64(dev, half):
    M, K, N = 5, 72, 40
    c, w, b, dy = _inputs(M, K, N, half)
    ops = (c, w.to(half).float(), b, dy)
    ref, e_torch = _refs(("half w", half), ops, half)
    leaves, dyd = _leaves(ops, dev, half, wdt=half)
    got = _run(leaves, dyd)
    assert got[2].dtype == half
    _check_all("half weight", got, ref, half, e_torch)


@pytest.mark.parametrize("half", ARITH, ids=IDS)
def test_3d_cond_without_bias(dev, half):
    ops = _inputs(10, 64, 96, half, bias=False, cshape=(2, 5, 64))
    ref, e_torch = _refs(("3d", half), ops, half)
    leaves, dy = _leaves(ops, dev, half)
    got = _run(leaves, dy)
    assert got[0].shape == (2, 5, 96) and got[1].shape == (2, 5, 64) and got[3] is None
    _check_all("3-D cond (2, 5, 64) -> 96", got, ref, half, e_torch)


@pytest.mark.parametrize("half", ARITH, ids=IDS)
@pytest.mark.parametrize("M,K,N", [(8, 128, 768), (17, 264, 72)])
def test_hard_inputs(dev, M, K, N, half):
    """c holds 0, +-20, +-88, +-104 (where expf overflows) in every row, and +-1e-30 in fp32; dy is scaled by 1e-7 in fp32 and 2^5 in the half modes."""
    ops = _inputs(M, K, N, half, hard=True, dy_scale=1e-7 if half is None else 32.0)
    ref, e_torch = _refs(("hard", M, K, N, half), ops, half)
    leaves, dy = _leaves(ops, dev, half)
    got = _run(leaves, dy)
    for name, t in zip(NAMES[:3], got[:3]):
        assert torch.isfinite(t).all(), f"{name} is not finite on the hard inputs"
    _check_all(f"hard ({M}, {K}, {N})", got, ref, half, e_torch)


def test_fp16_overflow_is_inf_exactly_where_fp64_overflows(dev):
    M, K, N = 4, 16, 16
    c = 0.25 * rnd(77, (M, K)).clamp(-1, 1)
    c[1] = 40.0           # s = 40 in every column of row 1
    c[2] = 2.0            # silu'(2) = 1.09
    w = 0.05 * rnd(78, (N, K)).clamp(-1, 1)
    w[3] = 300.0          # y[1, 3] = 16 * 40 * 300 = 192000
    dy = rnd(79, (M, N)).clamp(-1, 1)
    dy[2, 3] = 1000.0     # dc[2, :] = 1000 * 300 * 1.09 = 327000
    ops = (c.to(F16).float(), w.to(F16).float(), None, dy.to(F16))
    ref = _ref64(*ops, F16)
    leaves, dyd = _leaves(ops, dev, F16)
    y, dc, dW, _ = _run(leaves, dyd)
    for name, got, r in (("y", y, ref[0]), ("dc", dc, ref[1])):
        marked = r.abs() > 2 * 65504.0
        assert marked.any() and (r.abs()[~marked] < 65504.0 / 2).all(), f"{name}: the inputs must separate the marked elements"
        g = got.cpu().double()
        assert torch.equal(torch.isinf(g), marked) and torch.equal(torch.sign(g[marked]), torch.sign(r[marked])), f"{name}: +-inf exactly at the marked elements"
        assert (g[~marked] - r[~marked]).abs().max() <= 2.0 ** -10 * r[~marked].abs().max() + 1e-3
    assert dW.dtype == F32 and torch.isfinite(dW).all()
    assert marked[2].all() and torch.equal(marked.any(1), torch.tensor([False, False, True, False]))


# ------------------------------------------------------------------------------------------------------------------ bit contracts
@pytest.mark.parametrize("half", ARITH, ids=IDS)
def test_rows_do_not_depend_on_the_batch(dev, half):
    ops = _inputs(8, 264, 72, half)
    (c, w, b), _ = _leaves(ops, dev, half, grad=(False,) * 3)
    y8 = seam.ada_lin(c, w, b)
    assert torch.equal(y8[2:5], seam.ada_lin(c[2:5], w, b)) and torch.equal(y8[7:], seam.ada_lin(c[7:], w, b))
    c40 = torch.cat([c] * 5)          # 40 rows: the second pass of the forward
    assert torch.equal(seam.ada_lin(c40, w, b)[32:], y8)


@pytest.mark.parametrize("half", ARITH, ids=IDS)
def test_no_grad_bits_repeats_and_each_gradient_alone(dev, half):
    ops = _inputs(9, 264, 136, half)
    leaves, dy = _leaves(ops, dev, half)
    full = _run(leaves, dy)
    with torch.no_grad():
        assert torch.equal(seam.ada_lin(*leaves), full[0]), "torch.no_grad(): the same forward launch, the same bits"
    assert torch.equal(seam.ada_lin(*(t.detach() for t in leaves)), full[0])
    again = _run(leaves, dy)
    assert all(torch.equal(a, b) for a, b in zip(full, again)), "repeats are bit-identical"
    for i in range(3):
        only, _ = _leaves(ops, dev, half, grad=tuple(j == i for j in range(3)))
        got = _run(only, dy)
        assert torch.equal(got[1 + i], full[1 + i]) and all(got[1 + j] is None for j in range(3) if j != i), f"{NAMES[1 + i]} alone"


def test_frozen_operands_launch_nothing_for_them(dev, monkeypatch):
    ops = _inputs(8, 128, 256, None)
    seen = []
    orig = E.cond_lin_bwd
    monkeypatch.setattr(E, "cond_lin_bwd", lambda dy, c, w, dt, need=(True, True, True): seen.append(tuple(need)) or orig(dy, c, w, dt, need))
    for grad in ((True, False, True), (False, True, True), (False, False, True)):
        leaves, dy = _leaves(ops, dev, None, grad=grad)
        got = _run(leaves, dy)
        assert [g is not None for g in got[1:]] == list(grad)
    assert seen == [(True, False, True), (False, True, True), (False, False, True)]


@pytest.mark.parametrize("half", ARITH, ids=IDS)
def test_strided_misaligned_and_stride0_operands(dev, half, monkeypatch):
    M, K, N = 6, 72, 40
    ops = _inputs(M, K, N, half)
    leaves, dy = _leaves(ops, dev, half)
    want = _run(leaves, dy)
    dt = half or F32
    per16 = 16 // torch.empty(0, dtype=dt).element_size()
    seen = []
    orig = E.cond_lin_fwd
    monkeypatch.setattr(E, "cond_lin_fwd", lambda c, w, b, d: seen.append((c.data_ptr(), tuple(c.stride()))) or orig(c, w, b, d))
    # a column slice of a wider buffer: read in place
    wide = torch.zeros(M, K + 3 * per16, dtype=dt, device=dev)
    wide[:, per16:per16 + K] = leaves[0].detach()
    cs = wide[:, per16:per16 + K].requires_grad_()
    got = _run([cs, leaves[1], leaves[2]], dy)
    assert seen[-1] == (cs.data_ptr(), (K + 3 * per16, 1)), "a strided cond that meets the 16-byte rule is read in place"
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # one element off the 16-byte grid: copied once
    flat = torch.zeros(M * K + 1, dtype=dt, device=dev)
    flat[1:] = leaves[0].detach().reshape(-1)
    cm = flat[1:].view(M, K).requires_grad_()
    assert cm.data_ptr() % 16 != 0
    got = _run([cm, leaves[1], leaves[2]], dy)
    assert seen[-1][0] != cm.data_ptr() and seen[-1][0] % 16 == 0 and seen[-1][1] == (K, 1)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # y.sum().backward(): a stride-0 dy, copied once; the bits of a dense dy of ones
    ones = torch.ones(M, N, dtype=dt, device=dev)
    want1 = _run(leaves, ones)
    for t in leaves:
        t.grad = None
    seam.ada_lin(*leaves).sum().backward()
    assert all(torch.equal(t.grad, w1) for t, w1 in zip(leaves, want1[1:]))


def test_in_place_weight_update_is_seen_by_the_next_call(dev):
    ops = _inputs(8, 128, 256, None)
    (c, w, b), _ = _leaves(ops, dev, None, grad=(False,) * 3)
    y0 = seam.ada_lin(c, w, b)
    with torch.no_grad():
        w.mul_(2.0)
        b.zero_()
    y1 = seam.ada_lin(c, w, b)
    assert torch.equal(y1, seam.ada_lin(c, w.clone(), None)) and not torch.equal(y0, y1)
    assert not seam._WEIGHT_PLANES, "ada_lin keeps no operand cache"


def test_saved_tensors_are_cond_and_weight(dev):
    ops = _inputs(8, 128, 256, F16)
    leaves, dy = _leaves(ops, dev, F16, cdt=F32)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t), torch.autocast("cuda", dtype=F16):
        y = seam.ada_lin(*leaves)
    assert sorted((t.data_ptr(), tuple(t.shape), t.dtype) for t in saved) == sorted((t.data_ptr(), tuple(t.shape), t.dtype) for t in leaves[:2])
    y.backward(dy)


@pytest.mark.parametrize("half", ARITH, ids=IDS)
def test_double_backward_raises_and_an_empty_batch_launches_nothing(dev, half, monkeypatch):
    ops = _inputs(3, 72, 24, half)
    leaves, dy = _leaves(ops, dev, half)
    y = seam.ada_lin(*leaves)
    with pytest.raises(E.SdvarError, match="double backward"):
        torch.autograd.grad(y, leaves[0], dy, create_graph=True)
    monkeypatch.setattr(E, "load_library", lambda *a, **k: pytest.fail("M == 0 must not reach the library"))
    y0 = seam.ada_lin(leaves[0][:0], leaves[1], leaves[2])
    assert y0.shape == (0, 24) and y0.dtype == (half or F32)
    y0.sum().backward()
    assert all(t.grad is not None and not t.grad.any() for t in leaves)


def _guarded(n_bytes, dev):
    """A sentinel-filled byte buffer with n_bytes of payload at a 16-byte aligned offset; returns (buffer, payload offset)."""
    pad = 4096
    buf = torch.full((pad + n_bytes + pad,), 0x7B, dtype=torch.uint8, device=dev)
    off = pad + (-(buf.data_ptr() + pad)) % 16
    return buf, off


@pytest.mark.parametrize("half", ARITH, ids=IDS)
@pytest.mark.parametrize("M,K,N", [(9, 264, 72), (33, 136, 200)])
def test_nothing_is_written_outside_the_outputs_and_the_workspace(dev, M, K, N, half):
    ops = _inputs(M, K, N, half)
    (c, w, b), dy = _leaves(ops, dev, half, grad=(False,) * 3)
    lib, st = E.load_library(), E._stream()
    el = 4 if half is None else 2
    code = E.TRAIN_DTYPES[half or F32]
    sizes = {"y": M * N * el, "dc": M * K * el, "dW": N * K * 4, "db": N * 4, "ws": E.cond_lin_bwd_ws_bytes(M, N, K)}
    assert sizes["ws"] == math.ceil(N / 64) * M * K * 4
    bufs = {n: _guarded(s, dev) for n, s in sizes.items()}
    ptr = lambda n: C.c_void_p(bufs[n][0].data_ptr() + bufs[n][1])
    p = lambda t: C.c_void_p(t.data_ptr())
    E._check(lib.sdvar_op_cond_lin_fwd(p(c), code, K, p(w), 0, p(b), ptr("y"), code, M, N, K, st))
    E._check(lib.sdvar_op_cond_lin_bwd(p(dy), p(c), code, K, p(w), 0, ptr("dc"), ptr("dW"), ptr("db"), ptr("ws"), code, M, N, K, st))
    torch.cuda.synchronize()
    leaves, _ = _leaves(ops, dev, half)
    want = _run(leaves, dy)
    for n, t in zip(("y", "dc", "dW", "db"), want):
        buf, off = bufs[n]
        assert torch.equal(buf[off:off + sizes[n]], t.contiguous().view(-1).view(torch.uint8)), f"{n}: the bits of the seam call"
    for n, (buf, off) in bufs.items():
        assert (buf[:off] == 0x7B).all() and (buf[off + sizes[n]:] == 0x7B).all(), f"{n}: bytes outside the buffer were written"


# ------------------------------------------------------------------------------------------------------------------ the installers
@pytest.fixture
def slots():
    saved = SM.save_slots()
    yield SM
    SM.restore_slots(saved)


def _model_refs():
    """The stand-in's float64 loss and gradients at loss scales 1 and 1024, and e_torch per tensor and half dtype: torch's CPU run under torch.autocast."""
    if "model" not in _REFS:
        m, x0, cond, w, mask = CM.model_and_inputs()
        m = m.double()
        ref1 = CM.loss_and_grads(m, *(t.double() for t in (x0, cond, w, mask)))
        ref1k = {n: t * 1024.0 for n, t in ref1.items()}
        m = m.float()
        e = {}
        for half in (F16, BF16):
            tor = CM.loss_and_grads(m, x0, cond, w, mask, autocast=half, scale=1024.0)
            e[half] = {n: (tor[n].double() - ref1k[n]).abs().max().item() for n in ref1k}
        _REFS["model"] = (ref1, ref1k, e)
    return _REFS["model"]


def _compare_model(tag, got, ref, half=None, e_torch=None):
    print(f"\n{tag}")
    for n, r in ref.items():
        assert n in got, f"{n} received no gradient"
        _close(tag, n, got[n], r, half, None if e_torch is None else e_torch[n])


def _spy(monkeypatch):
    seen = []
    orig = seam.ada_lin
    monkeypatch.setattr(seam, "ada_lin", lambda cond, weight, bias=None: seen.append((weight.data_ptr(), cond.dtype, cond.numel() // cond.shape[-1])) or orig(cond, weight, bias))
    return seen


def _bound(m):
    return {n for n, q in m.named_modules() if isinstance(q, nn.Sequential) and "forward" in q.__dict__}


def _on_gpu(dev):
    m, x0, cond, w, mask = CM.model_and_inputs()
    return m.to(dev), tuple(t.to(dev) for t in (x0, cond, w, mask))


EVERY = dict(adaln=True, qknorm=True, linears=True)


@pytest.mark.parametrize("others", [False, True], ids=["alone", "every switch"])
def test_install_train_cond(dev, slots, monkeypatch, others):
    ref, _, _ = _model_refs()
    m, args = _on_gpu(dev)
    plain = CM.loss_and_grads(m, *args)
    seam.install_train(slots, m, cond=True, **(dict(ffn=True, **EVERY) if others else {}))
    assert _bound(m) == {"block.ada_lin", "head_nm.ada_lin"}, "the Linear subclass with its own forward and the in-place SiLU stay with torch"
    seen = _spy(monkeypatch)
    got = CM.loss_and_grads(m, *args)
    served = {m.block.ada_lin[1].weight.data_ptr(), m.head_nm.ada_lin[1].weight.data_ptr()}
    assert {s[0] for s in seen} == served and all(s[1] == F32 and s[2] == CM.B for s in seen)
    _compare_model(f"stand-in, install_train(cond=True{', every switch' if others else ''})", got, ref)
    if others:
        keys = {k[2] for k in seam._WEIGHT_PLANES}
        assert keys and not (keys & served), "a served ada_lin weight must not enter the weight-operand cache"
        assert m.head.weight.data_ptr() in keys
    # 65 rows: nn.Sequential.forward
    seen.clear()
    c65 = torch.randn(65, CM.D, device=dev)
    with torch.no_grad():
        y65 = m.head_nm.ada_lin(c65)
    assert not seen and y65.shape == (65, 2 * CM.C)
    if not others:
        with torch.no_grad():
            assert torch.equal(y65, F.linear(F.silu(c65), m.head_nm.ada_lin[1].weight, m.head_nm.ada_lin[1].bias))
    seam.uninstall_cond(m)
    assert not _bound(m)
    if others:
        seam.uninstall_linears(m)
        seam.uninstall_adaln(m)
        seam.uninstall_qknorm(m)
        m.block.ffn.fused_mlp_func = None
    SM.restore_slots({"slow_attn": SM._torch_attn, "flash_attn_func": None, "memory_efficient_attention": None, "fused_mlp_func": None})
    again = CM.loss_and_grads(m, *args)
    assert all(torch.equal(again[k], plain[k]) for k in plain), "after uninstall_cond the classes' own forwards are back"


@pytest.mark.parametrize("others", [False, True], ids=["alone", "every switch"])
@pytest.mark.parametrize("half", [F16, BF16], ids=IDS[1:])
def test_install_train_amp_cond(dev, slots, monkeypatch, half, others):
    _, ref, e_torch = _model_refs()
    m, args = _on_gpu(dev)
    seam.install_train_amp(slots, m, cond=True, **(dict(ffn="half", **EVERY) if others else {}))
    assert _bound(m) == {"block.ada_lin", "head_nm.ada_lin"}
    seen = _spy(monkeypatch)
    got = CM.loss_and_grads(m, *args, autocast=half, scale=1024.0)
    served = {m.block.ada_lin[1].weight.data_ptr(), m.head_nm.ada_lin[1].weight.data_ptr()}
    assert {s[0] for s in seen} == served and all(s[1] == F32 for s in seen), "both are fed the float32 condition under autocast"
    assert all(g.dtype == F32 for g in got.values())
    _compare_model(f"stand-in, install_train_amp(cond=True{', every switch' if others else ''}), autocast {half}", got, ref, half, e_torch[half])
    if others:
        keys = {k[2] for k in seam._WEIGHT_PLANES}
        assert keys and not (keys & served), "a served ada_lin weight must not enter the weight-operand cache"
    seam.uninstall_cond(m)
    assert not _bound(m)
