"""seam.fused_mlp_func_amp / fused_mlp_func_amp_grad on the GPU: the half-precision FFN (csrc/gemm_half.hip, csrc/mlp_half.hip) against float64, fp16 and bf16.

Reference = float64 forward and backward on the CPU on the operands as the kernels see them: x and the weights after .to(dtype), the biases in their fp32 values (the
test's biases are representable in the half dtype, so the half run below sees the same numbers), dy in half.  e_torch = the error, against that float64 result, of
torch's CPU autograd run in the half dtype on the same operands (F.linear, F.gelu(approximate='tanh'), F.linear).  Bar, for y, dx, dW1, dW2, db1, db2 separately, with
u = 2^-11 (fp16) / 2^-8 (bf16):
    err <= 2 e_torch + u max|ref| + 2e-5 max(1, max|ref|)
Every case asserts that e_torch is finite and prints err, e_torch, the bar and max|ref| per tensor.

Cases (M, Cin, hid, Cout), chosen for the GEMM's 128 x 128 tile, its 32-deep K-step and 4-stage ring, and the 32-row padding of the wgrad K dimension:
(1, 32, 32, 32) one row, one K-step; (33, 96, 128, 32) with every 7th row of x times 30 (Mp = 64: 31 zero rows; three K-steps, shorter than the ring is deep + 1);
(70, 64, 256, 64) two column tiles; (161, 32, 160, 96) two row tiles with a tail, a 32-column tail in fc1; (300, 128, 512, 128) with dy = randn 2^5 (a
GradScaler-sized dy whose torch half gradients stay finite); all operands half (every gradient half); fp32 x under torch.autocast through a stand-in FFN module after
install_train_amp(ffn="half").

Bit checks: operand rounding = .to(dtype) (as stored and transposed), zero tails, sentinels behind every buffer; _amp_grad under grad = _amp; repeated backward passes;
each gradient alone = the full run; misaligned and stride-0 dy = their aligned copies; an fp16 overflow gives inf in its own row only; an in-place weight update
replaces the cached operands; h^T of sdvar_op_gelu_bwd_h = the h that fc1's epilogue wrote; a one-row slice of a wider buffer = its dense copy.  A dy of another
dtype and double backward raise.

Measured on an MI355X (37 tests, under 3 s): the largest err / bar over all cases is 0.34 (y, bf16, reference call: err 1.26e-2 = e_torch - the rounding of y itself); per
tensor y 0.34, dx 0.24, dW1 0.27, dW2 0.33, db1 0.22, db2 0.31 (all operands half; with fp32 operands the unrounded fp32 gradients stay at dx 0.21, dW1 0.24, dW2 0.28,
db1 0.22 and db2 is exact to fp32 rounding: err <= 6e-5 at max|ref| 1667).  A CPU emulation of the contract gives 0.33 for y on the same cases.  DESIGN.md 4k.
"""
import math
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import rnd
from sdvar_amd import engine as E
from sdvar_amd import seam

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
NAMES = ("y", "dx", "dW1", "dW2", "db1", "db2")
CODE = {torch.float16: 1, torch.bfloat16: 2}
_REFS = {}
# label -> (seed, M, Cin, hid, Cout, scale every 7th row of x, dy scale)
CASES = {"one row": (10, 1, 32, 32, 32, 1.0, 1.0), "31 zero rows": (20, 33, 96, 128, 32, 30.0, 1.0), "two column tiles": (30, 70, 64, 256, 64, 1.0, 1.0),
         "row tail": (40, 161, 32, 160, 96, 1.0, 1.0), "scaled dy": (50, 300, 128, 512, 128, 1.0, 32.0)}


def _u(dtype):
    return 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8


@pytest.fixture(autouse=True)
def _grad_mode_on():
    """Grad mode is process-wide state and other test modules of the suite switch it off; these tests are about autograd."""
    with torch.enable_grad():
        yield


def _inputs(seed, M, Cin, hid, Cout, dtype, row_scale=1.0, dy_scale=1.0):
    """fp32 CPU x, W1, W2, b1, b2 (the biases representable in dtype) and the half dy."""
    x = rnd(seed, (M, Cin))
    x[::7] *= row_scale
    w1, w2 = rnd(seed + 1, (hid, Cin), Cin ** -0.5), rnd(seed + 2, (Cout, hid), hid ** -0.5)
    b1, b2 = rnd(seed + 3, (hid,), 0.5).to(dtype).float(), rnd(seed + 4, (Cout,), 0.5).to(dtype).float()
    dy = (rnd(seed + 5, (M, Cout)) * dy_scale).to(dtype)
    return x, w1, w2, b1, b2, dy


def _ffn_grads(x, w1, w2, b1, b2, dy):
    x, w1, w2, b1, b2 = (t.detach().clone().requires_grad_() for t in (x, w1, w2, b1, b2))
    y = F.linear(F.gelu(F.linear(x, w1, b1), approximate="tanh"), w2, b2)
    y.backward(dy)
    return [t.double() for t in (y.detach(), x.grad, w1.grad, w2.grad, b1.grad, b2.grad)]


def _refs(key, ops, dtype):
    """ops: fp32 CPU x, W1, W2, b1, b2 and the half dy -> (float64 reference, e_torch) for NAMES; computed once per key and never modified."""
    if key not in _REFS:
        x, w1, w2, b1, b2, dy = ops
        ref = _ffn_grads(x.to(dtype).double(), w1.to(dtype).double(), w2.to(dtype).double(), b1.double(), b2.double(), dy.double())
        tor = _ffn_grads(x.to(dtype), w1.to(dtype), w2.to(dtype), b1.to(dtype), b2.to(dtype), dy)
        _REFS[key] = (ref, [(t - r).abs().max().item() for t, r in zip(tor, ref)])
    return _REFS[key]


def _close(label, name, got, ref, e_torch, dtype):
    g = got.detach().cpu().double()
    assert g.shape == ref.shape, (label, name, g.shape, ref.shape)
    mref = ref.abs().max().item()
    err = (g - ref).abs().max().item()
    assert math.isfinite(e_torch) and math.isfinite(mref), f"{label} {name}: e_torch {e_torch}, max|ref| {mref}: an infinite bar hides everything"
    bar = 2 * e_torch + _u(dtype) * mref + 2e-5 * max(1.0, mref)
    print(f"{label} {str(dtype)[6:]} {name}: err {err:.3e}  e_torch {e_torch:.3e}  bar {bar:.3e}  max|ref| {mref:.3e}  err/bar {err / bar:.2f}")
    assert math.isfinite(err), f"{label} {name}: err {err}"
    assert err <= bar, f"{label} {name}: err {err:.3e} > bar {bar:.3e} (e_torch {e_torch:.3e}, max|ref| {mref:.3e})"


def _leaves(ops, dev, dtypes):
    """GPU leaves of x, W1, W2, b1, b2 in the given dtypes, and dy on the GPU."""
    return [t.to(dt).to(dev).requires_grad_() for t, dt in zip(ops[:5], dtypes)], ops[5].to(dev)


def _run(leaves, dy, dtype, fn=None, autocast=True):
    """One forward + backward; returns (y, dx, dW1, dW2, db1, db2)."""
    for t in leaves:
        t.grad = None
    x, w1, w2, b1, b2 = leaves
    with torch.autocast("cuda", dtype=dtype, enabled=autocast):
        y = (fn or seam.fused_mlp_func_amp_grad)(x, w1, w2, b1, b2)
    y.backward(dy)
    return (y.detach(),) + tuple(None if t.grad is None else t.grad.clone() for t in leaves)


# ------------------------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("label", list(CASES))
def test_fp32_operands_under_autocast_vs_fp64(dev, label, dtype):
    """The reference's case: fp32 x, fp32 master weights and biases under torch.autocast.  Half y, every gradient fp32 (unrounded)."""
    seed, M, Cin, hid, Cout, row_scale, dy_scale = CASES[label]
    ops = _inputs(seed, M, Cin, hid, Cout, dtype, row_scale, dy_scale)
    ref, e_torch = _refs((label, dtype), ops, dtype)
    leaves, dy = _leaves(ops, dev, [torch.float32] * 5)
    got = _run(leaves, dy, dtype)
    assert got[0].dtype == dtype and all(g.dtype == torch.float32 for g in got[1:])
    for name, g, r, e in zip(NAMES, got, ref, e_torch):
        _close(label, name, g, r, e, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_all_half_operands_vs_fp64(dev, dtype):
    """x, the weights and the biases all in the half dtype, no autocast: every gradient comes back in the half dtype."""
    label = "all half"
    ops = _inputs(60, 70, 64, 256, 64, dtype)
    ops = tuple(t.to(dtype).float() for t in ops[:5]) + (ops[5],)
    ref, e_torch = _refs((label, dtype), ops, dtype)
    leaves, dy = _leaves(ops, dev, [dtype] * 5)
    got = _run(leaves, dy, dtype, autocast=False)
    assert all(g.dtype == dtype for g in got)
    for name, g, r, e in zip(NAMES, got, ref, e_torch):
        _close(label, name, g, r, e, dtype)


class _FFN(nn.Module):
    """The reference's FFN (basic_var.py:33-52): the module global captured at construction, called with keywords."""

    def __init__(self, C_, hid, slot):
        super().__init__()
        self.fused_mlp_func = slot
        self.fc1, self.act, self.fc2 = nn.Linear(C_, hid), nn.GELU(approximate="tanh"), nn.Linear(hid, C_)

    def forward(self, x):
        if self.fused_mlp_func is not None:
            return self.fused_mlp_func(x=x, weight1=self.fc1.weight, weight2=self.fc2.weight, bias1=self.fc1.bias, bias2=self.fc2.bias, activation="gelu_approx",
                                       save_pre_act=self.training, return_residual=False, checkpoint_lvl=0, heuristic=0, process_group=None)
        return self.fc2(self.act(self.fc1(x)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_reference_call_through_ffn_forward(dev, dtype):
    """fp32 x (B, L, C) under torch.autocast through FFN.forward after install_train_amp(module, model, ffn='half')."""
    label = "reference call"
    B, L, C_, hid = 2, 35, 64, 256
    ops = _inputs(70, B * L, C_, hid, C_, dtype)
    ref, e_torch = _refs((label, dtype), ops, dtype)
    ffn = _FFN(C_, hid, None).to(dev)
    with torch.no_grad():
        for p, t in zip((ffn.fc1.weight, ffn.fc2.weight, ffn.fc1.bias, ffn.fc2.bias), ops[1:5]):
            p.copy_(t)
    mod = types.SimpleNamespace()
    seam.install_train_amp(mod, ffn, ffn="half")
    assert ffn.fused_mlp_func is seam.fused_mlp_func_amp_grad and mod.fused_mlp_func is seam.fused_mlp_func_amp_grad
    x = ops[0].reshape(B, L, C_).to(dev).requires_grad_()
    with torch.autocast("cuda", dtype=dtype):
        y = ffn(x)
    assert y.shape == (B, L, C_) and y.dtype == dtype
    y.backward(ops[5].to(dev).reshape(B, L, C_))
    got = (y.detach().reshape(B * L, C_), x.grad.reshape(B * L, C_), ffn.fc1.weight.grad, ffn.fc2.weight.grad, ffn.fc1.bias.grad, ffn.fc2.bias.grad)
    assert all(g.dtype == torch.float32 for g in got[1:])
    for name, g, r, e in zip(NAMES, got, ref, e_torch):
        _close(label, name, g, r, e, dtype)


# ------------------------------------------------------------------------------------------------------------------ bits
SENT = 0x7B7B


def _unblock(op, rows, K):
    """The K-blocked operand [K/32][rows][32] as a (rows, K) int16 tensor."""
    return op[:rows * K].view(K // 32, rows, 32).permute(1, 0, 2).reshape(rows, K)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("src", ["fp32", "half"])
def test_operand_rounding_is_a_cast_with_zero_tails_and_intact_sentinels(dev, dtype, src):
    lib, st = E.load_library(), E._stream()
    rows, cols, ld = 45, 96, 104                          # 45 rows pad to 64: 19 zero rows; a leading dimension wider than the matrix
    x = rnd(80, (rows, ld), 3.0)
    x[3, 5], x[4, 6], x[5, 7], x[6, 8] = 7e4, -7e4, 65519.9, 1e-7          # beyond fp16's range: inf, not a clamp; fp16's last rounding boundary; an fp16 subnormal
    xin = (x if src == "fp32" else x.to(dtype)).to(dev)
    want = xin[:, :cols].to(dtype).view(torch.int16)
    if dtype == torch.float16 and src == "fp32":
        assert torch.isinf(xin[:, :cols].to(dtype)[3, 5]) and torch.isinf(xin[:, :cols].to(dtype)[4, 6])
    part_want = None
    Kp = 64
    for transpose, n in ((0, rows * cols), (1, cols * Kp)):
        out = torch.full((n + 64,), SENT, dtype=torch.int16, device=dev)
        part = torch.full((Kp // 32 * cols + 8,), -7.0, dtype=torch.float32, device=dev) if transpose else None
        E._check(lib.sdvar_op_half_operand(seam._p(xin), 0 if src == "fp32" else CODE[dtype], ld, rows, cols, CODE[dtype], transpose, seam._p(out), seam._p(part), st))
        assert (out[n:] == SENT).all(), "the kernel wrote behind its operand"
        if not transpose:
            assert torch.equal(_unblock(out, rows, cols), want)
        else:
            got = _unblock(out, cols, Kp)
            assert torch.equal(got[:, :rows], want.t()) and (got[:, rows:] == 0).all()
            assert (part[Kp // 32 * cols:] == -7.0).all()
            v = xin[:, :cols].to(dtype).float()
            v = torch.cat([v, torch.zeros(Kp - rows, cols, device=dev)]).view(Kp // 32, 32, cols)
            s = torch.zeros(Kp // 32, cols, device=dev)
            for r in range(32):                           # the kernel's order: row by row in fp32
                s = s + v[:, r]
            part_want = s
            assert torch.equal(part[:Kp // 32 * cols].view(Kp // 32, cols).nan_to_num(nan=1.5), part_want.nan_to_num(nan=1.5))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_gelu_bwd_h_outputs_tails_and_sentinels(dev, dtype):
    lib, st = E.load_library(), E._stream()
    M, N, Mp = 37, 96, 64
    dh = rnd(81, (M, N)).to(dev)
    p = rnd(82, (M, N), 2.0).to(dtype)
    p[0, :4] = torch.tensor([30000.0, -30000.0, 0.0, -0.0]).to(dtype)          # both ends of g': 1 and 0, finite
    p = p.to(dev)
    bufs = [torch.full((n + 64,), SENT, dtype=torch.int16, device=dev) for n in (M * N, N * Mp, N * Mp)]
    part = torch.full((Mp // 32 * N + 8,), -7.0, dtype=torch.float32, device=dev)
    E._check(lib.sdvar_op_gelu_bwd_h(seam._p(dh), seam._p(p), M, N, CODE[dtype], seam._p(bufs[0]), seam._p(bufs[1]), seam._p(bufs[2]), seam._p(part), st))
    for b, n in zip(bufs, (M * N, N * Mp, N * Mp)):
        assert (b[n:] == SENT).all(), "the kernel wrote behind its operand"
    assert (part[Mp // 32 * N:] == -7.0).all()
    dpre, dpre_t, h_t = _unblock(bufs[0], M, N), _unblock(bufs[1], N, Mp), _unblock(bufs[2], N, Mp)
    assert torch.equal(dpre_t[:, :M], dpre.t()) and (dpre_t[:, M:] == 0).all() and (h_t[:, M:] == 0).all()
    dv = dpre.contiguous().view(dtype).float()
    assert torch.isfinite(dv).all() and dv[0, 0] == dh[0, 0].to(dtype).float() and dv[0, 1] == 0 and dv[0, 2] == (0.5 * dh[0, 2]).to(dtype).float()
    # against float64: dpre and h to a rounding of the half dtype
    p64 = p.double().cpu().requires_grad_()
    h64 = F.gelu(p64, approximate="tanh")
    h64.backward(dh.double().cpu())
    u = _u(dtype)
    assert (dv.cpu().double() - p64.grad).abs().max().item() <= 1.01 * u * p64.grad.abs().max().item() + 1e-6
    hv = h_t[:, :M].t().contiguous().view(dtype).float().cpu().double()
    assert ((hv - h64.detach()).abs() <= 1.01 * u * h64.detach().abs() + 1e-6).all()
    s = torch.zeros(Mp // 32, N, device=dev)
    v = torch.cat([dv, torch.zeros(Mp - M, N, device=dev)]).view(Mp // 32, 32, N)
    for r in range(32):
        s = s + v[:, r]
    assert torch.equal(part[:Mp // 32 * N].view(Mp // 32, N), s)
    # each output alone has the bits of the full call
    for i in range(3):
        alone = torch.full_like(bufs[i], SENT)
        args = [None, None, None]
        args[i] = seam._p(alone)
        E._check(lib.sdvar_op_gelu_bwd_h(seam._p(dh) if i < 2 else None, seam._p(p), M, N, CODE[dtype], *args, None, st))
        assert torch.equal(alone, bufs[i])


@pytest.fixture(scope="module")
def bit_case():
    return _inputs(90, 161, 64, 160, 96, torch.float16)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_grad_twin_has_the_inference_bits_and_repeats_are_identical(dev, dtype, bit_case):
    leaves, dy = _leaves(bit_case, dev, [torch.float32] * 5)
    dy = dy.to(dtype)
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        y0 = seam.fused_mlp_func_amp(*leaves)
        y1 = seam.fused_mlp_func_amp_grad(*leaves)
    a = _run(leaves, dy, dtype)
    b = _run(leaves, dy, dtype)
    assert torch.equal(y0, y1) and torch.equal(y0, a[0])
    for name, ta, tb in zip(NAMES, a, b):
        assert torch.equal(ta, tb), f"{name}: a repeated pass differs"
    xh = [t.detach().to(dtype).requires_grad_() if i < 3 else t for i, t in enumerate(leaves)]          # half x and weights: the same rounded operands, the same y
    c = _run(xh, dy, dtype, autocast=False)
    assert torch.equal(c[0], y0)
    for name, g32, gh in zip(NAMES[1:4], a[1:4], c[1:4]):
        assert gh.dtype == dtype and torch.equal(g32.to(dtype), gh), f"{name}: the half gradient is not the rounded fp32 gradient"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_each_gradient_alone_has_the_bits_of_the_full_run(dev, dtype, bit_case):
    leaves, dy = _leaves(bit_case, dev, [torch.float32] * 5)
    dy = dy.to(dtype)
    full = _run(leaves, dy, dtype)
    for i, name in enumerate(NAMES[1:]):
        only = [t.detach().clone().requires_grad_(j == i) for j, t in enumerate(leaves)]
        got = _run(only, dy, dtype)
        assert torch.equal(got[0], full[0])
        assert all((g is None) == (j != i) for j, g in enumerate(got[1:])), f"{name}: a gradient nobody asked for was returned"
        assert torch.equal(got[1 + i], full[1 + i]), f"{name} alone differs from the full run"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_misaligned_and_stride0_dy_give_the_bits_of_their_aligned_copies(dev, dtype, bit_case):
    leaves, dy = _leaves(bit_case, dev, [torch.float32] * 5)
    dy = dy.to(dtype)
    M, Cout = dy.shape
    want = _run(leaves, dy, dtype)
    flat = torch.zeros(M * Cout + 8, dtype=dtype, device=dev)
    mis = flat[1:1 + M * Cout].view(M, Cout)
    mis.copy_(dy)
    assert mis.data_ptr() % 16 != 0 and mis.is_contiguous()
    for name, w, g in zip(NAMES, want, _run(leaves, mis, dtype)):
        assert torch.equal(w, g), f"{name}: a misaligned dy changed the result"
    wide = torch.zeros(M, Cout + 8, dtype=dtype, device=dev)
    wide[:, :Cout] = dy
    for name, w, g in zip(NAMES, want, _run(leaves, wide[:, :Cout], dtype)):
        assert torch.equal(w, g), f"{name}: a strided dy changed the result"
    ones = torch.ones(M, Cout, dtype=dtype, device=dev)
    want1 = _run(leaves, ones, dtype)
    exp = torch.ones((), dtype=dtype, device=dev).expand(M, Cout)
    assert exp.stride() == (0, 0)
    for name, w, g in zip(NAMES, want1, _run(leaves, exp, dtype)):
        assert torch.equal(w, g), f"{name}: a stride-0 dy changed the result"


def test_fp16_overflow_is_inf_in_its_own_row_only(dev):
    M, Cin, hid, Cout = 130, 64, 128, 64
    x, w1, w2 = rnd(91, (M, Cin)), rnd(92, (hid, Cin), Cin ** -0.5).abs(), rnd(93, (Cout, hid), hid ** -0.5).abs()
    w1[:, 7] = 2.0
    hot = x.clone()
    hot[129, 5] = 7e4                                     # rounds to +inf in fp16; positive weights: p, h and y of that row are +inf, never inf - inf
    hot[3, 7] = 60000.0                                   # inside the range on read, the fc1 sum overflows
    ys = []
    with torch.no_grad():
        for xi in (x, hot):
            for xd in (xi.to(dev), xi.to(torch.float16).to(dev)):
                with torch.autocast("cuda", dtype=torch.float16):
                    ys.append(seam.fused_mlp_func_amp(xd, w1.to(dev), w2.to(dev)))
    y, yh, yhot, yhoth = ys
    assert torch.equal(y, yh) and torch.equal(yhot, yhoth)                # fp32 x rounded on read = a half x
    assert torch.isfinite(y).all()
    assert (yhot[129] == float("inf")).all() and (yhot[3] == float("inf")).all()
    keep = [r for r in range(M) if r not in (3, 129)]
    assert torch.equal(yhot[keep], y[keep]), "an overflowing row disturbed other rows"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_in_place_weight_update_replaces_the_cached_operands(dev, dtype, bit_case):
    seam.clear_caches()
    leaves, dy = _leaves(bit_case, dev, [torch.float32] * 5)
    dy = dy.to(dtype)
    first = _run(leaves, dy, dtype)
    n = len(seam._WEIGHT_PLANES)
    assert n == 4                                         # W1, W2 as stored and transposed
    with torch.no_grad():
        leaves[1].mul_(1.25)
        leaves[2].add_(0.01)
    second = _run(leaves, dy, dtype)
    assert len(seam._WEIGHT_PLANES) == n, "an in-place update stranded a stale operand"
    assert not torch.equal(first[0], second[0])
    fresh = [t.detach().clone().requires_grad_() for t in leaves]          # other addresses: new cache entries built from the updated values
    want = _run(fresh, dy, dtype)
    for name, w, g in zip(NAMES, want, second):
        assert torch.equal(w, g), f"{name}: the step after an in-place update did not see the updated weights"
    seam.clear_caches()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_h_t_has_the_bits_of_the_fc1_epilogue(dev, dtype):
    """h is never stored for the backward: sdvar_op_gelu_bwd_h recomputes it from the saved p.  What it writes as h^T must be, bit for bit, what fc1's epilogue
    wrote as fc2's operand - and p as the epilogue stores it must be the input that gives it."""
    lib, st = E.load_library(), E._stream()
    M, N, K, Mp = 37, 96, 64, 64
    x, w, b = rnd(83, (M, K), 2.0).to(dev), rnd(84, (N, K), 0.5).to(dev), rnd(85, (N,)).to(dev)
    xo, wo = seam._half_operand(x, dtype, False), seam._half_operand(w, dtype, False)
    h = torch.full((M * N + 64,), SENT, dtype=torch.int16, device=dev)
    p = torch.empty(M, N, dtype=dtype, device=dev)
    E._check(lib.sdvar_op_gemm_h(seam._p(xo), seam._p(wo), CODE[dtype], seam._p(b), None, 0, 0, seam._p(h), seam._p(p), M, N, K, 1, st))
    assert (h[M * N:] == SENT).all()
    h_t = torch.full((N * Mp,), SENT, dtype=torch.int16, device=dev)
    E._check(lib.sdvar_op_gelu_bwd_h(None, seam._p(p), M, N, CODE[dtype], None, None, seam._p(h_t), None, st))
    assert torch.equal(_unblock(h_t, N, Mp)[:, :M], _unblock(h, M, N).t())
    h2 = torch.full_like(h, SENT)                           # without p_out the epilogue writes the same h
    E._check(lib.sdvar_op_gemm_h(seam._p(xo), seam._p(wo), CODE[dtype], seam._p(b), None, 0, 0, seam._p(h2), None, M, N, K, 1, st))
    assert torch.equal(h, h2)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_double_backward_and_a_dy_of_the_wrong_dtype_raise(dev, dtype, bit_case):
    leaves, dy = _leaves(bit_case, dev, [torch.float32] * 5)
    dy = dy.to(dtype)
    with torch.autocast("cuda", dtype=dtype):
        y = seam.fused_mlp_func_amp_grad(*leaves)
    # autograd itself casts a mismatched gradient before it reaches a Function, so the check is reached by calling the backward on the graph node directly
    with pytest.raises(E.SdvarError, match="fused_mlp_func_amp_grad.*gradient of the output"):
        seam._MlpAmpGrad.backward(y.grad_fn, dy.float())
    other = torch.bfloat16 if dtype == torch.float16 else torch.float16
    with pytest.raises(E.SdvarError, match="gradient of the output"):
        seam._MlpAmpGrad.backward(y.grad_fn, dy.to(other))
    (gx,) = torch.autograd.grad(y, leaves[0], dy, create_graph=True)
    assert not gx.requires_grad                                       # no graph is built through the backward ...
    with pytest.raises(RuntimeError, match="does not require grad"):
        gx.sum().backward()
    (gx,) = torch.autograd.grad(y, leaves[0], dy.clone().requires_grad_(), create_graph=True)
    assert gx.requires_grad                                           # ... and where a differentiable dy asks for one, differentiating it raises
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("src", ["fp32", "half"])
def test_one_row_of_a_wider_buffer_is_a_valid_call(dev, dtype, src):
    """A (1, C) slice of a wider buffer counts as dense whatever its row stride is (33 here: no multiple of 4 or 8); it has the bits of its dense copy."""
    ops = _inputs(95, 1, 32, 64, 32, dtype)
    xdt = torch.float32 if src == "fp32" else dtype
    wide = torch.zeros(1, 33, dtype=xdt, device=dev)
    wide[:, :32] = ops[0].to(xdt).to(dev)
    xs = wide[:, :32]
    assert xs.stride(0) == 33 and xs.is_contiguous() and xs.data_ptr() % 16 == 0
    leaves, dy = _leaves(ops, dev, [xdt] + [torch.float32] * 4)
    want = _run(leaves, dy, dtype)
    got = _run([xs.detach().requires_grad_()] + leaves[1:], dy, dtype)
    for name, w, g in zip(NAMES, want, got):
        assert torch.equal(w, g), f"{name}: the one-row slice differs from its dense copy"
