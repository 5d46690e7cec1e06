"""seam.linear / linear_grad / linear_amp / linear_amp_grad and csrc/linear_train.hip on the GPU: the dense linears, forward and backward, against float64.

Reference = float64 forward and backward on the CPU on the operands as the kernels see them: fp32 values in the fp32 modes; x and the weight after .to(dtype), the
bias in its fp32 value (representable in the half dtype) and dy in half in the half modes.  Bars, per tensor (y, dx, dW, db):
    fp32 modes f32 / f16x2 / bf16x3:   err <= 2e-5 max|ref|                                            (the scale-free bar of tests/test_gpu_seam_mlp_grad.py)
    fp16 / bf16:                       err <= 2 e_torch + u max|ref| + 2e-5 max(1, max|ref|),  u = 2^-11 / 2^-8   (the rule of tests/test_gpu_seam_mlp_amp.py)
e_torch = the error, against the float64 result, of torch's CPU autograd run in the half dtype on the same operands; it is asserted finite.  Every test prints what
it measured.

Cases (M, K, N), chosen for the 32-row padding of the wgrad K dimension, the GEMM's 32-deep K-step and 128-wide tile and the 32 x 64 transposing tile: (1, 32, 32);
(33, 96, 32) with every 7th row of x times 30 (Mp = 64: 31 zero rows); (70, 64, 256); (161, 32, 96); (300, 128, 512) with dy 2^5 in the half modes and dy 1e-7 in the
fp32 modes (what mode f16x2 fails without its dy scale); (8, 128, 768), ada_lin with M = B; a 3-D x (2, 35, 64) with N 96 and no bias; all operands half.

Bit checks: the three entries against the single-purpose entries they replace (operands as stored and transposed, every format and dtype, zero tails, sentinels,
each output alone), colsum_part finished by sdvar_op_colsum against float64, grad twin under no_grad = inference twin, repeats, each gradient alone, misaligned and
stride-0 dy, in-place weight updates, an fp16 overflow.  Saved bytes under saved_tensors_hooks.  The stand-in model of tests/seam_linear_model.py through the
installers against its own float64 run; there e_torch is torch's CPU run of the same module under torch.autocast("cpu", dtype).

Measured on an MI355X (86 tests, under 4 s): the largest err / bar is 0.019 in the fp32 modes (y of (300, 128, 512), mode f32; with dy 1e-7 mode f16x2 stays below 0.01
on every tensor), 0.32 in the half modes (y, bf16, one row: err 7.45e-3 = e_torch, the rounding of y itself); through the installers 0.036 (fp32 modes, q_bias) and
0.51 (bf16, fc2.bias: err 1.03e-2, e_torch 6.6e-3, max|ref| 1.75); db from the 32-row partials 0.08 of its bar.  DESIGN.md 4o."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rnd
from sdvar_amd import engine as E
from sdvar_amd import seam
import seam_linear_model as SM

pytestmark = pytest.mark.gpu

MODES = ("f32", "f16x2", "bf16x3")
DTYPES = [torch.float16, torch.bfloat16]
NAMES = ("y", "dx", "dW", "db")
CODE = {torch.float16: 1, torch.bfloat16: 2}
FMT = {"f32": 0, "f16x2": 2, "bf16x3": 3}
NPL = {"f32": 1, "f16x2": 2, "bf16x3": 3}
SENT = 0x7B7B
_REFS = {}
# label -> (seed, x shape, N, bias, scale of every 7th row of x, dy scale in the half modes, dy scale in the fp32 modes)
CASES = {"one row": (10, (1, 32), 32, True, 1.0, 1.0, 1.0), "31 zero rows": (20, (33, 96), 32, True, 30.0, 1.0, 1.0),
         "two column tiles": (30, (70, 64), 256, True, 1.0, 1.0, 1.0), "row tail": (40, (161, 32), 96, True, 1.0, 1.0, 1.0),
         "scaled dy": (50, (300, 128), 512, True, 1.0, 32.0, 1e-7), "ada_lin": (60, (8, 128), 768, True, 1.0, 1.0, 1.0),
         "3-D no bias": (70, (2, 35, 64), 96, False, 1.0, 1.0, 1.0)}


def _u(dtype):
    return 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8


@pytest.fixture(autouse=True)
def _state():
    """Grad mode is process-wide state and other test modules switch it off; the GEMM mode and the caches are put back."""
    with torch.enable_grad():
        yield
    seam.configure(gemm_mode=E.DEFAULT_GEMM_MODE)
    seam.clear_caches()


def _inputs(label, half=None):
    """fp32 CPU x, W, b (None without a bias; representable in `half` when given) and dy (fp32, or `half`)."""
    seed, xshape, N, bias, row_scale, dy_half, dy_f32 = CASES[label]
    K = xshape[-1]
    x = rnd(seed, xshape)
    x.view(-1, K)[::7] *= row_scale
    w = rnd(seed + 1, (N, K), K ** -0.5)
    b = rnd(seed + 2, (N,), 0.5) if bias else None
    dy = rnd(seed + 3, tuple(xshape[:-1]) + (N,))
    if half is None:
        return x, w, b, dy * dy_f32
    return x, w, None if b is None else b.to(half).float(), (dy * dy_half).to(half)


def _lin_grads(x, w, b, dy):
    x, w = x.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
    b = None if b is None else b.detach().clone().requires_grad_()
    y = F.linear(x, w, b)
    y.backward(dy)
    return [t.double() for t in (y.detach(), x.grad, w.grad)] + [None if b is None else b.grad.double()]


def _refs(key, ops, half):
    """(float64 reference, e_torch) for NAMES, computed once per key and never modified; e_torch is None in the fp32 modes."""
    if key not in _REFS:
        x, w, b, dy = ops
        if half is None:
            _REFS[key] = (_lin_grads(x.double(), w.double(), None if b is None else b.double(), dy.double()), None)
        else:
            ref = _lin_grads(x.to(half).double(), w.to(half).double(), None if b is None else b.double(), dy.double())
            tor = _lin_grads(x.to(half), w.to(half), None if b is None else b.to(half), dy)
            _REFS[key] = (ref, [None if r is None else (t - r).abs().max().item() for t, r in zip(tor, ref)])
    return _REFS[key]


def _close(label, name, got, ref, half=None, e_torch=None):
    g = got.detach().cpu().double()
    assert g.shape == ref.shape, (label, name, g.shape, ref.shape)
    mref, err = ref.abs().max().item(), (g - ref).abs().max().item()
    if half is None:
        bar = 2e-5 * mref
        print(f"{label} {name}: err {err:.3e}  bar {bar:.3e}  max|ref| {mref:.3e}  err/bar {err / bar:.3f}")
    else:
        assert math.isfinite(e_torch) and math.isfinite(mref), f"{label} {name}: e_torch {e_torch}, max|ref| {mref}: an infinite bar hides everything"
        bar = 2 * e_torch + _u(half) * mref + 2e-5 * max(1.0, mref)
        print(f"{label} {str(half)[6:]} {name}: err {err:.3e}  e_torch {e_torch:.3e}  bar {bar:.3e}  max|ref| {mref:.3e}  err/bar {err / bar:.3f}")
    assert math.isfinite(err), f"{label} {name}: err {err}"
    assert err <= bar, f"{label} {name}: err {err:.3e} > bar {bar:.3e} (max|ref| {mref:.3e})"


def _leaves(ops, dev, dtypes=(torch.float32,) * 3, grad=(True, True, True)):
    return [None if t is None else t.to(dt).to(dev).requires_grad_(g) for t, dt, g in zip(ops[:3], dtypes, grad)], ops[3].to(dev)


def _run(leaves, dy, fn, autocast=None):
    """One forward + backward; returns (y, dx, dW, db)."""
    for t in leaves:
        if t is not None:
            t.grad = None
    with torch.autocast("cuda", dtype=autocast or torch.float16, enabled=autocast is not None):
        y = fn(*leaves)
    y.backward(dy)
    return (y.detach(),) + tuple(None if t is None or t.grad is None else t.grad.clone() for t in leaves)


# ------------------------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("label", list(CASES))
def test_fp32_modes_vs_fp64(dev, label, mode):
    seam.configure(gemm_mode=mode)
    ops = _inputs(label)
    ref, _ = _refs((label, None), ops, None)
    leaves, dy = _leaves(ops, dev)
    got = _run(leaves, dy, seam.linear_grad)
    assert all(g is None or g.dtype == torch.float32 for g in got)
    for name, g, r in zip(NAMES, got, ref):
        if r is not None:
            _close(f"{label} {mode}", name, g, r)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("label", list(CASES))
def test_fp32_operands_under_autocast_vs_fp64(dev, label, dtype):
    """The reference's case: fp32 x, fp32 master weight and bias under torch.autocast.  Half y, every gradient fp32 (unrounded)."""
    ops = _inputs(label, dtype)
    ref, e_torch = _refs((label, dtype), ops, dtype)
    leaves, dy = _leaves(ops, dev)
    got = _run(leaves, dy, seam.linear_amp_grad, autocast=dtype)
    assert got[0].dtype == dtype and all(g is None or g.dtype == torch.float32 for g in got[1:])
    for name, g, r, e in zip(NAMES, got, ref, e_torch):
        if r is not None:
            _close(label, name, g, r, dtype, e)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_all_half_operands_vs_fp64(dev, dtype):
    """x, the weight and the bias all in the half dtype, no autocast: every gradient comes back in the half dtype."""
    x, w, b, dy = _inputs("two column tiles", dtype)
    ops = (x.to(dtype).float(), w.to(dtype).float(), b, dy)
    ref, e_torch = _refs(("all half", dtype), ops, dtype)
    leaves, dy = _leaves(ops, dev, (dtype,) * 3)
    got = _run(leaves, dy, seam.linear_amp_grad)
    assert all(g.dtype == dtype for g in got)
    for name, g, r, e in zip(NAMES, got, ref, e_torch):
        _close("all half", name, g, r, dtype, e)


# ------------------------------------------------------------------------------------------------------------------ the entries, bit for bit
def _unblock(op, rows, K):
    """A K-blocked plane [K/32][rows][32] as a (rows, K) tensor."""
    return op[:rows * K].view(K // 32, rows, 32).permute(1, 0, 2).reshape(rows, K)


def _hard_dy(dev, rows=45, cols=96, ld=104):
    """45 rows pad to 64 (19 zero rows), 96 columns = one and a half transposing tiles, a leading dimension wider than the matrix; values beyond fp16's range, at its
    last rounding boundary and in its subnormals."""
    x = rnd(80, (rows, ld), 3.0)
    x[3, 5], x[4, 6], x[5, 7], x[6, 8] = 7e4, -7e4, 65519.9, 1e-7
    return x.to(dev), rows, cols, ld


def _row_order_sums(v, Kp):
    """float[Kp/32][cols]: the column sums of v (rows, cols) fp32 over each block of 32 rows, added row by row in fp32 - the kernels' order."""
    rows, cols = v.shape
    v = torch.cat([v, torch.zeros(Kp - rows, cols, device=v.device)]).view(Kp // 32, 32, cols)
    s = torch.zeros(Kp // 32, cols, device=v.device)
    for r in range(32):
        s = s + v[:, r]
    return s


@pytest.mark.parametrize("mode,scaled", [("f32", False), ("f16x2", False), ("f16x2", True), ("bf16x3", False)], ids=["f32", "f16x2", "f16x2 scaled", "bf16x3"])
def test_grad_operands_has_the_bits_of_the_entries_it_replaces(dev, mode, scaled):
    """A scale goes with format 2 only (asserted at the end of the other formats' runs)."""
    lib, st = E.load_library(), E._stream()
    x, rows, cols, ld = _hard_dy(dev)
    Kp, fmt, npl = 64, FMT[mode], NPL[mode]
    dense = x[:, :cols].contiguous()
    el = torch.float32 if mode == "f32" else torch.int16
    sent = 123.5 if mode == "f32" else SENT
    n, nt, pad = rows * cols, cols * Kp, 64
    sc = torch.zeros(4, device=dev) if scaled else None
    # what the backward launched before: split (with its own absmax scale), transpose_operand, colsum
    want = want_t = None
    if mode != "f32":
        want = torch.full((npl, n + pad), SENT, dtype=torch.int16, device=dev)
        if mode == "f16x2":
            E._check(lib.sdvar_op_split_planes_f16(seam._p(dense), seam._p(want), rows, cols, n + pad, seam._p(sc), st))
        else:
            E._check(lib.sdvar_op_split_planes(seam._p(dense), seam._p(want), rows, cols, n + pad, st))
    if scaled:
        assert sc[0].item() == 2.0 ** -4 and sc[1].item() == 16.0          # max|dy| = 7e4 = 0.53 * 2^17: S = 13 - 17
    want_t = torch.full((npl, nt + pad), sent, dtype=el, device=dev)
    E._check(lib.sdvar_op_transpose_operand(seam._p(x), ld, rows, cols, fmt, seam._p(want_t), nt + pad, seam._p(sc), st))
    out = None if mode == "f32" else torch.full((npl, n + pad), SENT, dtype=torch.int16, device=dev)
    out_t = torch.full((npl, nt + pad), sent, dtype=el, device=dev)
    part = torch.full((Kp // 32 * cols + 8,), -7.0, device=dev)
    E._check(lib.sdvar_op_grad_operands(seam._p(x), ld, rows, cols, fmt, seam._p(sc), seam._p(out), n + pad, seam._p(out_t), nt + pad, seam._p(part), st))
    if out is not None:
        assert torch.equal(out, want), "the row-major operand differs from sdvar_op_split_planes*"
        assert (out[:, n:] == SENT).all()
    assert torch.equal(out_t.view(torch.int32) if mode == "f32" else out_t, want_t.view(torch.int32) if mode == "f32" else want_t), "dy^T differs from sdvar_op_transpose_operand"
    assert (out_t[:, nt:] == sent).all(), "the kernel wrote behind its operand"
    for p in range(npl):                                      # zero tails in every plane
        t = out_t[p, :nt].view(cols, Kp) if mode == "f32" else _unblock(out_t[p], cols, Kp)
        assert (t[:, rows:] == 0).all()
    assert (part[Kp // 32 * cols:] == -7.0).all()
    got_part = part[:Kp // 32 * cols].view(Kp // 32, cols)
    assert torch.equal(got_part, _row_order_sums(dense, Kp)), "colsum_part: the sums of the UNSCALED dy in row order"
    db = torch.empty(cols, device=dev)
    E._check(lib.sdvar_op_colsum(seam._p(got_part), cols, Kp // 32, cols, seam._p(db), st))
    err = (db.double().cpu() - dense.double().sum(0).cpu()).abs()
    bar = 40 * 2.0 ** -24 * dense.double().abs().sum(0).cpu()
    print(f"grad_operands {mode}: db worst err / bar {(err / bar).max().item():.3f}")
    assert (err <= bar).all()
    # each output alone has the bits of the full call
    for i, full in enumerate((out, out_t, part)):
        if full is None:
            continue
        alone = torch.full_like(full, -7.0 if i == 2 else sent if i == 1 else SENT)
        args = [None, None, None]
        args[i] = seam._p(alone)
        E._check(lib.sdvar_op_grad_operands(seam._p(x), ld, rows, cols, fmt, seam._p(sc), args[0], n + pad, args[1], nt + pad, args[2], st))
        same = torch.equal(alone.view(torch.int32), full.view(torch.int32)) if full.dtype == torch.float32 and i == 1 else torch.equal(alone, full)
        assert same, f"output {i} alone differs from the full call"
    if mode != "f16x2":
        with pytest.raises(E.SdvarError, match="scale goes with format 2"):
            E._check(lib.sdvar_op_grad_operands(seam._p(x), ld, rows, cols, fmt, seam._p(part), None, 0, seam._p(out_t), nt + pad, None, st))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("src", ["fp32", "half"])
def test_grad_operands_h_has_the_bits_of_two_half_operand_calls(dev, dtype, src):
    lib, st = E.load_library(), E._stream()
    x, rows, cols, ld = _hard_dy(dev)
    xin = x if src == "fp32" else x.to(dtype)
    xd = 0 if src == "fp32" else CODE[dtype]
    Kp, n, nt, pad = 64, rows * cols, cols * 64, 64
    want = torch.full((n + pad,), SENT, dtype=torch.int16, device=dev)
    want_t = torch.full((nt + pad,), SENT, dtype=torch.int16, device=dev)
    want_part = torch.full((Kp // 32 * cols + 8,), -7.0, device=dev)
    E._check(lib.sdvar_op_half_operand(seam._p(xin), xd, ld, rows, cols, CODE[dtype], 0, seam._p(want), None, st))
    E._check(lib.sdvar_op_half_operand(seam._p(xin), xd, ld, rows, cols, CODE[dtype], 1, seam._p(want_t), seam._p(want_part), st))
    out, out_t, part = torch.full_like(want, SENT), torch.full_like(want_t, SENT), torch.full_like(want_part, -7.0)
    E._check(lib.sdvar_op_grad_operands_h(seam._p(xin), xd, ld, rows, cols, CODE[dtype], seam._p(out), seam._p(out_t), seam._p(part), st))
    assert torch.equal(out, want) and torch.equal(out_t, want_t)
    assert torch.equal(part.view(torch.int32), want_part.view(torch.int32))          # inf - inf = NaN in fp16's column 5 / 6 partials: compared as bits
    assert torch.equal(_unblock(out, rows, cols), xin[:, :cols].to(dtype).view(torch.int16)), "the operand is not .to(dtype)"
    assert (_unblock(out_t, cols, Kp)[:, rows:] == 0).all() and (out[n:] == SENT).all() and (out_t[nt:] == SENT).all() and (part[Kp // 32 * cols:] == -7.0).all()
    if dtype == torch.float16:
        assert torch.isinf(out[:n].view(dtype)).sum().item() == 2, "7e4 is +-inf in fp16: nothing is clamped"
    for i, full in enumerate((out, out_t, part)):
        alone = torch.full_like(full, -7.0 if i == 2 else SENT)
        args = [None, None, None]
        args[i] = seam._p(alone)
        E._check(lib.sdvar_op_grad_operands_h(seam._p(xin), xd, ld, rows, cols, CODE[dtype], *args, st))
        assert torch.equal(alone.view(torch.int32) if i == 2 else alone, full.view(torch.int32) if i == 2 else full), f"output {i} alone differs from the full call"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("rows", [45, 1, 64])
def test_operand_transpose_h_equals_half_operand_of_the_row_major_matrix(dev, dtype, rows):
    lib, st = E.load_library(), E._stream()
    K, Kp = 96, (rows + 31) // 32 * 32
    x = rnd(81, (rows, K), 3.0)
    x[0, 5] = 7e4
    x = x.to(dev)
    op = seam._half_operand(x, dtype, False)
    want = torch.full((K * Kp + 64,), SENT, dtype=torch.int16, device=dev)
    E._check(lib.sdvar_op_half_operand(seam._p(x), 0, K, rows, K, CODE[dtype], 1, seam._p(want), None, st))
    got = torch.full_like(want, SENT)
    E._check(lib.sdvar_op_operand_transpose_h(seam._p(op), rows, K, seam._p(got), st))
    assert torch.equal(got, want)
    assert (_unblock(got, K, Kp)[:, rows:] == 0).all() and (got[K * Kp:] == SENT).all()
    assert torch.equal(_unblock(got, K, Kp)[:, :rows], x.to(dtype).view(torch.int16).t())


# ------------------------------------------------------------------------------------------------------------------ the functions, bit for bit
PATHS = [("f32", None), ("f16x2", None), ("bf16x3", None), (None, torch.float16), (None, torch.bfloat16)]
PATH_IDS = ["f32", "f16x2", "bf16x3", "fp16", "bf16"]


def _path(mode, half):
    if mode is not None:
        seam.configure(gemm_mode=mode)
    return (seam.linear, seam.linear_grad) if half is None else (seam.linear_amp, seam.linear_amp_grad)


def _bit_case(half):
    return _inputs("row tail", half)


@pytest.mark.parametrize("mode,half", PATHS, ids=PATH_IDS)
def test_grad_twin_has_the_inference_bits_and_repeats_are_identical(dev, mode, half):
    inf, fn = _path(mode, half)
    leaves, dy = _leaves(_bit_case(half), dev)
    with torch.no_grad(), torch.autocast("cuda", dtype=half or torch.float16, enabled=half is not None):
        y0, y1 = inf(*leaves), fn(*leaves)
    a, b = _run(leaves, dy, fn, half), _run(leaves, dy, fn, half)
    assert torch.equal(y0, y1) and torch.equal(y0, a[0])
    for name, ta, tb in zip(NAMES, a, b):
        assert torch.equal(ta, tb), f"{name}: a repeated pass differs"
    with pytest.raises(E.SdvarError, match="requires grad and grad mode is on"), torch.autocast("cuda", dtype=half or torch.float16, enabled=half is not None):
        inf(*leaves)


@pytest.mark.parametrize("mode,half", PATHS, ids=PATH_IDS)
def test_each_gradient_alone_has_the_bits_of_the_full_run(dev, mode, half):
    _, fn = _path(mode, half)
    ops = _bit_case(half)
    leaves, dy = _leaves(ops, dev)
    full = _run(leaves, dy, fn, half)
    for i, name in enumerate(NAMES[1:]):
        only, _ = _leaves(ops, dev, grad=tuple(j == i for j in range(3)))
        got = _run(only, dy, fn, half)
        assert torch.equal(got[0], full[0])
        assert all((g is None) == (j != i) for j, g in enumerate(got[1:])), f"{name}: a gradient nobody asked for was returned"
        assert torch.equal(got[1 + i], full[1 + i]), f"{name} alone differs from the full run"


@pytest.mark.parametrize("mode,half", PATHS, ids=PATH_IDS)
def test_misaligned_and_stride0_dy_give_the_bits_of_their_aligned_copies(dev, mode, half):
    _, fn = _path(mode, half)
    leaves, dy = _leaves(_bit_case(half), dev)
    M, N = dy.shape
    want = _run(leaves, dy, fn, half)
    flat = torch.zeros(M * N + 8, dtype=dy.dtype, device=dev)
    mis = flat[1:1 + M * N].view(M, N)
    mis.copy_(dy)
    assert mis.data_ptr() % 16 != 0 and mis.is_contiguous()
    for name, w, g in zip(NAMES, want, _run(leaves, mis, fn, half)):
        assert torch.equal(w, g), f"{name}: a misaligned dy changed the result"
    ones = torch.ones(M, N, dtype=dy.dtype, device=dev)
    want1 = _run(leaves, ones, fn, half)
    for t in leaves:
        t.grad = None
    with torch.autocast("cuda", dtype=half or torch.float16, enabled=half is not None):
        y = fn(*leaves)
    y.sum().backward()                                     # the stride-0 dy autograd itself makes
    for name, w, g in zip(NAMES[1:], want1[1:], [t.grad for t in leaves]):
        assert torch.equal(w, g), f"{name}: a stride-0 dy changed the result"


@pytest.mark.parametrize("mode,half", PATHS, ids=PATH_IDS)
def test_in_place_weight_update_replaces_the_cached_operands(dev, mode, half):
    _, fn = _path(mode, half)
    seam.clear_caches()
    leaves, dy = _leaves(_bit_case(half), dev)
    first = _run(leaves, dy, fn, half)
    n = 1 if mode == "f32" else 2                         # the weight as stored (mode f32 reads the weight itself) and transposed
    assert len(seam._WEIGHT_PLANES) == n
    with torch.no_grad():
        leaves[1].mul_(1.25)
    second = _run(leaves, dy, fn, half)
    assert len(seam._WEIGHT_PLANES) == n, "an in-place update stranded a stale operand"
    assert not torch.equal(first[0], second[0])
    fresh = [t.detach().clone().requires_grad_() for t in leaves]          # other addresses: new cache entries built from the updated values
    for name, w, g in zip(NAMES, _run(fresh, dy, fn, half), second):
        assert torch.equal(w, g), f"{name}: the step after an in-place update did not see the updated weight"


def test_fp16_overflow_is_inf_in_its_own_row_and_column_only(dev):
    M, K, N = 130, 64, 96
    x, w = rnd(91, (M, K)).abs(), rnd(92, (N, K), K ** -0.5).abs()          # positive operands: an inf never meets a -inf
    dy = rnd(93, (M, N)).abs().to(torch.float16)
    hot_x, hot_dy = x.clone(), dy.clone()
    hot_x[129, 5] = 7e4                                   # rounds to +inf in fp16 as it is read
    hot_dy[3, 70] = float("inf")                          # what a GradScaler must get to see
    res = []
    for xi, di in ((x, dy), (hot_x, hot_dy)):
        leaves = [xi.to(dev).requires_grad_(), w.to(dev).requires_grad_(), torch.zeros(N, device=dev).requires_grad_()]
        res.append(_run(leaves, di.to(dev), seam.linear_amp_grad, torch.float16))
    (y, dx, dw, db), (yh, dxh, dwh, dbh) = res
    assert all(torch.isfinite(t).all() for t in (y, dx, dw, db))
    rows = [r for r in range(M) if r != 129]
    assert (yh[129] == float("inf")).all() and torch.equal(yh[rows], y[rows]), "the overflowing row of x: inf in its own row of y only"
    rows = [r for r in range(M) if r != 3]
    assert (dxh[3] == float("inf")).all() and torch.equal(dxh[rows], dx[rows]), "the inf of dy: its own row of dx only"
    cols = [c for c in range(N) if c != 70]
    assert (dwh[70] == float("inf")).all() and dbh[70] == float("inf") and torch.equal(dbh[cols], db[cols])
    fin = torch.isfinite(dwh[cols])
    assert (~fin).sum().item() == len(cols), "dW = dy^T x_h: the inf of x (row 129, column 5) reaches column 5 of every row of dW, and nothing else"
    assert not fin[:, 5].any() and torch.equal(dwh[cols][:, [k for k in range(K) if k != 5]], dw[cols][:, [k for k in range(K) if k != 5]])


@pytest.mark.parametrize("half", DTYPES, ids=["fp16", "bf16"])
def test_double_backward_and_a_dy_of_the_wrong_dtype_raise(dev, half):
    leaves, dy = _leaves(_bit_case(half), dev)
    with torch.autocast("cuda", dtype=half):
        y = seam.linear_amp_grad(*leaves)
    # autograd itself casts a mismatched gradient before it reaches a Function, so the check is reached by calling the backward on the graph node directly
    with pytest.raises(E.SdvarError, match="linear_amp_grad.*gradient of the output"):
        seam._LinearAmpGrad.backward(y.grad_fn, dy.float())
    (gx,) = torch.autograd.grad(y, leaves[0], dy.clone().requires_grad_(), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()
    y32 = seam.linear_grad(*leaves)
    (gx,) = torch.autograd.grad(y32, leaves[0], dy.float().requires_grad_(), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


def test_one_row_of_a_wider_buffer_has_the_bits_of_its_dense_copy(dev):
    """A (1, K) slice of a wider buffer counts as dense whatever its row stride is (33 here: no multiple of 4)."""
    ops = _inputs("one row")
    wide = torch.zeros(1, 33, device=dev)
    wide[:, :32] = ops[0].to(dev)
    xs = wide[:, :32]
    assert xs.stride(0) == 33 and xs.is_contiguous()
    for mode, half in PATHS:
        _, fn = _path(mode, half)
        leaves, dy = _leaves(ops, dev)
        dy = dy if half is None else dy.to(half)
        want = _run(leaves, dy, fn, half)
        got = _run([xs.detach().requires_grad_()] + leaves[1:], dy, fn, half)
        for name, w, g in zip(NAMES, want, got):
            assert torch.equal(w, g), f"{mode or half} {name}: the one-row slice differs from its dense copy"


# ------------------------------------------------------------------------------------------------------------------ saved memory
@pytest.mark.parametrize("frozen", [False, True], ids=["trained", "frozen weight"])
@pytest.mark.parametrize("mode,half", [("f16x2", None), ("f32", None), (None, torch.bfloat16)], ids=["f16x2", "f32", "bf16"])
def test_saved_bytes(dev, mode, half, frozen):
    _, fn = _path(mode, half)
    ops = _bit_case(half)
    M, K = ops[0].shape
    leaves, dy = _leaves(ops, dev, grad=(True, not frozen, True))
    params = {t.data_ptr() for t in leaves[1:]}
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        with torch.autocast("cuda", dtype=half or torch.float16, enabled=half is not None):
            y = fn(*leaves)
    extra = sum(t.numel() * t.element_size() for t in saved if t.data_ptr() not in params)
    want = 0 if frozen else (4 if half is None else 2) * M * K
    print(f"saved besides parameters: {extra} bytes (M {M}, K {K}); expected {want}")
    assert extra == want
    y.backward(dy)
    assert leaves[0].grad is not None and (leaves[1].grad is None) == frozen


# ------------------------------------------------------------------------------------------------------------------ through the installer
@pytest.fixture
def slots():
    saved = SM.save_slots()
    yield SM
    SM.restore_slots(saved)


def _model_refs():
    """The stand-in model's float64 loss and gradients at loss scales 1 and 1024, and e_torch per tensor and half dtype: torch's CPU run under torch.autocast."""
    if "model" not in _REFS:
        m, feats, cond, w, mask = SM.model_and_inputs()
        args64 = tuple(t.double() for t in (feats, cond, w, mask))
        m = m.double()
        ref1 = SM.loss_and_grads(m, *args64)
        ref1k = {n: t * 1024.0 for n, t in ref1.items()}              # the loss scale is a power of two: exact
        m = m.float()
        e = {}
        for half in DTYPES:
            tor = SM.loss_and_grads(m, feats, cond, w, mask, autocast=half, scale=1024.0)
            e[half] = {n: (tor[n].double() - ref1k[n]).abs().max().item() for n in ref1k}
        _REFS["model"] = (ref1, ref1k, e)
    return _REFS["model"]


def _spy(monkeypatch):
    """Which weights went through linear_grad and which through linear_amp_grad."""
    seen = {"fp32": set(), "half": set()}
    for key, name in (("fp32", "linear_grad"), ("half", "linear_amp_grad")):
        orig = getattr(seam, name)

        def wrapper(x, weight, bias=None, _orig=orig, _key=key):
            seen[_key].add(weight.data_ptr())
            return _orig(x, weight, bias)
        monkeypatch.setattr(seam, name, wrapper)
    return seen


def _compare_model(tag, got, ref, half=None, e_torch=None):
    print(f"\n{tag}")
    for n, r in ref.items():
        assert n in got, f"{n} received no gradient"
        _close(tag, n, got[n], r, half, None if e_torch is None else e_torch[n])


@pytest.mark.parametrize("mode", MODES)
def test_stand_in_model_fp32_with_every_switch_on(dev, slots, monkeypatch, mode):
    ref, _, _ = _model_refs()
    m, feats, cond, w, mask = SM.model_and_inputs()
    m = m.to(dev)
    args = tuple(t.to(dev) for t in (feats, cond, w, mask))
    plain = SM.loss_and_grads(m, *args)
    seam.configure(gemm_mode=mode)
    seam.install_train(slots, m, ffn=True, adaln=True, qknorm=True, linears=True)
    seen = _spy(monkeypatch)
    got = SM.loss_and_grads(m, *args)
    lin = {n: q.weight.data_ptr() for n, q in m.named_modules() if "forward" in q.__dict__ and isinstance(q, torch.nn.Linear)}
    assert set(lin) == {"word_embed", "head", "block.attn.mat_qkv", "block.attn.proj", "block.ffn.fc1", "block.ffn.fc2", "block.ada_lin.1"}
    called = {n for n, p in lin.items() if p in seen["fp32"]}
    assert called == set(lin) - {"block.ffn.fc1", "block.ffn.fc2"} and not seen["half"]          # the FFN slot takes the weights, not the modules
    _compare_model(f"stand-in, install_train(every switch), mode {mode}", got, ref)
    seam.uninstall_linears(m)
    seam.uninstall_adaln(m)
    seam.uninstall_qknorm(m)
    assert not any("forward" in q.__dict__ for q in m.modules())
    SM.restore_slots({"slow_attn": SM._torch_attn, "flash_attn_func": None, "memory_efficient_attention": None, "fused_mlp_func": None})
    m.block.ffn.fused_mlp_func = None
    again = SM.loss_and_grads(m, *args)
    assert all(torch.equal(again[k], plain[k]) for k in plain), "uninstall_linears must restore the class forwards"


@pytest.mark.parametrize("half", DTYPES, ids=["fp16", "bf16"])
def test_stand_in_model_under_autocast_with_every_switch_on(dev, slots, monkeypatch, half):
    _, ref, e_torch = _model_refs()
    m, feats, cond, w, mask = SM.model_and_inputs()
    m = m.to(dev)
    args = tuple(t.to(dev) for t in (feats, cond, w, mask))
    seam.install_train_amp(slots, m, ffn="half", adaln=True, qknorm=True, linears=True)
    seen = _spy(monkeypatch)
    got = SM.loss_and_grads(m, *args, autocast=half, scale=1024.0)
    ptr = lambda q: q.weight.data_ptr()
    assert seen["fp32"] == {ptr(m.word_embed)}, "word_embed runs inside autocast(enabled=False) on a float32 x: the fp32 path, in the middle of an autocast run"
    assert seen["half"] == {ptr(m.head), ptr(m.block.attn.mat_qkv), ptr(m.block.attn.proj), ptr(m.block.ada_lin[1])}, "head and the block's linears: the half path"
    assert all(g.dtype == torch.float32 for g in got.values())
    _compare_model(f"stand-in, install_train_amp(every switch), autocast {half}", got, ref, half, e_torch[half])
    seam.uninstall_linears(m)
    assert all(not isinstance(q, torch.nn.Linear) for q in m.modules() if "forward" in q.__dict__)
