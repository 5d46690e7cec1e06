"""seam.fused_mlp_func_grad on the GPU (the forward's GEMMs + csrc/mlp_bwd.hip + four backward GEMMs) against
F.linear(F.gelu(F.linear(x, W1, b1), approximate="tanh"), W2, b2) run forward AND backward in float64 on the CPU, from the same rnd(...) inputs and the same upstream
gradient.

Bar, per tensor (y, dx, dW1, db1, dW2, db2) and scale-free: err <= 2e-5 * max|ref| - the project's GEMM bar WITHOUT its max(1, .) floor, because several cases have tiny
gradients on purpose and a floor of 1 would hide anything there.  Torch's own fp32 autograd on the CPU stays at or below 1.1e-6 * max|ref| on every plain case below
(M in {1, 5, 33, 130, 300}, (C, hid) = (128, 512) and (256, 1024), also with dy * 1e-7), so the bar leaves >= 18x headroom over the reference's own fp32 error.
The hard pre-activation cases use max(2e-5 * max|ref|, 4 x the error torch's fp32 CPU autograd makes against fp64 on the same inputs), computed in the test (the rule
of test_gpu_seam_grad_hard.py).  No bar comes from the code under test.  Every test prints the errors it measured.
Measured on an MI355X, largest error over every case and mode as a fraction of max|ref|: y 3.9e-7, dx 1.0e-6, dW1 6.2e-6, db1 8.9e-7, dW2 6.1e-7, db2 3.9e-8; the
GELU-backward producer's dpre is within 1.7e-7 |dh| of fp64, the column sums within 1.6e-6 absolute.
"""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import rnd
from sdvar_amd import engine as E
from sdvar_amd import seam

pytestmark = pytest.mark.gpu
NAMES = ("y", "dx", "dW1", "db1", "dW2", "db2")
DIMS = (128, 512, 128)
ODD = (96, 160, 96)                 # no multiple of a GEMM tile in any dimension


@pytest.fixture(autouse=True)
def _grad_mode_on():
    """Grad mode is process-wide state and other test modules of the suite switch it off; these tests are about autograd."""
    with torch.enable_grad():
        yield


@pytest.fixture(params=E.GEMM_MODES)
def mode(request):
    seam.configure(gemm_mode=request.param)
    try:
        yield request.param
    finally:
        seam.configure(gemm_mode=E.DEFAULT_GEMM_MODE)
        seam.clear_caches()


# ------------------------------------------------------------------------------------------------------------------ helpers
@functools.lru_cache(maxsize=None)
def _inputs(seed, xshape, dims):
    """(x, W1, b1, W2, b2, dy) fp32 on the CPU; shared between tests and never modified (callers derive variants out of place)."""
    Cin, hid, Cout = dims
    assert xshape[-1] == Cin
    return (rnd(seed, xshape), rnd(seed + 1, (hid, Cin), 1 / math.sqrt(Cin)), rnd(seed + 2, (hid,)), rnd(seed + 3, (Cout, hid), 1 / math.sqrt(hid)), rnd(seed + 4, (Cout,)),
            rnd(seed + 5, tuple(xshape[:-1]) + (Cout,)))


def _autograd(ops, dy, dtype):
    """The reference in `dtype` on the CPU -> (y, dx, dW1, db1, dW2, db2)."""
    x, W1, b1, W2, b2 = (t.detach().to(dtype).requires_grad_() for t in ops)
    y = F.linear(F.gelu(F.linear(x, W1, b1), approximate="tanh"), W2, b2)
    y.backward(dy.to(dtype))
    return (y.detach(), x.grad, W1.grad, b1.grad, W2.grad, b2.grad)


_REFS = {}


def _ref(key, ops, dy):
    """fp64 reference, computed once per case key."""
    if key not in _REFS:
        _REFS[key] = _autograd(ops, dy, torch.float64)
    return _REFS[key]


def _seam(dev, ops, dy, grad=(True,) * 5, call=None):
    """Leaves on the device through fused_mlp_func_grad -> (y, dx, dW1, db1, dW2, db2), None where no gradient was asked for."""
    x, W1, b1, W2, b2 = (t.to(dev).requires_grad_(g) for t, g in zip(ops, grad))
    y = (call or seam.fused_mlp_func_grad)(x, W1, W2, b1, b2)
    assert y.requires_grad and y.shape == tuple(ops[0].shape[:-1]) + (W2.shape[0],)
    y.backward(dy if dy.is_cuda else dy.to(dev))
    return (y.detach(), x.grad, W1.grad, b1.grad, W2.grad, b2.grad)


def _close(name, got, ref, floor=0.0):
    got = got.cpu().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), name
    err, top = (got - ref).abs().max().item(), ref.abs().max().item()
    lim = max(2e-5 * top, floor)
    print(f"{name}: err {err:.3e} = {err / top if top else 0.0:.2e} max|ref|, bar {lim:.3e} ({'2e-5 max|ref|' if lim == 2e-5 * top else '4 x torch fp32'}), max|ref| {top:.3e}")
    assert err <= lim, (name, err, lim)


def _close_all(got, ref, floors=None):
    for i, name in enumerate(NAMES):
        _close(name, got[i], ref[i], 0.0 if floors is None else floors[i])


def _equal(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------------------------ 1. parity
CASES = [((1, 1, 128), DIMS), ((1, 5, 128), DIMS), ((1, 31, 128), DIMS), ((1, 33, 128), DIMS), ((1, 130, 128), DIMS), ((2, 65, 128), DIMS), ((1, 33, 96), ODD)]


@pytest.mark.parametrize("xshape,dims", CASES, ids=lambda v: "x".join(map(str, v)))
def test_parity(dev, mode, xshape, dims):
    """M = 1, 5, 31, 33, 130 rows (padded K of the wgrad GEMMs 32, 32, 32, 64, 160), a (2, 65, C) batch and widths that are no multiple of any tile."""
    *ops, dy = _inputs(100, xshape, dims)
    _close_all(_seam(dev, ops, dy), _ref(("plain", xshape, dims), ops, dy))


# ------------------------------------------------------------------------------------------------------------------ 2. forward bits
def test_forward_bits(dev, mode):
    """Under grad the output has fused_mlp_func's bits (fc1 with the bias epilogue + the GELU operand kernel against fc1's fused GELU epilogue); with grad off, or no
    operand requiring grad, the grad twin is the inference function."""
    for xshape, dims in (((1, 33, 128), DIMS), ((1, 130, 128), DIMS), ((1, 33, 96), ODD)):
        *ops, dy = _inputs(100, xshape, dims)
        x, W1, b1, W2, b2 = (t.to(dev) for t in ops)
        with torch.no_grad():
            y0 = seam.fused_mlp_func(x, W1, W2, b1, b2)
            assert torch.equal(seam.fused_mlp_func_grad(x, W1, W2, b1, b2), y0)
        y1 = seam.fused_mlp_func_grad(x, W1, W2, b1, b2)                     # grad mode on, nothing requires grad
        assert not y1.requires_grad and torch.equal(y1, y0)
        y2 = seam.fused_mlp_func_grad(x.clone().requires_grad_(), W1, W2, b1, b2)
        assert y2.requires_grad and torch.equal(y2.detach(), y0)
        y3 = seam.fused_mlp_func_grad(x, W1, W2.clone().requires_grad_(), None, None)
        with torch.no_grad():
            assert torch.equal(y3.detach(), seam.fused_mlp_func(x, W1, W2))
        print(f"{xshape} {dims}: forward bit-identical")


# ------------------------------------------------------------------------------------------------------------------ 3. tiny and large gradients
@pytest.mark.parametrize("mul", [1e-7, 1e4])
def test_gradient_range(dev, mode, mul):
    """Upstream gradients at the magnitude of an fp32 training run (1e-7) and far above 1: the same scale-free bar.  Mode f16x2 fails the small case unless the
    gradient operands carry their own power-of-two scale."""
    xshape = (1, 130, 128)
    *ops, dy = _inputs(100, xshape, DIMS)
    dys = dy * mul
    _close_all(_seam(dev, ops, dys), _ref(("mul", mul), ops, dys))


def test_zero_upstream_gradient(dev, mode):
    *ops, dy = _inputs(100, (1, 33, 128), DIMS)
    got = _seam(dev, ops, torch.zeros_like(dy))
    for name, g in zip(NAMES[1:], got[1:]):
        assert torch.isfinite(g).all() and not g.any(), name
    print("dy = 0: every gradient exactly zero")


# ------------------------------------------------------------------------------------------------------------------ 4. hard pre-activations
def _hard(variant):
    x, W1, b1, W2, b2, dy = _inputs(100, (1, 130, 128), DIMS)
    if variant == "x30":
        x = x * 30
    elif variant == "heavy_rows":
        x = x * torch.exp(2 * rnd(77, (130, 1)))
    else:
        b1 = b1.clone()
        b1[::7] = 1e4
        b1[3::7] = -1e4
    return (x, W1, b1, W2, b2), dy


@pytest.mark.parametrize("variant", ["x30", "heavy_rows", "bias_1e4"])
def test_hard_pre_activations(dev, mode, variant):
    """Saturated GELUs (x * 30), rows of very different magnitude (x * exp(2 randn) per row) and pre-activations at +-1e4 (through bias1, where gelu' must be exactly
    1 / 0 and finite).  Bar per tensor: max(2e-5 max|ref|, 4 x torch's fp32 CPU autograd error against fp64 on the same inputs).  Which term is the bar (it depends on the CPU side alone; printed by the test): 2e-5 max|ref|
    for every tensor of all three cases - torch's fp32 autograd stays at or below 1.8e-6 max|ref| (x30, dW1), 2.8e-6 (heavy_rows, dW1) and 6.1e-7 (bias_1e4, dW2) on these
    inputs, so four times its error never reaches the first term."""
    ops, dy = _hard(variant)
    ref = _ref(("hard", variant), ops, dy)
    assert all(torch.isfinite(r).all() for r in ref)
    t32 = _autograd(ops, dy, torch.float32)
    floors = [4.0 * (a.double() - r).abs().max().item() for a, r in zip(t32, ref)]
    for name, f, r in zip(NAMES, floors, ref):
        print(f"{variant} {name}: torch fp32 error {f / 4:.3e} = {f / 4 / r.abs().max().item():.2e} max|ref|")
    _close_all(_seam(dev, ops, dy), ref, floors)


# ------------------------------------------------------------------------------------------------------------------ 5. subsets
def test_gradient_subsets(dev, mode):
    """Only what needs_input_grad asks for is computed, and a gradient computed alone has the bits it has in the full run."""
    *ops, dy = _inputs(100, (1, 130, 128), DIMS)
    full = _seam(dev, ops, dy)
    for grad in ((True, False, False, False, False), (False, True, True, True, True), (False, False, False, True, False), (False, False, False, False, True),
                 (False, False, True, False, False)):
        got = _seam(dev, ops, dy, grad)
        for name, g, f, need in zip(NAMES[1:], got[1:], full[1:], grad):
            assert (g is not None) == need, (grad, name)
            if need:
                assert torch.equal(g, f), (grad, name)
        assert torch.equal(got[0], full[0])
    print("subsets bit-identical to the full run")


# ------------------------------------------------------------------------------------------------------------------ 6. determinism
@pytest.mark.parametrize("xshape,dims", [((1, 130, 128), DIMS), ((1, 680, 256), (256, 1024, 256))], ids=["130", "680"])
def test_backward_is_deterministic(dev, mode, xshape, dims):
    *ops, dy = _inputs(200, xshape, dims)
    a, b = _seam(dev, ops, dy), _seam(dev, ops, dy)
    assert _equal(a, b)
    _close_all(a, _ref(("det", xshape), ops, dy))


# ------------------------------------------------------------------------------------------------------------------ 7. upstream layouts
def test_upstream_layouts(dev, mode):
    """y.sum().backward() hands the backward a stride-0 expansion; a transposed consumer a non-contiguous dy; x may be a non-contiguous view."""
    x, W1, b1, W2, b2, dy = _inputs(100, (2, 65, 128), DIMS)
    ops = (x, W1, b1, W2, b2)
    leaves = lambda: [t.to(dev).requires_grad_() for t in ops]
    # stride-0 dy
    ts = leaves()
    seam.fused_mlp_func_grad(ts[0], ts[1], ts[3], ts[2], ts[4]).sum().backward()
    ref = _ref("ones", ops, torch.ones_like(dy))
    _close_all((ref[0],) + tuple(t.grad for t in ts), ref)
    # a transposed consumer: dy arrives as a (65, 2, C) tensor viewed back
    ts = leaves()
    w = dy.transpose(0, 1).contiguous().to(dev)
    (seam.fused_mlp_func_grad(ts[0], ts[1], ts[3], ts[2], ts[4]).transpose(0, 1) * w).sum().backward()
    ref = _ref(("plain", (2, 65, 128), DIMS), ops, dy)
    _close_all((ref[0],) + tuple(t.grad for t in ts), ref)
    # a non-contiguous x: every second token of a longer sequence
    wide = torch.zeros(2, 130, 128)
    wide[:, ::2] = x
    wl = wide.to(dev).requires_grad_()
    ts = leaves()
    xv = wl[:, ::2]
    assert not xv.is_contiguous()
    y = seam.fused_mlp_func_grad(xv, ts[1], ts[3], ts[2], ts[4])
    _close("y", y.detach(), ref[0])
    y.backward(dy.to(dev))
    _close("dx", wl.grad[:, ::2], ref[1])
    assert not wl.grad[:, 1::2].any()
    _close_all((ref[0], ref[1]) + tuple(t.grad for t in ts[1:]), ref)


# ------------------------------------------------------------------------------------------------------------------ 8. the module graph as the reference builds it
class FFN(nn.Module):
    """The reference's FFN restated (basic_var.py:33-52); the module-level slot is captured at construction."""
    def __init__(self, slot, in_features, hidden_features):
        super().__init__()
        self.fused_mlp_func = slot
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = nn.GELU(approximate='tanh')
        self.fc2 = nn.Linear(hidden_features, in_features)
        self.drop = nn.Identity()

    def forward(self, x):
        if self.fused_mlp_func is not None:
            return self.drop(self.fused_mlp_func(x=x, weight1=self.fc1.weight, weight2=self.fc2.weight, bias1=self.fc1.bias, bias2=self.fc2.bias, activation='gelu_approx',
                                                 save_pre_act=self.training, return_residual=False, checkpoint_lvl=0, heuristic=0, process_group=None))
        return self.drop(self.fc2(self.act(self.fc1(x))))


def test_module_graph_and_training_steps(dev, mode):
    """install_train(mod, model, ffn=True) on a restated FFN, called with the reference's keyword arguments inside x + ffn(x).mul(gamma2); two SGD-style steps with
    in-place weight updates: the second step's gradients belong to the UPDATED weights (cached planes replaced) and the cache does not grow."""
    import types
    Cin, hid, _ = DIMS
    x, W1, b1, W2, b2, dy = _inputs(100, (2, 65, 128), DIMS)
    gamma2 = rnd(300, (2, 1, Cin))
    mod = types.SimpleNamespace(fused_mlp_func=None, slow_attn=None)
    model = nn.Sequential(FFN(None, Cin, hid))
    seam.install_train(mod, model, ffn=True)
    ffn = model[0]
    assert ffn.fused_mlp_func is seam.fused_mlp_func_grad and mod.fused_mlp_func is seam.fused_mlp_func_grad
    with torch.no_grad():
        for p, v in zip((ffn.fc1.weight, ffn.fc1.bias, ffn.fc2.weight, ffn.fc2.bias), (W1, b1, W2, b2)):
            p.copy_(v)
    twin = FFN(None, Cin, hid).double()                      # the fp64 reference: the reference's own torch branch
    twin.load_state_dict({k: v.double() for k, v in ffn.state_dict().items()})
    model.to(dev).train()
    seam.clear_caches()
    sizes = []
    for step in range(2):
        xd = x.to(dev).requires_grad_()
        loss = ((xd + ffn(xd).mul(gamma2.to(dev))) * dy.to(dev)).sum()
        model.zero_grad()
        loss.backward()
        x64 = x.double().requires_grad_()
        twin.zero_grad()
        ((x64 + twin(x64).mul(gamma2.double())) * dy.double()).sum().backward()
        print(f"step {step}")
        _close("dx", xd.grad, x64.grad)
        for (name, p), q in zip(ffn.named_parameters(), twin.parameters()):
            _close(name, p.grad, q.grad)
        sizes.append(len(seam._WEIGHT_PLANES))
        with torch.no_grad():
            for p, q in zip(ffn.parameters(), twin.parameters()):
                p.add_(p.grad, alpha=-0.05)                  # in place: same storage, _version bumped
                q.copy_(p.detach().cpu().double())
    print("cache entries after each step:", sizes)
    assert sizes[1] == sizes[0] and sizes[0] <= 4


# ------------------------------------------------------------------------------------------------------------------ 9. the kernels alone
FMT = {"f32": 0, "f16x2": 2, "bf16x3": 3}
NPL = {"f32": 1, "f16x2": 2, "bf16x3": 3}
GUARD, SENT = 256, 0x5A5A


def _unblock(plane, R, Kp):
    """K-blocked (R x Kp) plane -> row-major."""
    return plane.view(Kp // 32, R, 32).permute(1, 0, 2).reshape(R, Kp)


def _operand_value(buf, fmt_name, R, Kp):
    """The (R x Kp) fp64 matrix an operand buffer of NPL planes encodes (planes recombined on the host)."""
    if fmt_name == "f32":
        return buf.view(R, Kp).double()
    if fmt_name == "f16x2":
        return sum(_unblock(buf[p].view(torch.float16), R, Kp).double() for p in range(2))
    return sum(_unblock((buf[p].to(torch.int32) << 16).view(torch.float32), R, Kp).double() for p in range(3))


def _guarded(npl, n, dtype, dev):
    """An operand buffer of npl * n elements between two sentinel regions."""
    whole = torch.full((2 * GUARD + npl * n,), SENT if dtype == torch.int16 else float(SENT), dtype=dtype, device=dev)
    whole[GUARD:-GUARD] = float("nan") if dtype == torch.float32 else 0x7E7E          # a producer must write every element of its operand, the zero tail included
    return whole, whole[GUARD:GUARD + npl * n].view(npl, n)


def _guards_intact(whole):
    s = whole[0].item()
    return bool((whole[:GUARD] == s).all() and (whole[-GUARD:] == s).all())


@pytest.mark.parametrize("fmt_name", ["f32", "f16x2", "bf16x3"])
@pytest.mark.parametrize("rows,cols", [(1, 32), (33, 96), (130, 128)])
def test_transpose_operand(dev, fmt_name, rows, cols):
    """x^T as a GEMM operand in the three formats, from an input with a leading dimension: planes recombined on the host equal x^T exactly (fp32, bf16x3: standard-normal
    values, no plane anywhere near the subnormal range) or to 2^-22 |x| + 2^-25 (f16x2: the format's stated precision above / below |x| = 2^-3); the
    padded tail is exactly zero in every plane; sentinels around the buffer are intact."""
    lib, st = E.load_library(), E._stream()
    Kp = (rows + 31) // 32 * 32
    wide = rnd(400 + rows, (rows, cols + 8))
    xd = wide.to(dev)[:, :cols]
    x = wide[:, :cols].double()
    scales = [None] + ([torch.tensor([8.0, 0.125, 0.0, 0.0], device=dev)] if fmt_name == "f16x2" else [])
    for sc in scales:
        whole, buf = _guarded(NPL[fmt_name], cols * Kp, torch.float32 if fmt_name == "f32" else torch.int16, dev)
        E._check(lib.sdvar_op_transpose_operand(_p(xd), xd.stride(0), rows, cols, FMT[fmt_name], _p(buf), cols * Kp, _p(sc), st))
        assert _guards_intact(whole)
        got = _operand_value(buf.cpu(), fmt_name, cols, Kp)
        want = x.T * (1.0 if sc is None else 8.0)
        err = (got[:, :rows] - want).abs()
        if fmt_name == "f16x2":
            assert (err <= 2.0 ** -22 * want.abs() + 2.0 ** -25).all(), err.max().item()
        else:
            assert torch.equal(got[:, :rows], want)
        for p in range(NPL[fmt_name]):                       # the zero tail, plane by plane (bit patterns)
            plane = buf[p].cpu()
            tail = (plane.view(cols, Kp) if fmt_name == "f32" else _unblock(plane, cols, Kp))[:, rows:]
            assert not tail.any() and tail.numel() == cols * (Kp - rows)
        print(f"{fmt_name} ({rows}, {cols}) scale {None if sc is None else 8}: max err {err.max().item():.3e}, tail of {Kp - rows} zero")


@pytest.mark.parametrize("M,N,ld", [(1, 32, 32), (33, 96, 104), (130, 128, 128), (680, 36, 40)])
def test_colsum(dev, M, N, ld):
    """Column sums against fp64: the kernel accumulates in double in a fixed order, so what remains is the final rounding to fp32 (2^-24 |sum|) plus double
    rounding noise (far below 2^-40 sum|x|); two runs are bit-identical."""
    lib, st = E.load_library(), E._stream()
    wide = rnd(500 + M, (M, ld))
    xd = wide.to(dev)[:, :N]
    whole, out = _guarded(1, N, torch.float32, dev)
    E._check(lib.sdvar_op_colsum(_p(xd), ld, M, N, _p(out), st))
    first = out.clone()
    E._check(lib.sdvar_op_colsum(_p(xd), ld, M, N, _p(out), st))
    assert torch.equal(first, out) and _guards_intact(whole)
    x = wide[:, :N].double()
    ref = x.sum(0)
    err = (out[0].cpu().double() - ref).abs()
    print(f"colsum ({M}, {N}): max err {err.max().item():.3e}")
    assert (err <= 2.0 ** -24 * ref.abs() * 1.001 + 2.0 ** -40 * x.abs().sum(0)).all()


@pytest.mark.parametrize("kind", [0, 1])
def test_gelu_bwd_producer(dev, kind):
    """dpre = dh * gelu_tanh'(pre) against fp64 autograd of F.gelu(approximate='tanh'), with pre = +-1e4, +-0, +-40 next to ordinary values.  Bar per element:
    4e-6 |dh| - gelu' is O(1) (|gelu'| <= 1.13) and is evaluated in about ten fp32 operations of at most 1 ulp (6e-8) each, the argument error of the exponential entering
    through s (1 - s) |2u| <= 0.3; 4e-6 is 64 ulp.  pre = +-0 gives dh / 2 within the same bar.  Also: h^T has the bits of the forward's GELU (sdvar_op_gelu_operand), dpre^T is dpre transposed with a zero tail,
    the 32-row column sums add up to db1, everything is finite."""
    lib, st = E.load_library(), E._stream()
    M, N = 33, 64
    Mp = 64
    pre = rnd(600, (M, N)) * 3
    pre[0, :8] = torch.tensor([1e4, -1e4, 0.0, -0.0, 40.0, -40.0, 12.0, -12.0])
    pre[32, -4:] = torch.tensor([1e4, -1e4, 40.0, -40.0])
    dh = rnd(601, (M, N))
    p64 = pre.double().requires_grad_()
    F.gelu(p64, approximate="tanh").backward(dh.double())
    ref = p64.grad
    assert torch.isfinite(ref).all()
    pd, dd = pre.to(dev), dh.to(dev)
    w_dpre, dpre = _guarded(1, M * N, torch.float32, dev)
    w_dt, dpre_t = _guarded(1, N * Mp, torch.float32, dev)
    w_ht, h_t = _guarded(1, N * Mp, torch.float32, dev)
    w_part, part = _guarded(1, (Mp // 32) * N, torch.float32, dev)
    E._check(lib.sdvar_op_gelu_bwd(_p(dd), _p(pd), M, N, 0, kind, None, _p(dpre), 0, _p(dpre_t), 0, _p(h_t), 0, _p(part), st))
    assert all(_guards_intact(w) for w in (w_dpre, w_dt, w_ht, w_part))
    got = dpre.view(M, N).cpu()
    assert torch.isfinite(got).all()
    err = (got.double() - ref).abs()
    print(f"kind {kind}: dpre max err {err.max().item():.3e}, max err / |dh| {(err / dh.abs().double().clamp_min(1e-30)).max().item():.3e}")
    assert (err <= 4e-6 * dh.abs().double()).all()
    assert got[0, 0] == dh[0, 0] and got[0, 1] == 0 and got[0, 4] == dh[0, 4] and got[0, 5] == 0           # gelu' is exactly 1 / 0 far out
    t = dpre_t.view(N, Mp).cpu()
    assert torch.equal(t[:, :M], got.T) and not t[:, M:].any()
    h = torch.empty(M, N, device=dev)
    E._check(lib.sdvar_op_gelu_operand(_p(pd), M, N, 0, kind, _p(h), 0, st))
    ht = h_t.view(N, Mp).cpu()
    assert torch.equal(ht[:, :M], h.cpu().T) and not ht[:, M:].any()
    db1 = torch.empty(N, device=dev)
    E._check(lib.sdvar_op_colsum(_p(part), N, Mp // 32, N, _p(db1), st))
    e1 = (db1.cpu().double() - got.double().sum(0)).abs()           # the summation alone: 33 fp32 additions of at most 2^-24 relative each, then double
    print(f"kind {kind}: db1 from the partial sums against the fp64 sum of dpre, max err {e1.max().item():.3e}")
    assert (e1 <= 40 * 2.0 ** -24 * got.abs().double().sum(0)).all()
    # only h^T (the weight2-only backward): no dh
    w_h2, h2 = _guarded(1, N * Mp, torch.float32, dev)
    E._check(lib.sdvar_op_gelu_bwd(None, _p(pd), M, N, 0, kind, None, None, 0, None, 0, _p(h2), 0, None, st))
    assert torch.equal(h2, h_t) and _guards_intact(w_h2)
