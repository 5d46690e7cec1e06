"""seam.qk_l2norm / install_qknorm / install_train(qknorm=True) (csrc/qknorm_train.hip) against torch in fp64 on the CPU, every element asserted.  Inputs, references and
the derivation of every bound: qknorm_cases.py.  The bounds come from the kernels' operation counts, and torch's float32 autograd on the CPU is asserted to meet them on
the same inputs (here and in test_seam_qknorm_host.py).

The stand-in model (two blocks of adaLN, an attention with attn_l2_norm=True written here in plain torch, and an FFN; C = 256, H = 4, B = 3, L = 14, a block-causal
mask) is compared per tensor with its own fp64 run on the CPU under the norm-wise rule of test_gpu_seam_adaln.py, err <= K u_p max|ref| per tensor.  float32
(u_p = 2^-24): a gradient element is a sum of up to N = B L C = 10752 products that each passed through the k ~ 40 rounded operations of that file's graph plus 12 more
here (per block: the bias add, the squares and their sum, the root, the division, the scale of q); with terms of random sign sum|t| ~ sqrt(N) |sum t|, so the worst case
is k sqrt(N) = 52 x 104 = 5400 roundings against the largest element: K = 8192, the next power of two.  autocast (u_p = 2^-11): k = 10 half roundings per product (that
graph's 8, plus q and k rounded to half by the attention) add in quadrature, sqrt(10) x 4 = 13 roundings against a typical element, times that file's margin of 6:
K = 80.  The forward alone (the KV-caching test): an output element is a sum of C = 256 products through 26 operations per block, 52 sqrt(256) = 832: K = 1024.
The uninstalled torch model on the GPU is held to the same bounds, so a bound that torch itself misses shows.  Bounds this loose check the WIRING only; the precision
of the operator rests on the element-wise tests above."""
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import qknorm_cases as QC
from sdvar_amd import engine as E
from sdvar_amd import seam
from sdvar_amd.seam import install_qknorm, qk_l2norm, uninstall_qknorm          # noqa: F401  (the feature under test: without it nothing here runs)

pytestmark = pytest.mark.gpu
IDS = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}
NAMES = ("dqkv", "dscale_log", "dq_bias", "dv_bias")


@pytest.fixture(autouse=True)
def _grad_mode():
    """Other test modules switch grad mode off for the process; these tests are about autograd."""
    with torch.enable_grad():
        yield


def _dev(c, dev):
    return tuple(None if t is None else t.to(dev) for t in c["in"])


def _blhc(layout, *ts):
    return tuple(t if layout == "BLHc" else t.permute(0, 2, 1, 3) for t in ts)


def _assert_all(name, got, ref, tol, dtype=torch.float32):
    assert QC.worst(name, got, ref, tol, dtype) <= 1.0, name


@pytest.mark.parametrize("dtype", QC.DTYPES, ids=IDS.values())
@pytest.mark.parametrize("H,B,L", QC.SHAPES)
def test_forward(dev, H, B, L, dtype):
    print(f"\nqk_l2norm forward H={H} B={B} L={L} {dtype}")
    for bias in (True, False):
        c = QC.full(H, B, L, dtype, bias)
        qkv, qb, vb, sl = _dev(c, dev)
        outs = {}
        for layout in ("BHLc", "BLHc"):
            q, k, v = seam.qk_l2norm(qkv, sl, QC.MAX_LOG, qb, vb, layout)
            assert q.shape == k.shape == v.shape == ((B, H, L, 64) if layout == "BHLc" else (B, L, H, 64))
            q, k, v = _blhc(layout, q, k, v)
            assert q.dtype == k.dtype == torch.float32 and v.dtype == dtype and q.is_contiguous() and k.is_contiguous()
            outs[layout] = (q, k, v)
        assert all(torch.equal(a, b) for a, b in zip(outs["BHLc"], outs["BLHc"]))          # the layout chooses a view, nothing else
        q, k, v = outs["BLHc"]
        for name, t in zip(("q", "k", "v"), (q, k, v)):
            _assert_all(f"{name} bias={bias}", t, c["ref"][name], c["tol"][name], dtype if name == "v" else torch.float32)
        if bias:
            assert v.is_contiguous() and v.data_ptr() != qkv[:, :, 2].data_ptr()
        else:
            assert v.data_ptr() == qkv[:, :, 2].data_ptr() and v.stride() == qkv[:, :, 2].stride()          # the reference's view: not written, not copied
        for slot, t in ((0, q), (1, k)):
            zero = torch.tensor([[f == "zero" for f in row] for row in QC.families(H, B, L, slot)]).view(B, L, H)
            if slot == 1 or not bias:
                assert float(t[zero.to(dev)].abs().sum()) == 0.0, "a zero head must give exact zeros"
        again = _blhc("BHLc", *seam.qk_l2norm(qkv, sl, QC.MAX_LOG, qb, vb))
        with_grad = _blhc("BHLc", *seam.qk_l2norm(qkv.clone().requires_grad_(True), sl, QC.MAX_LOG, qb, vb))
        with torch.no_grad():
            no_grad = _blhc("BHLc", *seam.qk_l2norm(qkv.clone().requires_grad_(True), sl.clone().requires_grad_(True), QC.MAX_LOG, qb, vb))
        assert with_grad[0].requires_grad and not no_grad[0].requires_grad
        for other in (again, with_grad, no_grad):          # repeats, the grad call and the no_grad call: the same bits
            assert all(torch.equal(a.detach(), b) for a, b in zip(other, (q, k, v)))


def _run_bwd(inputs, grads, layout="BHLc", need=(True, True, True, True), use=(True, True, True)):
    """Gradients of (qkv, scale_log, q_bias, v_bias) - None where not needed or the bias is absent - for the outputs of `use` with the upstream gradients `grads`
    ((B, L, H, 64) tensors, handed over in the layout's dim order)."""
    qkv, qb, vb, sl = inputs
    leaves = [None if t is None else t.detach().clone().requires_grad_(n) for t, n in zip((qkv, sl, qb, vb), need)]
    outs = seam.qk_l2norm(leaves[0], leaves[1], QC.MAX_LOG, leaves[2], leaves[3], layout)
    pick = [(o, g if layout == "BLHc" else g.permute(0, 2, 1, 3)) for o, g, u in zip(outs, grads, use) if u]
    ins = [t for t in leaves if t is not None and t.requires_grad]
    got = list(torch.autograd.grad([o for o, _ in pick], ins, [g for _, g in pick]))
    return [got.pop(0) if t is not None and t.requires_grad else None for t in leaves]


@pytest.mark.parametrize("dtype", QC.DTYPES, ids=IDS.values())
@pytest.mark.parametrize("H,B,L", QC.SHAPES)
def test_backward(dev, H, B, L, dtype):
    print(f"\nqk_l2norm backward H={H} B={B} L={L} {dtype}")
    for bias, layout in ((True, "BHLc"), (False, "BLHc")):
        c = QC.full(H, B, L, dtype, bias)
        QC.assert_torch32_meets_the_bounds(c, f"bias={bias}")
        inputs, g = _dev(c, dev), tuple(t.to(dev) for t in c["g"])
        got, again = _run_bwd(inputs, g, layout), _run_bwd(inputs, g, layout)
        for name, a, b in zip(NAMES, got, again):
            r = c["ref"][name]
            if r is None:
                assert a is None
                continue
            assert a.dtype == (dtype if name == "dqkv" else torch.float32) and a.shape == r.shape and a.is_contiguous(), name
            assert torch.equal(a, b), f"{name}: two runs must be bit-identical"
            _assert_all(f"{name} bias={bias}", a, r, c["tol"][name], dtype if name == "dqkv" else torch.float32)
        sl = c["in"][3]
        ds = got[1].cpu()
        assert float(ds[sl > QC.MAX_LOG].abs().sum()) == 0.0, "a head above max_log: dscale_log exactly 0"
        assert (ds[sl == QC.MAX_LOG] != 0).all(), "a head at max_log: the gradient passes"
        if B * L >= 3:
            assert float(got[0].view(B * L, -1)[B * L // 2].float().abs().sum()) == 0.0, "the zero row of the upstream gradients: exact zeros"


@pytest.mark.parametrize("dtype", (torch.float32, torch.float16), ids=("fp32", "fp16"))
def test_partial_needs(dev, dtype):
    """Only the gradients autograd asks for: each alone has the bits it has in the full run; without an upstream gradient of v the v slot of dqkv is exactly zero."""
    H, B, L = 30, 3, 41
    c = QC.full(H, B, L, dtype, True)
    inputs, g = _dev(c, dev), tuple(t.to(dev) for t in c["g"])
    fullrun = _run_bwd(inputs, g)
    for i in range(4):
        alone = _run_bwd(inputs, g, need=tuple(j == i for j in range(4)))
        assert all((a is None) == (j != i) for j, a in enumerate(alone))
        assert torch.equal(alone[i], fullrun[i]), NAMES[i]
    for use in ((True, True, False), (True, False, False), (False, True, True), (False, False, True)):
        part = _run_bwd(inputs, g, use=use)
        for slot in range(3):
            if use[slot]:
                assert torch.equal(part[0][:, :, slot], fullrun[0][:, :, slot])
            else:
                assert float(part[0][:, :, slot].float().abs().sum()) == 0.0, "an absent upstream gradient: an exactly zero slot"
        assert torch.equal(part[3], fullrun[3]) if use[2] else float(part[3].abs().sum()) == 0.0
        if use[0]:
            assert torch.equal(part[1], fullrun[1]) and torch.equal(part[2], fullrun[2])


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("fp32", "bf16"))
def test_strided_upstream_gradients(dev, dtype):
    """permute(0, 2, 1, 3) views of (B, L, H, 64) buffers - what the seam's attention backward returns for (B, H, L, 64) operands - are read in place; a gradient that
    breaks the stride rule gives the same values through one copy."""
    H, B, L = 3, 3, 41
    c = QC.full(H, B, L, dtype, True)
    inputs, g = _dev(c, dev), tuple(t.to(dev) for t in c["g"])
    base = _run_bwd(inputs, g, "BLHc")          # dense (B, L, H, 64) gradients
    views = tuple(t.permute(0, 2, 1, 3) for t in g)          # (B, H, L, 64) with the buffers' strides: what _run_bwd hands to autograd for BHLc
    assert all(not v.is_contiguous() and E.qknorm_grad_in_place(v) for v in views)
    for a, b in zip(_run_bwd(inputs, g, "BHLc"), base):
        assert torch.equal(a, b)
    other = tuple(v.contiguous().permute(0, 2, 1, 3) for v in views)          # (B, L, H, 64) over (B, H, L, 64) memory: the other stride order
    assert all(not t.is_contiguous() and E.qknorm_grad_in_place(t) for t in other)
    direct = E.qknorm_bwd(inputs[0], inputs[3], QC.MAX_LOG, inputs[1], *other)          # the engine never copies: read through their strides
    assert all(torch.equal(a, b) for a, b in zip(direct, base))
    bad = []
    for t in g:          # rows of 66 elements, starting one element in: misaligned, and strides that are no multiples of 4
        wide = torch.zeros(B, L, H, 66, dtype=t.dtype, device=dev)
        wide[..., 1:65] = t
        bad.append(wide[..., 1:65])
    assert all(not E.qknorm_grad_in_place(t) for t in bad)
    with pytest.raises(E.SdvarError, match="dq with strides .* breaks the stride rule"):
        E.qknorm_bwd(inputs[0], inputs[3], QC.MAX_LOG, inputs[1], *bad)
    for layout in ("BLHc", "BHLc"):
        for a, b in zip(_run_bwd(inputs, tuple(bad), layout), base):
            assert torch.equal(a, b)
    ql = inputs[0].clone().requires_grad_(True)
    q, k, v = seam.qk_l2norm(ql, inputs[3], QC.MAX_LOG, inputs[1], inputs[2])
    (gx,) = torch.autograd.grad(q.sum() + k.sum() + v.float().sum(), ql)          # stride-0 expansions of a scalar: no unit last stride, copied once
    ones = tuple(torch.ones(B, L, H, 64, dtype=t.dtype, device=dev) for t in g)
    assert torch.equal(gx, _run_bwd(inputs, ones)[0])


def test_misaligned_qkv_is_copied_once_and_errors_are_documented(dev):
    H, B, L = 3, 2, 5
    c = QC.full(H, B, L, torch.float32, True)
    qkv, qb, vb, sl = _dev(c, dev)
    flat = torch.zeros(qkv.numel() + 1, device=dev)
    flat[1:] = qkv.flatten()
    off = flat[1:].view(qkv.shape)          # dense, 4 bytes off the 16-byte grid
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    with pytest.raises(E.SdvarError, match="not dense and 16-byte aligned"):
        E.qknorm_fwd(off, sl, QC.MAX_LOG, qb, vb)
    for a, b in zip(seam.qk_l2norm(off, sl, QC.MAX_LOG, qb, vb), seam.qk_l2norm(qkv, sl, QC.MAX_LOG, qb, vb)):
        assert torch.equal(a, b)
    g = tuple(t.to(dev) for t in c["g"])
    for a, b in zip(_run_bwd((off, qb, vb, sl), g), _run_bwd((qkv, qb, vb, sl), g)):
        assert torch.equal(a, b)
    cases = [
        (lambda: seam.qk_l2norm(qkv, sl.cpu(), QC.MAX_LOG), r"scale_log is on cpu"),
        (lambda: seam.qk_l2norm(qkv, sl[:2], QC.MAX_LOG), r"scale_log is .* of shape \(2,\)"),
        (lambda: seam.qk_l2norm(qkv, sl, QC.MAX_LOG, qb.half()), r"q_bias is torch.float16"),
        (lambda: seam.qk_l2norm(qkv, sl, QC.MAX_LOG, qb, vb[:64]), r"v_bias is .* of shape \(64,\)"),
        (lambda: seam.qk_l2norm(qkv, sl, QC.MAX_LOG, layout="HBLc"), r"layout 'HBLc'"),
    ]
    for fn, words in cases:
        with pytest.raises(E.SdvarError, match=words):
            fn()
    ql = qkv.clone().requires_grad_(True)
    q, k, v = seam.qk_l2norm(ql, sl, QC.MAX_LOG, qb, vb)
    with pytest.raises(E.SdvarError, match="double backward.*without create_graph"):
        torch.autograd.grad(q.sum(), ql, create_graph=True)


# ------------------------------------------------------------------------------------------------------------------ the stand-in model
# the operator slots of this module, read by _SelfAttn.forward at call time as the reference's attention reads its module's
def _torch_attn(query, key, value, scale, attn_mask=None, dropout_p=0.0):
    return F.scaled_dot_product_attention(query, key, value, attn_mask=attn_mask, dropout_p=dropout_p, scale=scale)


slow_attn = _torch_attn
flash_attn_func = memory_efficient_attention = fused_mlp_func = None


class _SelfAttn(nn.Module):
    """An attention with per-head L2-normalised q and k and a learnt, clamped per-head scale of q, with the attributes a SelfAttention-like module carries."""

    def __init__(self, Cc, H):
        super().__init__()
        self.num_heads, self.head_dim, self.attn_l2_norm, self.scale = H, Cc // H, True, 1
        self.scale_mul_1H11 = nn.Parameter(torch.full((1, H, 1, 1), 4.0).log() + 0.25 * torch.randn(1, H, 1, 1))
        self.max_scale_mul = QC.MAX_LOG
        self.mat_qkv = nn.Linear(Cc, 3 * Cc, bias=False)
        self.q_bias, self.v_bias = nn.Parameter(0.5 * torch.randn(Cc)), nn.Parameter(0.5 * torch.randn(Cc))
        self.register_buffer("zero_k_bias", torch.zeros(Cc))
        self.proj, self.proj_drop, self.attn_drop = nn.Linear(Cc, Cc), nn.Identity(), 0.0
        self.using_flash = self.using_xform = False
        self.caching, self.cached_k, self.cached_v = False, None, None

    def forward(self, x, attn_bias):
        B, L, Cc = x.shape
        qkv = F.linear(x, self.mat_qkv.weight, torch.cat((self.q_bias, self.zero_k_bias, self.v_bias))).view(B, L, 3, self.num_heads, self.head_dim)
        kind = qkv.dtype
        flash = self.using_flash and attn_bias is None and kind != torch.float32
        q, k, v = qkv.unbind(2) if flash else qkv.permute(2, 0, 3, 1, 4).unbind(0)
        s = self.scale_mul_1H11.clamp_max(self.max_scale_mul).exp()
        q, k = F.normalize(q, dim=-1).mul(s.transpose(1, 2) if flash else s), F.normalize(k, dim=-1)
        if self.caching:
            if self.cached_k is None:
                self.cached_k, self.cached_v = k, v
            else:
                k = self.cached_k = torch.cat((self.cached_k, k), dim=1 if flash else 2)
                v = self.cached_v = torch.cat((self.cached_v, v), dim=1 if flash else 2)
        if flash:
            o = flash_attn_func(q.to(kind), k.to(kind), v.to(kind), dropout_p=0.0, softmax_scale=self.scale).view(B, L, Cc)
        else:
            o = slow_attn(query=q, key=k, value=v, scale=self.scale, attn_mask=attn_bias, dropout_p=0.0).transpose(1, 2).reshape(B, L, Cc)
        return self.proj_drop(self.proj(o))


class _FFN(nn.Module):
    def __init__(self, Cc):
        super().__init__()
        self.fused_mlp_func = None
        self.fc1, self.act, self.fc2 = nn.Linear(Cc, 4 * Cc), nn.GELU(approximate="tanh"), nn.Linear(4 * Cc, Cc)

    def forward(self, x):
        if self.fused_mlp_func is not None:
            return self.fused_mlp_func(x=x, weight1=self.fc1.weight, weight2=self.fc2.weight, bias1=self.fc1.bias, bias2=self.fc2.bias, activation="gelu_approx",
                                       save_pre_act=self.training, return_residual=False, checkpoint_lvl=0, heuristic=0, process_group=None)
        return self.fc2(self.act(self.fc1(x)))


class _Block(nn.Module):
    def __init__(self, Cc, H):
        super().__init__()
        self.C, self.drop_path = Cc, nn.Identity()
        self.attn, self.ffn, self.ln_wo_grad = _SelfAttn(Cc, H), _FFN(Cc), nn.LayerNorm(Cc, eps=1e-6, elementwise_affine=False)
        self.ada_lin = nn.Sequential(nn.SiLU(inplace=False), nn.Linear(Cc, 6 * Cc))

    def forward(self, x, cond_BD, attn_bias):
        gamma1, gamma2, scale1, scale2, shift1, shift2 = self.ada_lin(cond_BD).view(-1, 1, 6, self.C).unbind(2)
        x = x + self.attn(self.ln_wo_grad(x).mul(scale1.add(1)).add_(shift1), attn_bias=attn_bias).mul_(gamma1)
        return x + self.ffn(self.ln_wo_grad(x).mul(scale2.add(1)).add_(shift2)).mul(gamma2)


class _Model(nn.Module):
    def __init__(self, Cc=256, H=4):
        super().__init__()
        self.blocks = nn.ModuleList([_Block(Cc, H), _Block(Cc, H)])

    def forward(self, x, cond, attn_bias=None):
        for b in self.blocks:
            x = b(x, cond, attn_bias)
        return x


@pytest.fixture
def slots():
    """This module as the `module` argument of the installers, with its slots put back afterwards."""
    me = sys.modules[__name__]
    saved = {n: getattr(me, n) for n in ("slow_attn", "flash_attn_func", "memory_efficient_attention", "fused_mlp_func")}
    yield me
    for n, v in saved.items():
        setattr(me, n, v)
    seam.configure(gemm_mode=E.DEFAULT_GEMM_MODE)
    seam.clear_caches()


def _model_and_inputs():
    torch.manual_seed(4321)
    m = _Model()
    x, cond, w = QC.rnd(1, (3, 14, 256)), QC.rnd(2, (3, 256)), QC.rnd(3, (3, 14, 256))
    stage = torch.tensor([0] + [1] * 4 + [2] * 9)          # block-causal: a token sees its own stage and the earlier ones
    mask = torch.where(stage.view(14, 1) >= stage.view(1, 14), 0.0, -torch.inf).view(1, 1, 14, 14)
    return m, x, cond, w, mask


def _loss_and_grads(m, x, cond, w, mask, autocast=None, scale=1.0):
    xl, cl = x.detach().clone().requires_grad_(True), cond.detach().clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=autocast or torch.float16, enabled=autocast is not None):
        out = m(xl, cl, mask)
    loss = (out.float() * w).mean() * scale          # the mean: with the GradScaler's 65536 the upstream gradient is 6 w, inside fp16's range as a trainer's is
    loss.backward()
    res = {"loss": loss.detach().clone(), "x": xl.grad, "cond": cl.grad}
    res.update({n: None if q.grad is None else q.grad.clone() for n, q in m.named_parameters()})
    return res


def _compare(tag, got, ref, K, up):
    print(f"\n{tag}")
    for n, r in ref.items():
        assert got[n] is not None, f"{n} received no gradient"
        assert torch.isfinite(got[n]).all(), n
        r = r.double()
        tol = torch.full_like(r, K * up * float(r.abs().max()))
        assert QC.worst(n, got[n], r, tol) <= 1.0, (tag, n)


def _unbound(m):
    return not any("forward" in q.__dict__ for q in m.modules())


@pytest.mark.parametrize("extra", [dict(), dict(adaln=True, ffn=True)], ids=["qknorm", "qknorm+adaln+ffn"])
def test_stand_in_model_against_fp64(dev, slots, extra):
    m, x, cond, w, mask = _model_and_inputs()
    ref = {k: v.clone() for k, v in _loss_and_grads(m.double(), x.double(), cond.double(), w.double(), mask.double()).items()}
    m = m.float().to(dev)
    args = tuple(t.to(dev) for t in (x, cond, w, mask))
    plain = _loss_and_grads(m, *args)
    seam.configure(gemm_mode="f32")          # the FFN's GEMMs in float32 arithmetic, as the bound assumes
    seam.install_train(slots, m, qknorm=True, **extra)
    assert slots.slow_attn is seam.slow_attn_grad and sum("forward" in q.__dict__ for q in m.modules()) == (4 if extra else 2)
    inst = _loss_and_grads(m, *args)
    K, up = 8192, 2.0 ** -24
    _compare("stand-in, torch on the GPU", plain, ref, K, up)
    _compare(f"stand-in, install_train(qknorm=True, {extra})", inst, ref, K, up)
    seam.uninstall_qknorm(m)
    seam.uninstall_adaln(m)
    assert _unbound(m)
    slots.slow_attn = _torch_attn
    for q in m.modules():
        if isinstance(q, _FFN):
            q.fused_mlp_func = None
    again = _loss_and_grads(m, *args)
    assert all(torch.equal(again[k], plain[k]) for k in plain), "uninstall_qknorm must restore the class forward"


@pytest.mark.parametrize("half", (torch.float16, torch.bfloat16), ids=("fp16", "bf16"))
def test_stand_in_model_under_autocast_with_a_grad_scaler_step(dev, slots, half):
    m, x, cond, w, mask = _model_and_inputs()
    scale = 65536.0
    ref = {k: v.clone() for k, v in _loss_and_grads(m.double(), x.double(), cond.double(), w.double(), mask.double(), scale=scale).items()}
    m = m.float().to(dev)
    args = tuple(t.to(dev) for t in (x, cond, w, mask))
    plain = _loss_and_grads(m, *args, autocast=half, scale=scale)
    seam.install_train_amp(slots, m, ffn="half", qknorm=True)
    assert slots.slow_attn is seam.slow_attn_amp_grad and m.blocks[0].ffn.fused_mlp_func is seam.fused_mlp_func_amp_grad and m.blocks[0].attn.using_flash
    inst = _loss_and_grads(m, *args, autocast=half, scale=scale)
    K, up = 80, 2.0 ** -11 if half == torch.float16 else 2.0 ** -8
    _compare(f"stand-in, torch on the GPU, autocast {half}", plain, ref, K, up)
    _compare(f"stand-in, install_train_amp(ffn='half', qknorm=True), autocast {half}", inst, ref, K, up)
    # one optimiser step through a GradScaler: finite gradients are unscaled and applied, the scale stays
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    scaler = torch.amp.GradScaler("cuda", init_scale=scale, growth_interval=1000)
    before = {n: q.detach().clone() for n, q in m.named_parameters()}
    opt.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=half):
        out = m(args[0], args[1], args[3])
    scaler.scale((out.float() * args[2]).mean()).backward()
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() == scale, "the GradScaler found an inf / NaN gradient"
    for n, q in m.named_parameters():
        assert torch.isfinite(q).all() and not torch.equal(q, before[n]), n
    seam.uninstall_qknorm(m)
    assert _unbound(m)


def test_kv_caching_inference_path(dev, slots):
    """install_qknorm alone, under no_grad, two calls with caching=True (5 tokens, then 9 more, no mask): the stand-in's own outputs within the forward bound."""
    m, x, cond, _, _ = _model_and_inputs()

    def two_calls(model, xs, c):
        for b in model.blocks:
            b.attn.caching, b.attn.cached_k, b.attn.cached_v = True, None, None
        with torch.no_grad():
            outs = [model(xs[:, :5], c, None), model(xs[:, 5:], c, None)]
        assert model.blocks[1].attn.cached_k.shape == (3, 4, 14, 64)
        return outs

    ref = two_calls(m.double(), x.double(), cond.double())
    m = m.float().to(dev)
    plain = two_calls(m, x.to(dev), cond.to(dev))
    slots.slow_attn = seam.slow_attn          # the inference slot; the FFN stays torch's
    seam.install_qknorm(m)
    assert slots.slow_attn is seam.slow_attn and sum("forward" in q.__dict__ for q in m.modules()) == 2
    inst = two_calls(m, x.to(dev), cond.to(dev))
    assert m.blocks[0].attn.cached_k.dtype == torch.float32 and m.blocks[0].attn.cached_k.is_contiguous()
    K, up = 1024, 2.0 ** -24
    for tag, got in (("torch on the GPU", plain), ("install_qknorm", inst)):
        print(f"\nKV caching, {tag}")
        for i, (a, r) in enumerate(zip(got, ref)):
            assert QC.worst(f"call {i}", a, r, torch.full_like(r, K * up * float(r.abs().max()))) <= 1.0, (tag, i)
    seam.uninstall_qknorm(m)
    assert _unbound(m)
