"""seam.adaln_modulate / seam.gated_residual / install_train(adaln=True) (csrc/adaln_train.hip) against torch in fp64 on the CPU, every element asserted.  Inputs,
references and the derivation of every bound: adaln_cases.py.  The backward bounds come from the kernels' operation counts, and torch's float32 autograd on the CPU is
asserted to meet them on the same inputs (here and in test_seam_adaln_host.py).

The stand-in model (two blocks - one with its own ada_lin, one with a shared ada_gss - and a head norm at C = 256, H = 4, B = 3, L = 14, plain torch attention and FFN)
is compared per tensor with its own fp64 run on the CPU.  Its bound is norm-wise, err <= K u_p max|ref| per tensor.  float32 (u_p = 2^-24): a gradient element is a sum of
up to N = B L C = 10752 products that each passed through k ~ 40 rounded operations (two blocks of LayerNorm, modulation, four GEMMs, softmax, GELU, the gated sums);
with terms of random sign sum|t| ~ sqrt(N) |sum t|, so the worst case is k sqrt(N) ~ 4100 roundings against the largest element: K = 4096.  autocast(float16)
(u_p = 2^-11): the worst case of that count is no check at all (k = 8 half roundings per product give 8 sqrt(N) u_p = 0.4), so the bound is the random-walk one
with a stated margin: independent roundings add in quadrature, sqrt(k) u_p max|t| / rms(t) ~ sqrt(8) x 4 = 11 roundings against a typical element, times a margin
of 6: K = 64, 3 % of the tensor's largest element.  The uninstalled torch model on the GPU is held to the same bounds, so a bound that torch itself misses shows.
Bounds this loose check the WIRING only - that the bound forward computes the block the class computes, with every gradient reaching its parameter, the same images
dropped and the class forward restored - and catch gross errors; the precision of the operators rests on the element-wise tests above, not on this one."""
import pytest
import torch
import torch.nn as nn

import adaln_cases as AC
from sdvar_amd import engine as E
from sdvar_amd import seam

pytestmark = pytest.mark.gpu
HALVES = (torch.float16, torch.bfloat16)


@pytest.fixture(autouse=True)
def _grad_mode():
    """Other test modules switch grad mode off for the process; these tests are about autograd."""
    with torch.enable_grad():
        yield


def _views(mod, dev, one_row=False, dtype=None):
    """(gamma, scale, shift) as unbind(2) views of the (B, 1, 6, C) buffer on the device: batch stride 6 C, read in place."""
    m = mod.to(dev) if dtype is None else mod.to(dev, dtype)
    if one_row:
        m = m[:1]
    g, _, s, _, h, _ = m.unbind(2)
    return g, s, h


def _assert_all(name, got, ref, tol):
    assert AC.worst(name, got, ref, tol) <= 1.0, name


@pytest.mark.parametrize("Cc,B,L", AC.SHAPES)
def test_modulate_forward(dev, Cc, B, L):
    x, mod, fam, grp = AC.case(Cc, B, L)
    _, scale, shift = _views(mod, dev)
    assert scale.stride() == (6 * Cc, 6 * Cc, 1) and E.train_vec_in_place(scale)
    xd = x.to(dev)
    h = seam.adaln_modulate(xd, scale, shift)
    ref, tol = AC.fwd_ref(x, mod[:, :, 2], mod[:, :, 4])
    print(f"\nadaln_modulate forward C={Cc} B={B} L={L}")
    _assert_all("h", h, ref, tol)
    ex = AC.exact_rows(fam, grp, B, L)
    assert torch.equal(h.cpu()[ex], mod[:, :, 4].expand(B, L, Cc)[ex]), "constant / zero rows and scale == -1 must give shift bit for bit"
    assert torch.equal(h, seam.adaln_modulate(xd, scale, shift))
    hg = seam.adaln_modulate(xd.clone().requires_grad_(True), scale, shift)
    assert hg.requires_grad and torch.equal(hg.detach(), h)          # the grad call and the no-grad call: the same forward bits
    with torch.no_grad():
        assert torch.equal(seam.adaln_modulate(xd.clone().requires_grad_(True), scale, shift), h)


@pytest.mark.parametrize("layout", ["one_row", "BC"])
def test_modulate_forward_other_layouts(dev, layout):
    Cc, B, L = 260, 3, 41
    x, mod, _, _ = AC.case(Cc, B, L)
    if layout == "one_row":
        sc, sh = mod[:1, :, 2], mod[:1, :, 4]
    else:
        sc, sh = mod[:, 0, 2], mod[:, 0, 4]
        assert sc.shape == (B, Cc)
    h = seam.adaln_modulate(x.to(dev), sc.to(dev), sh.to(dev))
    print(f"\nadaln_modulate forward, layout {layout}")
    _assert_all("h", h, *AC.fwd_ref(x, sc, sh))


def _run_bwd(dev, x, scale, shift, g):
    xl, sl, hl = (t.detach().requires_grad_(True) for t in (x, scale, shift))          # leaves that ARE the views: strides and addresses as given
    h = seam.adaln_modulate(xl, sl, hl)
    return (h.detach(),) + torch.autograd.grad(h, (xl, sl, hl), g)


@pytest.mark.parametrize("Cc,B,L,one_row", AC.BWD_CASES)
def test_modulate_backward(dev, Cc, B, L, one_row):
    x, mod, _, _ = AC.case(Cc, B, L)
    g = AC.upstream(Cc, B, L)
    sc, sh = (mod[:1, :, 2], mod[:1, :, 4]) if one_row else (mod[:, :, 2], mod[:, :, 4])
    ref = AC.bwd_ref(x, sc, sh, g)
    tols = AC.bwd_bounds(x, sc, sh, g, ref[1:])
    t32 = AC.bwd_torch32(x, sc, sh, g)
    _, scale, shift = _views(mod, dev, one_row)
    got = _run_bwd(dev, x.to(dev), scale, shift, g.to(dev))
    again = _run_bwd(dev, x.to(dev), scale, shift, g.to(dev))
    print(f"\nadaln_modulate backward C={Cc} B={B} L={L} one_row={one_row}")
    for name, a, b, t, r, tol in zip(("dx", "dscale", "dshift"), got[1:], again[1:], t32[1:], ref[1:], tols):
        assert a.dtype == torch.float32 and a.shape == r.shape and torch.equal(a, b), name
        assert AC.worst(name + " torch float32 CPU", t, r, tol) <= 1.0          # the bound is honest
        _assert_all(name, a, r, tol)
    assert float(got[1].reshape(B * L, Cc)[B * L // 2].abs().max()) == 0.0 or B * L < 3          # the zero row of g: dx exactly 0


def test_modulate_backward_partial_needs(dev):
    """Only the gradients autograd asks for: each alone has the bits it has in the full run."""
    Cc, B, L = 260, 3, 41
    x, mod, _, _ = AC.case(Cc, B, L)
    g = AC.upstream(Cc, B, L).to(dev)
    _, scale, shift = _views(mod, dev)
    full = _run_bwd(dev, x.to(dev), scale, shift, g)
    for k in range(3):
        leaves = [t.detach().requires_grad_(i == k) for i, t in enumerate((x.to(dev), scale, shift))]
        h = seam.adaln_modulate(*leaves)
        (gk,) = torch.autograd.grad(h, leaves[k], g)
        assert torch.equal(gk, full[1 + k])


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("which", ["scale", "shift", "both"])
def test_half_modulation_vectors(dev, half, which):
    Cc, B, L = 260, 3, 41
    x, mod, _, _ = AC.case(Cc, B, L)
    g = AC.upstream(Cc, B, L, 16.0)
    sdt = half if which in ("scale", "both") else torch.float32
    hdt = half if which in ("shift", "both") else torch.float32
    sc, sh = mod[:, :, 2].to(sdt), mod[:, :, 4].to(hdt)          # the rounded inputs: the reference starts from them
    scale, shift = mod.to(dev, sdt)[:, :, 2], mod.to(dev, hdt)[:, :, 4]
    assert E.train_vec_in_place(scale) and E.train_vec_in_place(shift)
    ref = AC.bwd_ref(x, sc, sh, g)
    tols = AC.bwd_bounds(x, sc, sh, g, ref[1:])
    got = _run_bwd(dev, x.to(dev), scale, shift, g.to(dev))
    print(f"\nadaln_modulate with {which} in {half}")
    _assert_all("h", got[0], *AC.fwd_ref(x, sc, sh))
    assert got[1].dtype == torch.float32 and got[2].dtype == sdt and got[3].dtype == hdt
    for name, a, r, tol in zip(("dx", "dscale", "dshift"), got[1:], ref[1:], tols):
        _assert_all(name, a, r, tol)


def test_fp16_mixed_with_bf16_raises(dev):
    x = torch.zeros(2, 5, 64, device=dev)
    v = torch.zeros(2, 1, 64, device=dev)
    with pytest.raises(E.SdvarError, match="float16 mixed with bfloat16"):
        seam.adaln_modulate(x, v.half(), v.bfloat16())
    with pytest.raises(E.SdvarError, match="float16 mixed with bfloat16"):
        seam.gated_residual(x, x.half(), v.bfloat16())


def test_fp16_dshift_overflows_to_inf(dev):
    """Nothing is clamped: a column sum beyond 65504 is inf in an fp16 dshift (a GradScaler sees it) and finite in bf16 and fp32."""
    Cc, B, L = 64, 2, 5
    x, mod, _, _ = AC.case(Cc, B, L)
    g = torch.full((B, L, Cc), 65536.0, device=dev)
    out = {}
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        _, scale, shift = _views(mod, dev, dtype=dt)
        out[dt] = _run_bwd(dev, x.to(dev), scale, shift, g)[3]
        assert out[dt].dtype == dt
    assert torch.isinf(out[torch.float16]).all() and (out[torch.float16] > 0).all()
    assert torch.equal(out[torch.float32], torch.full((B, 1, Cc), 65536.0 * L, device=dev)) and torch.isfinite(out[torch.bfloat16]).all()
    assert torch.equal(out[torch.bfloat16].float(), out[torch.float32])          # 5 * 2^16 is a bf16 number


def _gate_inputs(Cc, B, L, kind, rs):
    x, mod, _, _ = AC.case(Cc, B, L)
    mod = mod.clone()
    if kind == "init1e-5":
        mod[:, :, 0] = 1e-5
    elif kind == "pm30":
        mod[:, :, 0] = 30.0 * torch.sign(mod[:, :, 0])
    y = AC.rnd(31 + Cc, (B, L, Cc))
    r = None if rs is None else torch.tensor(rs[:B], dtype=torch.float32)
    return x, y, mod, AC.upstream(Cc, B, L, 256.0), r


def _run_gate(x, y, gamma, r, g):
    xl, yl, gl = (t.detach().requires_grad_(True) for t in (x, y, gamma))
    out = seam.gated_residual(xl, yl, gl, r)
    return (out.detach(),) + torch.autograd.grad(out, (xl, yl, gl), g)


# y and gamma each float32 or half on its own, one half dtype per call: (fp32 y, half gamma) is what install_train_amp(ffn=True, adaln=True) produces (fused_mlp_func_grad
# returns float32, ada_lin half), (half y, fp32 gamma) what a shared_aln block produces under autocast (ada_gss + cond is float32)
GATE_DTYPES = [(torch.float32, torch.float32), (torch.float32, torch.float16), (torch.float32, torch.bfloat16), (torch.float16, torch.float32),
               (torch.bfloat16, torch.float32), (torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16)]


@pytest.mark.parametrize("ydt,gdt", GATE_DTYPES)
@pytest.mark.parametrize("rs", [None, (0.0, 1 / 0.9, 1 / 0.9)])
@pytest.mark.parametrize("kind", ["init1e-5", "rnd", "pm30"])
@pytest.mark.parametrize("Cc,L,one_row", [(260, 41, False), (1024, 41, True), (2048, 5, False), (3072, 5, False)])
def test_gated_residual(dev, ydt, gdt, rs, kind, Cc, L, one_row):
    B = 3
    x, y, mod, g, r = _gate_inputs(Cc, B, L, kind, rs)
    y, gm = y.to(ydt), (mod[:1] if one_row else mod)[:, :, 0].to(gdt)
    refs, tols = AC.gate_ref(x, y, gm, r, g)
    if ydt == torch.float32:
        for name, a, rf, t in zip(("out", "dy", "dgamma"), AC.gate_torch32(x, y, gm, r, g), refs, tols):
            assert AC.worst(name + " torch float32 CPU", a, rf, t) <= 1.0
    gamma = (mod[:1] if one_row else mod).to(dev, gdt)[:, :, 0]
    assert E.train_vec_in_place(gamma) and (one_row or gamma.stride(0) == 6 * Cc)
    rd = None if r is None else r.to(dev)
    yd = y.to(dev)
    y0 = yd.clone()
    gd = g.to(dev)
    out, dx, dy, dgamma = _run_gate(x.to(dev), yd, gamma, rd, gd)
    again = _run_gate(x.to(dev), yd, gamma, rd, gd)
    print(f"\ngated_residual C={Cc} L={L} y {ydt} gamma {kind} in {gdt} row_scale {rs} one_row={one_row}")
    assert torch.equal(yd, y0), "y must not be modified"
    assert out.dtype == torch.float32 and dy.dtype == ydt and dgamma.dtype == gdt and dgamma.shape == gamma.shape
    assert torch.equal(dx, gd)                     # the gradient of x: the upstream gradient itself
    for a, b in zip((out, dy, dgamma), (again[0], again[2], again[3])):
        assert torch.equal(a, b)
    for name, a, rf, t in zip(("out", "dy", "dgamma"), (out, dy, dgamma), refs, tols):
        _assert_all(name, a, rf, t)
    if r is not None:
        assert float(dy[0].float().abs().max()) == 0.0 and torch.equal(out[0], x.to(dev)[0])          # the dropped image
    with torch.no_grad():
        assert torch.equal(seam.gated_residual(x.to(dev), yd, gamma, rd), out)
    xl = x.to(dev).requires_grad_(True)          # only x needs a gradient: nothing is saved, no kernel runs, the gradient is g
    (gx,) = torch.autograd.grad(seam.gated_residual(xl, yd, gamma, rd), xl, gd)
    assert torch.equal(gx, gd)


def test_views_that_break_the_16_byte_rule_are_copied(dev):
    Cc, B, L = 260, 3, 41
    x, mod, _, _ = AC.case(Cc, B, L)
    g = AC.upstream(Cc, B, L).to(dev)
    wide = torch.zeros(B, 1, 6 * Cc + 3, device=dev)
    wide[:, :, 1:6 * Cc + 1] = mod.view(B, 1, 6 * Cc).to(dev)
    bad = wide[:, :, 1:6 * Cc + 1].view(B, 1, 6, Cc)          # rows start 4 bytes off the 16-byte grid, at a batch stride that is no multiple of 4 elements
    s_bad, h_bad = bad[:, :, 2], bad[:, :, 4]
    assert not E.train_vec_in_place(s_bad)
    with pytest.raises(E.SdvarError, match="16-byte rule"):
        E.adaln_fwd(x.to(dev), s_bad, h_bad)
    xw = torch.zeros(B, L, Cc + 4, device=dev)
    xw[:, :, :Cc] = x.to(dev)
    a = _run_bwd(dev, xw[:, :, :Cc], s_bad, h_bad, g)
    b = _run_bwd(dev, x.to(dev), s_bad.contiguous(), h_bad.contiguous(), g)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    y = AC.rnd(5, (B, L, Cc)).to(dev)
    assert not E.train_vec_in_place(bad[:, :, 0])
    ga, gb = _run_gate(xw[:, :, :Cc], y, bad[:, :, 0], None, g), _run_gate(x.to(dev), y, bad[:, :, 0].contiguous(), None, g)
    for u, v in zip(ga, gb):
        assert torch.equal(u, v)


def test_documented_errors(dev):
    x = torch.zeros(2, 5, 64, device=dev)
    v = torch.zeros(2, 1, 64, device=dev)
    cases = [
        (lambda: seam.adaln_modulate(x.cpu(), v, v), "GPU"),
        (lambda: seam.adaln_modulate(x, v.cpu(), v), "GPU"),
        (lambda: seam.gated_residual(x, x.cpu(), v), "GPU"),
        (lambda: seam.adaln_modulate(x.double(), v, v), r"float64.*\.float\(\)"),
        (lambda: seam.adaln_modulate(x, v.double(), v), r"float64.*\.float\(\)"),
        (lambda: seam.gated_residual(x, x.double(), v), "float64"),
        (lambda: seam.adaln_modulate(x.half(), v, v), r"float16.*\.float\(\)"),
        (lambda: seam.gated_residual(x.bfloat16(), x, v), r"bfloat16.*\.float\(\)"),
        (lambda: seam.adaln_modulate(x, v.half(), v.bfloat16()), "float16 mixed with bfloat16"),
        (lambda: seam.adaln_modulate(x, torch.zeros(3, 1, 64, device=dev), v), "does not broadcast"),
        (lambda: seam.adaln_modulate(x, v, torch.zeros(2, 5, 64, device=dev)), "does not broadcast"),
        (lambda: seam.gated_residual(x, x[:, :4], v), "expected"),
        (lambda: seam.gated_residual(x, x, torch.zeros(2, 1, 32, device=dev)), "does not broadcast"),
        (lambda: seam.gated_residual(x, x, v, torch.ones(3, device=dev)), r"row_scale.*float32 \(2,\)"),
        (lambda: seam.gated_residual(x, x, v, torch.ones(2, device=dev, dtype=torch.float16)), "row_scale"),
        (lambda: seam.adaln_modulate(torch.zeros(2, 5, 6, device=dev), torch.zeros(2, 1, 6, device=dev), torch.zeros(2, 1, 6, device=dev)), "multiple of 4 in"),
        (lambda: seam.adaln_modulate(torch.zeros(1, 2, 3076, device=dev), torch.zeros(1, 1, 3076, device=dev), torch.zeros(1, 1, 3076, device=dev)), "pad the channel"),
        (lambda: seam.adaln_modulate(x.view(10, 64), v, v), r"expected \(B, L, C\)"),
    ]
    for fn, words in cases:
        with pytest.raises(E.SdvarError, match=words):
            fn()
    for op in ("mod", "gate"):
        xl = x.clone().requires_grad_(True)
        out = seam.adaln_modulate(xl, v, v) if op == "mod" else seam.gated_residual(x, xl, v)
        (gx,) = torch.autograd.grad(out.sum(), xl, create_graph=False)
        assert gx.shape == x.shape
        out = seam.adaln_modulate(xl, v, v) if op == "mod" else seam.gated_residual(x, xl, v)
        with pytest.raises(E.SdvarError, match="double backward.*without create_graph"):
            torch.autograd.grad(out.sum(), xl, create_graph=True)


# ------------------------------------------------------------------------------------------------------------------ the stand-in model
class _Attn(nn.Module):
    def __init__(self, Cc, H):
        super().__init__()
        self.H, self.qkv, self.proj = H, nn.Linear(Cc, 3 * Cc), nn.Linear(Cc, Cc)

    def forward(self, x, attn_bias=None):
        B, L, Cc = x.shape
        q, k, v = self.qkv(x).view(B, L, 3, self.H, Cc // self.H).permute(2, 0, 3, 1, 4)
        return self.proj(torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=attn_bias).transpose(1, 2).reshape(B, L, Cc))


class _FFN(nn.Module):
    def __init__(self, Cc):
        super().__init__()
        self.fc1, self.act, self.fc2 = nn.Linear(Cc, 4 * Cc), nn.GELU(approximate="tanh"), nn.Linear(4 * Cc, Cc)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class _DropPath(nn.Module):          # helpers.py:39-56
    def __init__(self, p):
        super().__init__()
        self.drop_prob, self.scale_by_keep = p, True

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1 - self.drop_prob
        r = x.new_empty((x.shape[0],) + (1,) * (x.ndim - 1)).bernoulli_(keep)
        if keep > 0.0 and self.scale_by_keep:
            r.div_(keep)
        return x * r


class _Block(nn.Module):             # basic_var.py:128-159
    def __init__(self, Cc, H, shared, p):
        super().__init__()
        self.C, self.shared_aln = Cc, shared
        self.drop_path = _DropPath(p) if p > 0 else nn.Identity()
        self.attn, self.ffn, self.ln_wo_grad = _Attn(Cc, H), _FFN(Cc), nn.LayerNorm(Cc, eps=1e-6, elementwise_affine=False)
        if shared:
            self.ada_gss = nn.Parameter(torch.randn(1, 1, 6, Cc) / Cc ** 0.5)
        else:
            self.ada_lin = nn.Sequential(nn.SiLU(inplace=False), nn.Linear(Cc, 6 * Cc))

    def forward(self, x, cond_BD, attn_bias):
        if self.shared_aln:
            gamma1, gamma2, scale1, scale2, shift1, shift2 = (self.ada_gss + cond_BD).unbind(2)
        else:
            gamma1, gamma2, scale1, scale2, shift1, shift2 = self.ada_lin(cond_BD).view(-1, 1, 6, self.C).unbind(2)
        x = x + self.drop_path(self.attn(self.ln_wo_grad(x).mul(scale1.add(1)).add_(shift1), attn_bias=attn_bias).mul_(gamma1))
        x = x + self.drop_path(self.ffn(self.ln_wo_grad(x).mul(scale2.add(1)).add_(shift2)).mul(gamma2))
        return x


class _Head(nn.Module):              # basic_var.py:165-174
    def __init__(self, Cc):
        super().__init__()
        self.C, self.ln_wo_grad, self.ada_lin = Cc, nn.LayerNorm(Cc, eps=1e-6, elementwise_affine=False), nn.Sequential(nn.SiLU(inplace=False), nn.Linear(Cc, 2 * Cc))

    def forward(self, x_BLC, cond_BD):
        scale, shift = self.ada_lin(cond_BD).view(-1, 1, 2, self.C).unbind(2)
        return self.ln_wo_grad(x_BLC).mul(scale.add(1)).add_(shift)


class _Model(nn.Module):
    def __init__(self, Cc=256, H=4, p=0.0):
        super().__init__()
        self.C = Cc
        self.shared_ada_lin = nn.Sequential(nn.SiLU(inplace=False), nn.Linear(Cc, 6 * Cc))
        self.blocks = nn.ModuleList([_Block(Cc, H, False, p), _Block(Cc, H, True, p)])
        self.head_nm = _Head(Cc)

    def forward(self, x, cond, attn_bias=None):
        x = self.blocks[0](x, cond, attn_bias)
        x = self.blocks[1](x, self.shared_ada_lin(cond).view(-1, 1, 6, self.C), attn_bias)
        return self.head_nm(x, cond)


class _NS:
    pass


def _model_and_inputs(p=0.0):
    torch.manual_seed(1234)
    m = _Model(p=p)
    x, cond, w = AC.rnd(1, (3, 14, 256)), AC.rnd(2, (3, 256)), AC.rnd(3, (3, 14, 256))
    return m, x, cond, w


def _loss_and_grads(m, x, cond, w, autocast=False, scale=1.0):
    xl, cl = x.detach().clone().requires_grad_(True), cond.detach().clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        out = m(xl, cl)
    loss = (out.float() * w).mean() * scale          # the mean: with the GradScaler's 65536 the upstream gradient is 6 w, inside fp16's range as a trainer's is
    loss.backward()
    res = {"loss": loss.detach(), "x": xl.grad, "cond": cl.grad}
    res.update({n: q.grad for n, q in m.named_parameters()})
    return res


def _compare(tag, got, ref, K, up):
    print(f"\n{tag}")
    for n, r in ref.items():
        assert got[n] is not None and torch.isfinite(got[n]).all(), n
        r = r.double()
        tol = torch.full_like(r, K * up * float(r.abs().max()))
        assert AC.worst(n, got[n], r, tol) <= 1.0, (tag, n)


@pytest.mark.parametrize("autocast", [False, True])
def test_stand_in_model_against_fp64(dev, autocast):
    m, x, cond, w = _model_and_inputs()
    scale = 65536.0 if autocast else 1.0
    ref = _loss_and_grads(m.double(), x.double(), cond.double(), w.double(), scale=scale)
    ref = {k: v.clone() for k, v in ref.items()}
    m = m.float().to(dev)
    xd, cd, wd = x.to(dev), cond.to(dev), w.to(dev)
    plain = {k: v.clone() for k, v in _loss_and_grads(m, xd, cd, wd, autocast, scale).items()}
    ns = _NS()
    (seam.install_train_amp if autocast else seam.install_train)(ns, m, adaln=True)
    assert sum("forward" in q.__dict__ for q in m.modules()) == 3
    inst = {k: v.clone() for k, v in _loss_and_grads(m, xd, cd, wd, autocast, scale).items()}
    K, up = (64, 2.0 ** -11) if autocast else (4096, 2.0 ** -24)
    _compare(f"stand-in, torch on the GPU, autocast={autocast}", plain, ref, K, up)
    _compare(f"stand-in, install(adaln=True), autocast={autocast}", inst, ref, K, up)
    seam.uninstall_adaln(m)
    assert not any("forward" in q.__dict__ for q in m.modules())
    again = _loss_and_grads(m, xd, cd, wd, autocast, scale)
    assert all(torch.equal(again[k], plain[k]) for k in plain), "uninstall_adaln must restore the class forward"


def test_stand_in_model_drop_path(dev):
    """Training mode, drop_prob = 0.5: from one generator state the installed and the uninstalled model drop the SAME images, and an image dropped on both residual lines of
    both blocks comes out of the blocks equal to x exactly."""
    m, x, cond, _ = _model_and_inputs(p=0.5)
    m = m.to(dev).train()
    xd, cd = x.to(dev), cond.to(dev)

    def blocks_only(seed):
        torch.manual_seed(seed)
        with torch.no_grad():
            h = m.blocks[0](xd, cd, None)
            return m.blocks[1](h, m.shared_ada_lin(cd).view(-1, 1, 6, 256), None)

    seeds = range(32)
    plain = [blocks_only(s) for s in seeds]
    seam.install_train(_NS(), m, adaln=True)
    inst = [blocks_only(s) for s in seeds]
    seam.uninstall_adaln(m)
    kept_p = torch.stack([(o != xd).flatten(1).any(1) for o in plain])
    kept_i = torch.stack([(o != xd).flatten(1).any(1) for o in inst])
    assert torch.equal(kept_p, kept_i), "the installed model must drop the images the reference drops"
    assert (~kept_i).any() and kept_i.any()          # 96 images x 4 draws at p = 0.5: six images are expected to be dropped four times, most are not
    for o, q in zip(inst, plain):
        assert torch.isfinite(o).all() and (o - q).abs().max() <= 4096 * 2.0 ** -24 * q.abs().max()
