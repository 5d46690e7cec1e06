"""seam.adaln_modulate / seam.gated_residual / install_train(adaln=True) without a GPU: the entry points are exported and bound, every argument check answers before any
GPU call (the pointers below are never dereferenced), the workspace sizes are the documented ones, the installer binds and unbinds, and torch's float32 autograd on the
CPU meets the backward bounds of adaln_cases.py on every input family - the condition that keeps those bounds honest."""
import ctypes as C
import math

import pytest
import torch
import torch.nn as nn

import adaln_cases as AC
from sdvar_amd import engine as E
from sdvar_amd import seam

P = C.c_void_p(4096)          # a non-null, 16-byte aligned address that no check dereferences


@pytest.fixture(autouse=True)
def _grad_mode():
    """Other test modules switch grad mode off for the process; these tests are about autograd."""
    with torch.enable_grad():
        yield


def _lib():
    return E.load_library()


@pytest.mark.parametrize("B,L,Cc", [(1, 1, 4), (2, 5, 64), (3, 41, 260), (2, 681, 1024), (8, 680, 1024), (8, 680, 1920), (1, 32, 3072), (1, 33, 3072)])
def test_workspace_sizes(B, L, Cc):
    assert E.TRAIN_CHUNK == AC.CHUNK == 32
    chunks = math.ceil(L / 32)
    assert E.adaln_bwd_ws_bytes(B, L, Cc) == B * chunks * 2 * Cc * 4
    assert E.gate_add_bwd_ws_bytes(B, L, Cc) == B * chunks * Cc * 4


def test_workspace_size_of_a_bad_shape_raises():
    for bad in ((1, 1, 6), (1, 1, 3076), (0, 1, 64), (1, 0, 64)):
        assert _lib().sdvar_op_adaln_bwd_ws_bytes(*bad) == -1 and _lib().sdvar_op_gate_add_bwd_ws_bytes(*bad) == -1
        with pytest.raises(E.SdvarError):
            E.adaln_bwd_ws_bytes(*bad)


def _calls(Cc=64, x=P, vec=P, dt=0, out=P):
    lib = _lib()
    return {
        "adaln_fwd": lambda: lib.sdvar_op_adaln_fwd(x, vec, dt, 0, vec, 0, 0, out, 2, 5, Cc, 1e-6, None),
        "adaln_bwd": lambda: lib.sdvar_op_adaln_bwd(x, vec, dt, 0, P, out, P, 2, P, 0, 2, P, 2, 5, Cc, 1e-6, None),
        "gate_add_fwd": lambda: lib.sdvar_op_gate_add_fwd(x, P, 0, vec, dt, 0, None, out, 2, 5, Cc, None),
        "gate_add_bwd": lambda: lib.sdvar_op_gate_add_bwd(x, P, 0, vec, dt, 0, None, out, P, 2, P, 2, 5, Cc, None),
    }


@pytest.mark.parametrize("name", ["adaln_fwd", "adaln_bwd", "gate_add_fwd", "gate_add_bwd"])
def test_argument_errors_without_gpu(name):
    lib = _lib()
    for kw, word in ((dict(Cc=6), b"C=6"), (dict(Cc=3076), b"C=3076"), (dict(x=None), b"null"), (dict(vec=None), b"null"), (dict(dt=3), b"dtype"), (dict(dt=-1), b"dtype"),
                     (dict(x=C.c_void_p(4100)), b"16-byte"), (dict(vec=C.c_void_p(4104)), b"16-byte")):
        assert _calls(**kw)[name]() == 1, (name, kw)
        msg = lib.sdvar_last_error()
        assert word in msg and name.encode() in msg, (name, kw, msg)


def test_backward_entry_points_want_an_output_and_a_workspace():
    lib = _lib()
    assert lib.sdvar_op_adaln_bwd(P, P, 0, 0, P, None, None, 2, None, 0, 2, P, 2, 5, 64, 1e-6, None) == 1 and b"no output" in lib.sdvar_last_error()
    assert lib.sdvar_op_adaln_bwd(P, P, 0, 0, P, P, P, 2, None, 0, 2, None, 2, 5, 64, 1e-6, None) == 1 and b"workspace" in lib.sdvar_last_error()
    assert lib.sdvar_op_adaln_bwd(P, P, 0, 0, P, P, P, 3, None, 0, 2, P, 2, 5, 64, 1e-6, None) == 1 and b"dscale_rows" in lib.sdvar_last_error()
    assert lib.sdvar_op_gate_add_bwd(P, P, 0, P, 0, 0, None, None, None, 2, P, 2, 5, 64, None) == 1 and b"no output" in lib.sdvar_last_error()
    assert lib.sdvar_op_gate_add_bwd(P, P, 0, P, 0, 0, None, P, P, 2, None, 2, 5, 64, None) == 1 and b"workspace" in lib.sdvar_last_error()
    assert lib.sdvar_op_adaln_fwd(P, P, 0, 6, P, 0, 0, P, 2, 5, 64, 1e-6, None) == 1 and b"batch stride" in lib.sdvar_last_error()          # 24 bytes: rows off the 16-byte grid


def test_cpu_tensors_raise_naming_the_gpu():
    x, v = torch.zeros(2, 5, 64), torch.zeros(2, 1, 64)
    with pytest.raises(E.SdvarError, match="GPU"):
        seam.adaln_modulate(x, v, v)
    with pytest.raises(E.SdvarError, match="GPU"):
        seam.gated_residual(x, x, v)
    with pytest.raises(E.SdvarError, match="GPU"):
        seam.adaln_modulate(x.requires_grad_(True), v, v)


class _Branch(nn.Module):
    def __init__(self, Cc):
        super().__init__()
        self.lin = nn.Linear(Cc, Cc)

    def forward(self, x, attn_bias=None):
        return self.lin(x)


class _DropPath(nn.Module):
    def __init__(self, p):
        super().__init__()
        self.drop_prob, self.scale_by_keep = p, True


class _Block(nn.Module):
    def __init__(self, Cc, shared, p=0.0):
        super().__init__()
        self.attn, self.ffn, self.ln_wo_grad = _Branch(Cc), _Branch(Cc), nn.LayerNorm(Cc, eps=1e-6, elementwise_affine=False)
        self.drop_path = _DropPath(p) if p > 0 else nn.Identity()
        if shared:
            self.ada_gss = nn.Parameter(torch.randn(1, 1, 6, Cc))
        else:
            self.ada_lin = nn.Sequential(nn.SiLU(), nn.Linear(Cc, 6 * Cc))

    def forward(self, x, cond_BD, attn_bias):
        raise AssertionError("the class forward")


class _Head(nn.Module):
    def __init__(self, Cc):
        super().__init__()
        self.ln_wo_grad, self.ada_lin = nn.LayerNorm(Cc, eps=1e-6, elementwise_affine=False), nn.Sequential(nn.SiLU(), nn.Linear(Cc, 2 * Cc))

    def forward(self, x, cond_BD):
        raise AssertionError("the class forward")


class _Model(nn.Module):
    def __init__(self, Cc=16, p=0.0):
        super().__init__()
        self.blocks = nn.ModuleList([_Block(Cc, False, p), _Block(Cc, True, p)])
        self.head_nm = _Head(Cc)


class _NS:
    pass


def test_installer_wants_a_model():
    for fn in (seam.install_train, seam.install_train_amp):
        with pytest.raises(E.SdvarError, match="model"):
            fn(_NS(), None, adaln=True)
    ns = _NS()
    seam.install_train(ns)                      # the default: today's behaviour, no model needed
    assert ns.slow_attn is seam.slow_attn_grad and ns.fused_mlp_func is None


@pytest.mark.parametrize("installer", [seam.install_train, seam.install_train_amp])
@pytest.mark.parametrize("training", [False, True])
def test_installer_binds_records_and_unbinds(monkeypatch, installer, training):
    calls = []

    def fake_mod(x, scale, shift, eps=1e-6):
        calls.append(("mod", tuple(scale.shape), tuple(scale.stride()), eps))
        return x

    def fake_gate(x, y, gamma, row_scale=None):
        calls.append(("gate", tuple(gamma.shape), row_scale))
        return x + y

    monkeypatch.setattr(seam, "adaln_modulate", fake_mod)
    monkeypatch.setattr(seam, "gated_residual", fake_gate)
    Cc, B, L = 16, 3, 5
    model = _Model(Cc, p=0.5).train(training)
    ns = _NS()
    installer(ns, model, adaln=True)
    bound = [m for m in model.modules() if "forward" in m.__dict__]
    assert len(bound) == 3
    x, cond = torch.randn(B, L, Cc), torch.randn(B, Cc)
    with torch.no_grad():
        h = model.blocks[0](x, cond, None)
        assert [c[0] for c in calls] == ["mod", "gate", "mod", "gate"]
        assert calls[0][1] == (B, 1, Cc) and calls[0][2] == (6 * Cc, 6 * Cc, 1) and calls[0][3] == 1e-6          # the unbind(2) view itself, not a copy
        calls.clear()
        model.blocks[1](h, cond.view(B, 1, 1, Cc).expand(B, 1, 6, Cc), None)
        assert [c[0] for c in calls] == ["mod", "gate", "mod", "gate"]
        gates = [c[2] for c in calls if c[0] == "gate"]
        if training:
            assert all(r is not None and tuple(r.shape) == (B,) and r.dtype == torch.float32 and set(r.tolist()) <= {0.0, 2.0} for r in gates)
        else:
            assert gates == [None, None]
        calls.clear()
        model.head_nm(h, cond)
        assert [c[0] for c in calls] == ["mod"] and calls[0][1] == (B, 1, Cc) and calls[0][2][0] == 2 * Cc
    seam.uninstall_adaln(model)
    assert not any("forward" in m.__dict__ for m in model.modules())
    with pytest.raises(AssertionError, match="class forward"):
        model.head_nm(x, cond)


def test_drop_path_draw_is_the_references(monkeypatch):
    """The factor is drawn as helpers.py:43-45 draws it: the same generator position, the same images dropped."""
    dp = _DropPath(0.5).train()
    y = torch.zeros(6, 3, 8)
    torch.manual_seed(11)
    r = seam._drop_path_scale(dp, y)
    torch.manual_seed(11)
    want = y.new_empty((6, 1, 1)).bernoulli_(0.5).div_(0.5)
    assert torch.equal(r, want.view(6)) and seam._drop_path_scale(dp.eval(), y) is None and seam._drop_path_scale(nn.Identity(), y) is None


@pytest.mark.parametrize("Cc,B,L,one_row", AC.BWD_CASES)
def test_torch_float32_meets_the_backward_bounds(Cc, B, L, one_row):
    x, mod, fam, grp = AC.case(Cc, B, L)
    scale, shift = (mod[:1, :, 2], mod[:1, :, 4]) if one_row else (mod[:, :, 2], mod[:, :, 4])
    g = AC.upstream(Cc, B, L)
    ref = AC.bwd_ref(x, scale, shift, g)
    tols = AC.bwd_bounds(x, scale, shift, g, ref[1:])
    got = AC.bwd_torch32(x, scale, shift, g)
    print(f"\ntorch float32 CPU autograd, C={Cc} B={B} L={L} one_row={one_row}")
    for name, a, r, t in zip(("dx", "dscale", "dshift"), got[1:], ref[1:], tols):
        assert AC.worst(name, a, r, t) <= 1.0
    assert AC.worst("h (forward bar)", got[0], *AC.fwd_ref(x, scale, shift)) <= 1.0


@pytest.mark.parametrize("rs", [None, (0.0, 1 / 0.9, 1 / 0.9)])
@pytest.mark.parametrize("kind", ["init1e-5", "rnd", "pm30"])
def test_torch_float32_meets_the_gate_bounds(rs, kind):
    x, y, gamma, g, r = gate_inputs(260, 3, 41, kind, rs)
    refs, tols = AC.gate_ref(x, y, gamma, r, g)
    got = AC.gate_torch32(x, y, gamma, r, g)
    print(f"\ntorch float32 CPU autograd of the gated residual, gamma {kind}, row_scale {rs}")
    for name, a, rf, t in zip(("out", "dy", "dgamma"), got, refs, tols):
        assert AC.worst(name, a, rf, t) <= 1.0


def gate_inputs(Cc, B, L, kind, rs):
    x, mod, _, _ = AC.case(Cc, B, L)
    mod = mod.clone()
    if kind == "init1e-5":
        mod[:, :, 0] = 1e-5
    elif kind == "pm30":
        mod[:, :, 0] = 30.0 * torch.sign(mod[:, :, 0])
    y = AC.rnd(31 + Cc, (B, L, Cc))
    r = None if rs is None else torch.tensor(rs[:B], dtype=torch.float32)
    return x, y, mod[:, :, 0], AC.upstream(Cc, B, L, 256.0), r
