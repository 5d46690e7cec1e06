"""seam.qk_l2norm / install_qknorm / install_train(qknorm=True) without a GPU: the entry points are exported and bound, every argument check answers before any GPU call
(the pointers below are never dereferenced), the workspace size is the documented one, the installer binds and unbinds, and torch's float32 autograd on the CPU meets
every bound of qknorm_cases.py on every input family - the condition that keeps those bounds honest."""
import ctypes as C
import math

import pytest
import torch
import torch.nn as nn

import qknorm_cases as QC
from sdvar_amd import engine as E
from sdvar_amd import seam
from sdvar_amd.seam import install_qknorm, qk_l2norm, uninstall_qknorm          # noqa: F401  (the feature under test: without it nothing here runs)

P = C.c_void_p(4096)          # a non-null, 16-byte aligned address that no check dereferences
S9 = (C.c_int64 * 9)(192, 64, 192, 192, 64, 192, 192, 64, 192)


@pytest.fixture(autouse=True)
def _grad_mode():
    """Other test modules switch grad mode off for the process; these tests are about autograd."""
    with torch.enable_grad():
        yield


def _lib():
    return E.load_library()


@pytest.mark.parametrize("H,B,L", QC.SHAPES)
def test_torch_float32_on_the_cpu_meets_every_bound(H, B, L):
    print(f"\nqk_l2norm bounds, torch float32 on the CPU, H={H} B={B} L={L}")
    for dt in QC.DTYPES:
        for bias in (True, False):
            QC.assert_torch32_meets_the_bounds(QC.full(H, B, L, dt, bias), f"{dt} bias={bias}")


def test_the_cases_cover_every_family_and_every_kind_of_head():
    for slot in (0, 1):
        seen = {f for H, B, L in QC.SHAPES if B * L <= 10 for row in QC.families(H, B, L, slot) for f in row}
        assert seen == set(QC.FAMILIES)
    kinds = set()
    for H, B, L in QC.SHAPES:
        sl = QC.case(H, B, L)[3]
        k = {"at" if float(v) == QC.MAX_LOG else "above" if float(v) > QC.MAX_LOG else "below" for v in sl[:3]}
        assert H < 3 or k == {"at", "above", "below"}
        kinds |= k
    assert kinds == {"at", "above", "below"}
    assert torch.tensor(QC.MAX_LOG, dtype=torch.float32).item() == QC.MAX_LOG          # exactly a float32 number: "at max_log" survives the cast


@pytest.mark.parametrize("B,L,H", [(1, 1, 1), (2, 5, 3), (3, 41, 30), (2, 681, 16), (8, 680, 16), (8, 680, 30), (1, 32, 48), (1, 33, 48)])
def test_workspace_size(B, L, H):
    assert E.TRAIN_CHUNK == QC.CHUNK == 32
    assert E.qknorm_bwd_ws_bytes(B, L, H) == B * math.ceil(L / 32) * 3 * 64 * H * 4


def test_workspace_size_of_a_bad_shape_raises():
    for bad in ((1, 1, 0), (1, 1, 49), (0, 1, 4), (1, 0, 4), (2 ** 15, 2 ** 15, 4)):
        assert _lib().sdvar_op_qknorm_bwd_ws_bytes(*bad) == -1
        with pytest.raises(E.SdvarError):
            E.qknorm_bwd_ws_bytes(*bad)


def _calls(H=4, qkv=P, dt=0, vec=P, out=P, v=P, vb=P, ws=P, strides=S9, g=P):
    lib = _lib()
    return {
        "qknorm_fwd": lambda: lib.sdvar_op_qknorm_fwd(qkv, dt, vec, vb, P, 4.6, out, P, v, 2, 5, H, None),
        "qknorm_bwd": lambda: lib.sdvar_op_qknorm_bwd(qkv, dt, vec, P, 4.6, g, P, P, strides, out, P, P, P, ws, 2, 5, H, None),
    }


@pytest.mark.parametrize("name", ["qknorm_fwd", "qknorm_bwd"])
def test_argument_errors_without_gpu(name):
    lib = _lib()
    for kw, word in ((dict(H=0), b"H=0"), (dict(H=49), b"H=49"), (dict(qkv=None), b"null"), (dict(dt=3), b"dtype"), (dict(dt=-1), b"dtype"),
                     (dict(qkv=C.c_void_p(4100)), b"16-byte"), (dict(vec=C.c_void_p(4104)), b"16-byte"), (dict(out=C.c_void_p(4100)), b"16-byte")):
        assert _calls(**kw)[name]() == 1, (name, kw)
        msg = lib.sdvar_last_error()
        assert word in msg and name.encode() in msg, (name, kw, msg)


def test_entry_point_rules_without_gpu():
    lib = _lib()
    assert _calls(v=None)["qknorm_fwd"]() == 1 and b"both or neither" in lib.sdvar_last_error()
    assert _calls(vb=None)["qknorm_fwd"]() == 1 and b"both or neither" in lib.sdvar_last_error()
    assert lib.sdvar_op_qknorm_bwd(P, 0, P, P, 4.6, P, P, P, S9, None, None, None, None, P, 2, 5, 4, None) == 1 and b"no output" in lib.sdvar_last_error()
    assert _calls(ws=None)["qknorm_bwd"]() == 1 and b"workspace" in lib.sdvar_last_error()
    assert _calls(strides=None)["qknorm_bwd"]() == 1 and b"null" in lib.sdvar_last_error()
    for bad in ((194, 64, 192), (192, -64, 192), (192, 64, 6)):
        s = (C.c_int64 * 9)(*bad, 192, 64, 192, 192, 64, 192)
        assert _calls(strides=s)["qknorm_bwd"]() == 1 and b"multiples of 4" in lib.sdvar_last_error()
    assert _calls(g=C.c_void_p(4100))["qknorm_bwd"]() == 1 and b"aligned to 4 elements" in lib.sdvar_last_error()
    half_dv = lambda addr: lib.sdvar_op_qknorm_bwd(P, 1, P, P, 4.6, P, P, C.c_void_p(addr), S9, P, None, None, None, None, 2, 5, 4, None)
    assert half_dv(4100) == 1 and b"aligned to 4 elements" in lib.sdvar_last_error()          # a half dv: 8 bytes per lane


def test_documented_errors_name_the_argument():
    qkv, sl = torch.zeros(2, 5, 3, 4, 64), torch.zeros(4)
    cases = [
        (lambda: seam.qk_l2norm(qkv, sl, 4.6), r"qkv is a CPU tensor"),
        (lambda: seam.qk_l2norm(qkv.requires_grad_(False).clone().requires_grad_(True), sl, 4.6), r"qkv is a CPU tensor"),
        (lambda: seam.qk_l2norm(torch.zeros(2, 5, 3, 8, 32), sl, 4.6), r"head dim 32 of qkv"),
        (lambda: seam.qk_l2norm(torch.zeros(1, 2, 3, 49, 64), sl, 4.6), r"H = 49 heads of qkv"),
        (lambda: seam.qk_l2norm(qkv.double(), sl, 4.6), r"qkv is torch.float64"),
        (lambda: seam.qk_l2norm(qkv.to(torch.int32), sl, 4.6), r"qkv is torch.int32"),
        (lambda: seam.qk_l2norm(qkv.view(2, 5, 768), sl, 4.6), r"qkv has shape .*expected \(B, L, 3, H, 64\)"),
        (lambda: seam.qk_l2norm(qkv, sl, 4.6, layout="BLCh"), r"layout 'BLCh'"),
        (lambda: E.qknorm_fwd(qkv, sl, 4.6), r"qkv is a CPU tensor"),
        (lambda: E.qknorm_bwd(qkv, sl, 4.6, None, None, None, None), r"qkv is a CPU tensor"),
    ]
    for fn, words in cases:
        with pytest.raises(E.SdvarError, match=words):
            fn()


# ------------------------------------------------------------------------------------------------------------------ install / uninstall on a CPU stand-in
class _Attn(nn.Module):
    def __init__(self, l2, strip=()):
        super().__init__()
        self.num_heads, self.attn_l2_norm = 2, l2
        self.mat_qkv, self.proj = nn.Linear(128, 384, bias=False), nn.Linear(128, 128)
        self.q_bias, self.v_bias = nn.Parameter(torch.zeros(128)), nn.Parameter(torch.zeros(128))
        if l2:
            self.scale_mul_1H11, self.max_scale_mul = nn.Parameter(torch.zeros(1, 2, 1, 1)), 4.6
        for n in strip:
            delattr(self, n)

    def forward(self, x, attn_bias):
        return x


class _NS:
    pass


def _model(*l2):
    return nn.ModuleList([_Attn(v) for v in l2])


@pytest.mark.parametrize("how", ["install_qknorm", "install_train", "install_train_amp"])
def test_install_binds_only_l2_norm_modules_and_uninstall_restores(how):
    m = _model(True, False, True)
    if how == "install_qknorm":
        seam.install_qknorm(m)
    else:
        getattr(seam, how)(_NS(), m, qknorm=True)
    assert ["forward" in a.__dict__ for a in m] == [True, False, True]
    assert m[0].forward.__func__ is seam._qknorm_attn_forward
    seam.uninstall_adaln(m)          # the other installer's uninstall leaves these alone
    assert ["forward" in a.__dict__ for a in m] == [True, False, True]
    seam.uninstall_qknorm(m)
    assert not any("forward" in a.__dict__ for a in m)
    x = torch.zeros(1, 2, 128)
    assert m[0](x, None) is x          # the class forward is back
    getattr(seam, "install_train" if how == "install_qknorm" else how)(_NS(), m)          # qknorm=False (default) binds nothing
    assert not any("forward" in a.__dict__ for a in m)


def test_install_needs_the_model_and_a_self_attention_like_module():
    for fn in (seam.install_train, seam.install_train_amp):
        with pytest.raises(E.SdvarError, match="qknorm=True.*pass the model"):
            fn(_NS(), None, qknorm=True)
    with pytest.raises(E.SdvarError, match="pass the model"):
        seam.install_qknorm(None)
    for missing in ("q_bias", "v_bias", "scale_mul_1H11", "proj"):
        m = nn.ModuleList([_Attn(True, strip=(missing,))])
        with pytest.raises(E.SdvarError, match=f"_Attn has mat_qkv and attn_l2_norm=True but no {missing}"):
            seam.install_qknorm(m)
        assert "forward" not in m[0].__dict__


def test_the_bound_forward_raises_on_the_cpu_before_any_launch():
    m = _model(True)
    seam.install_qknorm(m)
    m[0].using_flash = m[0].using_xform = m[0].caching = False
    with pytest.raises(E.SdvarError, match="qkv is a CPU tensor"):
        m[0](torch.zeros(1, 2, 128), None)
