"""sdvar_amd.seam without a GPU: every unsupported case raises SdvarError before any kernel is touched, the C entry point reports argument errors through
sdvar_last_error, and install() sets the slots of a basic_var-like module and of the FFN objects that captured the slot at construction."""
import ctypes as C
import types

import pytest
import torch

from sdvar_amd import engine as E
from sdvar_amd import seam

class _Fake(torch.Tensor):
    """A CPU tensor that reports is_cuda = True: lets the argument checks that come AFTER the device check run without a GPU.  Nothing is ever launched on it:
    every case below must raise before the library is called."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)

    @property
    def is_cuda(self):
        return True


def _qkv(L=8, dtype=torch.float32, c=64, grad=False):
    t = torch.zeros(1, 2, L, c, dtype=dtype, requires_grad=grad)
    return _Fake(t)


def test_attention_error_cases():
    q = _qkv()
    with pytest.raises(E.SdvarError, match="dropout"):
        seam.slow_attn(q, q, q, 1.0, None, 0.1)
    with pytest.raises(E.SdvarError, match="dropout"):
        seam.memory_efficient_attention(q, q, q, None, p=0.5)
    with pytest.raises(E.SdvarError, match="CPU"):
        seam.slow_attn(torch.zeros(1, 2, 8, 64), q, q, 1.0)
    with pytest.raises(E.SdvarError, match="CPU"):
        seam.memory_efficient_attention(torch.zeros(1, 8, 2, 64), q, q)
    for bad in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(E.SdvarError, match="float32"):
            seam.slow_attn(_qkv(dtype=bad), q, q, 1.0)
    with pytest.raises(E.SdvarError, match="head dim"):
        seam.slow_attn(_qkv(c=32), _qkv(c=32), _qkv(c=32), 1.0)
    with pytest.raises(E.SdvarError, match="head dim"):
        seam.memory_efficient_attention(_qkv(c=128), _qkv(c=128), _qkv(c=128))
    g = _qkv(grad=True)
    assert g.requires_grad
    with torch.enable_grad():
        with pytest.raises(E.SdvarError, match="grad"):
            seam.slow_attn(g, q, q, 1.0)
        with pytest.raises(E.SdvarError, match="grad"):
            seam.slow_attn(q, q, g, 1.0)


def test_fused_mlp_error_cases():
    x, w1, w2 = _Fake(torch.zeros(3, 64)), _Fake(torch.zeros(256, 64)), _Fake(torch.zeros(64, 256))
    with pytest.raises(E.SdvarError, match="activation"):
        seam.fused_mlp_func(x, w1, w2, activation="relu")
    with pytest.raises(E.SdvarError, match="return_residual"):
        seam.fused_mlp_func(x, w1, w2, return_residual=True)
    with pytest.raises(E.SdvarError, match="process group"):
        seam.fused_mlp_func(x, w1, w2, process_group=object())
    with pytest.raises(E.SdvarError, match="CPU"):
        seam.fused_mlp_func(torch.zeros(3, 64), w1, w2)
    with pytest.raises(E.SdvarError, match="float32"):
        seam.fused_mlp_func(_Fake(torch.zeros(3, 64, dtype=torch.float16)), w1, w2)
    with pytest.raises(E.SdvarError, match="float32"):
        seam.fused_mlp_func(x, _Fake(torch.zeros(256, 64, dtype=torch.bfloat16)), w2)
    wg = _Fake(torch.zeros(256, 64, requires_grad=True))
    with torch.enable_grad():
        with pytest.raises(E.SdvarError, match="grad"):
            seam.fused_mlp_func(x, wg, w2)
    with pytest.raises(E.SdvarError, match="gemm_mode"):
        seam.configure(gemm_mode="fp8")


def test_op_sdpa_argument_errors_without_gpu():
    lib = E.load_library()
    i64 = C.c_int64
    buf = (C.c_float * 64)()                                        # host memory: only its (aligned) address is looked at, the call returns before any HIP call
    base = (C.addressof(buf) + 15) & ~15
    p = C.c_void_p(base)
    dense = lambda L: [2 * L * 64, L * 64, 64]
    ok = (i64 * 12)(*(dense(4) * 4))
    rc = lib.sdvar_op_sdpa(None, p, p, p, ok, None, 0, None, None, 1, 2, 4, 4, 64, 1.0, None)
    assert rc == 1 and b"null operand" in lib.sdvar_last_error()
    rc = lib.sdvar_op_sdpa(p, p, p, None, ok, None, 0, None, None, 1, 2, 4, 4, 64, 1.0, None)
    assert rc == 1 and b"null operand" in lib.sdvar_last_error()
    bad = (i64 * 12)(*(dense(4) + [2 * 4 * 66, 4 * 66, 66] + dense(4) * 2))            # k token stride 66 floats = 264 bytes
    rc = lib.sdvar_op_sdpa(p, p, p, p, bad, None, 0, None, None, 1, 2, 4, 4, 64, 1.0, None)
    assert rc == 1 and b"16-byte aligned" in lib.sdvar_last_error() and b"k strides" in lib.sdvar_last_error()
    rc = lib.sdvar_op_sdpa(C.c_void_p(base + 4), p, p, p, ok, None, 0, None, None, 1, 2, 4, 4, 64, 1.0, None)
    assert rc == 1 and b"q is not 16-byte aligned" in lib.sdvar_last_error()
    rc = lib.sdvar_op_sdpa(p, p, p, p, ok, None, 0, None, None, 1, 2, 4, 4, 32, 1.0, None)
    assert rc == 1 and b"head dim 32" in lib.sdvar_last_error()
    rc = lib.sdvar_op_sdpa(p, p, p, p, ok, None, 1, None, None, 1, 2, 4, 4, 64, 1.0, None)          # bias kind without a bias
    assert rc == 1 and b"bias" in lib.sdvar_last_error()
    rc = lib.sdvar_op_sdpa_skip_map(None, 1, (i64 * 3)(0, 0, 4), 1, 1, 4, 4, p, None)
    assert rc == 1 and b"null operand" in lib.sdvar_last_error()


class _FFN:
    def __init__(self, slot):
        self.fused_mlp_func = slot          # basic_var.py:36: the module global is captured at construction


class _Model:
    def __init__(self):
        self.ffns = [_FFN(None), _FFN(None), _FFN(None)]
        self.other = types.SimpleNamespace(weight=1)

    def modules(self):
        return [self, self.other] + self.ffns


def test_install_sets_slots_and_captured_attributes():
    mod = types.SimpleNamespace(slow_attn=object(), fused_mlp_func=None, memory_efficient_attention=None)
    model = _Model()
    seam.install(mod)
    assert mod.slow_attn is seam.slow_attn and mod.fused_mlp_func is seam.fused_mlp_func
    assert all(f.fused_mlp_func is None for f in model.ffns)               # no model given: captured attributes untouched
    seam.install(mod, model)
    assert all(f.fused_mlp_func is seam.fused_mlp_func for f in model.ffns)
    assert not hasattr(model.other, "fused_mlp_func") and not hasattr(model, "fused_mlp_func")
    assert mod.memory_efficient_attention is None


def test_install_on_real_modules():
    """nn.Module FFNs as the reference builds them: the slot attribute is a plain (non-parameter) attribute of a submodule."""
    import torch.nn as nn

    class FFN(nn.Module):
        def __init__(self):
            super().__init__()
            self.fused_mlp_func = None
            self.fc1 = nn.Linear(4, 8)

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.ffn = FFN()

    net = nn.Sequential(Block(), Block())
    seam.install(types.SimpleNamespace(), net)
    assert all(b.ffn.fused_mlp_func is seam.fused_mlp_func for b in net)
