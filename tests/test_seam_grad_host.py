"""seam.slow_attn_grad / memory_efficient_attention_grad / install_train without a GPU: the new names are public, install_train sets the slots a trainer needs, the
inference slots still refuse operands that require grad, every unsupported case of the differentiable slot raises SdvarError before the library is touched, and
sdvar_op_sdpa_lse / sdvar_op_sdpa_bwd report argument errors through sdvar_last_error before any HIP call."""
import ctypes as C
import types

import pytest
import torch

from sdvar_amd import engine as E
from sdvar_amd import seam


class _Fake(torch.Tensor):
    """A CPU tensor that reports is_cuda = True (the trick of tests/test_seam_host.py): the argument checks that come AFTER the device check run without a GPU.
    Nothing is ever launched on it: every case below must raise before the library is called."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)

    @property
    def is_cuda(self):
        return True


def _qkv(L=8, dtype=torch.float32, c=64, grad=False, H=2):
    return _Fake(torch.zeros(1, H, L, c, dtype=dtype, requires_grad=grad))


def test_new_names_are_public():
    for name in ("slow_attn_grad", "memory_efficient_attention_grad", "install_train"):
        assert name in seam.__all__ and callable(getattr(seam, name))
    lib = E.load_library()
    for name in ("sdvar_op_sdpa_lse", "sdvar_op_sdpa_bwd"):
        assert name in E._SIGNATURES and hasattr(lib, name)
    assert len({"slow_attn_grad", "memory_efficient_attention_grad", "install_train", "clear_caches"} & set(seam.__all__)) == 4


def test_abi_version_is_still_5():
    assert E.load_library().sdvar_abi_version() == 5 == E.ABI_VERSION


class _FFN:
    def __init__(self, slot):
        self.fused_mlp_func = slot          # basic_var.py:36: the module global is captured at construction


class _Model:
    def __init__(self, slot):
        self.ffns = [_FFN(slot), _FFN(slot), _FFN(None)]
        self.other = types.SimpleNamespace(weight=1)

    def modules(self):
        return [self, self.other] + self.ffns


def test_install_train_sets_the_slots():
    sentinel = object()
    mod = types.SimpleNamespace(slow_attn=object(), fused_mlp_func=seam.fused_mlp_func, memory_efficient_attention=sentinel, flash_attn_func=sentinel)
    model = _Model(seam.fused_mlp_func)
    seam.install_train(mod)
    assert mod.slow_attn is seam.slow_attn_grad and mod.fused_mlp_func is None
    assert model.ffns[0].fused_mlp_func is seam.fused_mlp_func               # no model given: captured attributes untouched
    seam.install_train(mod, model)
    assert all(f.fused_mlp_func is None for f in model.ffns)
    assert not hasattr(model.other, "fused_mlp_func") and not hasattr(model, "fused_mlp_func")
    assert mod.memory_efficient_attention is sentinel and mod.flash_attn_func is sentinel


def test_install_train_after_install_on_real_modules():
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
    mod = types.SimpleNamespace()
    seam.install(mod, net)
    assert all(b.ffn.fused_mlp_func is seam.fused_mlp_func for b in net)
    seam.install_train(mod, net)
    assert all(b.ffn.fused_mlp_func is None for b in net) and mod.fused_mlp_func is None and mod.slow_attn is seam.slow_attn_grad


# ------------------------------------------------------------------------------------------------------------------ the inference slots keep refusing grad
def test_slow_attn_still_raises_under_grad():
    q, g = _qkv(), _qkv(grad=True)
    with torch.enable_grad():
        with pytest.raises(E.SdvarError, match="no backward exists"):
            seam.slow_attn(g, q, q, 1.0)


def test_fused_mlp_func_still_raises_under_grad():
    x, w2 = _Fake(torch.zeros(3, 64)), _Fake(torch.zeros(64, 256))
    wg = _Fake(torch.zeros(256, 64, requires_grad=True))
    with torch.enable_grad():
        with pytest.raises(E.SdvarError, match="no backward exists"):
            seam.fused_mlp_func(x, wg, w2)


# ------------------------------------------------------------------------------------------------------------------ slow_attn_grad: unsupported cases
def test_grad_slot_dropout():
    g = _qkv(grad=True)
    with pytest.raises(E.SdvarError, match="dropout"):
        seam.slow_attn_grad(g, g, g, 1.0, None, 0.1)
    with pytest.raises(E.SdvarError, match="dropout"):
        seam.memory_efficient_attention_grad(g, g, g, None, p=0.5)


def test_grad_slot_cpu_tensors():
    g = _qkv(grad=True)
    with pytest.raises(E.SdvarError, match="CPU"):
        seam.slow_attn_grad(torch.zeros(1, 2, 8, 64, requires_grad=True), g, g, 1.0)
    with pytest.raises(E.SdvarError, match="CPU"):
        seam.slow_attn_grad(g, g, torch.zeros(1, 2, 8, 64), 1.0)


@pytest.mark.parametrize("bad", [torch.float16, torch.bfloat16, torch.float64])
def test_grad_slot_dtypes(bad):
    g = _qkv(grad=True)
    with pytest.raises(E.SdvarError, match="float32"):
        seam.slow_attn_grad(_qkv(dtype=bad, grad=True), g, g, 1.0)
    with pytest.raises(E.SdvarError, match="float32"):
        seam.slow_attn_grad(g, g, _qkv(dtype=bad), 1.0)


@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16])
def test_grad_slot_half_operands_name_the_autocast_slots(half):
    with pytest.raises(E.SdvarError, match="autocast slots.*no backward"):
        seam.slow_attn_grad(_qkv(dtype=half, grad=True), _qkv(dtype=half), _qkv(dtype=half), 1.0)


def test_grad_slot_head_dim():
    with pytest.raises(E.SdvarError, match="head dim"):
        seam.slow_attn_grad(_qkv(c=32, grad=True), _qkv(c=32), _qkv(c=32), 1.0)
    with pytest.raises(E.SdvarError, match="head dim"):
        seam.memory_efficient_attention_grad(_qkv(c=128, grad=True), _qkv(c=128), _qkv(c=128))


def test_grad_slot_mismatched_shapes():
    g = _qkv(grad=True)
    with pytest.raises(E.SdvarError, match="shapes do not match"):
        seam.slow_attn_grad(g, _qkv(L=8), _qkv(L=9), 1.0)                 # key and value disagree
    with pytest.raises(E.SdvarError, match="shapes do not match"):
        seam.slow_attn_grad(g, _qkv(H=3), _qkv(H=3), 1.0)                 # another head count
    with pytest.raises(E.SdvarError, match="dims"):
        seam.slow_attn_grad(_Fake(torch.zeros(2, 8, 64, requires_grad=True)), g, g, 1.0)


def test_grad_slot_mask_requiring_grad():
    g = _qkv(grad=True)
    m = _Fake(torch.zeros(1, 1, 8, 8, requires_grad=True))
    with torch.enable_grad():
        with pytest.raises(E.SdvarError, match="mask requires grad"):
            seam.slow_attn_grad(g, g, g, 1.0, attn_mask=m)


def test_grad_slot_mask_key_dim_not_materialised():
    g = _qkv(grad=True)
    with torch.enable_grad():
        with pytest.raises(E.SdvarError, match="key dimension must be materialised"):
            seam.slow_attn_grad(g, g, g, 1.0, attn_mask=_Fake(torch.zeros(1, 1, 8, 1)))
    with pytest.raises(E.SdvarError, match="mask is a CPU tensor"):
        seam.slow_attn_grad(g, g, g, 1.0, attn_mask=torch.zeros(1, 1, 8, 8))


# ------------------------------------------------------------------------------------------------------------------ the C entry points
i64 = C.c_int64
_buf = (C.c_float * 64)()                                       # host memory: only its (aligned) address is looked at, every call returns before any HIP call
_base = (C.addressof(_buf) + 15) & ~15
P = C.c_void_p(_base)
MIS = C.c_void_p(_base + 4)
DENSE = [2 * 4 * 64, 4 * 64, 64]
BAD = [2 * 4 * 66, 4 * 66, 66]                                  # token stride 66 floats = 264 bytes
BS = (i64 * 3)(0, 0, 4)


def _lse(q=P, k=P, v=P, out=P, lse=P, strides=None, bias=None, kind=0, bs=None, smap=None, hd=64):
    lib = E.load_library()
    st = (i64 * 12)(*(strides or DENSE * 4))
    rc = lib.sdvar_op_sdpa_lse(q, k, v, out, lse, st, bias, kind, bs, smap, 1, 2, 4, 4, hd, 1.0, None)
    return rc, lib.sdvar_last_error()


def _bwd(q=P, k=P, v=P, out=P, dout=P, lse=P, delta=P, dq=P, dk=P, dv=P, strides=None, bias=None, kind=0, bs=None, smap=None, hd=64):
    lib = E.load_library()
    st = (i64 * 24)(*(strides or DENSE * 8))
    rc = lib.sdvar_op_sdpa_bwd(q, k, v, out, dout, lse, delta, dq, dk, dv, st, bias, kind, bs, smap, 1, 2, 4, 4, hd, 1.0, None)
    return rc, lib.sdvar_last_error()


@pytest.mark.parametrize("which", ["q", "k", "v", "out"])
def test_op_sdpa_lse_null_operand(which):
    rc, err = _lse(**{which: None})
    assert rc == 1 and b"null operand" in err


def test_op_sdpa_lse_null_lse():
    rc, err = _lse(lse=None)
    assert rc == 1 and b"null lse" in err


def test_op_sdpa_lse_stride_not_multiple_of_4():
    rc, err = _lse(strides=DENSE + BAD + DENSE * 2)
    assert rc == 1 and b"16-byte aligned" in err and b"k strides" in err


def test_op_sdpa_lse_misaligned_pointer():
    rc, err = _lse(v=MIS)
    assert rc == 1 and b"v is not 16-byte aligned" in err


def test_op_sdpa_lse_head_dim_32():
    rc, err = _lse(hd=32)
    assert rc == 1 and b"head dim 32" in err


def test_op_sdpa_lse_bias_kind_without_bias():
    rc, err = _lse(kind=1)
    assert rc == 1 and b"bias pointer and bias kind 1 disagree" in err


def test_op_sdpa_lse_skip_map_without_bias():
    rc, err = _lse(smap=P)
    assert rc == 1 and b"skip map needs a bias" in err


@pytest.mark.parametrize("which", ["q", "k", "v", "out", "dout"])
def test_op_sdpa_bwd_null_operand(which):
    rc, err = _bwd(**{which: None})
    assert rc == 1 and b"null operand" in err


def test_op_sdpa_bwd_null_lse():
    rc, err = _bwd(lse=None)
    assert rc == 1 and b"null lse" in err


def test_op_sdpa_bwd_null_workspace():
    rc, err = _bwd(delta=None)
    assert rc == 1 and b"null delta" in err


@pytest.mark.parametrize("slot,name", [(4, b"dout"), (6, b"dk")])
def test_op_sdpa_bwd_stride_not_multiple_of_4(slot, name):
    rc, err = _bwd(strides=DENSE * slot + BAD + DENSE * (7 - slot))
    assert rc == 1 and b"16-byte aligned" in err and name + b" strides" in err


def test_op_sdpa_bwd_strides_of_an_absent_gradient_are_ignored():
    rc, err = _bwd(dk=None, strides=DENSE * 6 + BAD + DENSE, kind=1)         # gets past the stride checks, stops at the next one (the bias)
    assert rc == 1 and b"bias pointer and bias kind 1 disagree" in err


@pytest.mark.parametrize("which,name", [("dout", b"dout"), ("dq", b"dq"), ("dv", b"dv")])
def test_op_sdpa_bwd_misaligned_pointer(which, name):
    rc, err = _bwd(**{which: MIS})
    assert rc == 1 and name + b" is not 16-byte aligned" in err


def test_op_sdpa_bwd_head_dim_32():
    rc, err = _bwd(hd=32)
    assert rc == 1 and b"head dim 32" in err


def test_op_sdpa_bwd_bias_kind_without_bias():
    rc, err = _bwd(kind=2)
    assert rc == 1 and b"bias pointer and bias kind 2 disagree" in err


def test_op_sdpa_bwd_skip_map_without_bias():
    rc, err = _bwd(smap=P)
    assert rc == 1 and b"skip map needs a bias" in err


def test_op_sdpa_bwd_no_gradient_requested():
    rc, err = _bwd(dq=None, dk=None, dv=None)
    assert rc == 1 and b"dq, dk and dv are all NULL" in err
