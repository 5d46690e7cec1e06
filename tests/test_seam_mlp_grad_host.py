"""seam.fused_mlp_func_grad / install_train(ffn=True) without a GPU: the new name is public, install_train sets the FFN slots on request and keeps its default, every
argument error of fused_mlp_func (plus out_features % 32 under grad) is raised before the library is touched, and the operand producers of csrc/mlp_bwd.hip report
argument errors through sdvar_last_error before any HIP call."""
import ctypes as C
import types

import pytest
import torch

from sdvar_amd import engine as E
from sdvar_amd import seam


class _Fake(torch.Tensor):
    """A CPU tensor that reports is_cuda = True (the trick of tests/test_seam_host.py).  Nothing is ever launched on it: every case below must raise first."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)

    @property
    def is_cuda(self):
        return True


def _ops(Cin=64, hid=256, Cout=64, rows=3, grad=True, dtype=torch.float32):
    return (_Fake(torch.zeros(rows, Cin, dtype=dtype, requires_grad=grad)), _Fake(torch.zeros(hid, Cin, dtype=dtype, requires_grad=grad)),
            _Fake(torch.zeros(Cout, hid, dtype=dtype, requires_grad=grad)))


def test_new_name_is_public():
    assert "fused_mlp_func_grad" in seam.__all__ and callable(seam.fused_mlp_func_grad)
    lib = E.load_library()
    for name in ("sdvar_op_transpose_operand", "sdvar_op_gelu_operand", "sdvar_op_gelu_bwd", "sdvar_op_colsum", "sdvar_op_scale_pair"):
        assert name in E._SIGNATURES and hasattr(lib, name)
    assert lib.sdvar_abi_version() == 5 == E.ABI_VERSION                # additive entry points: no bump


class _FFN:
    def __init__(self, slot):
        self.fused_mlp_func = slot          # basic_var.py:36: the module global is captured at construction


class _Model:
    def __init__(self, slot):
        self.ffns = [_FFN(slot), _FFN(slot), _FFN(None)]
        self.other = types.SimpleNamespace(weight=1)

    def modules(self):
        return [self, self.other] + self.ffns


def test_install_train_ffn_sets_the_slots():
    sentinel = object()
    mod = types.SimpleNamespace(slow_attn=object(), fused_mlp_func=None, memory_efficient_attention=sentinel, flash_attn_func=sentinel)
    model = _Model(seam.fused_mlp_func)
    seam.install_train(mod, ffn=True)
    assert mod.slow_attn is seam.slow_attn_grad and mod.fused_mlp_func is seam.fused_mlp_func_grad
    assert model.ffns[0].fused_mlp_func is seam.fused_mlp_func               # no model given: captured attributes untouched
    seam.install_train(mod, model, ffn=True)
    assert all(f.fused_mlp_func is seam.fused_mlp_func_grad for f in model.ffns)
    assert not hasattr(model.other, "fused_mlp_func") and not hasattr(model, "fused_mlp_func")
    assert mod.memory_efficient_attention is sentinel and mod.flash_attn_func is sentinel


def test_install_train_default_still_sets_none():
    mod = types.SimpleNamespace()
    model = _Model(seam.fused_mlp_func_grad)
    seam.install_train(mod, model)
    assert mod.fused_mlp_func is None and all(f.fused_mlp_func is None for f in model.ffns)
    seam.install_train(mod, model, ffn=False)
    assert mod.fused_mlp_func is None and all(f.fused_mlp_func is None for f in model.ffns)


@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("kwargs,match", [(dict(activation="relu"), "activation"), (dict(return_residual=True), "return_residual"),
                                          (dict(process_group=object()), "process group")])
def test_unsupported_arguments_raise_like_the_inference_twin(grad, kwargs, match):
    x, w1, w2 = _ops(grad=grad)
    with torch.enable_grad():
        for fn in (seam.fused_mlp_func_grad,) + (() if grad else (seam.fused_mlp_func,)):
            with pytest.raises(E.SdvarError, match=match):
                fn(x, w1, w2, **kwargs)


def test_shape_errors():
    with torch.enable_grad():
        x, w1, w2 = _ops()
        with pytest.raises(E.SdvarError, match="shapes do not chain"):
            seam.fused_mlp_func_grad(x, w1, _Fake(torch.zeros(64, 128)))
        with pytest.raises(E.SdvarError, match="shapes do not chain"):
            seam.fused_mlp_func_grad(_Fake(torch.zeros(3, 32)), w1, w2)
        with pytest.raises(E.SdvarError, match="multiples of 32"):
            seam.fused_mlp_func_grad(*_ops(Cin=48))
        with pytest.raises(E.SdvarError, match="multiples of 32"):
            seam.fused_mlp_func_grad(*_ops(hid=80))
        with pytest.raises(E.SdvarError, match="bias1 has shape"):
            seam.fused_mlp_func_grad(x, w1, w2, bias1=_Fake(torch.zeros(64)))


def test_out_features_must_be_a_multiple_of_32_under_grad():
    with torch.enable_grad():
        with pytest.raises(E.SdvarError, match="out_features 48"):
            seam.fused_mlp_func_grad(*_ops(Cout=48))


@pytest.mark.parametrize("bad", [torch.float16, torch.bfloat16, torch.float64])
def test_dtypes(bad):
    x, w1, w2 = _ops()
    with torch.enable_grad():
        with pytest.raises(E.SdvarError, match="float32"):
            seam.fused_mlp_func_grad(_ops(dtype=bad)[0], w1, w2)
        with pytest.raises(E.SdvarError, match="float32"):
            seam.fused_mlp_func_grad(x, w1, w2, bias2=_Fake(torch.zeros(64, dtype=bad)))


def test_cpu_tensors_raise():
    x, w1, w2 = _ops()
    with torch.enable_grad():
        with pytest.raises(E.SdvarError, match="CPU"):
            seam.fused_mlp_func_grad(torch.zeros(3, 64, requires_grad=True), w1, w2)
        with pytest.raises(E.SdvarError, match="CPU"):
            seam.fused_mlp_func_grad(x, w1, torch.zeros(64, 256))
        with pytest.raises(E.SdvarError, match="CPU"):
            seam.fused_mlp_func_grad(x, w1, w2, bias1=torch.zeros(256))
    with pytest.raises(E.SdvarError, match="not a tensor"):
        seam.fused_mlp_func_grad(x, [1.0], w2)


def test_inference_twin_still_refuses_grad():
    x, w1, w2 = _ops()
    with torch.enable_grad():
        with pytest.raises(E.SdvarError, match="no backward exists"):
            seam.fused_mlp_func(x, w1, w2)


# ------------------------------------------------------------------------------------------------------------------ the C entry points
_buf = (C.c_float * 64)()                                       # host memory: only its (aligned) address is looked at, every call returns before any HIP call
_base = (C.addressof(_buf) + 15) & ~15
P = C.c_void_p(_base)
MIS = C.c_void_p(_base + 4)


def _err(rc):
    return rc, E.load_library().sdvar_last_error()


def test_op_transpose_operand_argument_errors():
    lib = E.load_library()
    rc, err = _err(lib.sdvar_op_transpose_operand(P, 36, 4, 36, 0, P, 0, None, None))
    assert rc == 1 and b"cols % 8" in err
    rc, err = _err(lib.sdvar_op_transpose_operand(P, 32, 4, 32, 1, P, 0, None, None))
    assert rc == 1 and b"format 1" in err
    rc, err = _err(lib.sdvar_op_transpose_operand(P, 32, 4, 32, 3, P, 1024, P, None))            # a scale with bf16x3 planes
    assert rc == 1 and b"scale goes with 2 only" in err
    rc, err = _err(lib.sdvar_op_transpose_operand(MIS, 32, 4, 32, 0, P, 0, None, None))
    assert rc == 1 and b"16-byte aligned" in err
    rc, err = _err(lib.sdvar_op_transpose_operand(P, 32, 33, 32, 2, P, 32 * 32, None, None))     # 33 rows pad to 64: the plane stride must hold 32 x 64
    assert rc == 1 and b"plane stride" in err
    rc, err = _err(lib.sdvar_op_transpose_operand(None, 32, 4, 32, 0, P, 0, None, None))
    assert rc == 1


def test_op_gelu_argument_errors():
    lib = E.load_library()
    rc, err = _err(lib.sdvar_op_gelu_operand(P, 4, 48, 0, 0, P, 0, None))
    assert rc == 1 and b"N % 32" in err
    rc, err = _err(lib.sdvar_op_gelu_operand(P, 4, 32, 2, 1, P, 64, None))
    assert rc == 1 and b"plane stride" in err
    rc, err = _err(lib.sdvar_op_gelu_bwd(P, P, 4, 32, 0, 0, None, None, 0, None, 0, None, 0, None, None))
    assert rc == 1 and b"no output" in err
    rc, err = _err(lib.sdvar_op_gelu_bwd(None, P, 4, 32, 0, 0, None, P, 0, None, 0, None, 0, None, None))
    assert rc == 1 and b"need dh" in err
    rc, err = _err(lib.sdvar_op_gelu_bwd(P, P, 4, 32, 3, 0, P, P, 128, None, 0, None, 0, None, None))
    assert rc == 1 and b"scale goes with format 2" in err
    rc, err = _err(lib.sdvar_op_gelu_bwd(P, P, 4, 32, 2, 1, None, None, 0, P, 32 * 16, None, 0, None, None))        # 4 rows pad to 32: 32 x 32 per plane
    assert rc == 1 and b"plane stride" in err
    rc, err = _err(lib.sdvar_op_gelu_bwd(P, MIS, 4, 32, 0, 0, None, P, 0, None, 0, None, 0, None, None))
    assert rc == 1 and b"16-byte aligned" in err


def test_op_colsum_and_scale_pair_argument_errors():
    lib = E.load_library()
    rc, err = _err(lib.sdvar_op_colsum(P, 6, 4, 6, P, None))
    assert rc == 1 and b"N % 4" in err
    rc, err = _err(lib.sdvar_op_colsum(MIS, 8, 4, 8, P, None))
    assert rc == 1 and b"16-byte aligned" in err
    rc, err = _err(lib.sdvar_op_scale_pair(None, 0, None, 0, None, None))
    assert rc == 1 and b"null scale" in err
