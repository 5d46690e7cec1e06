"""seam.fused_mlp_func_amp / fused_mlp_func_amp_grad and their installers without a GPU: the two names are public, install_amp(ffn_half=True) and
install_train_amp(ffn="half") set the module slot and every captured ffn.fused_mlp_func while the defaults and ffn=True set what they always set, every refusal is
raised before the library is touched (the fake tensors below could not survive a launch), and the C entry points of csrc/gemm_half.hip and csrc/mlp_half.hip report
argument errors through sdvar_last_error before any HIP call."""
import ctypes as C
import types
import warnings

import pytest
import torch

from sdvar_amd import engine as E
from sdvar_amd import seam

AMP = (seam.fused_mlp_func_amp, seam.fused_mlp_func_amp_grad)


class _Fake(torch.Tensor):
    """A CPU tensor that reports is_cuda = True (the trick of tests/test_seam_host.py).  Nothing is ever launched on it: every case below must raise first."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)

    @property
    def is_cuda(self):
        return True


def _ops(Cin=64, hid=256, Cout=64, rows=3, grad=False, dtype=torch.float16, wdtype=torch.float32):
    return (_Fake(torch.zeros(rows, Cin, dtype=dtype, requires_grad=grad)), _Fake(torch.zeros(hid, Cin, dtype=wdtype, requires_grad=grad)),
            _Fake(torch.zeros(Cout, hid, dtype=wdtype, requires_grad=grad)))


@pytest.fixture(autouse=True)
def _library_untouched(monkeypatch):
    """Every refusal comes before the library: loading it from seam is an error in this file's seam-level tests (the C-level tests call E.load_library themselves)."""
    def boom(*a, **k):
        raise AssertionError("the library was touched before the argument error")
    monkeypatch.setattr(seam.E, "_stream", boom)


def test_new_names_are_public():
    for name in ("fused_mlp_func_amp", "fused_mlp_func_amp_grad"):
        assert name in seam.__all__ and callable(getattr(seam, name))
    lib = E.load_library()
    for name in ("sdvar_op_gemm_h", "sdvar_op_half_operand", "sdvar_op_gelu_bwd_h"):
        assert name in E._SIGNATURES and hasattr(lib, name)
    assert lib.sdvar_abi_version() == 5 == E.ABI_VERSION                # additive entry points: no bump


class _FFN:
    def __init__(self, slot):
        self.fused_mlp_func = slot          # basic_var.py:36: the module global is captured at construction


class _Attn:
    using_flash = False


class _Model:
    def __init__(self, slot):
        self.ffns = [_FFN(slot), _FFN(slot), _FFN(None)]
        self.attn = _Attn()
        self.other = types.SimpleNamespace(weight=1)

    def modules(self):
        return [self, self.other, self.attn] + self.ffns


def test_install_amp_ffn_half_sets_the_slots():
    mod, model = types.SimpleNamespace(), _Model(None)
    seam.install_amp(mod, model, ffn_half=True)
    assert mod.fused_mlp_func is seam.fused_mlp_func_amp and all(f.fused_mlp_func is seam.fused_mlp_func_amp for f in model.ffns)
    assert mod.slow_attn is seam.slow_attn_amp and mod.flash_attn_func is seam.flash_attn_func and model.attn.using_flash is True
    assert not hasattr(model.other, "fused_mlp_func") and not hasattr(model, "fused_mlp_func")
    mod2, model2 = types.SimpleNamespace(), _Model(None)
    seam.install_amp(mod2, ffn_half=True)                                 # no model given: captured attributes untouched
    assert mod2.fused_mlp_func is seam.fused_mlp_func_amp and all(f.fused_mlp_func is None for f in model2.ffns)


def test_install_amp_default_is_unchanged():
    for kw in ({}, dict(ffn_half=False)):
        mod, model = types.SimpleNamespace(), _Model(None)
        seam.install_amp(mod, model, **kw)
        assert mod.fused_mlp_func is seam.fused_mlp_func and all(f.fused_mlp_func is seam.fused_mlp_func for f in model.ffns)
        assert mod.slow_attn is seam.slow_attn_amp and mod.flash_attn_func is seam.flash_attn_func


def test_install_train_amp_ffn_half_sets_the_slots():
    sentinel = object()
    mod, model = types.SimpleNamespace(memory_efficient_attention=sentinel), _Model(seam.fused_mlp_func)
    seam.install_train_amp(mod, ffn="half")
    assert mod.fused_mlp_func is seam.fused_mlp_func_amp_grad and model.ffns[0].fused_mlp_func is seam.fused_mlp_func
    seam.install_train_amp(mod, model, ffn="half")
    assert mod.fused_mlp_func is seam.fused_mlp_func_amp_grad and all(f.fused_mlp_func is seam.fused_mlp_func_amp_grad for f in model.ffns)
    assert mod.slow_attn is seam.slow_attn_amp_grad and mod.flash_attn_func is seam.flash_attn_func_grad and model.attn.using_flash is True
    assert mod.memory_efficient_attention is sentinel
    with pytest.raises(E.SdvarError, match="expected False, True or 'half'"):
        seam.install_train_amp(mod, model, ffn="bf16")


def test_install_train_amp_false_and_true_are_unchanged():
    for kw, slot in (({}, None), (dict(ffn=False), None), (dict(ffn=True), seam.fused_mlp_func_grad)):
        mod, model = types.SimpleNamespace(), _Model(seam.fused_mlp_func)
        seam.install_train_amp(mod, model, **kw)
        assert mod.fused_mlp_func is slot and all(f.fused_mlp_func is slot for f in model.ffns)
        assert mod.slow_attn is seam.slow_attn_amp_grad and mod.flash_attn_func is seam.flash_attn_func_grad


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("fn", AMP)
@pytest.mark.parametrize("kwargs,match", [(dict(activation="relu"), "activation"), (dict(return_residual=True), "return_residual"),
                                          (dict(process_group=object()), "process group")])
def test_unsupported_arguments_raise_like_the_fp32_twin(fn, kwargs, match):
    with pytest.raises(E.SdvarError, match=match):
        fn(*_ops(), **kwargs)


@pytest.mark.parametrize("fn", AMP)
def test_fp32_x_outside_autocast_points_to_the_fp32_slots(fn):
    assert not torch.is_autocast_enabled()
    with pytest.raises(E.SdvarError, match="fused_mlp_func") as ei:
        fn(*_ops(dtype=torch.float32))
    assert "autocast" in str(ei.value)
    assert ("fused_mlp_func_grad" in str(ei.value)) == (fn is seam.fused_mlp_func_amp_grad)


@pytest.mark.parametrize("fn", AMP)
def test_autocast_with_a_cpu_tensor_raises(fn):
    x, w1, w2 = _ops()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                  # without a GPU torch warns that it disables the context; the CPU refusal comes first either way
        with torch.autocast("cuda", dtype=torch.float16):
            with pytest.raises(E.SdvarError, match="CPU"):
                fn(torch.zeros(3, 64), w1, w2)
            with pytest.raises(E.SdvarError, match="CPU"):
                fn(x, w1, torch.zeros(64, 256))
            with pytest.raises(E.SdvarError, match="CPU"):
                fn(x, w1, w2, bias1=torch.zeros(256))
    with pytest.raises(E.SdvarError, match="not a tensor"):
        fn(x, [1.0], w2)


@pytest.mark.parametrize("fn", AMP)
def test_autocast_dtype_is_used_for_an_fp32_x(fn, monkeypatch):
    """With autocast reported as enabled for the GPU, a float32 x passes the dtype rule (the next refusal is reached) and a weight of the OTHER half dtype is named."""
    monkeypatch.setattr(seam, "_autocast_gpu_dtype", lambda: torch.bfloat16)
    with pytest.raises(E.SdvarError, match="mixed half dtypes: weight1 is torch.float16"):
        fn(*_ops(dtype=torch.float32, wdtype=torch.float16))
    monkeypatch.setattr(seam, "_autocast_gpu_dtype", lambda: torch.float32)          # an autocast dtype that is no half dtype is no half dtype
    with pytest.raises(E.SdvarError, match="no half dtype"):
        fn(*_ops(dtype=torch.float32))


@pytest.mark.parametrize("fn", AMP)
def test_dtype_refusals(fn):
    x, w1, w2 = _ops()
    with pytest.raises(E.SdvarError, match="mixed half dtypes"):
        fn(x, _ops(wdtype=torch.bfloat16)[1], w2)
    with pytest.raises(E.SdvarError, match="mixed half dtypes"):
        fn(x, w1, w2, bias2=_Fake(torch.zeros(64, dtype=torch.bfloat16)))
    with pytest.raises(E.SdvarError, match="float64"):
        fn(_ops(dtype=torch.float64)[0], w1, w2)
    with pytest.raises(E.SdvarError, match="float64"):
        fn(x, w1, _ops(wdtype=torch.float64)[2])
    with pytest.raises(E.SdvarError, match="float64"):
        fn(x, w1, w2, bias1=_Fake(torch.zeros(256, dtype=torch.float64)))


@pytest.mark.parametrize("fn", AMP)
def test_shape_errors(fn):
    x, w1, w2 = _ops()
    with pytest.raises(E.SdvarError, match="shapes do not chain"):
        fn(x, w1, _Fake(torch.zeros(64, 128)))
    with pytest.raises(E.SdvarError, match="shapes do not chain"):
        fn(_Fake(torch.zeros(3, 32, dtype=torch.float16)), w1, w2)
    with pytest.raises(E.SdvarError, match="multiples of 32"):
        fn(*_ops(Cin=48))
    with pytest.raises(E.SdvarError, match="multiples of 32"):
        fn(*_ops(hid=80))
    with pytest.raises(E.SdvarError, match="multiple of 8"):
        fn(*_ops(Cout=36))
    with pytest.raises(E.SdvarError, match="bias1 has shape"):
        fn(x, w1, w2, bias1=_Fake(torch.zeros(64)))


def test_out_features_must_be_a_multiple_of_32_under_grad():
    with torch.enable_grad():
        with pytest.raises(E.SdvarError, match="out_features 40"):
            seam.fused_mlp_func_amp_grad(*_ops(Cout=40, grad=True))


def test_inference_twin_refuses_grad():
    with torch.enable_grad():
        with pytest.raises(E.SdvarError, match="no backward exists"):
            seam.fused_mlp_func_amp(*_ops(grad=True))


# ------------------------------------------------------------------------------------------------------------------ the C entry points
_buf = (C.c_float * 64)()                                       # host memory: only its (aligned) address is looked at, every call returns before any HIP call
_base = (C.addressof(_buf) + 15) & ~15
P = C.c_void_p(_base)
MIS = C.c_void_p(_base + 4)


def _err(rc):
    return rc, E.load_library().sdvar_last_error()


def test_op_gemm_h_argument_errors():
    lib = E.load_library()
    ok = dict(x=P, w=P, dtype=1, bias=None, out=P, out_dtype=0, ldo=64, h=None, p=None, M=4, N=64, K=32, epi=0)

    def call(**kw):
        a = dict(ok, **kw)
        return _err(lib.sdvar_op_gemm_h(a["x"], a["w"], a["dtype"], a["bias"], a["out"], a["out_dtype"], a["ldo"], a["h"], a["p"], a["M"], a["N"], a["K"], a["epi"], None))
    for kw, msg in ((dict(dtype=0), b"dtype 0"), (dict(dtype=3), b"dtype 3"), (dict(epi=2), b"epilogue 2"), (dict(x=None), b"null operand"), (dict(w=None), b"null operand"),
                    (dict(K=48), b"K % 32"), (dict(K=0), b"K % 32"), (dict(N=36), b"N % 8"), (dict(M=0), b"M >= 1"), (dict(x=MIS), b"16-byte aligned"),
                    (dict(w=MIS), b"16-byte aligned"), (dict(bias=MIS), b"16-byte aligned"), (dict(out=MIS), b"16-byte aligned"), (dict(out=None), b"writes `out`"),
                    (dict(h=P), b"writes `out` only"), (dict(out_dtype=2), b"out_dtype 2"), (dict(ldo=32), b"ldo"), (dict(ldo=66), b"ldo"),
                    (dict(epi=1, out=None), b"writes h_out"), (dict(epi=1, h=P), b"not `out`"), (dict(epi=1, out=None, h=P, N=40), b"N % 32"),
                    (dict(epi=1, out=None, h=MIS), b"16-byte aligned"), (dict(epi=1, out=None, h=P, p=MIS), b"16-byte aligned")):
        rc, err = call(**kw)
        assert rc == 1 and msg in err, (kw, err)


def test_op_half_operand_argument_errors():
    lib = E.load_library()
    for args, msg in (((P, 0, 32, 4, 32, 0, 0, P, None), b"dtype 0"), ((P, 2, 32, 4, 32, 1, 0, P, None), b"input dtype 2"), ((P, 0, 32, 4, 32, 1, 2, P, None), b"transpose 2"),
                      ((None, 0, 32, 4, 32, 1, 0, P, None), b"null input"), ((P, 0, 32, 4, 32, 1, 0, None, None), b"no output"), ((P, 0, 32, 4, 32, 1, 1, None, None), b"no output"),
                      ((P, 0, 32, 4, 32, 1, 0, P, P), b"transposed form only"), ((P, 0, 40, 4, 40, 1, 0, P, None), b"cols % 32"), ((P, 0, 36, 4, 36, 1, 1, P, None), b"cols % 8"),
                      ((P, 0, 34, 4, 32, 1, 0, P, None), b"ldx"), ((P, 1, 36, 4, 32, 1, 0, P, None), b"ldx % 8"), ((P, 0, 16, 4, 32, 1, 0, P, None), b"ldx"),
                      ((MIS, 0, 32, 4, 32, 1, 0, P, None), b"16-byte aligned"), ((P, 0, 32, 4, 32, 1, 0, MIS, None), b"16-byte aligned")):
        rc, err = _err(lib.sdvar_op_half_operand(*args, None))
        assert rc == 1 and msg in err, (args, err)


def test_op_gelu_bwd_h_argument_errors():
    lib = E.load_library()
    for args, msg in (((P, P, 4, 32, 0, P, None, None, None), b"dtype 0"), ((P, None, 4, 32, 1, P, None, None, None), b"pre-activation"),
                      ((P, P, 4, 48, 1, P, None, None, None), b"N % 32"), ((P, P, 4, 32, 1, None, None, None, None), b"no output"),
                      ((None, P, 4, 32, 1, P, None, None, None), b"need dh"), ((None, P, 4, 32, 2, None, None, None, P), b"need dh"),
                      ((P, MIS, 4, 32, 1, P, None, None, None), b"16-byte aligned"), ((P, P, 4, 32, 1, None, MIS, None, None), b"16-byte aligned")):
        rc, err = _err(lib.sdvar_op_gelu_bwd_h(*args, None))
        assert rc == 1 and msg in err, (args, err)
