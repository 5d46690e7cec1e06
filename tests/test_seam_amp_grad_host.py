"""seam.slow_attn_amp_grad / memory_efficient_attention_amp_grad / flash_attn_func_grad / install_train_amp without a GPU: the new names are public and the library
exports sdvar_op_sdpa_hm_lse / sdvar_op_sdpa_h_bwd with the declared signatures, install_train_amp sets the slots a mixed-precision trainer needs, every unsupported
case raises SdvarError naming the function before the library is touched, with grad off the functions hand over to their inference twins, and the two C entries
report argument errors through sdvar_last_error before any HIP call."""
import ctypes as C
import types

import pytest
import torch

from sdvar_amd import engine as E
from sdvar_amd import seam

HALVES = [torch.float16, torch.bfloat16]


class _Fake(torch.Tensor):
    """A CPU tensor that reports is_cuda = True (the trick of tests/test_seam_host.py): the argument checks that come AFTER the device check run without a GPU.
    Nothing is ever launched on it: every case below must raise before the library is called."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)

    @property
    def is_cuda(self):
        return True


def _qkv(L=8, dtype=torch.float16, c=64, grad=False, H=2):
    return _Fake(torch.zeros(1, H, L, c, dtype=dtype, requires_grad=grad))


@pytest.fixture(autouse=True)
def _grad_mode_on():
    with torch.enable_grad():
        yield


def test_new_names_are_public_and_exported():
    for name in ("slow_attn_amp_grad", "memory_efficient_attention_amp_grad", "flash_attn_func_grad", "install_train_amp"):
        assert name in seam.__all__ and callable(getattr(seam, name))
    lib = E.load_library()
    for name, nargs in (("sdvar_op_sdpa_hm_lse", 20), ("sdvar_op_sdpa_h_bwd", 25)):
        assert name in E._SIGNATURES and hasattr(lib, name)
        restype, argtypes = E._SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == nargs
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)
    # the lse entry is sdvar_op_sdpa_hm's signature with one more pointer after `out`
    hm, lse = E._SIGNATURES["sdvar_op_sdpa_hm"][1], E._SIGNATURES["sdvar_op_sdpa_hm_lse"][1]
    assert list(lse) == list(hm[:4]) + [C.c_void_p] + list(hm[4:])


def test_abi_version_is_still_5():
    assert E.load_library().sdvar_abi_version() == 5 == E.ABI_VERSION


# ------------------------------------------------------------------------------------------------------------------ install_train_amp
class _FFN:
    def __init__(self, slot):
        self.fused_mlp_func = slot          # basic_var.py:36: the module global is captured at construction


class _Attn:
    def __init__(self):
        self.using_flash = False            # basic_var.py:81: decided at construction


class _Model:
    def __init__(self, slot):
        self.ffns = [_FFN(slot), _FFN(None)]
        self.attns = [_Attn(), _Attn()]
        self.other = types.SimpleNamespace(weight=1)

    def modules(self):
        return [self, self.other] + self.ffns + self.attns


@pytest.mark.parametrize("ffn", [False, True])
def test_install_train_amp_sets_the_slots(ffn):
    sentinel = object()
    mod = types.SimpleNamespace(slow_attn=object(), flash_attn_func=None, fused_mlp_func=seam.fused_mlp_func, memory_efficient_attention=sentinel)
    model = _Model(seam.fused_mlp_func)
    slot = seam.fused_mlp_func_grad if ffn else None
    seam.install_train_amp(mod, ffn=ffn)
    assert mod.slow_attn is seam.slow_attn_amp_grad and mod.flash_attn_func is seam.flash_attn_func_grad and mod.fused_mlp_func is slot
    assert model.ffns[0].fused_mlp_func is seam.fused_mlp_func and not model.attns[0].using_flash         # no model given: nothing of it is touched
    seam.install_train_amp(mod, model, ffn=ffn)
    assert all(f.fused_mlp_func is slot for f in model.ffns) and all(a.using_flash is True for a in model.attns)
    assert not hasattr(model.other, "fused_mlp_func") and not hasattr(model.other, "using_flash") and not hasattr(model, "using_flash")
    assert mod.memory_efficient_attention is sentinel
    assert set(vars(mod)) == {"slow_attn", "flash_attn_func", "fused_mlp_func", "memory_efficient_attention"}


@pytest.mark.parametrize("half", HALVES)
def test_ffn_slot_of_install_train_amp_raises_on_half_input(half):
    """ffn=True under autocast: fused_mlp_func_grad takes fp32 operands only and says so on a half x (the reference hands its FFN an fp32 x under autocast)."""
    mod = types.SimpleNamespace()
    seam.install_train_amp(mod, ffn=True)
    w1, w2 = _Fake(torch.zeros(256, 64, requires_grad=True)), _Fake(torch.zeros(64, 256))
    with pytest.raises(E.SdvarError, match="fused_mlp_func_grad: x is .*only float32"):
        mod.fused_mlp_func(_Fake(torch.zeros(3, 64, dtype=half)), w1, w2)


# ------------------------------------------------------------------------------------------------------------------ rejections
SLOTS = [("slow_attn_amp_grad", lambda q, k, v, **kw: seam.slow_attn_amp_grad(q, k, v, 1.0, **kw)),
         ("memory_efficient_attention_amp_grad", lambda q, k, v, attn_mask=None, **kw: seam.memory_efficient_attention_amp_grad(q, k, v, attn_bias=attn_mask, **kw))]


@pytest.mark.parametrize("name,fn", SLOTS)
def test_amp_grad_cpu_tensors(name, fn):
    g = _qkv(grad=True)
    with pytest.raises(E.SdvarError, match=f"^{name}: query is a CPU tensor"):
        fn(torch.zeros(1, 2, 8, 64, dtype=torch.float16, requires_grad=True), g, g)
    with pytest.raises(E.SdvarError, match=f"^{name}: value is a CPU tensor"):
        fn(g, g, torch.zeros(1, 2, 8, 64, dtype=torch.float16))
    with pytest.raises(E.SdvarError, match=f"^{name}: the mask is a CPU tensor"):
        fn(g, g, g, attn_mask=torch.zeros(1, 1, 8, 8) if name.startswith("slow") else torch.zeros(1, 1, 2, 2))


@pytest.mark.parametrize("name,fn", SLOTS)
def test_amp_grad_head_dim_and_dims(name, fn):
    with pytest.raises(E.SdvarError, match=f"^{name}: head dim 32"):
        fn(_qkv(c=32, grad=True), _qkv(c=32), _qkv(c=32))
    with pytest.raises(E.SdvarError, match=f"^{name}: query has 3 dims"):
        fn(_Fake(torch.zeros(2, 8, 64, dtype=torch.float16, requires_grad=True)), _qkv(), _qkv())
    with pytest.raises(E.SdvarError, match=f"^{name}: shapes do not match"):
        fn(_qkv(grad=True), _qkv(L=8), _qkv(L=9))


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("name,fn", SLOTS)
def test_amp_grad_dtype_combinations(name, fn, half):
    other = torch.bfloat16 if half == torch.float16 else torch.float16
    h, f = _qkv(dtype=half, grad=True), _qkv(dtype=torch.float32, grad=True)
    with pytest.raises(E.SdvarError, match=f"^{name}: value is torch.float32 next to"):
        fn(h, f, f)
    with pytest.raises(E.SdvarError, match=f"^{name}: value is torch.float32 next to"):
        fn(f, h, f)
    with pytest.raises(E.SdvarError, match=f"^{name}: mixed half dtypes: query"):
        fn(_qkv(dtype=other, grad=True), h, h)
    with pytest.raises(E.SdvarError, match=f"^{name}: mixed half dtypes: key"):
        fn(f, _qkv(dtype=other), h)
    with pytest.raises(E.SdvarError, match=f"^{name}: query is torch.float64"):
        fn(_qkv(dtype=torch.float64, grad=True), h, h)


@pytest.mark.parametrize("half", HALVES)
def test_amp_grad_masks(half):
    other = torch.bfloat16 if half == torch.float16 else torch.float16
    g = _qkv(dtype=half, grad=True)
    with pytest.raises(E.SdvarError, match="^slow_attn_amp_grad: the mask is .* but the operands are"):
        seam.slow_attn_amp_grad(g, g, g, 1.0, attn_mask=_Fake(torch.zeros(1, 1, 8, 8, dtype=other)))
    with pytest.raises(E.SdvarError, match="^slow_attn_amp_grad: the mask is torch.float64"):
        seam.slow_attn_amp_grad(g, g, g, 1.0, attn_mask=_Fake(torch.zeros(1, 1, 8, 8, dtype=torch.float64)))
    with pytest.raises(E.SdvarError, match="^slow_attn_amp_grad: the mask requires grad"):
        seam.slow_attn_amp_grad(g, g, g, 1.0, attn_mask=_Fake(torch.zeros(1, 1, 8, 8, requires_grad=True)))
    with pytest.raises(E.SdvarError, match="^memory_efficient_attention_amp_grad: the mask requires grad"):
        seam.memory_efficient_attention_amp_grad(g, g, g, attn_bias=_Fake(torch.zeros(1, 1, 2, 2, dtype=half, requires_grad=True)))
    with pytest.raises(E.SdvarError, match="^slow_attn_amp_grad: .*key dimension must be materialised"):
        seam.slow_attn_amp_grad(g, g, g, 1.0, attn_mask=_Fake(torch.zeros(1, 1, 8, 1)))


def test_amp_grad_dropout():
    g = _qkv(grad=True)
    with pytest.raises(E.SdvarError, match="^slow_attn_amp_grad: dropout"):
        seam.slow_attn_amp_grad(g, g, g, 1.0, None, 0.1)
    with pytest.raises(E.SdvarError, match=r"^memory_efficient_attention_amp_grad: p > 0 \(dropout\)"):
        seam.memory_efficient_attention_amp_grad(g, g, g, None, p=0.5)
    with pytest.raises(E.SdvarError, match="^flash_attn_func_grad: dropout_p > 0"):
        seam.flash_attn_func_grad(g, g, g, dropout_p=0.1)


@pytest.mark.parametrize("kw,msg", [({"causal": True}, "causal"), ({"window_size": (8, 0)}, "window_size"), ({"softcap": 30.0}, "softcap"),
                                    ({"alibi_slopes": torch.zeros(2)}, "alibi_slopes"), ({"return_attn_probs": True}, "return_attn_probs")])
def test_flash_grad_flash_only_arguments(kw, msg):
    g = _Fake(torch.zeros(1, 8, 2, 64, dtype=torch.float16, requires_grad=True))
    with pytest.raises(E.SdvarError, match=f"^flash_attn_func_grad: {msg}"):
        seam.flash_attn_func_grad(g, g, g, **kw)


def test_flash_grad_operands():
    g = _Fake(torch.zeros(1, 8, 2, 64, dtype=torch.float16, requires_grad=True))
    with pytest.raises(E.SdvarError, match="^flash_attn_func_grad: q is a CPU tensor"):
        seam.flash_attn_func_grad(torch.zeros(1, 8, 2, 64, dtype=torch.float16), g, g)
    with pytest.raises(E.SdvarError, match="^flash_attn_func_grad: k is torch.float32"):
        seam.flash_attn_func_grad(g, _Fake(torch.zeros(1, 8, 2, 64)), g)
    with pytest.raises(E.SdvarError, match="^flash_attn_func_grad: mixed dtypes"):
        seam.flash_attn_func_grad(g, g, _Fake(torch.zeros(1, 8, 2, 64, dtype=torch.bfloat16)))
    with pytest.raises(E.SdvarError, match="^flash_attn_func_grad: head dim 32"):
        seam.flash_attn_func_grad(*(_Fake(torch.zeros(1, 8, 2, 32, dtype=torch.float16, requires_grad=True)) for _ in range(3)))
    with pytest.raises(E.SdvarError, match="^flash_attn_func_grad: shapes do not match"):
        seam.flash_attn_func_grad(g, g, _Fake(torch.zeros(1, 9, 2, 64, dtype=torch.float16)))


@pytest.mark.parametrize("half", HALVES)
def test_wrong_dout_dtype_raises(half):
    ctx = types.SimpleNamespace(sdpa=((0, 1, 2), 1.0, 0, None, (1, 2, 8, 8), half, "slow_attn_amp_grad"), needs_input_grad=(True,) * 3 + (False,) * 5)
    with pytest.raises(E.SdvarError, match=f"^slow_attn_amp_grad: the gradient of the output is torch.float32 but the output is {half}"):
        seam._SdpaFn.backward(ctx, torch.zeros(1, 8, 2, 64))


# ------------------------------------------------------------------------------------------------------------------ the existing slots keep refusing grad
@pytest.mark.parametrize("half", HALVES)
def test_inference_slots_still_raise_under_grad(half):
    g, q = _qkv(dtype=half, grad=True), _qkv(dtype=half)
    with pytest.raises(E.SdvarError, match="^slow_attn_amp: query requires grad.*no backward exists"):
        seam.slow_attn_amp(g, q, q, 1.0)
    with pytest.raises(E.SdvarError, match="^memory_efficient_attention_amp: value requires grad.*no backward exists"):
        seam.memory_efficient_attention_amp(q, q, g)
    fg = _Fake(torch.zeros(1, 8, 2, 64, dtype=half, requires_grad=True))
    with pytest.raises(E.SdvarError, match="^flash_attn_func: q requires grad.*no backward exists"):
        seam.flash_attn_func(fg, fg, fg)
    with pytest.raises(E.SdvarError, match="^slow_attn_grad: .*autocast slots.*no backward"):
        seam.slow_attn_grad(g, q, q, 1.0)


# ------------------------------------------------------------------------------------------------------------------ delegation
def test_grad_off_delegates_to_the_inference_twin(monkeypatch):
    calls = []
    buf = torch.zeros(1, 8, 2, 64, dtype=torch.float16)
    monkeypatch.setattr(seam, "_sdpa_amp", lambda who, *a: calls.append(("amp", who)) or buf)
    monkeypatch.setattr(seam, "flash_attn_func", lambda q, k, v, softmax_scale=None: calls.append(("flash", softmax_scale)) or buf)
    g, q = _qkv(grad=True), _qkv()
    m = _Fake(torch.zeros(1, 1, 8, 8))
    with torch.no_grad():
        out = seam.slow_attn_amp_grad(g, g, g, 1.0, attn_mask=m)
    assert out.shape == (1, 2, 8, 64) and calls == [("amp", "slow_attn_amp_grad")]
    seam.slow_attn_amp_grad(q, _qkv(dtype=torch.float32), q, 1.0)            # grad mode on, nothing requires grad
    seam.memory_efficient_attention_amp_grad(q, q, q)
    assert calls[1:] == [("amp", "slow_attn_amp_grad"), ("amp", "memory_efficient_attention_amp_grad")]
    f = _Fake(torch.zeros(1, 8, 2, 64, dtype=torch.float16))
    assert seam.flash_attn_func_grad(f, f, f, softmax_scale=0.5) is buf and calls[-1] == ("flash", 0.5)
    with torch.no_grad():
        fg = _Fake(torch.zeros(1, 8, 2, 64, dtype=torch.float16, requires_grad=True))
        assert seam.flash_attn_func_grad(fg, fg, fg) is buf and calls[-1] == ("flash", None)


def test_three_fp32_operands_go_to_the_fp32_grad_path(monkeypatch):
    calls = []
    monkeypatch.setattr(seam, "_sdpa_grad", lambda who, q, k, v, idx, scale, mask: calls.append((who, idx, scale)) or torch.zeros(1, 8, 2, 64))
    g = _qkv(dtype=torch.float32, grad=True)
    seam.slow_attn_amp_grad(g, g, g, 0.25)
    seam.memory_efficient_attention_amp_grad(g, g, g, scale=0.5)
    assert calls == [("slow_attn_amp_grad", (0, 1, 2), 0.25), ("memory_efficient_attention_amp_grad", (0, 2, 1), 0.5)]


# ------------------------------------------------------------------------------------------------------------------ the C entry points
i64 = C.c_int64
_buf = (C.c_float * 64)()                                       # host memory: only its (aligned) address is looked at, every call returns before any HIP call
_base = (C.addressof(_buf) + 15) & ~15
P = C.c_void_p(_base)
MIS = C.c_void_p(_base + 4)
DENSE = [2 * 4 * 64, 4 * 64, 64]
BAD8 = [2 * 4 * 68, 4 * 68, 68]                                 # token stride 68 elements: fine for fp32 rows (272 bytes), not for half rows (136 bytes)
BAD4 = [2 * 4 * 66, 4 * 66, 66]                                 # token stride 66 floats = 264 bytes


def _lse(q=P, k=P, v=P, out=P, lse=P, strides=None, dtype=1, qf=0, kf=0, bias=None, kind=0, bs=None, smap=None, hd=64):
    lib = E.load_library()
    st = (i64 * 12)(*(strides or DENSE * 4))
    rc = lib.sdvar_op_sdpa_hm_lse(q, k, v, out, lse, st, dtype, qf, kf, bias, kind, bs, smap, 1, 2, 4, 4, hd, 1.0, None)
    return rc, lib.sdvar_last_error()


def _bwd(q=P, k=P, v=P, out=P, dout=P, lse=P, delta=P, dq=P, dk=P, dv=P, strides=None, dtype=1, qf=0, kf=0, bias=None, kind=0, bs=None, smap=None, hd=64):
    lib = E.load_library()
    st = (i64 * 24)(*(strides or DENSE * 8))
    rc = lib.sdvar_op_sdpa_h_bwd(q, k, v, out, dout, lse, delta, dq, dk, dv, st, dtype, qf, kf, bias, kind, bs, smap, 1, 2, 4, 4, hd, 1.0, None)
    return rc, lib.sdvar_last_error()


def test_op_sdpa_hm_lse_argument_errors():
    rc, err = _lse(lse=None)
    assert rc == 1 and b"sdpa_hm_lse: lse is NULL" in err
    rc, err = _lse(lse=C.c_void_p(_base + 2))
    assert rc == 1 and b"sdpa_hm_lse: lse is NULL or not 4-byte aligned" in err
    rc, err = _lse(v=None)
    assert rc == 1 and b"null operand" in err
    rc, err = _lse(dtype=3)
    assert rc == 1 and b"dtype 3" in err
    rc, err = _lse(hd=32)
    assert rc == 1 and b"head dim 32" in err
    rc, err = _lse(strides=DENSE + BAD8 + DENSE * 2)
    assert rc == 1 and b"k strides" in err and b"multiple of 8" in err
    rc, err = _lse(strides=DENSE + BAD8 + DENSE * 2, kf=1, kind=1)         # fp32 k: multiples of 4 pass; stops at the next check
    assert rc == 1 and b"bias pointer and bias kind 1 disagree" in err
    rc, err = _lse(smap=P)
    assert rc == 1 and b"skip map needs a bias" in err


@pytest.mark.parametrize("which", ["q", "k", "v", "out", "dout"])
def test_op_sdpa_h_bwd_null_operand(which):
    rc, err = _bwd(**{which: None})
    assert rc == 1 and b"sdpa_h_bwd: null operand" in err


def test_op_sdpa_h_bwd_argument_errors():
    rc, err = _bwd(lse=None)
    assert rc == 1 and b"sdpa_h_bwd: null lse" in err
    rc, err = _bwd(delta=None)
    assert rc == 1 and b"sdpa_h_bwd: null delta" in err
    rc, err = _bwd(dq=None, dk=None, dv=None)
    assert rc == 1 and b"dq, dk and dv are all NULL" in err
    rc, err = _bwd(dtype=0)
    assert rc == 1 and b"dtype 0" in err
    rc, err = _bwd(qf=2)
    assert rc == 1 and b"q_f32 = 2" in err
    rc, err = _bwd(hd=128)
    assert rc == 1 and b"head dim 128" in err
    rc, err = _bwd(kind=4, bias=P, bs=(i64 * 3)(0, 0, 4))
    assert rc == 1 and b"bias kind 4" in err
    rc, err = _bwd(kind=3)
    assert rc == 1 and b"bias pointer and bias kind 3 disagree" in err
    rc, err = _bwd(smap=P)
    assert rc == 1 and b"skip map needs a bias" in err


@pytest.mark.parametrize("slot,name", [(0, b"q"), (4, b"dout"), (6, b"dk"), (7, b"dv")])
def test_op_sdpa_h_bwd_half_strides_must_be_multiples_of_8(slot, name):
    rc, err = _bwd(strides=DENSE * slot + BAD8 + DENSE * (7 - slot))
    assert rc == 1 and b"16-byte aligned" in err and name + b" strides" in err and b"multiple of 8" in err


def test_op_sdpa_h_bwd_fp32_operands_and_their_gradients_use_multiples_of_4():
    # q and dq are fp32 with q_f32: a stride of 68 floats passes for both, 66 does not; the half tensors still need multiples of 8
    rc, err = _bwd(strides=BAD8 + DENSE * 4 + BAD8 + DENSE * 2, qf=1, kind=1)
    assert rc == 1 and b"bias pointer and bias kind 1 disagree" in err
    rc, err = _bwd(strides=DENSE * 5 + BAD4 + DENSE * 2, qf=1)
    assert rc == 1 and b"dq strides" in err and b"multiple of 4" in err
    rc, err = _bwd(strides=DENSE * 6 + BAD8 + DENSE, qf=1)
    assert rc == 1 and b"dk strides" in err and b"multiple of 8" in err


def test_op_sdpa_h_bwd_strides_of_an_absent_gradient_are_ignored():
    rc, err = _bwd(dk=None, strides=DENSE * 6 + BAD4 + DENSE, kind=1)        # gets past the stride checks, stops at the next one (the bias)
    assert rc == 1 and b"bias pointer and bias kind 1 disagree" in err


@pytest.mark.parametrize("which,name", [("dout", b"dout"), ("dq", b"dq"), ("dv", b"dv")])
def test_op_sdpa_h_bwd_misaligned_pointer(which, name):
    rc, err = _bwd(**{which: MIS})
    assert rc == 1 and name + b" is not 16-byte aligned" in err
