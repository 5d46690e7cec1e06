"""seam.flash_attn_func / seam.enable_flash without a GPU: every unsupported case raises SdvarError before any kernel is touched, sdvar_op_sdpa_h reports argument
errors through sdvar_last_error before any device work, enable_flash sets the module slot and the using_flash flags (and only those), and install() keeps its
hands off flash_attn_func."""
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


def _t(L=8, dtype=torch.float16, c=64, B=1, H=2, grad=False):
    return _Fake(torch.zeros(B, L, H, c, dtype=dtype, requires_grad=grad))


def test_exported_names():
    assert "flash_attn_func" in seam.__all__ and "enable_flash" in seam.__all__


@pytest.mark.parametrize("kwargs, match", [
    (dict(dropout_p=0.1), "dropout"),
    (dict(causal=True), "causal"),
    (dict(window_size=(128, 0)), "window_size"),
    (dict(window_size=(-1, 0)), "window_size"),
    (dict(softcap=30.0), "softcap"),
    (dict(alibi_slopes=torch.zeros(2)), "alibi"),
    (dict(return_attn_probs=True), "return_attn_probs"),
])
def test_option_refusals(kwargs, match):
    q = _t()
    with pytest.raises(E.SdvarError, match=match):
        seam.flash_attn_func(q, q, q, **kwargs)


def test_operand_refusals():
    for dt in (torch.float16, torch.bfloat16):
        q = _t(dtype=dt)
        with pytest.raises(E.SdvarError, match="CPU"):
            seam.flash_attn_func(torch.zeros(1, 8, 2, 64, dtype=dt), q, q)
        with pytest.raises(E.SdvarError, match="CPU"):
            seam.flash_attn_func(q, q, torch.zeros(1, 8, 2, 64, dtype=dt))
    q = _t()
    f32 = _t(dtype=torch.float32)
    with pytest.raises(E.SdvarError, match="float32.*slow_attn.*memory_efficient_attention"):
        seam.flash_attn_func(f32, f32, f32)
    with pytest.raises(E.SdvarError, match="float32"):
        seam.flash_attn_func(q, f32, q)                                             # the reference's mixed case: fp32 normalised q / k next to a half v
    f64 = _t(dtype=torch.float64)
    with pytest.raises(E.SdvarError, match="float64"):
        seam.flash_attn_func(f64, f64, f64)
    with pytest.raises(E.SdvarError, match="mixed dtypes"):
        seam.flash_attn_func(q, _t(dtype=torch.bfloat16), q)
    with pytest.raises(E.SdvarError, match="mixed dtypes"):
        seam.flash_attn_func(_t(dtype=torch.bfloat16), _t(dtype=torch.bfloat16), q)
    with pytest.raises(E.SdvarError, match="head dim 32"):
        seam.flash_attn_func(_t(c=32), _t(c=32), _t(c=32))
    with pytest.raises(E.SdvarError, match="head dim 128"):
        seam.flash_attn_func(_t(c=128), _t(c=128), _t(c=128))
    with pytest.raises(E.SdvarError, match="dims"):
        seam.flash_attn_func(_Fake(torch.zeros(8, 2, 64, dtype=torch.float16)), q, q)
    with pytest.raises(E.SdvarError, match="shapes do not match"):
        seam.flash_attn_func(q, _t(L=5), _t(L=6))                                   # k and v disagree
    with pytest.raises(E.SdvarError, match="shapes do not match"):
        seam.flash_attn_func(q, _t(H=3), _t(H=3))                                   # heads
    with pytest.raises(E.SdvarError, match="shapes do not match"):
        seam.flash_attn_func(q, _t(B=2), _t(B=2))                                   # batch
    with pytest.raises(E.SdvarError, match="shapes do not match"):
        seam.flash_attn_func(_t(L=0), q, q)
    g = _t(grad=True)
    assert g.requires_grad
    with torch.enable_grad():
        with pytest.raises(E.SdvarError, match="grad"):
            seam.flash_attn_func(g, q, q)
        with pytest.raises(E.SdvarError, match="grad"):
            seam.flash_attn_func(q, q, g)


def test_fp32_slots_still_refuse_half_operands():
    """The new slot changes nothing about the others: under autocast the masked calls (mixed / half dtypes into slow_attn) still raise."""
    q = _Fake(torch.zeros(1, 2, 8, 64, dtype=torch.float16))
    with pytest.raises(E.SdvarError, match="float32"):
        seam.slow_attn(q, q, q, 1.0)
    with pytest.raises(E.SdvarError, match="float32"):
        seam.memory_efficient_attention(q, q, q)


def test_op_sdpa_h_argument_errors_without_gpu():
    lib = E.load_library()
    i64 = C.c_int64
    buf = (C.c_uint16 * 128)()                                      # host memory: only its (aligned) address is looked at, the call returns before any HIP call
    base = (C.addressof(buf) + 15) & ~15
    p = C.c_void_p(base)
    dense = [4 * 2 * 64, 64, 2 * 64]                                # (batch, head, token) strides of a (1, 4, 2, 64) tensor
    ok = (i64 * 12)(*(dense * 4))

    def call(q=p, k=p, v=p, out=p, strides=ok, dtype=1, B=1, H=2, Lq=4, Lk=4, hd=64):
        rc = lib.sdvar_op_sdpa_h(q, k, v, out, strides, dtype, B, H, Lq, Lk, hd, 0.125, None)
        return rc, lib.sdvar_last_error()

    rc, err = call(q=None)
    assert rc == 1 and b"null operand" in err
    rc, err = call(out=None)
    assert rc == 1 and b"null operand" in err
    rc, err = call(q=C.c_void_p(base + 2))
    assert rc == 1 and b"q is not 16-byte aligned" in err
    rc, err = call(out=C.c_void_p(base + 2))
    assert rc == 1 and b"out is not 16-byte aligned" in err
    for which, name in ((0, b"q"), (1, b"k"), (2, b"v"), (3, b"out")):
        s = dense * 4
        s[3 * which + 2] = 4                                        # token stride 4 elements = 8 bytes
        rc, err = call(strides=(i64 * 12)(*s))
        assert rc == 1 and name + b" strides" in err and b"multiple of 8" in err
    s = dense * 4
    s[1] = -64
    rc, err = call(strides=(i64 * 12)(*s))
    assert rc == 1 and b"q strides" in err
    for bad in (0, 3):
        rc, err = call(dtype=bad)
        assert rc == 1 and b"dtype %d" % bad in err
    rc, err = call(hd=32)
    assert rc == 1 and b"head dim 32" in err
    for kw in (dict(B=0), dict(H=0), dict(Lq=0), dict(Lk=0)):
        rc, err = call(**kw)
        assert rc == 1 and b"bad extents" in err


class _Attn:
    def __init__(self):
        self.using_flash = False
        self.using_xform = False
        self.fused_mlp_func = None


class _Model:
    def __init__(self):
        self.attns = [_Attn(), _Attn()]
        self.other = types.SimpleNamespace(weight=1)

    def modules(self):
        return [self, self.other] + self.attns


def test_enable_flash_sets_the_slot_and_the_flags_only():
    mod = types.SimpleNamespace(slow_attn="s", fused_mlp_func="f", memory_efficient_attention=None, flash_attn_func=None)
    model = _Model()
    seam.enable_flash(mod)
    assert mod.flash_attn_func is seam.flash_attn_func
    assert (mod.slow_attn, mod.fused_mlp_func, mod.memory_efficient_attention) == ("s", "f", None)
    assert not any(a.using_flash for a in model.attns)                     # no model given: flags untouched
    seam.enable_flash(mod, model)
    assert all(a.using_flash is True for a in model.attns)
    assert all(a.using_xform is False and a.fused_mlp_func is None for a in model.attns)
    assert not hasattr(model, "using_flash") and not hasattr(model.other, "using_flash")
    assert vars(model.other) == {"weight": 1}


def test_enable_flash_on_real_modules():
    import torch.nn as nn

    class Attn(nn.Module):
        def __init__(self):
            super().__init__()
            self.using_flash = False
            self.proj = nn.Linear(4, 4)

    net = nn.Sequential(Attn(), nn.Sequential(Attn()), nn.Linear(4, 4))
    ns = types.SimpleNamespace()
    seam.enable_flash(ns, net)
    assert ns.flash_attn_func is seam.flash_attn_func
    assert net[0].using_flash is True and net[1][0].using_flash is True
    assert not hasattr(net[2], "using_flash") and not hasattr(net, "using_flash")


def test_install_leaves_flash_attn_func_alone():
    bare = types.SimpleNamespace()
    seam.install(bare, _Model())
    assert not hasattr(bare, "flash_attn_func")
    marker = object()
    mod = types.SimpleNamespace(flash_attn_func=marker)
    model = _Model()
    seam.install(mod, model)
    assert mod.flash_attn_func is marker
    assert not any(a.using_flash for a in model.attns)


def test_misaligned_dense_operand_is_copied_to_an_aligned_buffer(monkeypatch):
    """A dense tensor whose storage offset breaks the 16-byte rule (a slice of a flat buffer) is its own .contiguous(): the call must hand the library a fresh,
    aligned copy, and operands that meet the rule must go through untouched.  The library is replaced by a recorder; nothing runs."""
    seen = []

    class _Lib:
        @staticmethod
        def sdvar_op_sdpa_h(q, k, v, out, strides, dtype, B, H, Lq, Lk, hd, scale, stream):
            seen.append((q.value, k.value, v.value, out.value, list(strides), dtype, B, H, Lq, Lk, hd, scale))
            return 0

    monkeypatch.setattr(E, "load_library", lambda *a, **k: _Lib)
    monkeypatch.setattr(E, "_stream", lambda: None)
    flat = torch.zeros(1 * 8 * 2 * 64 + 8 + 4, dtype=torch.bfloat16)
    first = (-(flat.data_ptr() // 2)) % 8                          # elements up to the next 16-byte boundary
    good, odd = _Fake(flat[first:first + 1024].view(1, 8, 2, 64)), _Fake(flat[first + 4:first + 4 + 1024].view(1, 8, 2, 64))
    assert good.data_ptr() % 16 == 0 and odd.data_ptr() % 16 == 8 and odd.is_contiguous()
    out = seam.flash_attn_func(odd, good, good)
    q, k, v, o, strides, dtype, B, H, Lq, Lk, hd, scale = seen[-1]
    assert q % 16 == 0 and q != odd.data_ptr()
    assert k == good.data_ptr() and v == good.data_ptr() and o == out.data_ptr()
    assert strides == [8 * 2 * 64, 64, 2 * 64] * 4 and (dtype, B, H, Lq, Lk, hd, scale) == (2, 1, 2, 8, 8, 64, 0.125)
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (1, 8, 2, 64) and out.is_contiguous()
