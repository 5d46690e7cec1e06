"""The autocast slots of sdvar_amd.seam (slow_attn_amp, memory_efficient_attention_amp, install_amp) without a GPU: every refusal is an SdvarError raised before
the library is touched, install_amp sets what install + enable_flash set plus the slow_attn slot, the fp32 slots still refuse half operands, sdvar_op_sdpa_hm reports
argument errors through sdvar_last_error before any HIP call, and sdvar_op_sdpa_skip_map accepts the half bias kinds.  The last test is a host emulation, on exact
integer data, of the kernel's fp32 -> half load paths and of its bias lane map against the documented MFMA operand layouts."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from sdvar_amd import engine as E
from sdvar_amd import seam


class _Fake(torch.Tensor):
    """A CPU tensor that reports is_cuda = True (the trick of test_seam_host.py): the checks that come AFTER the device check run without a GPU.  Nothing is ever
    launched on it: every case below must raise before the library is called."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)

    @property
    def is_cuda(self):
        return True


def _t(dtype=torch.float16, L=8, c=64, grad=False, B=1, H=2):
    return _Fake(torch.zeros(B, H, L, c, dtype=dtype, requires_grad=grad))


@pytest.fixture
def no_library(monkeypatch):
    """Any touch of the library fails the test: the refusals come first."""
    def boom(*a, **k):
        raise AssertionError("the library was touched before the refusal")
    monkeypatch.setattr(E, "load_library", boom)


def test_refusals_come_before_the_library(no_library):
    h, b, f = _t(torch.float16), _t(torch.bfloat16), _t(torch.float32)
    for fn, who in ((lambda *a, **k: seam.slow_attn_amp(a[0], a[1], a[2], 1.0, *a[3:], **k), "slow_attn_amp"),
                    (seam.memory_efficient_attention_amp, "memory_efficient_attention_amp")):
        with pytest.raises(E.SdvarError, match=who + ".*value is torch.float32"):
            fn(h, h, f)
        with pytest.raises(E.SdvarError, match="value is torch.float32"):
            fn(f, b, f)
        with pytest.raises(E.SdvarError, match="mixed half dtypes"):
            fn(h, b, b)
        with pytest.raises(E.SdvarError, match="mixed half dtypes"):
            fn(f, b, h)
        for bad in ((_t(torch.float64), h, h), (h, _t(torch.float64), h), (f, f, _t(torch.float64))):
            with pytest.raises(E.SdvarError, match="float64"):
                fn(*bad)
        with pytest.raises(E.SdvarError, match="CPU"):
            fn(torch.zeros(1, 2, 8, 64, dtype=torch.float16), h, h)
        with pytest.raises(E.SdvarError, match="CPU"):
            fn(h, h, h, torch.zeros(1, 1, 8, 8))                                    # a CPU mask
        with pytest.raises(E.SdvarError, match="head dim 32"):
            fn(_t(c=32), _t(c=32), _t(c=32))
        with pytest.raises(E.SdvarError, match="shapes do not match"):
            fn(h, _t(L=9), _t(L=10))
        with pytest.raises(E.SdvarError, match="shapes do not match"):
            fn(h, _t(B=2), _t(B=2))
        with pytest.raises(E.SdvarError, match="3 dims"):
            fn(_Fake(torch.zeros(2, 8, 64, dtype=torch.float16)), h, h)
        g = _t(grad=True)
        with torch.enable_grad():
            for ops in ((g, h, h), (h, g, h), (f, h, g)):
                with pytest.raises(E.SdvarError, match="grad"):
                    fn(*ops)
        with torch.no_grad():                                                       # allowed by the grad rule: goes on to the next refusal
            with pytest.raises(E.SdvarError, match="mask"):
                fn(g, h, h, _Fake(torch.zeros(1, 1, 8, 8, dtype=torch.bfloat16)))
        with pytest.raises(E.SdvarError, match="the mask is torch.bfloat16 but the operands are torch.float16"):
            fn(f, f, h, _Fake(torch.zeros(1, 1, 8, 8, dtype=torch.bfloat16)))
        with pytest.raises(E.SdvarError, match="the mask is torch.float16 but the operands are torch.bfloat16"):
            fn(b, b, b, _Fake(torch.zeros(1, 1, 8, 8, dtype=torch.float16)))
        with pytest.raises(E.SdvarError, match="the mask is torch.float64"):
            fn(h, h, h, _Fake(torch.zeros(1, 1, 8, 8, dtype=torch.float64)))
        with pytest.raises(E.SdvarError, match="does not broadcast"):
            fn(h, h, h, _Fake(torch.zeros(1, 1, 8, 7)))
    with pytest.raises(E.SdvarError, match="dropout"):
        seam.slow_attn_amp(h, h, h, 1.0, None, 0.1)
    with pytest.raises(E.SdvarError, match="dropout"):
        seam.memory_efficient_attention_amp(h, h, h, None, p=0.5)


def test_fp32_slots_and_flash_still_refuse_what_the_amp_slots_take(no_library):
    h, f = _t(torch.float16), _t(torch.float32)
    for bad in (torch.float16, torch.bfloat16):
        with pytest.raises(E.SdvarError, match="float32"):
            seam.slow_attn(f, f, _t(bad), 1.0)
        with pytest.raises(E.SdvarError, match="float32"):
            seam.memory_efficient_attention(_t(bad), _t(bad), _t(bad))
    with pytest.raises(E.SdvarError, match="float32"):
        seam.flash_attn_func(f, h, h)                                               # mixed operands stay refused by the flash slot


class _FFN:
    def __init__(self):
        self.fused_mlp_func = None


class _Attn:
    def __init__(self):
        self.using_flash = False


class _Model:
    def __init__(self):
        self.ffns, self.attns, self.other = [_FFN(), _FFN()], [_Attn(), _Attn()], types.SimpleNamespace(weight=1)

    def modules(self):
        return [self, self.other] + self.ffns + self.attns


def test_install_amp_on_a_namespace():
    sentinel = object()
    mod = types.SimpleNamespace(slow_attn=None, fused_mlp_func=None, flash_attn_func=None, memory_efficient_attention=sentinel)
    model = _Model()
    seam.install_amp(mod)
    assert mod.slow_attn is seam.slow_attn_amp and mod.fused_mlp_func is seam.fused_mlp_func and mod.flash_attn_func is seam.flash_attn_func
    assert mod.memory_efficient_attention is sentinel
    assert all(f.fused_mlp_func is None for f in model.ffns) and not any(a.using_flash for a in model.attns)       # no model given
    seam.install_amp(mod, model)
    assert all(f.fused_mlp_func is seam.fused_mlp_func for f in model.ffns) and all(a.using_flash is True for a in model.attns)
    assert not hasattr(model.other, "fused_mlp_func") and not hasattr(model.other, "using_flash")
    assert mod.slow_attn is seam.slow_attn_amp and mod.memory_efficient_attention is sentinel
    seam.install(mod, model)                                                        # install() alone goes back to the fp32 slot
    assert mod.slow_attn is seam.slow_attn


def test_install_amp_on_real_modules():
    import torch.nn as nn

    class FFN(nn.Module):
        def __init__(self):
            super().__init__()
            self.fused_mlp_func = None
            self.fc1 = nn.Linear(4, 8)

    class Attn(nn.Module):
        def __init__(self):
            super().__init__()
            self.using_flash = False
            self.proj = nn.Linear(4, 4)

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.ffn, self.attn = FFN(), Attn()

    net = nn.Sequential(Block(), Block())
    ns = types.SimpleNamespace()
    seam.install_amp(ns, net)
    assert all(b.ffn.fused_mlp_func is seam.fused_mlp_func and b.attn.using_flash is True for b in net)
    assert ns.slow_attn is seam.slow_attn_amp and ns.flash_attn_func is seam.flash_attn_func and not hasattr(ns, "memory_efficient_attention")


def test_op_sdpa_hm_argument_errors_without_gpu():
    lib = E.load_library()
    assert lib.sdvar_abi_version() == 5
    i64 = C.c_int64
    buf = (C.c_float * 64)()                                        # host memory: only its (aligned) address is looked at, every call returns before any HIP call
    base = (C.addressof(buf) + 15) & ~15
    p = C.c_void_p(base)
    dense = lambda L: [2 * L * 64, L * 64, 64]
    ok = (i64 * 12)(*(dense(4) * 4))
    b3 = (i64 * 3)(0, 0, 4)

    def call(q=p, k=p, v=p, out=p, strides=ok, dtype=1, qf=0, kf=0, bias=None, kind=0, bs=None, smap=None, c=64):
        rc = lib.sdvar_op_sdpa_hm(q, k, v, out, strides, dtype, qf, kf, bias, kind, bs, smap, 1, 2, 4, 4, c, 1.0, None)
        return rc, lib.sdvar_last_error()

    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(strides=None)):
        rc, err = call(**kw)
        assert rc == 1 and b"null operand" in err
    for bad in (0, 3):
        rc, err = call(dtype=bad)
        assert rc == 1 and b"dtype %d" % bad in err
    rc, err = call(c=32)
    assert rc == 1 and b"head dim 32" in err
    half12 = (i64 * 12)(*(dense(4) + [2 * 4 * 68, 4 * 68, 68] + dense(4) * 2))          # k token stride 68 halves = 136 bytes
    rc, err = call(strides=half12)
    assert rc == 1 and b"k strides" in err and b"multiple of 8" in err
    rc, err = call(strides=half12, kf=1)                                                # the same strides in floats meet the fp32 rule
    assert not (rc == 1 and b"k strides" in err)
    f12 = (i64 * 12)(*([2 * 4 * 66, 4 * 66, 66] + dense(4) * 3))                        # q token stride 66 floats
    rc, err = call(strides=f12, qf=1)
    assert rc == 1 and b"fp32 q strides" in err and b"multiple of 4" in err
    rc, err = call(q=C.c_void_p(base + 8))
    assert rc == 1 and b"q is not 16-byte aligned" in err
    rc, err = call(kind=1)                                                              # a bias kind without a bias
    assert rc == 1 and b"bias pointer and bias kind 1 disagree" in err
    rc, err = call(bias=p, kind=0)
    assert rc == 1 and b"disagree" in err
    rc, err = call(bias=p, kind=4, bs=b3)
    assert rc == 1 and b"bias kind 4" in err
    rc, err = call(bias=p, kind=3)
    assert rc == 1 and b"bias strides" in err
    rc, err = call(smap=p)
    assert rc == 1 and b"a skip map needs a bias" in err
    rc, err = call(qf=2)
    assert rc == 1 and b"q_f32" in err


def test_skip_map_takes_the_half_bias_kinds_as_far_as_its_argument_checks_go():
    lib = E.load_library()
    i64 = C.c_int64
    buf = (C.c_float * 8)()
    p = C.c_void_p(C.addressof(buf))
    for kind in (1, 2, 3, 4):                                       # accepted kinds reach the next check: a negative stride
        rc = lib.sdvar_op_sdpa_skip_map(p, kind, (i64 * 3)(0, 0, -4), 1, 1, 4, 4, p, None)
        assert rc == 1 and b"negative bias stride" in lib.sdvar_last_error()
    for kind in (0, 5):
        rc = lib.sdvar_op_sdpa_skip_map(p, kind, (i64 * 3)(0, 0, -4), 1, 1, 4, 4, p, None)
        assert rc == 1 and b"bias kind %d" % kind in lib.sdvar_last_error()


# ------------------------------------------------------------------------------------------------------ host emulation of the kernel's maps, exact integer data

def _mfma_32x32x16(A, B):
    """D = A B from per-lane fragments, by the documented gfx950 layout of v_mfma_f32_32x32x16_{f16,bf16}: lane l (r = l & 31, h = l >> 5) holds A[r][8h + j] and
    B[8h + j][r] in element j; D[(i & 3) + 8 (i >> 2) + 4h][r] is register i of lane l."""
    Am, Bm = np.zeros((32, 16)), np.zeros((16, 32))
    for l in range(64):
        r, h = l & 31, l >> 5
        Am[r, 8 * h:8 * h + 8] = A[l]
        Bm[8 * h:8 * h + 8, r] = B[l]
    Dm = Am @ Bm
    D = np.zeros((64, 16))
    for l in range(64):
        r, h = l & 31, l >> 5
        for i in range(16):
            D[l, i] = Dm[(i & 3) + 8 * (i >> 2) + 4 * h, r]
    return D


@pytest.mark.parametrize("q_f32, k_f32", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_host_emulation_of_the_load_paths_and_the_bias_lane_map(q_f32, k_f32):
    """One wave (32 queries) against one 64-key tile, following attention_sdpa_hm_kernel's address arithmetic step by step: Q fragments from a strided row of halves
    or of floats (two 16-byte pieces per 8 channels, packed pairwise in order), K staged by 256 threads through the swizzled LDS image (the second 16 bytes of an
    fp32 chunk at +16 bytes), the K fragment read back, S^T = K Q^T on the emulated MFMA, then the bias of register i taken from group j = 4 sub + (i >> 2),
    element i & 3, on the vector path (packed words per bias kind) and on the element path.  Small integers are exact in every format involved."""
    rng = np.random.default_rng(5)
    Lk, qs2, ks2 = 64, 3 * 64, 2 * 64                      # token strides in elements: rows of a shared buffer
    Q, K = rng.integers(-3, 4, (32, 64)).astype(np.float64), rng.integers(-3, 4, (Lk, 64)).astype(np.float64)
    bias = rng.integers(-4, 5, (32, Lk)).astype(np.float64)
    qmem, kmem = np.zeros(32 * qs2), np.zeros(Lk * ks2)    # one array slot per ELEMENT (float or half: the emulation counts elements, the kernel bytes / element size)
    for r in range(32):
        qmem[r * qs2:r * qs2 + 64] = Q[r]
    for r in range(Lk):
        kmem[r * ks2:r * ks2 + 64] = K[r]
    # Q fragments: lane (li, lh), k-step c, element j = channel 16 c + 8 lh + j
    qf = np.zeros((4, 64, 8))
    for lane in range(64):
        li, lh = lane & 31, lane >> 5
        off = li * qs2 + 8 * lh
        for c in range(4):
            if q_f32:
                lo, hi = qmem[off + 16 * c:off + 16 * c + 4], qmem[off + 16 * c + 4:off + 16 * c + 8]          # two 16-byte loads
                qf[c, lane] = [lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]]                          # pack8: pairs in order
            else:
                qf[c, lane] = qmem[off + 16 * c:off + 16 * c + 8]                                               # one 16-byte load
    # K staging through LDS: [key][8 chunks of 8 halves], chunk index swizzled
    lds = np.full((64 * 8, 8), np.nan)
    for tid in range(256):
        skey, sch = tid >> 3, tid & 7
        for i in range(2):
            key = skey + 32 * i
            p0 = min(key, Lk - 1) * ks2 + 8 * sch                                                               # element address of the chunk, both formats
            chunk = np.concatenate((kmem[p0:p0 + 4], kmem[p0 + 4:p0 + 8])) if k_f32 else kmem[p0:p0 + 8]        # fp32: rk | rkh (+16 bytes = +4 floats)
            lds[key * 8 + (sch ^ ((key >> 1) & 7))] = chunk
    assert not np.isnan(lds).any()
    S = np.zeros((2, 64, 16))
    for sub in range(2):
        for c in range(4):
            kf = np.zeros((64, 8))
            for lane in range(64):
                li, lh = lane & 31, lane >> 5
                kf[lane] = lds[(32 * sub + li) * 8 + ((2 * c + lh) ^ ((li >> 1) & 7))]
            S[sub] += _mfma_32x32x16(kf, qf[c])
    want = Q @ K.T
    for packed in (True, False):
        for kind in (1, 2, 3):
            bvals = (bias > 0).astype(np.float64) if kind == 2 else bias
            for lane in range(64):
                li, lh = lane & 31, lane >> 5
                row = bvals[li]
                bq = np.zeros((8, 4))
                for j in range(8):
                    key = (j >> 2) * 32 + 8 * (j & 3) + 4 * lh
                    if packed:
                        bq[j] = row[key:key + 4]                   # fp32: one 16-byte load; uint8: 4 bytes of one word; half: 2 words of 2 halves, low half first
                    else:
                        bq[j] = [row[min(key + e, Lk - 1)] for e in range(4)]
                for sub in range(2):
                    for i in range(16):
                        key = 32 * sub + (i & 3) + 8 * (i >> 2) + 4 * lh
                        assert S[sub, lane, i] == want[li, key]
                        assert bq[4 * sub + (i >> 2)][i & 3] == bvals[li, key]
