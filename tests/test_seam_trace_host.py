"""The launches of seam's attention and FFN slots, without a GPU: every case runs a slot end to end (forward and, where asked, backward) on CPU tensors that report
is_cuda (the _Fake of tests/test_seam_host.py) against a recorder in the library's place, and the recorded (entry name, arguments) sequence, the returned tensor's
shape / strides / dtype and those of every gradient must equal tests/seam_launch_trace.json.  That file is DATA: it was recorded from the code as it stood before the
slots were folded onto one operand check, one launcher and one autograd function (`python tests/test_seam_trace_host.py --record` rewrites it from the code at hand),
so the test pins which entry a call reaches, with which strides, which operands are read in place and which are copied.

How arguments are recorded: scalars as they are, ctypes arrays as lists, a pointer as None, as "in:<name>%16=<r>" when it is the data_ptr() of a named input of the
case (read in place; r = address % 16) or as "new" (a buffer or a copy the seam made)."""
import contextlib
import ctypes as C
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdvar_amd import engine as E  # noqa: E402
from sdvar_amd import seam  # noqa: E402

TRACE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "seam_launch_trace.json")
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


class _Fake(torch.Tensor):
    """A CPU tensor that reports is_cuda = True (the trick of tests/test_seam_host.py)."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)

    @property
    def is_cuda(self):
        return True


class _Recorder:
    """Stands in for the loaded library: every entry records (name, normalised arguments) and returns 0."""

    def __init__(self):
        self.calls, self.inputs, self._alive = [], {}, []

    def name(self, **tensors):
        for n, t in tensors.items():
            if t is not None:
                self.inputs.setdefault(t.data_ptr(), n)
                self._alive.append(t)           # its address cannot be handed to a later buffer while the case runs

    def mark(self, label):
        self.calls.append(["--", [label]])

    def _norm(self, x):
        if x is None or isinstance(x, (bool, int, float, str)):
            return x
        if isinstance(x, C.c_void_p):
            if x.value is None:
                return None
            return f"in:{self.inputs[x.value]}%16={x.value % 16}" if x.value in self.inputs else "new"
        if isinstance(x, C.Array):
            return list(x)
        raise TypeError(f"unexpected argument {x!r}")

    def __getattr__(self, entry):
        def call(*args):
            self.calls.append([entry, [self._norm(a) for a in args]])
            return 0
        return call


@contextlib.contextmanager
def _recording(autocast=None):
    """The recorder in the library's place, caches empty, the GEMM mode and grad mode restored afterwards.  autocast: the dtype torch.autocast would report for the GPU."""
    rec = _Recorder()
    saved = (E.load_library, E._stream, seam._gemm_mode, seam._autocast_gpu_dtype)
    E.load_library, E._stream = (lambda *a, **k: rec), (lambda: None)
    seam._autocast_gpu_dtype = lambda: autocast
    seam.clear_caches()
    try:
        with torch.enable_grad():
            yield rec
    finally:
        E.load_library, E._stream, seam._gemm_mode, seam._autocast_gpu_dtype = saved
        seam.clear_caches()


def _desc(t):
    return None if t is None else {"shape": list(t.shape), "strides": list(t.stride()), "dtype": str(t.dtype)}


def _offset_by_one(shape, dtype):
    """A dense tensor one element into a flat buffer: data_ptr % 16 = the element size."""
    n = 1
    for s in shape:
        n *= s
    return torch.zeros(n + 8, dtype=dtype)[1:1 + n].view(shape)


# ------------------------------------------------------------------------------------------------------------------ attention
def _operand(kind, shape, dtype, blhc, buf, j):
    if kind == "dense":
        t = torch.zeros(shape, dtype=dtype)
    elif kind == "view":                                # the reference's views of one (B, L, 3, H, 64) buffer
        t = buf.unbind(2)[j]
        t = t if blhc else t.permute(0, 2, 1, 3)
    elif kind in ("pad66", "pad68"):                    # row stride 66: breaks both rules; 68: breaks the half rule only
        t = torch.zeros(tuple(shape[:-1]) + (int(kind[3:]),), dtype=dtype)[..., :64]
    elif kind == "transposed":                          # the other layout's memory: strides are fine, read in place
        t = torch.zeros((shape[0], shape[2], shape[1], 64), dtype=dtype).permute(0, 2, 1, 3)
    elif kind == "lastdim":                             # last stride != 1
        t = torch.zeros(tuple(shape[:-1]) + (128,), dtype=dtype)[..., ::2]
    else:
        assert kind == "off1", kind
        t = _offset_by_one(shape, dtype)
    assert tuple(t.shape) == tuple(shape)
    return t


def _mask(kind, dtype, B, H, Lq, Lk):
    if kind is None:
        return None
    if kind == "b4":
        m = torch.zeros(1, 1, Lq, Lk, dtype=dtype)
    elif kind == "2d":
        m = torch.zeros(Lq, Lk, dtype=dtype)
    elif kind == "full":
        m = torch.zeros(B, H, Lq, Lk, dtype=dtype)
    elif kind == "expand":                              # xformers' attn_bias.expand(B, H, -1, -1): stride 0 over B and H
        m = torch.zeros(1, 1, Lq, Lk, dtype=dtype).expand(B, H, Lq, Lk)
    elif kind == "slice":                               # the reference's attn_bias[:, :, :ed, :ed]
        m = torch.zeros(1, 1, Lq + 6, Lk + 6, dtype=dtype)[:, :, :Lq, :Lk]
    elif kind == "row":
        m = torch.zeros(1, 1, 1, Lk, dtype=dtype)
    else:
        assert kind == "keyT", kind                     # key stride != 1: materialised by the seam
        m = torch.zeros(1, 1, Lk, Lq, dtype=dtype).transpose(2, 3)
    return _Fake(m)


def _run_attn(rec, slot, dt=(F32, F32, F32), B=1, H=2, Lq=8, Lk=None, mask=None, mask_dt=torch.bool, ops="dense", grad=None, no_grad=False, dout="dense",
              scale=0.125, calls=1):
    fn, blhc = getattr(seam, slot), not slot.startswith("slow")
    Lk = Lq if Lk is None else Lk
    ops = (ops,) * 3 if isinstance(ops, str) else ops
    buf = torch.zeros(B, Lq, 3, H, 64, dtype=dt[2]) if "view" in ops else None
    shape = lambda L: (B, L, H, 64) if blhc else (B, H, L, 64)
    q, k, v = (_Fake(_operand(kind, shape(L), d, blhc, buf, j).requires_grad_(bool(grad and grad[j])))
               for j, (kind, L, d) in enumerate(zip(ops, (Lq, Lk, Lk), dt)))
    m = _mask(mask, dt[2] if mask_dt == "half" else mask_dt, B, H, Lq, Lk)
    rec.name(q=q, k=k, v=v, mask=m)
    results = []
    for i in range(calls):
        if i:
            rec.mark(f"call {i + 1}")
        with torch.no_grad() if no_grad else contextlib.nullcontext():
            if slot.startswith("slow"):
                out = fn(q, k, v, scale, attn_mask=m)
            elif slot.startswith("flash"):
                out = fn(q, k, v, softmax_scale=scale)
            else:
                out = fn(q, k, v, attn_bias=m, scale=scale)
        res = {"out": _desc(out), "requires_grad": out.requires_grad}
        if out.requires_grad:
            if dout == "dense":
                g = torch.zeros(out.shape, dtype=out.dtype)
            elif dout == "expand":                      # out.sum().backward(): every stride 0
                g = torch.zeros((), dtype=out.dtype).expand(out.shape)
            elif dout == "like":                        # out's own (permuted) strides
                g = torch.zeros_like(out)
            else:
                assert dout == "off1", dout
                g = _offset_by_one(tuple(out.shape), out.dtype)
            rec.name(dout=g)
            rec.mark("backward")
            wanted = [(n, t) for n, t in (("dq", q), ("dk", k), ("dv", v)) if t.requires_grad]
            grads = torch.autograd.grad(out, [t for _, t in wanted], g)
            res.update({n: _desc(gr) for (n, _), gr in zip(wanted, grads)})
        results.append(res)
    return results


A = dict
ALL3 = (True, True, True)
ATTN = {
    # the fp32 inference slots
    "slow_attn nomask": A(slot="slow_attn"),
    "slow_attn bool b4 views Lq70": A(slot="slow_attn", Lq=70, H=3, mask="b4", ops="view"),
    "slow_attn f32 2d cached Lk>Lq": A(slot="slow_attn", B=2, Lq=8, Lk=24, mask="2d", mask_dt=F32),
    "slow_attn slice mask": A(slot="slow_attn", Lq=16, mask="slice", mask_dt=F32),
    "slow_attn row mask": A(slot="slow_attn", Lq=9, Lk=12, mask="row"),
    "slow_attn keyT mask": A(slot="slow_attn", mask="keyT", mask_dt=F32),
    "slow_attn pad66 copied": A(slot="slow_attn", ops=("pad66", "dense", "pad66")),
    "slow_attn pad68 transposed in place": A(slot="slow_attn", ops=("pad68", "transposed", "dense")),
    "slow_attn lastdim copied": A(slot="slow_attn", ops=("dense", "lastdim", "dense")),
    "slow_attn same mask twice": A(slot="slow_attn", mask="b4", calls=2),
    "slow_attn grad mode on no grad operand": A(slot="slow_attn", mask="b4"),
    "memory_efficient_attention nomask scale None": A(slot="memory_efficient_attention", scale=None, ops="view", B=2),
    "memory_efficient_attention expand mask": A(slot="memory_efficient_attention", B=2, Lq=12, mask="expand", mask_dt=F32, scale=0.3),
    "memory_efficient_attention full bool": A(slot="memory_efficient_attention", B=2, H=3, Lq=8, Lk=11, mask="full"),
    # the fp32 grad slots
    "slow_attn_grad no_grad": A(slot="slow_attn_grad", mask="b4", grad=ALL3, no_grad=True),
    "slow_attn_grad detached": A(slot="slow_attn_grad", mask="2d", mask_dt=F32),
    "slow_attn_grad all views": A(slot="slow_attn_grad", Lq=70, mask="b4", ops="view", grad=ALL3),
    "slow_attn_grad nomask q only": A(slot="slow_attn_grad", grad=(True, False, False)),
    "slow_attn_grad kv only cached": A(slot="slow_attn_grad", Lq=8, Lk=20, mask="row", mask_dt=F32, grad=(False, True, True)),
    "slow_attn_grad dout expand": A(slot="slow_attn_grad", mask="slice", grad=ALL3, dout="expand"),
    "slow_attn_grad dout off1": A(slot="slow_attn_grad", grad=ALL3, dout="off1"),
    "slow_attn_grad dout like": A(slot="slow_attn_grad", B=2, grad=ALL3, dout="like"),
    "slow_attn_grad pad66 copied": A(slot="slow_attn_grad", ops=("dense", "pad66", "dense"), grad=ALL3),
    "slow_attn_grad same mask twice": A(slot="slow_attn_grad", mask="b4", grad=ALL3, calls=2),
    "memory_efficient_attention_grad scale None": A(slot="memory_efficient_attention_grad", scale=None, B=2, H=3, ops="view", mask="expand", grad=ALL3),
    "memory_efficient_attention_grad no grad operand": A(slot="memory_efficient_attention_grad", scale=None),
    "memory_efficient_attention_grad q only dout off1": A(slot="memory_efficient_attention_grad", Lq=9, Lk=12, grad=(True, False, False), dout="off1"),
    # flash
    "flash_attn_func f16": A(slot="flash_attn_func", dt=(F16,) * 3, scale=None, ops="view"),
    "flash_attn_func bf16 cached off1 v": A(slot="flash_attn_func", dt=(BF16,) * 3, Lq=8, Lk=24, ops=("dense", "dense", "off1"), scale=0.2),
    "flash_attn_func pad68 copied": A(slot="flash_attn_func", dt=(F16,) * 3, ops=("pad68", "dense", "dense")),
    "flash_attn_func_grad no_grad": A(slot="flash_attn_func_grad", dt=(F16,) * 3, grad=ALL3, no_grad=True, scale=None),
    "flash_attn_func_grad no grad operand": A(slot="flash_attn_func_grad", dt=(BF16,) * 3, scale=0.5, ops=("off1", "dense", "dense")),
    "flash_attn_func_grad bf16 views": A(slot="flash_attn_func_grad", dt=(BF16,) * 3, B=2, Lq=16, ops="view", grad=ALL3, scale=None),
    "flash_attn_func_grad f16 kv only off1 pad68": A(slot="flash_attn_func_grad", dt=(F16,) * 3, Lq=8, Lk=9, ops=("off1", "pad68", "dense"), grad=(False, True, True)),
    "flash_attn_func_grad dout expand": A(slot="flash_attn_func_grad", dt=(F16,) * 3, grad=ALL3, dout="expand"),
}
for _h, _n in ((F16, "f16"), (BF16, "bf16")):
    ATTN.update({
        # the autocast inference slots
        f"slow_attn_amp {_n} nomask 3 half": A(slot="slow_attn_amp", dt=(_h,) * 3, ops="view"),
        f"slow_attn_amp {_n} nomask f32 q": A(slot="slow_attn_amp", dt=(F32, _h, _h)),
        f"slow_attn_amp {_n} bool mask 3 half": A(slot="slow_attn_amp", dt=(_h,) * 3, Lq=70, mask="b4"),
        f"slow_attn_amp {_n} half mask f32 q k": A(slot="slow_attn_amp", dt=(F32, F32, _h), Lq=8, Lk=24, mask="2d", mask_dt="half"),
        f"slow_attn_amp {_n} f32 slice mask twice": A(slot="slow_attn_amp", dt=(_h,) * 3, mask="slice", mask_dt=F32, calls=2),
        f"slow_attn_amp {_n} 3 f32": A(slot="slow_attn_amp", mask="b4"),
        f"slow_attn_amp {_n} pad68 f32 in place half copied": A(slot="slow_attn_amp", dt=(F32, _h, _h), ops=("pad68", "pad68", "dense"), mask="row"),
        f"slow_attn_amp {_n} off1": A(slot="slow_attn_amp", dt=(F32, _h, _h), ops=("off1", "off1", "dense")),
        f"memory_efficient_attention_amp {_n} expand half mask": A(slot="memory_efficient_attention_amp", dt=(_h,) * 3, B=2, H=3, mask="expand", mask_dt="half",
                                                                   scale=None, ops="view"),
        f"memory_efficient_attention_amp {_n} nomask f32 k": A(slot="memory_efficient_attention_amp", dt=(_h, F32, _h), Lq=8, Lk=9, scale=None),
        f"memory_efficient_attention_amp {_n} nomask 3 half": A(slot="memory_efficient_attention_amp", dt=(_h,) * 3, scale=0.2),
        # the autocast grad slots
        f"slow_attn_amp_grad {_n} no_grad": A(slot="slow_attn_amp_grad", dt=(F32, F32, _h), mask="b4", grad=ALL3, no_grad=True),
        f"slow_attn_amp_grad {_n} detached nomask": A(slot="slow_attn_amp_grad", dt=(_h,) * 3),
        f"slow_attn_amp_grad {_n} 3 half bool mask": A(slot="slow_attn_amp_grad", dt=(_h,) * 3, Lq=70, H=3, mask="b4", ops="view", grad=ALL3),
        f"slow_attn_amp_grad {_n} f32 q k half mask": A(slot="slow_attn_amp_grad", dt=(F32, F32, _h), B=2, mask="2d", mask_dt="half", grad=ALL3),
        f"slow_attn_amp_grad {_n} f32 q nomask q only": A(slot="slow_attn_amp_grad", dt=(F32, _h, _h), grad=(True, False, False)),
        f"slow_attn_amp_grad {_n} kv only cached": A(slot="slow_attn_amp_grad", dt=(_h,) * 3, Lq=8, Lk=20, mask="row", mask_dt=F32, grad=(False, True, True)),
        f"slow_attn_amp_grad {_n} 3 f32": A(slot="slow_attn_amp_grad", mask="b4", grad=ALL3),
        f"slow_attn_amp_grad {_n} 3 f32 no grad operand": A(slot="slow_attn_amp_grad", mask="b4"),
        f"slow_attn_amp_grad {_n} dout expand": A(slot="slow_attn_amp_grad", dt=(_h,) * 3, mask="slice", mask_dt=F32, grad=ALL3, dout="expand"),
        f"slow_attn_amp_grad {_n} dout off1": A(slot="slow_attn_amp_grad", dt=(F32, _h, _h), grad=ALL3, dout="off1"),
        f"slow_attn_amp_grad {_n} copies": A(slot="slow_attn_amp_grad", dt=(F32, _h, _h), ops=("off1", "pad68", "off1"), grad=ALL3, dout="like"),
        f"slow_attn_amp_grad {_n} same mask twice": A(slot="slow_attn_amp_grad", dt=(_h,) * 3, mask="b4", grad=ALL3, calls=2),
        f"memory_efficient_attention_amp_grad {_n} expand mask scale None": A(slot="memory_efficient_attention_amp_grad", dt=(F32, F32, _h), B=2, H=3, mask="expand",
                                                                              mask_dt="half", scale=None, grad=ALL3),
        f"memory_efficient_attention_amp_grad {_n} nomask views": A(slot="memory_efficient_attention_amp_grad", dt=(_h,) * 3, ops="view", scale=None, grad=ALL3),
        f"memory_efficient_attention_amp_grad {_n} 3 f32 q only": A(slot="memory_efficient_attention_amp_grad", scale=None, grad=(True, False, False)),
    })


def _case_fp32_off1(rec):
    """A dense fp32 operand at data_ptr % 16 == 4, each of q, k, v in turn: slow_attn, then slow_attn_grad forward + backward, then memory_efficient_attention."""
    results = []
    for j in range(3):
        ops = tuple("off1" if i == j else "dense" for i in range(3))
        rec.mark(f"operand {j}")
        results += _run_attn(rec, "slow_attn", ops=ops, mask="b4")
        results += _run_attn(rec, "slow_attn_grad", ops=ops, mask="b4", grad=ALL3)
        results += _run_attn(rec, "memory_efficient_attention", ops=ops)
    return results


# ------------------------------------------------------------------------------------------------------------------ the FFN
def _run_mlp(rec, slot, mode=None, xdt=F32, wdt=F32, bias=True, xshape=(2, 5, 64), hid=128, Cout=64, grad=None, no_grad=False, dy="dense", steps=("call",)):
    fn = getattr(seam, slot)
    if mode is not None:
        seam.configure(mode)
    grad = grad or (False,) * 5
    x = _Fake(torch.zeros(xshape, dtype=xdt, requires_grad=grad[0]))
    w1, w2 = _Fake(torch.zeros(hid, xshape[-1], dtype=wdt, requires_grad=grad[1])), _Fake(torch.zeros(Cout, hid, dtype=wdt, requires_grad=grad[2]))
    b1 = _Fake(torch.zeros(hid, requires_grad=grad[3])) if bias else None
    b2 = _Fake(torch.zeros(Cout, requires_grad=grad[4])) if bias else None
    rec.name(x=x, w1=w1, w2=w2, b1=b1, b2=b2)
    results = []
    for step in steps:
        rec.mark(step)
        if step == "update":                            # an optimiser step: the weights' _version moves
            with torch.no_grad():
                w1.add_(1.0)
                w2.add_(1.0)
            continue
        with torch.no_grad() if no_grad else contextlib.nullcontext():
            out = fn(x, w1, w2, b1, b2)
        res = {"out": _desc(out), "requires_grad": out.requires_grad}
        if out.requires_grad:
            if dy == "dense":
                g = torch.zeros(out.shape, dtype=out.dtype)
            elif dy == "expand":
                g = torch.zeros((), dtype=out.dtype).expand(out.shape)
            else:
                assert dy == "off1", dy
                g = _offset_by_one(tuple(out.shape), out.dtype)
            rec.name(dy=g)
            rec.mark("backward")
            wanted = [(n, t) for n, t in (("dx", x), ("dw1", w1), ("dw2", w2), ("db1", b1), ("db2", b2)) if t is not None and t.requires_grad]
            grads = torch.autograd.grad(out, [t for _, t in wanted], g)
            res.update({n: _desc(gr) for (n, _), gr in zip(wanted, grads)})
        results.append(res)
    return results


ALL5 = (True,) * 5
MLP = {}
for _m in E.GEMM_MODES:
    MLP.update({
        f"fused_mlp_func {_m} bias twice": A(slot="fused_mlp_func", mode=_m, steps=("call", "call")),
        f"fused_mlp_func {_m} nobias": A(slot="fused_mlp_func", mode=_m, bias=False, xshape=(7, 64), Cout=40),
        f"fused_mlp_func {_m} M0": A(slot="fused_mlp_func", mode=_m, xshape=(0, 64)),
        f"fused_mlp_func_grad {_m} no_grad": A(slot="fused_mlp_func_grad", mode=_m, grad=ALL5, no_grad=True),
        f"fused_mlp_func_grad {_m} nothing requires grad": A(slot="fused_mlp_func_grad", mode=_m, bias=False, Cout=40),
        f"fused_mlp_func_grad {_m} all update all": A(slot="fused_mlp_func_grad", mode=_m, grad=ALL5, steps=("call", "call", "update", "call")),
        f"fused_mlp_func_grad {_m} nobias": A(slot="fused_mlp_func_grad", mode=_m, bias=False, grad=ALL5, xshape=(70, 64)),
        f"fused_mlp_func_grad {_m} frozen weights": A(slot="fused_mlp_func_grad", mode=_m, grad=(True, False, False, False, False)),
        f"fused_mlp_func_grad {_m} x without grad": A(slot="fused_mlp_func_grad", mode=_m, grad=(False, True, True, True, True)),
        f"fused_mlp_func_grad {_m} w2 b2 only dy expand": A(slot="fused_mlp_func_grad", mode=_m, grad=(False, False, True, False, True), dy="expand"),
        f"fused_mlp_func_grad {_m} dy off1": A(slot="fused_mlp_func_grad", mode=_m, grad=ALL5, dy="off1"),
        f"fused_mlp_func_grad {_m} M0": A(slot="fused_mlp_func_grad", mode=_m, grad=ALL5, xshape=(0, 64)),
    })
for _h, _n in ((F16, "f16"), (BF16, "bf16")):
    MLP.update({
        f"fused_mlp_func_amp {_n} half x bias twice": A(slot="fused_mlp_func_amp", xdt=_h, steps=("call", "call")),
        f"fused_mlp_func_amp {_n} f32 x autocast nobias": A(slot="fused_mlp_func_amp", autocast=_h, bias=False, xshape=(7, 64), Cout=40),
        f"fused_mlp_func_amp {_n} half weights": A(slot="fused_mlp_func_amp", xdt=_h, wdt=_h),
        f"fused_mlp_func_amp {_n} M0": A(slot="fused_mlp_func_amp", xdt=_h, xshape=(0, 64)),
        f"fused_mlp_func_amp_grad {_n} no_grad": A(slot="fused_mlp_func_amp_grad", autocast=_h, grad=ALL5, no_grad=True),
        f"fused_mlp_func_amp_grad {_n} nothing requires grad": A(slot="fused_mlp_func_amp_grad", xdt=_h, bias=False, Cout=40),
        f"fused_mlp_func_amp_grad {_n} all update all": A(slot="fused_mlp_func_amp_grad", autocast=_h, grad=ALL5, steps=("call", "call", "update", "call")),
        f"fused_mlp_func_amp_grad {_n} half x nobias": A(slot="fused_mlp_func_amp_grad", xdt=_h, bias=False, grad=ALL5, xshape=(70, 64)),
        f"fused_mlp_func_amp_grad {_n} frozen weights": A(slot="fused_mlp_func_amp_grad", autocast=_h, grad=(True, False, False, False, False)),
        f"fused_mlp_func_amp_grad {_n} x without grad": A(slot="fused_mlp_func_amp_grad", xdt=_h, grad=(False, True, True, True, True)),
        f"fused_mlp_func_amp_grad {_n} w2 b2 only dy expand": A(slot="fused_mlp_func_amp_grad", xdt=_h, grad=(False, False, True, False, True), dy="expand"),
        f"fused_mlp_func_amp_grad {_n} dy off1": A(slot="fused_mlp_func_amp_grad", autocast=_h, grad=ALL5, dy="off1"),
        f"fused_mlp_func_amp_grad {_n} M0": A(slot="fused_mlp_func_amp_grad", xdt=_h, grad=ALL5, xshape=(0, 64)),
    })

FP32_OFF1 = "fp32 dense operand at address % 16 == 4"
CASES = sorted(list(ATTN) + list(MLP) + [FP32_OFF1])


def run_case(name):
    spec = dict(ATTN.get(name) or MLP.get(name) or {})
    with _recording(autocast=spec.pop("autocast", None)) as rec:
        if name == FP32_OFF1:
            results = _case_fp32_off1(rec)
        elif name in ATTN:
            results = _run_attn(rec, **spec)
        else:
            results = _run_mlp(rec, **spec)
        return json.loads(json.dumps({"calls": rec.calls, "results": results}))


@pytest.fixture(scope="module")
def expected():
    with open(TRACE) as f:
        return json.load(f)


def test_the_trace_file_lists_exactly_the_cases(expected):
    assert sorted(expected) == CASES


@pytest.mark.parametrize("name", CASES)
def test_launch_trace(name, expected):
    got, want = run_case(name), expected[name]
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]]
    for g, w in zip(got["calls"], want["calls"]):
        assert g == w
    assert got["results"] == want["results"]


def test_recorded_entries_are_the_librarys():
    """Every entry a case reaches exists in engine._SIGNATURES with the recorded number of arguments: the recorder accepts anything, the library would not."""
    with open(TRACE) as f:
        for case in json.load(f).values():
            for entry, args in case["calls"]:
                if entry != "--":
                    assert len(E._SIGNATURES[entry][1]) == len(args), entry


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_seam_trace_host.py --record")
    with open(TRACE, "w") as f:
        json.dump({name: run_case(name) for name in CASES}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(CASES)} cases to {TRACE}")
