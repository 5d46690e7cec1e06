"""GPU: sdvar_op_gemm_h_ex, the half GEMM as the engine's GEMM mode 'f16' launches it (csrc/gemm_half.hip): per-tensor scale, the three epilogues, the gated
residual in and out of place.  Conventions of tests/test_gpu_gemm_exact.py: guarded buffers pre-filled with INT_FILL / HALF_FILL, failures name the first element.

Exact-integer cases.  x, w integers in [-8, 8]; the weight operand holds w * 2^S (S in {0, 3, -2}: |w 2^S| <= 64, multiples of 1/4 - exact in fp16) and w_scale =
2^-S; bias in [-8, 8], res in [-64, 64], gate in {-2, -1, -1/2, 0, 1/2, 1, 2}.  Every product is an integer (times 2^S) of magnitude <= 64 and every partial sum of at
most K = 1024 of them is below 2^16 (times 2^S): fp32 accumulation is exact in any order.  acc * 2^-S = the integer dot product, v = that + bias (|v| <= 65544),
v * gate a multiple of 1/2 below 2^18 and res + v * gate one below 2^18 + 64: all exact in fp32's 24 bits.  So epilogues 0 and 2 must equal int64 arithmetic BIT FOR
BIT, epilogue 1's pre_out must be the fp16 rounding of the saturated v bit for bit, and its h_out is the GELU of exactly that value, held to the derived bound the
existing half-GEMM test uses (gemm_exact_cases.gelu_bound, 'exp' form, one rounding to fp16).

Real-valued case (257, 384, 1024), one per epilogue, against float64 on the fp16-rounded operands.  The fp32 MFMA chain of length K is held to
|acc - sum| <= K u sum_k |x_k w_k|, u = 2^-24 (the classical bound of recursive summation; products of fp16 values are exact in fp32), and each epilogue operation
adds its own rounding: one u per fp32 operation on the magnitude it rounds - written out in RealCase and the three tests.  Nothing is fitted."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gemm_exact_cases as G
from conftest import rnd
from sdvar_amd import engine as E
from test_gpu_gemm_exact import GuardedPlanes, GuardedRows, assert_same, assert_within, half_operand
from test_gpu_ops import _p, _st

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

MS, NS, KS = (1, 33, 130, 257), (128, 136, 192), (32, 96, 1024)          # N = 136: the tile edge falls inside a 32-column group
RPGS = (1, 5, 36)                                                        # the gate row changes inside a 32-row tile and inside a 128-row tile
S_EXP = (0, 3, -2)
SHAPES = [(m, n, k) for m in MS for n in NS for k in KS]
F16_MAX = 65504.0
U = G.U32


class Case:
    """CPU tensors; integers (gate: small powers of two as well) held in int64 / float64 - `v` and ref() are exact."""

    def __init__(self, M, N, K):
        g = np.random.Generator(np.random.Philox(key=[M * 1000 + N, K]))
        self.M, self.N, self.K = M, N, K
        self.X = torch.from_numpy(g.integers(-8, 9, size=(M, K)))
        self.W = torch.from_numpy(g.integers(-8, 9, size=(N, K)))
        self.X[1::3] = 0                                                   # one row in three with two non-zero entries: |v| <= 136, the curved part of the GELU
        for i in range(1, M, 3):
            self.X[i, g.integers(0, K, size=2)] = torch.from_numpy(g.choice(np.array([-8, -3, -1, 1, 2, 8]), size=2))
        self.bias = torch.from_numpy(g.integers(-8, 9, size=(N,)))
        self.res = torch.from_numpy(g.integers(-64, 65, size=(M, N)))
        self.gate = torch.from_numpy(g.choice(np.array([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0]), size=(M, 2 * N)))      # (gate rows, gate_stride = 2 N)
        self.v = self.X @ self.W.t() + self.bias                           # int64
        assert int(self.v.abs().max()) < 2 ** 17

    def ref2(self, rpg):
        gr = self.gate[:(self.M + rpg - 1) // rpg, :self.N].repeat_interleave(rpg, 0)[:self.M]
        return (self.res.double() + self.v.double() * gr).float()         # a multiple of 1/2 below 2^19: exact in float64 and in fp32


@functools.lru_cache(maxsize=None)
def case(M, N, K):
    return Case(M, N, K)


def operands(c, S, dev):
    return (half_operand(c.X.float(), torch.float16, dev), half_operand(c.W.float() * 2.0 ** S, torch.float16, dev),
            torch.tensor([2.0 ** -S], device=dev), c.bias.float().to(dev))


def launch(c, S, epi, dev, what, rpg=1, inplace=False, ops=None):
    """One sdvar_op_gemm_h_ex launch into guarded buffers with ldo = ldres = N + 8.  Returns out (M, N) fp32, or (pre_out fp16 (M, N), h as float64) for epilogue 1."""
    lib = E.load_library()
    M, N, K = c.M, c.N, c.K
    Xo, Wo, sc, b = ops if ops is not None else operands(c, S, dev)
    if epi == 1:
        h, pre = GuardedPlanes(1, M, N, dev), GuardedRows(M, N, N, dev, words=torch.int16)
        E._check(lib.sdvar_op_gemm_h_ex(_p(Xo), _p(Wo), 1, _p(sc), _p(b), None, 0, h.ptr, pre.ptr, None, 0, None, 1, 0, M, N, K, 1, _st()))
        h.check_guards(what + " h_out"); pre.check_guards(what + " pre_out")
        return pre.interior(torch.float16), h.value("f16", what)
    if epi == 0:
        out = GuardedRows(M, N, N + 8, dev)
        E._check(lib.sdvar_op_gemm_h_ex(_p(Xo), _p(Wo), 1, _p(sc), _p(b), out.ptr, N + 8, None, None, None, 0, None, 1, 0, M, N, K, 0, _st()))
        out.check_guards(what + " out")
        return out.interior()
    gate = c.gate.float().to(dev).contiguous()
    res = GuardedRows(M, N, N + 8, dev, init=c.res.float())
    out = res if inplace else GuardedRows(M, N, N + 8, dev)
    E._check(lib.sdvar_op_gemm_h_ex(_p(Xo), _p(Wo), 1, _p(sc), _p(b), out.ptr, N + 8, None, None, res.ptr, N + 8, _p(gate), rpg, 2 * N, M, N, K, 2, _st()))
    out.check_guards(what + " out")                                       # the guard rows behind row M - 1 and the strip beyond column N included
    if not inplace:
        res.check_guards(what + " res", untouched=True)
    return out.interior()


def test_bias_epilogue_exact(dev):
    for i, (M, N, K) in enumerate(SHAPES):
        c, S = case(M, N, K), S_EXP[i % 3]
        what = f"gemm_h_ex epilogue 0 ({M}, {N}, {K}) S = {S}"
        assert_same(launch(c, S, 0, dev, what), c.v.float().to(dev), what)


def test_gelu_epilogue_exact(dev):
    """pre_out bit for bit; h_out = fp16(gelu(pre_out)) within gelu_bound.  N = 136 is not a legal epilogue-1 width (N % 32: h_out is the next GEMM's K-blocked
    operand) and must be refused."""
    worst = 0.0
    for i, (M, N, K) in enumerate(SHAPES):
        c, S = case(M, N, K), S_EXP[(i + 1) % 3]
        what = f"gemm_h_ex epilogue 1 ({M}, {N}, {K}) S = {S}"
        if N % 32:
            with pytest.raises(E.SdvarError):
                launch(c, S, 1, dev, what)
            continue
        pre, h = launch(c, S, 1, dev, what)
        ph = c.v.double().clamp(-F16_MAX, F16_MAX).to(torch.float16)      # saturate, then one nearest-even rounding
        assert_same(pre, ph.to(dev), what + " pre_out")
        p = ph.double()
        ref, bound = G.gelu64(p), G.gelu_bound(p, "exp", "f16")
        err = assert_within(h.cpu(), ref, bound, what + " h_out")
        worst = max(worst, G.gelu_worst_ratio(err, bound, ref)[0])
    print(f"gemm_h_ex GELU err / bound: worst {worst:.3f}")


def test_gated_residual_exact_in_and_out_of_place(dev):
    for i, (M, N, K) in enumerate(SHAPES):
        c, S = case(M, N, K), S_EXP[(i + 2) % 3]
        ops = operands(c, S, dev)
        for rpg in RPGS:
            what = f"gemm_h_ex epilogue 2 ({M}, {N}, {K}) S = {S} rows_per_gate {rpg}"
            ref = c.ref2(rpg).to(dev)
            out = launch(c, S, 2, dev, what, rpg, ops=ops)
            assert_same(out, ref, what)
            assert_same(launch(c, S, 2, dev, what + " in place", rpg, inplace=True, ops=ops), out, what + " in place against out of place")


# ------------------------------------------------------------------------------------------------------------------------ real values
RM, RN, RK, RS = 257, 384, 1024, 3


class RealCase:
    def __init__(self):
        M, N, K = RM, RN, RK
        self.M, self.N, self.K = M, N, K
        self.X = rnd(31, (M, K)).to(torch.float16)
        self.W = rnd(32, (N, K), K ** -0.5).to(torch.float16)              # fp16-rounded; times 2^RS in the operand (exact: no overflow near 2^3 * 0.2)
        self.bias, self.res, self.gate = rnd(33, (N,)), rnd(34, (M, N)), rnd(35, (M, 2 * N))
        x, w = self.X.double(), self.W.double()
        self.sum = x @ w.t()                                               # float64: error ~ 2^-53, nothing against the bounds below
        self.e_acc = K * U * (x.abs() @ w.abs().t())                       # |acc 2^-S - sum| <= K u sum_k |x_k w_k| (the scale is a power of two: exact)
        self.vref = self.sum + self.bias.double()
        self.e_v = self.e_acc + U * (self.vref.abs() + self.e_acc)         # v = fl(acc s + bias): one rounding of the sum on top


@functools.lru_cache(maxsize=None)
def real_case():
    return RealCase()


def real_ops(c, dev):
    return (half_operand(c.X.float(), torch.float16, dev), half_operand(c.W.float() * 2.0 ** RS, torch.float16, dev), torch.tensor([2.0 ** -RS], device=dev), c.bias.to(dev))


class _Shim:
    """launch() reads M, N, K, gate and res of a case."""

    def __init__(self, c):
        self.M, self.N, self.K, self.gate, self.res = c.M, c.N, c.K, c.gate, c.res


def test_real_bias(dev):
    c = real_case()
    out = launch(_Shim(c), RS, 0, dev, "gemm_h_ex real epilogue 0", ops=real_ops(c, dev)).double().cpu()
    err = assert_within(out, c.vref, c.e_v, "gemm_h_ex real epilogue 0")
    print(f"gemm_h_ex real epilogue 0: worst err / bound {float((err / c.e_v).max()):.4f}")


def test_real_gelu(dev):
    """p = fp16(v): within the fp32 error of v plus one fp16 rounding (2^-11 relative, 2^-25 absolute below the normal range); h against the GELU of the kernel's OWN p
    (an exactly known fp16 argument) within gelu_bound."""
    c = real_case()
    pre, h = launch(_Shim(c), RS, 1, dev, "gemm_h_ex real epilogue 1", ops=real_ops(c, dev))
    p = pre.double().cpu()
    assert_within(p, c.vref, c.e_v + 2.0 ** -11 * (c.vref.abs() + c.e_v) + 2.0 ** -25, "gemm_h_ex real epilogue 1 pre_out")
    assert_within(h.cpu(), G.gelu64(p), G.gelu_bound(p, "exp", "f16"), "gemm_h_ex real epilogue 1 h_out")


def test_real_gated_residual(dev):
    """out = fl(res + fl(v g)): |v g| carries e_v |g|, the product one rounding, the sum one more."""
    c = real_case()
    rpg = 36
    g = c.gate[:(c.M + rpg - 1) // rpg, :c.N].repeat_interleave(rpg, 0)[:c.M].double()
    ref = c.res.double() + c.vref * g
    e_prod = c.e_v * g.abs()
    e_prod = e_prod + U * ((c.vref * g).abs() + e_prod)
    bound = e_prod + U * (ref.abs() + e_prod)
    ops = real_ops(c, dev)
    out = launch(_Shim(c), RS, 2, dev, "gemm_h_ex real epilogue 2", rpg, ops=ops)
    err = assert_within(out.double().cpu(), ref, bound, "gemm_h_ex real epilogue 2")
    print(f"gemm_h_ex real epilogue 2: worst err / bound {float((err / bound).max()):.4f}")
    assert_same(launch(_Shim(c), RS, 2, dev, "gemm_h_ex real epilogue 2 in place", rpg, inplace=True, ops=ops), out, "gemm_h_ex real epilogue 2 in place")


# ------------------------------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_come_before_any_launch(dev):
    lib = E.load_library()
    c = case(33, 128, 96)
    M, N, K = c.M, c.N, c.K
    Xo, Wo, sc, b = operands(c, 0, dev)
    gate = torch.zeros(M * 2 * N + 4, device=dev)
    res = GuardedRows(M, N, N + 8, dev, init=c.res.float())
    out = GuardedRows(M, N, N + 8, dev)

    def call(res_ptr=res.ptr, gate_ptr=_p(gate), rpg=1, n=N, k=K, epi=2):
        return lib.sdvar_op_gemm_h_ex(_p(Xo), _p(Wo), 1, _p(sc), _p(b), out.ptr, N + 8, None, None, res_ptr, N + 8, gate_ptr, rpg, 2 * N, M, n, k, epi, _st())
    assert call(res_ptr=None) == 1 and b"res" in lib.sdvar_last_error()
    assert call(gate_ptr=None) == 1
    assert call(k=K - 16) == 1 and b"K" in lib.sdvar_last_error()
    assert call(n=N - 4) == 1
    assert call(gate_ptr=C.c_void_p(gate.data_ptr() + 4)) == 1 and b"aligned" in lib.sdvar_last_error()
    assert call(rpg=0) == 1 and b"rows_per_gate" in lib.sdvar_last_error()
    assert call(epi=3) == 1
    assert lib.sdvar_op_gemm_h_ex(_p(Xo), _p(Wo), 2, _p(sc), _p(b), out.ptr, N + 8, None, None, None, 0, None, 1, 0, M, N, K, 0, _st()) == 1      # bf16 has no engine tier
    torch.cuda.synchronize()
    out.check_guards("gemm_h_ex argument errors", untouched=True)
    res.check_guards("gemm_h_ex argument errors (res)", untouched=True)
    with pytest.raises(E.SdvarError):                                     # the Python binding reports the same
        E.gemm_h_ex(Xo, Wo, M, N, K, 2, w_scale=sc, bias=b, out=torch.zeros(M, N + 8, device=dev), ldo=N + 8, gate=gate, gate_stride=2 * N)
    E.gemm_h_ex(Xo, Wo, M, N, K, 0, w_scale=sc, bias=b, out=(o := torch.zeros(M, N, device=dev)), ldo=N)
    assert_same(o, c.v.float().to(dev), "engine.gemm_h_ex epilogue 0")
