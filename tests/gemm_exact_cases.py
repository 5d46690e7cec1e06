"""Inputs on which every GEMM kernel of the library has ONE right answer, and the GELU bound that goes with them.  Imports without a GPU
(tests/test_gemm_exact_host.py checks the premises; tests/test_gpu_gemm_exact.py runs the kernels).

Exact-integer cases.  X (M, K) and W (N, K) hold integers in [-3, 3], bias integers in [-8, 8], res in [-64, 64], gate in [-2, 2].  Then
  * every operand is a fixed point of every operand format: fp32, fp16 (the f16x2 activation planes, low plane zero), fp16 after the f16x2 weight scale (max |W| = 3
    is pinned, so the scale is 2^11 and the scaled weights are multiples of 2^11 up to 6144 = 3 * 2^11, exact in 11 significand bits), bf16 (8 bits);
  * every product is an integer of at most 9 and every partial sum of any subset of a dot product, in any order, is an integer of magnitude <= 9 K <= 36864 < 2^24
    for K <= 4096 (with the weight scale: 2^11 times such an integer, the same 24-bit significand), so fp32 accumulation is exact whatever the tile, the K split, the
    ring depth or the MFMA shape;
  * v = acc + bias (|v| <= 36872), v * gate (<= 73744) and res + v * gate (<= 73808) are integers below 2^24 as well: epilogues 0 and 2 are exact, fused or not.
So epilogues 0 and 2 must return the float64 product BIT FOR BIT, and epilogue 1 sees an exactly known v: what is left is the error of the GELU evaluation alone.
One row in three of X has at most two non-zero entries: there |v| <= 2 * 9 + 8 = 26, the curved part of GELU (the other rows reach thousands, where GELU(v) = v or 0).

GELU bound (gelu_bound).  Derived from the operation count of common.h's gelu_tanh / gelu_tanh_h with u = 2^-24 (fp32's unit roundoff); nothing in it comes from a
GPU run.  See the docstrings of gelu_c_tanh and gelu_c_exp.

Graded-scale cases (graded_case).  X = diag(r) A, W = diag(c) B with r, c powers of two: a power-of-two scale commutes with every fp32 / bf16 rounding while nothing
leaves the normal range, so out(X, W) must equal out(A, B) * r_i * c_j bit for bit.  A ~ N(0, 1) and B ~ N(0, 1) / sqrt(K) are snapped to the grids 2^-20 and 2^-25 (a
change of at most 2^-21 resp. 2^-26: still full 23 / 24-bit significands) so that the "nothing underflows" condition can be PROVED for every summation order instead
of hoped for: every product (of the values, of their bf16 roundings or of their bf16x3 planes) is a multiple of 2^-45, hence so is every partial sum, and a non-zero
one is at least 2^-45 in magnitude; graded_chain_floor follows that through the gated-residual epilogue."""
import functools
import math

import numpy as np
import torch

from conftest import rnd

U32 = 2.0 ** -24                      # unit roundoff of fp32
TINY32 = 2.0 ** -126                  # smallest normal fp32
INT_FILL = 0x7FC5A3C1                 # canary of fp32 buffers: as a float a NaN with a payload no kernel produces
HALF_FILL = 0x7E5B                    # canary of 16-bit buffers (an fp16 NaN; as bf16 a finite 2^125-sized number no case reaches)

MS = (1, 33, 80, 130, 257, 300, 700)
NS = (128, 192, 384, 528)
KS = (32, 64, 96, 160, 1024, 4096)    # 1, 2, 3, 5, 32, 128 K-steps


def shape_list(ms=MS, ns=NS, ks=KS, pair_ks=(96, 1024), sweep=(257, 384)):
    """Every (M, N) with K = 96 and K = 1024, and every K with (257, 384)."""
    out = [(m, n, k) for m in ms for n in ns for k in pair_ks]
    out += [(sweep[0], sweep[1], k) for k in ks if (sweep[0], sweep[1], k) not in out]
    return out


def rows_per_gate_for(M, i):
    """1, 5 or 7, rotating with the case index, preferring a value that leaves a ragged last gate group."""
    if M == 1:
        return 1
    order = [(1, 5, 7), (5, 7, 1), (7, 5, 1)][i % 3]
    for r in order:
        if r > 1 and M % r:
            return r
    return order[0]


def weight_scale(W):
    """The f16x2 splitter's weight scale: the power of two that brings max |W| into (2^12, 2^13] (tests/test_gpu_ops.py test_split_planes_f16_accuracy_and_scale)."""
    m = float(W.abs().max())
    S = 13 - math.ceil(math.log2(m)) if m > 0 else 0
    if m * 2.0 ** S <= 2 ** 12:
        S += 1
    assert 2 ** 12 < m * 2.0 ** S <= 2 ** 13
    return 2.0 ** S


class IntCase:
    """One exact-integer case.  Tensors are CPU float32 holding integers; `v` = X W^T + bias in float64 (exact, on BLAS), never modified."""

    def __init__(self, seed, M, N, K):
        g = np.random.Generator(np.random.Philox(key=[seed, 7001]))
        X = g.integers(-3, 4, size=(M, K)).astype(np.float32)
        for i in range(1, M, 3):                                       # the GELU rows: at most two non-zero entries
            X[i] = 0
            cols = g.integers(0, K, size=2)
            X[i, cols] = g.choice(np.array([-3, -2, -1, 1, 2, 3], dtype=np.float32), size=2)
        W = g.integers(-3, 4, size=(N, K)).astype(np.float32)
        # rows 2, 5, 8, .. of X and rows 0, 4, 8, .. of W share one sign pattern (every other such X row negated): their dot products are ~ +-2.9 K instead of
        # ~ 4 sqrt(K), beyond 2048 (256) for K >= 1024 (96), where the fp16 (bf16) outputs of sdvar_op_gemm_h must round
        s = g.choice(np.array([-1, 1], dtype=np.float32), size=K)
        X[2::3] = np.abs(X[2::3]) * s
        X[2::6] *= -1
        W[0::4] = np.abs(W[0::4]) * s
        W[N // 2, K // 2] = 3.0                                        # pins max |W| = 3: the f16x2 weight scale is 2^11
        self.M, self.N, self.K = M, N, K
        self.X, self.W = torch.from_numpy(X), torch.from_numpy(W)
        self.bias = torch.from_numpy(g.integers(-8, 9, size=(N,)).astype(np.float32))
        self.res = torch.from_numpy(g.integers(-64, 65, size=(M, N)).astype(np.float32))
        # gate table: row g of the first N columns gates rows [g * rows_per_gate, ...); the second N columns are other integers, as in the adaLN table the model passes
        self.gate = torch.from_numpy(g.integers(-2, 3, size=(M, 2 * N)).astype(np.float32))
        self.gelu_rows = torch.zeros(M, dtype=torch.bool)
        self.gelu_rows[1::3] = True
        self.v = self.X.double() @ self.W.double().t() + self.bias.double()

    def gate_rows(self, rows_per_gate):
        R = (self.M + rows_per_gate - 1) // rows_per_gate
        return self.gate[:R, :self.N].double().repeat_interleave(rows_per_gate, 0)[:self.M]

    def ref(self, epi, rows_per_gate=1):
        """float64 reference of the epilogue: 0 bias, 1 GELU(tanh) of the exact v, 2 res + v * gate[row / rows_per_gate]."""
        if epi == 0:
            return self.v
        if epi == 1:
            return gelu64(self.v)
        return self.res.double() + self.v * self.gate_rows(rows_per_gate)


@functools.lru_cache(maxsize=None)
def int_case(M, N, K, seed=1):
    return IntCase(seed, M, N, K)


# ---------------------------------------------------------------------------------------------------------------- GELU
K0, K1 = 0.7978845608028654, 0.044715                      # sqrt(2 / pi), and the cubic's coefficient (nn.GELU(approximate='tanh'))
C0_SRC, C1_SRC = -2.3022081986, -0.10294324                # the literals of gelu_tanh_h in common.h
C0_TRUE = -2.0 * math.log2(math.e) * math.sqrt(2.0 / math.pi)
C1_TRUE = K1 * C0_TRUE
TANH_ULPS = 5.0                                            # tanhf is the device library's (OCML, built to the OpenCL full-profile table: tanh <= 5 ulp)


def gelu64(v):
    """GELU(tanh) in float64 in its cancellation-free form v * sigmoid(2 u) = v / (1 + exp(-2 u)), u = sqrt(2/pi) (v + 0.044715 v^3): the same function as
    0.5 v (1 + tanh u), which in float64 loses every digit of (1 + tanh u) beyond v ~ -6 (test_gemm_exact_host.py holds the two together where both are good)."""
    v = v.double()
    z = -2.0 * K0 * (v + K1 * v * v * v)
    return torch.where(z > 700, torch.zeros_like(v), v / (1.0 + torch.exp(z.clamp(max=700.0))))


def _const_err(src, true):
    """Relative error, in units of u, of the fp32 value of a source literal against the constant it stands for."""
    return abs(float(np.float32(src)) - true) / abs(true) / U32


def gelu_c_tanh(v):
    """c(v) of gelu_tanh: 0.5 x (1 + tanhf(k0 (x + k1 x x x))), x = v exact.
      k1 x x x           k1 rounded (1) + three multiplications (3)                                  -> 4 u on the cubic term
      x + (.)            same sign: the relative error of the sum is at most the larger term's, + 1  -> 5 u
      k0 (.)             k0 rounded (1) + one multiplication (1)                                     -> inner has 7 u
      t = tanhf(inner)   the argument's error moves t by (1 - t^2) 7 u |inner|; tanhf itself is good to TANH_ULPS ulp <= 2 TANH_ULPS u |t|
      s = 1 + t          one rounding (1 u of s); relative to s the error of t is divided by (1 + t): (1 - t^2) / (1 + t) = 1 - t
      (0.5 x) s          0.5 x is exact, one multiplication (1)
    c = 2 + 7 (1 - t) |inner| + 2 TANH_ULPS |t| / (1 + t).  For v -> -inf the last term grows without bound - the formula cancels there, and a result of 0 where
    GELU is 1e-30 is within it; the term is capped at 2^24 (bound = |gelu|)."""
    v = v.double()
    inner = K0 * (v + K1 * v * v * v)
    t = torch.tanh(inner)
    one_plus_t = 2.0 / (1.0 + torch.exp((-2.0 * inner).clamp(max=700.0)))          # 1 + tanh without the cancellation
    one_minus_t = 2.0 / (1.0 + torch.exp((2.0 * inner).clamp(max=700.0)))
    canc = (2.0 * TANH_ULPS * t.abs() / one_plus_t.clamp_min(1e-300)).clamp(max=2.0 ** 24)
    return 2.0 + 7.0 * one_minus_t * inner.abs() + canc


def gelu_c_exp(v):
    """c(v) of gelu_tanh_h: w = x fma(x x, C1, C0); e = exp2(w); x rcp(1 + e), x = v exact.
      x x                1 u;  C1 (x x): + C1's literal against 0.044715 C0 (_const_err, < 1);  C0: its literal (_const_err, < 1)
      fma                both terms are negative: the sum's relative error is at most the larger term's, + 1 for the single rounding of the fma
      w = x (.)          + 1                                                                          -> e_w = max(1 + err C1, err C0) + 2  (about 4.5 u)
      e = exp2(w)        v_exp_f32 is good to 1 ulp <= 2 u, and the argument's ABSOLUTE error e_w u |w| is amplified to ln 2 e_w u |w| relative in e
      d = 1 + e          relative to d the error of e weighs e / (1 + e); + 1 for the addition
      rcp(d)             v_rcp_f32: 1 ulp <= 2 u;   x (.)  + 1
    c = e / (1 + e) (2 + ln 2 e_w |w|) + 4."""
    v = v.double()
    e_w = max(1.0 + _const_err(C1_SRC, C1_TRUE), _const_err(C0_SRC, C0_TRUE)) + 2.0
    w = v * (C0_TRUE + C1_TRUE * v * v)
    frac = 1.0 / (1.0 + torch.exp2((-w).clamp(max=1000.0)))                        # e / (1 + e) = 1 / (1 + 2^-w)
    return frac * (2.0 + math.log(2.0) * e_w * w.abs()) + 4.0


def gelu_bound(v, form, out):
    """|got - gelu64(v)| allowed at an exactly known fp32 argument v.  form: 'tanh' (sdvar_op_gemm, sdvar_op_gemm_bf16x3) or 'exp' (sdvar_op_gemm_f16x2,
    sdvar_op_gemm_h).  out: where the value goes -
      'f32'     a float, or the bf16x3 planes, whose three-way split is exact: c(v) u |g|, floor 0;
      'f16x2'   two fp16 planes: + 2^-22 relative (high plane to 2^-11, low plane to 2^-11 of the rest) + the documented 2^-25 absolute (fp16's subnormal half-spacing,
                once the low plane is subnormal: gemm_f16x2.hip header, test_split_planes_f16_accuracy_and_scale);
      'f16' / 'bf16'   one rounding to the half type: unit roundoff 2^-11 / 2^-8 of the computed value, 2^-25 / 2^-134 absolute below the normal range.
    The 'exp' form overflows v_exp_f32 for w > 128, i.e. where |GELU| < 26 * 2^-128 is below fp32's normal range anyway: 2^-126 absolute covers the flush."""
    g = gelu64(v).abs()
    if form == "tanh":
        assert out == "f32"
        return gelu_c_tanh(v) * U32 * g
    e = gelu_c_exp(v) * U32 * g + TINY32
    if out == "f32":
        return e
    if out == "f16x2":
        return e + 2.0 ** -22 * (g + e) + 2.0 ** -25
    uh, sub = {"f16": (2.0 ** -11, 2.0 ** -25), "bf16": (2.0 ** -8, 2.0 ** -134)}[out]
    return e + uh * (g + e) + sub


def gelu_worst_ratio(err, bound, ref):
    """(worst err / bound, the same over the elements whose bound is below half of |gelu| - beyond, on the far left, the tanh form has cancelled to 0 and err / bound
    is 1 by construction).  Reported, never asserted on."""
    ok = bound > 0
    ratio = torch.where(ok, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    sharp = ok & (bound < 0.5 * ref.abs())
    return float(ratio.max()) if ratio.numel() else 0.0, float(ratio[sharp].max()) if bool(sharp.any()) else 0.0


def gelu_tanh_f32(v):
    """gelu_tanh of common.h, operation by operation, in torch float32 on the CPU."""
    x = v.float()
    k0, k1 = torch.tensor(K0, dtype=torch.float32), torch.tensor(K1, dtype=torch.float32)
    inner = k0 * (x + k1 * x * x * x)
    return 0.5 * x * (1.0 + torch.tanh(inner))


def gelu_exp_f32(v):
    """gelu_tanh_h of common.h, operation by operation, in torch float32 on the CPU (the fma through float64: the product of two floats is exact there)."""
    x = v.float()
    c0, c1 = float(np.float32(C0_SRC)), float(np.float32(C1_SRC))
    p = ((x * x).double() * c1 + c0).float()
    w = x * p
    return x * (1.0 / (1.0 + torch.exp2(w)))


# ---------------------------------------------------------------------------------------------------------------- graded scales
R_EXP, C_EXP = (0, 6, -6, -12), (0, 3, -5, -10)
R_EXP_F16X2 = (0, 3, 6)
A_GRID, B_GRID, G_GRID = 20, 25, 20                        # A, res on 2^-20, B on 2^-25, gate on 2^-20


def _snap(t, bits):
    return (t.double() * 2.0 ** bits).round().mul(2.0 ** -bits).float()


class GradedCase:
    def __init__(self, M, N, K, r_exp=R_EXP, c_exp=C_EXP):
        self.M, self.N, self.K = M, N, K
        self.A, self.B = _snap(rnd(21, (M, K)), A_GRID), _snap(rnd(22, (N, K), 1 / math.sqrt(K)), B_GRID)
        self.res0, self.gate = _snap(rnd(23, (M, N)), A_GRID), _snap(rnd(24, (M, 2 * N)), G_GRID)
        self.r_exp = torch.tensor(r_exp)[(torch.arange(M) // 5) % len(r_exp)]               # changes every 5 rows
        self.c_exp = torch.tensor(c_exp)[(torch.arange(N) // 8) % len(c_exp)]               # blocks of 8 columns: one 32-column tile mixes all four
        self.r, self.c = torch.pow(2.0, self.r_exp.double()), torch.pow(2.0, self.c_exp.double())
        self.scale = self.r[:, None] * self.c[None, :]                                       # float64 (M, N), powers of two
        self.X, self.W = (self.A.double() * self.r[:, None]).float(), (self.B.double() * self.c[:, None]).float()
        self.res = (self.res0.double() * self.scale).float()
        self.bias = torch.zeros(N)


@functools.lru_cache(maxsize=None)
def graded_case(M, N, K, f16x2=False):
    return GradedCase(M, N, K, R_EXP_F16X2 if f16x2 else R_EXP)


GRADED_SHAPES = ((257, 384, 1024), (130, 192, 96))


def graded_chain_floor(gc):
    """Smallest magnitude a NON-ZERO intermediate of the unscaled run out(A, B) can have, in any summation order:
      products a b (of fp32 values, of their bf16 roundings, of bf16x3 planes - all multiples of the grids) are multiples of 2^-(A_GRID + B_GRID), rounded or not;
      sums of such multiples are such multiples: a non-zero partial sum, and v, is >= 2^-45;
      v * gate >= 2^-45 * min |gate| >= 2^-65 in magnitude and, once rounded, a multiple of its own ulp >= 2^-24 of that;
      res + v * gate is a multiple of min(2^-20, that ulp): non-zero >= 2^-89.
    Times the smallest scale r c this must stay a normal fp32 (>= 2^-126)."""
    sum_floor = 2.0 ** -(A_GRID + B_GRID)
    gmin = float(gc.gate[gc.gate != 0].abs().min())
    assert gmin >= 2.0 ** -G_GRID
    prod_floor = sum_floor * gmin
    return min(sum_floor, prod_floor * 2.0 ** -24)
