"""Inputs on which every decoder / encoder convolution kernel of csrc/conv.hip has ONE right answer.  Imports without a GPU (tests/test_conv_exact_host.py proves
the premises; tests/test_gpu_conv_exact.py runs the kernels).  The conventions are those of tests/gemm_exact_cases.py: INT_FILL, HALF_FILL, weight_scale.

A case is a convolution (B, Cin, H, W) -> (B, N, Ho, Wo) in one of the forms the library runs:
  src 'prep'     sdvar_op_vae_prep mode 0, up 0, then taps 9 (3x3, pad 1), 1 (1x1) or 4 (the fused nearest-2x up-sampling: four 2x2 phase convolutions on the input grid)
  src 'prep_up'  sdvar_op_vae_prep up 1 (the planes of the up-sampled tensor), then the 3x3 convolution over (2H, 2W)
  src 's2d'      sdvar_op_vae_s2d_planes + sdvar_op_vae_s2d_weights: Downsample2x (pad right / bottom, stride 2) as a 3x3 convolution over the space-to-depth tensor
  src 'img'      sdvar_op_vae_img_planes: the encoder's conv_in, 3 image channels padded to 32
and one of three operand kinds:

'int' - exact integers.  x and w in [-3, 3] (one weight pinned to 3: the f16x2 weight scale is 2^11), bias in [-8, 8], res in [-64, 64].  Every value is a fixed point
  of fp32 and of both splitters (low planes zero), a scaled f16x2 weight is a multiple of the power-of-two scale, and no partial sum of any order reaches 2^24
  (3x3, Cin <= 640: 81 * 640 + 72; the four phase weight sets of sdvar_op_upconv_weights are sums of at most four weights, |weff| <= 12, a phase dot product
  <= 36 * 4 * Cin).  The output of every kernel, loop, split and tile must equal the float64 conv2d bit for bit.

'dense' - f16x2 only; the low planes carry data.  x = a + c 2^-12, w = a' + c' 2^-12 with a, a' in [-2, 2], c, c' in {-1, 0, 1} and c = 0 where a = 0.  (Where a = 0 the
  splitter would put c 2^-12 into the HIGH plane and the hh product of two such values would have grain 2^-24; with a != 0 the high plane is a - a tie at
  |a| = 1, c = -sign(a) rounds to the even neighbour, which is a - and the low plane c 2^-12 is a normal fp16.)  The kernels form hh, hl and lh (never ll): every term
  is a multiple of 2^-12 and every partial sum is below 4.01 * 9 * 96 < 2^12, 24 bits.  One weight is pinned to 2 + 2^-12 (scale 2^11; the scaled low plane is +-1/2).
  With the fused up-sampling the 3x3 weight is non-zero on its four corner taps only: every phase weight is then ONE corner weight, inside the value set (a sum of
  several could cancel to a' = 0, c' != 0).

'sparse' - the low planes carry data and every dot product is short: x is non-zero only on the pixel lattice (y % 3 == 1, x % 3 == 1) - a 3x3 window (a 2x2 window
  of the up-sampling phases) holds at most one lattice pixel - and there on at most 7 channels spread over all channel blocks; w is dense.  Each output is ONE known tap
  of ONE known pixel, which pins the tap geometry.
    bf16x3: values s (1 + b 2^-10 + c 2^-20), s = +-1, b, c in {0, 1}, c <= b.  split3 TRUNCATES, so the planes are (s, s b 2^-10, s c 2^-20) only for same-sign
            nested values (1 - 2^-10 would split as 1 - 2^-8, 3 * 2^-10: grains 2^-8 and 2^-10, and a (1, 1) product at 2^-20 * 2^-2 ...); with them the six products the
            kernel forms - (0,0) (0,1) (1,0) (0,2) (1,1) (2,0), never (1,2) (2,1) (2,2) - are multiples of 2^-20 and 7 terms below 1.01 stay below 2^3: 23 bits.
            bias and res are integers in [-4, 4] here: 7.02 + 8 < 2^4, 24 bits.
    f16x2:  the 'dense' value set on the lattice.
The reference of 'dense' and 'sparse' is the float64 sum of exactly the plane products the kernels form (PRODUCTS), of the planes the host model of the splitters
gives (split_f16x2, split_bf16x3 - the GPU test reads the producers' planes back and holds them to this model bit for bit), divided by the weight scale.

prove_exact() shows (max |partial sum|) / grain < 2^24 for a case from its operand planes alone: the grain of a plane is the largest power of two that divides all
its elements, a product's grain the product of the two, and no partial sum of any subset in any order exceeds sum |x plane| * |w plane| + |bias| + |res|."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from gemm_exact_cases import HALF_FILL, INT_FILL, weight_scale  # noqa: F401  (re-exported: the conv tests use the GEMM tests' canaries and scale rule)

PRODUCTS = {2: ((0, 0), (0, 1), (1, 0)),                                   # (x plane, w plane): conv_f16x2_kernel (all three loops) and conv_f16x2_reuse_kernel
            3: ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))}           # conv_bf16x3_kernel
NPL = {2: 2, 3: 3}
CBM, CBN = 256, 160                                                        # workgroup tile of conv.hip
_UP_ROWS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}    # (phase bit, tap bit) -> 3x3 kernel rows / columns summed (upconv_weight_kernel)


# ---------------------------------------------------------------------------------------------------------------- host models of the splitters
def split_f16x2(v):
    """common.h split2h: h = fp16(v) to nearest even, l = fp16(v - h).  v float32 -> [h, l] as float32."""
    v = v.float()
    h = v.half().float()
    return [h, (v - h).half().float()]


def split_bf16x3(v):
    """common.h split3: p0 = v truncated to its upper 16 bits, p1 = (v - p0) truncated, p2 = the rest.  v float32 -> [p0, p1, p2] as float32."""
    def trunc(t):
        return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)
    v = v.float()
    p0 = trunc(v)
    r1 = v - p0
    p1 = trunc(r1)
    return [p0, p1, trunc(r1 - p1)]


def split(v, pf):
    return split_f16x2(v) if pf == 2 else split_bf16x3(v)


def plane_bits(p, pf):
    """float32 plane values (exactly representable in the plane's type) -> the 16-bit words the library stores"""
    if pf == 2:
        return p.half().view(torch.int16)
    return (p.contiguous().view(torch.int32) >> 16).to(torch.int16)


def guard_rows(W):
    return (W + 3 + 15) // 16 * 16


def x_plane_words(planes, pf, G):
    """planes: NPL float32 tensors (B, C, H, W) -> int16 words [NPL][C / 32][G + B (H + 2)(W + 2) + G][32], zero frame and zero guards (the producers' layout)"""
    B, C, H, W = planes[0].shape
    out = []
    for p in planes:
        t = F.pad(plane_bits(p, pf), (1, 1, 1, 1))                                    # (B, C, H + 2, W + 2)
        t = t.permute(1, 0, 2, 3).reshape(C // 32, 32, B * (H + 2) * (W + 2)).permute(0, 2, 1)
        out.append(F.pad(t, (0, 0, G, G)))
    return torch.stack(out).contiguous()


def w_plane_words(planes, pf):
    """planes: NPL float32 tensors (N, Cin, kh, kw) -> int16 words [NPL][taps Cin / 32][N][32], k = tap Cin + cin (conv_weight_planes_kernel)"""
    N, Cin, kh, kw = planes[0].shape
    out = [plane_bits(p, pf).permute(0, 2, 3, 1).reshape(N, kh * kw * Cin // 32, 32).permute(1, 0, 2) for p in planes]
    return torch.stack(out).contiguous()


def upconv_weff(w):
    """upconv_weight_kernel on the host: w (N, Cin, 3, 3) -> weff (4 phases, N, Cin, 2, 2) in float32, summed in the kernel's order (our sums are exact in any order)"""
    N, Cin = w.shape[:2]
    weff = torch.zeros(4, N, Cin, 2, 2)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    for ky in _UP_ROWS[(py, ty)]:
                        for kx in _UP_ROWS[(px, tx)]:
                            weff[2 * py + px, :, :, ty, tx] += w[:, :, ky, kx]
    return weff


def s2d_tensor(x):
    """(B, C, H, W) -> the space-to-depth tensor (B, 4C, H / 2, W / 2), channel (2 py + px) C + c = x[2y + py][2x + px][c]"""
    return torch.cat([x[:, :, py::2, px::2] for py in range(2) for px in range(2)], 1)


def s2d_weight(w):
    """s2d_weight_kernel on the host: (N, C, 3, 3) -> (N, 4C, 3, 3)"""
    N, C = w.shape[:2]
    w2 = torch.zeros(N, 4 * C, 3, 3)
    for py in range(2):
        for px in range(2):
            for dy in (0, 1):
                for dx in (0, 1):
                    ky, kx = 2 * dy + py, 2 * dx + px
                    if ky <= 2 and kx <= 2:
                        w2[:, (2 * py + px) * C:(2 * py + px + 1) * C, dy + 1, dx + 1] = w[:, :, ky, kx]
    return w2


# ---------------------------------------------------------------------------------------------------------------- cases
def _rng(*key):
    return np.random.Generator(np.random.Philox(np.random.SeedSequence(list(key))))


def _ints(g, lo, hi, shape):
    return torch.from_numpy(g.integers(lo, hi + 1, size=shape).astype(np.float32))


def _dense_f16(g, shape):
    """a + c 2^-12, a in [-2, 2], c in {-1, 0, 1}, c = 0 where a = 0"""
    a = g.integers(-2, 3, size=shape)
    c = g.integers(-1, 2, size=shape) * (a != 0)
    return torch.from_numpy((a + c * 2.0 ** -12).astype(np.float32))


def _nested_bf16(g, shape, zeros=False):
    """s (1 + b 2^-10 + c 2^-20), c <= b; zeros: one value in four is 0"""
    s = g.choice(np.array([-1.0, 1.0]), size=shape)
    lvl = g.integers(0, 3, size=shape)                               # 0: 1, 1: 1 + 2^-10, 2: 1 + 2^-10 + 2^-20
    v = s * (1.0 + (lvl >= 1) * 2.0 ** -10 + (lvl >= 2) * 2.0 ** -20)
    if zeros:
        v = v * (g.integers(0, 4, size=shape) != 0)
    return torch.from_numpy(v.astype(np.float32))


class ConvCase:
    """kind 'int' | 'dense' | 'sparse'; pf: the plane format the values are made for (None: every format - 'int').  Tensors are CPU float32 and never modified."""

    def __init__(self, kind, pf, B, H, W, Cin, N, taps=9, src="prep", seed=1):
        assert kind in ("int", "dense", "sparse") and src in ("prep", "prep_up", "s2d", "img") and taps in (1, 4, 9)
        self.kind, self.pf, self.B, self.H, self.W, self.Cin, self.N, self.taps, self.src = kind, pf, B, H, W, Cin, N, taps, src
        self.up = taps == 4
        g = _rng(seed, 9001, B, H, W, Cin, N, taps)
        k = 1 if taps == 1 else 3
        # ---- the tensor the conv kernel sees (xk: B, Cin, Hk, Wk) and the weight the test hands to the library (w)
        if src == "s2d":                                             # the caller's tensor is (B, Cin / 4, 2H, 2W); H, W are those of the space-to-depth tensor
            self.x_in = _ints(g, -3, 3, (B, Cin // 4, 2 * H, 2 * W))
            self.w_in = _ints(g, -3, 3, (N, Cin // 4, 3, 3))
            self.w_in[N // 2, 0, 0, 0] = 3.0                         # tap (0, 0) survives in phase (0, 0): max |w_s2d| = 3
            self.xk, self.w = s2d_tensor(self.x_in), s2d_weight(self.w_in)
        elif src == "img":
            self.x_in = _ints(g, -3, 3, (B, 3, H, W))
            self.w_in = _ints(g, -3, 3, (N, 3, 3, 3))
            self.w_in[N // 2, 1, 1, 1] = 3.0
            self.xk, self.w = F.pad(self.x_in, (0, 0, 0, 0, 0, Cin - 3)), F.pad(self.w_in, (0, 0, 0, 0, 0, Cin - 3))
        else:
            if kind == "int":
                x, w = _ints(g, -3, 3, (B, Cin, H, W)), _ints(g, -3, 3, (N, Cin, k, k))
                w[N // 2, Cin // 2] = 3.0                            # every tap of one (cout, cin): max |w| = 3, and max |weff| = 12 with the fused up-sampling
            elif kind == "dense":
                x, w = _dense_f16(g, (B, Cin, H, W)), _dense_f16(g, (N, Cin, k, k))
                w[N // 2, Cin // 2] = 2.0 + 2.0 ** -12
            else:
                val = (lambda shape, zeros=False: _dense_f16(g, shape)) if pf == 2 else (lambda shape, zeros=False: _nested_bf16(g, shape, zeros))
                x = torch.zeros(B, Cin, H, W)
                for b in range(B):
                    for y in range(1, H, 3):
                        for xx in range(1, W, 3):
                            cb = Cin // 32
                            ch = [32 * (i % cb) + int(g.integers(0, 32)) for i in range(7)]          # <= 7 channels, every channel block taken
                            x[b, ch, y, xx] = val((len(ch),))
                w = val((N, Cin, k, k), True)
                if pf == 2:
                    w[N // 2, Cin // 2] = 2.0 + 2.0 ** -12
            if self.up and kind != "int":                           # corner taps only: each phase weight is one corner weight
                keep = torch.zeros(3, 3)
                keep[0::2, 0::2] = 1.0
                w = w * keep
            self.x_in, self.w_in, self.w = x, w, w
            self.xk = F.interpolate(x, scale_factor=2, mode="nearest") if src == "prep_up" else x
        self.Hk, self.Wk = self.xk.shape[2:]                         # what the conv kernel is told (H, W)
        self.Ho, self.Wo = (2 * self.Hk, 2 * self.Wk) if self.up else (self.Hk, self.Wk)
        self.M, self.Mo = B * self.Hk * self.Wk, B * self.Ho * self.Wo
        small = kind == "sparse" and pf == 3
        self.bias = _ints(g, -4 if small else -8, 4 if small else 8, (N,))
        self.res = None if self.up else _ints(g, -4 if small else -64, 4 if small else 64, (B, N, self.Ho, self.Wo))
        self.weff = upconv_weff(self.w) if self.up else None         # (4, N, Cin, 2, 2)
        self._refs = {}

    @property
    def id(self):
        return f"{self.kind}{'' if self.pf is None else self.pf}_{self.src}_B{self.B}_{self.H}x{self.W}_{self.Cin}-{self.N}_t{self.taps}"

    # the weight tensor whose planes the kernel multiplies: w (N, Cin, k, k), or the phase weights (4 N, Cin, 2, 2) with the fused up-sampling
    def kernel_weight(self):
        return self.weff.reshape(4 * self.N, self.Cin, 2, 2) if self.up else self.w

    def scale(self, pf):
        """the f16x2 weight scale (one over the whole tensor, all four phases included); 1 for bf16x3"""
        return weight_scale(self.kernel_weight()) if pf == 2 else 1.0

    def x_planes(self, pf):
        return split(self.xk, pf)

    def w_planes(self, pf):
        """planes of (kernel weight * scale), float32"""
        return split(self.kernel_weight() * self.scale(pf), pf)

    def _conv(self, xp, wq):
        """float64 convolution of one x plane with one w plane, in the kernel's form -> (B, N, Ho, Wo)"""
        xp, wq = xp.double(), wq.double()
        if not self.up:
            return F.conv2d(xp, wq, padding=1 if self.taps == 9 else 0)
        out = torch.zeros(self.B, self.N, self.Ho, self.Wo, dtype=torch.float64)
        full = F.conv2d(F.pad(xp, (1, 1, 1, 1)), wq)                 # (B, 4N, H + 1, W + 1): full[y', x'] = sum_t w[ty, tx] x[y' - 1 + ty, x' - 1 + tx]
        for py in range(2):
            for px in range(2):
                ph = 2 * py + px
                out[:, :, py::2, px::2] = full[:, ph * self.N:(ph + 1) * self.N, py:py + self.Hk, px:px + self.Wk]
        return out

    def plane_sum(self, pf, absolute=False):
        """float64 sum over PRODUCTS[pf] of conv(x plane, w plane) / scale; absolute: of the planes' magnitudes (the bound of every partial sum)"""
        xs, ws = self.x_planes(pf), self.w_planes(pf)
        tot = None
        for i, j in PRODUCTS[pf]:
            if not bool(xs[i].any()) or not bool(ws[j].any()):
                continue
            t = self._conv(xs[i].abs(), ws[j].abs()) if absolute else self._conv(xs[i], ws[j])
            tot = t if tot is None else tot + t
        return tot / self.scale(pf)

    def conv2d64(self):
        """the plain float64 conv2d of the operation (no planes) -> (B, N, Ho, Wo), without bias"""
        if self.src == "s2d":
            return F.conv2d(F.pad(self.x_in.double(), (0, 1, 0, 1)), self.w_in.double(), stride=2)
        if self.src == "img":
            return F.conv2d(self.x_in.double(), self.w_in.double(), padding=1)
        xin = F.interpolate(self.x_in.double(), scale_factor=2, mode="nearest") if (self.up or self.src == "prep_up") else self.x_in.double()
        return F.conv2d(xin, self.w_in.double(), padding=0 if self.taps == 1 else 1)

    def ref(self, pf, res):
        """float64 (B, N, Ho, Wo): 'int' - conv2d + bias (+ res), the same for every format; else the plane-product sum of format pf.  Cached, never modified."""
        key = ("int" if self.kind == "int" else pf, bool(res))
        if key not in self._refs:
            base = self.conv2d64() if self.kind == "int" else self.plane_sum(pf)
            r = base + self.bias.double()[None, :, None, None]
            if res:
                r = r + self.res.double()
            self._refs[key] = r
        return self._refs[key]


def grain_log2(t):
    """largest e with every element of t a multiple of 2^e (t float32 / float64, not all zero)"""
    t = t.double()
    m, ex = np.frexp(t[t != 0].numpy())                               # t = m 2^ex, 0.5 <= |m| < 1: m 2^53 is an integer
    mi = np.abs(np.ldexp(m, 53)).astype(np.int64)
    tz = np.log2((mi & -mi).astype(np.float64)).astype(np.int64)      # trailing zero bits of that integer
    return int((ex - 53 + tz).min())


def prove_exact(case, pf):
    """(max |partial sum| bound, grain, bits) of the case in format pf, from the operand planes alone - see the module docstring.  Everything is taken at the scale of
    the accumulator (scaled weights): the epilogue's multiplication by 2^-S is exact."""
    xs, ws = case.x_planes(pf), case.w_planes(pf)
    S = case.scale(pf)
    e = 0                                                             # bias and res are integers: grain 2^0 after the scale is undone, i.e. S before
    for i, j in PRODUCTS[pf]:
        if bool(xs[i].any()) and bool(ws[j].any()):
            e = min(e, grain_log2(xs[i]) + grain_log2(ws[j]) - int(math.log2(S)))
    bound = float(case.plane_sum(pf, absolute=True).max()) + float(case.bias.abs().max()) + (float(case.res.abs().max()) if case.res is not None else 0.0)
    return bound, 2.0 ** e, math.log2(bound / 2.0 ** e)


@functools.lru_cache(maxsize=None)
def case(kind, pf, B, H, W, Cin, N, taps=9, src="prep"):
    return ConvCase(kind, pf, B, H, W, Cin, N, taps, src)


# (B, H, W, Cin, N, taps, src)
INT_SHAPES = [
    (1, 1, 1, 32, 32, 9, "prep"),            # M = 1: one pixel, eight frame neighbours
    (1, 1, 33, 32, 48, 9, "prep"),           # M = 33: one wave and one row of the next; N tail inside the second 32-column MFMA tile
    (1, 3, 85, 64, 32, 9, "prep"),           # M = 255: the last row of the tile is dead
    (1, 257, 1, 32, 32, 9, "prep"),          # M = 257: a second tile of one row; W = 1: both dx neighbours are frame
    (3, 6, 7, 96, 160, 9, "prep"),           # image boundaries inside a tile, rows that wrap inside a wave's 32 rows; 3 channel blocks (both ring depths wrap); N = one tile
    (2, 1, 256, 32, 200, 9, "prep"),         # H = 1; two N tiles, the second with a tail; tap-reuse eligible
    (2, 5, 1, 160, 32, 9, "prep"),           # W = 1; 5 channel blocks
    (1, 5, 9, 64, 90, 9, "prep"),            # N % 4 != 0: conv_pp 2 falls back to 1, no split
    (1, 4, 5, 32, 320, 9, "prep"),           # N = two full tiles
    (1, 3, 5, 640, 32, 9, "prep"),           # Cin = 640: 180 K-steps
    (2, 5, 7, 160, 48, 1, "prep"),           # 1x1: 5 K-steps (a split of 3 is ragged: 2, 2, 1)
    (1, 17, 16, 64, 160, 1, "prep"),         # 1x1, two tiles with a tail
    (2, 3, 5, 64, 48, 4, "prep"),            # fused up-sampling, odd H and W, all four phases
    (1, 3, 3, 32, 90, 4, "prep"),            # the same with N % 4 != 0
    (1, 3, 5, 32, 32, 9, "prep_up"),         # prep with up = 1, then 3x3 over (6, 10)
    (1, 3, 5, 32, 48, 9, "s2d"),             # Downsample2x of (1, 8, 6, 10)
    (2, 5, 7, 32, 32, 9, "img"),             # conv_in: 3 channels padded to 32
    # fused GroupNorm statistics: H W % 256 == 0, N in {128, 160, 320}
    (2, 16, 16, 32, 128, 9, "prep"),
    (1, 16, 16, 64, 160, 9, "prep"),
    (1, 8, 32, 32, 320, 9, "prep"),
    # the shapes of test_gpu_conv_tap_reuse.py CASES (TAP_REUSE_SHAPES below) not listed above
    (1, 4, 64, 32, 32, 9, "prep"),
    (2, 2, 128, 64, 160, 9, "prep"),
    (1, 1, 512, 32, 48, 9, "prep"),
    (1, 2, 128, 96, 160, 9, "prep"),
    (1, 2, 128, 64, 160, 4, "prep"),
    (1, 3, 100, 32, 32, 9, "prep"),
]
TAP_REUSE_SHAPES = [(1, 4, 64, 32, 32, 9), (2, 2, 128, 64, 160, 9), (2, 1, 256, 32, 200, 9), (1, 1, 512, 32, 48, 9), (1, 2, 128, 96, 160, 9), (1, 2, 128, 64, 160, 4),
                    (1, 3, 100, 32, 32, 9)]
DENSE_SHAPES = [                             # f16x2 only
    (1, 5, 7, 32, 48, 9, "prep"),            # one tile
    (2, 3, 5, 64, 200, 9, "prep"),           # two N tiles
    (1, 3, 5, 96, 32, 9, "prep"),            # Cin = 96: the bound's longest dot product
    (1, 3, 5, 64, 48, 4, "prep"),            # the up-sampling taps
    (1, 4, 64, 32, 48, 9, "prep"),           # tap-reuse eligible
    (1, 2, 128, 32, 32, 4, "prep"),          # tap-reuse eligible, up-sampling taps
]
SPARSE_SHAPES = [
    (1, 7, 8, 64, 48, 9, "prep"),            # one tile
    (2, 4, 10, 96, 200, 9, "prep"),          # two N tiles, two images
    (1, 4, 5, 64, 32, 4, "prep"),            # the up-sampling taps
    (1, 4, 64, 32, 32, 9, "prep"),           # tap-reuse eligible (f16x2)
]


def int_cases():
    return [case("int", None, *s) for s in INT_SHAPES]


def split_plane_cases(pf):
    out = [case("sparse", pf, *s) for s in SPARSE_SHAPES]
    if pf == 2:
        out = [case("dense", 2, *s) for s in DENSE_SHAPES] + out
    return out


# ---------------------------------------------------------------------------------------------------------------- what must run (the header's rules, not conv.hip's code)
def expected_slices(force_split, nkt):
    """K slices a forced split comes out as: clipped to the K-steps, no empty trailing slice"""
    s = max(1, min(force_split, nkt))
    kps = -(-nkt // s)
    return -(-nkt // kps)


def stats_fuse(c, split):
    return split == 1 and (c.Hk * c.Wk) % CBM == 0 and c.N % 32 == 0 and CBN % (c.N // 32) == 0


def tap_reuse_eligible(c, pf, pp_used, reuse, split):
    W, HW = c.Wk, c.Hk * c.Wk
    return pf == 2 and pp_used == 2 and reuse == 1 and c.taps in (9, 4) and split == 1 and HW % CBM == 0 and (W % CBM == 0 or (CBM % W == 0 and W >= 64))
