"""GPU: every GEMM kernel of the library on inputs with ONE right answer (tests/gemm_exact_cases.py; premises checked without a GPU in test_gemm_exact_host.py).

Exact-integer cases: operands in [-3, 3] are fixed points of every operand format and no partial sum can round, so epilogues 0 (bias) and 2 (gated residual) must
equal the float64 product bit for bit - for any tile, K split, ring depth, accumulation order or MFMA shape.  Epilogue 1 (GELU) then sees an exactly known argument
and is held to a bound DERIVED from the operation count of its formula (gemm_exact_cases.gelu_bound); torch float32 on the CPU, evaluating the same formula, is held
to the same bound in the same test, and the worst err / bound is printed (recorded in DESIGN.md section 4a, never used as a bar).

Canaries: every output lives inside a larger buffer pre-filled with a fixed bit pattern - 8 guard rows before and after `out`, 4 padding columns per row (ldo = N + 4)
where the entry point takes ldo > N, guard blocks around and between output planes, the same around a separate `res`.  After the launch every guard word must still
hold the pattern, and an interior element that was never written shows up as the pattern (a NaN), not as a plausible number.  Failures name the first (row, column).

Kernel proof: each case asserts that the intended kernel ran - sdvar_debug_get_gemm_cfg after an f16x2 / row-block call (kernel code, K split, hybrid-tail launches),
sdvar_debug_plan_gemm under the same forcing for fp32 and bf16x3 (their launchers execute exactly that plan; they keep no launch counters).  sdvar_op_gemm_h has one
kernel and no planner.

Graded scales: X = diag(r) A, W = diag(c) B with powers of two r, c.  fp32, bf16x3 and the bf16 half GEMM must return out(A, B) * r_i * c_j bit for bit; f16x2 (one
power-of-two scale per weight tensor, unscaled activations) is held per element to the project's 2e-5 bar on the NORMALISED output, so a small-scale block cannot
hide behind a large one."""
import ctypes as C

import pytest
import torch

import gemm_exact_cases as G
from sdvar_amd import engine as E
from test_gpu_ops import VARIANTS, _p, _planes, _planes_h, _st

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

GUARD_ROWS, GUARD_WORDS = 8, 64
SHAPES = G.shape_list()
SKINNY_SHAPES = G.shape_list(ms=(1, 33, 80), ns=(16, 128, 528), sweep=(33, 128))
HYBRID_SHAPES = [(2704, 3072, 256), (2700, 3200, 256)]
SPLITS = (1, 2, 3, 5)
WORST = {}            # (mode, what) -> worst ratio seen, printed by the tests that update it


# ------------------------------------------------------------------------------------------------------------------------ guarded buffers
class GuardedRows:
    """A row-major (M, N) output with leading dimension ld inside GUARD_ROWS rows of fill on both sides; words = torch.int32 (fp32 data) or torch.int16 (half data)."""

    def __init__(self, M, N, ld, dev, words=torch.int32, init=None):
        self.M, self.N, self.ld, self.fill = M, N, ld, (G.INT_FILL if words == torch.int32 else G.HALF_FILL)
        self.buf = torch.full((M + 2 * GUARD_ROWS, ld), self.fill, dtype=words, device=dev)
        if init is not None:
            self.buf[GUARD_ROWS:GUARD_ROWS + M, :N] = init.to(dev).contiguous().view(words)
        self.before = self.buf.clone() if init is not None else None
        self.ptr = C.c_void_p(self.buf.data_ptr() + GUARD_ROWS * ld * self.buf.element_size())          # 8 rows of 4- or 2-byte words: 16-byte aligned for any ld

    def interior(self, dtype=torch.float32):
        return self.buf[GUARD_ROWS:GUARD_ROWS + self.M, :self.N].contiguous().view(dtype)

    def check_guards(self, what, untouched=False):
        """Every guard row and padding column still holds the fill; untouched: the interior is what it was, too (a separate `res`, an output the epilogue does not use)."""
        if untouched:
            bad = self.buf != (self.before if self.before is not None else self.fill)
        else:
            bad = self.buf != self.fill
            bad[GUARD_ROWS:GUARD_ROWS + self.M, :self.N] = False
        if bool(bad.any()):
            r, c = bad.nonzero()[0].tolist()
            raise AssertionError(f"{what}: {int(bad.sum())} word(s) outside the output were written; first at row {r - GUARD_ROWS}, column {c} (M = {self.M}, N = {self.N}, ld = {self.ld})")


class GuardedPlanes:
    """P K-blocked planes (N / 32, M, 32) of 16-bit words with GUARD_WORDS of fill before, between and after them."""

    def __init__(self, P, M, N, dev):
        self.P, self.M, self.N, self.n = P, M, N, M * N
        self.stride = self.n + GUARD_WORDS
        self.buf = torch.full((GUARD_WORDS + P * self.stride,), G.HALF_FILL, dtype=torch.int16, device=dev)
        self.ptr = C.c_void_p(self.buf.data_ptr() + 2 * GUARD_WORDS)

    def plane(self, k):
        o = GUARD_WORDS + k * self.stride
        return self.buf[o:o + self.n].view(self.N // 32, self.M, 32)

    def check_guards(self, what, untouched=False):
        bad = self.buf != G.HALF_FILL
        if not untouched:
            for k in range(self.P):
                o = GUARD_WORDS + k * self.stride
                bad[o:o + self.n] = False
        if bool(bad.any()):
            raise AssertionError(f"{what}: {int(bad.sum())} word(s) outside the output planes were written; first at word {int(bad.nonzero()[0]) - GUARD_WORDS} "
                                 f"(plane stride {self.stride}, plane size {self.n})")

    def value(self, fmt, what):
        """float64 (M, N) sum of the planes; fmt 'f16' | 'bf16'.  A word of the first plane that still holds the fill was never written."""
        hi = self.plane(0).permute(1, 0, 2).reshape(self.M, self.N)
        unwritten = hi == G.HALF_FILL
        if bool(unwritten.any()):
            r, c = unwritten.nonzero()[0].tolist()
            raise AssertionError(f"{what}: {int(unwritten.sum())} plane element(s) never written; first at ({r}, {c})")
        if fmt == "f16":
            v = sum(self.plane(k).view(torch.float16).double() for k in range(self.P))
        else:
            v = sum((self.plane(k).to(torch.int32) << 16).view(torch.float32).double() for k in range(self.P))
        return v.permute(1, 0, 2).reshape(self.M, self.N)


def assert_same(got, ref, what):
    """got == ref element for element (both on the device, same dtype); names the first bad (row, column)."""
    if torch.equal(got, ref):
        return
    bad = (got != ref) | torch.isnan(got)
    r, c = bad.nonzero()[0].tolist()
    nanfill = bool(torch.isnan(got[r, c]))
    raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ; first at ({r}, {c}): got {got[r, c].item()!r}"
                         f"{' (the fill pattern: never written)' if nanfill else ''}, exact {ref[r, c].item()!r}")


def assert_within(got, ref, bound, what):
    err = (got - ref).abs()
    bad = ~(err <= bound)                   # NaN-safe
    if bool(bad.any()):
        r, c = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements miss the bound; first at ({r}, {c}): got {got[r, c].item()!r}, reference {ref[r, c].item()!r}, "
                             f"bound {bound[r, c].item():.3e}")
    return err


# ------------------------------------------------------------------------------------------------------------------------ operands and references on the device
_OPS, _REFS = {}, {}


def device_ops(c, dev, key=None, f16x2_only=False):
    """The operands of an IntCase / GradedCase in every format, uploaded and split once per case."""
    key = key or ("int", c.M, c.N, c.K)
    if key not in _OPS:
        o = dict(M=c.M, N=c.N, K=c.K, X32=c.X.to(dev), W32=c.W.to(dev), res=c.res, gate=c.gate.to(dev).contiguous())
        o["bias1"] = torch.cat([torch.zeros(1), c.bias]).to(dev)                 # bias1[1:] is the bias 4 bytes off the 16-byte grid
        o["bias"] = c.bias.to(dev)
        o["gate1"] = torch.cat([c.gate, torch.zeros(c.M, 1)], 1).to(dev).contiguous()     # the same table with an odd stride
        o["Xh"], _ = _planes_h(c.X, dev)
        o["Wh"], o["sc"] = _planes_h(c.W, dev, scaled=True)
        if not f16x2_only:
            o["Xb"], o["Wb"] = _planes(c.X, dev), _planes(c.W, dev)
        _OPS[key] = o
    return _OPS[key]


def int_ref(c, epi, rpg, dev):
    key = (c.M, c.N, c.K, epi, rpg)
    if key not in _REFS:
        _REFS[key] = c.ref(epi, rpg).float().to(dev)
    return _REFS[key]


def gelu_ref(c, form, out, dev):
    """(gelu64(v), bound) on the device, and - once per case and form - the CPU float32 evaluation of the same formula against the fp32 bound."""
    key = (c.M, c.N, c.K, form, out)
    if key not in _REFS:
        if (c.M, c.N, c.K, form, "cpu") not in _REFS:
            fn = G.gelu_tanh_f32 if form == "tanh" else G.gelu_exp_f32
            ref, b32 = G.gelu64(c.v), G.gelu_bound(c.v, form, "f32")
            err = (fn(c.v).double() - ref).abs()
            assert bool((err <= b32).all()), f"torch float32 on the CPU misses the derived bound of the {form} form: {float((err / b32.clamp_min(1e-300)).max())}"
            note_ratio(("cpu float32", form), err, b32, ref)
            _REFS[(c.M, c.N, c.K, form, "cpu")] = True
        _REFS[key] = (G.gelu64(c.v).to(dev), G.gelu_bound(c.v, form, out).to(dev))
    return _REFS[key]


def drop_cached(M, N, K):
    """Forget the device operands and references of one (large) shape."""
    for cache in (_OPS, _REFS):
        for key in [k for k in cache if (M, N, K) in (k[:3], k[1:4])]:
            del cache[key]


def note_ratio(key, err, bound, ref):
    worst, sharp = G.gelu_worst_ratio(err, bound, ref)
    w = WORST.setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], worst), max(w[1], sharp)


def print_ratios(*prefixes):
    for key, (worst, sharp) in sorted(WORST.items()):
        if key[0] in prefixes:
            print(f"GELU err / bound, {key[0]} ({key[1]} form): worst {worst:.3f}; {sharp:.3f} where the bound is below |gelu| / 2")


# ------------------------------------------------------------------------------------------------------------------------ planner / launch proof
def kernel_plan(mode, M, N, K, vec=True):
    out4 = (C.c_int32 * 4)()
    E._check(E.load_library().sdvar_debug_plan_gemm(mode, M, N, K, 4 if vec else 0, out4))
    return list(out4)


def slices(split, K):
    """K slices a forced split comes out as: clipped to the K-steps, no empty trailing slice (a short last slice is fine)."""
    nkt = K // 32
    s = max(1, min(split, nkt))
    kps = -(-nkt // s)
    return -(-nkt // kps)


def skinny_slices(split, K):
    nkt = K // 32
    sp = max(-(-nkt // 32), split)
    kps = -(-nkt // sp)
    return -(-nkt // kps)


class forced:
    """sdvar_debug_set_gemm_cfg(bm, split) for the duration of a block."""

    def __init__(self, bm, split):
        self.cfg = (bm, split)

    def __enter__(self):
        E._check(E.load_library().sdvar_debug_set_gemm_cfg(*self.cfg))

    def __exit__(self, *exc):
        E._check(E.load_library().sdvar_debug_set_gemm_cfg(0, 0))


class variant:
    def __init__(self, name, value):
        self.name, self.value = name.encode(), value

    def __enter__(self):
        E._check(E.load_library().sdvar_debug_set_variant(self.name, self.value))

    def __exit__(self, *exc):
        E._check(E.load_library().sdvar_debug_set_variant(self.name, -1))


# ------------------------------------------------------------------------------------------------------------------------ one guarded launch
def launch(kind, o, epi, rpg, dev, what, res=None, inplace=False, unaligned=False):
    """One call of sdvar_op_gemm (kind 'f32'), _bf16x3, _f16x2 or _rowblk on the operands `o` into guarded buffers.  Returns the result - float32 (M, N) on the device,
    or float64 for plane outputs - after every guard has been checked.  res: CPU float32 (M, N), default o['res']; inplace: res IS out (as the model calls it)."""
    lib = E.load_library()
    M, N, K = o["M"], o["N"], o["K"]
    ld = N + 3 if unaligned else N + 4
    ldres = N + 5 if unaligned else N + 8
    res = o["res"] if res is None else res
    to_planes = epi == 1 and kind != "f32"
    out = GuardedRows(M, N, ld, dev, init=res if (epi == 2 and inplace) else None)
    outp = GuardedPlanes(3 if kind == "bf16x3" else 2, M, N, dev) if to_planes else None
    resb = None
    if epi == 2:
        resb = out if inplace else GuardedRows(M, N, ldres, dev, init=res)
    bias = C.c_void_p(o["bias1"].data_ptr() + 4) if unaligned else _p(o["bias"])
    gate, gs = (o["gate1"], 2 * N + 1) if unaligned else (o["gate"], 2 * N)
    tail = (epi, resb.ptr if resb else None, resb.ld if resb else N, _p(gate) if epi == 2 else None, rpg, gs, _st())
    pp, ps = (outp.ptr, outp.stride) if outp else (None, 0)
    if kind == "f32":
        E._check(lib.sdvar_op_gemm(_p(o["X32"]), K, _p(o["W32"]), bias, out.ptr, ld, M, N, K, *tail))
    elif kind == "bf16x3":
        E._check(lib.sdvar_op_gemm_bf16x3(_p(o["Xb"]), M * K, _p(o["Wb"]), N * K, bias, out.ptr, ld, pp, ps, M, N, K, *tail))
    elif kind == "f16x2":
        E._check(lib.sdvar_op_gemm_f16x2(_p(o["Xh"]), M * K, _p(o["Wh"]), N * K, _p(o["sc"]), bias, out.ptr, ld, pp, ps, M, N, K, *tail))
    else:
        E._check(lib.sdvar_op_gemm_rowblk(None, 0, None, None, 1, 0, _p(o["Xh"]), M * K, _p(o["Wh"]), N * K, _p(o["sc"]), bias, out.ptr, ld, None, 0, M, N, K, *tail[:-1],
                                          None, None, None, None, 0, 0, 0, 0, 0, _st()))
    out.check_guards(what + " out", untouched=to_planes)
    if resb is not None and not inplace:
        resb.check_guards(what + " res", untouched=True)
    if to_planes:
        outp.check_guards(what + " out_planes")
        return outp.value("bf16" if kind == "bf16x3" else "f16", what)
    return out.interior()


def check_int(kind, c, epi, rpg, dev, what, **kw):
    """One exact-integer case through one kernel: epilogues 0 / 2 bit for bit, epilogue 1 within the derived GELU bound."""
    o = device_ops(c, dev)
    got = launch(kind, o, epi, rpg, dev, what, **kw)
    if epi != 1:
        assert_same(got, int_ref(c, epi, rpg, dev), what)
        return
    form, outk = ("tanh", "f32") if kind in ("f32", "bf16x3") else ("exp", "f16x2")
    ref, bound = gelu_ref(c, form, outk, dev)
    err = assert_within(got.double(), ref, bound, what)
    note_ratio((kind, form), err, bound, ref)


def shapes_and_gates(shapes):
    for i, (M, N, K) in enumerate(shapes):
        yield G.int_case(M, N, K), ([1, 5, 7] if (M, N) == (257, 384) else [G.rows_per_gate_for(M, i)])


def run_family(kind, mode, bm, epi, dev, shapes=SHAPES, splits=SPLITS, **kw):
    """Every shape x every distinct K split of one forced tile (bm 0: the automatic choice), with the proof that this tile and split ran."""
    for c, rpgs in shapes_and_gates(shapes):
        M, N, K = c.M, c.N, c.K
        if epi == 1 and kind != "f32" and N % 32:
            continue                                                                           # plane outputs are K-blocked by 32 columns
        want = sorted({(skinny_slices if bm == 16 else slices)(s, K) for s in splits}) if bm else [0]
        for split in want:
            for rpg in (rpgs if epi == 2 else [1]):
                what = f"{kind} bm {bm} split {split} epi {epi} rows_per_gate {rpg} ({M}, {N}, {K})"
                with forced(bm, split):
                    plan = kernel_plan(mode, M, N, K, vec=not kw.get("unaligned", False))
                    E.last_gemm_cfg()                                                      # reset the launch counters
                    check_int(kind, c, epi, rpg, dev, what, **kw)
                    cfg = E.last_gemm_cfg()
                if bm:
                    assert plan[:3] == [bm, split, 0], (what, plan)
                else:
                    assert plan[0] in ((32, 64, 128) if mode == 0 else (32, 64, 128, 256) if mode == 1 else (16, 32, 64, 128, 256, 512, 768)), (what, plan)
                if mode == 2:
                    assert [cfg["bm"], cfg["split"], cfg["tail_launches"]] == [plan[0], plan[1], int(plan[2] > 0)], (what, cfg, plan)


# ------------------------------------------------------------------------------------------------------------------------ exact-integer tests
@pytest.mark.parametrize("bm", [0, 32, 64, 128])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_f32_exact(dev, bm, epi):
    """sdvar_op_gemm: the automatic choice and every row tile (32, 64, 128) x K split that sdvar_debug_set_gemm_cfg can force for it."""
    run_family("f32", 0, bm, epi, dev)
    if epi == 1: print_ratios("f32", "cpu float32")


@pytest.mark.parametrize("bm", [0, 128, 256])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_bf16x3_exact(dev, bm, epi):
    """sdvar_op_gemm_bf16x3: the automatic choice, the LDS-DMA 128 x 128 and 256 x 128 kernels, K splits 1, 2, 3."""
    run_family("bf16x3", 1, bm, epi, dev, splits=(1, 2, 3))
    if epi == 1: print_ratios("bf16x3")


@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_bf16x3_exact_gemm_v2_off(dev, epi):
    """The 128-row tile on the kernel without the LDS-DMA ("gemm_v2" 0)."""
    with variant("gemm_v2", 0):
        run_family("bf16x3", 1, 128, epi, dev, splits=(1, 2, 3))


def test_gemm_bf16x3_exact_hybrid_tail(dev):
    """A shape on which the planner takes the hybrid tail on its own: full rounds unsplit, the partial last round split along K and reduced per tile.  bf16x3 has no
    forcing hook and no launch counter for the tail: the planner's answer (which its launcher executes) is the proof.  Of the small-K candidates every one the
    planner takes the tail for is run; with the cost model of this commit the two K = 256 shapes go to 64-row tiles and (2700, 3200, 512) takes the tail split 8
    ways.  Skipped only if a refit leaves none."""
    ran = []
    for (M, N, K) in HYBRID_SHAPES + [(2700, 3200, 512)]:
        plan = kernel_plan(1, M, N, K)
        if not (plan[0] == 256 and plan[2] > 0):
            continue
        c = G.int_case(M, N, K)
        for epi in (0, 1, 2):
            check_int("bf16x3", c, epi, 7, dev, f"bf16x3 hybrid tail {plan} epi {epi} ({M}, {N}, {K})")
        drop_cached(M, N, K)
        ran.append((M, N, K, plan[2]))
    if not ran:
        pytest.skip("the planner takes the hybrid tail for none of the small-K shapes")
    print("bf16x3 hybrid tail ran on (M, N, K, tail split):", ran)


@pytest.mark.parametrize("bm", [0, 32, 64, 128, 256, 512, 768])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_f16x2_exact(dev, bm, epi):
    """sdvar_op_gemm_f16x2: the automatic choice and every tile kernel (32 / 64-row, 128 x 128, 256 x 128, 256 x 256 = 512, 256 x 192 = 768) x K splits 1, 2, 3, 5."""
    run_family("f16x2", 2, bm, epi, dev)
    if epi == 1: print_ratios("f16x2", "cpu float32")


@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_f16x2_exact_skinny(dev, epi):
    """The skinny kernel (bm 16, M <= 80), forced, on N down to 16 and its own K splits."""
    run_family("f16x2", 2, 16, epi, dev, shapes=SKINNY_SHAPES)


@pytest.mark.parametrize("M,N,K", HYBRID_SHAPES)
def test_gemm_f16x2_exact_hybrid_tail(dev, M, N, K):
    """The hybrid tail forced with (256, -4); the launch counter proves that the tail kernels ran."""
    c = G.int_case(M, N, K)
    for epi in (0, 1, 2):
        what = f"f16x2 hybrid tail epi {epi} ({M}, {N}, {K})"
        with forced(256, -4):
            E.last_gemm_cfg()
            check_int("f16x2", c, epi, 7, dev, what)
            cfg = E.last_gemm_cfg()
        assert cfg["bm"] == 256 and cfg["split"] == 1 and cfg["tail_launches"] == 1, (what, cfg)
    drop_cached(M, N, K)


@pytest.mark.parametrize("name,value,bm", VARIANTS)
def test_gemm_f16x2_exact_variants(dev, name, value, bm):
    """Every kernel variant that only a switch selects (VARIANTS of test_gpu_ops.py), on the K sweep and the ragged shapes, all three epilogues."""
    shapes = [(257, 384, K) for K in G.KS] + [(1, 128, 96), (130, 192, 96), (300, 528, 1024), (700, 192, 96)]
    with variant(name, value):
        for epi in (0, 1, 2):
            run_family("f16x2", 2, bm, epi, dev, shapes=shapes, splits=(1,) if bm == 512 else (1, 3))


@pytest.mark.parametrize("bm", [32, 64, 128, 256, 512, 768])
@pytest.mark.parametrize("epi", [0, 2])
def test_gemm_f16x2_exact_unaligned_epilogue(dev, bm, epi):
    """The element-wise epilogue path: bias pointer 4 bytes off the 16-byte grid, odd ldo, ldres and gate_stride, N = 260."""
    run_family("f16x2", 2, bm, epi, dev, shapes=[(130, 260, 96), (257, 260, 1024), (33, 260, 160)], splits=(1,), unaligned=True)


@pytest.mark.parametrize("epi", [0, 2])
def test_gemm_rowblk_exact_plane_operand(dev, epi):
    """sdvar_op_gemm_rowblk on operand planes (x == NULL), K up to 4096 unsplit, bias and gated-residual epilogues."""
    for c, _ in shapes_and_gates(G.shape_list(ms=(1, 33, 80), ns=(16, 128, 528), sweep=(33, 128))):
        for rpg in ([1, 5, 7] if epi == 2 and c.M > 1 else [1]):
            what = f"rowblk epi {epi} rows_per_gate {rpg} ({c.M}, {c.N}, {c.K})"
            E.last_gemm_cfg()
            check_int("rowblk", c, epi, rpg, dev, what)
            assert E.last_gemm_cfg()["bm"] == 17, what


@pytest.mark.parametrize("kind", ["f32", "bf16x3", "f16x2", "rowblk"])
def test_gated_residual_in_place(dev, kind):
    """The model calls epilogue 2 in place (res == out); every other case here keeps res in a guarded buffer of its own."""
    for (M, N, K) in ((33, 128, 1024), (80, 528, 96)) + (() if kind == "rowblk" else ((257, 384, 160),)):
        for rpg in (1, 5, 7):
            check_int(kind, G.int_case(M, N, K), 2, rpg, dev, f"{kind} in place rows_per_gate {rpg} ({M}, {N}, {K})", inplace=True)


# ------------------------------------------------------------------------------------------------------------------------ the half-precision GEMM
HALF = {"f16": (1, torch.float16), "bf16": (2, torch.bfloat16)}


def half_operand(t, dt, dev):
    """fp32 (rows, K) CPU -> one K-blocked plane (K / 32, rows, 32) of dt on the device (built on the CPU: the values are exact, or rounded by torch's cast)."""
    rows, K = t.shape
    return t.to(dt).view(rows, K // 32, 32).permute(1, 0, 2).contiguous().to(dev)


def launch_h(X, W, bias, name, out_half, epi, dev, what):
    """sdvar_op_gemm_h into guarded buffers.  Returns out (fp32 or half, (M, N)) for epilogue 0, (pre_out (M, N) half, h as float64 (M, N)) for epilogue 1."""
    lib = E.load_library()
    code, dt = HALF[name]
    (M, K), N = X.shape, W.shape[0]
    Xo, Wo = half_operand(X, dt, dev), half_operand(W, dt, dev)
    b = bias.to(dev) if bias is not None else None
    if epi == 0:
        out = GuardedRows(M, N, N + 8, dev, words=torch.int16 if out_half else torch.int32)               # ldo > N
        E._check(lib.sdvar_op_gemm_h(_p(Xo), _p(Wo), code, _p(b), out.ptr, code if out_half else 0, N + 8, None, None, M, N, K, 0, _st()))
        out.check_guards(what + " out")
        return out.interior(dt if out_half else torch.float32)
    h, pre = GuardedPlanes(1, M, N, dev), GuardedRows(M, N, N, dev, words=torch.int16)
    E._check(lib.sdvar_op_gemm_h(_p(Xo), _p(Wo), code, _p(b), None, 0, 0, h.ptr, pre.ptr, M, N, K, 1, _st()))
    h.check_guards(what + " h_out"); pre.check_guards(what + " pre_out")
    return pre.interior(dt), h.value(name, what)


@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_gemm_h_exact(dev, name):
    """sdvar_op_gemm_h's contract on exact integers: fp32 output bit-equal to the product; half output = ONE nearest-even rounding of it (outputs beyond 2048 / 256 do
    round); epilogue 1: pre_out = the rounded v bit for bit, h_out = GELU of THAT value within the derived bound plus one rounding to the half type."""
    _, dt = HALF[name]
    for M, N, K in SHAPES:
        c = G.int_case(M, N, K)
        what = f"gemm_h {name} ({M}, {N}, {K})"
        assert_same(launch_h(c.X, c.W, c.bias, name, False, 0, dev, what), c.v.float().to(dev), what + " fp32 out")
        vh = c.v.float().to(dt)
        assert_same(launch_h(c.X, c.W, c.bias, name, True, 0, dev, what), vh.to(dev), what + " half out")
        if N % 32 == 0:
            pre, h = launch_h(c.X, c.W, c.bias, name, True, 1, dev, what)
            assert_same(pre, vh.to(dev), what + " pre_out")
            p = vh.double()
            ref, bound = G.gelu64(p), G.gelu_bound(p, "exp", name)
            err = assert_within(h.cpu(), ref, bound, what + " h_out")
            note_ratio(("gemm_h " + name, "exp"), err, bound, ref)
    big = G.int_case(257, 384, 4096).v.abs().max().item()
    assert big > 2048                                                                          # the half outputs did have to round
    print_ratios("gemm_h " + name)


@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_gemm_h_bits_do_not_depend_on_M_or_N(dev, name):
    """The header's promise: an element is one fp32 MFMA chain over k in ascending order, whatever M, N or the tile it falls into.  Random (inexact) operands: here the
    bits DO depend on the summation order."""
    gc = G.graded_case(257, 384, 1024)
    A, B, b = gc.A, gc.B * 8, gc.res0[0, :384].contiguous()
    for out_half in (False, True):
        full = launch_h(A, B, b, name, out_half, 0, dev, "gemm_h full")
        for (m, n) in ((130, 192), (1, 8), (257, 136)):
            part = launch_h(A[:m].contiguous(), B[:n].contiguous(), b[:n].contiguous(), name, out_half, 0, dev, f"gemm_h ({m}, {n})")
            assert_same(part, full[:m, :n].contiguous(), f"gemm_h {name} ({m}, {n}) against (257, 384), half out {out_half}")
    pre, h = launch_h(A, B, b, name, True, 1, dev, "gemm_h full")
    pre2, h2 = launch_h(A[:130].contiguous(), B[:192].contiguous(), b[:192].contiguous(), name, True, 1, dev, "gemm_h (130, 192)")
    assert_same(pre2, pre[:130, :192].contiguous(), f"gemm_h {name} pre_out")
    assert_same(h2, h[:130, :192].contiguous(), f"gemm_h {name} h_out")


# ------------------------------------------------------------------------------------------------------------------------ graded scales
class _Plain:
    """A GradedCase's unscaled (A, B, res0) or scaled (X, W, res) operands under the attribute names device_ops reads."""

    def __init__(self, gc, scaled):
        self.M, self.N, self.K = gc.M, gc.N, gc.K
        self.X, self.W, self.res = (gc.X, gc.W, gc.res) if scaled else (gc.A, gc.B, gc.res0)
        self.bias, self.gate = gc.bias, gc.gate


def graded_pair(kind, gc, epi, dev, what, f16x2=False):
    base = launch(kind, device_ops(_Plain(gc, False), dev, ("graded", gc.M, gc.K, False, f16x2), f16x2), epi, 5, dev, what + " (A, B)")
    scaled = launch(kind, device_ops(_Plain(gc, True), dev, ("graded", gc.M, gc.K, True, f16x2), f16x2), epi, 5, dev, what + " (X, W)")
    return base, scaled


@pytest.mark.parametrize("kind,mode,bms,splits", [("f32", 0, (0, 32, 64, 128), (1, 2, 3)), ("bf16x3", 1, (0, 128, 256), (1, 2, 3))])
def test_graded_scales_commute_bit_for_bit(dev, kind, mode, bms, splits):
    """fp32 and bf16x3 are scale-free: out(diag(r) A, diag(c) B) == out(A, B) * r_i * c_j in every bit (no tolerance: a power of two commutes with every rounding
    away from underflow, which test_gemm_exact_host.py rules out), for the automatic choice and each forced tile and K split, epilogues 0 and 2."""
    for M, N, K in G.GRADED_SHAPES:
        gc = G.graded_case(M, N, K)
        scale = gc.scale.to(dev)
        for bm in bms:
            for split in (sorted({slices(s, K) for s in splits}) if bm else [0]):
                for epi in (0, 2):
                    what = f"graded {kind} bm {bm} split {split} epi {epi} ({M}, {N}, {K})"
                    with forced(bm, split):
                        plan = kernel_plan(mode, M, N, K)
                        base, scaled = graded_pair(kind, gc, epi, dev, what)
                    assert not bm or plan[:3] == [bm, split, 0], (what, plan)
                    assert_same(scaled, (base.double() * scale).float(), what)


def test_graded_scales_commute_gemm_h_bf16(dev):
    """sdvar_op_gemm_h on bf16 operands with fp32 output: the operands' rounding to bf16 commutes with the scales as well."""
    for M, N, K in G.GRADED_SHAPES:
        gc = G.graded_case(M, N, K)
        base = launch_h(gc.A, gc.B, None, "bf16", False, 0, dev, "graded gemm_h (A, B)")
        scaled = launch_h(gc.X, gc.W, None, "bf16", False, 0, dev, "graded gemm_h (X, W)")
        assert_same(scaled, (base.double() * gc.scale.to(dev)).float(), f"graded gemm_h bf16 ({M}, {N}, {K})")


@pytest.mark.parametrize("bm", [0, 32, 64, 128, 256, 512, 768])
def test_graded_scales_f16x2_normalised_error(dev, bm):
    """f16x2 is NOT scale-free: one power-of-two scale per weight tensor, unscaled fp16 activation planes.  Row scales 2^{0, 3, 6} (the tiny-activation floor belongs to
    test_split_gemm_outlier_and_tiny_activations), column scales 2^{0, 3, -5, -10}: against fp64, per element, |got - ref| / (r_i c_j) <= 2e-5 max(1, max |ref / (r c)|) -
    the bar of every GEMM test of the project, applied to the normalised output.  Prints the worst normalised error per scale class."""
    for M, N, K in G.GRADED_SHAPES:
        gc = G.graded_case(M, N, K, True)
        o = device_ops(_Plain(gc, True), dev, ("graded", M, K, True, True), True)
        v = gc.X.double() @ gc.W.double().t()
        for epi in (0, 2):
            what = f"graded f16x2 bm {bm} epi {epi} ({M}, {N}, {K})"
            ref = v if epi == 0 else gc.res.double() + v * gc.gate[:(M + 4) // 5, :N].double().repeat_interleave(5, 0)[:M]
            with forced(bm, 1 if bm else 0):
                E.last_gemm_cfg()
                got = launch("f16x2", o, epi, 5, dev, what).cpu().double()
                cfg = E.last_gemm_cfg()
            assert not bm or cfg["bm"] == bm, (what, cfg)
            nref = ref / gc.scale
            bar = 2e-5 * max(1.0, float(nref.abs().max()))
            nerr = (got - ref).abs() / gc.scale
            for re_ in G.R_EXP_F16X2:
                for ce in G.C_EXP:
                    cls = nerr[gc.r_exp == re_][:, gc.c_exp == ce]
                    print(f"{what}: r 2^{re_} c 2^{ce}: worst normalised error {float(cls.max()):.3e} (bar {bar:.3e})")
            assert_within(got / gc.scale, nref, torch.full_like(nref, bar), what)
