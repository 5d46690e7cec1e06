"""The premises of tests/conv_exact_cases.py, proved on the CPU: every operand is a fixed point of its splitter (or splits into exactly the planes the case's
argument assumes), the 2^24 bound holds for every case and plane format from the operand planes alone, the sparse case has its lattice property, weight_scale gives
the scale the cases assume, and the host models of the library's re-packing kernels (phase weights, space-to-depth) reproduce the plain float64 conv2d."""
import pytest
import torch

import conv_exact_cases as X

INT_CASES = X.int_cases()
SPLIT_CASES = [(c, pf) for pf in (2, 3) for c in X.split_plane_cases(pf)]


def test_splitter_models_on_known_values():
    """split2h rounds to nearest even, split3 truncates: the values the docstring of conv_exact_cases argues with"""
    v = torch.tensor([1.0 - 2.0 ** -12, -1.0 + 2.0 ** -12, 2.0 + 2.0 ** -12, 2048.0 - 0.5, 2.0 ** -12])
    h, l = X.split_f16x2(v)
    assert h.tolist() == [1.0, -1.0, 2.0, 2048.0, 2.0 ** -12]                       # the two ties go to the even neighbour; with a = 0 the HIGH plane takes c 2^-12
    assert l.tolist() == [-2.0 ** -12, 2.0 ** -12, 2.0 ** -12, -0.5, 0.0]
    p = X.split_bf16x3(torch.tensor([1.0 + 2.0 ** -10 + 2.0 ** -20, -(1.0 + 2.0 ** -10), 1.0 - 2.0 ** -10]))
    assert [q[0].item() for q in p] == [1.0, 2.0 ** -10, 2.0 ** -20]
    assert [q[1].item() for q in p] == [-1.0, -2.0 ** -10, 0.0]
    assert [q[2].item() for q in p] == [1.0 - 2.0 ** -8, 3 * 2.0 ** -10, 0.0]       # mixed signs: NOT (1, -2^-10, 0) - why the bf16x3 value set is nested and same-sign
    assert X.plane_bits(torch.tensor([1.0, -2.0]), 2).tolist() == [0x3C00, 0xC000 - 65536]
    assert X.plane_bits(torch.tensor([1.0, -2.0]), 3).tolist() == [0x3F80, 0xC000 - 65536]


@pytest.mark.parametrize("c", INT_CASES, ids=lambda c: c.id)
def test_int_case_premises(c):
    """Integers in range; fixed points of both splitters (low planes zero), scaled or not; the f16x2 scale is the assumed power of two; < 2^24 in both formats; and
    the plane-product reference machinery (phase weights, space-to-depth weights, channel padding) equals the plain float64 conv2d exactly."""
    for t, m in ((c.xk, 3), (c.w, 3), (c.bias, 8)) + (((c.res, 64),) if c.res is not None else ()):
        assert bool((t == t.round()).all()) and float(t.abs().max()) <= m
    assert float(c.w.abs().max()) == 3.0
    kw = c.kernel_weight()
    assert float(kw.abs().max()) == (12.0 if c.up else 3.0)
    assert c.scale(2) == (2.0 ** 9 if c.up else 2.0 ** 11) == X.weight_scale(kw)     # 12 * 2^9 = 6144, 3 * 2^11 = 6144: inside (2^12, 2^13]
    for pf in (2, 3):
        xs, ws = c.x_planes(pf), c.w_planes(pf)
        assert torch.equal(xs[0], c.xk) and torch.equal(ws[0], kw * c.scale(pf))
        assert not any(bool(p.any()) for p in xs[1:] + ws[1:])
        bound, grain, bits = X.prove_exact(c, pf)
        assert grain == 1.0 and bits < 24
        assert bound <= (36 * 4 if c.up else 9 * c.taps) * c.Cin + 72
        assert torch.equal(c.plane_sum(pf), c.conv2d64())
    assert c.Cin <= 640


@pytest.mark.parametrize("c,pf", SPLIT_CASES, ids=lambda v: v.id if hasattr(v, "id") else str(v))
def test_split_plane_case_premises(c, pf):
    """The planes are exactly the ones the argument assumes, the low planes carry data, and (max |partial sum|) / grain < 2^24 from the operand planes alone."""
    xs, ws = c.x_planes(pf), c.w_planes(pf)
    kw, S = c.kernel_weight(), c.scale(pf)
    assert torch.equal(sum(p.double() for p in xs), c.xk.double()) and torch.equal(sum(p.double() for p in ws), kw.double() * S)       # nothing lost in the split
    nzx, nzw = c.xk != 0, kw != 0
    if pf == 2:
        assert S == 2.0 ** 11 == X.weight_scale(kw) and float(kw.abs().max()) == 2.0 + 2.0 ** -12
        a, lo = xs[0], xs[1] * 2.0 ** 12
        assert bool((a == a.round()).all()) and float(a.abs().max()) <= 2 and bool((a != 0)[nzx].all())               # high plane: the integer a, non-zero wherever x is
        assert bool(((lo == 0) | (lo.abs() == 1)).all())                                                              # low plane: c 2^-12, a normal fp16
        a, lo = ws[0] / S, ws[1] / S * 2.0 ** 12
        assert bool((a == a.round()).all()) and float(a.abs().max()) <= 2 and bool((a != 0)[nzw].all())
        assert bool(((lo == 0) | (lo.abs() == 1)).all())
        assert bool(xs[1].any()) and bool(ws[1].any())                                                                # hl and lh are exercised
    else:
        for planes, nz in ((xs, nzx), (ws, nzw)):
            assert bool((planes[0].abs() == 1)[nz].all()) and not bool(planes[0][~nz].any())
            for k, e in ((1, 10), (2, 20)):
                q = planes[k] * 2.0 ** e
                assert bool(((q == 0) | (q == planes[0])).all())                                                      # s b 2^-10, s c 2^-20 with the sign of the high plane
                assert bool(planes[k].any())
            assert not bool((planes[2] != 0)[planes[1] == 0].any())                                                   # nested: c <= b
    bound, grain, bits = X.prove_exact(c, pf)
    assert grain == (2.0 ** -12 if pf == 2 else 2.0 ** -20)
    assert bits < 24, (bound, grain)
    if c.kind == "dense":
        assert c.Cin <= 96 and bound < 4.01 * 9 * 96 + 72 < 2.0 ** 12
    # the reference is a multiple of the grain below 2^24 grains: an fp32 number, so .float() of it loses nothing
    for res in ((False, True) if c.res is not None else (False,)):
        r = c.ref(pf, res)
        assert torch.equal(r.float().double(), r) and bool((r / grain == (r / grain).round()).all())
    if c.up:                                                                                                          # every phase weight is one corner weight
        assert torch.equal(c.weff.permute(1, 2, 0, 3, 4).reshape(c.N, c.Cin, -1).abs().sort(-1).values,
                           c.w[:, :, 0::2, 0::2].repeat(1, 1, 2, 2).reshape(c.N, c.Cin, -1).abs().sort(-1).values)
        assert not bool(c.w[:, :, 1, :].any()) and not bool(c.w[:, :, :, 1].any())


@pytest.mark.parametrize("c,pf", [v for v in SPLIT_CASES if v[0].kind == "sparse"], ids=lambda v: v.id if hasattr(v, "id") else str(v))
def test_sparse_lattice(c, pf):
    """x lives on the pitch-3 lattice with at most 7 channels per pixel, spread over every channel block; so every 3x3 (2x2) window holds at most one lattice pixel
    and each output is one tap of one pixel: the reference equals that single product sum, gathered by hand."""
    nz = (c.xk != 0).any(1)                                                # (B, H, W)
    ys, xs = torch.meshgrid(torch.arange(c.Hk), torch.arange(c.Wk), indexing="ij")
    on = (ys % 3 == 1) & (xs % 3 == 1)
    assert not bool(nz[:, ~on].any()) and bool(nz[:, on].any())
    per_pixel = (c.xk != 0).sum(1)
    assert int(per_pixel.max()) <= 7
    blocks = (c.xk != 0).view(c.B, c.Cin // 32, 32, c.Hk, c.Wk).any(2).sum(1)
    assert int(blocks.max()) == c.Cin // 32 or int(per_pixel.max()) < c.Cin // 32
    k = 2 if c.up else 3
    cnt = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(nz.float()[:, None], (1, 1, 1, 1)), k, stride=1) * k * k
    assert float(cnt.max()) <= 1.0 + 1e-6
    if c.up:
        return
    # by hand: output (b, n, y, x) = sum over the <= 7 channels of the one lattice pixel (ly, lx) in its window of the plane products with tap (ly - y + 1, lx - x + 1)
    xp, wq = [p.double() for p in c.x_planes(pf)], [p.double() for p in c.w_planes(pf)]
    want = torch.zeros(c.B, c.N, c.Hk, c.Wk, dtype=torch.float64)
    for b in range(c.B):
        for ly in range(1, c.Hk, 3):
            for lx in range(1, c.Wk, 3):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        y, x = ly - dy, lx - dx
                        if 0 <= y < c.Hk and 0 <= x < c.Wk:
                            for i, j in X.PRODUCTS[pf]:
                                want[b, :, y, x] += wq[j][:, :, dy + 1, dx + 1] @ xp[i][b, :, ly, lx]
    assert torch.equal(want / c.scale(pf), c.plane_sum(pf))


def test_products_cover_the_header_claim():
    """conv.hip's header: six plane products for bf16x3, three (hh, hl, lh) for f16x2 - the reference sums exactly those, and never a product of two low planes"""
    assert len(X.PRODUCTS[3]) == 6 and len(X.PRODUCTS[2]) == 3
    assert all(i + j <= 2 for i, j in X.PRODUCTS[3]) and all(i + j <= 1 for i, j in X.PRODUCTS[2])


def test_case_lists_cover_what_they_must():
    shapes = {(c.B, c.H, c.W, c.Cin, c.N, c.taps) for c in INT_CASES}
    assert set(X.TAP_REUSE_SHAPES) <= shapes
    assert {c.M for c in INT_CASES} >= {1, 33, 255, 257}
    assert {c.N for c in INT_CASES} >= {32, 48, 90, 160, 200, 320}
    assert {c.Cin for c in INT_CASES} >= {32, 64, 96, 160, 640}
    assert {c.taps for c in INT_CASES} == {1, 4, 9} and {c.src for c in INT_CASES} == {"prep", "prep_up", "s2d", "img"}
    assert {c.N for c in INT_CASES if X.stats_fuse(c, 1)} >= {128, 160, 320}
    assert X.expected_slices(2, 9) == 2 and X.expected_slices(4, 9) == 3 and X.expected_slices(4, 18) == 4 and X.expected_slices(3, 5) == 3 and X.expected_slices(7, 5) == 5
