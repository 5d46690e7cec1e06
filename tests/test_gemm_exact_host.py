"""No GPU: the premises of tests/test_gpu_gemm_exact.py, checked on the cases of tests/gemm_exact_cases.py themselves.
  * every integer operand is a fixed point of fp16, of fp16 after the f16x2 weight scale, and of bf16;
  * max_ij sum_k |x_ik| |w_jk| < 2^24, also through the bias and the gated-residual arithmetic: no partial sum, in any order, can round;
  * numpy float32 accumulation in three random k orders reproduces the float64 reference;
  * the GELU reference is the function nn.GELU(approximate='tanh') computes, and the two fp32 formulas of common.h, evaluated by torch on the CPU, meet the derived bound;
  * the graded cases cannot underflow: every scaled intermediate is zero or a normal fp32."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_exact_cases as G

HOST_SHAPES = [(1, 128, 32), (33, 192, 96), (80, 16, 160), (130, 260, 96), (257, 384, 1024), (300, 528, 1024), (700, 128, 96), (257, 384, 4096), (2704, 3072, 256), (2700, 3200, 256)]


@pytest.mark.parametrize("M,N,K", HOST_SHAPES)
def test_integer_operands_are_fixed_points_of_every_plane_format(M, N, K):
    c = G.int_case(M, N, K)
    S = G.weight_scale(c.W)
    assert S == 2.0 ** 11                                                   # max |W| = 3 is pinned
    for t, lo, hi in ((c.X, -3, 3), (c.W, -3, 3), (c.bias, -8, 8), (c.res, -64, 64), (c.gate, -2, 2)):
        assert torch.equal(t, t.round()) and lo <= float(t.min()) and float(t.max()) <= hi
    for t in (c.X, c.W):
        assert torch.equal(t.half().float(), t) and torch.equal(t.bfloat16().float(), t)
    ws = c.W * S
    assert torch.equal(ws.half().float(), ws) and float(ws.abs().max()) <= 65504
    if M >= 3:
        nz = (c.X != 0).sum(1)
        assert int(nz[c.gelu_rows].max()) <= 2 and float(c.v[c.gelu_rows].abs().max()) <= 26
        assert float(c.v[~c.gelu_rows].abs().max()) > 26 or K <= 32         # the other rows leave the curved part


@pytest.mark.parametrize("M,N,K", HOST_SHAPES)
def test_no_partial_sum_can_round(M, N, K):
    c = G.int_case(M, N, K)
    worst = float((c.X.abs().double() @ c.W.abs().double().t()).max())     # bounds every partial sum of every subset of a dot product
    assert worst <= 9 * K and worst < 2 ** 24
    assert worst * G.weight_scale(c.W) / 2 ** 11 < 2 ** 24                  # with the weight scale: 2^11 times an integer below 2^24
    vmax = worst + float(c.bias.abs().max())
    assert vmax < 2 ** 24 and 2 * vmax + 64 < 2 ** 24                       # |v|, |v gate| and |res + v gate|
    for epi, rpg in ((0, 1), (2, 1), (2, 5), (2, 7)):
        ref = c.ref(epi, rpg)
        assert torch.equal(ref, ref.round()) and float(ref.abs().max()) < 2 ** 24 and torch.equal(ref.float().double(), ref)
    # one rounding to the half types is the only inexact step of sdvar_op_gemm_h's half outputs, and these cases do exercise it
    if M >= 3 and K >= 96:
        assert float(c.v.abs().max()) > (2048 if K >= 1024 else 256)


@pytest.mark.parametrize("M,N,K", [(33, 192, 96), (130, 128, 1024), (257, 384, 4096)])
def test_float32_accumulation_in_random_orders_is_exact(M, N, K):
    c = G.int_case(M, N, K)
    X, W = c.X.numpy(), c.W.numpy()
    g = np.random.Generator(np.random.Philox(key=[5, 7002]))
    for _ in range(3):
        perm = g.permutation(K)
        acc = np.zeros((M, N), dtype=np.float32)
        for k0 in range(0, K, 64):                                         # strictly sequential float32 adds, 64 k at a time to keep it quick
            p = (X[:, perm[k0:k0 + 64], None] * W.T[None, perm[k0:k0 + 64], :]).astype(np.float32)
            for j in range(p.shape[1]):
                acc += p[:, j, :]
        assert acc.dtype == np.float32
        assert np.array_equal(acc.astype(np.float64) + c.bias.numpy().astype(np.float64), c.v.numpy())


def test_gelu_reference_is_nn_gelu_tanh():
    v = torch.arange(-40, 41, dtype=torch.float64)
    a, b = G.gelu64(v), F.gelu(v, approximate="tanh")
    ok = v >= -5                                                            # beyond, float64's 1 + tanh(u) has lost its digits; the stable form has not
    assert float(((a - b).abs() / b.abs().clamp_min(1e-300))[ok & (v != 0)].max()) < 1e-9
    assert float((a - b).abs().max()) < 1e-15 * 40
    assert a[v == 0].item() == 0 and float(a[v == -40]) == 0.0 and float(a[v == 40]) == 40.0
    # the constants of gelu_tanh_h stand for -2 log2(e) sqrt(2/pi) and 0.044715 times that, to better than fp32's unit roundoff
    assert G._const_err(G.C0_SRC, G.C0_TRUE) < 1 and G._const_err(G.C1_SRC, G.C1_TRUE) < 1


@pytest.mark.parametrize("form,fn", [("tanh", G.gelu_tanh_f32), ("exp", G.gelu_exp_f32)])
def test_cpu_float32_formulas_meet_the_derived_gelu_bound(form, fn):
    v = torch.cat([torch.arange(-36872, 36873, 97, dtype=torch.float64), torch.arange(-64, 65, dtype=torch.float64)])
    got, ref, bound = fn(v).double(), G.gelu64(v), G.gelu_bound(v, form, "f32")
    err = (got - ref).abs()
    assert bool((err <= bound).all()), (v[err > bound][:5], err[err > bound][:5], bound[err > bound][:5])
    assert bool((got[bound == 0] == ref[bound == 0]).all())
    print("gelu %s: worst err / bound on the CPU %.3f (%.3f where the bound is below |gelu| / 2)" % ((form,) + G.gelu_worst_ratio(err, bound, ref)))
    assert float(G.gelu_c_exp(torch.tensor([30.0])).item()) <= 6.0 + 1e-9  # far right both forms cost a handful of roundings
    assert 5.0 <= float(G.gelu_c_tanh(torch.tensor([30.0])).item()) <= 2.0 + G.TANH_ULPS + 1e-9


@pytest.mark.parametrize("M,N,K", G.GRADED_SHAPES)
@pytest.mark.parametrize("f16x2", [False, True])
def test_graded_cases_commute_with_their_scales_and_cannot_underflow(M, N, K, f16x2):
    gc = G.graded_case(M, N, K, f16x2)
    # the operands sit on their grids and are floats; the scaled operands are exact power-of-two multiples, in fp32 and after a rounding to bf16
    for t, bits in ((gc.A, G.A_GRID), (gc.B, G.B_GRID), (gc.res0, G.A_GRID), (gc.gate, G.G_GRID)):
        s = t.double() * 2.0 ** bits
        assert torch.equal(s, s.round())
    assert torch.equal(gc.X.double(), gc.A.double() * gc.r[:, None]) and torch.equal(gc.W.double(), gc.B.double() * gc.c[:, None])
    assert torch.equal(gc.X.bfloat16().double(), gc.A.bfloat16().double() * gc.r[:, None])
    assert torch.equal(gc.W.bfloat16().double(), gc.B.bfloat16().double() * gc.c[:, None])
    assert torch.equal(gc.res.double(), gc.res0.double() * gc.scale)
    exps = G.R_EXP_F16X2 if f16x2 else G.R_EXP
    assert sorted(set(gc.r_exp.tolist())) == sorted(exps) and sorted(set(gc.c_exp.tolist())) == sorted(G.C_EXP)
    assert len(set(gc.c_exp[:32].tolist())) == 4                            # one 32-column tile mixes all four column scales
    # nothing leaves the normal range: the smallest non-zero intermediate times the smallest scale, the largest times the largest
    smin, smax = float(gc.scale.min()), float(gc.scale.max())
    assert G.graded_chain_floor(gc) * smin >= G.TINY32
    big = float((gc.A.abs().double() @ gc.B.abs().double().t()).max())    # bounds every partial sum
    top = (float(gc.res0.abs().max()) + big * float(gc.gate.abs().max())) * smax
    assert top < 2.0 ** 127
    # each scaled PRODUCT is normal as well (bf16x3's smallest plane products are covered by the 2^-45 granularity above)
    amin, bmin = float(gc.A[gc.A != 0].abs().min()), float(gc.B[gc.B != 0].abs().min())
    assert amin * bmin * smin >= G.TINY32
    if f16x2:
        # activations stay inside the fp16 range and above the documented floor of the low plane (|x| >= 2^-3 keeps 2^-22 relative: most elements are smaller, and
        # that is the floor test_split_gemm_outlier_and_tiny_activations owns); weights: the smallest column scale is 2^-10 of the largest
        assert float(gc.X.abs().max()) < 65504 and min(exps) == 0
