"""seam.cross_entropy / CrossEntropyLoss / install_trainer (sdvar_xent_train_fwd, sdvar_xent_train_bwd; csrc/xent_train.hip) against torch in fp64 on the CPU: the
loss of the reference's trainer (trainer.py:37-38, 112-120) in both directions.  Every bound below is derived from the kernels' operation counts (first order,
u = 2^-24, expf / logf 1 ulp = 2 u), and torch's own float32 cross_entropy on the CPU is asserted to meet the same bound on the same inputs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
_BL = {1: (1, 1), 5: (1, 5), 1362: (2, 681)}


@pytest.fixture(autouse=True)
def _grad_mode_on():
    """Other test modules switch grad mode off for the whole process when they are imported; these tests are about autograd."""
    with torch.enable_grad():
        yield


def _rounds(V):
    return (V + 255) // 256


def lse_bound_c(V):
    """c of |lse_hip - lse_64| <= c u max(1, |lse|, |x_t|): xent_bound_c of tests/test_gpu_var_forward.py (the forward's lse is formed by the same operations as
    sdvar_xent_stats') without its last subtraction lse - x_t (2 units): 48 + 4 R relative on s = sum exp(x - m), 20 for logf, 1 for m + log s.  R = ceil(V / 256)."""
    return 69 + 4 * _rounds(V)


def loss_bound_c(V, eps):
    """c of |loss_hip - loss_64| <= c u S, S = max(1, |lse|, |x_t|, A), A = mean_j |x_j| of the row, for
        loss = (1 - eps) nll + eps t2,   nll = lse - x_t,   t2 = lse - sumx / V.
    eps == 0: the kernel evaluates nll alone: xent_bound_c = 71 + 4 R (lse_bound_c plus u |nll| <= 2 u S).  Otherwise, in units of u S (|nll|, |t2|, |loss| <= 2 S):
      (1 - eps)(71 + 4 R)   the error of nll, weighted
      eps (69 + 4 R)        the error of lse inside t2
      eps (R + 9)           sumx / V: an element passes 2 additions inside its float4, at most R down its lane's sum and 6 in the butterfly, (R + 8) u sum_j |x_j|,
                            over V: (R + 8) u A; the division rounds by u |sumx / V| <= u A
      eps 2                 the subtraction lse - sumx / V rounds by u |t2|
      4                     the factor 1 - float(eps) is off by at most u absolute (u eps from float(eps), u (1 - eps) from the subtraction): u |nll|; its product
                            with nll rounds by at most u |nll|
      eps 4                 float(eps) is off by u eps: u eps |t2|; its product with t2 rounds by u eps |t2|
      2                     the final addition rounds by u |loss|
    Sum: 71 + 4 R + eps (R + 9) + 4 + 4 eps + 2 = 77 + 4 R + eps (R + 13)."""
    R = _rounds(V)
    return 71 + 4 * R if eps == 0 else 77 + 4 * R + eps * (R + 13)


def grad_bound(V, eps, g, p, onehot, lse, xabsmax):
    """Per-element bound |g| u (p_j c1(row) + c2_j) for dlogits[row, j] = g (exp(x_j - lse) - (1 - eps) [j == t] - eps / V):
      c1(row) = (71 + 4 R) S + 5, S = max(1, |lse|, max_j |x_j|): the relative error of exp(x_j - lse_hip) is the absolute error of its exponent, (69 + 4 R) u S from
                lse_hip (lse_bound_c) plus u |x_j - lse| <= 2 u S from the subtraction, plus 2 u for expf; 3 more for the roundings that scale with p_j: q - eps / V,
                the product with g, and g itself (reduction 'mean' rounds grad / count once)
      c2_j    = 5 ([j == t] + eps / V): at the target 1 - eps carries u absolute, q = p - (1 - eps) rounds by at most u, and the three roundings above act on
                |q| <= 1; elsewhere eps / V carries 2 u relative (float(eps), the division) and the same three roundings act on it."""
    R = _rounds(V)
    S = torch.clamp(torch.maximum(lse.abs(), xabsmax), min=1.0)
    c1 = (71 + 4 * R) * S + 5
    return g.abs().unsqueeze(1) * U * (p * c1.unsqueeze(1) + 5.0 * (onehot + eps / V))


def _inputs(V, N):
    """The inputs of test_xent_stats_shapes_and_confident_rows (same generator, same order): logits 3 N(0, 1), every third row confident - its target at +30, the others
    around 30 - ln 1e4 - ln(V - 1), nll about 1e-4."""
    B, L = _BL[N]
    gen = torch.Generator().manual_seed(V + 7 * L)
    lg = torch.randn(B, L, V, generator=gen) * 3
    tg = torch.randint(0, V, (B, L), generator=gen)
    conf = torch.zeros(B, L, dtype=torch.bool)
    conf.view(-1)[::3] = True
    lo = 30.0 - np.log(1e4) - np.log(V - 1) + 0.3 * torch.randn(B, L, V, generator=gen)
    lg[conf] = lo[conf]
    lg.view(-1, V)[conf.view(-1), tg.view(-1)[conf.view(-1)]] = 30.0
    return lg.view(N, V).contiguous(), tg.view(N).contiguous(), conf.view(N)


def _upstream(N, seed):
    """The per-row upstream gradient of reduction 'none': random, with a GradScaler's 65536 and a 0 among them."""
    g = torch.randn(N, generator=torch.Generator().manual_seed(seed))
    g[0] = 65536.0
    if N > 1:
        g[N // 2] = 0.0
        g[N - 1] = -65536.0
    return g


def _ref_grad(lg, tg, eps, reduction, g, dtype):
    x = lg.detach().to(dtype).clone().requires_grad_(True)
    out = F.cross_entropy(x, tg, reduction=reduction, label_smoothing=eps)
    out.backward(g.to(dtype))
    return out.detach(), x.grad


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("N", [1, 5, 1362])
@pytest.mark.parametrize("V", [4, 1000, 4096, 16384])
def test_loss_and_gradient_shapes_and_confident_rows(dev, V, N, eps):
    """Forward and backward on V = 4 (one float4, 63 idle lanes), 1000 (a ragged last round), 4096 (the product's), 16384 (64 rounds) and N = 1, 5, 1362 rows (none a
    multiple of the 4 rows per workgroup), eps 0 and 0.1, every third row confident (fp64 nll in [0.5e-4, 2e-4]).  loss and lse against fp64 F.cross_entropy /
    logsumexp within loss_bound_c / lse_bound_c; input.grad of reductions 'none' (random upstream gradient with 65536, -65536 and 0), 'mean' and 'sum' against fp64
    autograd within grad_bound, each row's gradients summing to 0 within the row's summed bound; torch's float32 CPU results meet every one of these bounds too; two
    runs are bit-identical (loss, lse, the 'mean' value, dlogits).  The worst err / bound ratios are printed."""
    from sdvar_amd import engine as E, seam
    lg, tg, conf = _inputs(V, N)
    x64 = lg.double()
    ref = F.cross_entropy(x64, tg, reduction="none", label_smoothing=eps)
    nll64 = F.cross_entropy(x64, tg, reduction="none")
    assert 0.5e-4 <= nll64[conf].min().item() and nll64[conf].max().item() <= 2e-4
    lse64 = torch.logsumexp(x64, -1)
    xt = x64.gather(-1, tg.unsqueeze(-1)).squeeze(-1)
    S = torch.clamp(torch.maximum(torch.maximum(lse64.abs(), xt.abs()), x64.abs().mean(-1)), min=1.0)
    lbound = loss_bound_c(V, eps) * U * S
    sbound = lse_bound_c(V) * U * torch.clamp(torch.maximum(lse64.abs(), xt.abs()), min=1.0)
    lgd, tgd = lg.to(dev), tg.to(dev)

    # forward: the engine call gives loss and lse; the no-grad seam call gives the same loss bits
    loss, lse, _, _ = E.xent_train_fwd(lgd, tgd, eps, -100, "none", True)
    loss2, lse2, _, _ = E.xent_train_fwd(lgd, tgd, eps, -100, "none", True)
    assert torch.equal(loss, loss2) and torch.equal(lse, lse2)
    assert torch.equal(seam.cross_entropy(lgd, tgd, eps), loss)
    err = (loss.cpu().double() - ref).abs()
    serr = (lse.cpu().double() - lse64).abs()
    cpu32 = (F.cross_entropy(lg, tg, reduction="none", label_smoothing=eps).double() - ref).abs()
    print(f"\nxent_train V={V} N={N} eps={eps}: loss err/bound {(err / lbound).max().item():.3f} (max|err| {err.max().item():.2e}; torch float32 on the CPU "
          f"{(cpu32 / lbound).max().item():.3f}), lse err/bound {(serr / sbound).max().item():.3f}")
    assert (cpu32 <= lbound).all()
    assert (err <= lbound).all(), (err / lbound).max().item()
    assert (serr <= sbound).all(), (serr / sbound).max().item()

    p = torch.softmax(x64, -1)
    onehot = torch.zeros_like(p).scatter_(1, tg.unsqueeze(1), 1.0)
    xabsmax = x64.abs().amax(-1)
    for reduction in ("none", "mean", "sum"):
        g = _upstream(N, V + N) if reduction == "none" else torch.tensor(0.75 if reduction == "mean" else -1.5)
        out64, grad64 = _ref_grad(lg, tg, eps, reduction, g, torch.float64)
        _, grad32 = _ref_grad(lg, tg, eps, reduction, g, torch.float32)
        grow = g.double() if reduction == "none" else (g.double() / (N if reduction == "mean" else 1)).expand(N)
        gb = grad_bound(V, eps, grow, p, onehot, lse64, xabsmax)
        runs = []
        for _ in range(2):
            xd = lgd.clone().requires_grad_(True)
            out = seam.cross_entropy(xd, tgd, eps, reduction)
            out.backward(g.to(dev))
            runs.append((out.detach(), xd.grad))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        out, grad = runs[0]
        assert grad.dtype == torch.float32 and grad.shape == (N, V)
        if reduction == "none":
            assert torch.equal(out, loss)
        else:
            # reduced in fp64 from the float32 rows: the rows' bounds, averaged / summed, and two roundings of the result
            vb = (lbound.mean() if reduction == "mean" else lbound.sum()) + 2 * U * out64.abs()
            assert out.dim() == 0 and (out.cpu().double() - out64).abs() <= vb
        gerr = (grad.cpu().double() - grad64).abs()
        g32err = (grad32.double() - grad64).abs()
        nz = gb > 0
        ratio = (gerr[nz] / gb[nz]).max().item() if nz.any() else 0.0
        ratio32 = (g32err[nz] / gb[nz]).max().item() if nz.any() else 0.0
        rowsum = grad.cpu().double().sum(-1).abs()
        print(f"  {reduction}: grad err/bound {ratio:.3f} (torch float32 on the CPU {ratio32:.3f}), max |row sum| / bound "
              f"{(rowsum[gb.sum(-1) > 0] / gb.sum(-1)[gb.sum(-1) > 0]).max().item():.3f}")
        assert (g32err <= gb).all()
        assert (gerr <= gb).all(), ratio
        assert (rowsum <= gb.sum(-1)).all()


def _row_bounds(lg, tg, V, eps, grow):
    """(loss bound per row, gradient bound per element) of rows with in-range or ignored targets (clamped for the gather: an ignored row's loss and gradient are exactly
    0 on both sides); a -inf logit is left out of the scales."""
    x64 = lg.double()
    xf = x64.masked_fill(torch.isinf(x64), 0.0)
    tc = tg.clamp(0, V - 1)
    lse64 = torch.logsumexp(x64, -1)
    xt = xf.gather(-1, tc.unsqueeze(-1)).squeeze(-1)
    S = torch.clamp(torch.maximum(torch.maximum(lse64.abs(), xt.abs()), xf.abs().mean(-1)), min=1.0)
    p = torch.softmax(x64, -1)
    onehot = torch.zeros_like(p).scatter_(1, tc.unsqueeze(1), 1.0)
    return loss_bound_c(V, eps) * U * S, grad_bound(V, eps, grow, p, onehot, lse64, xf.abs().amax(-1))


def test_ignore_index_out_of_range_and_inf(dev):
    """target -100: loss 0, gradient 0, left out of 'mean''s denominator ('mean' and its gradient against fp64 torch).  A target of V or -1: NaN loss and a NaN gradient
    row, every other row as without it.  A row with one -inf logit and eps = 0 matches torch: finite loss, zero gradient at that column."""
    from sdvar_amd import seam
    V, N, eps = 1000, 11, 0.1
    lg, tg = torch.randn(N, V, generator=torch.Generator().manual_seed(5)) * 2, torch.randint(0, V, (N,), generator=torch.Generator().manual_seed(6))
    tg[2] = tg[7] = -100
    counted = N - 2
    lgd = lg.to(dev)
    for reduction, g in (("none", _upstream(N, 3)), ("mean", torch.tensor(1.25)), ("sum", torch.tensor(1.0))):
        out64, grad64 = _ref_grad(lg, tg, eps, reduction, g, torch.float64)
        grow = g.double() if reduction == "none" else (g.double() / (counted if reduction == "mean" else 1)).expand(N)
        lb, gb = _row_bounds(lg, tg, V, eps, grow)
        xd = lgd.clone().requires_grad_(True)
        out = seam.cross_entropy(xd, tg.to(dev), eps, reduction)
        out.backward(g.to(dev))
        assert (xd.grad[2] == 0).all() and (xd.grad[7] == 0).all() and (grad64[2] == 0).all() and (grad64[7] == 0).all()
        if reduction == "none":
            assert out[2].item() == 0.0 and out[7].item() == 0.0 and out64[2].item() == 0.0
            assert ((out.cpu().double() - out64).abs() <= lb).all()
        else:           # 'mean' divides by the 9 counted rows, not by 11
            assert (out.cpu().double() - out64).abs() <= lb[tg != -100].sum() / (counted if reduction == "mean" else 1) + 2 * U * out64.abs()
        assert ((xd.grad.cpu().double() - grad64).abs() <= gb).all()
    every = seam.cross_entropy(lgd, torch.full((N,), -100, device=dev), eps, "mean")
    assert torch.isnan(every)                                                          # 0 / 0, as torch
    good = tg.clone()
    good[2], good[7] = 1, 2
    base = lgd.clone().requires_grad_(True)
    lb = seam.cross_entropy(base, good.to(dev), eps)
    lb.sum().backward()
    bad = good.clone()
    bad[3], bad[9] = V, -1
    xd = lgd.clone().requires_grad_(True)
    lo = seam.cross_entropy(xd, bad.to(dev), eps)
    lo.sum().backward()
    keep = torch.ones(N, dtype=torch.bool, device=dev)
    keep[3] = keep[9] = False
    assert torch.isnan(lo[3]) and torch.isnan(lo[9]) and torch.isnan(xd.grad[3]).all() and torch.isnan(xd.grad[9]).all()
    assert torch.equal(lo[keep], lb[keep]) and torch.equal(xd.grad[keep], base.grad[keep])
    assert torch.isnan(seam.cross_entropy(lgd, bad.to(dev), eps, "mean"))
    # one -inf logit, eps = 0
    li = lg.clone()
    li[4, 17] = float("-inf")
    tgi = good.clone()
    tgi[4] = 3
    out64, grad64 = _ref_grad(li, tgi, 0.0, "none", torch.ones(N), torch.float64)
    lb, gb = _row_bounds(li, tgi, V, 0.0, torch.ones(N, dtype=torch.float64))
    xd = li.to(dev).requires_grad_(True)
    out = seam.cross_entropy(xd, tgi.to(dev), 0.0)
    out.sum().backward()
    assert torch.isfinite(out).all() and torch.isfinite(out64).all() and ((out.cpu().double() - out64).abs() <= lb).all()
    assert xd.grad[4, 17].item() == 0.0 and grad64[4, 17].item() == 0.0 and torch.isfinite(xd.grad).all()
    assert ((xd.grad.cpu().double() - grad64).abs() <= gb).all()


def test_strided_view_and_no_grad_bits(dev):
    """A row-strided view (ld > V) is read in place and gives the bits of its contiguous copy, loss and gradient; a view that misses the 16-byte rule is copied once and
    gives the same bits too; the no-grad call gives the bits of the grad call, for every reduction."""
    from sdvar_amd import engine as E, seam
    V, N, eps = 1000, 9, 0.1
    wide = (torch.randn(N, V + 24, generator=torch.Generator().manual_seed(11)) * 3).to(dev)
    tg = torch.randint(0, V, (N,), generator=torch.Generator().manual_seed(12)).to(dev)
    g = _upstream(N, 13).to(dev)
    for off in (4, 3):                  # columns 4 .. V + 3: 16-byte aligned rows at stride V + 24; columns 3 .. V + 2: misaligned
        base = wide.clone().requires_grad_(True)
        view = base[:, off:off + V]
        assert view.stride(0) == V + 24 and (view.data_ptr() % 16 == 0) == (off == 4)
        out = seam.cross_entropy(view, tg, eps)
        out.backward(g)
        dense = wide[:, off:off + V].contiguous().requires_grad_(True)
        outd = seam.cross_entropy(dense, tg, eps)
        outd.backward(g)
        assert torch.equal(out, outd) and torch.equal(base.grad[:, off:off + V], dense.grad)
        assert (base.grad[:, :off] == 0).all() and (base.grad[:, off + V:] == 0).all()
        with torch.no_grad():
            assert torch.equal(seam.cross_entropy(view, tg, eps), out)
        assert torch.equal(seam.cross_entropy(view.detach(), tg, eps), out)
    v = wide[:, 4:V + 4]
    assert v.stride(0) == V + 24 and torch.equal(E.xent_train_fwd(v, tg, eps)[0], seam.cross_entropy(v.contiguous(), tg, eps))          # the engine reads the view itself
    with pytest.raises(E.SdvarError, match="16-byte"):
        E.xent_train_fwd(wide[:, 3:V + 3], tg, eps)
    for reduction in ("mean", "sum"):
        x = v.detach().clone().requires_grad_(True)
        a = seam.cross_entropy(x, tg, eps, reduction)
        with torch.no_grad():
            b = seam.cross_entropy(x, tg, eps, reduction)
        assert torch.equal(a.detach(), b)


def _trainer_expr(loss_fn, logits, gt, lw, B, V, scale=None):
    loss = loss_fn(logits.view(-1, V), gt.view(-1)).view(B, -1).mul(lw).sum(-1).mean()
    (loss if scale is None else loss * scale).backward()
    return loss.detach()


@pytest.mark.parametrize("ed", [None, 5])
def test_trainer_expression(dev, ed):
    """trainer.py:112-120 on B = 3, patch_nums (1, 2, 3) (L = 14), V = 4096, eps 0.1, lw = 1 / L with the last stage's weights x 0.37: loss and the leaf's gradient
    against the same expression in fp64 torch; ed = 5: the progressive case (logits cut to [:, :ed], contiguous as the reference's are).  Under
    torch.autocast(float16) with the loss multiplied by 65536 before backward() the gradient is float32 and EXACTLY 65536 x the unscaled one."""
    import torch.nn as nn
    from sdvar_amd import seam
    B, L, V, eps = 3, 14, 4096, 0.1
    Lu = L if ed is None else ed
    lgfull = torch.randn(B, L, V, generator=torch.Generator().manual_seed(21)) * 2.5
    gt = torch.randint(0, V, (B, L), generator=torch.Generator().manual_seed(22))[:, :Lu].contiguous()
    lg = lgfull[:, :Lu].contiguous()
    lw = torch.ones(1, L) / L
    lw[:, 5:] *= 0.37
    lw = lw[:, :Lu].contiguous()
    x64 = lg.double().requires_grad_(True)
    ref = _trainer_expr(nn.CrossEntropyLoss(label_smoothing=eps, reduction="none"), x64, gt, lw.double(), B, V)
    x32 = lg.clone().requires_grad_(True)
    ref32 = _trainer_expr(nn.CrossEntropyLoss(label_smoothing=eps, reduction="none"), x32, gt, lw, B, V)
    fn = seam.CrossEntropyLoss(label_smoothing=eps, reduction="none")
    xd = lg.to(dev).requires_grad_(True)
    out = _trainer_expr(fn, xd, gt.to(dev), lw.to(dev), B, V)
    flat = lg.double().view(-1, V)
    lse64 = torch.logsumexp(flat, -1)
    xt = flat.gather(-1, gt.view(-1, 1)).squeeze(-1)
    S = torch.clamp(torch.maximum(torch.maximum(lse64.abs(), xt.abs()), flat.abs().mean(-1)), min=1.0)
    w = (lw.double() / B).expand(B, Lu).reshape(-1)
    # the rows' loss bounds through the weighted sum, plus the float32 roundings of mul / sum / mean (at most Lu + B + 2 of them, on non-negative terms that add up to the loss)
    vbound = (w * loss_bound_c(V, eps) * U * S).sum() + (Lu + B + 2) * U * ref.abs()
    assert (out.cpu().double() - ref).abs() <= vbound and (ref32.double() - ref).abs() <= vbound
    p = torch.softmax(flat, -1)
    onehot = torch.zeros_like(p).scatter_(1, gt.view(-1, 1), 1.0)
    gb = grad_bound(V, eps, w, p, onehot, lse64, flat.abs().amax(-1)) + 2 * U * x64.grad.view(-1, V).abs()        # w itself: the roundings of 1 / B and the product
    gerr = (xd.grad.cpu().double().view(-1, V) - x64.grad.view(-1, V)).abs()
    print(f"\ntrainer expression ed={ed}: loss err/bound {((out.cpu().double() - ref).abs() / vbound).item():.3f}, grad err/bound {(gerr / gb).max().item():.3f}")
    assert ((x32.grad.double().view(-1, V) - x64.grad.view(-1, V)).abs() <= gb).all()
    assert (gerr <= gb).all()
    xa = lg.to(dev).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16):
        outa = _trainer_expr(fn, xa, gt.to(dev), lw.to(dev), B, V, scale=65536.0)
    assert xa.grad.dtype == torch.float32 and torch.equal(outa, out)
    assert torch.equal(xa.grad, xd.grad * 65536.0)


def test_install_trainer(dev):
    from types import SimpleNamespace
    from sdvar_amd import seam
    tr = SimpleNamespace(label_smooth=0.1, train_loss=None, val_loss=None)
    seam.install_trainer(tr)
    assert isinstance(tr.train_loss, seam.CrossEntropyLoss) and (tr.train_loss.label_smoothing, tr.train_loss.reduction) == (0.1, "none")
    assert isinstance(tr.val_loss, seam.CrossEntropyLoss) and (tr.val_loss.label_smoothing, tr.val_loss.reduction) == (0.0, "mean")
    V, N = 4096, 37
    lg = torch.randn(N, V, generator=torch.Generator().manual_seed(31)) * 3
    tg = torch.randint(0, V, (N,), generator=torch.Generator().manual_seed(32))
    x64 = lg.double()
    want = F.cross_entropy(x64, tg)
    got = tr.val_loss(lg.to(dev), tg.to(dev))
    lse64 = torch.logsumexp(x64, -1)
    S = torch.clamp(torch.maximum(lse64.abs(), x64.gather(-1, tg.unsqueeze(-1)).squeeze(-1).abs()), min=1.0)
    assert got.dim() == 0 and got.dtype == torch.float32
    assert (got.cpu().double() - want).abs() <= (loss_bound_c(V, 0.0) * U * S).mean() + 2 * U * want.abs()
    tl = tr.train_loss(lg.to(dev), tg.to(dev))
    assert tl.shape == (N,) and torch.allclose(tl.cpu().double(), F.cross_entropy(x64, tg, reduction="none", label_smoothing=0.1), rtol=1e-5, atol=1e-5)
    with pytest.raises(seam.SdvarError, match="label_smooth"):
        seam.install_trainer(SimpleNamespace())


def test_errors_name_the_remedy(dev):
    from sdvar_amd import seam
    x = torch.randn(6, 64, device=dev)
    t = torch.randint(0, 64, (6,), device=dev)
    with pytest.raises(seam.SdvarError, match=r"\.float\(\)"):
        seam.cross_entropy(x.half(), t)
    with pytest.raises(seam.SdvarError, match=r"\.float\(\)"):
        seam.cross_entropy(x.double(), t)
    with pytest.raises(seam.SdvarError, match="weight=None"):
        seam.cross_entropy(x, t, weight=torch.ones(64, device=dev))
    with pytest.raises(seam.SdvarError, match="weight=None"):
        seam.CrossEntropyLoss(weight=torch.ones(64, device=dev))
    with pytest.raises(seam.SdvarError, match=r"view\(-1, V\)"):
        seam.cross_entropy(x.view(2, 3, 64), t.view(2, 3))
    with pytest.raises(seam.SdvarError, match="reduction"):
        seam.cross_entropy(x, t, reduction="batchmean")
    with pytest.raises(seam.SdvarError, match="label_smoothing"):
        seam.cross_entropy(x, t, label_smoothing=1.5)
    with pytest.raises(seam.SdvarError, match="one GPU"):
        seam.cross_entropy(x.cpu(), t)
    xg = x.clone().requires_grad_(True)
    loss = seam.cross_entropy(xg, t, 0.1, "mean")
    with pytest.raises(seam.SdvarError, match="without create_graph"):
        torch.autograd.grad(loss, xg, create_graph=True)
