"""seam.AdamW / seam.install_optimizer (sdvar_optim_grad_stats, sdvar_optim_adamw_step; csrc/optim.hip) against float64 on the CPU, every element asserted.

The error bound of one step (first order, u = 2^-24 per float32 operation, in the kernel's operation order as include/sdvar_hip.h states it), with G = |g'| the true
scaled and clipped gradient, s = sqrt(v'), de = s / sqrt(bc2) + eps, q = |m'| / de and ss = lr / bc1:
  g'   = g * gscale.  gscale = inv_scale * coef carries 7 u: norm = float(sqrt(S) inv_scale) 2 u (S is a float64 sum: its own error is 2^-29 of that), norm + 1e-6f 3 u,
         float(max_norm) and the division 5 u, inv_scale once more and the product 7 u; the product with g makes CG = 8 u G.  (Without scale and clipping g' = g exactly;
         the bound keeps 8.)
  m'   = float(b1) m + float(1 - b1) g':   the first product 2 u b1 |m|, the second (CG + 2) u (1 - b1) G, the sum u (b1 |m| + (1 - b1) G):
         Em = u (3 b1 |m| + (CG + 3)(1 - b1) G) - ABSOLUTE in b1 |m| + (1 - b1) G, so an m' that cancels to nearly nothing is held to the same figure.
  v'   = float(b2) v + (float(1 - b2) g') g':   2 u b2 v; (CG + 2) u then (2 CG + 3) u on (1 - b2) G^2; the sum u v':   Ev = u (3 b2 v + (2 CG + 4)(1 - b2) G^2)
  s    : Es = min(Ev / (2 s), sqrt(Ev)) + u s   (|sqrt a - sqrt b| <= sqrt|a - b| covers v' at and near 0)
  de   : the division by float(sqrt(bc2)) 2 u s / sqrt(bc2), float(eps) u eps, the sum u de:   Ede = Es / sqrt(bc2) + 3 u de
  p'   = p float(1 - lr wd) - ss (m' / de):   2 u |p (1 - lr wd)|;  the quotient Em / de + q Ede / de + u q, float(ss) and the product 2 u more on q;  the difference u |p'|:
         Ep = u (2 |p (1 - lr wd)| + |p'|) + ss (Em / de + q Ede / de + 3 u q)
Each of Em, Ev, Ep also gets a few units of 2^-126 (the smallest normal float32) per operation for results that leave the normal range (g = 1e-30 squares to 1e-60).
torch's own float32 clip_grad_norm_ + AdamW(foreach=False) on the CPU is asserted to meet the same bounds on the same inputs: it does the same roundings in another
order (lerp for m', addcmul for v', addcdiv for p').
global_grad_norm: float(sqrt(S) * inv_scale) from the float64 sum is ONE float32 rounding (2 with a scale that is no power of two); asserted at the 4 u the
feature's specification allows."""
import copy
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ETA = 2.0 ** -126
CG = 8
BETAS, EPS = (0.9, 0.95), 1e-8
GROUP_HYPER = ((1e-3, 0.05), (3e-4, 0.0))          # (lr, weight_decay) of the two groups, one weight decay 0
N_GROUP0 = 8                                       # parameters 0 .. 7 are group 0, the rest group 1


def _shape_set():
    """The numels around every path: 1 (a lone scalar lane), 3 / 4 / 5 (below, at and above one float4), 1023 / 1024 / 1025 (one 256-thread round of float4 and its
    neighbours), CH - 1 / CH / CH + 1 (one chunk, the tail chunk of 1 element) and 2 CH + 3 (three workgroups, a 3-element tail); then a 2-D (5, 7) tensor, a
    1027-element view that starts 4 bytes into its buffer (the scalar path for a whole tensor; its gradient is such a view too), a parameter without a gradient and a
    zero-element parameter."""
    from sdvar_amd import engine as E
    CH = E.OPTIM_CHUNK
    shapes = [(n,) for n in (1, 3, 4, 5, 1023, 1024, 1025, CH - 1, CH, CH + 1, 2 * CH + 3)] + [(5, 7), (1027,), (6,), (0,)]
    return shapes, dict(misaligned=12, nograd=13)


def _many_set():
    """One tensor more than a launch carries: the second launch of every pass holds a single 5-element tensor."""
    from sdvar_amd import engine as E
    return [(5,)] * (E.OPTIM_TENSORS_PER_LAUNCH + 1), dict(misaligned=None, nograd=None)


def _groups(params, hyper=GROUP_HYPER):
    return [dict(params=params[:N_GROUP0], lr=hyper[0][0], weight_decay=hyper[0][1], lr_sc=1.0, wd_sc=1.0),
            dict(params=params[N_GROUP0:], lr=hyper[1][0], weight_decay=hyper[1][1], lr_sc=1.0, wd_sc=0.0)]


def _hyper_of(i, hyper=GROUP_HYPER):
    return hyper[0] if i < N_GROUP0 else hyper[1]


def _grads(shapes, seed, nograd=None, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return [None if i == nograd else torch.randn(s, generator=gen) * scale for i, s in enumerate(shapes)]


_PROBLEMS = {}


def _problem(kind):
    """CPU inputs of a case, built once per session and never modified: parameters, and a non-trivial state - m and v from three torch float32 steps, `step` set to 7."""
    if kind not in _PROBLEMS:
        shapes, special = _shape_set() if kind == "shapes" else _many_set()
        gen = torch.Generator().manual_seed(11 if kind == "shapes" else 12)
        ps = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in shapes]
        opt = torch.optim.AdamW(_groups(ps), betas=BETAS, eps=EPS, foreach=False)
        for k in range(3):
            for p, g in zip(ps, _grads(shapes, 100 + k, special["nograd"], 0.3)):
                p.grad = g
            opt.step()
        for st in opt.state.values():
            st["step"] = torch.tensor(7.0)
        for p in ps:
            p.grad = None
        _PROBLEMS[kind] = types.SimpleNamespace(shapes=shapes, special=special, params=[p.detach().clone() for p in ps], sd=opt.state_dict(),
                                                m=[opt.state[p]["exp_avg"].clone() if p in opt.state else None for p in ps],
                                                v=[opt.state[p]["exp_avg_sq"].clone() if p in opt.state else None for p in ps])
    return _PROBLEMS[kind]


def _device_params(cpu_params, dev, misaligned=None):
    out = []
    for i, p in enumerate(cpu_params):
        if i == misaligned:
            buf = torch.empty(p.numel() + 1, device=dev)
            buf[1:].copy_(p)
            q = torch.nn.Parameter(buf[1:])
            assert q.data_ptr() % 16 == 4 and q.is_contiguous()
        else:
            q = torch.nn.Parameter(p.detach().clone().to(dev))
        out.append(q)
    return out


def _set_grads(params, grads, dev, misaligned=None):
    """Freshly allocated gradient tensors (zero_grad(set_to_none=True) in the reference: new addresses every step)."""
    for i, (p, g) in enumerate(zip(params, grads)):
        if g is None:
            p.grad = None
        elif i == misaligned:
            buf = torch.empty(g.numel() + 1, device=dev)
            buf[1:].copy_(g)
            p.grad = buf[1:]
        else:
            p.grad = g.detach().clone().to(dev)


def ref_norm_coef(grads, grad_clip, inv_scale=1.0):
    tot = math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads if g is not None and g.numel())) * inv_scale
    return tot, (1.0 if grad_clip <= 0 else min(1.0, grad_clip / (tot + 1e-6)))


def ref_step(p, g, m, v, step_new, lr, wd, gfac):
    """One AdamW step of one tensor in float64 from float32 (or float64) inputs -> (p', m', v') and the bounds (Ep, Em, Ev) of the module docstring."""
    b1, b2 = BETAS
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    gp = g * gfac
    m2 = b1 * m + (1 - b1) * gp
    v2 = b2 * v + (1 - b2) * gp * gp
    bc1, rb = 1 - b1 ** step_new, math.sqrt(1 - b2 ** step_new)
    s = v2.sqrt()
    de = s / rb + EPS
    ss, decay = lr / bc1, 1 - lr * wd
    p2 = p * decay - ss * m2 / de
    G = gp.abs()
    Em = U * (3 * b1 * m.abs() + (CG + 3) * (1 - b1) * G) + 3 * ETA
    Ev = U * (3 * b2 * v + (2 * CG + 4) * (1 - b2) * G * G) + 4 * ETA
    Es = torch.minimum(torch.where(s > 0, Ev / (2 * s), torch.full_like(s, math.inf)), Ev.sqrt()) + U * s
    Ede = Es / rb + 3 * U * de
    q = m2.abs() / de
    Ep = U * (2 * (p * decay).abs() + p2.abs()) + ss * (Em / de + q * Ede / de + 3 * U * q) + 3 * ETA
    return (p2, m2, v2), (Ep, Em, Ev)


def _ratio(x, ref, bound):
    return ((x.detach().cpu().double().reshape(ref.shape) - ref).abs() / bound).max().item() if ref.numel() else 0.0


def _check_against_ref(label, params, opt, refs, worst):
    """p, m, v of every tensor that took part within its bounds; `worst` collects the largest err / bound ratios per quantity."""
    for i, (p, ref) in enumerate(zip(params, refs)):
        if ref is None:
            continue
        (p2, m2, v2), (Ep, Em, Ev) = ref
        st = opt.state[p]
        for name, x, r, b in (("p", p, p2, Ep), ("m", st["exp_avg"], m2, Em), ("v", st["exp_avg_sq"], v2, Ev)):
            ratio = _ratio(x, r, b)
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert ratio <= 1.0, f"{label}: tensor {i} ({tuple(p.shape)}): {name} err / bound = {ratio:.3f}"


def _seam_opt(params, sd, grad_clip, hyper=GROUP_HYPER):
    from sdvar_amd import seam
    opt = seam.AdamW(_groups(params, hyper), betas=BETAS, eps=EPS, grad_clip=grad_clip)
    if sd is not None:
        opt.load_state_dict(copy.deepcopy(sd))
    return opt


def _snapshot(params, opt):
    out = []
    for p in params:
        st = opt.state.get(p, {})
        out.append(tuple(t.detach().clone() for t in (p, *(st[k] for k in ("exp_avg", "exp_avg_sq", "step") if k in st))))
    return out


def _same_bits(a, b):
    return all(len(x) == len(y) and all(torch.equal(s.cpu(), t.cpu()) for s, t in zip(x, y)) for x, y in zip(a, b))


@pytest.mark.parametrize("grad_clip", [0.0, 0.5])
@pytest.mark.parametrize("kind", ["shapes", "many"])
def test_single_step_vs_fp64(dev, kind, grad_clip):
    """One step from a non-trivial state (m, v from three torch steps, step = 7 held on the CPU as a non-fused torch checkpoint holds it) over the shape set and over
    TENSORS_PER_LAUNCH + 1 tensors, without clipping and with a grad_clip that bites: p, m, v within the module docstring's bounds of the float64 step, as is torch's own
    float32 CPU step; step becomes 8; the `_version` of every updated parameter moves; global_grad_norm within 4 u; the parameter without a gradient and its absent state are untouched; the gradients keep their bits;
    two runs are bit-identical."""
    from sdvar_amd import engine as E
    pr = _problem(kind)
    mis, nog = pr.special["misaligned"], pr.special["nograd"]
    grads = _grads(pr.shapes, 501, nog, 0.3)
    norm64, coef64 = ref_norm_coef(grads, grad_clip)
    assert (coef64 < 0.9) == (grad_clip > 0), coef64
    refs = [None if g is None or g.numel() == 0 else ref_step(p, g, m, v, 8.0, *_hyper_of(i), coef64)
            for i, (p, g, m, v) in enumerate(zip(pr.params, grads, pr.m, pr.v))]
    worst, runs = {}, []
    for _ in range(2):
        params = _device_params(pr.params, dev, mis)
        opt = _seam_opt(params, pr.sd, grad_clip)
        _set_grads(params, grads, dev, mis)
        versions = [p._version for p in params]
        opt.step()
        assert all((p._version > v0) == (refs[i] is not None) for i, (p, v0) in enumerate(zip(params, versions)))          # written behind torch's back, but declared
        _check_against_ref(f"seam {kind}", params, opt, refs, worst)
        for i, p in enumerate(params):
            if refs[i] is not None:
                st = opt.state[p]["step"]
                assert st.device == p.device and st.dtype == torch.float32 and st.dim() == 0 and st.item() == 8.0
                assert torch.equal(p.grad.cpu(), grads[i])                      # read, never modified
        if nog is not None:
            assert torch.equal(params[nog].cpu(), pr.params[nog]) and len(opt.state[params[nog]]) == 0
        gn = opt.global_grad_norm
        assert gn.dim() == 0 and gn.dtype == torch.float32 and gn.device == params[0].device
        nerr = abs(gn.item() - norm64) / norm64
        rec = opt.stats_record.cpu()
        assert nerr <= 4 * U, nerr
        assert rec[2].item() == 0.0 and abs(rec[1].item() - coef64) <= 5 * U * coef64
        runs.append(_snapshot(params, opt))
    assert _same_bits(runs[0], runs[1])
    if kind == "many":
        assert len(pr.shapes) > E.OPTIM_TENSORS_PER_LAUNCH

    # torch's own float32 step on the CPU meets the same bounds on the same inputs
    tparams = [torch.nn.Parameter(p.clone()) for p in pr.params]
    topt = torch.optim.AdamW(_groups(tparams), betas=BETAS, eps=EPS, foreach=False)
    topt.load_state_dict(copy.deepcopy(pr.sd))
    for p, g in zip(tparams, grads):
        p.grad = None if g is None else g.clone()
    if grad_clip > 0:
        torch.nn.utils.clip_grad_norm_(tparams, grad_clip, foreach=False)
    topt.step()
    tworst = {}
    _check_against_ref(f"torch float32 {kind}", tparams, topt, refs, tworst)
    print(f"\nadamw {kind} grad_clip={grad_clip}: worst err / bound  seam p {worst['p']:.3f} m {worst['m']:.3f} v {worst['v']:.3f};  torch float32 on the CPU "
          f"p {tworst['p']:.3f} m {tworst['m']:.3f} v {tworst['v']:.3f};  norm err {nerr / U:.2f} u")


def _fresh(dev, shapes, seed, grad_clip, hyper=GROUP_HYPER):
    """Device parameters without state (m = v = 0, step 0) and their CPU twins."""
    gen = torch.Generator().manual_seed(seed)
    cpu = [torch.randn(s, generator=gen) for s in shapes]
    params = _device_params(cpu, dev)
    return cpu, params, _seam_opt(params, None, grad_clip, hyper)


def test_hard_gradients(dev):
    """Gradients whose float32 squares overflow (1e25: the norm must come out finite and right, and the clipped update must match the float64 one), whose squares
    underflow (1e-30: a non-zero norm, coef exactly 1), and g = 0 on v = 0 (0 / (0 + eps): no NaN, p moves by the weight decay alone)."""
    from sdvar_amd import engine as E
    shapes = [(5,), (1025,), (E.OPTIM_CHUNK + 1,)] + [(3,)] * 6          # parameter 8 is in the group without weight decay
    worst = {}
    for val, clip in ((1e25, 2.0), (1e-30, 2.0)):
        cpu, params, opt = _fresh(dev, shapes, 21, clip)
        grads = [torch.full(s, val) for s in shapes]
        grads[1][::2] *= -1
        norm64, coef64 = ref_norm_coef(grads, clip)
        _set_grads(params, grads, dev)
        opt.step()
        rec = opt.stats_record.cpu()
        assert math.isfinite(rec[0].item()) and rec[0].item() > 0 and abs(rec[0].item() - norm64) <= 4 * U * norm64, (rec, norm64)
        assert rec[2].item() == 0.0
        if val < 1:
            assert rec[1].item() == 1.0 and coef64 == 1.0
        else:
            assert abs(rec[1].item() - coef64) <= 5 * U * coef64
        refs = [ref_step(p, g, torch.zeros_like(p), torch.zeros_like(p), 1.0, *_hyper_of(i), coef64) for i, (p, g) in enumerate(zip(cpu, grads))]
        _check_against_ref(f"g = {val}", params, opt, refs, worst)
    cpu, params, opt = _fresh(dev, shapes, 22, 2.0)
    _set_grads(params, [torch.zeros(s) for s in shapes], dev)
    opt.step()
    assert opt.global_grad_norm.item() == 0.0 and opt.stats_record[1].item() == 1.0
    for i, (c, p) in enumerate(zip(cpu, params)):
        lr, wd = _hyper_of(i)
        assert torch.isfinite(p).all()
        assert torch.equal(p.cpu(), c * torch.tensor(1 - lr * wd, dtype=torch.float64).float())          # one float32 product, the decay factor rounded from float64
        assert opt.state[p]["exp_avg"].abs().max().item() == 0.0 and opt.state[p]["exp_avg_sq"].abs().max().item() == 0.0 and opt.state[p]["step"].item() == 1.0
    print(f"\nadamw hard gradients: worst err / bound p {worst['p']:.3f} m {worst['m']:.3f} v {worst['v']:.3f}")


@pytest.mark.parametrize("bad", [math.inf, math.nan])
def test_nonfinite_gradient_skips_the_step(dev, bad):
    """One inf / NaN in the LAST element of the last chunk of the largest tensor, no scaler: p, m, v and every step keep their bits, global_grad_norm is not finite; the
    next clean step updates as a step from the untouched state does, with step advanced by one only."""
    pr = _problem("shapes")
    mis, nog = pr.special["misaligned"], pr.special["nograd"]
    params = _device_params(pr.params, dev, mis)
    opt = _seam_opt(params, pr.sd, 0.5)
    grads = _grads(pr.shapes, 601, nog, 0.3)
    big = max(range(len(pr.shapes)), key=lambda i: pr.params[i].numel())
    poisoned = [None if g is None else g.clone() for g in grads]
    poisoned[big][-1] = bad
    before_p = [p.detach().clone() for p in params]
    _set_grads(params, poisoned, dev, mis)
    opt.step()
    assert not math.isfinite(opt.global_grad_norm.item()) and opt.stats_record[2].item() == 1.0
    for i, p in enumerate(params):
        assert torch.equal(p, before_p[i])
        if grads[i] is not None and grads[i].numel():
            st = opt.state[p]
            assert torch.equal(st["exp_avg"].cpu(), pr.m[i]) and torch.equal(st["exp_avg_sq"].cpu(), pr.v[i]) and st["step"].item() == 7.0
    # the next clean step: step 8, and the result of a step from the untouched state
    norm64, coef64 = ref_norm_coef(grads, 0.5)
    refs = [None if g is None or g.numel() == 0 else ref_step(p, g, m, v, 8.0, *_hyper_of(i), coef64)
            for i, (p, g, m, v) in enumerate(zip(pr.params, grads, pr.m, pr.v))]
    _set_grads(params, grads, dev, mis)
    opt.step()
    assert opt.stats_record[2].item() == 0.0 and abs(opt.global_grad_norm.item() - norm64) <= 4 * U * norm64
    _check_against_ref("after a skipped step", params, opt, refs, {})
    assert all(opt.state[p]["step"].item() == 8.0 for i, p in enumerate(params) if refs[i] is not None)


def _mlp_params(dev, seed=31):
    gen = torch.Generator().manual_seed(seed)
    shapes = [(32, 16), (32,), (32, 32), (32,), (4, 32), (4,)]
    cpu = [torch.randn(s, generator=gen) * (0.3 if len(s) == 2 else 0.1) for s in shapes]
    x, y = torch.randn(64, 16, generator=gen), torch.randn(64, 4, generator=gen)
    return cpu, [torch.nn.Parameter(c.clone().to(dev)) for c in cpu], x.to(dev), y.to(dev)


def _mlp_loss(ps, x, y):
    h = torch.tanh(x @ ps[0].t() + ps[1])
    h = torch.tanh(h @ ps[2].t() + ps[3])
    return ((h @ ps[4].t() + ps[5] - y) ** 2).mean()


def _drive(opt, scaler, params, x, y, unscale, poison=None):
    """The reference's AmpOptimizer.backward_clip_step restated on torch's public calls (nothing of the reference is imported)."""
    scaler.scale(_mlp_loss(params, x, y)).backward()
    if poison is not None:
        params[poison].grad.view(-1)[0] = math.inf
    if unscale:
        scaler.unscale_(opt)
    scaler.step(opt)
    norm = opt.global_grad_norm
    scaler.update()
    opt.zero_grad(set_to_none=True)
    return norm


@pytest.mark.parametrize("unscale", [True, False])
def test_gradscaler_contract(dev, unscale):
    """GradScaler(init_scale=2^11) driving seam.AdamW on a three-layer float32 MLP, with the explicit unscale_ (the reference's flow: grad_scale arrives as None) and
    without it (grad_scale = the scale tensor: the kernel unscales).  A clean step lands within the single-step bound of the float64 step on the UNSCALED gradients, as
    does seam.AdamW fed those gradients directly; global_grad_norm is the unscaled norm.  With an inf in one gradient the step is skipped and the scale halves."""
    from sdvar_amd import seam
    hyper = ((1e-2, 0.05), (1e-2, 0.05))
    with torch.enable_grad():
        cpu, params, x, y = _mlp_params(dev)
        _, twin, _, _ = _mlp_params(dev)
        _mlp_loss(twin, x, y).backward()
        grads = [p.grad.detach().cpu().clone() for p in twin]
        norm64, coef64 = ref_norm_coef(grads, 0.05)
        assert coef64 < 0.9
        refs = [ref_step(p, g, torch.zeros_like(p), torch.zeros_like(p), 1.0, *hyper[0], coef64) for p, g in zip(cpu, grads)]
        direct = seam.AdamW(twin, lr=hyper[0][0], weight_decay=hyper[0][1], betas=BETAS, eps=EPS, grad_clip=0.05)
        direct.step()
        _check_against_ref("direct", twin, direct, refs, {})

        opt = seam.AdamW(params, lr=hyper[0][0], weight_decay=hyper[0][1], betas=BETAS, eps=EPS, grad_clip=0.05)
        scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 11)
        norm = _drive(opt, scaler, params, x, y, unscale)
        worst = {}
        _check_against_ref(f"scaler unscale_={unscale}", params, opt, refs, worst)
        assert abs(norm.item() - norm64) <= 4 * U * norm64, (norm.item(), norm64)
        assert scaler.get_scale() == 2.0 ** 11 and all(opt.state[p]["step"].item() == 1.0 for p in params)
        assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")

        before = _snapshot(params, opt)
        norm = _drive(opt, scaler, params, x, y, unscale, poison=2)
        assert _same_bits(before, _snapshot(params, opt))
        assert not math.isfinite(norm.item()) and scaler.get_scale() == 2.0 ** 10
    print(f"\nadamw under GradScaler, unscale_={unscale}: worst err / bound p {worst['p']:.3f} m {worst['m']:.3f} v {worst['v']:.3f}")


def test_back_to_back_steps_without_sync(dev):
    """Two steps enqueued with no synchronisation between them, on freshly allocated gradient tensors and with another lr, equal the same two steps with a device
    synchronise in between, bit for bit: nothing the first step's launches read may be overwritten by the host work of the second."""
    pr = _problem("many")
    g1, g2 = _grads(pr.shapes, 701), _grads(pr.shapes, 702)
    out = []
    for sync in (False, True):
        params = _device_params(pr.params, dev)
        opt = _seam_opt(params, pr.sd, 0.5)
        _set_grads(params, g1, dev)
        opt.step()
        if sync:
            torch.cuda.synchronize()
        for group in opt.param_groups:
            group["lr"] *= 0.37
        _set_grads(params, g2, dev)
        opt.step()
        torch.cuda.synchronize()
        out.append(_snapshot(params, opt))
        assert all(opt.state[p]["step"].item() == 9.0 for p in params)
    assert _same_bits(out[0], out[1])


def test_five_step_trajectory(dev):
    """Five steps over the shape set on a fixed-seed gradient stream with grad_clip = 1 and lr / weight decay changed every step (as lr_wd_annealing does): the largest
    |p - p64| of seam.AdamW may be at most twice that of torch's float32 CPU AdamW(foreach=False) after clip_grad_norm_ on the same stream, plus one ulp of the largest
    |p|.  Both do the same number of roundings per step in a different order; 2 is the allowance for the order, not a measured figure.
    Measured: the two errors are printed by this test and recorded in DESIGN.md section 4n."""
    pr = _problem("shapes")
    mis, nog = pr.special["misaligned"], pr.special["nograd"]
    params = _device_params(pr.params, dev, mis)
    opt = _seam_opt(params, pr.sd, 1.0)
    tparams = [torch.nn.Parameter(p.clone()) for p in pr.params]
    topt = torch.optim.AdamW(_groups(tparams), betas=BETAS, eps=EPS, foreach=False)
    topt.load_state_dict(copy.deepcopy(pr.sd))
    p64 = [p.double() for p in pr.params]
    m64 = [None if m is None else m.double() for m in pr.m]
    v64 = [None if v is None else v.double() for v in pr.v]
    for k in range(5):
        hyper = tuple((lr * (1.0 - 0.15 * k), wd * (1.0 + 0.3 * k)) for lr, wd in GROUP_HYPER)
        for o in (opt, topt):
            for group, (lr, wd) in zip(o.param_groups, hyper):
                group["lr"], group["weight_decay"] = lr, wd
        grads = _grads(pr.shapes, 800 + k, nog, 0.5)
        _, coef64 = ref_norm_coef(grads, 1.0)
        assert coef64 < 1.0
        for i, g in enumerate(grads):
            if g is not None and g.numel():
                (p64[i], m64[i], v64[i]), _ = ref_step(p64[i], g, m64[i], v64[i], 8.0 + k, *_hyper_of(i, hyper), coef64)
        _set_grads(params, grads, dev, mis)
        opt.step()
        for p, g in zip(tparams, grads):
            p.grad = None if g is None else g.clone()
        torch.nn.utils.clip_grad_norm_(tparams, 1.0, foreach=False)
        topt.step()
    err_s = max((p.detach().cpu().double() - r).abs().max().item() for p, r in zip(params, p64) if r.numel())
    err_t = max((p.detach().double() - r).abs().max().item() for p, r in zip(tparams, p64) if r.numel())
    pmax = max(r.abs().max().item() for r in p64 if r.numel())
    ulp = 2.0 ** (math.floor(math.log2(pmax)) - 23)
    print(f"\nadamw five steps: max |p - p64|  seam {err_s:.3e}  torch float32 on the CPU {err_t:.3e}  (one ulp of max |p| = {pmax:.3f}: {ulp:.3e})")
    assert all(opt.state[p]["step"].item() == 12.0 for i, p in enumerate(params) if i != nog and p.numel())
    assert err_s <= 2 * err_t + ulp, (err_s, err_t, ulp)


def test_install_optimizer_continues_a_torch_run(dev):
    """A stand-in AmpOptimizer whose torch.optim.AdamW(fused=True) has taken two steps: after install_optimizer one seam step matches the float64 continuation of that
    state (clipped: late clipping is on), and after loading the seam's state_dict() back into torch.optim.AdamW(fused=True) the next torch step matches too."""
    from sdvar_amd import seam
    shapes = [(5, 7), (1025,), (3,)] + [(4,)] * 5 + [(33,), (1,)]
    gen = torch.Generator().manual_seed(41)
    cpu = [torch.randn(s, generator=gen) for s in shapes]
    params = _device_params(cpu, dev)
    topt = torch.optim.AdamW(_groups(params), betas=BETAS, eps=EPS, fused=True)
    for k in range(2):
        _set_grads(params, _grads(shapes, 900 + k, None, 0.3), dev)
        topt.step()
    vo = types.SimpleNamespace(optimizer=topt, grad_clip=0.5, early_clipping=True, late_clipping=False)
    seam.install_optimizer(vo)
    assert type(vo.optimizer) is seam.AdamW and vo.late_clipping is True and vo.early_clipping is False
    state = lambda: ([p.detach().cpu().clone() for p in params], [vo.optimizer.state[p]["exp_avg"].cpu().clone() for p in params],
                     [vo.optimizer.state[p]["exp_avg_sq"].cpu().clone() for p in params])
    p0, m0, v0 = state()
    grads = _grads(shapes, 902, None, 0.3)
    norm64, coef64 = ref_norm_coef(grads, 0.5)
    refs = [ref_step(p, g, m, v, 3.0, *_hyper_of(i), coef64) for i, (p, g, m, v) in enumerate(zip(p0, grads, m0, v0))]
    _set_grads(params, grads, dev)
    vo.optimizer.step()
    _check_against_ref("seam after torch", params, vo.optimizer, refs, {})
    assert abs(vo.optimizer.global_grad_norm.item() - norm64) <= 4 * U * norm64

    p1, m1, v1 = state()
    back = torch.optim.AdamW(_groups(params), betas=BETAS, eps=EPS, fused=True)
    back.load_state_dict(vo.optimizer.state_dict())
    grads = _grads(shapes, 903, None, 0.3)
    refs = [ref_step(p, g, m, v, 4.0, *_hyper_of(i), 1.0) for i, (p, g, m, v) in enumerate(zip(p1, grads, m1, v1))]
    _set_grads(params, grads, dev)
    back.step()
    _check_against_ref("torch after seam", params, back, refs, {})
    assert all(back.state[p]["step"].item() == 4.0 for p in params)
