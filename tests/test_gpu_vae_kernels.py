"""The VQVAE decoder's kernels one by one against fp64 on the CPU (csrc/vae.hip, csrc/conv.hip): GroupNorm statistics (stand-alone and fused into the conv
epilogue), the fused up-sampling convolution, the three attention kernels and conv_out - under inputs whose statistics real checkpoints show (group means far
from 0 next to their spread, non-trivial GroupNorm affines, attention scores over +-30) - and the whole decoder under a checkpoint-like init.

Bars (from the project, not from these measurements): 2e-5 * max(1, |ref|) for every single-kernel comparison (the bar of test_gpu_vae.py's convolution and prep
tests and of the attention tests), plus the f16x2 planes' own 2^-22 relative / 2^-25 absolute representation floor where a test reads planes; 1e-4 on the image
for the whole decoder.  |mean| / std of a group stays <= 100: the statistics are stored as float, so the mean alone carries half an ulp of |mean| (3.8e-6 std at
100) and from |mean| / std ~ 256 on that alone exceeds the bar - a limit of the format, not of the kernels."""
import ctypes as C
import time

import pytest
import torch
import torch.nn.functional as F

from conftest import rnd
from sdvar_amd import engine as E

pytestmark = pytest.mark.gpu

BAR = 2e-5
F16_REL, F16_ABS = 2.0 ** -22, 2.0 ** -25
RATIOS = (0, 10, 30, 100)
NPL = {3: 3, 2: 2}
VARIANTS = [(3, None), (2, 0), (2, 1), (2, 2)]          # (plane format, f16x2 K loop "conv_pp"): bf16x3 and the three f16x2 loops


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(16)
    yield
    torch.set_num_threads(n)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _rows(x):
    """(B, C, H, W) -> channel-last rows (B H W, C)"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def _unrows(r, B, H, W):
    return r.view(B, H, W, -1).permute(0, 3, 1, 2)


def _guard(W):
    return (W + 3 + 15) // 16 * 16


def _unplanes_any(xp, pf):
    if pf == 3:
        return sum((xp[k].to(torch.int32) << 16).view(torch.float32).double() for k in range(3))
    return sum(xp[k].view(torch.float16).double() for k in range(2))


def _rel_err(got, want):
    """max |got - want| / max(1, |want|), fp64"""
    return float(((got - want).abs() / want.abs().clamp(min=1.0)).max())


def _set_pp(lib, pp):
    E._check(lib.sdvar_debug_set_variant(b"conv_pp", -1 if pp is None else pp))


def dc_offsets(B, C, std, seed=0):
    """(B, C) per-channel DC offsets: group g of image b gets |mean| / std = RATIOS[(g + b + seed) % 4], the sign alternating every 4 groups (and per image)."""
    dc = torch.empty(B, C, dtype=torch.float64)
    cpg = C // 32
    for b in range(B):
        for g in range(32):
            r = RATIOS[(g + b + seed) % 4]
            s = -1.0 if (g // 4 + b) % 2 else 1.0
            dc[b, g * cpg:(g + 1) * cpg] = s * r * std[b]
    return dc


def group_stats64(x):
    """x (B, C, H, W) fp64 -> mean, rstd (B, 32) in fp64 (eps 1e-6, basic_vae.py:20)"""
    B = x.shape[0]
    xg = x.reshape(B, 32, -1)
    return xg.mean(-1), 1.0 / torch.sqrt(xg.var(-1, unbiased=False) + 1e-6)


def normalised_err(x64, stats):
    """x64 (B, C, H, W) fp64 on the CPU, stats (B, 32, 2) float from the HIP path: max |(x - m) r - (x - m64) r64| / max(1, |(x - m64) r64|)"""
    B = x64.shape[0]
    m64, r64 = group_stats64(x64)
    st = stats.double().cpu()
    xg = x64.reshape(B, 32, -1)
    want = (xg - m64[..., None]) * r64[..., None]
    got = (xg - st[..., 0:1]) * st[..., 1:2]
    return _rel_err(got, want)


def ratios_reached(x64):
    B = x64.shape[0]
    xg = x64.reshape(B, 32, -1)
    return (xg.mean(-1).abs() / xg.std(-1, unbiased=False)).max().item()


# ---------------------------------------------------------------------------------------------------- A. stand-alone GroupNorm statistics
def _a_input(C, H, W):
    """N(0, 1) x (1, 0.37) per image; every group then shifted so that its sample mean is dc_offsets' ratio times its sample std (ratios exactly 0 .. 100)"""
    B = 2
    std = torch.tensor([1.0, 0.37], dtype=torch.float64)
    x = rnd(100 + C + H + W, (B, C, H, W)).double() * std[:, None, None, None]
    xg = x.view(B, 32, -1)
    ratio = dc_offsets(B, C, torch.ones(B, dtype=torch.float64))[:, ::C // 32]
    xg += (ratio * xg.std(-1, unbiased=False) - xg.mean(-1))[..., None]
    return x.float()


A_SHAPES = [(C, H, H) for C in (128, 160, 320, 640) for H in (8, 16, 64, 130, 256)] + [(160, 40, 72)]


@pytest.mark.parametrize("C,H,W", A_SHAPES)
def test_gn_stats_standalone(dev, C, H, W):
    """sdvar_op_vae_gn_stats (gn_partial_kernel + gn_finalize_kernel with the decoder's chunking): H = 130 has a ragged last chunk (3 rows per chunk, 1 in the
    last), H = 256 the longest fp32 runs per thread; (160, 40, 72) is rectangular.  Groups at |mean| / std 0, 10, 30, 100 with mixed signs, two images of different
    spread.  Measured before the fix (one-pass variance): see DESIGN.md section 4b."""
    lib = E.load_library()
    x = _a_input(C, H, W)
    B = x.shape[0]
    part = torch.zeros(B * min(H, 64) * 64, dtype=torch.float64, device=dev)
    stats = torch.zeros(B, 32, 2, device=dev)
    xr = _rows(x.to(dev))                        # every device argument stays referenced until the launch is done (no temporary is freed early)
    E._check(lib.sdvar_op_vae_gn_stats(_p(xr), B, C, H, W, _p(part), _p(stats), _st()))
    torch.cuda.synchronize()
    err = normalised_err(x.double(), stats)
    print(f"gn_stats C={C} H={H} W={W}: {err:.2e} (|mean|/std up to {ratios_reached(x.double()):.0f})")
    assert err <= BAR, err


@pytest.mark.parametrize("pf", [3, 2])
@pytest.mark.parametrize("C,H,W", A_SHAPES)
def test_gn_stats_then_prep_groupnorm_silu(dev, C, H, W, pf):
    """The same tensors through the statistics pass and sdvar_op_vae_prep (mode 3: GroupNorm with gamma ~ 1 + N(0, 0.3), beta ~ N(0, 0.5), then SiLU)
    against fp64 GroupNorm + SiLU."""
    lib = E.load_library()
    x = _a_input(C, H, W)
    B = x.shape[0]
    gamma, beta = 1 + rnd(7, (C,), 0.3), rnd(8, (C,), 0.5)
    xr, gd, bd = _rows(x.to(dev)), gamma.to(dev), beta.to(dev)
    part = torch.zeros(B * min(H, 64) * 64, dtype=torch.float64, device=dev)
    stats = torch.zeros(B, 32, 2, device=dev)
    E._check(lib.sdvar_op_vae_gn_stats(_p(xr), B, C, H, W, _p(part), _p(stats), _st()))
    G = _guard(W); M = B * (H + 2) * (W + 2); R = M + 2 * G
    xp = torch.full((pf, C // 32, R, 32), 0x7FC0 if pf == 3 else 0x7E00, dtype=torch.int16, device=dev)
    E._check(lib.sdvar_op_vae_prep(_p(xr), _p(stats), _p(gd), _p(bd), _p(xp), (C // 32) * R * 32, pf, B, C, H, W, 0, 3, G, _st()))
    torch.cuda.synchronize()
    v = _unplanes_any(xp, pf).permute(1, 0, 2).reshape(R, C)[G:G + M].view(B, H + 2, W + 2, C)[:, 1:-1, 1:-1].cpu()
    del xp
    want = F.silu(F.group_norm(x.double(), 32, gamma.double(), beta.double(), eps=1e-6)).permute(0, 2, 3, 1)
    bound = BAR * want.abs().clamp(min=1.0) + (F16_REL * want.abs() + F16_ABS if pf == 2 else 0.0)
    excess = ((v - want).abs() - bound).max().item()
    print(f"gn_stats + prep pf={pf} C={C} H={H} W={W}: max|err| {(v - want).abs().max().item():.2e}")
    assert excess <= 0, excess


# ---------------------------------------------------------------------------------------------------- conv helpers
def _x_planes(lib, x, pf, dev):
    """(B, C, H, W) float -> the decoder's operand planes of x (sdvar_op_vae_prep mode 0): (planes, plane stride, rows, guard)"""
    B, Cin, H, W = x.shape
    G = _guard(W); R = B * (H + 2) * (W + 2) + 2 * G
    xp = torch.full((pf, Cin // 32, R, 32), 0x7FC0 if pf == 3 else 0x7E00, dtype=torch.int16, device=dev)
    xr = _rows(x.to(dev))
    E._check(lib.sdvar_op_vae_prep(_p(xr), None, None, None, _p(xp), (Cin // 32) * R * 32, pf, B, Cin, H, W, 0, 0, G, _st()))
    torch.cuda.synchronize()
    return xp, (Cin // 32) * R * 32, R, G


def _w_planes(lib, w, pf, dev):
    """3x3 / 1x1 weight (Cout, Cin, k, k) -> planes, scale (f16x2) as the decoder binds them"""
    Cout, Cin, k, _ = w.shape
    taps = k * k
    wp = torch.zeros(pf, taps * Cin // 32, Cout, 32, dtype=torch.int16, device=dev)
    wsc = torch.zeros(4, device=dev)
    wd = w.to(dev).contiguous()
    E._check(lib.sdvar_op_conv_weight_planes(_p(wd), _p(wp), Cout, Cin, taps, taps * Cin * Cout, pf, _p(wsc), _st()))
    torch.cuda.synchronize()
    return wp, (wsc if pf == 2 else None)


def _upconv_planes(lib, w, pf, dev):
    """Upsample2x weight (C, C, 3, 3) -> four phase plane sets npl * wps apart and the f16x2 scale, as the decoder's binder builds them: the phase weights of
    sdvar_op_upconv_weights, one weight scale over all four phases (f16x2), each phase packed with taps = 4."""
    Cout, Cin = w.shape[:2]
    wps = 4 * Cin * Cout
    weff = torch.zeros(4, Cout, Cin, 4, device=dev)
    wd = w.to(dev).contiguous()
    E._check(lib.sdvar_op_upconv_weights(_p(wd), _p(weff), Cout, Cin, _st()))
    wp = torch.zeros(4, pf, wps, dtype=torch.int16, device=dev)
    wsc = None
    if pf == 2:                                  # the scale of all four phases (weight_scale_f16 over weff, as Binder::upconv); 2^S * weff is exact
        wsc = torch.zeros(4, device=dev)
        tmp = torch.zeros(2, 16 * Cout * Cin, dtype=torch.int16, device=dev)
        E._check(lib.sdvar_op_split_planes_f16(_p(weff), _p(tmp), 16 * Cout, Cin, 16 * Cout * Cin, _p(wsc), _st()))
        weff = weff * wsc[0]
    for ph in range(4):
        E._check(lib.sdvar_op_conv_weight_planes(_p(weff[ph]), _p(wp[ph]), Cout, Cin, 4, wps, pf, None, _st()))
    torch.cuda.synchronize()
    return wp, wps, wsc


def _conv_ex(lib, xpl, wp, wps, wsc, bias, res, B, H, W, N, Cin, taps, pf, dev, up=-1, w_phase_stride=0, split=0, ws=None, gn=True):
    xp, xps, R, G = xpl
    Ho, Wo = (2 * H, 2 * W) if up >= 0 else (H, W)
    out = torch.full((B * Ho * Wo, N), float("nan"), device=dev)
    part = torch.zeros(B * ((H * W) // 256 + 1) * 64 * (4 if up >= 0 else 1), dtype=torch.float64, device=dev) if gn else None
    stats = torch.zeros(B, 32, 2, device=dev)
    done = C.c_int32(-1)
    E._check(lib.sdvar_op_conv_planes_ex(_p(xp), xps, R, G, _p(wp), wps, pf, _p(wsc), _p(bias), _p(res), _p(out), B, H, W, N, Cin, taps, _p(ws),
                                         ws.numel() if ws is not None else 0, split, up, w_phase_stride, _p(part), _p(stats) if gn else None,
                                         C.byref(done) if gn else None, _st()))
    torch.cuda.synchronize()
    return out, stats, done.value


# ---------------------------------------------------------------------------------------------------- B. statistics fused into the conv epilogue
@pytest.mark.parametrize("pf,pp", VARIANTS)
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("N", [128, 160, 320, 640])
@pytest.mark.parametrize("HW", [16, 32, 64])
def test_conv_fused_gn_stats(dev, pf, pp, res, N, HW):
    """sdvar_op_conv_planes_ex with fused statistics (conv_epilogue / conv_epilogue16): the output carries the DC offsets of A through its bias; the HIP
    statistics against fp64 statistics of the HIP output itself (out.double()), which separates the statistics arithmetic from the convolution error."""
    lib = E.load_library()
    B, Cin, H, W = 2, 64, HW, HW
    x = rnd(20 + N, (B, Cin, H, W))
    w = rnd(21, (N, Cin, 3, 3)) / (9 * Cin) ** 0.5
    # the offsets of A through the bias (per channel, so both images share them), scaled to 0.92 of the output's spread (~1, ~1.41 with the N(0, 1) residual):
    # sample spreads vary by a few %, and the ratios stay <= 100
    bias = dc_offsets(1, N, torch.tensor([0.92 * (2 ** 0.5 if res else 1.0)]))[0].float()
    r = rnd(22, (B, N, H, W)) if res else None
    _set_pp(lib, pp)
    try:
        wp, wsc = _w_planes(lib, w, pf, dev)
        out, stats, done = _conv_ex(lib, _x_planes(lib, x, pf, dev), wp, 9 * Cin * N, wsc, bias.to(dev), _rows(r.to(dev)) if res else None, B, H, W, N, Cin, 9, pf, dev)
    finally:
        _set_pp(lib, None)
    assert done == 1
    o64 = _unrows(out.cpu(), B, H, W).double()
    err = normalised_err(o64, stats)
    print(f"fused stats pf={pf} pp={pp} res={res} N={N} HW={HW}^2: {err:.2e} (|mean|/std up to {ratios_reached(o64):.0f})")
    assert err <= BAR, err


@pytest.mark.parametrize("pf,pp", VARIANTS)
def test_conv_fused_gn_stats_not_where_it_cannot_run(dev, pf, pp):
    """gn_done == 0 where the fused statistics must not run: H W not a multiple of 256, or a split K (the slabs are reduced by another kernel)."""
    lib = E.load_library()
    Cin, N = 64, 160
    _set_pp(lib, pp)
    try:
        wp, wsc = _w_planes(lib, rnd(23, (N, Cin, 3, 3)) / 24.0, pf, dev)
        b = torch.zeros(N, device=dev)
        for B, H, W, split in ((2, 12, 12, 0), (1, 16, 20, 0), (2, 16, 16, 2)):
            ws = torch.empty(max(split, 1) * B * H * W * N, device=dev)
            x = rnd(24, (B, Cin, H, W))
            out, _, done = _conv_ex(lib, _x_planes(lib, x, pf, dev), wp, 9 * Cin * N, wsc, b, None, B, H, W, N, Cin, 9, pf, dev, split=split, ws=ws)
            assert done == 0, (B, H, W, split)
            want = F.conv2d(x.double(), (rnd(23, (N, Cin, 3, 3)) / 24.0).double(), padding=1)
            assert _rel_err(_unrows(out.cpu(), B, H, W).double(), want) <= BAR
    finally:
        _set_pp(lib, None)


# ---------------------------------------------------------------------------------------------------- C. fused up-sampling convolution
_UP_REF = {}


def _up_case(Cin, N, B, H, W):
    key = (Cin, N, B, H, W)
    if key not in _UP_REF:
        x = rnd(30 + Cin + H, (B, Cin, H, W))
        w = rnd(31 + N, (N, Cin, 3, 3)) / (9 * Cin) ** 0.5
        bias = dc_offsets(1, N, torch.tensor([0.92]))[0].float() if N % 32 == 0 else rnd(32, (N,), 0.1)          # the offsets of A (as in B)
        want = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), w.double(), bias.double(), padding=1)
        _UP_REF[key] = (x, w, bias, want)
    return _UP_REF[key]


UP_SHAPES = [(640, 640, B, 16, 16) for B in (1, 2)] + [(320, 320, B, 32, 32) for B in (1, 2)] + [(320, 320, B, 64, 64) for B in (1, 2)] + \
            [(160, 160, B, 128, 128) for B in (1, 2)] + [(96, 96, 3, 6, 7), (64, 90, 1, 8, 8)]


@pytest.mark.parametrize("pf,pp", VARIANTS)
@pytest.mark.parametrize("Cin,N,B,H,W", UP_SHAPES)
def test_upsample_conv_fused_phases(dev, pf, pp, Cin, N, B, H, W):
    """taps = 4, up_phase = 0 (the four 2x2 phase convolutions of Upsample2x in one launch, with the decoder's phase weight layout) against fp64
    conv2d(interpolate(x, 2, nearest)); the decoder's shapes, a ragged one (M not a multiple of 256, N not of 160) and N % 4 != 0 (the pp = 1 fallback of the
    16-byte epilogue).  Where the statistics fuse, the four phases' statistics against fp64 statistics of the HIP output."""
    lib = E.load_library()
    x, w, bias, want = _up_case(Cin, N, B, H, W)
    npl = NPL[pf]
    _set_pp(lib, pp)
    try:
        wp, wps, wsc = _upconv_planes(lib, w, pf, dev)
        out, stats, done = _conv_ex(lib, _x_planes(lib, x, pf, dev), wp, wps, wsc, bias.to(dev), None, B, H, W, N, Cin, 4, pf, dev, up=0, w_phase_stride=npl * wps)
    finally:
        _set_pp(lib, None)
    got = _unrows(out.cpu(), B, 2 * H, 2 * W).double()
    assert torch.isfinite(got).all()
    err = _rel_err(got, want)
    fuse = N % 32 == 0 and 160 % (N // 32) == 0 and (H * W) % 256 == 0
    assert done == (1 if fuse else 0)
    serr = normalised_err(got, stats) if done else 0.0
    print(f"upconv pf={pf} pp={pp} Cin={Cin} N={N} B={B} H={H} W={W}: out {err:.2e}, fused stats {serr:.2e}")
    assert err <= BAR, err
    assert serr <= BAR, serr


@pytest.mark.parametrize("pf,pp", VARIANTS)
@pytest.mark.parametrize("Cin,N,B,H,W", [UP_SHAPES[0], UP_SHAPES[3], UP_SHAPES[8]])
def test_upsample_conv_up9_form(dev, pf, pp, Cin, N, B, H, W):
    """The decoder's other Upsample2x form (too few tiles for the phase launch): prep with up = 1, then the 3x3 convolution over the up-sampled planes with
    the decoder's split-K workspace - same input, same bar."""
    lib = E.load_library()
    x, w, bias, want = _up_case(Cin, N, B, H, W)
    Ho, Wo = 2 * H, 2 * W
    G = _guard(Wo); R = B * (Ho + 2) * (Wo + 2) + 2 * G
    xp = torch.full((pf, Cin // 32, R, 32), 0x7FC0 if pf == 3 else 0x7E00, dtype=torch.int16, device=dev)
    xr = _rows(x.to(dev))
    E._check(lib.sdvar_op_vae_prep(_p(xr), None, None, None, _p(xp), (Cin // 32) * R * 32, pf, B, Cin, H, W, 1, 0, G, _st()))
    ws = torch.empty(64 << 20, device=dev)
    _set_pp(lib, pp)
    try:
        wp, wsc = _w_planes(lib, w, pf, dev)
        out, stats, done = _conv_ex(lib, (xp, (Cin // 32) * R * 32, R, G), wp, 9 * Cin * N, wsc, bias.to(dev), None, B, Ho, Wo, N, Cin, 9, pf, dev, ws=ws)
    finally:
        _set_pp(lib, None)
    got = _unrows(out.cpu(), B, Ho, Wo).double()
    err = _rel_err(got, want)
    serr = normalised_err(got, stats) if done else 0.0
    print(f"up9 pf={pf} pp={pp} Cin={Cin} N={N} B={B} H={H}: out {err:.2e}, fused stats ({done}) {serr:.2e}")
    assert err <= BAR, err
    assert serr <= BAR, serr


# ---------------------------------------------------------------------------------------------------- D. decoder attention
def _attn_input(B, C, N, seed):
    """qkv rows (B N, 3C): q, k ~ N(0, 5.5) so that q.k / sqrt(C) ~ N(0, 5.5^2) spans about +-30 (5.5 standard deviations: the extremes of 2 N^2 scores); in every
    5th query of each image q is one shared vector u and the last key is u scaled so that those rows' largest score (30, or 1 above their largest other score)
    sits on the last key."""
    q = rnd(seed, (B, N, C), 5.5 ** 0.5).double()
    k = rnd(seed + 1, (B, N, C), 5.5 ** 0.5).double()
    v = rnd(seed + 2, (B, N, C)).double()
    for b in range(B):
        u = q[b, 0].clone()
        rows = torch.arange(0, N, 5)
        q[b, rows] = u
        s_other = (k[b, :-1] @ u).max().item() / C ** 0.5
        t = max(30.0, s_other + 1.0)
        k[b, -1] = u * (t * C ** 0.5 / (u @ u))
    qkv = torch.cat([q, k, v], -1).float()
    qd, kd, vd = qkv.double().split(C, -1)
    s = qd @ kd.transpose(1, 2) / C ** 0.5
    assert (s[:, ::5].argmax(-1) == N - 1).all()
    want = torch.softmax(s, -1) @ vd
    return qkv.reshape(B * N, 3 * C).contiguous(), want.reshape(B * N, C), s.abs().max().item()


_ATTN_CASES = [(1, N, C, 2) for N in (256, 1024) for C in (64, 128, 640)] + \
              [(0, N, C, 2) for N in (256, 1024) for C in (64, 128, 640, 160)] + [(0, 169, 64, 2), (0, 169, 160, 2)] + \
              [(2, 4096, 128, 3), (2, 169, 64, 2)]


@pytest.mark.parametrize("kernel,N,C,B", _ATTN_CASES)
def test_vae_attention_kernels(dev, kernel, N, C, B):
    """sdvar_op_vae_attn with each kernel forced: 1 = matrix cores (N in {256, 1024}), 0 = fp32 FMA with the probabilities in LDS (C % 64 != 0 and a ragged last
    group of 16 queries included), 2 = probabilities in global scratch, with a workspace for one image so that B = 3 takes three launches.  kernel = -1 (the
    decoder's choice) equals the forced kernel the decoder picks, bit for bit."""
    lib = E.load_library()
    qkv, want, smax = _attn_input(B, C, N, 40 + N + C)
    qd = qkv.to(dev)
    per_img = (N + 15) // 16 * N * 20
    ws = torch.empty(per_img + 7, device=dev) if kernel == 2 else None
    out = torch.full((B * N, C), float("nan"), device=dev)
    E._check(lib.sdvar_op_vae_attn(_p(qd), _p(out), B, C, N, _p(ws), ws.numel() if ws is not None else 0, kernel, _st()))
    torch.cuda.synchronize()
    err = _rel_err(out.cpu().double(), want)
    print(f"vae attention kernel={kernel} N={N} C={C} B={B}: {err:.2e} (|score| up to {smax:.0f})")
    assert err <= BAR, err
    auto = 1 if (N in (256, 1024) and C % 64 == 0) else (0 if (32 * 256 + 32 * 16) * 4 + N * 20 * 4 <= 160 * 1024 else 2)
    if auto == kernel:
        out2 = torch.full_like(out, float("nan"))
        E._check(lib.sdvar_op_vae_attn(_p(qd), _p(out2), B, C, N, _p(ws), ws.numel() if ws is not None else 0, -1, _st()))
        torch.cuda.synchronize()
        assert torch.equal(out, out2)


def test_vae_attention_refuses_forced_kernels_that_cannot_take_the_shape(dev):
    lib = E.load_library()
    qkv = torch.zeros(4096 * 3 * 160, device=dev)
    out = torch.zeros(4096 * 160, device=dev)
    ws = torch.zeros(16, device=dev)
    for kernel, N, C in ((1, 169, 64), (1, 256, 160), (1, 512, 64), (0, 4096, 64), (2, 256, 64), (3, 256, 64)):
        assert lib.sdvar_op_vae_attn(_p(qkv), _p(out), 1, C, N, _p(ws), ws.numel(), kernel, _st()) == 1, (kernel, N, C)


# ---------------------------------------------------------------------------------------------------- E. conv_out
@pytest.mark.parametrize("C", [32, 128, 160])
def test_vae_conv_out(dev, C):
    """sdvar_op_vae_conv_out (convout_weight_kernel, convout_partial_kernel, convout_gather_kernel): GroupNorm with gamma ~ 1 + N(0, 0.3) (a few negative), beta
    ~ N(0, 0.5), SiLU, the 3-channel 3x3 conv with bias ~ N(0, 0.1), clamp; B H W = 1200 rows (not a multiple of the 256-row block).  Statistics in fp64 cast
    to float isolate conv_out.  Condition: at most 5 % of the fp64 reference's pixels saturate (|ref| >= 1), or the clamp would hide the error under them."""
    lib = E.load_library()
    B, H, W = 3, 20, 20
    std = torch.tensor([1.0, 0.5, 2.0], dtype=torch.float64)
    x = (rnd(50 + C, (B, C, H, W)).double() * std[:, None, None, None] + dc_offsets(B, C, std)[..., None, None]).float()
    gamma = 1 + rnd(51, (C,), 0.3)
    gamma[::11] = -gamma[::11].abs()
    beta, bias = rnd(52, (C,), 0.5), rnd(53, (3,), 0.1)
    w = rnd(54, (3, C, 3, 3)) * (0.5 / (9 * C) ** 0.5)
    m64, r64 = group_stats64(x.double())
    stats = torch.stack([m64, r64], -1).float().contiguous()
    ref = F.conv2d(F.silu(F.group_norm(x.double(), 32, gamma.double(), beta.double(), eps=1e-6)), w.double(), bias.double(), padding=1)
    sat = (ref.abs() >= 1).double().mean().item()
    assert sat <= 0.05, sat
    img = torch.full((B, 3, H, W), float("nan"), device=dev)
    ws = torch.empty((C + B * H * W) * 28, device=dev)
    args = [_rows(x.to(dev)), stats.to(dev), gamma.to(dev), beta.to(dev), w.to(dev), bias.to(dev)]
    E._check(lib.sdvar_op_vae_conv_out(*[_p(t) for t in args], _p(img), B, C, H, W, _p(ws), _st()))
    torch.cuda.synchronize()
    want = ref.clamp(-1, 1)
    err = _rel_err(img.cpu().double(), want)
    print(f"conv_out C={C}: {err:.2e} (saturated {100 * sat:.1f} %)")
    assert err <= BAR, err


# ---------------------------------------------------------------------------------------------------- F. the whole decoder under a checkpoint-like init
_F_REF = {}


def _f_case():
    """tests/vae_ckpt_init.py: ch = 160 (the reference checkpoint's geometry), latent 16, B = 2; the fp64 reference once per session."""
    if not _F_REF:
        from vae_ckpt_init import checkpoint_like_state_dict, reference_fp64
        f_hat = rnd(12, (2, 32, 16, 16), 1.5)
        sd = checkpoint_like_state_dict(f_hat)
        t0 = time.time()
        y, ratios = reference_fp64(sd, f_hat)
        _F_REF.update(sd=sd, f_hat=f_hat, y=y, ratios=ratios, secs=time.time() - t0)
    return _F_REF


@pytest.mark.parametrize("cm", ["bf16x3", "f16x2"])
def test_decoder_checkpoint_like_init_vs_fp64(dev, cm):
    """The whole HIP decode (engine.VaeCtx) against the fp64 CPU decode of the same weights: GroupNorm affines and conv biases far from the stress init's identity
    / constant, residual-stream groups at |mean| / std 10..30.  Condition (from the reference alone): at most 5 % of its pixels saturate (|ref| >= 1)."""
    c = _f_case()
    y = c["y"]
    sat = (y.abs() >= 1).double().mean().item()
    print(f"fp64 reference: {c['secs']:.1f} s; saturated {100 * sat:.2f} %; |mean|/std at the GroupNorms: " + " ".join(f"{r:.1f}" for r in c["ratios"]))
    assert sat <= 0.05, sat
    ctx = E.VaeCtx(c["sd"], 2, dev, latent_hw=16, conv_mode=cm)
    got = ctx.decode(c["f_hat"].to(dev)).cpu().double()
    err = (got - y.clamp(-1, 1)).abs().max().item()
    print(f"decoder {cm}: max|err| {err:.2e}")
    assert err <= 1e-4, err
