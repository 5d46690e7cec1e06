"""The tap-reuse K loop of the f16x2 decoder convolution (csrc/conv.hip conv_f16x2_reuse_kernel: X staged once per row of taps) against fp64 conv2d on the CPU,
at the smallest shapes at which it can still go wrong, and the same cases on the present loop with the switch off ("conv_tap_reuse" 0).

Bar: 2e-5 * max(1, |ref|) per element (the bar of test_gpu_vae_kernels.py), for the output and for the fused GroupNorm statistics (that file's test B: the
HIP statistics against fp64 statistics of the HIP output).  Which loop ran is asserted through sdvar_debug_get_conv_cfg."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from conftest import rnd
from sdvar_amd import engine as E

pytestmark = pytest.mark.gpu

BAR = 2e-5
PF = 2                   # f16x2 planes
NAN16 = 0x7E00           # an fp16 NaN


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _rows(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def _unrows(r, B, H, W):
    return r.view(B, H, W, -1).permute(0, 3, 1, 2)


def _rel_err(got, want):
    return float(((got - want).abs() / want.abs().clamp(min=1.0)).max())


def _x_planes(lib, x, dev, nan_tail=False):
    """(B, C, H, W) -> the decoder's f16x2 operand planes (sdvar_op_vae_prep mode 0) over a NaN-filled buffer; nan_tail: the guard rows behind the last image NaN again"""
    B, Cin, H, W = x.shape
    G = (W + 3 + 15) // 16 * 16
    Mp = B * (H + 2) * (W + 2); R = Mp + 2 * G
    xp = torch.full((PF, Cin // 32, R, 32), NAN16, dtype=torch.int16, device=dev)
    xr = _rows(x.to(dev))
    E._check(lib.sdvar_op_vae_prep(_p(xr), None, None, None, _p(xp), (Cin // 32) * R * 32, PF, B, Cin, H, W, 0, 0, G, _st()))
    torch.cuda.synchronize()
    if nan_tail:
        xp[:, :, G + Mp:, :] = NAN16
    return xp, (Cin // 32) * R * 32, R, G


def _w_planes(lib, w, dev):
    Cout, Cin, k, _ = w.shape
    taps = k * k
    wp = torch.zeros(PF, taps * Cin // 32, Cout, 32, dtype=torch.int16, device=dev)
    wsc = torch.zeros(4, device=dev)
    wd = w.to(dev).contiguous()
    E._check(lib.sdvar_op_conv_weight_planes(_p(wd), _p(wp), Cout, Cin, taps, taps * Cin * Cout, PF, _p(wsc), _st()))
    torch.cuda.synchronize()
    return wp, wsc


def _upconv_planes(lib, w, dev):
    """the four phase weight sets of Upsample2x as the decoder's binder builds them (one scale over all phases, each phase packed with taps = 4)"""
    Cout, Cin = w.shape[:2]
    wps = 4 * Cin * Cout
    weff = torch.zeros(4, Cout, Cin, 4, device=dev)
    wd = w.to(dev).contiguous()
    E._check(lib.sdvar_op_upconv_weights(_p(wd), _p(weff), Cout, Cin, _st()))
    wp = torch.zeros(4, PF, wps, dtype=torch.int16, device=dev)
    wsc = torch.zeros(4, device=dev)
    tmp = torch.zeros(2, 16 * Cout * Cin, dtype=torch.int16, device=dev)
    E._check(lib.sdvar_op_split_planes_f16(_p(weff), _p(tmp), 16 * Cout, Cin, 16 * Cout * Cin, _p(wsc), _st()))
    weff = weff * wsc[0]
    for ph in range(4):
        E._check(lib.sdvar_op_conv_weight_planes(_p(weff[ph]), _p(wp[ph]), Cout, Cin, 4, wps, PF, None, _st()))
    torch.cuda.synchronize()
    return wp, wps, wsc


def _conv(lib, xpl, wp, wps, wsc, bias, res, B, H, W, N, Cin, taps, dev, up=-1, w_phase_stride=0):
    """sdvar_op_conv_planes_ex into a NaN-filled output -> (output rows, GroupNorm statistics, gn_done, 1 if the tap-reuse loop ran)"""
    xp, xps, R, G = xpl
    Ho, Wo = (2 * H, 2 * W) if up >= 0 else (H, W)
    out = torch.full((B * Ho * Wo, N), float("nan"), device=dev)
    part = torch.zeros(B * ((H * W) // 256 + 1) * 64 * (4 if up >= 0 else 1), dtype=torch.float64, device=dev)
    stats = torch.zeros(B, 32, 2, device=dev)
    done = C.c_int32(-1)
    E._check(lib.sdvar_op_conv_planes_ex(_p(xp), xps, R, G, _p(wp), wps, PF, _p(wsc), _p(bias), _p(res), _p(out), B, H, W, N, Cin, taps, None, 0, 0, up, w_phase_stride,
                                         _p(part), _p(stats), C.byref(done), _st()))
    torch.cuda.synchronize()
    took = C.c_int32(-1)
    E._check(lib.sdvar_debug_get_conv_cfg(C.byref(took)))
    return out, stats, done.value, took.value


def _stats_err(x64, stats):
    """max |(x - m) r - (x - m64) r64| / max(1, |(x - m64) r64|) with the HIP {mean, rstd} against fp64 group statistics of x64 (eps 1e-6)"""
    B = x64.shape[0]
    xg = x64.reshape(B, 32, -1)
    m64, r64 = xg.mean(-1), 1.0 / torch.sqrt(xg.var(-1, unbiased=False) + 1e-6)
    st = stats.double().cpu()
    return _rel_err((xg - st[..., 0:1]) * st[..., 1:2], (xg - m64[..., None]) * r64[..., None])


# (B, H, W, Cin, Cout, residual, fused up-sampling, eligible)
CASES = [
    (1, 4, 64, 32, 32, False, False, True),          # one tile of four image rows: frame columns inside the staged span
    (2, 2, 128, 64, 160, False, False, True),        # one tile per image, image boundary between tiles, two channel blocks; fused GroupNorm statistics
    (2, 1, 256, 32, 200, False, False, True),        # H = 1: both dy neighbours are frame rows; two N tiles, the second with a tail
    (1, 1, 512, 32, 48, False, False, True),         # two tiles per image row: the halo columns are the neighbour tile's pixels
    (1, 2, 128, 96, 160, True, False, True),         # residual; three channel blocks (both rings wrap)
    (1, 2, 128, 64, 160, False, True, True),         # fused up-sampling: taps = 4, four phases
    (1, 3, 100, 32, 32, False, False, False),        # ineligible: the present loop
]
_REF = {}


def _case(case):
    """inputs and the fp64 reference of a case, computed once"""
    if case not in _REF:
        B, H, W, Cin, N, res, up, _ = case
        seed = 700 + 7 * W + Cin + N
        x = rnd(seed, (B, Cin, H, W))
        w = rnd(seed + 1, (N, Cin, 3, 3)) / (9 * Cin) ** 0.5
        bias = rnd(seed + 2, (N,), 0.5)
        r = rnd(seed + 3, (B, N, H, W)) if res else None
        xin = F.interpolate(x.double(), scale_factor=2, mode="nearest") if up else x.double()
        want = F.conv2d(xin, w.double(), bias.double(), padding=1)
        if res:
            want = want + r.double()
        _REF[case] = (x, w, bias, r, want)
    return _REF[case]


def _run_case(lib, case, dev, nan_tail=False):
    B, H, W, Cin, N, res, up, _ = case
    x, w, bias, r, want = _case(case)
    xpl = _x_planes(lib, x, dev, nan_tail)
    rd = _rows(r.to(dev)) if res else None
    if up:
        wp, wps, wsc = _upconv_planes(lib, w, dev)
        out, stats, done, took = _conv(lib, xpl, wp, wps, wsc, bias.to(dev), None, B, H, W, N, Cin, 4, dev, up=0, w_phase_stride=PF * wps)
        got = _unrows(out.cpu(), B, 2 * H, 2 * W).double()
    else:
        wp, wsc = _w_planes(lib, w, dev)
        out, stats, done, took = _conv(lib, xpl, wp, 9 * Cin * N, wsc, bias.to(dev), rd, B, H, W, N, Cin, 9, dev)
        got = _unrows(out.cpu(), B, H, W).double()
    return got, want, stats, done, took


@pytest.mark.parametrize("reuse", [1, 0])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d_%dx%d_%d-%d%s%s" % (c[0], c[1], c[2], c[3], c[4], "_res" if c[5] else "", "_up" if c[6] else ""))
def test_conv_tap_reuse_vs_fp64(dev, case, reuse):
    """Every case on the tap-reuse loop (asserted through sdvar_debug_get_conv_cfg; the ineligible shape must report the present loop) and, with the switch at 0,
    on the present loop.  Where the statistics fuse (N = 160, H W % 256 == 0) the fused GroupNorm statistics are checked against fp64 statistics of the output."""
    lib = E.load_library()
    E._check(lib.sdvar_debug_set_variant(b"conv_tap_reuse", reuse))
    try:
        got, want, stats, done, took = _run_case(lib, case, dev)
    finally:
        E._check(lib.sdvar_debug_set_variant(b"conv_tap_reuse", -1))
    B, H, W, Cin, N = case[:5]
    assert took == (1 if (reuse and case[7]) else 0), took
    assert torch.isfinite(got).all()
    err = _rel_err(got, want)
    fuse = N % 32 == 0 and 160 % (N // 32) == 0 and (H * W) % 256 == 0
    assert done == (1 if fuse else 0)
    serr = _stats_err(got, stats) if done else 0.0
    print(f"tap reuse={reuse} took={took} B={B} {H}x{W} {Cin}->{N} res={case[5]} up={case[6]}: out {err:.2e}, fused stats ({done}) {serr:.2e}")
    assert err <= BAR, err
    assert serr <= BAR, serr


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[5]], ids=["rows", "split_row", "up"])
def test_conv_tap_reuse_reads_no_guard_rows(dev, case):
    """The guard rows behind the last image hold NaN: the rows of the 272-row stage behind the staged span must not bring them into a real pixel (they are clamped
    into the span), so the output stays finite and inside the bar."""
    lib = E.load_library()
    got, want, _, _, took = _run_case(lib, case, dev, nan_tail=True)
    assert took == 1
    assert torch.isfinite(got).all()
    assert _rel_err(got, want) <= BAR
