"""CPU emulation of the decoder's stand-alone GroupNorm statistics pass (csrc/vae.hip gn_partial_kernel + gn_finalize_kernel), in the kernel's own summation order:
fp32 running sums per (pixel lane, channel quad) thread over the pixels p = lane, lane + npl, ... of a chunk of rows, fp64 sums of those per (chunk, channel), fp64
merges of the channels of a group and of the chunks.  It pins the arithmetic the kernel uses without a GPU: the one-pass form E[x^2] - E[x]^2 loses the variance of a group whose mean is large next to its
spread, the shifted sums around a pivot per channel (the chunk's first value of the channel) with Chan merges of channels and chunks do not.

Bar: 2e-5 on the normalised value (x - mean) rstd against fp64, with mean and rstd cast to float as the kernel stores them: the bar of every single-kernel comparison
of the decoder (tests/test_gpu_vae_kernels.py).  |mean| / std stays <= 100: the float storage of the mean alone costs half an ulp of |mean|, 3.8e-6 std at 100, and
more than the bar from about 256 on (a limit of the stored format, not of the summation)."""
import numpy as np
import pytest

from conftest import rnd

BAR = 2e-5


def _chunking(C, H):
    nch = min(H, 64)
    rpc = (H + nch - 1) // nch
    return rpc, (H + rpc - 1) // rpc, 320 // (C // 4)


def emulate_stats(x, shifted):
    """x (H, W, C) float32 of one image -> (mean, rstd) float32 (32,) as gn_partial_kernel + gn_finalize_kernel compute them; shifted = False: the one-pass
    form of the parent kernels (fp32 sums of x and x^2, var = E[x^2] - E[x]^2 in fp64)."""
    H, W, C = x.shape
    cpg = C // 32
    rpc, chunks, npl = _chunking(C, H)
    assert H % rpc == 0 and (rpc * W) % npl == 0, "emulated shapes have whole chunks and whole pixel-lane rounds"
    npix = rpc * W
    xc = x.reshape(chunks, npix // npl, npl, C)                       # [chunk][step][pixel lane][channel]: thread (lane, quad) runs over the steps
    K = xc[:, 0, 0, :] if shifted else np.zeros((chunks, C), np.float32)          # pivot of channel c: the chunk's first pixel
    s = np.zeros((chunks, npl, C), np.float32)
    ss = np.zeros((chunks, npl, C), np.float32)
    for k in range(npix // npl):
        d = xc[:, k] - K[:, None, :]
        s = s + d
        ss = ss + d * d
    s1 = s.astype(np.float64).sum(1)                                  # per (chunk, channel), fp64 over the pixel lanes
    s2 = ss.astype(np.float64).sum(1)
    n = float(npix)
    count = n * cpg * chunks
    if not shifted:
        a = s1.reshape(chunks, 32, cpg).sum(-1).sum(0)
        mean = a / count
        var = np.maximum(s2.reshape(chunks, 32, cpg).sum(-1).sum(0) / count - mean * mean, 0.0)
    else:                                                             # per channel sum x, M2_c; per (chunk, group) {sum, M2}; chunks merged (Chan, one pass)
        sc = n * K.astype(np.float64) + s1
        m = (s2 + (sc * sc - s1 * s1) * (1.0 / n)).reshape(chunks, 32, cpg).sum(-1)
        tot = sc.reshape(chunks, 32, cpg).sum(-1)
        m2 = m - tot * tot / (n * cpg)
        a = tot.sum(0)
        mean = a / count
        var = np.maximum(((m2 + tot * tot / (n * cpg)).sum(0) - a * mean) / count, 0.0)
    return mean.astype(np.float32), (1.0 / np.sqrt(var + 1e-6)).astype(np.float32)


def normalised_error(x, mean, rstd):
    H, W, C = x.shape
    xg = x.astype(np.float64).reshape(H * W, 32, C // 32)
    m64 = xg.mean(axis=(0, 2))
    r64 = 1.0 / np.sqrt(xg.var(axis=(0, 2)) + 1e-6)
    want = (xg - m64[None, :, None]) * r64[None, :, None]
    got = (xg - mean.astype(np.float64)[None, :, None]) * rstd.astype(np.float64)[None, :, None]
    return float(np.abs(got - want).max())


def dc_input(seed, C, H, ratio):
    """N(0, 1) + a DC offset of +-ratio per group (signs alternate over the 32 groups), channel-last (H, W = H, C) float32."""
    x = rnd(seed, (H, H, C)).numpy()
    sign = np.where(np.arange(32) % 2 == 0, 1.0, -1.0)
    dc = np.repeat(sign * ratio, C // 32).astype(np.float32)
    return (x + dc[None, None, :]).astype(np.float32)


SHAPES = [(640, 16), (320, 64), (160, 256)]


@pytest.mark.parametrize("C,H", SHAPES)
@pytest.mark.parametrize("ratio", [0, 10, 30, 100])
def test_shifted_sums_hold_the_bar(C, H, ratio):
    x = dc_input(31 + C + H, C, H, ratio)
    err = normalised_error(x, *emulate_stats(x, shifted=True))
    print(f"shifted C={C} H={H} |mean|/std={ratio}: {err:.2e}")
    assert err <= BAR, err


@pytest.mark.parametrize("C,H", SHAPES)
def test_one_pass_form_fails_at_ratio_100(C, H):
    """The emulation sees the bug the shifted sums fix: the one-pass variance misses the bar at |mean|/std = 100 on every shape (and stays exact at 0)."""
    x = dc_input(31 + C + H, C, H, 100)
    err = normalised_error(x, *emulate_stats(x, shifted=False))
    print(f"one-pass C={C} H={H} |mean|/std=100: {err:.2e}")
    assert err > BAR, err
    x0 = dc_input(31 + C + H, C, H, 0)
    assert normalised_error(x0, *emulate_stats(x0, shifted=False)) <= BAR
