"""The image -> token half of the VQVAE against fp64 on the CPU, on inputs where kernels go wrong (csrc/quant.hip, csrc/vae.hip, csrc/api.hip):

  A  sdvar_op_quant_nearest where |z|^2 + |e|^2 - 2 z.e cancels (|z|^2 is 10^3 .. 10^4 times the distances at stake), ragged N and V, duplicates, edge rows;
  B  the raw-stream operand producers (s2d planes -> Downsample2x convolution, image planes) under group means far from 0, and their planes read back;
  C  the whole encoder under a checkpoint-like init (tests/vae_ckpt_init.py) against the fp64 encoder, the bar set by the float restatement's own error;
  D  the ten-scale residual quantisation per scale (tests/quant_chain_check.py: bounds derived there) in every Phi layout, staged and unstaged;
  E  the public path (img_to_idxBl, img_to_reconstructed_img) and the codebook-dependent state across load_state_dict / refresh_hip / a second bind.

Bars come from the project and from derivations, not from these measurements: 2e-5 max(1, |ref|) for a single kernel, the f16x2 planes' 2^-22 relative /
2^-25 absolute representation floor on an operand (as tests/test_gpu_vae_kernels.py), quant_chain_check's rounding bounds for the ids."""
import ctypes as C
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rnd
from quant_chain_check import check_chain, checkpoint_like_f, nearest_report, quant_model, three_decade_codebook
from sdvar_amd import engine as E
from sdvar_amd.ladder import LADDER_256, LADDER_512, LADDER_1024

pytestmark = pytest.mark.gpu

BAR = 2e-5
F16_REL, F16_ABS = 2.0 ** -22, 2.0 ** -25
MODES = ["f16x2", "bf16x3"]
PF = {"f16x2": 2, "bf16x3": 3}


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


def _guard(W):
    return (W + 3 + 15) // 16 * 16


def _unplanes(xp, pf):
    """(npl, ...) int16 planes -> the value they hold, in double (on the planes' device)"""
    if pf == 3:
        return sum((xp[k].to(torch.int32) << 16).view(torch.float32).double() for k in range(3))
    return sum(xp[k].view(torch.float16).double() for k in range(2))


# ---------------------------------------------------------------------------------------------------- A. nearest code where the formula cancels
def _nearest_case(N, V, offset, seed):
    """Codebook: one centre c (|c_i| = offset, random signs) plus 0.05 N(0, 1) per code.  Even rows are planted next to a code (E[j] + 0.005 N(0, 1)), odd rows
    are free draws from the codes' own distribution.  Duplicate codes where V allows: (3, 4) in neighbouring lanes, (7, 71) in two waves, (10, 266) in one thread's
    two rounds, (1, V - 1); the first planted rows sit next to the duplicates' higher index.  From N = 9: the last row is all zero, the one before equals a code.
    -> z, codebook (float), planted (N,) bool"""
    g = np.random.Generator(np.random.Philox(key=[seed, 99]))
    c = offset * np.where(g.random(32) < 0.5, -1.0, 1.0)
    cb = (c + 0.05 * g.standard_normal((V, 32))).astype(np.float32)
    dups = [(lo, hi) for lo, hi in ((3, 4), (7, 71), (10, 266), (1, V - 1)) if lo < hi < V]
    for lo, hi in dups:
        cb[hi] = cb[lo]
    z = (c + 0.05 * g.standard_normal((N, 32))).astype(np.float32)
    planted = np.zeros(N, dtype=bool)
    planted[::2] = True
    j = g.integers(0, V, size=N)
    for i, (_, hi) in enumerate(dups):
        if 2 * i < N:
            j[2 * i] = hi
    z[planted] = cb[j[planted]] + (0.005 * g.standard_normal((int(planted.sum()), 32))).astype(np.float32)
    if N >= 9:
        z[N - 1] = 0.0
        z[N - 2] = cb[j[N - 2]]
        planted[N - 2:] = True                                    # the edge rows take the exact check where decidable, like the planted ones
    return torch.from_numpy(z), torch.from_numpy(cb), torch.from_numpy(planted)


@pytest.mark.parametrize("offset", [2, 8])
@pytest.mark.parametrize("V", [1, 64, 257, 1000, 4096])
@pytest.mark.parametrize("N", [1, 7, 9, 4099])
def test_nearest_code_cancellation_regime(dev, N, V, offset):
    """Rule (a) of quant_chain_check (near-optimal within the rounding bound of the float formula) on every row; rule (b) (the fp64 argmin, lowest index of
    identical codes) on the decidable planted and edge rows.  N = 7, 9, 4099 leave a ragged last group of QN_ROWS = 8 rows, V = 1, 257, 1000 a ragged stride of
    the 256 threads.  Condition (from the fp64 reference alone): at least 95 % of the planted rows are decidable.  Free rows take (a) only: there the float
    reference formula itself leaves the fp64 argmin on 0.15 % (offset 2) to 3.9 % (offset 8) of the rows."""
    lib = E.load_library()
    z, cb, planted = _nearest_case(N, V, offset, 1000 * offset + N + V)
    zd, cd = z.to(dev), cb.to(dev)
    ids = torch.full((N,), -7, dtype=torch.int64, device=dev)
    e2 = torch.empty(V, device=dev)
    E._check(lib.sdvar_op_quant_nearest(_p(zd), N, _p(cd), V, 32, _p(e2), _p(ids), _st()))
    torch.cuda.synchronize()
    k = ids.cpu()
    assert k.min().item() >= 0 and k.max().item() < V, (k.min().item(), k.max().item())
    nr = nearest_report(z.double(), cb.double(), k)
    dec = nr["decidable"] & planted
    share = dec.sum().item() / planted.sum().item()
    worst = nr["excess_over_bound"].max().item()
    wrong = int((dec & (k != nr["want"])).sum())
    free_off = ((k != nr["want"]) & ~planted).double().sum().item() / max(1, int((~planted).sum()))
    print(f"nearest N={N} V={V} offset={offset}: |z|^2/best median {nr['z2_over_best'].median().item():.3g}; planted rows decidable {100 * share:.1f} %; worst excess/bound "
          f"{worst:.3g}; decidable planted rows off the fp64 argmin {wrong}; free rows off the fp64 argmin {100 * free_off:.2f} %")
    assert share >= 0.95, share
    assert worst <= 1.0, worst
    assert wrong == 0, wrong


# ---------------------------------------------------------------------------------------------------- B. raw-stream producers
def _stream_input(B, C_, H, seed):
    """(B, C, H, H) float: N(0, 1) plus a per-group offset of 0, 10 or 30 spreads (cycling over the groups, shifted per image), the sign alternating every 3 groups"""
    x = rnd(seed, (B, C_, H, H))
    cpg = C_ // 32
    for b in range(B):
        for gI in range(32):
            r = (0.0, 10.0, 30.0)[(gI + b) % 3]
            x[b, gI * cpg:(gI + 1) * cpg] += r * (-1.0 if (gI // 3 + b) % 2 else 1.0)
    return x


_B_REF = {}


def _s2d_case(C_, H, B):
    key = (C_, H, B)
    if key not in _B_REF:
        x = _stream_input(B, C_, H, 300 + C_ + H)
        w = rnd(301 + C_, (C_, C_, 3, 3), (C_ * 9) ** -0.5)
        b = rnd(302, (C_,), 0.1)
        xp = F.pad(x.double(), (0, 1, 0, 1))
        ref = torch.cat([F.conv2d(xp[i:i + 1], w.double(), b.double(), stride=2) for i in range(B)])
        # what the f16x2 planes cannot hold of x, through the convolution: sum |w| (2^-22 |x| + 2^-25)
        floor = torch.cat([F.conv2d(F16_REL * xp[i:i + 1].abs() + F16_ABS, w.double().abs(), stride=2) for i in range(B)])
        _B_REF.clear()                                            # one geometry at a time (the parametrisation keeps a geometry's variants together)
        _B_REF[key] = (x, w, b, ref, floor)
    return _B_REF[key]


@pytest.mark.parametrize("mode", MODES)                         # the decorator nearest the function varies slowest: a geometry's four variants run together
@pytest.mark.parametrize("split", [0, 4])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C_,H", [(160, 256), (160, 128), (320, 64), (320, 32)])
def test_s2d_downsample_conv_raw_stream(dev, mode, split, B, C_, H):
    """sdvar_op_vae_s2d_planes + sdvar_op_vae_s2d_weights + the 3x3 convolution over the space-to-depth planes (one pass and split-K 4) against fp64
    conv2d(pad(x, (0, 1, 0, 1)), stride 2) at the encoder's four Downsample2x geometries, the input a raw residual stream: channel groups at |mean| / std 0, 10
    and 30 with mixed signs.  Bar: 2e-5 max(1, max|ref|), plus for f16x2 what its planes cannot represent of the operand, propagated through |w|."""
    lib = E.load_library()
    x, w, b, ref, floor = _s2d_case(C_, H, B)
    pf = PF[mode]
    Ho = H // 2
    G = _guard(Ho)
    rows = B * (Ho + 2) * (Ho + 2) + 2 * G
    ops = rows * 4 * C_
    planes = torch.full((pf * ops,), 0x7E00 if pf == 2 else 0x7FC0, dtype=torch.int16, device=dev)          # NaN until the producer writes
    xr = x.to(dev).permute(0, 2, 3, 1).contiguous()
    wd, bd = w.to(dev), b.to(dev)
    E._check(lib.sdvar_op_vae_s2d_planes(_p(xr), _p(planes), ops, pf, B, C_, H, H, G, _st()))
    w4 = torch.empty(C_, 4 * C_, 3, 3, device=dev)
    E._check(lib.sdvar_op_vae_s2d_weights(_p(wd), _p(w4), C_, C_, _st()))
    wps = 9 * 4 * C_ * C_
    wp = torch.empty(pf * wps, dtype=torch.int16, device=dev)
    sc = torch.zeros(4, device=dev)
    E._check(lib.sdvar_op_conv_weight_planes(_p(w4), _p(wp), C_, 4 * C_, 9, wps, pf, _p(sc) if pf == 2 else None, _st()))
    M = B * Ho * Ho
    out = torch.full((M, C_), float("nan"), device=dev)
    ws = torch.empty(4 * M * C_, device=dev) if split else None
    E._check(lib.sdvar_op_conv_planes(_p(planes), ops, rows, G, _p(wp), wps, pf, _p(sc) if pf == 2 else None, _p(bd), None, _p(out), B, Ho, Ho, C_, 4 * C_, 9,
                                      _p(ws), ws.numel() if ws is not None else 0, split, _st()))
    torch.cuda.synchronize()
    got = out.view(B, Ho, Ho, C_).permute(0, 3, 1, 2).cpu().double()
    err = (got - ref).abs()
    bound = BAR * max(1.0, ref.abs().max().item()) + (floor if pf == 2 else 0.0)
    print(f"s2d conv {mode} split={split} B={B} C={C_} H={H}: max|err| {err.max().item():.2e} (max|ref| {ref.abs().max().item():.1f}, bar {BAR * max(1.0, ref.abs().max().item()):.2e}"
          + (f" + plane floor up to {floor.max().item():.1e})" if pf == 2 else ")"))
    assert torch.isfinite(got).all()
    assert ((err - bound).max().item()) <= 0, (err - bound).max().item()


def _u8_images(B, H, seed):
    """(B, 3, H, H) on the u8 grid v / 127.5 - 1, with exact -1 and +1 pixels (corners and a block included)"""
    g = np.random.Generator(np.random.Philox(key=[seed, 5]))
    u = g.integers(0, 256, size=(B, 3, H, H))
    u[:, :, 0, 0] = 0; u[:, :, -1, -1] = 255; u[:, :, 0, -1] = 255; u[:, :, -1, 0] = 0
    u[0, :, 8:16, 8:16] = 255; u[-1, :, 8:16, 8:16] = 0
    return torch.from_numpy(u.astype(np.float32)) / 127.5 - 1.0


def _check_reconstruction(got64, want64, pf, what):
    if pf == 3:
        assert torch.equal(got64, want64), f"{what}: bf16x3 planes do not reconstruct the input exactly"
    else:
        excess = ((got64 - want64).abs() - (F16_REL * want64.abs() + F16_ABS)).max().item()
        assert excess <= 0, f"{what}: f16x2 planes {excess:.3g} over their representation floor"


@pytest.mark.parametrize("mode", MODES)
def test_img_planes_read_back(dev, mode):
    """sdvar_op_vae_img_planes at 256^2, B = 3 on u8-grid images with exact +-1: the guard rows, the zero frame and the pad channels 3..31 are +0 bit for bit
    (every plane word 0), channels 0..2 reconstruct the image (exactly for bf16x3, to the plane floor for f16x2)."""
    lib = E.load_library()
    B, H, pf = 3, 256, PF[mode]
    img = _u8_images(B, H, 7).to(dev)
    assert (img == 1).any() and (img == -1).any()
    G = _guard(H)
    M = B * (H + 2) * (H + 2)
    R = M + 2 * G
    planes = torch.full((pf, R, 32), 0x7E00 if pf == 2 else 0x7FC0, dtype=torch.int16, device=dev)
    E._check(lib.sdvar_op_vae_img_planes(_p(img), _p(planes), R * 32, pf, B, H, H, G, _st()))
    torch.cuda.synchronize()
    assert (planes[:, :G] == 0).all() and (planes[:, G + M:] == 0).all(), "guard rows"
    body = planes[:, G:G + M].view(pf, B, H + 2, H + 2, 32)
    assert (body[..., 3:] == 0).all(), "pad channels 3..31"
    frame = torch.ones(H + 2, H + 2, dtype=torch.bool, device=dev)
    frame[1:-1, 1:-1] = False
    assert (body[:, :, frame] == 0).all(), "zero frame"
    got = _unplanes(body[:, :, 1:-1, 1:-1, :3], pf)
    _check_reconstruction(got, img.permute(0, 2, 3, 1).double(), pf, "img_planes")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C_,H,B", [(160, 64, 3), (24, 6, 2), (8, 2, 1)])
def test_s2d_planes_read_back(dev, mode, C_, H, B):
    """sdvar_op_vae_s2d_planes read back: plane channel (2 py + px) C + c of pixel (oy, ox) holds x[c][2 oy + py][2 ox + px] (exactly for bf16x3, to the plane
    floor for f16x2), guard rows and the zero frame are +0 bit for bit.  C = 24: a phase boundary inside a 32-channel plane chunk; (8, 2): the smallest shape."""
    lib = E.load_library()
    pf = PF[mode]
    x = _stream_input(B, 32, H, 400 + H)[:, :C_].contiguous() if C_ < 32 else _stream_input(B, C_, H, 400 + H)
    xr = x.to(dev).permute(0, 2, 3, 1).contiguous()
    Ho = H // 2
    G = _guard(Ho)
    M = B * (Ho + 2) * (Ho + 2)
    R = M + 2 * G
    nch = 4 * C_ // 32
    planes = torch.full((pf, nch, R, 32), 0x7E00 if pf == 2 else 0x7FC0, dtype=torch.int16, device=dev)
    E._check(lib.sdvar_op_vae_s2d_planes(_p(xr), _p(planes), nch * R * 32, pf, B, C_, H, H, G, _st()))
    torch.cuda.synchronize()
    assert (planes[:, :, :G] == 0).all() and (planes[:, :, G + M:] == 0).all(), "guard rows"
    body = planes[:, :, G:G + M].reshape(pf, nch, B, Ho + 2, Ho + 2, 32).permute(0, 2, 3, 4, 1, 5).reshape(pf, B, Ho + 2, Ho + 2, 4 * C_)
    frame = torch.ones(Ho + 2, Ho + 2, dtype=torch.bool, device=dev)
    frame[1:-1, 1:-1] = False
    assert (body[:, :, frame] == 0).all(), "zero frame"
    got = _unplanes(body[:, :, 1:-1, 1:-1], pf)                                                   # (B, Ho, Ho, 4 C)
    want = xr.double().view(B, Ho, 2, Ho, 2, C_).permute(0, 1, 3, 2, 4, 5).reshape(B, Ho, Ho, 4 * C_)
    _check_reconstruction(got, want, pf, "s2d_planes")


# ---------------------------------------------------------------------------------------------------- C. the whole encoder under a checkpoint-like init
_ENC = {}


def _enc_case(hw):
    """The checkpoint-like state_dict calibrated on this case's images, the fp64 encoder's f and GroupNorm ratios, and the float restatement's f: once per session."""
    if hw not in _ENC:
        from torch_ref_encode import img_to_f_torch
        from vae_ckpt_init import checkpoint_like_encoder_state_dict, encoder_model, encoder_reference_fp64
        B, pns = (2, LADDER_256) if hw == 256 else (1, LADDER_512)
        img = _u8_images(B, hw, hw)
        t0 = time.time()
        sd = checkpoint_like_encoder_state_dict(img, patch_nums=pns)
        f64, ratios = encoder_reference_fp64(sd, img, patch_nums=pns)
        vae = encoder_model(sd, patch_nums=pns)
        f32 = img_to_f_torch(vae, img)
        _ENC[hw] = dict(img=img, sd=sd, pns=pns, f64=f64, ratios=ratios, e32=(f32.double() - f64).abs().max().item(), vae=vae, secs=time.time() - t0)
    return _ENC[hw]


@pytest.mark.parametrize("cm", MODES)
@pytest.mark.parametrize("hw", [256, 512])
def test_encoder_checkpoint_like_init_vs_fp64(dev, hw, cm):
    """The whole HIP encode (engine.VaeEncCtx) against the fp64 CPU encode of the same weights: GroupNorm affines and conv biases far from the stress init's
    identity / constant, every residual-stream group at |mean| / std 10 .. 30 (the Downsample2x convolutions read that stream raw); 512^2 runs the three attention
    blocks at 1024 keys with C = 640.  Condition (from the reference alone): the largest |mean| / std at a GroupNorm lies in 10 .. 100 (100: the limit of float
    statistics, tests/test_gpu_vae_kernels.py).  Bar: max(4 e32, 2e-5 max(1, max|f64|)) with e32 the float restatement's own error against fp64 in the same
    run (4 = f16x2's 2^-22 operand precision over float's 2^-24; the second term is the single-kernel bar).  Measured: DESIGN.md section 4c."""
    c = _enc_case(hw)
    f64 = c["f64"]
    print(f"encoder {hw}^2: init + fp64 + float references {c['secs']:.1f} s; max|f64| {f64.abs().max().item():.2f}; per-channel offsets of f up to "
          f"{f64.mean((0, 2, 3)).abs().max().item():.2f}; |mean|/std at the GroupNorms: " + " ".join(f"{r:.1f}" for r in c["ratios"]))
    assert 10.0 <= max(c["ratios"]) <= 100.0, max(c["ratios"])
    assert f64.abs().max().item() <= 10.0
    B = c["img"].shape[0]
    sd = {k: v for k, v in c["sd"].items() if k.startswith(("encoder.", "quant_conv."))}
    ctx = E.VaeEncCtx(sd, B, dev, latent_hw=hw // 16, conv_mode=cm)
    got = ctx.encode(c["img"].to(dev)).cpu().double()
    ctx.close()
    err = (got - f64).abs().max().item()
    bar = max(4 * c["e32"], BAR * max(1.0, f64.abs().max().item()))
    print(f"encoder {hw}^2 {cm}: max|f_hip - f64| {err:.2e}; float restatement e32 {c['e32']:.2e}; bar {bar:.2e}")
    assert err <= bar, (err, bar)


# ---------------------------------------------------------------------------------------------------- D. the residual quantisation chain on HIP
def _run_chain(dev, vae, f, max_batch, B=None):
    """QuantCtx.encode(per_scale=True) of f[:B] -> (ids, f_hat, per-scale f_hat) on the CPU"""
    ctx = E.QuantCtx(vae.state_dict(), vae.quantize.v_patch_nums, max_batch, dev)
    try:
        ids, f_hat, ps = ctx.encode(f[:B].to(dev), per_scale=True)
        torch.cuda.synchronize()
        return ids.cpu(), f_hat.cpu(), ps.cpu()
    finally:
        ctx.close()


def _assert_chain(name, f, ids, f_hat, ps, vae64):
    rep = check_chain(f, ids, ps, vae64, f_hat_out=f_hat)
    print(f"\n{name}\n{rep}")
    assert rep.ok, rep.failures
    return rep


@pytest.mark.parametrize("hw", [256, 512])
def test_chain_on_encoder_f(dev, hw):
    """The f of test C (the fp64 encoder's, rounded to float) through QuantCtx.encode with the checkpoint-like model's codebook (V = 4096, N(0, 1)) and its four
    partially shared Phi; then idxBl_to_var_input of the device's own ids against the fp64 restatement (bar 2e-5 max(1, max|ref|))."""
    from torch_ref_encode import idxBl_to_var_input_torch
    c = _enc_case(hw)
    vae, vae64 = c["vae"], _double(c["vae"])
    f = c["f64"].float()
    B = f.shape[0]
    ids, f_hat, ps = _run_chain(dev, vae, f, B)
    rep = _assert_chain(f"chain on the encoder's f, {hw}^2, B = {B}", f, ids, f_hat, ps, vae64)
    assert rep.decidable >= 0.95, rep.decidable
    pns = c["pns"]
    ends = np.cumsum([p * p for p in pns])
    ms = [ids[:, e - p * p:e].contiguous() for p, e in zip(pns, ends)]
    dq = quant_on(dev, vae)
    vi = dq.idxBl_to_var_input([t.to(dev) for t in ms]).cpu().double()
    dq.refresh_hip()
    ref = idxBl_to_var_input_torch(vae64, ms)
    err = (vi - ref).abs().max().item()
    print(f"idxBl_to_var_input {hw}^2: max|err| {err:.2e} (max|ref| {ref.abs().max().item():.2f})")
    assert tuple(vi.shape) == (B, ends[-1] - 1, 32)
    assert err <= BAR * max(1.0, ref.abs().max().item()), err


def _double(vae):
    import copy
    return copy.deepcopy(vae).double()


def quant_on(dev, vae):
    """a copy of vae's quantizer on the device (the public Quantizer methods need GPU parameters)"""
    import copy
    return copy.deepcopy(vae.quantize).to(dev)


@pytest.mark.parametrize("B", [1, 3, 4])
def test_chain_three_decade_codebook(dev, B):
    """Synthetic checkpoint-like f (offsets of a few units, max|f| <= 10) against a V = 4096 codebook whose row norms span three decades; max_batch = 4 and
    B = 1, 3, max_batch.  Condition (from the reference): at least 95 % of the rows decidable."""
    vae = quant_model(three_decade_codebook(4096, 2), LADDER_256)
    f = checkpoint_like_f(4, 16, seed=21)
    ids, f_hat, ps = _run_chain(dev, vae, f, 4, B)
    rep = _assert_chain(f"three-decade codebook, B = {B} of max_batch 4", f[:B], ids, f_hat, ps, _double(vae))
    assert rep.decidable >= 0.95, rep.decidable


@pytest.mark.parametrize("share,name", [(1, "shared"), (0, "non-shared"), (4, "partially shared (4)"), (3, "partially shared (3)")])
@pytest.mark.parametrize("pns", [LADDER_256, LADDER_512], ids=["ladder256", "ladder512"])
def test_chain_every_phi_layout(dev, pns, share, name):
    """The three Phi layouts QuantCtx reads (quantize.quant_resi.qresi / .<k> / .qresi_ls.<k>), each Phi with its own weights and bias, on both ladders (HW = 32 is
    the largest map quant_phi_rest_kernel<true> stages in LDS), B = 3."""
    vae = quant_model(three_decade_codebook(512, 5), pns, share_quant_resi=share)
    f = checkpoint_like_f(3, pns[-1], seed=31 + share)
    ids, f_hat, ps = _run_chain(dev, vae, f, 3)
    rep = _assert_chain(f"Phi {name}, ladder {pns}", f, ids, f_hat, ps, _double(vae))
    assert rep.decidable >= 0.95, rep.decidable


@pytest.mark.parametrize("pns,B", [((1, 2, 3, 5, 9), 3), (LADDER_1024, 1), (LADDER_1024, 2)], ids=["hw9", "hw64-B1", "hw64-B2"])
def test_chain_unstaged_phi_kernel(dev, pns, B):
    """quant_phi_rest_kernel<false> (csrc/quant.hip, quant_encode_stage): HW^2 = 81 is not a multiple of 4, and HW = 64 needs 512 KB where the staged form has
    140 KB of LDS - both take the unstaged kernel (HW = 64 is also the largest map QMAX_HW allows, and fourteen scales)."""
    assert (pns[-1] ** 2) % 4 != 0 or (32 * pns[-1] ** 2 + 288) * 4 > 140 * 1024
    vae = quant_model(three_decade_codebook(512, 6), pns)
    f = checkpoint_like_f(B, pns[-1], seed=41)
    ids, f_hat, ps = _run_chain(dev, vae, f, B)
    rep = _assert_chain(f"unstaged Phi, ladder {pns}, B = {B}", f, ids, f_hat, ps, _double(vae))
    assert rep.decidable >= 0.95, rep.decidable


# ---------------------------------------------------------------------------------------------------- E. public path and reload
def _public_model(dev):
    from sdvar_amd.vqvae import VQVAE
    c = _enc_case(256)
    vae = VQVAE(vocab_size=4096, ch=160, v_patch_nums=c["pns"]).to(dev)
    vae.load_state_dict(c["sd"], strict=True)
    return c, vae


def _host_copy(vae):
    """the device model's quantizer parameters in a .double() CPU container for check_chain"""
    from sdvar_amd.vqvae import VQVAE
    m = VQVAE(vocab_size=vae.V, ch=32, with_encoder=False, v_patch_nums=vae.quantize.v_patch_nums)
    m.quantize.load_state_dict({k: v.detach().cpu() for k, v in vae.quantize.state_dict().items()})
    return m.double()


def test_public_path_is_the_composition_bit_for_bit(dev):
    c, vae = _public_model(dev)
    x = c["img"].to(dev)
    f = vae.img_to_f(x)
    ids = vae.img_to_idxBl(x)
    ids2 = vae.quantize.f_to_idxBl_or_fhat(f, to_fhat=False)
    assert len(ids) == len(c["pns"]) and all(torch.equal(a, b) for a, b in zip(ids, ids2))
    fh = vae.quantize.f_to_idxBl_or_fhat(f, to_fhat=True)
    rec = vae.img_to_reconstructed_img(x, last_one=True)
    assert torch.equal(rec, vae.fhat_to_img(fh[-1]))
    recs = vae.img_to_reconstructed_img(x, last_one=False)
    assert len(recs) == len(fh) and all(torch.equal(r, vae.fhat_to_img(h)) for r, h in zip(recs, fh))
    rep = check_chain(f, ids, fh, _host_copy(vae))
    print(f"\npublic path on the HIP encoder's own f\n{rep}")
    assert rep.ok, rep.failures


def test_codebook_reload_and_refresh(dev):
    """After load_state_dict with a permuted and rescaled codebook, and after refresh_hip() following an in-place edit of the codebook, the ids are those of the
    new codebook under check_chain (|e_v|^2 is cached per bind: a stale one fails rule (a) on most rows)."""
    c, vae = _public_model(dev)
    f = c["f64"].float().to(dev)
    q = vae.quantize
    ids0 = torch.cat(q.f_to_idxBl_or_fhat(f, to_fhat=False), 1)
    perm = torch.randperm(4096, generator=torch.Generator().manual_seed(3))
    scale = 0.5 + 1.5 * torch.rand(4096, 1, generator=torch.Generator().manual_seed(4))
    sd = {k: v.clone() for k, v in c["sd"].items()}
    sd["quantize.embedding.weight"] = (sd["quantize.embedding.weight"] * scale)[perm].contiguous()
    vae.load_state_dict(sd, strict=True)
    ids1 = q.f_to_idxBl_or_fhat(f, to_fhat=False)
    fh1 = q.f_to_idxBl_or_fhat(f, to_fhat=True)
    rep = check_chain(f, ids1, fh1, _host_copy(vae))
    print(f"\nafter load_state_dict with a permuted and rescaled codebook\n{rep}")
    assert rep.ok, rep.failures
    assert not torch.equal(torch.cat(ids1, 1), ids0)
    with torch.no_grad():
        q.embedding.weight.copy_(q.embedding.weight.flip(0) * 0.75)
    q.refresh_hip()
    ids2 = q.f_to_idxBl_or_fhat(f, to_fhat=False)
    fh2 = q.f_to_idxBl_or_fhat(f, to_fhat=True)
    rep = check_chain(f, ids2, fh2, _host_copy(vae))
    print(f"\nafter an in-place codebook edit and refresh_hip()\n{rep}")
    assert rep.ok, rep.failures


def test_second_bind_recomputes_code_norms(dev):
    """sdvar_quant_bind on a handle that has already encoded: the |e_v|^2 cache (e2_ready, csrc/api.hip) belongs to the previous codebook and must be rebuilt."""
    vae = quant_model(three_decade_codebook(512, 7), LADDER_256)
    f = checkpoint_like_f(2, 16, seed=51)
    ctx = E.QuantCtx(vae.state_dict(), LADDER_256, 2, dev)
    try:
        ids, f_hat, ps = ctx.encode(f.to(dev), per_scale=True)
        assert check_chain(f, ids, ps, _double(vae), f_hat_out=f_hat).ok
        vae2 = quant_model(torch.randn(512, 32, generator=torch.Generator().manual_seed(8)) * 2.0, LADDER_256)
        ctx.codebook = vae2.quantize.embedding.weight.data.to(dev).contiguous()                   # kept alive by the context, like the first one
        n = len(ctx.pw)
        aw = (C.c_void_p * n)(*[t.data_ptr() for t in ctx.pw]); ab = (C.c_void_p * n)(*[t.data_ptr() for t in ctx.pb])
        E._check(ctx.lib.sdvar_quant_bind(ctx.h, _p(ctx.codebook), aw, ab))
        ids, f_hat, ps = ctx.encode(f.to(dev), per_scale=True)
        torch.cuda.synchronize()
        rep = check_chain(f, ids, ps, _double(vae2), f_hat_out=f_hat)
        print(f"\nafter a second sdvar_quant_bind\n{rep}")
        assert rep.ok, rep.failures
    finally:
        ctx.close()
