"""VQVAE image side on the GPU: the encoder's new operand producers (space-to-depth Downsample2x, conv_in), the nearest-code kernel, and the
public methods (img_to_idxBl, f_to_idxBl_or_fhat, idxBl_to_var_input, img_to_reconstructed_img, idxBl_to_img) against the reference fixtures
of tests/golden/make_encode_golden.py, in both convolution operand formats."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden_parts, rnd

pytestmark = pytest.mark.gpu
MODES = ["f16x2", "bf16x3"]
_SD = {}


def _guard(W):
    return (W + 3 + 15) // 16 * 16


def _conv_on_planes(E, lib, dev, mode, xplanes, ops, rows, G, w, b, B, H, W, Cin, force_split=0):
    pf = 3 if mode == "bf16x3" else 2
    npl = 3 if mode == "bf16x3" else 2
    Cout = w.shape[0]
    wps = 9 * Cin * Cout
    wp = torch.empty(npl * wps, dtype=torch.int16, device=dev)
    sc = torch.zeros(4, device=dev)
    E._check(lib.sdvar_op_conv_weight_planes(E._ptr(w.contiguous()), E._ptr(wp), Cout, Cin, 9, wps, pf, E._ptr(sc) if pf == 2 else None, E._stream()))
    out = torch.empty(B * H * W, Cout, device=dev)
    ws = torch.empty(16 * B * H * W * Cout, device=dev) if force_split else None
    E._check(lib.sdvar_op_conv_planes(E._ptr(xplanes), ops, rows, G, E._ptr(wp), wps, pf, E._ptr(sc) if pf == 2 else None, E._ptr(b), None, E._ptr(out),
                                      B, H, W, Cout, Cin, 9, E._ptr(ws), ws.numel() if ws is not None else 0, force_split, E._stream()))
    return out.view(B, H, W, Cout).permute(0, 3, 1, 2)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C_,H,split", [(160, 32, 0), (320, 16, 0), (320, 64, 0), (320, 16, 4)])
def test_s2d_downsample_conv(dev, mode, C_, H, split):
    from sdvar_amd import engine as E
    lib = E.load_library()
    B = 2
    x = rnd(1, (B, C_, H, H)).to(dev)
    w = rnd(2, (C_, C_, 3, 3), (C_ * 9) ** -0.5).to(dev)
    b = rnd(3, (C_,), 0.1).to(dev)
    ref = F.conv2d(F.pad(x.double(), (0, 1, 0, 1)), w.double(), b.double(), stride=2)
    Ho = H // 2
    G = _guard(Ho)
    rows = B * (Ho + 2) * (Ho + 2) + 2 * G
    ops = rows * 4 * C_
    npl = 3 if mode == "bf16x3" else 2
    planes = torch.empty(npl * ops, dtype=torch.int16, device=dev)
    xr = x.permute(0, 2, 3, 1).contiguous()
    E._check(lib.sdvar_op_vae_s2d_planes(E._ptr(xr), E._ptr(planes), ops, 3 if mode == "bf16x3" else 2, B, C_, H, H, G, E._stream()))
    w4 = torch.empty(C_, 4 * C_, 3, 3, device=dev)
    E._check(lib.sdvar_op_vae_s2d_weights(E._ptr(w), E._ptr(w4), C_, C_, E._stream()))
    out = _conv_on_planes(E, lib, dev, mode, planes, ops, rows, G, w4, b, B, Ho, Ho, 4 * C_, split)
    err = (out.double() - ref).abs().max().item()
    assert err <= 2e-5 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("mode", MODES)
def test_conv_in_on_image_planes(dev, mode):
    from sdvar_amd import engine as E
    lib = E.load_library()
    B, H, Co = 2, 64, 160
    img = (rnd(4, (B, 3, H, H)).clamp(-3, 3) / 3).to(dev)
    w = rnd(5, (Co, 3, 3, 3), 27 ** -0.5).to(dev)
    b = rnd(6, (Co,), 0.1).to(dev)
    ref = F.conv2d(img.double(), w.double(), b.double(), padding=1)
    G = _guard(H)
    rows = B * (H + 2) * (H + 2) + 2 * G
    ops = rows * 32
    npl = 3 if mode == "bf16x3" else 2
    planes = torch.empty(npl * ops, dtype=torch.int16, device=dev)
    E._check(lib.sdvar_op_vae_img_planes(E._ptr(img), E._ptr(planes), ops, 3 if mode == "bf16x3" else 2, B, H, H, G, E._stream()))
    w32 = torch.zeros(Co, 32, 3, 3, device=dev)
    w32[:, :3] = w
    out = _conv_on_planes(E, lib, dev, mode, planes, ops, rows, G, w32, b, B, H, H, 32)
    err = (out.double() - ref).abs().max().item()
    assert err <= 2e-5 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("V", [4096, 64])
def test_nearest_code(dev, V):
    from sdvar_amd import engine as E
    lib = E.load_library()
    N = 1000
    z = rnd(7, (N, 32), 0.5).to(dev)
    cb = rnd(8, (V, 32)).to(dev)
    cb[V // 2] = cb[3]                                         # planted duplicates: the lower index must win
    cb[V - 1] = cb[5]
    z[10] = cb[3]; z[11] = cb[5]
    ids = torch.empty(N, dtype=torch.int64, device=dev)
    e2 = torch.empty(V, device=dev)
    E._check(lib.sdvar_op_quant_nearest(E._ptr(z), N, E._ptr(cb), V, 32, E._ptr(e2), E._ptr(ids), E._stream()))
    z64, c64 = z.double().cpu(), cb.double().cpu()
    d = (z64 * z64).sum(1, keepdim=True) + (c64 * c64).sum(1) - 2 * z64 @ c64.T
    best = d.min(1).values
    got = d.gather(1, ids.cpu().view(-1, 1)).view(-1)
    scale = (z64 * z64).sum(1) + (c64 * c64).sum(1).mean()
    assert ((got - best) / scale).max().item() <= 1e-6
    assert ids[10].item() == 3 and ids[11].item() == 5


def _model(name, dev):
    from sdvar_amd.vqvae import VQVAE
    from sdvar_amd.weights import vae_state_dict
    g = golden_parts(name)
    pns = tuple(int(p) for p in g["patch_nums"])
    if name not in _SD:
        _SD[name] = vae_state_dict(pns, "perf", int(g["wseed"]), with_encoder=True)
    vae = VQVAE(vocab_size=4096, ch=160, v_patch_nums=pns).to(dev)
    vae.load_state_dict(_SD[name], strict=True)
    x = (torch.from_numpy(g["img_u8"]).float() / 127.5 - 1.0).to(dev)
    return g, vae, x


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["encode_256", "encode_512"])
def test_img_to_idxBl_matches_reference(dev, monkeypatch, mode, name):
    monkeypatch.setenv("SDVAR_CONV_MODE", mode)
    g, vae, x = _model(name, dev)
    f = vae.img_to_f(x)
    err = (f.cpu() - torch.from_numpy(g["f"])).abs().max().item()
    print(f"{name} {mode}: f max|diff| {err:.2e} (tolerance {float(g['f_tol']):.0e}; no id can flip within {float(g['f_tol']) * float(g['margin_safety']):.1e})")
    assert err <= float(g["f_tol"]) and float(g["margin_safety"]) >= 1.0          # make_encode_golden.py: the fixture's ids are stable within f_tol
    ids = vae.img_to_idxBl(x)
    pns = tuple(int(p) for p in g["patch_nums"])
    assert [tuple(t.shape) for t in ids] == [(x.shape[0], p * p) for p in pns] and ids[0].dtype == torch.int64
    assert np.array_equal(torch.cat(ids, 1).cpu().numpy(), g["ids"])


@pytest.mark.parametrize("name", ["encode_256", "encode_512"])
def test_f_to_fhat_and_var_input(dev, name):
    g, vae, _ = _model(name, dev)
    f = torch.from_numpy(g["f"]).to(dev)
    fh = vae.quantize.f_to_idxBl_or_fhat(f, to_fhat=True)
    assert len(fh) == len(g["patch_nums"])
    assert (fh[-1].cpu() - torch.from_numpy(g["f_hat"])).abs().max().item() <= 1e-5
    for k, s in enumerate(g["per_scale"]):
        assert (fh[int(s)].cpu() - torch.from_numpy(g["f_hat_per_scale"][k])).abs().max().item() <= 1e-5
    ids = vae.quantize.f_to_idxBl_or_fhat(f, to_fhat=False)
    assert np.array_equal(torch.cat(ids, 1).cpu().numpy(), g["ids"])
    L = g["ids"].shape[1]
    gt = [torch.from_numpy(g["ids"][:, b:e]).to(dev) for b, e in zip(np.cumsum([0] + [p * p for p in g["patch_nums"]])[:-1], np.cumsum([p * p for p in g["patch_nums"]]))]
    vi = vae.quantize.idxBl_to_var_input(gt)
    assert tuple(vi.shape) == (f.shape[0], L - 1, 32)
    assert (vi.cpu() - torch.from_numpy(g["var_input"])).abs().max().item() <= 1e-5


@pytest.mark.parametrize("mode", MODES)
def test_reconstruction_and_idxBl_to_img(dev, monkeypatch, mode):
    monkeypatch.setenv("SDVAR_CONV_MODE", mode)
    g, vae, x = _model("encode_256", dev)
    img = vae.img_to_reconstructed_img(x[:1], last_one=True)
    err = (img[0].cpu() - torch.from_numpy(g["recon0"])).abs().max().item()
    print(f"recon {mode}: max|diff| {err:.2e}")
    assert err <= 1e-4
    imgs = vae.img_to_reconstructed_img(x[:1], last_one=False)
    assert len(imgs) == len(g["patch_nums"]) and torch.equal(imgs[-1], img)
    pn = [int(p) for p in g["patch_nums"]]
    ends = np.cumsum([p * p for p in pn])
    gt = [torch.from_numpy(g["ids"][:, e - p * p:e]).to(dev) for p, e in zip(pn, ends)]
    from_ids = vae.idxBl_to_img(gt, same_shape=True, last_one=False)
    assert len(from_ids) == len(pn)
    for k, s in enumerate(g["per_scale"]):
        want = vae.fhat_to_img(torch.from_numpy(g["f_hat_per_scale"][k]).to(dev))
        assert (from_ids[int(s)] - want).abs().max().item() <= 1e-4
    assert torch.equal(vae.idxBl_to_img(gt, same_shape=True, last_one=True), from_ids[-1])
    # embed_to_img from the codebook vectors of the same ids
    E_ = vae.quantize.embedding.weight
    ms_h = [E_[t].transpose(1, 2).reshape(t.shape[0], 32, p, p) for t, p in zip(gt, pn)]
    assert (vae.embed_to_img(ms_h, all_to_max_scale=True, last_one=True) - from_ids[-1]).abs().max().item() <= 1e-5


def test_batch_independence_determinism_and_reload(dev):
    g, vae, x = _model("encode_256", dev)
    x3 = torch.cat([x, x[:1]], 0)
    f3 = vae.img_to_f(x3)
    ids3 = torch.cat(vae.img_to_idxBl(x3), 1)
    for b in range(3):
        f1 = vae.img_to_f(x3[b:b + 1])
        assert (f1 - f3[b:b + 1]).abs().max().item() <= 1e-5
        assert torch.equal(torch.cat(vae.img_to_idxBl(x3[b:b + 1]), 1), ids3[b:b + 1])
    assert torch.equal(vae.img_to_f(x3), f3)
    sd = {k: v.clone() for k, v in _SD["encode_256"].items()}
    sd["encoder.conv_in.weight"] = sd["encoder.conv_in.weight"] * 1.5
    sd["quant_conv.bias"] = sd["quant_conv.bias"] + 0.25
    vae.load_state_dict(sd, strict=True)
    f_new = vae.img_to_f(x3)
    assert (f_new - f3).abs().max().item() > 0.1
