"""VQVAE image side (encoder + multi-scale quantisation) without a GPU: the encoder's bind walk, argument errors of the new C-ABI entry points,
the SdvarError of every unsupported case, and the PyTorch restatement (tests/torch_ref_encode.py) against the reference fixture."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden_parts
from sdvar_amd.ladder import LADDER_256


def _desc(E, ch, B=1, latent=16):
    d = E._VaeDesc()
    d.ch, d.z_channels, d.n_mult, d.num_res_blocks, d.max_batch, d.latent_hw = ch, 32, 5, 2, B, latent
    for i, m in enumerate((1, 1, 2, 2, 4)):
        d.ch_mult[i] = m
    return d


@pytest.mark.parametrize("ch", [160, 32])
def test_encoder_bind_walk_matches_state_dict(ch):
    from sdvar_amd import engine as E
    from sdvar_amd.weights import vae_state_dict
    lib = E.load_library()
    sd = vae_state_dict(LADDER_256, "perf", 1, ch=ch, with_encoder=True)
    names = E.VaeEncCtx.tensor_names(sd)
    assert len(set(names)) == len(names)
    used = {n + s for n in names for s in (".weight", ".bias")}
    assert used == {k for k in sd if k.startswith(("encoder.", "quant_conv."))}
    assert lib.sdvar_vae_enc_tensor_count(C.byref(_desc(E, ch))) == 2 * len(names)


def test_encode_argument_errors_without_gpu():
    from sdvar_amd import engine as E
    lib = E.load_library()
    h = C.c_void_p()
    d = _desc(E, 160)
    d.ch = 48                                                   # not a multiple of 32
    assert lib.sdvar_vae_enc_create(C.byref(d), C.byref(h)) == 1 and b"multiples of 32" in lib.sdvar_last_error()
    assert lib.sdvar_vae_enc_create(None, C.byref(h)) == 1
    assert lib.sdvar_vae_enc_tensor_count(None) == -1
    assert lib.sdvar_vae_enc_encode(None, None, 1, None, None) == 1 and b"null" in lib.sdvar_last_error()
    assert lib.sdvar_vae_enc_bind(None, None, 0, None) == 1
    assert lib.sdvar_vae_enc_destroy(None) == 0
    assert lib.sdvar_quant_encode(None, None, 1, None, None, None, None) == 1 and b"not bound" in lib.sdvar_last_error()
    assert lib.sdvar_op_quant_nearest(None, 4, None, 64, 32, None, None, None) == 1
    assert lib.sdvar_op_vae_s2d_planes(None, None, 0, 2, 1, 32, 8, 8, 7, None) == 1 and b"s2d_planes" in lib.sdvar_last_error()
    assert lib.sdvar_op_vae_img_planes(None, None, 0, 2, 1, 8, 8, 11, None) == 1 and b"img_planes" in lib.sdvar_last_error()
    assert lib.sdvar_op_vae_s2d_weights(None, None, 4, 4, None) == 1


def _vqvae(**kw):
    from sdvar_amd.vqvae import VQVAE
    return VQVAE(vocab_size=64, ch=32, v_patch_nums=(1, 2, 4), **kw)


def test_public_methods_raise_on_cpu_and_unsupported_cases():
    from sdvar_amd.engine import SdvarError
    vae = _vqvae()
    img = torch.zeros(1, 3, 64, 64)
    f = torch.zeros(1, 32, 4, 4)
    ids = [torch.zeros(1, p * p, dtype=torch.int64) for p in (1, 2, 4)]
    for call in (lambda: vae.img_to_idxBl(img), lambda: vae.img_to_reconstructed_img(img, last_one=True),
                 lambda: vae.idxBl_to_img(ids, same_shape=True), lambda: vae.quantize.f_to_idxBl_or_fhat(f, True),
                 lambda: vae.quantize.idxBl_to_var_input(ids),
                 lambda: vae.embed_to_img([torch.zeros(1, 32, p, p) for p in (1, 2, 4)], all_to_max_scale=True)):
        with pytest.raises(SdvarError, match="GPU"):
            call()
    with pytest.raises(SdvarError, match="all_to_max_scale"):
        vae.quantize.embed_to_fhat([torch.zeros(1, 32, p, p) for p in (1, 2, 4)], all_to_max_scale=False)
    with pytest.raises(SdvarError, match="same_shape"):
        vae.idxBl_to_img(ids, same_shape=False)
    with pytest.raises(SdvarError, match="with_encoder=False"):
        _vqvae(with_encoder=False).img_to_idxBl(img)
    assert _vqvae(using_znorm=True).quantize.using_znorm and not vae.quantize.using_znorm
    with pytest.raises(SdvarError, match="non-square"):
        vae.quantize._ladder([(1, 1), (2, 3), (4, 4)])
    assert vae.quantize._ladder([(1, 1), 2, (4, 4)]) == (1, 2, 4)
    assert not any("forward" in type(m).__dict__ for m in vae.modules() if type(m).__module__ == "sdvar_amd.vqvae")


def test_using_znorm_is_refused_before_any_device_work():
    from sdvar_amd.engine import SdvarError
    q = _vqvae(using_znorm=True).quantize
    with pytest.raises(SdvarError, match="using_znorm"):
        q._ctx(torch.device("cpu"), 1, (1, 2, 4))


@pytest.mark.parametrize("name", ["encode_256"])
def test_torch_restatement_reproduces_the_reference_fixture(name):
    from sdvar_amd.vqvae import VQVAE
    from sdvar_amd.weights import vae_state_dict
    from torch_ref_encode import f_to_idxBl_or_fhat_torch, idxBl_to_var_input_torch, img_to_f_torch
    g = golden_parts(name)
    pns = tuple(int(p) for p in g["patch_nums"])
    vae = VQVAE(vocab_size=4096, ch=160, v_patch_nums=pns)
    vae.load_state_dict(vae_state_dict(pns, "perf", int(g["wseed"]), with_encoder=True), strict=True)
    x = torch.from_numpy(g["img_u8"]).float() / 127.5 - 1.0
    torch.set_num_threads(8)
    f = img_to_f_torch(vae, x)
    assert (f - torch.from_numpy(g["f"])).abs().max().item() <= 1e-5
    ids = f_to_idxBl_or_fhat_torch(vae, torch.from_numpy(g["f"]), False)
    assert np.array_equal(torch.cat(ids, 1).numpy(), g["ids"])
    fh = f_to_idxBl_or_fhat_torch(vae, torch.from_numpy(g["f"]), True)
    assert (fh[-1] - torch.from_numpy(g["f_hat"])).abs().max().item() <= 1e-5
    vi = idxBl_to_var_input_torch(vae, ids)
    assert (vi - torch.from_numpy(g["var_input"])).abs().max().item() <= 1e-5
