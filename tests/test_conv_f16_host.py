"""Host, no GPU: the premises of tests/test_gpu_conv_f16_exact.py and the Python rules of conv_mode "f16" that are decided before any device call.

Premises: on every f16x2 'dense' and 'sparse' case of tests/conv_exact_cases.py the plane-0-only product has ONE right answer in fp32 (every partial sum below
2^24 grains) and that answer is not the three-product reference's: a kernel that keeps hl or lh, or reads plane 1 at all, cannot pass the GPU test."""
import pytest
import torch

import conv_exact_cases as X
import conv_f16_cases as H
from sdvar_amd import engine as E

SPLIT_CASES = H.split_plane_cases()


@pytest.mark.parametrize("c", SPLIT_CASES, ids=lambda c: c.id)
def test_plane0_product_is_exact_and_differs_from_three_products(c):
    bound, grain, bits = H.prove_exact_hh(c)
    assert bound / grain < 2 ** 24, (c.id, bound, grain, bits)
    for res in ((False, True) if c.res is not None else (False,)):
        hh, three = H.hh_ref(c, res), c.ref(2, res)
        assert torch.equal(hh.float().double(), hh), f"{c.id}: the plane-0 reference is not an fp32 value"
        differ = float((hh != three).double().mean())
        print(f"{c.id} res {int(res)}: {bits:.1f} bits, differs from the three-product reference on {100 * differ:.1f} % of outputs")
        assert differ >= 0.3, (c.id, differ)


def test_int_cases_have_zero_low_planes_and_cover_the_paths():
    """'int' operands are fixed points of the splitter, so the plane-0 product IS the float64 conv2d; the case list holds the sizes the GPU test names"""
    cases = H.int_cases()
    assert {c.M for c in cases} >= {1, 33, 255, 257}
    assert {c.taps for c in cases} == {1, 4, 9} and any(c.src == "prep_up" for c in cases)
    assert {c.taps * (c.Cin // 32) for c in cases} >= {1, 180}
    assert any(c.N % X.CBN for c in cases) and all(c.N % 4 == 0 for c in cases)
    assert any(X.stats_fuse(c, 1) for c in cases) and any(X.tap_reuse_eligible(c, 2, 2, 1, 1) for c in cases)
    for c in cases:
        assert not bool(c.x_planes(2)[1].any()) and not bool(c.w_planes(2)[1].any()), c.id
        assert torch.equal(H.hh_ref(c, False), c.ref(2, False)), c.id


def test_expected_kernel_codes():
    reuse = X.case("int", None, 1, 4, 64, 32, 32, 9, "prep")
    plain = X.case("int", None, 3, 6, 7, 96, 160, 9, "prep")
    assert H.expected_kernel(reuse, 1, 1) == 4 and H.expected_kernel(reuse, 0, 1) == 3 and H.expected_kernel(reuse, 1, 2) == 3
    assert H.expected_kernel(plain, 1, 1) == 3


# ---------------------------------------------------------------------------------------------------------------- engine rules (no device call)
def test_resolve_conv_mode_decoder(monkeypatch):
    monkeypatch.delenv("SDVAR_CONV_MODE", raising=False)
    assert E.resolve_conv_mode(None) == "f16x2"
    for m in ("bf16x3", "f16x2", "f16"):
        assert E.resolve_conv_mode(m) == m
    assert E.CONV_MODES == ("bf16x3", "f16x2", "f16")
    assert [E._CONV_PLANE_FORMAT[m] for m in E.CONV_MODES] == [3, 2, H.PF_HH]
    monkeypatch.setenv("SDVAR_CONV_MODE", "f16")
    assert E.resolve_conv_mode(None) == "f16"
    assert E.resolve_conv_mode("bf16x3") == "bf16x3"                    # the argument wins over the environment


def test_unknown_mode_lists_all_three(monkeypatch):
    monkeypatch.delenv("SDVAR_CONV_MODE", raising=False)
    with pytest.raises(E.SdvarError) as ei:
        E.resolve_conv_mode("fp8")
    for m in ("'bf16x3'", "'f16x2'", "'f16'", "'fp8'"):
        assert m in str(ei.value), str(ei.value)
    with pytest.raises(E.SdvarError) as ei:                              # before the state_dict is looked at or the library is loaded
        E.VaeCtx({}, 1, "cpu", conv_mode="fp8")
    assert "'f16'" in str(ei.value)
    monkeypatch.setenv("SDVAR_CONV_MODE", "f8")
    with pytest.raises(E.SdvarError):
        E.resolve_conv_mode(None)


def test_encoder_refuses_f16_and_maps_the_environment(monkeypatch):
    monkeypatch.delenv("SDVAR_CONV_MODE", raising=False)
    with pytest.raises(E.SdvarError) as ei:
        E.resolve_conv_mode("f16", encoder=True)
    assert "decoder" in str(ei.value) and "'f16x2'" in str(ei.value)
    with pytest.raises(E.SdvarError) as ei:
        E.VaeEncCtx({}, 1, "cpu", conv_mode="f16")                       # refused before anything else happens
    assert "decoder" in str(ei.value)
    monkeypatch.setenv("SDVAR_CONV_MODE", "f16")
    assert E.resolve_conv_mode(None, encoder=True) == "f16x2"           # encoding feeds the nearest-code search: ids must not move
    assert E.resolve_conv_mode("bf16x3", encoder=True) == "bf16x3"
    with pytest.raises(E.SdvarError):                                    # the explicit argument is still refused with the environment set
        E.resolve_conv_mode("f16", encoder=True)
    monkeypatch.setenv("SDVAR_CONV_MODE", "bf16x3")
    assert E.resolve_conv_mode(None, encoder=True) == "bf16x3"
    with pytest.raises(E.SdvarError) as ei:
        E.resolve_conv_mode("fp8", encoder=True)
    assert "'f16'" not in str(ei.value)


def test_vqvae_has_the_switch():
    from sdvar_amd.vqvae import VQVAE
    vae = VQVAE(vocab_size=64, z_channels=32, ch=32, with_encoder=False)
    assert vae.conv_mode is None
    vae.conv_mode = "fp8"
    with pytest.raises(E.SdvarError):
        vae.fhat_to_img(torch.zeros(1, 32, 16, 16))                      # a CPU tensor: refused before any device call either way
