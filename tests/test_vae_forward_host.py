"""VQVAE.forward / Quantizer.forward / evaluate.eval_vae: what can be checked without a GPU - the public signatures (the reference's parameter
names, vqvae.py:56 and quant.py:52), the beta argument, and the refusals, which must come before any device work."""
import inspect

import pytest
import torch

PNS = (1, 2, 4)


def _vae(**kw):
    from sdvar_amd.vqvae import VQVAE
    return VQVAE(vocab_size=64, ch=32, v_patch_nums=PNS, **kw)


def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_forward_signatures_match_the_reference():
    from sdvar_amd.vqvae import VQVAE, Quantizer
    E = inspect.Parameter.empty
    assert _params(VQVAE.forward) == [("self", E), ("inp", E), ("ret_usages", False)]                 # vqvae.py:56
    assert _params(Quantizer.forward) == [("self", E), ("f_BChw", E), ("ret_usages", False)]          # quant.py:52
    # a real method, not nn.Module's placeholder
    assert VQVAE.forward is not torch.nn.Module.forward and Quantizer.forward is not torch.nn.Module.forward
    from sdvar_amd import evaluate
    assert [n for n, _ in _params(evaluate.eval_vae)] == ["vae", "ld_val"]


def test_beta_is_accepted_and_stored():
    from sdvar_amd.vqvae import Quantizer
    assert _vae().quantize.beta == 0.25                                                                # quant.py:18
    assert _vae(beta=1.0).quantize.beta == 1.0
    assert Quantizer(64, 32, PNS, beta=0.5).beta == 0.5
    assert inspect.signature(Quantizer.__init__).parameters["beta"].default == 0.25
    assert "beta" not in _vae(beta=0.5).state_dict()                                                   # the checkpoint layout is untouched


def test_cpu_input_is_refused():
    from sdvar_amd.engine import SdvarError
    vae = _vae()
    with pytest.raises(SdvarError, match="GPU tensors"):
        vae(torch.zeros(1, 3, 64, 64))
    with pytest.raises(SdvarError, match="GPU tensors"):
        vae.quantize(torch.zeros(1, 32, 4, 4), ret_usages=True)


def test_training_mode_is_refused():
    from sdvar_amd.engine import SdvarError
    vae = _vae()
    vae.train()
    with pytest.raises(SdvarError, match="training mode"):
        vae(torch.zeros(1, 3, 64, 64))
    with pytest.raises(SdvarError, match="training mode"):
        vae.quantize(torch.zeros(1, 32, 4, 4))
    vae.eval()
    with pytest.raises(SdvarError, match="GPU tensors"):                                                # eval mode again: only the device is wrong
        vae(torch.zeros(1, 3, 64, 64))


def test_input_that_requires_grad_is_refused():
    from sdvar_amd.engine import SdvarError
    vae = _vae()
    x = torch.zeros(1, 3, 64, 64, requires_grad=True)
    f = torch.zeros(1, 32, 4, 4, requires_grad=True)
    with torch.enable_grad():                                                                           # other test modules switch grad mode off globally
        with pytest.raises(SdvarError, match="no backward exists"):
            vae(x)
        with pytest.raises(SdvarError, match="no backward exists"):
            vae.quantize(f)
    with torch.no_grad():                                                                               # grad mode off: nothing to differentiate, so the device decides
        with pytest.raises(SdvarError, match="GPU tensors"):
            vae(x)


def test_eval_vae_refuses_an_empty_loader_and_restores_the_mode():
    from sdvar_amd import evaluate
    from sdvar_amd.engine import SdvarError
    vae = _vae()
    vae.train()
    with pytest.raises(SdvarError, match="no images"):
        evaluate.eval_vae(vae, [])
    assert vae.training


def test_new_entry_points_are_declared_and_bound():
    """Additive ABI: the three new symbols are in the header and the binding, and the version is still 5 (tests/test_abi.py compares the full sets)."""
    from sdvar_amd import engine as E
    lib = E.load_library()
    for name, nargs in (("sdvar_quant_encode_stats", 10), ("sdvar_vae_decode_raw", 5), ("sdvar_img_err_stats", 6)):
        assert hasattr(lib, name) and len(E._SIGNATURES[name][1]) == nargs
    assert E.ABI_VERSION == 5
    assert lib.sdvar_img_err_stats(None, None, 0, None, 0, None) == 1 and b"img_err_stats" in lib.sdvar_last_error()
    assert lib.sdvar_quant_encode_stats(None, None, 1, None, None, None, None, None, None, None) == 1


def test_allreduce_vae_sums_without_a_process_group():
    import numpy as np
    from sdvar_amd import dist as D
    hits = np.arange(6, dtype=np.int64).reshape(2, 3)
    out = D.allreduce_vae_sums(torch.tensor([1.5, 2.5], dtype=torch.float64), 0.75, 12, 3, hits)
    assert out[:5] == (1.5, 2.5, 0.75, 12.0, 3.0) and np.array_equal(out[5], hits) and out[5].dtype == np.int64


def test_usages_of_the_reference_fixture():
    """quant.py:100-102 is host arithmetic here: the fixture's ema array gives the reference's usages (B = 2, 16 x 16 rows per image, world size 1)."""
    from conftest import golden
    from sdvar_amd.vqvae import Quantizer
    g = golden("vae_forward_256")
    q = Quantizer(4096, 32, tuple(int(p) for p in g["patch_nums"]))
    q.ema_vocab_hit_SV.copy_(torch.from_numpy(g["ema"]))
    got = q._usages(2 * 16 * 16)
    assert len(got) == 10 and max(abs(a - b) for a, b in zip(got, g["usages"])) <= 1e-9
    assert abs(float(g["margin"]) - 0.01) < 1e-15 and float(abs(g["ema"].astype("float64") - float(g["margin"])).min()) > 1e-6
