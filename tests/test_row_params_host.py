"""Host side of the per-image sampling parameters (engine.RowParams, engine.Noise with sequences, the *_rows symbols): no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import row_params_cases as RC
from conftest import ROOT, state_dicts
from oracle import var_oracle as orc
from sdvar_amd import engine as E
from sdvar_amd.ladder import LADDER_256, as_ladder
from sdvar_amd.noise import exponential_noise

torch.set_grad_enabled(False)
LAD = as_ladder(LADDER_256)
ROWS_SYMBOLS = ("sdvar_cfg_sample_rows", "sdvar_verify_accept_rows", "sdvar_cfg_combine_rows", "sdvar_gumbel_mix_rows")


def _build(B, cfg, top_k, top_p, seed=0, image_offset=0, kind="device"):
    return E.RowParams.build(B, LAD, cfg, top_k, top_p, E.Noise(kind, seed, image_offset))


@pytest.mark.parametrize("form", ["list", "tuple", "numpy", "tensor"])
def test_tables_are_the_scalar_roundings(form):
    cfg, top_k, top_p = [1.5, 3.0, 0.75, 0.1], [900, 0, 40, 4096], [0.96, 0.0, 0.5, 1e-8]
    seeds, offs = [7, 2**63 + 5, 2**32, 0xFFFFFFFFFFFFFFFF], [0, 3, 2**32 - 1, 9]
    as_tensor = lambda x: torch.tensor(x, dtype=torch.float64 if isinstance(x[0], float) else torch.int64)
    conv = {"list": list, "tuple": tuple, "numpy": np.array, "tensor": as_tensor}[form]
    sd = seeds if form in ("numpy", "tensor") else conv(seeds)              # 64-bit seeds do not fit an int64 array: python ints there
    r = _build(4, conv(cfg), conv(top_k), conv(top_p), sd, conv(offs))
    assert r is not None and r.dev is None and r.fac.dtype == np.float32 and r.fac.shape == (LAD.S, 4, 2)
    for s in range(LAD.S):
        for b in range(4):
            t = LAD.cfg_t(cfg[b], s)
            assert r.fac[s, b, 0] == np.float32(1.0 + t) and r.fac[s, b, 1] == np.float32(t), (s, b)
    for b in range(4):
        row = r.img[b]
        assert row["top_k"] == top_k[b] and row["use_top_p"] == (1 if top_p[b] > 0 else 0)
        assert row["top_p_thr"] == np.float32(1.0 - top_p[b])
        assert (int(row["seed_hi"]) << 32) | int(row["seed_lo"]) == seeds[b] and row["index"] == offs[b] and not row["reserved"].any()
    assert r.img.dtype.itemsize == 32 and r.img_off == r.fac.nbytes


def test_all_scalar_builds_nothing():
    assert _build(3, 1.5, 900, 0.96, 5, 2) is None
    assert _build(3, np.float32(1.5), np.int64(900), torch.tensor(0.96), 5) is None
    assert not E.Noise("host", 5, 2).per_image and E.Noise("host", [5], 2).per_image


def test_one_sequence_is_enough_and_scalars_broadcast():
    r = _build(3, 1.5, [900, 0, 40], 0.96, 11, 4)
    assert r.cfg == [1.5] * 3 and r.top_p == [0.96] * 3 and r.seeds == [11] * 3
    assert r.index == [4, 5, 6]                                             # scalar seed: the counter stays image_offset + b
    r = _build(3, 1.5, 900, 0.96, [11, 12, 13])
    assert r.index == [0, 0, 0] and r.seeds == [11, 12, 13]                 # a sequence of seeds: every image is image 0 of its own stream
    assert _build(3, 1.5, 900, 0.96, 11, [8, 8, 2]).index == [8, 8, 2]
    assert _build(3, 1.5, 900, 0.96, [1, 2, 3], 5).index == [5, 5, 5]


@pytest.mark.parametrize("kw", [dict(cfg=[1.5, 2.0]), dict(top_k=[1, 2, 3, 4]), dict(top_p=[0.5]), dict(seed=[1, 2]), dict(image_offset=[0, 1])])
def test_wrong_length_raises(kw):
    a = dict(cfg=1.5, top_k=900, top_p=0.96, seed=0, image_offset=0)
    a.update(kw)
    with pytest.raises(E.SdvarError, match=next(iter(kw)) if "image_offset" not in kw and "seed" not in kw else "entries"):
        _build(3, **a)


def test_negative_top_k_raises():
    with pytest.raises(E.SdvarError, match="top_k"):
        _build(3, 1.5, [900, -1, 0], 0.96)


def test_seed_sequences_need_the_philox_stream():
    for kind, kw in (("torch", {}), ("fn", dict(fn=lambda d, B, l, V: np.ones((B * l, V), np.float32)))):
        with pytest.raises(E.SdvarError, match="sequence of seeds"):
            E.Noise(kind, [1, 2, 3], **kw)
        with pytest.raises(E.SdvarError):
            E.Noise(kind, 1, [0, 1, 2], **kw)
        n = E.Noise(kind, 4, **kw)                                          # per-image cfg / top_k / top_p keep working with these noise kinds
        r = E.RowParams.build(3, LAD, [1.0, 2.0, 3.0], 0, 0.0, n)
        assert r is not None and r.seeds == [4] * 3 and r.index == [0, 1, 2]
        assert n.tensor(0, 3, 4, 8, "cpu").shape == (12, 8)


def test_host_noise_rows():
    seeds, offs, l, V = [9, 2**40 + 1, 9], [0, 7, 1], 9, 16
    for draw in (0, 5, 3 | E.GUMBEL_DRAW):
        q = E.Noise("host", seeds, offs).tensor(draw, 3, l, V, "cpu").view(3, l, V).numpy()
        for b in range(3):
            assert np.array_equal(q[b], exponential_noise(seeds[b], draw, 1, l, V, offs[b])[0])
    q = E.Noise("host", 9, [4, 2, 0]).tensor(1, 3, l, V, "cpu").view(3, l, V).numpy()
    for b, o in enumerate([4, 2, 0]):
        assert np.array_equal(q[b], exponential_noise(9, 1, 1, l, V, o)[0])
    # a scalar seed and offset: the batch stream, as before
    assert np.array_equal(E.Noise("host", 9, 2).tensor(1, 3, l, V, "cpu").view(3, l, V).numpy(), exponential_noise(9, 1, 3, l, V, 2))
    assert E.Noise("device", seeds, offs).tensor(0, 3, l, V, "cpu") is None
    with pytest.raises(E.SdvarError):
        E.Noise("host", seeds).tensor(0, 2, l, V, "cpu")


def test_symbols_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "sdvar_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = E.load_library()
    for s in ROWS_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", code), f"{s} is not declared in include/sdvar_hip.h"
        assert s in E._SIGNATURES and hasattr(lib, s)
    assert "sdvar_row_image" in code and C.sizeof(E._RowImage) == 32


def test_rows_entry_points_check_their_arguments_without_gpu():
    """Null tables, B against the table length and a negative top_k are argument errors, reported before anything is launched."""
    lib = E.load_library()
    p = C.c_void_p(4096)                                                    # never dereferenced: every call below fails its argument checks
    img = (E._RowImage * 2)()
    lens = (C.c_int32 * 1)(4)
    sample = lambda fac, im, host, n: lib.sdvar_cfg_sample_rows(p, 2, 4, 8, fac, im, host, n, None, 0, p, 4, None, None)
    assert sample(None, p, img, 2) == 1 and b"null parameter table" in lib.sdvar_last_error()
    assert sample(p, None, img, 2) == 1 and sample(p, p, None, 2) == 1
    assert sample(p, p, img, 3) == 1 and b"tables hold 3" in lib.sdvar_last_error()
    img[1].top_k = -5
    assert sample(p, p, img, 2) == 1 and b"top_k[1] = -5" in lib.sdvar_last_error()
    verify = lambda fac, n: lib.sdvar_verify_accept_rows(p, 2, 4, 8, 1, lens, fac, n, p, 4, 0.5, 0, 0, 0.0, None, p, None, None, None, None)
    assert verify(None, 2) == 1 and b"null parameter table" in lib.sdvar_last_error()
    assert verify(p, 1) == 1 and b"holds 1" in lib.sdvar_last_error()
    combine = lambda fac, n: lib.sdvar_cfg_combine_rows(p, 2, 4, 8, 1, lens, fac, n, p, None)
    assert combine(None, 2) == 1 and combine(p, 4) == 1 and b"holds 4" in lib.sdvar_last_error()
    assert lib.sdvar_gumbel_mix_rows(None, p, 2, 4, 0.0, 0.27, None, p, 2, 0, p, None) == 1          # no quantizer


def test_out_of_scope_paths_name_the_argument():
    for name, v in (("cfg", [1.5, 2.0]), ("top_k", (900, 0)), ("top_p", np.array([0.9, 0.5])), ("g_seed", torch.tensor([1, 2]))):
        with pytest.raises(E.SdvarError, match=name):
            E.scalar_arg("handoff", **{name: v})
    with pytest.raises(E.SdvarError, match="per-image seeds"):
        E.scalar_arg("resume_ar", noise=E.Noise("device", [1, 2]))
    E.scalar_arg("handoff", cfg=1.5, top_k=np.int64(3), top_p=torch.tensor(0.5), noise=E.Noise("host", 3, 1))


def test_committed_seeds_clear_the_golden_margin():
    """Every image of the GPU end-to-end test keeps MIN_MARGIN on its own oracle run (B = 1): no token may be excused on the GPU.  The committed seeds
    are the ones pick_seeds finds."""
    sd, sdv = state_dicts(RC.DEPTH, LADDER_256)
    m, q = orc.OracleVAR(sd, RC.DEPTH, LADDER_256), orc.OracleQuant(sdv, LADDER_256)
    for s in RC.SETS:
        assert min(RC.oracle_run(m, q, s).margins) >= RC.MIN_MARGIN, s
    assert RC.pick_seeds(m, q) == [s.seed for s in RC.SETS]
    assert any(s.top_k == 0 and s.top_p == 0.0 for s in RC.SETS) and len({(s.cfg, s.top_k, s.top_p, s.seed) for s in RC.SETS}) == 3
