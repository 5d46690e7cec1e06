"""No GPU: the planner's view of GEMM mode 'f16' (an f16x2 model with one flag, planned as mode 2 with flags bit 3: sdvar_debug_plan_gemm's `mode` 3 stays
rejected, as tests/test_gemm_plan_host.py requires) and the agreement of header, library and binding on sdvar_op_gemm_h_ex.  sdvar_debug_plan_gemm is pure host
code; the variant `h16_min_m` is a host-side switch (restored in a `finally`)."""
import ctypes
import json
import os
import re

import pytest

from conftest import GOLDEN, ROOT

SHAPES = [(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096), (2304, 768), (5760, 1920), (4096, 1920)]      # (N, K) of the block and head GEMMs at d16, d12, d30


def _plan(lib, mode, M, N, K, flags=7):
    from sdvar_amd import engine as E
    out = (ctypes.c_int32 * 4)()
    E._check(lib.sdvar_debug_plan_gemm(mode, M, N, K, flags, out))
    return list(out)


@pytest.mark.parametrize("thr", [None, 1, 48, 1024])
def test_f16_tier_plans_the_half_kernel_from_h16_min_m_rows(thr):
    from sdvar_amd import engine as E
    lib = E.load_library()
    try:
        if thr is not None:
            E.set_variant("h16_min_m", thr)
        t = 2704 if thr is None else thr                                  # the default, stated in DESIGN.md section 4
        for N, K in SHAPES:
            for M in sorted({1, 8, 36, 47, 48, 80, 256, 1023, 1024, 1600, 2703, 2704, 5440, t - 1, t, t + 1} - {0}):
                for flags in (0, 4, 5, 7):
                    got = _plan(lib, 2, M, N, K, flags | E.PLAN_FLAG_F16)
                    if M >= t:
                        assert got == [E.HALF_KERNEL_CODE, 1, 0, 0], (M, N, K, flags, got)
                    else:
                        assert got == _plan(lib, 2, M, N, K, flags) and got[0] != E.HALF_KERNEL_CODE, (M, N, K, flags, got)
    finally:
        E.set_variant("h16_min_m", -1)


def test_modes_0_to_2_replay_the_fixture_whatever_the_threshold():
    from sdvar_amd import engine as E
    lib = E.load_library()
    with open(os.path.join(GOLDEN, "gemm_plan.json")) as f:
        rows = json.load(f)
    try:
        E.set_variant("h16_min_m", 1)
        bad = [r for r in rows if _plan(lib, *r[:5]) != r[5:]]
    finally:
        E.set_variant("h16_min_m", -1)
    assert not bad, (len(bad), bad[:5])
    assert {r[0] for r in rows} == {0, 1, 2}


def test_variant_range_and_modes():
    from sdvar_amd import engine as E
    lib = E.load_library()
    assert lib.sdvar_debug_set_variant(b"h16_min_m", 0) == 1              # 0 rows is no threshold; < 0 = back to the default
    assert lib.sdvar_debug_set_variant(b"h16_min_m", -1) == 0
    out = (ctypes.c_int32 * 4)()
    assert lib.sdvar_debug_plan_gemm(3, 64, 128, 64, 4, out) == 1 and lib.sdvar_debug_plan_gemm(3, 4096, 128, 64, 4 | E.PLAN_FLAG_F16, out) == 1
    assert E.GEMM_MODES == ("f32", "bf16x3", "f16x2") and E.ENGINE_GEMM_MODES == E.GEMM_MODES + ("f16",)


def test_header_library_and_binding_agree_on_gemm_h_ex():
    from sdvar_amd import engine as E
    lib = E.load_library()
    with open(os.path.join(ROOT, "include", "sdvar_hip.h")) as f:
        hdr = f.read()
    m = re.search(r"int sdvar_op_gemm_h_ex\(([^;]*)\);", hdr)
    assert m, "sdvar_op_gemm_h_ex is not declared in include/sdvar_hip.h"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    names = [re.split(r"[\s\*]+", p)[-1] for p in params]
    assert names == ["x", "w", "dtype", "w_scale", "bias", "out", "ldo", "h_out", "pre_out", "res", "ldres", "gate", "rows_per_gate", "gate_stride", "M", "N", "K",
                     "epilogue", "stream"]
    res, args = E._SIGNATURES["sdvar_op_gemm_h_ex"]
    assert res is ctypes.c_int32 and len(args) == len(params)
    for p, a in zip(params, args):
        assert (a is ctypes.c_void_p) == ("*" in p) and (a is ctypes.c_int32) == p.startswith("int32_t"), (p, a)
    assert hasattr(lib, "sdvar_op_gemm_h_ex") and callable(E.gemm_h_ex)
    assert lib.sdvar_abi_version() == E.ABI_VERSION                        # additive: no ABI bump
    # argument errors need no device: they are reported before anything is launched
    assert lib.sdvar_op_gemm_h_ex(None, None, 1, None, None, None, 0, None, None, None, 0, None, 1, 0, 8, 8, 32, 0, None) == 1
