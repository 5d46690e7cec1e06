"""The GEMM planner (csrc/gemm_plan.h) is a pure function of the shape, checkable without a GPU: sdvar_debug_plan_gemm must return, row for row, the plan recorded
in tests/golden/gemm_plan.json (produced by the per-file cost models this planner replaced: tests/golden/make_gemm_plan.py).  No tolerance, no skipped rows: every
output bit of a GEMM depends on the tile and K split chosen here."""
import ctypes
import importlib.util
import json
import os

from conftest import GOLDEN


def _rows():
    with open(os.path.join(GOLDEN, "gemm_plan.json")) as f:
        return json.load(f)


def test_fixture_covers_the_planner():
    rows = _rows()
    spec = importlib.util.spec_from_file_location("make_gemm_plan", os.path.join(GOLDEN, "make_gemm_plan.py"))
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    assert [tuple(r[:5]) for r in rows] == list(gen.cases())              # the whole table, in order
    assert {16, 32, 64, 128, 256, 512, 768} <= {r[5] for r in rows}
    assert any(r[7] > 0 for r in rows) and any(r[6] > 1 for r in rows) and any(r[8] == 1 for r in rows)
    for mode in (0, 1, 2):
        assert any(r[0] == mode and r[6] > 1 for r in rows)


def test_plan_equals_fixture():
    from sdvar_amd import engine as E
    lib = E.load_library()
    out = (ctypes.c_int32 * 4)()
    bad = []
    for r in _rows():
        E._check(lib.sdvar_debug_plan_gemm(*r[:5], out))
        if list(out) != r[5:]:
            bad.append((r, list(out)))
    assert not bad, (len(bad), bad[:10])


def test_plan_rejects_bad_arguments():
    from sdvar_amd import engine as E
    lib = E.load_library()
    out = (ctypes.c_int32 * 4)()
    assert lib.sdvar_debug_plan_gemm(3, 64, 128, 64, 4, out) == 1
    assert lib.sdvar_debug_plan_gemm(2, 64, 128, 48, 4, out) == 1 and b"K" in lib.sdvar_last_error()
    assert lib.sdvar_debug_plan_gemm(2, 64, 128, 64, 4, None) == 1
