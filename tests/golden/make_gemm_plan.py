"""Regenerates tests/golden/gemm_plan.json: the GEMM planner's choice (kernel code, K split, hybrid tail split, QKV fused) over the table of shapes below,
one compact row [mode, M, N, K, flags, kernel, split, tail, fused] each.  Needs the built library, no GPU:

    python tests/golden/make_gemm_plan.py [path/to/libsdvar_hip.so]

The committed bytes were NOT produced by this tree's planner: they come from commit fd8cd9c (the last one with the per-file choose_cfg / choose_cfg_p /
choose_cfg_h and the decisions written out inside the three *_nt functions), built with a throw-away patch that exported those functions and the unchanged
post-processing of *_nt under this same entry point.  tests/test_gemm_plan_host.py holds sdvar_debug_plan_gemm against them row by row, so regenerate the file
only when a change of the plan is the point of the change.  Run with no SDVAR_* variable set."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
WIDTHS = (768, 1024, 1280, 1536, 1920)
VOCAB = 4096
ROWS = (1, 2, 8, 16, 18, 32, 50, 64, 72, 80, 81, 128, 144, 200, 256, 288, 400, 512, 513, 576, 800, 1024, 1352, 1600, 2048, 2704, 4096, 5440, 6800, 10880, 21760)
DEFER, QKV, VEC = 1, 2, 4          # flag bits of sdvar_debug_plan_gemm


def cases():
    """(mode, M, N, K, flags) in file order."""
    for mode in (0, 1, 2):
        for C in WIDTHS:
            for i, (N, K) in enumerate(((3 * C, C), (C, C), (4 * C, C), (C, 4 * C), (VOCAB, C))):
                flag_sets = [VEC, VEC | DEFER] + ([VEC | QKV, VEC | QKV | DEFER] if mode == 2 and i == 0 else [])
                for M in ROWS:
                    for flags in flag_sets:
                        yield mode, M, N, K, flags


def plan_rows(lib):
    lib.sdvar_debug_plan_gemm.restype = ctypes.c_int32
    lib.sdvar_debug_plan_gemm.argtypes = [ctypes.c_int32] * 5 + [ctypes.POINTER(ctypes.c_int32)]
    out = (ctypes.c_int32 * 4)()
    rows = []
    for case in cases():
        assert lib.sdvar_debug_plan_gemm(*case, out) == 0, case
        rows.append(list(case) + list(out))
    return rows


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "..", "..", "sdvar_amd", "csrc", "libsdvar_hip.so")
    rows = plan_rows(ctypes.CDLL(os.path.abspath(path)))
    with open(os.path.join(HERE, "gemm_plan.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")
    print(len(rows), "rows")


if __name__ == "__main__":
    main()
