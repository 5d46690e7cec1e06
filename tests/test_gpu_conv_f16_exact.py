"""GPU: the one-product convolution format (plane_format 6: f16x2 planes, X plane 0 times W plane 0 and nothing else) on inputs with ONE right answer - the
counterpart of test_gpu_conv_exact.py for conv_f16x2_kernel<EPI, 2, 1> and conv_f16x2_reuse_kernel<EPI, TW, 1>.  Premises: test_conv_f16_host.py.

Everything goes through sdvar_op_conv_planes_ex.  The operands are those of test_gpu_conv_exact.operands (the library's own producers under format 2, held to the
host model word for word), copied, and then EVERY word of X plane 1 and W plane 1 is overwritten with an fp16 NaN: a kernel that brings plane 1 into a product
returns NaN.  'int' cases must equal the float64 conv2d bit for bit; 'dense' and 'sparse' cases the plane-0-only reference (conv_f16_cases.hh_ref), which differs
from the three-product one on 30 - 99 % of the outputs - what fails if hl or lh survives, if a plane or tap is mis-indexed, or if a counted s_waitcnt lets a
K-step be read before it landed.  Canaries, guard rows and the asserted plan are those of test_gpu_conv_exact.py."""
import ctypes as C

import pytest
import torch

import conv_exact_cases as X
import conv_f16_cases as H
from sdvar_amd import engine as E
from test_gpu_conv_exact import BACK, CANARY, FILL64, FRONT, _first, _p, _plan, _rows, _set, _st, _untouched, operands
from test_gpu_vae_kernels import BAR, normalised_err

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

INT_CASES = H.int_cases()
SPLIT_CASES = H.split_plane_cases()
_OPS, _REFS = {}, {}


def operands_hh(lib, c, dev):
    """the format-2 operands of the case, as copies whose plane 1 (X: guards and frame included; W: all four phase sets) holds NaN in every word"""
    if c.id not in _OPS:
        o = dict(operands(lib, c, 2, dev))
        xp, wp = o["xp"].clone(), o["wp"].clone()
        xp[1] = X.HALF_FILL
        if c.up:
            wp[:, 1] = X.HALF_FILL                        # [phase][plane][...]
        else:
            wp[1] = X.HALF_FILL
        o.update(xp=xp, wp=wp, xp0=xp.clone(), wp0=wp.clone())
        _OPS[c.id] = o
    return _OPS[c.id]


def reference(c, res, dev):
    key = (c.id, res)
    if key not in _REFS:
        r64 = c.ref(2, res) if c.kind == "int" else H.hh_ref(c, res)
        r32 = _rows(r64).float()
        assert torch.equal(r32.double(), _rows(r64))
        _REFS[key] = (r32.to(dev), r64)
    return _REFS[key]


def run_conv(lib, c, dev, reuse=1, res=False, force_split=0, auto_ws=False, gn=True):
    """One format-6 launch inside canaries; asserts result, path, guards and returns the plan quadruple."""
    o = operands_hh(lib, c, dev)
    ref32, ref64 = reference(c, res, dev)
    M, Mo, N = c.M, c.Mo, c.N
    nkt = c.taps * (c.Cin // 32)
    what = f"{c.id} format 6 tap_reuse {reuse} res {int(res)} force_split {force_split}{' auto split' if auto_ws else ''}{'' if gn else ' no gn'}"

    out = torch.full((FRONT + Mo + BACK, N), X.INT_FILL, dtype=torch.int32, device=dev)
    ws_floats = (force_split if force_split > 0 else 16) * M * N if (force_split > 0 or auto_ws) else 0
    ws = torch.full((ws_floats + CANARY,), X.INT_FILL, dtype=torch.int32, device=dev) if ws_floats else None
    npart = c.B * ((c.Hk * c.Wk) // 256) * 64 * (4 if c.up else 1)
    part = torch.full((npart + CANARY,), FILL64, dtype=torch.int64, device=dev) if gn else None
    stats = torch.full((c.B * 64 + CANARY,), X.INT_FILL, dtype=torch.int32, device=dev) if gn else None
    done = C.c_int32(-1)
    outp = C.c_void_p(out.data_ptr() + FRONT * N * 4)
    E._check(lib.sdvar_op_conv_planes_ex(_p(o["xp"]), o["xps"], o["R"], o["G"], _p(o["wp"]), o["wps"], H.PF_HH, _p(o["wsc"]), _p(o["bias"]), _p(o["res"]) if res else None,
                                         outp, c.B, c.Hk, c.Wk, N, c.Cin, c.taps, _p(ws), ws_floats, force_split, 0 if c.up else -1, o["wstride"], _p(part), _p(stats),
                                         C.byref(done) if gn else None, _st()))
    torch.cuda.synchronize()
    plan, took = _plan(lib)

    # ---- the path: kernel 3 (per-tap) or 4 (tap-reuse, the header's rule), "conv_pp" reported as 2 whatever it is set to
    if c.up or not (force_split > 0 or auto_ws):
        split = 1
    elif force_split > 0:
        split = X.expected_slices(force_split, nkt)
    else:
        split = plan[2]
        assert 1 <= split <= 16 and split == X.expected_slices(split, nkt), f"{what}: reported split {split}"
    kern = H.expected_kernel(c, reuse, split)
    fused = bool(gn) and X.stats_fuse(c, split)
    want_plan = [kern, 2, split, int(fused)]
    assert plan == want_plan and took == int(kern == 4), f"{what}: ran {plan} (tap reuse {took}), must run {want_plan}"
    assert not gn or done.value == int(fused), f"{what}: gn_done {done.value}"

    # ---- the result, bit for bit, and the rows around it
    got = out[FRONT:FRONT + Mo].view(torch.float32)
    if not torch.equal(got, ref32):
        bad = (got != ref32) | torch.isnan(got)
        m, n = _first(bad)
        b, rem = divmod(m, c.Ho * c.Wo)
        y, x = divmod(rem, c.Wo)
        unwritten = int(out[FRONT + m, n]) == X.INT_FILL
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} outputs differ; first at (image {b}, row {y}, column {x}, channel {n}): got {got[m, n].item()!r}"
                             f"{' (the fill pattern: never written)' if unwritten else ''}, exact {ref32[m, n].item()!r}")
    for lo, hi, name in ((0, FRONT, "before"), (FRONT + Mo, FRONT + Mo + BACK, "behind")):
        bad = out[lo:hi] != X.INT_FILL
        if bool(bad.any()):
            r, n = _first(bad)
            raise AssertionError(f"{what}: {int(bad.sum())} word(s) stored {name} the result; first at output row {lo + r - FRONT} (M = {Mo}), channel {n}")

    # ---- workspace, statistics, residual, operands
    if ws is not None:
        used = split * M * N if split > 1 else 0
        _untouched(ws, X.INT_FILL, used, ws.numel(), f"{what}: split-K workspace behind {split} slab(s)")
        holes = ws[:used] == X.INT_FILL
        assert not bool(holes.any()), f"{what}: {int(holes.sum())} workspace word(s) of the {split} slabs never written; first at {_first(holes)[0]}"
    if gn:
        if fused:
            _untouched(part, FILL64, npart, part.numel(), f"{what}: gn_part")
            holes = part[:npart] == FILL64
            assert not bool(holes.any()), f"{what}: {int(holes.sum())} gn_part double(s) never written; first at {_first(holes)[0]}"
            _untouched(stats, X.INT_FILL, c.B * 64, stats.numel(), f"{what}: stats")
            serr = normalised_err(ref64, stats[:c.B * 64].view(torch.float32).view(c.B, 32, 2))
            assert serr <= BAR, f"{what}: fused GroupNorm statistics off by {serr:.3e} (bar {BAR})"
        else:
            _untouched(part, FILL64, 0, part.numel(), f"{what}: gn_part (statistics not fused)")
            _untouched(stats, X.INT_FILL, 0, stats.numel(), f"{what}: stats (gn_done == 0)")
    if res:
        assert torch.equal(o["res"], o["res0"]), f"{what}: the residual was modified"
    assert torch.equal(o["xp"], o["xp0"]) and torch.equal(o["wp"], o["wp0"]), f"{what}: an operand plane was modified"
    return plan


def run_all_forms(lib, c, dev, pp=None):
    """tap reuse 1 and 0, with and without the residual, unsplit and with forced splits 2 and 3 where K allows, and - where the statistics fuse - once without gn_part"""
    nkt = c.taps * (c.Cin // 32)
    plans = []
    try:
        for reuse in (1, 0):
            _set(lib, pp, reuse)
            for res in ((False, True) if c.res is not None else (False,)):
                plans.append(run_conv(lib, c, dev, reuse, res))
                if not c.up:
                    for fs in (2, 3):
                        if fs <= nkt:
                            plans.append(run_conv(lib, c, dev, reuse, res, force_split=fs))
            if X.stats_fuse(c, 1):
                plans.append(run_conv(lib, c, dev, reuse, False, gn=False))
    finally:
        _set(lib, None, -1)
    return plans


@pytest.mark.parametrize("c", INT_CASES, ids=lambda c: c.id)
def test_conv_f16_exact_integers(dev, c):
    plans = run_all_forms(E.load_library(), c, dev)
    print(f"{c.id} format 6: {len(plans)} launches exact; plans {sorted(set(map(tuple, plans)))}")


@pytest.mark.parametrize("c", SPLIT_CASES, ids=lambda c: c.id)
def test_conv_f16_plane0_only(dev, c):
    plans = run_all_forms(E.load_library(), c, dev)
    print(f"{c.id} format 6: {len(plans)} launches equal the plane-0 product; plans {sorted(set(map(tuple, plans)))}")


def test_conv_f16_ignores_conv_pp(dev):
    """There are no one-product forms of loops 0 and 1: "conv_pp" 0 and 1 run kernel 3 / 4 all the same (asserted through the plan)"""
    lib = E.load_library()
    for pp in (0, 1):
        for c in (X.case("int", None, 3, 6, 7, 96, 160, 9, "prep"), X.case("int", None, 1, 2, 128, 64, 160, 4, "prep")):
            run_all_forms(lib, c, dev, pp=pp)


def test_conv_f16_chosen_split(dev):
    """conv_choose_split with the one-product K-step cost: Cin = 640 on one tile must come out split, exactly that many slabs written"""
    lib = E.load_library()
    c = X.case("int", None, 1, 3, 5, 640, 32, 9, "prep")
    for res in (False, True):
        plan = run_conv(lib, c, dev, 1, res, auto_ws=True)
        assert plan[0] == 3 and plan[2] > 1, plan


def test_conv_f16_n_not_multiple_of_4(dev):
    """N = 90: an argument error before anything is launched"""
    lib = E.load_library()
    c = X.case("int", None, 1, 5, 9, 64, 90, 9, "prep")
    o = operands(lib, c, 2, dev)
    out = torch.full((c.Mo + BACK, c.N), X.INT_FILL, dtype=torch.int32, device=dev)
    rc = lib.sdvar_op_conv_planes_ex(_p(o["xp"]), o["xps"], o["R"], o["G"], _p(o["wp"]), o["wps"], H.PF_HH, _p(o["wsc"]), _p(o["bias"]), None, _p(out), c.B, c.Hk, c.Wk, c.N,
                                     c.Cin, c.taps, None, 0, 0, -1, 0, None, None, None, _st())
    torch.cuda.synchronize()
    msg = lib.sdvar_last_error().decode()
    assert rc != 0 and "N % 4" in msg and "N=90" in msg, (rc, msg)
    assert bool((out == X.INT_FILL).all())
    rc = lib.sdvar_op_conv_planes(_p(o["xp"]), o["xps"], o["R"], o["G"], _p(o["wp"]), o["wps"], H.PF_HH, _p(o["wsc"]), _p(o["bias"]), None, _p(out), c.B, c.Hk, c.Wk, c.N,
                                  c.Cin, c.taps, None, 0, 0, _st())
    assert rc != 0 and bool((out == X.INT_FILL).all())
