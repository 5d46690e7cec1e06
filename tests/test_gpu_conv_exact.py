"""GPU: every convolution kernel of csrc/conv.hip on inputs with ONE right answer (tests/conv_exact_cases.py; premises proved without a GPU in
test_conv_exact_host.py) - the counterpart of test_gpu_gemm_exact.py for the conv family.

Exact: 'int' cases must equal the float64 conv2d bit for bit in every variant - bf16x3, and f16x2 with "conv_pp" 0, 1, 2 and the tap-reuse loop on and off - for
every tile tail, K split (forced 2, 3, 4 and chosen), residual, tap set and producer.  'dense' and 'sparse' cases put data into the low planes and must equal the
float64 sum of the plane products the kernels form.  No tolerance anywhere except the fused GroupNorm statistics, which stay under the project's bar of 2e-5
(test_gpu_vae_kernels.normalised_err) against fp64 statistics of the exact output.

Producers: the planes come from the library's own producers (sdvar_op_vae_prep up 0 / 1, sdvar_op_vae_s2d_planes + _s2d_weights, sdvar_op_vae_img_planes,
sdvar_op_conv_weight_planes, sdvar_op_upconv_weights) and are read back and held to the host model word for word BEFORE the convolution runs: a producer's fault is
reported as the producer's.

Canaries: the output sits between FRONT and BACK (>= 256: a tail tile has up to 255 dead rows) guard rows of INT_FILL and is pre-filled with it (a never-written
element is a NaN); the split-K workspace, gn_part and stats each have a canary block behind their documented size and must be untouched where they are not used;
the residual must be unchanged.  Both guard regions of every x plane and channel block are overwritten with HALF_FILL (an fp16 NaN, a 2^125-sized bf16) after the
producer ran: by the layout argument of conv.hip a stored output reads the one-pixel frame at most and tail rows are clamped to M - 1, so nothing may change.

Path: every run asserts sdvar_debug_get_conv_plan = {kernel, conv_pp used, K split used, statistics fused} against the rules of include/sdvar_hip.h."""
import ctypes as C

import pytest
import torch

import conv_exact_cases as X
from sdvar_amd import engine as E
from test_gpu_vae_kernels import BAR, normalised_err

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

VARIANTS = [(3, None), (2, 0), (2, 1), (2, 2)]          # (plane format, f16x2 K loop "conv_pp")
VIDS = ["bf16x3", "f16x2_pp0", "f16x2_pp1", "f16x2_pp2"]
FRONT, BACK = 16, 256                                    # guard rows of the output
CANARY = 1024                                            # canary words behind the workspace, gn_part and stats
FILL64 = (X.INT_FILL << 32) | X.INT_FILL                 # gn_part (doubles): a NaN as well
INT_CASES = X.int_cases()
SPLIT_CASES = [(c, v) for v in VARIANTS for c in X.split_plane_cases(v[0])]


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _rows(t):
    """(B, C, H, W) -> channel-last rows [B H W][C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def _first(bad):
    return tuple(bad.nonzero()[0].tolist())


# ------------------------------------------------------------------------------------------------------------------------ operands through the library's producers
_OPS, _REFS = {}, {}


def _same_words(got, want, what):
    got = got.cpu()
    if not torch.equal(got, want):
        bad = got != want
        i = _first(bad)
        raise AssertionError(f"PRODUCER {what}: {int(bad.sum())} of {bad.numel()} words differ from the host model; first at {i}: got {int(got[i]) & 0xFFFF:#06x}, "
                             f"want {int(want[i]) & 0xFFFF:#06x}")


def operands(lib, c, pf, dev):
    """x planes, w planes, scale, bias, res of a case in plane format pf, built once by the library's producers and checked against the host model."""
    key = (c.id, pf)
    if key in _OPS:
        return _OPS[key]
    npl, cb = X.NPL[pf], c.Cin // 32
    G = X.guard_rows(c.Wk)
    Mp = c.B * (c.Hk + 2) * (c.Wk + 2)
    R = Mp + 2 * G
    xps = cb * R * 32
    xp = torch.full((npl, cb, R, 32), X.HALF_FILL, dtype=torch.int16, device=dev)
    if c.src in ("prep", "prep_up"):
        xr = _rows(c.x_in).to(dev)
        E._check(lib.sdvar_op_vae_prep(_p(xr), None, None, None, _p(xp), xps, pf, c.B, c.Cin, c.H, c.W, 1 if c.src == "prep_up" else 0, 0, G, _st()))
    elif c.src == "s2d":
        xr = _rows(c.x_in).to(dev)
        E._check(lib.sdvar_op_vae_s2d_planes(_p(xr), _p(xp), xps, pf, c.B, c.Cin // 4, 2 * c.H, 2 * c.W, G, _st()))
    else:
        xr = c.x_in.contiguous().to(dev)
        E._check(lib.sdvar_op_vae_img_planes(_p(xr), _p(xp), xps, pf, c.B, c.H, c.W, G, _st()))
    torch.cuda.synchronize()
    _same_words(xp, X.x_plane_words(c.x_planes(pf), pf, G), f"x planes ({c.src}, format {pf}) of {c.id} [plane, channel block, row, channel]")
    xp[:, :, :G] = X.HALF_FILL                            # both guard regions of every plane and channel block
    xp[:, :, G + Mp:] = X.HALF_FILL

    S = c.scale(pf)
    wsc = torch.zeros(4, device=dev) if pf == 2 else None
    wplanes = c.w_planes(pf)
    if c.up:
        wps = 4 * c.Cin * c.N
        weff = torch.zeros(4, c.N, c.Cin, 4, device=dev)
        wd = c.w.contiguous().to(dev)
        E._check(lib.sdvar_op_upconv_weights(_p(wd), _p(weff), c.N, c.Cin, _st()))
        torch.cuda.synchronize()
        assert torch.equal(weff.cpu(), c.weff.reshape(4, c.N, c.Cin, 4)), f"PRODUCER sdvar_op_upconv_weights of {c.id}: phase weights differ from the host model"
        wp = torch.zeros(4, npl, wps, dtype=torch.int16, device=dev)
        if pf == 2:                                       # one scale over all four phases, as the decoder's binder takes it
            tmp = torch.zeros(2, 16 * c.N * c.Cin, dtype=torch.int16, device=dev)
            E._check(lib.sdvar_op_split_planes_f16(_p(weff), _p(tmp), 16 * c.N, c.Cin, 16 * c.N * c.Cin, _p(wsc), _st()))
            weff = (weff * wsc[0]).contiguous()
        for ph in range(4):
            E._check(lib.sdvar_op_conv_weight_planes(_p(weff[ph]), _p(wp[ph]), c.N, c.Cin, 4, wps, pf, None, _st()))
        torch.cuda.synchronize()
        for ph in range(4):
            want = X.w_plane_words([q[ph * c.N:(ph + 1) * c.N] for q in wplanes], pf)
            _same_words(wp[ph].view(npl, 4 * cb, c.N, 32), want, f"w planes of phase {ph} (format {pf}) of {c.id} [plane, K block, cout, k]")
        wstride = npl * wps
    else:
        wps = c.taps * c.Cin * c.N
        if c.src == "s2d":
            w_in = c.w_in.contiguous().to(dev)
            wd = torch.zeros(c.N, c.Cin, 3, 3, device=dev)
            E._check(lib.sdvar_op_vae_s2d_weights(_p(w_in), _p(wd), c.N, c.Cin // 4, _st()))
            torch.cuda.synchronize()
            assert torch.equal(wd.cpu(), c.w), f"PRODUCER sdvar_op_vae_s2d_weights of {c.id}: weights differ from the host model"
        else:
            wd = c.w.contiguous().to(dev)
        wp = torch.zeros(npl, c.taps * cb, c.N, 32, dtype=torch.int16, device=dev)
        E._check(lib.sdvar_op_conv_weight_planes(_p(wd), _p(wp), c.N, c.Cin, c.taps, wps, pf, _p(wsc), _st()))
        torch.cuda.synchronize()
        _same_words(wp, X.w_plane_words(wplanes, pf), f"w planes (format {pf}) of {c.id} [plane, K block, cout, k]")
        wstride = 0
    if pf == 2:
        assert wsc[:2].tolist() == [S, 1.0 / S], f"PRODUCER weight scale of {c.id}: {wsc[:2].tolist()}, want {S}"
    res = _rows(c.res).to(dev) if c.res is not None else None
    o = dict(xp=xp, xps=xps, R=R, G=G, wp=wp, wps=wps, wstride=wstride, wsc=wsc, bias=c.bias.to(dev), res=res, res0=res.clone() if res is not None else None,
             xp0=xp.clone(), wp0=wp.clone())
    _OPS[key] = o
    return o


def reference(c, pf, res, dev):
    """(rows [B Ho Wo][N] float32 on the device, the same as float64 (B, N, Ho, Wo) on the CPU), cached"""
    key = (c.id, "int" if c.kind == "int" else pf, res)
    if key not in _REFS:
        r64 = c.ref(pf, res)
        r32 = _rows(r64).float()
        assert torch.equal(r32.double(), _rows(r64))
        _REFS[key] = (r32.to(dev), r64)
    return _REFS[key]


# ------------------------------------------------------------------------------------------------------------------------ one guarded launch
def _plan(lib):
    out4 = (C.c_int32 * 4)()
    E._check(lib.sdvar_debug_get_conv_plan(out4))
    took = C.c_int32(-1)
    E._check(lib.sdvar_debug_get_conv_cfg(C.byref(took)))
    return list(out4), took.value


def _untouched(buf, fill, lo, hi, what):
    bad = buf[lo:hi] != fill
    if bool(bad.any()):
        raise AssertionError(f"{what}: {int(bad.sum())} word(s) written that must stay untouched; first at offset {lo + _first(bad)[0]} (documented size {lo})")


def run_conv(lib, c, pf, pp, dev, reuse=1, res=False, force_split=0, auto_ws=False, gn=True):
    """One sdvar_op_conv_planes_ex launch of the case inside canaries; asserts everything and returns the plan quadruple."""
    o = operands(lib, c, pf, dev)
    ref32, ref64 = reference(c, pf, res, dev)
    M, Mo, N = c.M, c.Mo, c.N
    nkt = c.taps * (c.Cin // 32)
    what = f"{c.id} format {pf} conv_pp {pp} tap_reuse {reuse} res {int(res)} force_split {force_split}{' auto split' if auto_ws else ''}{'' if gn else ' no gn'}"

    out = torch.full((FRONT + Mo + BACK, N), X.INT_FILL, dtype=torch.int32, device=dev)
    ws_floats = (force_split if force_split > 0 else 16) * M * N if (force_split > 0 or auto_ws) else 0
    ws = torch.full((ws_floats + CANARY,), X.INT_FILL, dtype=torch.int32, device=dev) if ws_floats else None
    npart = c.B * ((c.Hk * c.Wk) // 256) * 64 * (4 if c.up else 1)
    part = torch.full((npart + CANARY,), FILL64, dtype=torch.int64, device=dev) if gn else None
    stats = torch.full((c.B * 64 + CANARY,), X.INT_FILL, dtype=torch.int32, device=dev) if gn else None
    done = C.c_int32(-1)
    outp = C.c_void_p(out.data_ptr() + FRONT * N * 4)
    E._check(lib.sdvar_op_conv_planes_ex(_p(o["xp"]), o["xps"], o["R"], o["G"], _p(o["wp"]), o["wps"], pf, _p(o["wsc"]), _p(o["bias"]), _p(o["res"]) if res else None, outp,
                                         c.B, c.Hk, c.Wk, N, c.Cin, c.taps, _p(ws), ws_floats, force_split, 0 if c.up else -1, o["wstride"], _p(part), _p(stats),
                                         C.byref(done) if gn else None, _st()))
    torch.cuda.synchronize()
    plan, took = _plan(lib)

    # ---- the path
    pp_used = 0 if pf == 3 else (1 if (pp == 2 and N % 4) else pp)
    if c.up or not (force_split > 0 or auto_ws):
        split = 1
    elif force_split > 0:
        split = X.expected_slices(force_split, nkt)
    else:                                                             # chosen by the library: what it reports must be a split it can have made; the workspace check below confirms it
        split = plan[2]
        assert 1 <= split <= 16 and split == X.expected_slices(split, nkt), f"{what}: reported split {split}"
    took_exp = X.tap_reuse_eligible(c, pf, pp_used, reuse, split)
    fused = bool(gn) and X.stats_fuse(c, split)
    want_plan = [0 if pf == 3 else 2 if took_exp else 1, pp_used, split, int(fused)]
    assert plan == want_plan and took == int(took_exp), f"{what}: ran {plan} (tap reuse {took}), must run {want_plan} (tap reuse {int(took_exp)})"
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


def _set(lib, pp, reuse):
    E._check(lib.sdvar_debug_set_variant(b"conv_pp", -1 if pp is None else pp))
    E._check(lib.sdvar_debug_set_variant(b"conv_tap_reuse", reuse))


def run_all_forms(lib, c, pf, pp, dev):
    """Every form of one case in one variant: tap reuse on / off where the shape is eligible, with and without the residual, unsplit, forced splits 2, 3, 4 (the
    ragged ones included: 9 cb K-steps over 2 or 4 slices, 5 over 3) and - where the statistics can fuse - once without gn_part."""
    nkt = c.taps * (c.Cin // 32)
    eligible = X.tap_reuse_eligible(c, pf, 0 if pf == 3 else pp, 1, 1)
    plans = []
    try:
        for reuse in ((1, 0) if eligible else (1,)):
            _set(lib, pp, reuse)
            for res in ((False, True) if c.res is not None else (False,)):
                plans.append(run_conv(lib, c, pf, pp, dev, reuse, res))
                if reuse == 1 and not c.up and c.N % 4 == 0:
                    for fs in (2, 3, 4):
                        if fs <= nkt:
                            plans.append(run_conv(lib, c, pf, pp, dev, reuse, res, force_split=fs))
            if X.stats_fuse(c, 1):
                plans.append(run_conv(lib, c, pf, pp, dev, reuse, False, gn=False))
    finally:
        _set(lib, None, -1)
    return plans


# ------------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("pf,pp", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("c", INT_CASES, ids=lambda c: c.id)
def test_conv_exact_integers(dev, c, pf, pp):
    """Exact-integer operands: the float64 conv2d, bit for bit, in every form (run_all_forms), inside canaries, on the asserted path."""
    plans = run_all_forms(E.load_library(), c, pf, pp, dev)
    print(f"{c.id} format {pf} conv_pp {pp}: {len(plans)} launches exact; plans {sorted(set(map(tuple, plans)))}")


@pytest.mark.parametrize("c,v", SPLIT_CASES, ids=lambda a: a.id if hasattr(a, "id") else VIDS[VARIANTS.index(a)])
def test_conv_exact_split_planes(dev, c, v):
    """The low planes carry data ('dense': f16x2; 'sparse': both formats): the float64 sum of exactly the plane products the kernels form (hh, hl, lh; the six of
    bf16x3), bit for bit, in every form."""
    pf, pp = v
    plans = run_all_forms(E.load_library(), c, pf, pp, dev)
    print(f"{c.id} format {pf} conv_pp {pp}: {len(plans)} launches exact; plans {sorted(set(map(tuple, plans)))}")


@pytest.mark.parametrize("pf,pp", VARIANTS, ids=VIDS)
def test_conv_chosen_split(dev, pf, pp):
    """A workspace and few tiles: conv_choose_split picks a K split itself (Cin = 640, one tile: 180 K-steps).  The reported split must be > 1 and exactly that many
    slabs of the workspace must have been written."""
    lib = E.load_library()
    c = X.case("int", None, 1, 3, 5, 640, 32, 9, "prep")
    try:
        _set(lib, pp, -1)
        for res in (False, True):
            plan = run_conv(lib, c, pf, pp, dev, 1, res, auto_ws=True)
            assert plan[2] > 1, plan
    finally:
        _set(lib, None, -1)


@pytest.mark.parametrize("pf,pp", VARIANTS, ids=VIDS)
def test_conv_n_not_multiple_of_4(dev, pf, pp):
    """N = 90: "conv_pp" 2 must fall back to 1 (asserted in run_conv through the plan), a split is never chosen even with a workspace, and a forced split is refused
    with an error before anything is launched: output and workspace stay untouched."""
    lib = E.load_library()
    c = X.case("int", None, 1, 5, 9, 64, 90, 9, "prep")
    try:
        _set(lib, pp, -1)
        plan = run_conv(lib, c, pf, pp, dev, 1, True, auto_ws=True)
        assert plan[1] == (0 if pf == 3 else 1 if pp == 2 else pp) and plan[2] == 1, plan
        o = operands(lib, c, pf, dev)
        out = torch.full((c.Mo + BACK, c.N), X.INT_FILL, dtype=torch.int32, device=dev)
        ws = torch.full((2 * c.M * c.N + CANARY,), X.INT_FILL, dtype=torch.int32, device=dev)
        rc = lib.sdvar_op_conv_planes_ex(_p(o["xp"]), o["xps"], o["R"], o["G"], _p(o["wp"]), o["wps"], pf, _p(o["wsc"]), _p(o["bias"]), None, _p(out), c.B, c.Hk, c.Wk, c.N,
                                         c.Cin, c.taps, _p(ws), 2 * c.M * c.N, 2, -1, 0, None, None, None, _st())
        torch.cuda.synchronize()
        assert rc != 0, "a forced K split with N % 4 != 0 must be refused"
        assert bool((out == X.INT_FILL).all()) and bool((ws == X.INT_FILL).all())
    finally:
        _set(lib, None, -1)


def test_tap_reuse_shapes_are_those_of_the_tap_reuse_tests():
    from test_gpu_conv_tap_reuse import CASES
    assert [(B, H, W, Cin, N, 4 if up else 9) for B, H, W, Cin, N, _, up, _ in CASES] == X.TAP_REUSE_SHAPES
    for (B, H, W, Cin, N, _, up, eligible), s in zip(CASES, X.TAP_REUSE_SHAPES):
        assert X.tap_reuse_eligible(X.case("int", None, *s, "prep"), 2, 2, 1, 1) == eligible
