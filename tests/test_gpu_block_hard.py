"""GPU: ln_modulate, qk_norm_append and sdvar_op_attention over the five KV-cache formats against the float64 references and per-element bars of
tests/block_hard_cases.py (bars and cases are checked on the CPU by test_block_hard_host.py).  Every kernel is called through the C ABI the way
test_gpu_ops.py calls it; caches for the attention cases are packed on the host, so an attention failure is the attention kernel's.  Nothing is filtered:
every output element of every case has a defined value.  Run with -s to see each case's worst err / tol (DESIGN.md section 4a quotes them)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import block_hard_cases as B
from conftest import rnd
from sdvar_amd import engine as E

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, off_elems=0):
    return C.c_void_p(t.data_ptr() + off_elems * t.element_size()) if t is not None else None


def _i32(vals):
    return (C.c_int32 * len(vals))(*vals)


def _unplanes(p, pfmt):
    """K-blocked operand planes (P, K/32, rows, 32) int16 on the CPU -> float64 (rows, K): the sum of the planes (bf16x3: pfmt 3, f16x2: pfmt 2)."""
    if pfmt == 3:
        v = sum((p[k].to(torch.int32) << 16).view(torch.float32).double() for k in range(3))
    else:
        v = sum(p[k].view(torch.float16).double() for k in range(2))
    return v.permute(1, 0, 2).reshape(v.shape[1], -1)


def _assert_bar(out, ref, tol, what):
    out = out.double()
    assert bool(torch.isfinite(out).all()), f"{what}: non-finite output"
    err = (out - ref).abs()
    r, i = B.worst(err, tol)
    idx = tuple(int(x) for x in np.unravel_index(i, tuple(ref.shape)))
    print(f"{what}: worst err / tol {r:.3f}")
    assert r <= 1.0, f"{what}: element {idx} got {float(out[idx])!r} want {float(ref[idx])!r}: err {float(err[idx]):.3e} = {r:.2f} x tol {float(tol[idx]):.3e}"
    return r


def _assert_planes(planes, pfmt, o32, what):
    """The operand-plane outputs against the fp32 output of the same call: bf16x3 planes equal its bits, f16x2 planes hold it (saturated at the fp16 range) to
    2^-21.9 relative or 2^-24.9 absolute."""
    got = _unplanes(planes.cpu(), pfmt)
    want = o32.double().view(got.shape)
    if pfmt == 3:
        assert torch.equal(got, want), f"{what}: bf16x3 planes differ from the fp32 output"
    else:
        want = want.clamp(-B.F16_MAX, B.F16_MAX)
        assert bool(((got - want).abs() <= B.f16x2_plane_tol(want)).all()), f"{what}: f16x2 planes off by {float(((got - want).abs() / B.f16x2_plane_tol(want)).max()):.2f} x the plane rule"


# ------------------------------------------------------------------------------------------------------------------ attention
def _attention(dev, c, fmt, kc, vc, pfmt=None, qbeg=None, vis=None):
    """One sdvar_op_attention call on device caches kc / vc: the fp32 output (R, l, H * 64), or with pfmt the operand planes.  Returns (rc, tensor)."""
    lib = E.load_library()
    q = c.q.to(dev)
    qbeg, vis = list(qbeg or c.qbeg), list(vis or c.vis)
    n = len(qbeg)
    M = c.R * c.l
    if pfmt is None:
        out = torch.empty(c.R, c.l, c.H * 64, device=dev)
        rc = lib.sdvar_op_attention(_p(q), _p(kc), _p(vc), fmt, _p(out), None, 0, 3, c.R, c.H, c.l, c.Lp, c.Ktot, n, _i32(qbeg), _i32(vis), _st())
    else:
        out = torch.zeros(pfmt, c.H * 2, M, 32, dtype=torch.int16, device=dev)
        rc = lib.sdvar_op_attention(_p(q), _p(kc), _p(vc), fmt, None, _p(out), M * c.H * 64, pfmt, c.R, c.H, c.l, c.Lp, c.Ktot, n, _i32(qbeg), _i32(vis), _st())
    torch.cuda.synchronize()
    return rc, out


def _caches(dev, c, fmt, stale=False):
    kc, vc = B.pack_cache(c, fmt, stale)
    return kc.to(dev).contiguous(), vc.to(dev).contiguous()


@pytest.mark.parametrize("fmt", B.FORMATS)
@pytest.mark.parametrize("name", B.HARD_ATTN + ("A6_stages16",))
def test_attention_hard_inputs(dev, name, fmt):
    """A1 diffuse tail, A2 staircases around the deferred maximum, A3 clamp scale, A4 V dynamic range, A6 the 16-stage table: fp32 output within the per-element bar,
    and (A1 - A4) both operand-plane outputs against it."""
    c = B.attn_case(name)
    kc, vc = _caches(dev, c, fmt)
    rc, out = _attention(dev, c, fmt, kc, vc)
    E._check(rc)
    ref, tol = B.attn_ref(name, fmt)
    _assert_bar(out.cpu(), ref, tol, f"attention {name} format {fmt}")
    if name in B.HARD_ATTN:
        for pfmt in (3, 2):
            rc, pl = _attention(dev, c, fmt, kc, vc, pfmt=pfmt)
            E._check(rc)
            _assert_planes(pl, pfmt, out.cpu(), f"attention {name} format {fmt} planes {pfmt}")


@pytest.mark.parametrize("fmt", B.FORMATS)
@pytest.mark.parametrize("name", B.STALE_ATTN)
def test_attention_ignores_a_stale_cache_tail(dev, name, fmt):
    """A5: the cursor was rolled back (sdvar_kv_set_len) and rows [Ktot, Lp) still hold the largest finite leftovers - +-65504 in every plane (formats 3, 4), +-3e38 in
    every plane (format 2); NaN for formats 0 and 1, which never read past Ktot.  The output is bit-identical to the one over a zero tail."""
    c = B.attn_case(name)
    outs = []
    for stale in (False, True):
        kc, vc = _caches(dev, c, fmt, stale)
        rc, out = _attention(dev, c, fmt, kc, vc)
        E._check(rc)
        outs.append(out.cpu())
    assert bool(torch.isfinite(outs[1]).all())
    assert torch.equal(outs[0], outs[1]), f"{name} format {fmt}: {int((outs[0] != outs[1]).sum())} elements depend on the rows past Ktot"
    ref, tol = B.attn_ref(name, fmt)
    _assert_bar(outs[1], ref, tol, f"attention {name} format {fmt} stale tail")


@pytest.mark.parametrize("fmt", B.FORMATS)
@pytest.mark.parametrize("name", B.EDGE_ATTN)
def test_attention_length_edges(dev, name, fmt):
    """A7: Ktot at the 32-key tile edge +-1, l at the 32-query wave, 128-query workgroup, 129-query kernel threshold and 256-query workgroup edges +-1; formats 3 and 4
    with l >= 129 (the 8-wave kernel) under every schedule."""
    lib = E.load_library()
    c = B.attn_case(name)
    kc, vc = _caches(dev, c, fmt)
    ref, tol = B.attn_ref(name, fmt)
    scheds = (-1, 0, 1, 2, 3) if (fmt >= 3 and c.l >= 129) else (-1,)
    try:
        for sched in scheds:
            if sched >= 0:
                E._check(lib.sdvar_debug_set_variant(b"attn_pp_sched", sched))
            rc, out = _attention(dev, c, fmt, kc, vc)
            E._check(rc)
            _assert_bar(out.cpu(), ref, tol, f"attention {name} format {fmt} sched {sched}")
    finally:
        E._check(lib.sdvar_debug_set_variant(b"attn_pp_sched", -1))


@pytest.mark.parametrize("fmt", B.FORMATS)
def test_attention_refuses_17_stages(dev, fmt):
    lib = E.load_library()
    c = B.attn_case("A6_stages16")
    kc, vc = _caches(dev, c, fmt)
    qbeg, vis = list(B.A6_QBEG) + [360], list(B.A6_VIS) + [400]
    rc, _ = _attention(dev, c, fmt, kc, vc, qbeg=qbeg, vis=vis)
    assert rc == 1 and b"stage" in lib.sdvar_last_error()                     # SDVAR_ERR_ARG, checked before any GPU call
    rc, _ = _attention(dev, c, fmt, kc, vc)                                   # ... and the 16 of the same table are taken
    E._check(rc)


def _kernel_names(fn):
    """Names of the GPU kernels launched by fn(), from torch's profiler (the library launches through the HIP runtime torch traces)."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if "attention" in e.name]


@pytest.mark.parametrize("fmt", [3, 4])
def test_attention_launch_path_at_the_129_query_threshold(dev, fmt):
    """Formats 3 and 4: 129 queries per (row, head) and more run attention_f16x2_pp_kernel (8 waves, 256 queries per workgroup), 128 and fewer the 4-wave
    attention_f16x2_kernel - so that the edge cases above cover the kernel they mean to cover."""
    for l, pp in ((128, False), (129, True), (257, True), (33, False)):
        c = B.attn_case(f"A7_l{l}")
        kc, vc = _caches(dev, c, fmt)
        _attention(dev, c, fmt, kc, vc)                                       # first use outside the trace (LDS opt-in, module load)
        names = _kernel_names(lambda: _attention(dev, c, fmt, kc, vc))
        assert len(names) >= 1, "the profiler recorded no attention kernel"
        assert all(("attention_f16x2_pp_kernel" in n) == pp for n in names) and all("attention_f16x2" in n for n in names), (l, names)


@pytest.mark.parametrize("fmt", [3, 4])
def test_v_beyond_fp16_saturates_in_the_cache(dev, fmt):
    """A |v| of 1e5 is appended as +-65504 in format 3 AND in format 4 (one fp16 plane: a bare cast would store inf, and 0 x inf would turn every query that
    MASKS that key into NaN).  The append saturates; attention over the saturated row matches the float64 reference on the saturated values."""
    lib = E.load_library()
    R, H, l, Lp = 1, 2, 8, 64
    NP = 2 if fmt == 3 else 1
    qkv = rnd(77, (R * l, 3 * H * 64))
    t = qkv.view(R, l, 3, H, 64)
    t[0, 5, 2, :, 3] = 1e5; t[0, 5, 2, :, 4] = -1e5; t[0, 6, 2, 0, 10] = 65504.0; t[0, 6, 2, 0, 11] = 65520.0
    sm = torch.full((H,), math.log(4.0), device=dev)
    qo = torch.zeros(R, H, l, 64, device=dev)
    kc = torch.zeros(R, H, NP, Lp, 64, dtype=torch.int16, device=dev); vc = torch.zeros_like(kc)
    qd = qkv.to(dev)
    E._check(lib.sdvar_op_qk_norm_append(_p(qd), _p(sm), _p(qo), _p(kc), _p(vc), fmt, R, l, H, Lp, 0, _st()))
    vbits = vc.cpu()
    vh = vbits.view(torch.float16)
    assert bool(torch.isfinite(vh.float()).all())
    assert bool((vh[0, :, 0, 5, 3] == 65504).all() and (vh[0, :, 0, 5, 4] == -65504).all()) and float(vh[0, 0, 0, 6, 10]) == 65504 and float(vh[0, 0, 0, 6, 11]) == 65504
    if fmt == 3:
        assert bool(((vbits[0, :, 1, 5, 3:5] & 0x7FFF) == 0).all())                # the low plane of a saturated value is zero
    q, k, v = B.qkv_split(qkv, R, l, H)
    c = B.AttnCase("vsat", qo.cpu(), B.cache_values(kc.cpu(), fmt)[:, :, :l].float(), v.clamp(-B.F16_MAX, B.F16_MAX), (0, 4), (4, 8))
    assert c.Lp == Lp
    rc, out = _attention(dev, c, fmt, kc, vc)                                  # queries 0 .. 3 mask key 5
    E._check(rc)
    ref, tol = B.attn_ref_of(c, fmt)
    _assert_bar(out.cpu(), ref, tol, f"attention over a saturated V row, format {fmt}")


# ------------------------------------------------------------------------------------------------------------------ LayerNorm + modulation
def _ln(dev, c, x=None, mod=None, pfmt=None):
    lib = E.load_library()
    xd, md = (c.x if x is None else x).to(dev), (c.mod if mod is None else mod).to(dev)
    Cw = c.C
    if pfmt is None:
        out = torch.empty(c.rows, Cw, device=dev)
        rc = lib.sdvar_op_ln_modulate(_p(xd), _p(md, 2 * Cw), _p(md, 4 * Cw), _p(out), None, 0, 3, c.rows, Cw, c.rpi, c.mod_stride, _st())
    else:
        out = torch.zeros(pfmt, Cw // 32, c.rows, 32, dtype=torch.int16, device=dev)
        rc = lib.sdvar_op_ln_modulate(_p(xd), _p(md, 2 * Cw), _p(md, 4 * Cw), None, _p(out), c.rows * Cw, pfmt, c.rows, Cw, c.rpi, c.mod_stride, _st())
    torch.cuda.synchronize()
    E._check(rc)
    return out.cpu()


@pytest.mark.parametrize("shape", B.LN_SHAPES, ids=lambda s: "C%d_r%d_i%d" % s[:3])
def test_ln_modulate_hard_rows(dev, shape):
    """All three instantiations (C <= 1024 / 2048 / 3072) at their upper edges, both lane maps (C % 8), partial last workgroups, every row family: within the
    per-element bar; constant rows, zero rows and scale == -1 give `shift` bit for bit; plane outputs (C % 32 == 0) against the fp32 output."""
    c = B.ln_case(*shape)
    out = _ln(dev, c)
    ref, tol, _ = B.ln_ref(c)
    _assert_bar(out, ref, tol, f"ln_modulate {c.name}")
    exact = B.ln_exact_mask(c)
    assert torch.equal(out[exact], c.shift[exact]), f"{c.name}: rows {[i for i in range(c.rows) if exact[i] and not torch.equal(out[i], c.shift[i])]} differ from shift"
    if c.planes:
        for pfmt in (3, 2):
            _assert_planes(_ln(dev, c, pfmt=pfmt), pfmt, out, f"ln_modulate {c.name} planes {pfmt}")


def test_ln_modulate_refuses_c_3076(dev):
    lib = E.load_library()
    x = torch.zeros(4, 3076, device=dev); mod = torch.zeros(1, 6 * 3076, device=dev); out = torch.empty_like(x)
    rc = lib.sdvar_op_ln_modulate(_p(x), _p(mod, 2 * 3076), _p(mod, 4 * 3076), _p(out), None, 0, 3, 4, 3076, 4, 6 * 3076, _st())
    assert rc == 1 and b"ln_modulate" in lib.sdvar_last_error()


@pytest.mark.parametrize("Cw", [1024, 2304])
def test_ln_modulate_planes_saturate_and_keep_nan(dev, Cw):
    """An output beyond +-65504 saturates in the f16x2 planes (and only there); a NaN input makes its own row NaN in every output and touches no other row.
    The output is pushed out of range by a shift of +-1e5: a 3e4 channel cannot do it, LayerNorm bounds |x - mean| / sigma by sqrt(C - 1) <= 56, which a scale of
    30 takes to 1.7e3 at most (the one3e4 rows under the +-30 groups of test_ln_modulate_hard_rows are that case, and stay finite in both plane formats)."""
    c = B.ln_case(Cw, 5, 5, 10, 0)                                               # five rows of five families, one group with a random scale
    x, mod = c.x.clone(), c.mod.clone()
    x[2, 17] = float("nan")
    mod[0, 4 * Cw + 100] = 1e5; mod[0, 4 * Cw + 101] = -1e5                      # shift: the output of these channels leaves the fp16 range in every row
    c2 = B.LnCase(c.name + "_sat", c.rows, Cw, c.rpi, torch.nan_to_num(x, nan=0.0), mod, c.row_family, c.group_family)
    out = _ln(dev, c2, x=x)
    good = [0, 1, 3, 4]
    assert bool(torch.isnan(out[2]).all()) and bool(torch.isfinite(out[good]).all())
    x_ok = x.clone(); x_ok[2] = c.x[2]
    ref_ok = _ln(dev, c2, x=x_ok)
    assert torch.equal(out[good], ref_ok[good])                                  # the NaN row touched no other row
    ref, tol, _ = B.ln_ref(B.LnCase(c2.name, c.rows, Cw, c.rpi, x_ok, mod, c.row_family, c.group_family))
    _assert_bar(ref_ok, ref, tol, f"ln_modulate {c2.name}")
    assert float(ref_ok[:, 100].min()) > 9e4 and float(ref_ok[:, 101].max()) < -9e4
    for pfmt in (3, 2):
        pl = _unplanes(_ln(dev, c2, x=x, pfmt=pfmt), pfmt)
        assert bool(torch.isnan(pl[2]).all()) and bool(torch.isfinite(pl[good]).all())
        if pfmt == 3:
            assert torch.equal(pl[good], out[good].double())
        else:
            want = out[good].double().clamp(-B.F16_MAX, B.F16_MAX)
            assert bool((pl[good][:, 100] == B.F16_MAX).all() and (pl[good][:, 101] == -B.F16_MAX).all())
            assert bool(((pl[good] - want).abs() <= B.f16x2_plane_tol(want)).all())


# ------------------------------------------------------------------------------------------------------------------ QK-norm append
def _append(dev, fmt, qkv, sm, kc, vc, R, l, H, Lp, pos0):
    lib = E.load_library()
    qd = qkv.to(dev)
    smd = sm.to(dev) if sm is not None else None
    qo = torch.full((R, H, l, 64), float("nan"), device=dev)
    E._check(lib.sdvar_op_qk_norm_append(_p(qd), _p(smd), _p(qo), _p(kc), _p(vc), fmt, R, l, H, Lp, pos0, _st()))
    torch.cuda.synchronize()
    return qo.cpu()


def _check_append(dev, fmt, qkv, sm, caches, caches0, R, l, H, Lp, pos0, what):
    """One append into the format-`fmt` device caches (and the same append into format-0 companions): q and the written window against
    the float64 reference by the format's rule, every bit outside the window unchanged.  Returns the number of fp16 elements that differ by one ulp."""
    before = B.decode_cache(caches[0].cpu(), caches[1].cpu(), fmt)
    qo = _append(dev, fmt, qkv, sm, caches[0], caches[1], R, l, H, Lp, pos0)
    after = B.decode_cache(caches[0].cpu(), caches[1].cpu(), fmt)
    for b, a, nm in zip(before, after, "KV"):
        assert torch.equal(b[..., :pos0, :], a[..., :pos0, :]), f"{what}: {nm} rows before position {pos0} changed"
        assert torch.equal(b[..., pos0 + l:, :], a[..., pos0 + l:, :]), f"{what}: {nm} rows from position {pos0 + l} on changed"
    qn, kn, vv, mag = B.qk_ref(qkv, sm, R, l, H)
    q32, k32, v32 = B.qkv_split(qkv, R, l, H)
    assert bool(torch.isfinite(qo).all())
    if sm is None:
        assert torch.equal(qo.double(), qn)                                      # q * 2^-5 is exact
    else:
        assert bool(((qo.double() - qn).abs() <= 2e-5 * mag).all()), f"{what}: q off by {float(((qo.double() - qn).abs() / (2e-5 * mag).clamp_min(1e-300)).max()):.2f} x the bar"
    win = slice(pos0, pos0 + l)
    Kw, Vw = after[0][..., win, :], after[1][..., win, :]
    Kv, Vv = B.cache_values(Kw, fmt), B.cache_values(Vw, fmt)
    assert bool(torch.isfinite(Kv).all() and torch.isfinite(Vv).all())
    ulps = 0
    if fmt == 0:
        if sm is None:
            assert torch.equal(Kv, kn)
        else:
            assert bool(((Kv - kn).abs() <= 2e-5 * kn.norm(dim=-1, keepdim=True)).all())
        assert torch.equal(Vv, vv)
    elif fmt in (1, 4):
        kh = B.k_norm_fp32(qkv, sm, R, l, H).half().view(torch.int16).to(torch.int32)
        d = (Kw[:, :, 0].to(torch.int32) - kh).abs()
        assert int(d.max()) <= 1, f"{what}: K differs from .half() of the fp32-normalised k by more than one fp16 ulp"
        ulps = int((d > 0).sum())
        if sm is None:
            assert ulps == 0
        assert torch.equal(Vw[:, :, 0], v32.clamp(-B.F16_MAX, B.F16_MAX).half().view(torch.int16))
    if fmt != 0:
        qo0 = _append(dev, 0, qkv, sm, caches0[0], caches0[1], R, l, H, Lp, pos0)
        assert torch.equal(qo, qo0), f"{what}: q differs from the format-0 kernel's"          # one normalisation, whatever the cache format
        K0, V0 = caches0[0].cpu()[:, :, win].double(), caches0[1].cpu()[:, :, win].double()
        if fmt in (1, 4):
            assert torch.equal(Kw[:, :, 0], K0.float().half().view(torch.int16)), f"{what}: K is not the fp16 rounding of the format-0 kernel's k"
        elif fmt == 2:
            assert torch.equal(Kv, K0) and torch.equal(Vv, V0), f"{what}: the bf16x3 planes do not sum to the format-0 bits"
        else:
            assert bool(((Kv - K0).abs() <= B.f16x2_plane_tol(K0)).all() and ((Vv - V0).abs() <= B.f16x2_plane_tol(V0)).all())
    return ulps


def _device_caches(dev, fmt, R, H, Lp, seed):
    kc, vc = B.empty_cache(fmt, R, H, Lp, seed)
    return kc.to(dev).contiguous(), vc.to(dev).contiguous()


@pytest.mark.parametrize("fmt", B.FORMATS)
def test_qk_norm_append_sampler_pattern(dev, fmt):
    """The sampler's ten appends at the ladder's cursor positions, then a rejected round: stages 6 and 7 appended again with new data over the old rows.  After every call
    the window holds the new values and every other bit of the cache - live neighbours, leftovers past the cursor, the other keys of a partly overwritten 16-key
    block of format 2's permuted V^T - is what it was."""
    R, H, Lp = 2, 3, B.SAMPLER_LP
    sm = torch.tensor([B.LN100_F32, 6.0, -0.7])
    caches = _device_caches(dev, fmt, R, H, Lp, 900)
    caches0 = _device_caches(dev, 0, R, H, Lp, 910) if fmt != 0 else None
    calls = list(range(10)) + list(B.SAMPLER_REDO)
    ulps = n = 0
    for i, j in enumerate(calls):
        l, pos0 = B.SAMPLER_LENS[j], B.SAMPLER_POS0[j]
        qkv = rnd(920 + i, (R * l, 3 * H * 64))
        ulps += _check_append(dev, fmt, qkv, sm, caches, caches0, R, l, H, Lp, pos0, f"append {i} (stage {j}) format {fmt}")
        n += R * l * H * 64
    assert ulps <= 1e-3 * n, (ulps, n)


@pytest.mark.parametrize("l2", [True, False], ids=["l2norm", "raw"])
@pytest.mark.parametrize("fmt", B.FORMATS)
@pytest.mark.parametrize("R,l,H,pos0", [(3, 37, 5, 31), (3, 37, 5, 33), (2, 33, 3, 63)])
def test_qk_norm_append_edge_vectors(dev, R, l, H, pos0, fmt, l2):
    """scale_mul exactly at ln 100, above it, at 0 and negative - and NULL (attn_l2_norm = False: q * 2^-5 exactly, k raw); all-zero q and k on the same (row, head)
    (zeros, no NaN), one-hot vectors, magnitudes of 1e-15 and 1e15, a v channel at 6e4; R l H not a multiple of 4, l not a multiple of 32, pos0 next to a multiple of 32."""
    Lp = 128
    sm = torch.tensor([B.LN100_F32, 6.0, 0.0, -2.0, 1.0][-H:]) if l2 else None
    qkv = B.qk_edge_inputs(1000 + pos0, R, l, H, extremes=l2)
    caches = _device_caches(dev, fmt, R, H, Lp, 930)
    caches0 = _device_caches(dev, 0, R, H, Lp, 940) if fmt != 0 else None
    ulps = _check_append(dev, fmt, qkv, sm, caches, caches0, R, l, H, Lp, pos0, f"edge append format {fmt}")
    assert ulps <= 1e-3 * R * l * H * 64, ulps
    after = B.decode_cache(caches[0].cpu(), caches[1].cpu(), fmt)
    Kv = B.cache_values(after[0][..., pos0:pos0 + l, :], fmt)
    assert bool((Kv[:, 0, 0] == 0).all())                                        # the all-zero k: zeros in the cache
