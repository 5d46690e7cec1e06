"""Stage 0 from the per-class table (sdvar_stage_first / ModelCtx.forward_first, include/sdvar_hip.h): the table rows are made by the ordinary launch sequence in batches
of the call's R rows, so everything here is BIT equality - table on against "stage0_table" 0, and against place_first + forward(x, 0, 1).  A difference would mean that
some kernel's row result depends on the other rows of its call; that is a finding about that kernel, not something a tolerance may cover."""
from contextlib import contextmanager

import pytest
import torch

from conftest import rnd, state_dicts
from sdvar_amd import engine as E
from sdvar_amd.ladder import LADDER_256

pytestmark = pytest.mark.gpu
PNS = LADDER_256
NC = 1000
# every (GEMM mode, fp16 cache) a model context can be built with: cache formats fp32, fp16, bf16x3 planes, f16x2 planes and the one-plane fp16 cache of both plane modes
COMBOS = [("f32", False), ("f32", True), ("bf16x3", False), ("bf16x3", True), ("f16x2", False), ("f16x2", True)]
LABELS = {1: [[0], [NC - 1]], 3: [[NC - 1, 0, NC - 1]], 8: [[417] * 8, [0, 5, 5, NC - 1, 123, 0, 77, 500]]}
COMPUTE_CLASSES = ("gemm", "gemm_small", "ln_modulate", "attention", "attention_small", "qk_norm_append")

_CTX = {}


def _ctx(dev, depth, mode="f16x2", kv_fp16=False, shared_aln=False):
    key = (depth, mode, kv_fp16, shared_aln)
    if key not in _CTX:
        sd, _ = state_dicts(depth, PNS, vae=False, shared_aln=shared_aln)
        _CTX[key] = E.ModelCtx(sd, depth, PNS, 8, 2, dev, kv_fp16=kv_fp16, gemm_mode=mode)
    return _CTX[key]


def _set(name, value):
    E._check(E.load_library().sdvar_debug_set_variant(name, value))


@contextmanager
def _table(on):
    _set(b"stage0_table", 1 if on else 0)
    try:
        yield
    finally:
        _set(b"stage0_table", -1)


def _stage01(ctx, dev, labels=None, first=True, cond=None):
    """(stage-0 logits, logits of an ordinary stage-1 forward on fixed inputs) of one call; first: forward_first, else place_first + forward(x, 0, 1)."""
    f = dict(device=dev, dtype=torch.float32)
    if cond is not None:
        ctx.begin_cond(cond)
    else:
        ctx.begin(torch.tensor(labels, dtype=torch.int64, device=dev))
    R, V, C, l1 = ctx.R, ctx.V, ctx.Cw, ctx.lad.lens[1]
    lg0 = torch.full((R, 1, V), float("nan"), **f)
    if first:
        ctx.forward_first(lg0)
    else:
        x = torch.empty(R, 1, C, **f)
        ctx.place_first(x, 1)
        ctx.forward(x, 0, 1, lg0)
    assert ctx.kv_len() == 1
    x1 = rnd(7, (R, l1, C)).to(dev)
    lg1 = torch.full((R, l1, V), float("nan"), **f)
    ctx.forward(x1, 1, 1, lg1)
    ctx.kv_set_len(0)
    return lg0, lg1


def _same(a, b, what):
    for name, u, v in zip(("stage-0 logits", "stage-1 logits"), a, b):
        assert torch.isfinite(u).all() and torch.equal(u, v), f"{what}: {name} differ, max |d| = {(u - v).abs().max().item():.3e}"


def _launches(ctx, dev, labels, cond=None):
    """per-class launch counts of forward_first alone (the begin and its table build stay outside the profile)"""
    if cond is not None:
        ctx.begin_cond(cond)
    else:
        ctx.begin(torch.tensor(labels, dtype=torch.int64, device=dev))
    lg = torch.empty(ctx.R, 1, ctx.V, device=dev)
    E.prof_enable(True)
    try:
        ctx.forward_first(lg)
        p = E.prof_collect()
    finally:
        E.prof_enable(False)
        ctx.kv_set_len(0)
    return {k: v["launches"] for k, v in p.items()}


@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("mode,kv_fp16", COMBOS)
def test_table_equals_computed_bitwise(dev, depth, mode, kv_fp16):
    ctx = _ctx(dev, depth, mode, kv_fp16)
    for B in (1, 3, 8):
        for labels in LABELS[B]:
            with _table(False):
                off = _stage01(ctx, dev, labels)
                plain = _stage01(ctx, dev, labels, first=False)
            with _table(True):
                on = _stage01(ctx, dev, labels)
            _same(off, plain, f"{mode} fp16={kv_fp16} d{depth} B={B}: computed forward_first against place_first + forward")
            _same(on, off, f"{mode} fp16={kv_fp16} d{depth} B={B} labels={labels}: table against computed")


@pytest.mark.parametrize("mode,kv_fp16", [("f32", False), ("bf16x3", False), ("f16x2", False), ("f16x2", True)])
def test_table_hit_launches_nothing_but_the_copy(dev, mode, kv_fp16):
    ctx = _ctx(dev, 4, mode, kv_fp16)
    labels = [3, NC - 1, 3]
    with _table(True):
        n = _launches(ctx, dev, labels)
    assert all(n[c] == 0 for c in COMPUTE_CLASSES), n
    assert n["embed_misc"] == 1, n
    with _table(False):
        n = _launches(ctx, dev, labels)
    assert n["gemm_small"] >= 4 * 4 + 1 and n["attention_small"] == 4 and n["gemm"] == 0, n          # per block QKV, proj, fc1, fc2; the head


def _computes(n):
    return n["gemm_small"] > 0 and n["attention_small"] > 0


def test_fallbacks_compute_and_equal_the_plain_path(dev):
    ctx = _ctx(dev, 4)
    labels = [NC - 1, 0, 17]
    with _table(True):
        want = _stage01(ctx, dev, labels, first=False)
        # begin_cond with the very rows begin(labels) looks up (its adaLN parameters come from GEMMs over the call's rows, not from the per-class adaLN table,
        # so the reference is the plain path of a begin_cond call)
        sd, _ = state_dicts(4, PNS, vae=False)
        emb = sd["class_emb.weight"].float()
        cond = torch.cat([emb[labels], emb[[NC] * len(labels)]]).contiguous().to(dev)
        _same(_stage01(ctx, dev, cond=cond), _stage01(ctx, dev, cond=cond, first=False), "begin_cond")
        assert _computes(_launches(ctx, dev, None, cond=cond))
        # a cap of 0 MiB
        _set(b"stage0_table_mb", 0)
        try:
            _same(_stage01(ctx, dev, labels), want, "cap 0 MiB")
            assert _computes(_launches(ctx, dev, labels))
        finally:
            _set(b"stage0_table_mb", -1)
        assert not _computes(_launches(ctx, dev, labels))                      # and back on the table
        # the f16x2 guard counts the operand planes of the pass: it must run
        E.f16x2_guard(True)
        try:
            g_first = _stage01(ctx, dev, labels)
            g_plain = _stage01(ctx, dev, labels, first=False)
            assert _computes(_launches(ctx, dev, labels))
        finally:
            E.f16x2_guard(False)
        _same(g_first, g_plain, "f16x2 guard on")
        # a shared_aln model: its conditioning goes through one Linear per call, there is no per-class table
        sh = _ctx(dev, 4, shared_aln=True)
        _same(_stage01(sh, dev, labels), _stage01(sh, dev, labels, first=False), "shared_aln")
        assert _computes(_launches(sh, dev, labels))


def test_table_is_rebuilt_when_weights_switches_or_batch_change(dev):
    lib = E.load_library()
    sd, _ = state_dicts(4, PNS, vae=False)
    ctx = E.ModelCtx(sd, 4, PNS, 8, 2, dev)           # its own context: the weights are re-bound below
    labels = [5, NC - 1, 5]

    def check(what, lab=labels):
        with _table(True):
            on = _stage01(ctx, dev, lab)
            assert not _computes(_launches(ctx, dev, lab)), what
        with _table(False):
            off = _stage01(ctx, dev, lab, first=False)
        _same(on, off, what)
        return on

    base = check("first build")
    # one block's weights change
    sd2 = dict(sd)
    for k in ("blocks.1.attn.mat_qkv.weight", "blocks.1.ffn.fc2.bias"):
        sd2[k] = sd[k] * 1.25
    ctx.bind(sd2)
    moved = check("after re-binding block 1")
    assert not torch.equal(moved[0], base[0]), "the re-bound weights did not change stage 0: the test checks nothing"
    ctx.bind(sd)
    _same(check("after binding the first weights again"), base, "first weights again")
    # a variant switch and a forced tile: whatever they change, the table follows
    try:
        _set(b"rowblk", 2)
        check("rowblk 2")
        _set(b"rowblk", -1)
        E._check(lib.sdvar_debug_set_rowblk(0))
        check("rowblk 0 through its own setter")
        E._check(lib.sdvar_debug_set_rowblk(-1))
        E._check(lib.sdvar_debug_set_gemm_cfg(32, 2))
        check("forced 32-row tile, K split 2")
    finally:
        _set(b"rowblk", -1)
        E._check(lib.sdvar_debug_set_rowblk(-1))
        E._check(lib.sdvar_debug_set_gemm_cfg(0, 0))
    _same(check("switches back to default"), base, "default switches again")
    # B 3 -> 8 -> 3
    check("B = 8", [1, 2, 3, 4, 5, 5, NC - 1, 0])
    _same(check("B = 3 again"), base, "B = 3 again")


def _sampler(dev):
    sd_d, sd_v = state_dicts(2, PNS)
    sd_t, _ = state_dicts(4, PNS)
    B = 3
    return E.Sampler(E.ModelCtx(sd_t, 4, PNS, B, 2, dev), E.QuantCtx(sd_v, PNS, B, dev), E.ModelCtx(sd_d, 2, PNS, B, 1, dev))


def test_samplers_end_to_end(dev):
    smp = _sampler(dev)
    labels = torch.tensor([3, NC - 1, 3], dtype=torch.int64, device=dev)
    runs = {
        "plain_ar": lambda: smp.plain_ar(labels, 1.5, 900, 0.96, E.Noise("host", 0)),
        "spec natural": lambda: smp.spec_decode(labels, 1.5, 2, 900, 0.96, E.Noise("host", 0)),
        "spec accept_all": lambda: smp.spec_decode(labels, 1.5, 2, 900, 0.96, E.Noise("host", 0), thr=0.0),
    }
    for name, run in runs.items():
        out = {}
        for on in (False, True):
            with _table(on):
                r = run()
                out[on] = (r.ids.clone(), r.f_hat.clone(), r.stats)
        assert torch.equal(out[True][0], out[False][0]), f"{name}: ids differ"
        assert torch.equal(out[True][1], out[False][1]), f"{name}: f_hat differs"
        assert out[True][2] == out[False][2], f"{name}: stats differ"
