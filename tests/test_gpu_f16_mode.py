"""GPU: the engine's opt-in GEMM mode 'f16' (ModelCtx(gemm_mode="f16")): an f16x2 model whose block and head GEMMs run as one fp16 product on the high operand
planes (csrc/gemm_half.hip) in calls of at least `h16_min_m` rows.  Tiny model throughout: depth 4 (C = 256), patch_nums (1, 2, 3, 4, 6) (L = 66), V = 4096, B = 2,
'perf'-initialised weights.  The sampler's stage calls have 4 .. 144 rows, the unpaired per-stage calls 2 .. 72 and the teacher-forced call 132, so the half path is
reached by lowering the variant `h16_min_m` (restored in a `finally`).

Accuracy yardstick (test 3): computed on the CPU with no code under test - oracle.var_oracle.OracleVAR with a shim in place of the module's `F` whose `linear`, for
the weights of the five GEMM shapes only, rounds input (saturated at +-65504) and weight to fp16, accumulates in fp32 and rounds fc1's output to fp16 before the
GELU.  e_ref = max |shim oracle - fp32 oracle| over all logits is what ONE fp16 product per GEMM costs on this model; the HIP mode is held to 2 e_ref against the
fp32 oracle (the factor 2: the accumulation order differs, and an fp32 difference of one ulp can flip an fp16 rounding downstream)."""
import contextlib

import pytest
import torch
import torch.nn.functional as TF

from conftest import rnd
from sdvar_amd import engine as E

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DEPTH, PNS, V, B = 4, (1, 2, 3, 4, 6), 4096, 2
C_ = 64 * DEPTH
LENS = [p * p for p in PNS]
L = sum(LENS)
BIG = 1 << 30                    # an h16_min_m above every M
_MEMO = {}


@contextlib.contextmanager
def h16_min_m(v):
    E.set_variant("h16_min_m", v)
    try:
        yield
    finally:
        E.set_variant("h16_min_m", -1)


def weights(depth=DEPTH):
    from sdvar_amd.weights import var_state_dict
    if depth not in _MEMO:
        _MEMO[depth] = var_state_dict(depth, PNS, "perf", 1234, V=V)
    return _MEMO[depth]


def quant(dev):
    from sdvar_amd.weights import vae_state_dict
    if "vae" not in _MEMO:
        _MEMO["vae"] = vae_state_dict(PNS, "stress", ch=32, with_encoder=False)
    return E.QuantCtx(_MEMO["vae"], PNS, B, dev)


def tf_inputs(dev):
    return torch.tensor([3, 977], device=dev), rnd(71, (B, L - 1, 32)).to(dev)


def tf_logits_hip(ctx, labels, xv, dev, staged=False, cfgs=None):
    """(R, L, V) logits of one teacher-forced pass: all stages in one call, or (staged) stage by stage on the KV cache.  cfgs: collects last_gemm_cfg()['bm'] per call."""
    R = labels.shape[0]
    x = torch.empty(R, L, C_, device=dev)
    out = torch.empty(R, L, V, device=dev)
    ctx.begin_rows(labels)
    ctx.embed_teacher(xv, x)
    if not staged:
        ctx.forward(x, 0, len(PNS), out)
        if cfgs is not None:
            cfgs.append(E.last_gemm_cfg()["bm"])
    else:
        bg = 0
        for s, l in enumerate(LENS):
            lg = torch.empty(R, l, V, device=dev)
            ctx.forward(x[:, bg:bg + l].contiguous(), s, 1, lg)
            if cfgs is not None:
                cfgs.append(E.last_gemm_cfg()["bm"])
            out[:, bg:bg + l] = lg
            bg += l
    ctx.kv_set_len(0)
    return out


# ------------------------------------------------------------------------------------------------------------------------ 1. the switch
def test_switch_exists(dev):
    from sdvar_amd import seam
    assert E.GEMM_MODES == ("f32", "bf16x3", "f16x2")
    assert E.ENGINE_GEMM_MODES == E.GEMM_MODES + ("f16",) and E.ENGINE_GEMM_MODES[-1] == "f16"
    ctx = E.ModelCtx(weights(), DEPTH, PNS, B, 1, dev, gemm_mode="f16")
    assert ctx.gemm_mode == "f16"
    ctx.close()
    with pytest.raises(E.SdvarError):
        seam.configure(gemm_mode="f16")
    with pytest.raises(E.SdvarError):
        E.ModelCtx(weights(), DEPTH, PNS, B, 1, dev, gemm_mode="f8")


def test_var_module_attribute(dev):
    """VAR.gemm_mode picks the sampler's arithmetic and is part of engine_ctx's cache key, as tf_gemm_mode is for VAR.forward."""
    from sdvar_amd import VAR, VQVAE
    vae = VQVAE(vocab_size=V, ch=32, with_encoder=False, v_patch_nums=PNS)
    m = VAR(vae, depth=DEPTH, embed_dim=C_, num_heads=DEPTH, patch_nums=PNS, cond_drop_rate=0.0)
    m.load_state_dict(weights(), strict=False)
    m = m.to(dev).eval()
    assert m.gemm_mode is None and m.engine_ctx(B).gemm_mode == E.DEFAULT_GEMM_MODE
    m.gemm_mode = "f16"
    assert m.engine_ctx(B).gemm_mode == "f16"
    m.gemm_mode = None
    assert m.engine_ctx(B).gemm_mode == "f16"                              # None = whatever the cached context runs
    m.tf_gemm_mode = "f16"
    labels, xv = tf_inputs(dev)
    out = m(labels, xv)
    assert m._tf_ctx.gemm_mode == "f16" and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------------------------------ 2. dispatch
def test_below_threshold_is_f16x2_bit_for_bit(dev):
    labels, xv = tf_inputs(dev)
    lab = torch.tensor([3, 977], device=dev)
    res = {}
    with h16_min_m(BIG):
        for mode in ("f16x2", "f16"):
            ctx, q = E.ModelCtx(weights(), DEPTH, PNS, B, len(PNS), dev, gemm_mode=mode), quant(dev)
            cfgs = []
            lg = tf_logits_hip(ctx, labels, xv, dev, cfgs=cfgs)
            assert cfgs[0] != E.HALF_KERNEL_CODE
            r = E.Sampler(ctx, q).plain_ar(lab, 1.5, 900, 0.96, E.Noise("host", 0))
            res[mode] = (lg, r.ids.clone(), r.f_hat.clone())
            if mode == "f16":
                assert r.stats["gemm_mode"] == ("f16", None) and r.stats["last_gemm_half"] is False
            ctx.close()
    for a, b, what in zip(res["f16"], res["f16x2"], ("teacher-forced logits", "plain_ar ids", "plain_ar f_hat")):
        assert torch.equal(a, b), what


def test_half_kernel_runs_and_changes_the_logits(dev):
    labels, xv = tf_inputs(dev)
    with h16_min_m(BIG):
        ctx = E.ModelCtx(weights(), DEPTH, PNS, B, len(PNS), dev, gemm_mode="f16x2")
        base = tf_logits_hip(ctx, labels, xv, dev)
        ctx.close()
    with h16_min_m(1):
        ctx = E.ModelCtx(weights(), DEPTH, PNS, B, len(PNS), dev, gemm_mode="f16")
        cfgs = []
        lg = tf_logits_hip(ctx, labels, xv, dev, cfgs=cfgs)
        assert cfgs == [E.HALF_KERNEL_CODE]
        ctx2 = E.ModelCtx(weights(), DEPTH, PNS, B, len(PNS), dev, gemm_mode="f16x2")       # the variant does not touch an f16x2 model
        cfgs2 = []
        same = tf_logits_hip(ctx2, labels, xv, dev, cfgs=cfgs2)
        assert cfgs2[0] != E.HALF_KERNEL_CODE and torch.equal(same, base)
        ctx.close(); ctx2.close()
    assert bool(torch.isfinite(lg).all()) and not torch.equal(lg, base)


def test_threshold_48_picks_the_kernel_by_rows(dev):
    """Unpaired rows R = 2: stage calls of 2, 8, 18, 32, 72 rows - only the last reaches 48.  The same stages as chunks (0, 1) and (2, 3, 4): 10 rows -> f16x2, 122 rows ->
    half kernel, on the cache the first chunk wrote.  The choice is asserted, not bits across different M."""
    labels, xv = tf_inputs(dev)
    with h16_min_m(48):
        ctx = E.ModelCtx(weights(), DEPTH, PNS, B, len(PNS), dev, gemm_mode="f16")
        cfgs = []
        staged = tf_logits_hip(ctx, labels, xv, dev, staged=True, cfgs=cfgs)
        want = [2 * l >= 48 for l in LENS]
        assert want == [False, False, False, False, True]
        assert [c == E.HALF_KERNEL_CODE for c in cfgs] == want, cfgs
        x = torch.empty(B, L, C_, device=dev)
        ctx.begin_rows(labels); ctx.embed_teacher(xv, x)
        n01, out = LENS[0] + LENS[1], torch.empty(B, L, V, device=dev)
        lg = torch.empty(B, n01, V, device=dev)
        ctx.forward(x[:, :n01].contiguous(), 0, 2, lg)
        assert E.last_gemm_cfg()["bm"] != E.HALF_KERNEL_CODE
        out[:, :n01] = lg
        lg = torch.empty(B, L - n01, V, device=dev)
        ctx.forward(x[:, n01:].contiguous(), 2, 3, lg)
        assert E.last_gemm_cfg()["bm"] == E.HALF_KERNEL_CODE
        out[:, n01:] = lg
        assert ctx.kv_len() == L
        ctx.kv_set_len(0)
        ctx.close()
    assert bool(torch.isfinite(staged).all()) and bool(torch.isfinite(out).all())
    print("h16_min_m = 48: max |staged - chunked| logits", (staged - out).abs().max().item())


def test_planner_reports_the_half_kernel(dev):
    import ctypes
    lib, out = E.load_library(), (ctypes.c_int32 * 4)()
    with h16_min_m(48):
        E._check(lib.sdvar_debug_plan_gemm(2, 48, 768, 256, 7 | E.PLAN_FLAG_F16, out))
        assert list(out) == [E.HALF_KERNEL_CODE, 1, 0, 0]
        E._check(lib.sdvar_debug_plan_gemm(2, 47, 768, 256, 7 | E.PLAN_FLAG_F16, out))
        got = list(out)
        E._check(lib.sdvar_debug_plan_gemm(2, 47, 768, 256, 7, out))
        assert got == list(out)


# ------------------------------------------------------------------------------------------------------------------------ 3. accuracy
class _ShimF:
    """torch.nn.functional with `linear` replaced for the five GEMM weight shapes (module docstring)."""

    def __init__(self):
        self.shapes = {(3 * C_, C_), (C_, C_), (4 * C_, C_), (C_, 4 * C_), (V, C_)}

    def __getattr__(self, name):
        return getattr(TF, name)

    def linear(self, x, w, b=None):
        if tuple(w.shape) not in self.shapes:
            return TF.linear(x, w, b)
        y = TF.linear(x.clamp(-65504.0, 65504.0).half().float(), w.half().float(), b)        # fp16 operands, fp32 accumulation
        return y.half().float() if tuple(w.shape) == (4 * C_, C_) else y                    # fc1: rounded to fp16 before the GELU


def _oracle_logits(labels, xv):
    """(all stages in one call, stage by stage on the KV cache), each (B, L, V), of oracle.var_oracle as it stands at the time of the call."""
    from oracle import var_oracle as orc
    from torch_ref_tf import tf_input, tf_logits
    m = orc.OracleVAR(weights(), DEPTH, PNS)
    one = tf_logits(m, labels, xv)
    x, cond = tf_input(m, labels, xv)
    m.kv_reset()
    parts, bg = [], 0
    for s, l in enumerate(LENS):
        parts.append(m.forward(x[:, bg:bg + l], cond, s, 1))
        bg += l
    m.kv_reset()
    return one, torch.cat(parts, 1)


def test_accuracy_against_the_fp16_operand_oracle(dev, monkeypatch):
    from oracle import var_oracle as orc
    labels, xv = tf_inputs(dev)
    ref = _oracle_logits(labels.cpu(), xv.cpu())
    monkeypatch.setattr(orc, "F", _ShimF())
    shim = _oracle_logits(labels.cpu(), xv.cpu())
    monkeypatch.undo()
    assert orc.F is TF
    e_ref = max((s - r).abs().max().item() for s, r in zip(shim, ref))
    assert e_ref > 0
    with h16_min_m(1):
        ctx = E.ModelCtx(weights(), DEPTH, PNS, B, len(PNS), dev, gemm_mode="f16")
        cfgs = []
        hip = (tf_logits_hip(ctx, labels, xv, dev, cfgs=cfgs).cpu(), tf_logits_hip(ctx, labels, xv, dev, staged=True, cfgs=cfgs).cpu())
        ctx.close()
    assert all(c == E.HALF_KERNEL_CODE for c in cfgs), cfgs
    e_hip = max((h - r).abs().max().item() for h, r in zip(hip, ref))
    e_shim = max((h - s).abs().max().item() for h, s in zip(hip, shim))
    print(f"f16 mode accuracy: e_ref {e_ref:.3e}, max|HIP f16 - fp32 oracle| {e_hip:.3e}, max|HIP f16 - shim oracle| {e_shim:.3e}, max|logit| {ref[0].abs().max().item():.3e}")
    assert e_hip <= 2 * e_ref, (e_hip, e_ref)


# ------------------------------------------------------------------------------------------------------------------------ 4. determinism, 5. speculative loop
def test_plain_ar_repeats_bit_for_bit(dev):
    lab = torch.tensor([3, 977], device=dev)
    with h16_min_m(1):
        ctx, q = E.ModelCtx(weights(), DEPTH, PNS, B, 1, dev, gemm_mode="f16"), quant(dev)
        sm = E.Sampler(ctx, q)
        runs = []
        for _ in range(2):
            r = sm.plain_ar(lab, 1.5, 900, 0.96, E.Noise("host", 0))
            assert r.stats["last_gemm_half"] is True
            runs.append((r.ids.clone(), r.f_hat.clone()))
        ctx.close()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert int(runs[0][0].min()) >= 0 and int(runs[0][0].max()) < V


def test_spec_decode_in_f16(dev):
    lab = torch.tensor([3, 977], device=dev)
    with h16_min_m(1):
        dc = E.ModelCtx(weights(2), 2, PNS, B, 1, dev, gemm_mode="f16")
        tc = E.ModelCtx(weights(), DEPTH, PNS, B, 2, dev, gemm_mode="f16")
        r = E.Sampler(tc, quant(dev), dc).spec_decode(lab, 1.5, 2, 900, 0.96, E.Noise("host", 0), thr=0.0)
        ids, f_hat, st = r.ids.clone(), r.f_hat.clone(), r.stats
        dc.close(); tc.close()
    assert tuple(ids.shape) == (B, L) and int(ids.min()) >= 0 and int(ids.max()) < V
    assert bool(torch.isfinite(f_hat).all())
    assert 1 <= st["target_calls"] <= len(PNS) and 0 <= st["accepted_tokens"] <= L
    assert st["gemm_mode"] == ("f16", "f16")
