"""seam.teacher_embed (csrc/embed_train.hip) and install_embed on the GPU: the bit contracts, exactness on integers, float64 references with per-element bounds
(tests/embed_cases.py derives them), the condition drop, the documented safe path for labels / levels out of range with sentinels around every buffer, the operand rules
and the installers on tests/seam_embed_model.py.

Sizes: ladders (1, 2, 3) (L 14, first_l 1) and (2, 3) (L 13, first_l 4), plus (1, 2, 3, 4, 5) (L 55: seven chunks of 8 tokens, so every slice of the second backward pass
adds more than one partial); tokens = first_l, a stage boundary, L; C = 4 (one lane), 64, 132 (a ragged wave), 1028 and 3072 (past one workgroup's 256 / 128 columns);
K = 4, 32, 64 (K > 32 takes the two-columns-per-lane kernels); B = 1, 3, 33, 70; NC1 = 6.

Largest err / bound on an MI355X (one run; the table in DESIGN.md 4q): fp32 x 0.35, dxv 0.39, dclass 0.42, dpos_start 0.45, dW 0.24, dbias 0.26, dlvl 0.45,
dpos_1LC 0.47; with a half x and g: x 1.00 (the rounding of the result is the bound itself), the gradients 0.02 - 0.33.  The stand-in's ladder is (2, 3, 4): with a first
stage of one token the gradient of the attention scale at prog_si 0 is exactly zero and a relative bar has nothing to hold on to."""
import ctypes as C

import math
import pytest
import torch

from sdvar_amd import engine as E
from sdvar_amd import seam
import embed_cases as EC
import seam_embed_model as EM
import seam_linear_model as SM

pytestmark = pytest.mark.gpu

F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
DT_IDS = {F32: "fp32", F16: "fp16", BF16: "bf16"}
# (ladder, tokens, C, K, B)
CASES = [((1, 2, 3), None, 4, 4, 1), ((1, 2, 3), 5, 64, 32, 3), ((1, 2, 3), 1, 132, 32, 33), ((1, 2, 3), None, 132, 64, 33), ((1, 2, 3), None, 1028, 32, 3),
         ((1, 2, 3), None, 3072, 64, 3), ((2, 3), None, 64, 32, 70), ((2, 3), 4, 132, 4, 3), ((2, 3), 9, 1028, 64, 3), ((2, 3), None, 3072, 4, 1), ((2, 3), None, 132, 32, 33),
         ((1, 2, 3, 4, 5), None, 132, 32, 3), ((1, 2, 3, 4, 5), 30, 64, 64, 3)]
CASE_IDS = [f"{'-'.join(map(str, p))}_T{t}_C{c}_K{k}_B{b}" for p, t, c, k, b in CASES]
SMALL = [CASES[1], CASES[8], CASES[10]]
_REFS = {}


@pytest.fixture(autouse=True)
def _state():
    """Grad mode is process-wide state and other test modules switch it off; the caches are put back."""
    with torch.enable_grad():
        yield
    seam.clear_caches()


def _case(pns, T, Cc, K, B, **kw):
    key = (pns, T, Cc, K, B, tuple(sorted(kw.items(), key=str)))
    if key not in _REFS:
        _REFS[key] = EC.make(pns, B, Cc, K, T=T, seed=len(pns) + Cc + K + B, **kw)
    return _REFS[key]


def _bounds(c, key, **kw):
    k = ("bounds", id(c), key)
    if k not in _REFS:
        _REFS[k] = EC.bounds(c, **kw)
    return _REFS[k]


def _run(c, dev, drop=True, out_dtype=F32, need=None, xv_grad=True, with_g=True, with_gc=True, label=None, grad_mode=True):
    """One forward + backward through seam.teacher_embed on the GPU -> {'x', 'cond', gradient names}.  need: the names that require grad (None: all)."""
    d = EC.to_device(c, dev)
    need = set(EC.GRADS if need is None else need)
    params = [d[n].clone().requires_grad_(n in need) for n in EC.PARAMS]
    xv = d["xv"].requires_grad_(True) if ("xv" in need and xv_grad) else d["xv"]
    lab = d["label"] if label is None else label.to(dev)
    kw = dict(tokens=c["T"], drop=(d["r"], c["rate"]) if drop else None, out_dtype=out_dtype)
    if not grad_mode:
        with torch.no_grad():
            x, cond = seam.teacher_embed(lab, xv, *params, d["lvl"], **kw)
        return dict(x=x, cond=cond)
    x, cond = seam.teacher_embed(lab, xv, *params, d["lvl"], **kw)
    outs, grads = [], []
    if with_g:
        outs.append(x); grads.append(d["g"].to(out_dtype))
    if with_gc:
        outs.append(cond); grads.append(d["gc"])
    res = dict(x=x.detach(), cond=cond.detach())
    if need and outs:
        torch.autograd.backward(outs, grads)
        for n, p in zip(EC.PARAMS, params):
            res[n] = p.grad
        res["xv"] = xv.grad if xv.requires_grad else None
    return res


def _torch_class_rows(c, dev, drop=True):
    d = EC.to_device(c, dev)
    j = torch.where(d["r"] < c["rate"], EC.NC1 - 1, d["label"]) if drop else d["label"]
    cond = d["class_emb"][j]
    fl, T = c["first_l"], c["T"]
    sos = cond.unsqueeze(1).expand(c["B"], fl, -1) + d["pos_start"].expand(c["B"], fl, -1)
    sos = sos + (d["lvl_emb"][d["lvl"][0, :fl]].unsqueeze(0).expand(c["B"], -1, -1) + d["pos_1LC"][:, :fl])
    return sos, cond


# ------------------------------------------------------------------------------------------------------------------ 1. bits
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_bits(dev, case):
    c = _case(*case)
    full = _run(c, dev)
    sos, cond = _torch_class_rows(c, dev)
    assert torch.equal(full["cond"], cond), "cond carries the bits of torch's gather"
    assert torch.equal(full["x"][:, :c["first_l"]], sos), "the rows l < first_l carry the bits of torch's float32 expression"
    for half in (F16, BF16):
        assert torch.equal(_run(c, dev, out_dtype=half, grad_mode=False)["x"], full["x"].to(half)), f"{half}: one rounding of the float32 value"
    ng = _run(c, dev, grad_mode=False)
    assert torch.equal(ng["x"], full["x"]) and torch.equal(ng["cond"], full["cond"]), "no_grad runs the same kernel"
    again = _run(c, dev)
    for n, t in full.items():
        assert t is not None and torch.equal(again[n], t), f"{n}: repeats are bit-identical"
    one = dict(c, B=1, label=c["label"][:1], r=c["r"][:1], xv_long=c["xv_long"][:1], g=c["g"][:1], gc=c["gc"][:1])
    assert torch.equal(_run(one, dev, grad_mode=False)["x"][0], full["x"][0]), "a row's bits do not depend on B"


@pytest.mark.parametrize("gdt", [F32, F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("case", SMALL, ids=[CASE_IDS[1], CASE_IDS[8], CASE_IDS[10]])
def test_each_gradient_alone_has_the_bits_of_the_full_run(dev, case, gdt):
    c = _case(*case, gdtype=gdt)
    full = _run(c, dev, out_dtype=gdt)
    for name in EC.GRADS:
        alone = _run(c, dev, out_dtype=gdt, need=[name])
        assert torch.equal(alone[name], full[name]), name
        assert all(alone[n] is None for n in EC.GRADS if n != name), "nothing else is computed"


# ------------------------------------------------------------------------------------------------------------------ 2. exact on integers
@pytest.mark.parametrize("gdt", [F32, F16, BF16], ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_exact_on_integers(dev, case, gdt):
    """Small integers everywhere: every partial sum in any order is an integer below 2^24, so float32 (and the half x, whose values stay below 2^8) is exact."""
    pns, T, Cc, K, B = case
    c = _case(*case, kind="int", labels="same" if B == 33 else "random", gdtype=gdt)
    top = EC.assert_integer_case_is_exact(c, drop=False)
    x64, cond64, gr64 = EC.run(c, F64, drop=False)
    if gdt != F32:
        assert float(x64.abs().max()) <= 256, "the half output holds these integers exactly"
    got = _run(c, dev, drop=False, out_dtype=gdt)
    assert torch.equal(got["x"].cpu().double(), x64) and torch.equal(got["cond"].cpu().double(), cond64)
    for n in EC.GRADS:
        assert torch.equal(got[n].cpu().double(), gr64[n]), f"{n} (largest sum of |terms| {top})"
    T_ = c["T"]
    assert not got["pos_1LC"][:, T_:].any() and not got["xv"][:, max(T_ - c["first_l"], 0):].any(), "the zero tails"
    used = set(c["lvl"][0, :T_].tolist())
    assert all(not got["lvl_emb"][s].any() for s in range(c["S"]) if s not in used)
    assert all(not got["class_emb"][j].any() for j in range(EC.NC1) if j not in set(c["label"].tolist()))
    if B == 33:
        assert got["class_emb"][2].any(), "all 33 images on one label"


# ------------------------------------------------------------------------------------------------------------------ 3. against float64
@pytest.mark.parametrize("kind", ["normal", "heavy"])
@pytest.mark.parametrize("dt", [F32, F16, BF16], ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_against_float64_per_element(dev, case, dt, kind):
    """|err| <= 1.01 (n + 1) 2^-24 sum|terms| per element (+ half an ulp of a half x); the reference reads the same rounded half g."""
    c = _case(*case, kind=kind, gdtype=dt)
    ref, bnd = _bounds(c, dt, out_dtype=dt)
    got = _run(c, dev, out_dtype=dt)
    line = []
    for n in ("x", "cond") + EC.GRADS:
        ratio, zeros_exact, finite = EC.worst(got[n], ref[n], bnd[n])
        line.append(f"{n} {ratio:.3f}")
        assert finite, f"{n}: non-finite values"
        assert zeros_exact, f"{n}: an element without terms is not exactly 0"
        assert ratio <= 1.0, f"{n}: err / bound = {ratio}"
    print(f"\nerr/bound {kind} {DT_IDS[dt]} {case}: " + "  ".join(line))


def test_torch_float32_meets_the_same_bounds():
    """The sanity check of the bound, on the CPU, on two of the cases above."""
    for case in (CASES[3], CASES[8]):
        for kind in ("normal", "heavy"):
            EC.assert_torch_float32_meets_bounds(_case(*case, kind=kind))


# ------------------------------------------------------------------------------------------------------------------ 4. the condition drop
def test_condition_drop(dev):
    c = dict(_case((2, 3), None, 64, 32, 3))
    B = 8
    rate = 0.3
    at = torch.tensor(rate, dtype=F32)
    below = torch.nextafter(at, torch.tensor(0.0))
    c.update(B=B, rate=rate, r=torch.stack([at, below, at, below, torch.tensor(0.0), torch.tensor(0.99), below, at]), label=torch.tensor([0, 1, 2, 3, 4, 0, 4, 4]),
             xv_long=c["xv_long"][:1].expand(B, -1, -1).contiguous(), g=c["g"][:1].expand(B, -1, -1).contiguous(), gc=c["gc"][:1].expand(B, -1).contiguous())
    d = EC.to_device(c, dev)
    want = torch.where(d["r"] < rate, EC.NC1 - 1, d["label"])
    assert want.tolist() == [0, 5, 2, 5, 5, 0, 5, 4], "float32(rate) itself is kept, the float32 below it is dropped"
    got = _run(c, dev)
    assert torch.equal(got["cond"], d["class_emb"][want]), "j_b read back through cond"
    counts = torch.bincount(want.cpu(), minlength=EC.NC1)
    assert [bool(got["class_emb"][j].any()) for j in range(EC.NC1)] == [bool(n) for n in counts.tolist()]
    plain = _run(c, dev, drop=False)
    assert torch.equal(plain["cond"], d["class_emb"][d["label"]]), "drop=None uses the label as it is"
    as32 = _run(c, dev, label=c["label"].to(torch.int32))
    assert all(torch.equal(as32[n], got[n]) for n in got), "int32 and int64 labels agree"
    zero = _run(dict(c, rate=0.0), dev)
    assert torch.equal(zero["cond"], plain["cond"]), "rate 0 drops nothing (r >= 0)"


# ------------------------------------------------------------------------------------------------------------------ 5. guards
def _guarded(n_bytes, dev):
    """A sentinel-filled byte buffer with n_bytes of payload at a 16-byte aligned offset; returns (buffer, payload offset)."""
    pad = 4096
    buf = torch.full((pad + n_bytes + pad,), 0x7B, dtype=torch.uint8, device=dev)
    off = pad + (-(buf.data_ptr() + pad)) % 16
    return buf, off


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [CASES[8], CASES[10], CASES[12]], ids=[CASE_IDS[8], CASE_IDS[10], CASE_IDS[12]])
def test_out_of_range_indices_and_nothing_written_outside_the_buffers(dev, case, dt):
    """The documented safe path: a label of NC1 and a level of S are never used as an index - their rows are NaN, everything else is finite and has the bits of the seam
    call; 0x7B sentinels around every output and the workspace stay intact."""
    c = dict(_case(*case, gdtype=dt))
    B, T, L, fl, Cc, K, S, NC1 = c["B"], c["T"], c["L"], c["first_l"], c["C"], c["K"], c["S"], EC.NC1
    bad_b, bad_l = B - 1, T - 1
    c["label"] = c["label"].clone(); c["label"][bad_b] = NC1
    c["lvl"] = c["lvl"].clone(); c["lvl"][0, bad_l] = S
    c["r"] = torch.ones(B)                                    # nothing dropped: the bad label is used
    d = EC.to_device(c, dev)
    lib, st = E.load_library(), E._stream()
    el = 4 if dt == F32 else 2
    code = E.TRAIN_DTYPES[dt]
    rows = d["xv"].shape[1]
    sizes = {"x": B * T * Cc * el, "cond": B * Cc * 4, "dpos": L * Cc * 4, "dps": fl * Cc * 4, "dl": S * Cc * 4, "dcls": NC1 * Cc * 4, "db": Cc * 4, "dw": Cc * K * 4,
             "dxv": B * rows * K * 4, "ws": E.embed_bwd_ws_bytes(B, T, Cc, K)}
    assert sizes["ws"] == (T * Cc + math.ceil(T / 8) * Cc * K) * 4
    bufs = {n: _guarded(s, dev) for n, s in sizes.items()}
    ptr = lambda n: C.c_void_p(bufs[n][0].data_ptr() + bufs[n][1])
    p = lambda t: C.c_void_p(t.data_ptr())
    g = d["g"].to(dt).contiguous()
    xbs, xrs = d["xv"].stride(0), d["xv"].stride(1)
    E._check(lib.sdvar_op_embed_fwd(p(d["label"]), 1, p(d["r"]), c["rate"], p(d["lvl"]), p(d["xv"]), xbs, xrs, p(d["class_emb"]), p(d["pos_start"]), p(d["word_w"]), p(d["word_b"]),
                                    p(d["lvl_emb"]), p(d["pos_1LC"]), ptr("x"), code, ptr("cond"), B, T, L, fl, Cc, K, S, NC1, st))
    E._check(lib.sdvar_op_embed_bwd(p(g), code, p(d["gc"]), p(d["label"]), 1, p(d["r"]), c["rate"], p(d["lvl"]), p(d["xv"]), xbs, xrs, p(d["word_w"]), ptr("dpos"), ptr("dps"),
                                    ptr("dl"), ptr("dcls"), ptr("db"), ptr("dw"), ptr("dxv"), rows, ptr("ws"), B, T, L, fl, Cc, K, S, NC1, st))
    torch.cuda.synchronize()
    got = _run(c, dev, out_dtype=dt)
    x = got["x"].float()
    nan = torch.zeros(B, T, dtype=torch.bool, device=dev)
    nan[bad_b, :fl] = True
    nan[:, bad_l] = True
    assert x[nan].isnan().all() and x[~nan].isfinite().all(), "NaN exactly on the rows of the bad label and the bad level"
    assert got["cond"][bad_b].isnan().all() and got["cond"][:bad_b].isfinite().all()
    assert all(got[n].isfinite().all() for n in EC.GRADS), "the bad rows add nothing that is not finite"
    ok_b = [b for b in range(B) if b != bad_b]
    want_cls = torch.zeros(NC1, Cc, dtype=F64)
    for b in ok_b:
        want_cls[c["label"][b]] += c["gc"][b].double() + c["g"][b, :fl].double().sum(0)
    assert torch.allclose(got["class_emb"].cpu().double(), want_cls, rtol=1e-5, atol=1e-4), "the bad image adds nothing to dclass"
    names = {"x": "x", "cond": "cond", "dpos": "pos_1LC", "dps": "pos_start", "dl": "lvl_emb", "dcls": "class_emb", "db": "word_b", "dw": "word_w", "dxv": "xv"}
    for n, key in names.items():
        buf, off = bufs[n]
        assert torch.equal(buf[off:off + sizes[n]], got[key].contiguous().view(-1).view(torch.uint8)), f"{n}: the bits of the seam call"
    for n, (buf, off) in bufs.items():
        assert (buf[:off] == 0x7B).all() and (buf[off + sizes[n]:] == 0x7B).all(), f"{n}: bytes outside the buffer were written"


# ------------------------------------------------------------------------------------------------------------------ 6. operands
def test_operands(dev, monkeypatch):
    c = _case(*CASES[10])
    d = EC.to_device(c, dev)
    seen = []
    orig_f, orig_b = E.embed_fwd, E.embed_bwd
    monkeypatch.setattr(E, "embed_fwd", lambda *a, **k: seen.append(("fwd", a[1].data_ptr(), tuple(a[1].stride()))) or orig_f(*a, **k))
    monkeypatch.setattr(E, "embed_bwd", lambda *a, **k: seen.append(("bwd", tuple(a[11]) if len(a) > 11 else tuple(k.get("need")), a[0])) or orig_b(*a, **k))
    base = _run(c, dev)
    assert seen[0][0] == "fwd" and seen[0][2] == ((c["L"] - c["first_l"] + 2) * c["K"], c["K"], 1), "the slice of the longer tensor is read in place: its strides, no copy"
    # a misaligned xv is copied once, and the result does not change
    seen.clear()
    flat = torch.zeros(d["xv"].numel() + 1, device=dev)
    mis = flat[1:].view(d["xv"].shape).copy_(d["xv"])
    params = [d[n] for n in EC.PARAMS]
    with torch.no_grad():
        x, _ = seam.teacher_embed(d["label"], mis, *params, d["lvl"], tokens=c["T"], drop=(d["r"], c["rate"]))
    assert seen[0][1] != mis.data_ptr() and seen[0][1] % 16 == 0 and torch.equal(x, base["x"])
    # a stride-0 upstream gradient
    leaves = [t.clone().requires_grad_(True) for t in params]
    x, cond = seam.teacher_embed(d["label"], d["xv"], *leaves, d["lvl"], tokens=c["T"], drop=None)
    x.sum().backward()
    assert torch.equal(leaves[5].grad[0, 0], torch.full((c["C"],), float(c["B"]), device=dev)) and torch.equal(leaves[3].grad, torch.full((c["C"],), float(c["B"] * (c["T"] - c["first_l"])), device=dev))
    # frozen parameters launch nothing for them
    seen.clear()
    frozen = _run(c, dev, need=["class_emb"])
    assert seen[-1][0] == "bwd" and seen[-1][1] == (False, True, False, False, False, False, False)
    assert torch.equal(frozen["class_emb"], base["class_emb"])
    # double backward raises
    leaves = [t.clone().requires_grad_(True) for t in params]
    x, cond = seam.teacher_embed(d["label"], d["xv"], *leaves, d["lvl"], tokens=c["T"])
    with pytest.raises(E.SdvarError, match="double backward"):
        torch.autograd.grad(x, leaves[2], d["g"], create_graph=True)
    # an in-place weight update is seen by the next call
    w = d["word_w"].clone()
    p2 = list(params); p2[2] = w
    with torch.no_grad():
        a, _ = seam.teacher_embed(d["label"], d["xv"], *p2, d["lvl"], tokens=c["T"])
        w.mul_(2.0)
        b, _ = seam.teacher_embed(d["label"], d["xv"], *p2, d["lvl"], tokens=c["T"])
        p3 = list(params); p3[2] = d["word_w"] * 2.0
        want, _ = seam.teacher_embed(d["label"], d["xv"], *p3, d["lvl"], tokens=c["T"])
    assert torch.equal(b, want) and not torch.equal(a, b), "there is no operand cache"
    assert not seam._WEIGHT_PLANES


# ------------------------------------------------------------------------------------------------------------------ 7. the installers
@pytest.fixture
def slots():
    saved = SM.save_slots()
    yield SM
    SM.restore_slots(saved)


R_FIXED = torch.tensor([0.9, 0.1, 0.5])          # against cond_drop_rate 0.3: the second image is dropped


@pytest.fixture
def fixed_rand(monkeypatch):
    """torch.rand as the model draws it, with the same values on the CPU and on the GPU; counts the draws."""
    draws = []
    monkeypatch.setattr(torch, "rand", lambda n, device=None, **k: draws.append(n) or R_FIXED[:n].to(device))
    return draws


def _u(dtype):
    return 2.0 ** -11 if dtype == F16 else 2.0 ** -8


def _close(label, name, got, ref, half=None, e_torch=None):
    g = got.detach().cpu().double()
    assert g.shape == ref.shape, (label, name, g.shape, ref.shape)
    assert torch.isfinite(g).all(), f"{label} {name}: non-finite values"
    mref, err = ref.abs().max().item(), (g - ref).abs().max().item()
    if half is None:
        bar = 2e-5 * mref
        print(f"{label} fp32 {name}: err {err:.3e}  bar {bar:.3e}  max|ref| {mref:.3e}  err/bar {err / bar if bar else 0.0:.3f}")
    else:
        assert math.isfinite(e_torch) and math.isfinite(mref), f"{label} {name}: e_torch {e_torch}, max|ref| {mref}: an infinite bar hides everything"
        bar = 2 * e_torch + _u(half) * mref + 2e-5 * max(1.0, mref)
        print(f"{label} {str(half)[6:]} {name}: err {err:.3e}  e_torch {e_torch:.3e}  bar {bar:.3e}  max|ref| {mref:.3e}  err/bar {err / bar:.3f}")
    assert err <= bar, f"{label} {name}: err {err:.3e} > bar {bar:.3e} (max|ref| {mref:.3e})"


def _model_refs(prog_si):
    """The stand-in's float64 loss and gradients at loss scales 1 and 1024, and e_torch per tensor and half dtype: torch's CPU run under torch.autocast.  Call it with
    torch.rand already fixed."""
    key = ("model", prog_si)
    if key not in _REFS:
        m, label, feats, w = EM.model_and_inputs()
        m.prog_si = prog_si
        m = m.double()
        ref1 = EM.loss_and_grads(m, label, feats.double(), w.double())
        ref1k = {n: t * 1024.0 for n, t in ref1.items()}
        m = m.float()
        e = {}
        for half in (F16, BF16):
            tor = EM.loss_and_grads(m, label, feats, w, autocast=half, scale=1024.0)
            e[half] = {n: (tor[n].double() - ref1k[n]).abs().max().item() for n in ref1k}
        _REFS[key] = (ref1, ref1k, e)
    return _REFS[key]


def _compare_model(tag, got, ref, half=None, e_torch=None):
    print(f"\n{tag}")
    for n, r in ref.items():
        assert n in got, f"{n} received no gradient"
        _close(tag, n, got[n], r, half, None if e_torch is None else e_torch[n])


def _on_gpu(dev, prog_si):
    m, label, feats, w = EM.model_and_inputs()
    m.prog_si = prog_si
    return m.to(dev), (label.to(dev), feats.to(dev), w.to(dev))


def _uninstall_all(m):
    seam.uninstall_embed(m)
    seam.uninstall_cond(m)
    seam.uninstall_linears(m)
    seam.uninstall_adaln(m)
    seam.uninstall_qknorm(m)
    for b in m.blocks:
        b.ffn.fused_mlp_func = None
    SM.restore_slots({"slow_attn": SM._torch_attn, "flash_attn_func": None, "memory_efficient_attention": None, "fused_mlp_func": None})
    assert not any("forward" in q.__dict__ for q in m.modules())


EVERY = dict(adaln=True, qknorm=True, linears=True, cond=True)


def _check_stage0(m, got, prog_si):
    if prog_si == 0:
        for n in ("word_embed.weight", "word_embed.bias"):
            assert n in got and got[n].shape == dict(m.named_parameters())[n].shape and not got[n].any(), f"{n}: a zero tensor, not None"


@pytest.mark.parametrize("prog_si", [-1, 0, 1])
@pytest.mark.parametrize("others", [False, True], ids=["alone", "every switch"])
def test_install_train_embed(dev, slots, fixed_rand, monkeypatch, others, prog_si):
    ref, _, _ = _model_refs(prog_si)
    m, args = _on_gpu(dev, prog_si)
    plain = EM.loss_and_grads(m, *args)
    seam.install_train(slots, m, embed=True, **(dict(ffn=True, **EVERY) if others else {}))
    assert "forward" in m.__dict__
    calls = []
    orig = seam.teacher_embed
    monkeypatch.setattr(seam, "teacher_embed", lambda *a, **k: calls.append(k) or orig(*a, **k))
    fixed_rand.clear()
    got = EM.loss_and_grads(m, *args)
    assert fixed_rand == [EM.B], "rand is drawn exactly once per call"
    assert len(calls) == 1 and calls[0]["out_dtype"] == F32 and calls[0]["tokens"] == (m.L if prog_si < 0 else m.begin_ends[prog_si][1])
    _compare_model(f"stand-in prog_si {prog_si}, install_train(embed=True{', every switch' if others else ''})", got, ref)
    _check_stage0(m, got, prog_si)
    if others:
        keys = {k[2] for k in seam._WEIGHT_PLANES}
        assert keys and m.word_embed.weight.data_ptr() not in keys, "word_embed's module forward is not called: its weight stays out of the weight-operand cache"
        assert "forward" in m.word_embed.__dict__, "linears=True did bind it"
    _uninstall_all(m)
    again = EM.loss_and_grads(m, *args)
    assert all(torch.equal(again[k], plain[k]) for k in plain), "after the uninstalls the classes' own forwards are back"


@pytest.mark.parametrize("prog_si", [-1, 0, 1])
@pytest.mark.parametrize("others", [False, True], ids=["alone", "every switch"])
@pytest.mark.parametrize("half", [F16, BF16], ids=["fp16", "bf16"])
def test_install_train_amp_embed(dev, slots, fixed_rand, monkeypatch, half, others, prog_si):
    _, ref, e_torch = _model_refs(prog_si)
    m, args = _on_gpu(dev, prog_si)
    if others:          # the finding: adaln=True without embed=True cannot run a model that hands its blocks the autocast dtype
        seam.install_train_amp(slots, m, adaln=True)
        with pytest.raises(E.SdvarError, match="x is torch.(float16|bfloat16); it must be torch.float32"):
            EM.loss_and_grads(m, *args, autocast=half, scale=1024.0)
        seam.uninstall_adaln(m)
    seam.install_train_amp(slots, m, embed=True, **(dict(ffn="half", **EVERY) if others else {}))
    calls, streams = [], []
    orig, orig_ln = seam.teacher_embed, seam.adaln_modulate
    monkeypatch.setattr(seam, "teacher_embed", lambda *a, **k: calls.append(k) or orig(*a, **k))
    monkeypatch.setattr(seam, "adaln_modulate", lambda x, *a, **k: streams.append(x.dtype) or orig_ln(x, *a, **k))
    fixed_rand.clear()
    got = EM.loss_and_grads(m, *args, autocast=half, scale=1024.0)
    assert fixed_rand == [EM.B] and len(calls) == 1
    assert calls[0]["out_dtype"] == (F32 if others else half), "float32 into the seam's residual stream, the autocast dtype into the model's own blocks"
    if others:
        assert streams and all(s == F32 for s in streams), "the blocks see float32"
    assert all(g.dtype == F32 for g in got.values())
    _compare_model(f"stand-in prog_si {prog_si}, install_train_amp(embed=True{', every switch' if others else ''}), autocast {half}", got, ref, half, e_torch[half])
    _check_stage0(m, got, prog_si)
    if others:
        keys = {k[2] for k in seam._WEIGHT_PLANES}
        assert keys and m.word_embed.weight.data_ptr() not in keys
    _uninstall_all(m)
