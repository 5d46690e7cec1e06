"""seam.teacher_embed / install_embed without a GPU: every documented refusal (an SdvarError raised before the library is touched, on CPU tensors that report is_cuda -
the _Fake of tests/test_seam_cond_host.py, restated here), the launch arguments of one fp32 and one autocast call against a recorder in the library's place (which
operands are read in place, xv's strides), the workspace size and the entry points' own argument errors from the real library, the installers, the finding that motivates
the feature (a half residual stream into adaln_modulate raises) and the dtype the bound forward asks the kernel for.  Also the CPU-side checks of tests/embed_cases.py:
torch's float32 autograd meets the per-element bounds, and the integer cases stay inside the exact range."""
import contextlib
import ctypes as C
import math

import pytest
import torch

from sdvar_amd import engine as E
from sdvar_amd import seam
import embed_cases as EC
import seam_embed_model as EM
import seam_linear_model as SM

F32, F16, BF16, F64, I64, I32 = torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.int64, torch.int32
FWD, BWD, WS = "sdvar_op_embed_fwd", "sdvar_op_embed_bwd", "sdvar_op_embed_bwd_ws_bytes"
NAMES = ("label", "xv", "class_emb", "pos_start", "word_w", "word_b", "lvl_emb", "pos_1LC", "lvl")


@pytest.fixture(autouse=True)
def _grad_mode():
    """Grad mode is process-wide state and other test modules switch it off."""
    with torch.enable_grad():
        yield


class _Fake(torch.Tensor):
    """A CPU tensor that reports is_cuda = True."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)

    @property
    def is_cuda(self):
        return True


class _Recorder:
    """Stands in for the loaded library: every entry records (name, arguments: pointers as the name of the tensor they belong to, or "new") and returns 0."""

    def __init__(self):
        self.calls, self.inputs, self._alive = [], {}, []

    def name(self, **tensors):
        for n, t in tensors.items():
            if t is not None:
                self.inputs.setdefault(t.data_ptr(), n)
                self._alive.append(t)

    def _norm(self, x):
        if isinstance(x, C.c_void_p):
            return None if x.value is None else self.inputs.get(x.value, "new")
        return x

    def __getattr__(self, entry):
        def call(*args):
            self.calls.append((entry, [self._norm(a) for a in args]))
            return 0
        return call

    def launches(self):
        return [c for c in self.calls if c[0] != WS]


@contextlib.contextmanager
def _recording(autocast=None):
    rec = _Recorder()
    saved = (E.load_library, E._stream, seam._autocast_gpu_dtype)
    E.load_library, E._stream = (lambda *a, **k: rec), (lambda: None)
    seam._autocast_gpu_dtype = lambda: autocast
    seam.clear_caches()
    try:
        with torch.enable_grad():
            yield rec
    finally:
        E.load_library, E._stream, seam._autocast_gpu_dtype = saved


def _ops(B=3, pns=(2, 3), Cc=64, K=32, NC1=6, grad=True, spare=2):
    """The nine operands of teacher_embed as _Fake tensors, by name; xv is a slice of a longer tensor."""
    first_l, L, lvl, _ = EC.ladder(pns)
    z = lambda *s, dt=F32, g=False: _Fake(torch.zeros(*s, dtype=dt, requires_grad=g))
    o = dict(label=z(B, dt=I64), class_emb=z(NC1, Cc, g=grad), pos_start=z(1, first_l, Cc, g=grad), word_w=z(Cc, K, g=grad), word_b=z(Cc, g=grad),
             lvl_emb=z(len(pns), Cc, g=grad), pos_1LC=z(1, L, Cc, g=grad), lvl=_Fake(lvl.clone()))
    o["xv_long"] = z(B, L - first_l + spare, K)
    o["xv"] = o["xv_long"][:, :L - first_l]
    return o, (B, L, first_l, Cc, K, len(pns), NC1)


def _call(o, **kw):
    return seam.teacher_embed(*(o[n] for n in NAMES), **kw)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_cpu_tensors_are_refused_by_name_before_any_launch():
    with _recording() as rec:
        o, _ = _ops()
        for name, word in (("label", "label_B"), ("xv", "x_BLCv_wo_first_l"), ("class_emb", "class_emb"), ("word_w", "word_w"), ("lvl", "lvl_1L"), ("pos_1LC", "pos_1LC")):
            bad = dict(o)
            bad[name] = torch.zeros(o[name].shape, dtype=o[name].dtype)
            with pytest.raises(E.SdvarError, match=f"teacher_embed: {word} is a CPU tensor"):
                _call(bad)
        with pytest.raises(E.SdvarError, match="teacher_embed: word_b is not a tensor"):
            _call(dict(o, word_b=None))
        assert rec.calls == []


def test_documented_refusals_name_the_remedy_and_launch_nothing():
    with _recording() as rec:
        o, (B, L, first_l, Cc, K, S, NC1) = _ops()
        fk = lambda *s, dt=F32: _Fake(torch.zeros(*s, dtype=dt))
        cases = [
            (dict(o, xv=fk(B, L - first_l, K, dt=F64)), {}, r"x_BLCv_wo_first_l is torch.float64; .*pass x_BLCv_wo_first_l.float\(\)"),
            (dict(o, word_w=fk(Cc, K, dt=F64)), {}, r"word_w is torch.float64; .*pass word_w.float\(\)"),
            (dict(o, class_emb=fk(NC1, Cc, dt=F16)), {}, r"class_emb is torch.float16; .*float32 master weights: pass class_emb.float\(\)"),
            (dict(o, pos_1LC=fk(1, L, Cc, dt=BF16)), {}, r"pos_1LC is torch.bfloat16; .*pass pos_1LC.float\(\)"),
            (dict(o, label=fk(B, dt=F32)), {}, r"label_B is torch.float32; .*pass label_B.long\(\)"),
            (dict(o, lvl=fk(1, L, dt=I32)), {}, r"lvl_1L is torch.int32; .*pass lvl_1L.long\(\)"),
            (dict(o, label=fk(B, 1, dt=I64)), {}, r"label_B has shape \(3, 1\)"),
            (dict(o, class_emb=fk(NC1, Cc + 4)), {}, rf"class_emb has shape \(6, {Cc + 4}\); expected \(6, {Cc}\)"),
            (dict(o, word_b=fk(Cc + 4)), {}, "word_b has shape"),
            (dict(o, lvl_emb=fk(S, Cc + 4)), {}, "lvl_emb has shape"),
            (dict(o, pos_1LC=fk(1, L + 1, Cc)), {}, "pos_1LC has shape"),
            (dict(o, pos_start=fk(1, first_l, Cc + 4)), {}, "pos_start has shape"),
            (dict(o, xv=fk(B + 1, L - first_l, K)), {}, r"x_BLCv_wo_first_l has shape \(4, 9, 32\)"),
            (dict(o, xv=fk(B, L - first_l - 1, K)), {}, "x_BLCv_wo_first_l has shape"),
            (dict(o, xv=fk(B, L - first_l, K + 4)), {}, "x_BLCv_wo_first_l has shape"),
            (dict(o, word_w=fk(66, K), class_emb=fk(NC1, 66)), {}, r"C = 66 .*multiple of 4 in \[4, 3072\]"),
            (dict(o, word_w=fk(3076, K)), {}, "C = 3076"),
            (dict(o, word_w=fk(Cc, 30)), {}, r"K = 30 .*multiple of 4 in \[4, 64\].*linear_grad"),
            (dict(o, word_w=fk(Cc, 68)), {}, "K = 68"),
            (o, dict(tokens=first_l - 1), rf"tokens = {first_l - 1} is outside \[first_l, L\] = \[{first_l}, {L}\]"),
            (o, dict(tokens=L + 1), f"tokens = {L + 1} is outside"),
            (dict(o, word_w=fk(Cc * K + 1)[1:].view(Cc, K)), {}, "word_w with strides .* is not dense and 16-byte aligned"),          # reaches the engine only when the seam's copy is bypassed
            (o, dict(drop=(fk(B, dt=F64), 0.1)), "drop's r is torch.float64"),
            (o, dict(drop=(fk(B + 1), 0.1)), r"drop's r has shape \(4,\)"),
            (o, dict(drop=0.1), r"drop must be None or \(r, rate\)"),
            (o, dict(out_dtype=F64), "out_dtype torch.float64"),
        ]
        for ops, kw, words in cases:
            if "not dense" in words:          # the seam copies such a parameter once; the engine itself refuses it
                with pytest.raises(E.SdvarError, match=f"embed_fwd: {words}"):
                    E.embed_fwd(*(ops[n] for n in NAMES))
                continue
            with pytest.raises(E.SdvarError, match=f"teacher_embed: {words}"):
                _call(ops, **kw)
        r = _Fake(torch.zeros(B, requires_grad=True))
        with pytest.raises(E.SdvarError, match="drop's r requires grad"):
            _call(o, drop=(r, 0.1))
        assert rec.calls == []


class _OtherDevice(_Fake):
    @property
    def device(self):
        return torch.device("meta")


def test_operands_on_different_devices_are_refused():
    with _recording() as rec, torch.no_grad():
        o, (B, L, first_l, Cc, K, S, NC1) = _ops(grad=False)
        with pytest.raises(E.SdvarError, match="teacher_embed: lvl_emb is on meta; every operand must be on label's GPU"):
            _call(dict(o, lvl_emb=_OtherDevice(torch.zeros(S, Cc))))
        assert rec.calls == []


# ------------------------------------------------------------------------------------------------------------------ recorded launches
def test_fp32_call_reads_everything_in_place_and_passes_the_strides_of_xv():
    with _recording() as rec:
        o, (B, L, first_l, Cc, K, S, NC1) = _ops()
        r = _Fake(torch.zeros(B))
        rec.name(r=r, **{n: o[n] for n in NAMES})
        T = 9                                              # the ladder (2, 3) up to a boundary: 4 + 5 of the second stage's tokens
        x, cond = _call(o, tokens=T, drop=(r, 0.25))
        assert x.shape == (B, T, Cc) and x.dtype == F32 and cond.shape == (B, Cc) and cond.dtype == F32
        row, batch = K, (L - first_l + 2) * K              # the slice's strides, not those of a copy
        assert rec.launches() == [(FWD, ["label", 1, "r", 0.25, "lvl", "xv", batch, row, "class_emb", "pos_start", "word_w", "word_b", "lvl_emb", "pos_1LC", "new", 0, "new",
                                        B, T, L, first_l, Cc, K, S, NC1, None])]
        g = torch.zeros(B, T, Cc)
        rec.name(g=g)
        x.backward(_Fake(g))
        assert rec.calls[1] == (WS, [B, T, Cc, K])
        assert rec.launches()[1] == (BWD, ["g", 0, None, "label", 1, "r", 0.25, "lvl", "xv", batch, row, "word_w", "new", "new", "new", "new", "new", "new", None, 0, None,
                                           B, T, L, first_l, Cc, K, S, NC1, None])          # no gc; xv asks for no gradient; the recorder's workspace has 0 bytes
        assert o["class_emb"].grad.shape == (NC1, Cc) and o["pos_start"].grad.shape == (1, first_l, Cc) and o["word_w"].grad.shape == (Cc, K)
        assert o["word_b"].grad.shape == (Cc,) and o["lvl_emb"].grad.shape == (S, Cc) and o["pos_1LC"].grad.shape == (1, L, Cc)
        assert not seam._WEIGHT_PLANES and not seam._SKIP_MAPS


@pytest.mark.parametrize("half,code", [(F16, 1), (BF16, 2)])
def test_half_output_call_and_frozen_parameters(half, code):
    """The call the bound forward makes under autocast without adaln: a half x; int32 labels; no drop; only cond's gradient arrives; frozen word_embed and pos_1LC."""
    with _recording(autocast=half) as rec:
        o, (B, L, first_l, Cc, K, S, NC1) = _ops()
        o["label"] = _Fake(torch.zeros(B, dtype=I32))
        for n in ("word_w", "word_b", "pos_1LC"):
            o[n] = _Fake(o[n].detach().clone())
        rec.name(**{n: o[n] for n in NAMES})
        x, cond = _call(o, out_dtype=half)
        assert x.dtype == half and cond.dtype == F32
        (name, args), = rec.launches()
        assert name == FWD and args[:4] == ["label", 0, None, 0.0] and args[14:17] == ["new", code, "new"] and args[18] == L
        gc = torch.zeros(B, Cc)
        rec.name(gc=gc)
        cond.backward(_Fake(gc))
        name, args = rec.launches()[1]
        assert name == BWD and args[:3] == [None, 0, "gc"], "no gradient reached x: g is NULL"
        assert args[12:20] == [None, "new", "new", "new", None, None, None, 0], "dpos_1LC, dbias, dW and dxv are not asked for"
        assert o["word_w"].grad is None and o["pos_1LC"].grad is None and o["class_emb"].grad is not None


def test_what_is_read_in_place_and_what_is_copied():
    with _recording() as rec, torch.no_grad():
        o, (B, L, first_l, Cc, K, S, NC1) = _ops(grad=False)
        n = L - first_l
        flat = _Fake(torch.zeros(B * n * K + 1))
        shifted = flat[1:].view(B, n, K)                     # base + 4 bytes: copied once
        wide = _Fake(torch.zeros(B, n, K + 2))[:, :, :K]      # row stride K + 2 floats: copied once
        padded = _Fake(torch.zeros(B, n, K + 4))[:, :, :K]    # row stride K + 4 floats: inside the 16-byte rule
        half = _Fake(torch.zeros(B, n, K, dtype=F16))         # .float(), as the reference does
        turned = _Fake(torch.zeros(B, K, n)).transpose(1, 2)  # last stride n, not 1: copied once
        assert turned.shape == (B, n, K) and turned.stride(2) != 1
        for t, in_place, row in ((o["xv"], True, K), (shifted, False, K), (wide, False, K), (padded, True, K + 4), (half, False, K), (turned, False, K)):
            rec.calls.clear(); rec.inputs.clear()
            rec.name(xv=t)
            _call(dict(o, xv=t))
            (name, args), = rec.launches()
            assert name == FWD and args[5] == ("xv" if in_place else "new") and args[7] == row, (tuple(t.shape), tuple(t.stride()), args)
        rec.calls.clear(); rec.inputs.clear()
        long_half = _Fake(torch.zeros(B, n + 5, K, dtype=F16))          # of a half tensor only the rows the call reads are converted
        seen = []
        real = seam._embed_xv
        seam._embed_xv = lambda xv, rows=None: seen.append(real(xv, rows)) or seen[-1]
        try:
            _call(dict(o, xv=long_half), tokens=first_l + 3)
        finally:
            seam._embed_xv = real
        assert tuple(seen[0].shape) == (B, 3, K) and seen[0].dtype == F32 and rec.launches()[0][1][18] == first_l + 3
        rec.calls.clear()
        _call(dict(o, xv=None), tokens=first_l)               # no word rows: xv may be None and is passed as NULL
        assert rec.launches()[0][1][5] is None and rec.launches()[0][1][18] == first_l


def test_stride0_and_misaligned_gradients_are_copied_once():
    with _recording() as rec:
        o, (B, L, first_l, Cc, K, S, NC1) = _ops()
        dense = torch.zeros(B, L, Cc)
        rec.name(g=dense)
        _call(o)[0].backward(_Fake(dense))
        assert rec.launches()[-1][1][0] == "g"
        _call(o)[0].backward(_Fake(dense[:1, :1].expand(B, L, Cc)))
        assert rec.launches()[-1][1][0] == "new"
        flat = torch.zeros(B * L * Cc + 1)
        _call(o)[0].backward(_Fake(flat[1:].view(B, L, Cc)))
        assert rec.launches()[-1][1][0] == "new"


def test_no_grad_runs_the_same_forward_and_saves_nothing():
    with _recording() as rec:
        o, _ = _ops()
        with torch.no_grad():
            x, cond = _call(o)
        assert not x.requires_grad and not cond.requires_grad and [n for n, _ in rec.launches()] == [FWD]
        x, cond = _call(o)
        saved = x.grad_fn.saved_tensors
        assert len(saved) == 3 and {tuple(t.shape) for t in saved} == {tuple(o["label"].shape), tuple(o["xv"].shape), tuple(o["word_w"].shape)}, "label, xv, word_w: nothing of x's size"


# ------------------------------------------------------------------------------------------------------------------ the installers
class _NS:
    pass


def _bound(m):
    return {n for n, q in m.named_modules() if getattr(q.__dict__.get("forward"), "__func__", None) is seam._embed_var_forward}


@pytest.mark.parametrize("installer", [seam.install_train, seam.install_train_amp])
def test_embed_keyword(installer):
    with pytest.raises(E.SdvarError, match="embed=True .*pass the model"):
        installer(_NS(), None, embed=True)
    m = EM.Model()
    installer(_NS(), m)                               # the default binds nothing
    assert not any("forward" in q.__dict__ for q in m.modules())
    installer(_NS(), m, embed=True)
    assert _bound(m) == {""} and sum("forward" in q.__dict__ for q in m.modules()) == 1, "exactly one forward, on the model itself"
    seam.uninstall_embed(m)
    assert not any("forward" in q.__dict__ for q in m.modules())
    wrapped = torch.nn.Sequential(torch.nn.Identity(), EM.Model())
    seam.install_embed(wrapped)
    assert _bound(wrapped) == {"1"}
    seam.uninstall_embed(wrapped)
    for gone in ("lvl_embed", "cond_drop_rate", "begin_ends"):
        m = EM.Model()
        delattr(m, gone) if gone == "lvl_embed" else m.__dict__.pop(gone)
        with pytest.raises(E.SdvarError, match=f"embed=True found no VAR-like module: Model has no {gone}"):
            installer(_NS(), m, embed=True)
    m = EM.Model()
    del m.shared_ada_lin
    with pytest.raises(E.SdvarError, match="Model has no shared_ada_lin"):
        seam.install_embed(m)


def test_a_half_residual_stream_into_adaln_modulate_raises():
    """The finding: install_train_amp(adaln=True) binds a block forward that hands x to adaln_modulate, which takes float32 only - and the reference model's own forward
    casts x_BLC to the autocast dtype."""
    with _recording(autocast=F16) as rec:
        x = _Fake(torch.zeros(2, 5, 64, dtype=F16))
        v = _Fake(torch.zeros(2, 1, 64, dtype=F16))
        with pytest.raises(E.SdvarError, match=r"adaln_fwd: x is torch.float16; it must be torch.float32 \(pass x.float\(\)\)"):
            seam.adaln_modulate(x, v, v)
        m = EM.Model()
        seam.install_train_amp(_NS(), m, adaln=True)
        blk = m.blocks[0]
        with pytest.raises(E.SdvarError, match="x is torch.float16; it must be torch.float32"):
            blk(x=_Fake(torch.zeros(2, 5, EM.C, dtype=F16)), cond_BD=_Fake(torch.zeros(2, EM.C)), attn_bias=None)
        assert rec.launches() == [] or all(n != "sdvar_op_adaln_fwd" for n, _ in rec.launches())


class _Stop(Exception):
    pass


@pytest.mark.parametrize("autocast", [None, F16, BF16])
@pytest.mark.parametrize("adaln", [False, True])
@pytest.mark.parametrize("prog_si", [-1, 0, 1])
def test_the_bound_forward_asks_for_the_fp32_stream_only_with_adaln_bound(monkeypatch, autocast, adaln, prog_si):
    seen, draws = [], []
    monkeypatch.setattr(seam, "_autocast_gpu_dtype", lambda: autocast)
    monkeypatch.setattr(seam, "teacher_embed", lambda *a, **k: seen.append((a, k)) or (_ for _ in ()).throw(_Stop()))
    real_rand = torch.rand
    monkeypatch.setattr(torch, "rand", lambda *a, **k: draws.append(a) or real_rand(*a, **k))
    m = EM.Model()
    m.prog_si = prog_si
    seam.install_train_amp(_NS(), m, adaln=adaln, embed=True)
    label, feats = torch.zeros(EM.B, dtype=I64), torch.zeros(EM.B, m.L - m.first_l, EM.K)
    with pytest.raises(_Stop):
        m(label, feats)
    (a, k), = seen
    assert k["out_dtype"] == (F32 if adaln or autocast is None else autocast)
    assert k["tokens"] == (m.L if prog_si < 0 else m.begin_ends[prog_si][1]) and a[1] is feats, "x_BLCv_wo_first_l goes to the kernel as it is: the slice is the kernel's"
    assert a[2] is m.class_emb.weight and a[4] is m.word_embed.weight and a[5] is m.word_embed.bias and a[8] is m.lvl_1L
    r, rate = k["drop"]
    assert draws == [(EM.B,)] and tuple(r.shape) == (EM.B,) and rate == m.cond_drop_rate, "one draw of B uniforms per call"
    seam.uninstall_embed(m)
    seam.uninstall_adaln(m)
    assert not any("forward" in q.__dict__ for q in m.modules())


# ------------------------------------------------------------------------------------------------------------------ the library, no GPU
@pytest.mark.parametrize("B,T,Cc,K", [(1, 1, 4, 4), (8, 680, 1024, 32), (32, 680, 1920, 32), (3, 13, 132, 64), (70, 9, 3072, 4)])
def test_workspace_size(B, T, Cc, K):
    assert E.EMBED_TOK == 8 and E.embed_bwd_ws_bytes(B, T, Cc, K) == (T * Cc + math.ceil(T / 8) * Cc * K) * 4


def test_workspace_size_of_a_bad_shape_raises():
    lib = E.load_library()
    for bad in ((0, 8, 64, 32), (1, 0, 64, 32), (1, 8, 66, 32), (1, 8, 3076, 32), (1, 8, 0, 32), (1, 8, 64, 30), (1, 8, 64, 68), (1, 8, 64, 0), (1 << 20, 1 << 10, 64, 32)):
        assert lib.sdvar_op_embed_bwd_ws_bytes(*bad) == -1 and b"embed_bwd_ws_bytes" in lib.sdvar_last_error()
        with pytest.raises(E.SdvarError):
            E.embed_bwd_ws_bytes(*bad)


def test_the_entries_report_argument_errors_before_any_launch():
    """The real library, no GPU: every refusal below is decided on the host before a launch (the pointers are made-up addresses that are never dereferenced)."""
    lib = E.load_library()
    P, odd = C.c_void_p(0x10000), C.c_void_p(0x10004)

    def fwd(label=P, i64=1, r=P, rate=0.1, lvl=P, xv=P, xbs=9 * 32, xrs=32, cls=P, ps=P, w=P, b=P, le=P, pos=P, x=P, xdt=0, cond=P, B=3, T=13, L=13, first_l=4, Cc=64, K=32,
            S=2, NC1=6):
        return lib.sdvar_op_embed_fwd(label, i64, r, rate, lvl, xv, xbs, xrs, cls, ps, w, b, le, pos, x, xdt, cond, B, T, L, first_l, Cc, K, S, NC1, None)

    def bwd(g=P, gdt=0, gc=P, label=P, i64=1, r=P, rate=0.1, lvl=P, xv=P, xbs=9 * 32, xrs=32, w=P, dpos=P, dps=P, dl=P, dcls=P, db=P, dw=P, dxv=P, xv_rows=9, ws=P, B=3, T=13,
            L=13, first_l=4, Cc=64, K=32, S=2, NC1=6):
        return lib.sdvar_op_embed_bwd(g, gdt, gc, label, i64, r, rate, lvl, xv, xbs, xrs, w, dpos, dps, dl, dcls, db, dw, dxv, xv_rows, ws, B, T, L, first_l, Cc, K, S, NC1, None)

    common = [(dict(Cc=66), b"C=66"), (dict(Cc=3076), b"C=3076"), (dict(K=30), b"K=30"), (dict(K=68), b"K=68"), (dict(B=0), b"B=0"), (dict(T=3), b"first_l=4, T=3"),
              (dict(T=14), b"T=14, L=13"), (dict(first_l=0), b"first_l=0"), (dict(S=0), b"S=0"), (dict(NC1=0), b"NC1=0"), (dict(label=odd), b"16-byte"), (dict(r=odd), b"16-byte"),
              (dict(lvl=odd), b"16-byte"), (dict(w=odd), b"16-byte"), (dict(xv=None), b"xv must be given"), (dict(xv=odd), b"xv must be given"), (dict(xrs=28), b"xv strides"),
              (dict(xrs=34), b"xv strides"), (dict(xbs=8 * 32), b"xv strides"), (dict(xbs=9 * 32 + 2), b"xv strides")]
    for name, f, more in (("embed_fwd", fwd, [(dict(xdt=3), b"x_dtype=3"), (dict(x=None), b"null"), (dict(cond=None), b"null"), (dict(cls=None), b"null"), (dict(lvl=None), b"null"),
                                               (dict(x=odd), b"16-byte"), (dict(pos=odd), b"16-byte")]),
                          ("embed_bwd", bwd, [(dict(gdt=3), b"g_dtype=3"), (dict(dpos=None, dps=None, dl=None, dcls=None, db=None, dw=None, dxv=None), b"no output"),
                                               (dict(ws=None), b"workspace"), (dict(g=odd), b"16-byte"), (dict(dw=odd), b"16-byte"), (dict(ws=odd), b"16-byte"),
                                               (dict(label=None), b"dclass needs label"), (dict(g=None, gc=None), b"dclass needs label"), (dict(lvl=None), b"dlvl needs lvl"),
                                               (dict(xv_rows=8), b"xv_rows=8"), (dict(w=None), b"dxv needs W")])):
        for kw, word in common + more:
            assert f(**kw) == 1, (name, kw)
            msg = lib.sdvar_last_error()
            assert word in msg and name.encode() in msg, (name, kw, msg)
    assert fwd(xv=None, T=4) != 1 or b"xv" not in lib.sdvar_last_error(), "xv may be NULL when T == first_l"


# ------------------------------------------------------------------------------------------------------------------ the cases' own checks, on the CPU
@pytest.mark.parametrize("kind", ["normal", "heavy"])
@pytest.mark.parametrize("pns,T", [((1, 2, 3), None), ((2, 3), 9), ((2, 3), 4)])
def test_torch_float32_meets_the_bounds_of_the_cases(pns, T, kind):
    c = EC.make(pns, B=33, C=132, K=32, T=T, seed=3, kind=kind)
    ratios = EC.assert_torch_float32_meets_bounds(c)
    print({n: round(v, 3) for n, v in ratios.items()})
    assert ratios["cond"] == 0.0


def test_integer_cases_stay_inside_the_exact_range():
    for pns, B, Cc, K, T, labels in [((1, 2, 3), 33, 132, 64, None, "same"), ((2, 3), 70, 64, 32, 9, "random"), ((1, 2, 3, 4, 5), 3, 1028, 32, None, "random")]:
        c = EC.make(pns, B, Cc, K, T=T, kind="int", labels=labels)
        assert EC.assert_integer_case_is_exact(c, drop=False) < 2 ** 24
        x, _, gr = EC.run(c, F64, drop=False)
        assert all(bool((t == t.round()).all()) for t in [x] + list(gr.values()))
