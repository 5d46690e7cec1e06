"""seam.linear / linear_grad / linear_amp / linear_amp_grad and their installer without a GPU: argument errors, which nn.Linear modules get the bound forward, and the
launches of a forward and backward - on CPU tensors that report is_cuda (the _Fake of tests/test_seam_trace_host.py, restated here) against a recorder in the
library's place.  What is pinned:
  - every documented refusal is an SdvarError that names its argument, raised before any launch;
  - a full backward launches at most one sdvar_op_scale_pair (mode f16x2 only), exactly ONE gradient-operand pass, one transposed-x operand, two GEMMs and one
    sdvar_op_colsum; a frozen weight costs no wgrad GEMM and no transposed operand, an x without grad no dgrad GEMM; M == 0 launches nothing;
  - the weight operands of a d36 model (36 blocks x 5 weights + head and word_embed, forward and backward kinds: 364 entries) are all cache hits on the second pass."""
import contextlib
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sdvar_amd import engine as E  # noqa: E402
from sdvar_amd import seam  # noqa: E402
import seam_linear_model as SM  # noqa: E402

F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
GEMMS = ("sdvar_op_gemm", "sdvar_op_gemm_f16x2", "sdvar_op_gemm_bf16x3", "sdvar_op_gemm_h")
GRAD_PASSES = ("sdvar_op_grad_operands", "sdvar_op_grad_operands_h")
# what the single pass replaces: none of these may be launched on dy
X_T = ("sdvar_op_transpose_operand", "sdvar_op_operand_transpose_h")


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
        return list(x) if isinstance(x, C.Array) else x

    def __getattr__(self, entry):
        def call(*args):
            self.calls.append((entry, [self._norm(a) for a in args]))
            return 0
        return call

    def names(self):
        return [c[0] for c in self.calls]

    def count(self, *entries):
        return sum(c[0] in entries for c in self.calls)


@contextlib.contextmanager
def _recording(autocast=None, mode=None):
    rec = _Recorder()
    saved = (E.load_library, E._stream, seam._gemm_mode, seam._autocast_gpu_dtype)
    E.load_library, E._stream = (lambda *a, **k: rec), (lambda: None)
    seam._autocast_gpu_dtype = lambda: autocast
    seam.clear_caches()
    if mode is not None:
        seam.configure(mode)
    try:
        with torch.enable_grad():
            yield rec
    finally:
        E.load_library, E._stream, seam._gemm_mode, seam._autocast_gpu_dtype = saved
        seam.clear_caches()


def _ops(M=5, K=64, N=96, xdt=F32, wdt=F32, bias=True, grad=(True, True, True), xshape=None):
    x = _Fake(torch.zeros(xshape or (M, K), dtype=xdt, requires_grad=grad[0]))
    w = _Fake(torch.zeros(N, K, dtype=wdt, requires_grad=grad[1]))
    b = _Fake(torch.zeros(N, dtype=wdt, requires_grad=grad[2])) if bias else None
    return x, w, b


# ------------------------------------------------------------------------------------------------------------------ errors
FOUR = ("linear", "linear_grad", "linear_amp", "linear_amp_grad")


@pytest.mark.parametrize("fn", FOUR)
def test_cpu_tensors_are_refused_by_name_before_any_launch(fn):
    with _recording(autocast=BF16) as rec, torch.no_grad():
        x, w, b = torch.zeros(4, 32), torch.zeros(32, 32), torch.zeros(32)
        with pytest.raises(E.SdvarError, match=rf"{fn}: x is a CPU tensor"):
            getattr(seam, fn)(x, w, b)
        with pytest.raises(E.SdvarError, match=rf"{fn}: weight is a CPU tensor"):
            getattr(seam, fn)(_Fake(x), w, b)
        with pytest.raises(E.SdvarError, match=rf"{fn}: bias is a CPU tensor"):
            getattr(seam, fn)(_Fake(x), _Fake(w), b)
        with pytest.raises(E.SdvarError, match=rf"{fn}: x is not a tensor"):
            getattr(seam, fn)(None, _Fake(w), None)
        assert rec.calls == []


@pytest.mark.parametrize("fn", FOUR)
def test_documented_refusals_name_their_argument_and_launch_nothing(fn):
    amp, grad = "amp" in fn, fn.endswith("grad")
    f = getattr(seam, fn)
    with _recording(autocast=BF16 if amp else None) as rec:
        ctx = contextlib.nullcontext() if grad else torch.no_grad()
        with ctx:
            x, w, b = _ops(grad=(grad,) * 3)
            cases = [
                (lambda: f(_Fake(x.detach().double()), w, b), "x is torch.float64"),
                (lambda: f(x, _Fake(w.detach().double()), b), "weight is torch.float64"),
                (lambda: f(x, w, _Fake(b.detach().double())), "bias is torch.float64"),
                (lambda: f(_Fake(torch.zeros(5, 48)), _Fake(torch.zeros(96, 48)), None), "in_features 48 .*multiple of 32"),
                (lambda: f(x, _Fake(torch.zeros(96, 32)), b), r"shapes do not chain: x \(5, 64\), weight \(96, 32\)"),
                (lambda: f(x, _Fake(torch.zeros(96, 64, 1)), b), "shapes do not chain"),
                (lambda: f(x, w, _Fake(torch.zeros(95))), r"bias has shape \(95,\), expected \(96,\)"),
                (lambda: f(x, w, _Fake(torch.zeros(1, 96))), "bias has shape"),
                (lambda: f(_Fake(torch.zeros(5, 64, dtype=torch.int32)), w, b), "x is torch.int32"),
            ]
            if amp:
                cases += [
                    (lambda: f(_Fake(x.detach().to(F16)), w, _Fake(b.detach().to(BF16))), "mixed half dtypes: bias is torch.bfloat16 .* torch.float16"),
                    (lambda: f(x, _Fake(w.detach().to(F16)), b), "mixed half dtypes: weight is torch.float16"),
                    (lambda: f(x, _Fake(torch.zeros(100, 64)), None), "out_features 100 .*multiple of 8"),
                ]
            else:
                cases += [
                    (lambda: f(_Fake(x.detach().to(F16)), w, b), rf"x is torch.float16; .*float32 operands only - use {fn.replace('linear', 'linear_amp')}"),
                    (lambda: f(x, _Fake(w.detach().to(BF16)), b), "weight is torch.bfloat16; .*linear_amp"),
                ]
            if grad:
                cases += [(lambda: f(x, _Fake(torch.zeros(40, 64, requires_grad=True)), None), "out_features 40 .*multiple of 32 under grad")]
            for call, words in cases:
                with pytest.raises(E.SdvarError, match=f"{fn}: {words}"):
                    call()
        assert rec.calls == []
    if amp:
        with _recording(autocast=None) as rec, torch.no_grad():
            x, w, b = _ops(grad=(False,) * 3)
            with pytest.raises(E.SdvarError, match=rf"{fn}: x is torch.float32 and torch.autocast is not enabled.*use {fn.replace('_amp', '')} "):
                f(x, w, b)
            assert rec.calls == []


@pytest.mark.parametrize("fn", ("linear", "linear_amp"))
def test_inference_twins_refuse_operands_that_require_grad(fn):
    with _recording(autocast=F16) as rec:
        for i, name in enumerate(("x", "weight", "bias")):
            ops = _ops(grad=tuple(j == i for j in range(3)))
            with pytest.raises(E.SdvarError, match=rf"{fn}: {name} requires grad and grad mode is on.*{fn}_grad"):
                getattr(seam, fn)(*ops)
            with torch.no_grad():
                assert getattr(seam, fn)(*ops).shape == (5, 96)
        assert rec.count(*GEMMS) == 3


class _OtherDevice(_Fake):
    @property
    def device(self):
        return torch.device("meta")


@pytest.mark.parametrize("fn", FOUR)
def test_operands_on_different_devices_are_refused(fn):
    with _recording(autocast=F16) as rec, torch.no_grad():
        x, w, b = _ops(grad=(False,) * 3)
        with pytest.raises(E.SdvarError, match=f"{fn}: operands live on different devices"):
            getattr(seam, fn)(x, _OtherDevice(torch.zeros(96, 64)), b)
        assert rec.calls == []


def test_the_entries_report_argument_errors_before_any_launch():
    """The real library, no GPU: every refusal below is decided on the host before a launch (pointers are made-up addresses that are never dereferenced)."""
    lib = E.load_library()
    P, odd = C.c_void_p(0x10000), C.c_void_p(0x10004)
    a = lib.sdvar_op_grad_operands
    cases = [
        (lambda: a(None, 64, 4, 64, 3, None, P, 256, P, 2048, P, None), "need dy"),
        (lambda: a(P, 64, 4, 48, 3, None, P, 192, P, 1536, P, None), "cols %% 32|cols % 32"),
        (lambda: a(P, 64, 0, 64, 3, None, P, 256, P, 2048, P, None), "rows=0"),
        (lambda: a(P, 64, 4, 64, 1, None, P, 256, P, 2048, P, None), "format 1"),
        (lambda: a(P, 64, 4, 64, 3, None, None, 0, None, 0, None, None), "no output"),
        (lambda: a(odd, 64, 4, 64, 3, None, P, 256, P, 2048, P, None), "16-byte aligned"),
        (lambda: a(P, 64, 4, 64, 3, None, odd, 256, P, 2048, P, None), "16-byte aligned"),
        (lambda: a(P, 64, 4, 64, 3, None, P, 256, odd, 2048, P, None), "16-byte aligned"),
        (lambda: a(P, 64, 4, 64, 3, P, P, 256, P, 2048, P, None), "scale goes with format 2"),
        (lambda: a(P, 64, 4, 64, 0, None, P, 256, P, 2048, P, None), "format 0 has no row-major operand"),
        (lambda: a(P, 64, 4, 64, 2, None, P, 200, P, 2048, P, None), "plane stride"),
        (lambda: a(P, 64, 4, 64, 2, None, P, 256, P, 1024, P, None), "plane stride"),
        (lambda: a(P, 62, 4, 64, 2, None, P, 256, P, 2048, P, None), "ld=62"),
    ]
    h = lib.sdvar_op_grad_operands_h
    cases += [
        (lambda: h(None, 0, 64, 4, 64, 1, P, P, P, None), "need dy"),
        (lambda: h(P, 0, 64, 4, 48, 1, P, P, P, None), "cols=48"),
        (lambda: h(P, 0, 64, 4, 64, 3, P, P, P, None), "dtype 3"),
        (lambda: h(P, 2, 64, 4, 64, 1, P, P, P, None), "input dtype 2"),
        (lambda: h(P, 1, 68, 4, 64, 1, P, P, P, None), "ld=68"),
        (lambda: h(P, 0, 64, 4, 64, 1, None, None, None, None), "no output"),
        (lambda: h(odd, 0, 64, 4, 64, 1, P, P, P, None), "16-byte aligned"),
        (lambda: h(P, 0, 64, 4, 64, 1, P, odd, P, None), "16-byte aligned"),
    ]
    t = lib.sdvar_op_operand_transpose_h
    cases += [
        (lambda: t(None, 4, 64, P, None), "need both operands"),
        (lambda: t(P, 4, 64, None, None), "need both operands"),
        (lambda: t(P, 4, 48, P, None), "K=48"),
        (lambda: t(P, 0, 64, P, None), "rows=0"),
        (lambda: t(odd, 4, 64, P, None), "16-byte aligned"),
        (lambda: t(P, 4, 64, odd, None), "16-byte aligned"),
    ]
    for call, words in cases:
        with pytest.raises(E.SdvarError, match=words):
            E._check(call())


# ------------------------------------------------------------------------------------------------------------------ launches
def _fwd_bwd(rec, fn, ops, dy_kind="dense"):
    x, w, b = ops
    rec.name(x=x, w=w, b=b)
    y = getattr(seam, fn)(x, w, b)
    n_fwd = len(rec.calls)
    wanted = [t for t in ops if t is not None and t.requires_grad]
    dy = torch.zeros(y.shape, dtype=y.dtype) if dy_kind == "dense" else torch.zeros((), dtype=y.dtype).expand(y.shape)
    rec.name(dy=dy)
    grads = torch.autograd.grad(y, wanted, dy)
    return y, grads, rec.calls[:n_fwd], rec.calls[n_fwd:]


@pytest.mark.parametrize("mode", E.GEMM_MODES)
def test_fp32_full_backward_reads_dy_once(mode):
    with _recording(mode=mode) as rec:
        ops = _ops(M=70, xshape=(2, 35, 64))
        y, grads, fwd, bwd = _fwd_bwd(rec, "linear_grad", ops)
        assert y.shape == (2, 35, 96) and y.dtype == F32 and [tuple(g.shape) for g in grads] == [(2, 35, 64), (96, 64), (96,)]
        assert sum(c[0] in GEMMS for c in fwd) == 1
        names = [c[0] for c in bwd]
        assert names.count("sdvar_op_scale_pair") == (1 if mode == "f16x2" else 0)
        assert names.count("sdvar_op_grad_operands") == 1 and sum(n in X_T for n in names) == 2           # x^T, and W^T on its first use (cached from then on)
        assert sum(n in GEMMS for n in names) == 2 and names.count("sdvar_op_colsum") == 1
        assert not any(n.startswith("sdvar_op_split_planes") or n == "sdvar_op_half_operand" for n in names)
        tr = [c for c in bwd if c[0] == "sdvar_op_transpose_operand"]
        assert sorted(c[1][0] for c in tr) == ["w", "x"], "the only transposed operands are x's and the weight's: dy^T comes from the single pass"
        (gp,) = [c for c in bwd if c[0] == "sdvar_op_grad_operands"]
        assert gp[1][0] == "dy" and gp[1][1:5] == [96, 70, 96, seam._OPERAND_FORMAT[mode]]
        assert (gp[1][6] is None) == (mode == "f32") and gp[1][8] == "new" and gp[1][10] == "new"
        (cs,) = [c for c in bwd if c[0] == "sdvar_op_colsum"]
        assert cs[1][1:4] == [96, 3, 96]                      # the partials of 96 = pad32(70) rows, not dy
        # a second backward: the weight's transposed operand is cached
        _, _, _, bwd2 = _fwd_bwd(rec, "linear_grad", ops)
        assert sum(c[0] in X_T for c in bwd2) == 1 and sum(c[0] in GRAD_PASSES for c in bwd2) == 1


@pytest.mark.parametrize("half", (F16, BF16))
@pytest.mark.parametrize("xdt", ("f32", "half"))
def test_amp_full_backward_reads_dy_once_and_transposes_the_saved_operand(half, xdt):
    with _recording(autocast=half) as rec:
        ops = _ops(M=70, xdt=F32 if xdt == "f32" else half)
        y, grads, fwd, bwd = _fwd_bwd(rec, "linear_amp_grad", ops)
        assert y.dtype == half and [g.dtype for g in grads] == [ops[0].dtype, F32, F32]
        assert [c[0] for c in fwd] == ["sdvar_op_half_operand", "sdvar_op_half_operand", "sdvar_op_gemm_h"]
        names = [c[0] for c in bwd]
        assert names.count("sdvar_op_scale_pair") == 0 and names.count("sdvar_op_grad_operands_h") == 1
        assert names.count("sdvar_op_operand_transpose_h") == 1 and names.count("sdvar_op_gemm_h") == 2 and names.count("sdvar_op_colsum") == 1
        ho = [c for c in bwd if c[0] == "sdvar_op_half_operand"]
        assert [c[1][0] for c in ho] == ["w"], "the only half_operand call of the backward is the weight's transposed operand, built once"
        (xt,) = [c for c in bwd if c[0] == "sdvar_op_operand_transpose_h"]
        assert xt[1][0] == "new" and xt[1][1:3] == [70, 64], "x^T comes from the forward's saved half operand, not from x"


@pytest.mark.parametrize("fn,kw", [("linear_grad", dict(mode="f32")), ("linear_grad", dict(mode="f16x2")), ("linear_grad", dict(mode="bf16x3")),
                                   ("linear_amp_grad", dict(autocast=F16))])
def test_only_the_gradients_asked_for_are_computed(fn, kw):
    with _recording(**kw) as rec:
        # frozen weight: no wgrad GEMM, no transposed operand of x, nothing of x saved
        _, grads, _, bwd = _fwd_bwd(rec, fn, _ops(grad=(True, False, True)))
        names = [c[0] for c in bwd]
        assert len(grads) == 2 and sum(n in GEMMS for n in names) == 1 and sum(n in GRAD_PASSES for n in names) == 1
        assert not any(c[0] in X_T and c[1][0] != "w" for c in bwd)
        (gp,) = [c for c in bwd if c[0] in GRAD_PASSES]
        assert gp[1][8 if fn == "linear_grad" else 7] is None, "no transposed dy operand without a wgrad"
    with _recording(**kw) as rec:
        # x without grad: no dgrad GEMM, no W^T operand, no row-major dy operand
        _, grads, _, bwd = _fwd_bwd(rec, fn, _ops(grad=(False, True, True)))
        names = [c[0] for c in bwd]
        assert len(grads) == 2 and sum(n in GEMMS for n in names) == 1 and sum(n in X_T for n in names) == 1
        assert not any(c[1][0] == "w" for c in bwd)
        (gp,) = [c for c in bwd if c[0] in GRAD_PASSES]
        assert gp[1][6] is None
    with _recording(**kw) as rec:
        # the bias alone: the pass writes the partials only; no GEMM, no scale
        _, grads, _, bwd = _fwd_bwd(rec, fn, _ops(grad=(False, False, True)), dy_kind="expand")
        assert [c[0] for c in bwd] == [GRAD_PASSES[fn == "linear_amp_grad"], "sdvar_op_colsum"]
        assert bwd[0][1][0] == "new", "a stride-0 dy is copied once"


@pytest.mark.parametrize("fn,kw", [("linear_grad", dict(mode="f16x2")), ("linear_amp_grad", dict(autocast=BF16))])
def test_no_rows_no_launch(fn, kw):
    with _recording(**kw) as rec:
        y, grads, fwd, bwd = _fwd_bwd(rec, fn, _ops(xshape=(0, 64)))
        assert y.shape == (0, 96) and rec.calls == []
        assert [tuple(g.shape) for g in grads] == [(0, 64), (96, 64), (96,)] and all((g == 0).all() for g in grads)


def test_grad_twins_without_grad_launch_what_the_inference_twins_launch():
    for fn, kw in (("linear", dict(mode="f16x2")), ("linear", dict(mode="f32")), ("linear_amp", dict(autocast=F16))):
        def trace(f, grad, no_grad):
            with _recording(**kw) as rec:
                ops = _ops(grad=(grad,) * 3)
                rec.name(x=ops[0], w=ops[1], b=ops[2])
                with torch.no_grad() if no_grad else contextlib.nullcontext():
                    y = getattr(seam, f)(*ops)
                assert not y.requires_grad
                return rec.calls

        want = trace(fn, False, False)
        assert len(want) >= 1 and trace(fn + "_grad", False, False) == want and trace(fn + "_grad", True, True) == want, fn


# ------------------------------------------------------------------------------------------------------------------ the installer
def test_installer_binds_exactly_the_qualifying_linears_and_needs_the_model():
    m, *_ = SM.model_and_inputs()
    m.add_module("narrow_in", nn.Linear(40, 64))
    want = {n for n, q in m.named_modules() if isinstance(q, nn.Linear) and n not in ("odd", "narrow_in")}
    assert want == {"word_embed", "head", "block.attn.mat_qkv", "block.attn.proj", "block.ffn.fc1", "block.ffn.fc2", "block.ada_lin.1"}
    bound = lambda: {n for n, q in m.named_modules() if "forward" in q.__dict__}
    saved = SM.save_slots()
    try:
        for call in (lambda: seam.install_linears(None), lambda: seam.install_train(SM, None, linears=True), lambda: seam.install_train_amp(SM, linears=True)):
            with pytest.raises(E.SdvarError, match="linears=True binds a forward.*pass the model|install_linears.*pass the model"):
                call()
        seam.install_train(SM, m)                           # the default binds nothing
        seam.install_train_amp(SM, m)
        assert bound() == set()
        seam.install_linears(m)
        assert bound() == want
        assert all(m.get_submodule(n).forward.__func__ is seam._linear_module_forward for n in want)
        seam.uninstall_linears(m)
        assert bound() == set() and m.head.forward.__func__ is nn.Linear.forward
        seam.install_train(SM, m, linears=True)
        assert bound() == want
        seam.uninstall_linears(m)
        seam.install_train_amp(SM, m, ffn="half", adaln=True, qknorm=True, linears=True)
        assert bound() == want | {"block", "block.attn"}
        seam.uninstall_linears(m)
        assert bound() == {"block", "block.attn"}, "uninstall_linears takes off its own forwards only"
    finally:
        SM.restore_slots(saved)


def test_the_bound_forward_dispatches_at_call_time():
    lin = nn.Linear(64, 96)
    seam.install_linears(lin)
    lin.weight, lin.bias = nn.Parameter(_Fake(lin.weight.detach())), nn.Parameter(_Fake(lin.bias.detach()))
    x32 = _Fake(torch.zeros(3, 64))
    with _recording(autocast=None, mode="bf16x3") as rec:
        assert lin(x32).dtype == F32 and rec.count("sdvar_op_gemm_bf16x3") == 1 and rec.count("sdvar_op_gemm_h") == 0
    with _recording(autocast=F16) as rec:                    # head: a float32 input under autocast
        assert lin(x32).dtype == F16 and rec.count("sdvar_op_gemm_h") == 1
    with _recording(autocast=None) as rec:                   # a half input outside autocast
        lin.weight.data, lin.bias.data = lin.weight.data.to(BF16), lin.bias.data.to(BF16)
        assert lin(_Fake(torch.zeros(3, 64, dtype=BF16))).dtype == BF16 and rec.count("sdvar_op_gemm_h") == 1


# ------------------------------------------------------------------------------------------------------------------ the cache
@pytest.mark.parametrize("fn,kw", [("linear_grad", dict(mode="bf16x3")), ("linear_grad", dict(mode="f16x2")), ("linear_amp_grad", dict(autocast=BF16))])
def test_a_d36_models_weight_operands_are_all_cache_hits_on_the_second_pass(fn, kw):
    n_w = 36 * 5 + 2
    with _recording(**kw) as rec:
        ws = [_Fake(torch.zeros(32, 32, requires_grad=True)) for _ in range(n_w)]
        rec.name(**{f"w{i}": w for i, w in enumerate(ws)})
        x = _Fake(torch.zeros(2, 32, requires_grad=True))

        def one_pass():
            start = len(rec.calls)
            ys = [getattr(seam, fn)(x, w) for w in ws]          # model order forward ...
            for y, w in zip(reversed(ys), reversed(ws)):        # ... and reversed backward
                torch.autograd.grad(y, (x, w), torch.zeros(y.shape, dtype=y.dtype))
            producers = ("sdvar_op_split_planes", "sdvar_op_split_planes_f16", "sdvar_op_transpose_operand", "sdvar_op_half_operand")
            return sum(c[0] in producers and str(c[1][0]).startswith("w") for c in rec.calls[start:])

        assert one_pass() == 2 * n_w
        assert len(seam._WEIGHT_PLANES) == 2 * n_w == 364 <= seam._WEIGHT_PLANES_MAX
        assert one_pass() == 0, "a weight operand was rebuilt on the second pass: the cache is smaller than the model"
