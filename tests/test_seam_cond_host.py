"""seam.ada_lin / install_cond without a GPU: which Sequentials get the bound forward, every documented refusal (an SdvarError raised before the library is touched, on
CPU tensors that report is_cuda - the _Fake of tests/test_seam_host.py, restated here), the launch arguments of one fp32 and one autocast call against a recorder in
the library's place (which operands are read in place, which are copied), the workspace size, and the entry points' own argument errors."""
import contextlib
import ctypes as C
import math

import pytest
import torch
import torch.nn as nn

from sdvar_amd import engine as E
from sdvar_amd import seam
import seam_cond_model as CM

F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
FWD, BWD, WS = "sdvar_op_cond_lin_fwd", "sdvar_op_cond_lin_bwd", "sdvar_op_cond_lin_bwd_ws_bytes"


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


def _ops(M=5, K=64, N=96, cdt=F32, wdt=F32, bias=True, grad=(True, True, True), cshape=None):
    c = _Fake(torch.zeros(cshape or (M, K), dtype=cdt, requires_grad=grad[0]))
    w = _Fake(torch.zeros(N, K, dtype=wdt, requires_grad=grad[1]))
    b = _Fake(torch.zeros(N, dtype=F32, requires_grad=grad[2])) if bias else None
    return c, w, b


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_cpu_tensors_are_refused_by_name_before_any_launch():
    with _recording() as rec:
        c, w, b = torch.zeros(4, 64), torch.zeros(96, 64), torch.zeros(96)
        for args, word in (((c, w, b), "cond is a CPU tensor"), ((_Fake(c), w, b), "weight is a CPU tensor"), ((_Fake(c), _Fake(w), b), "bias is a CPU tensor"),
                           ((None, _Fake(w), None), "cond is not a tensor")):
            with pytest.raises(E.SdvarError, match=f"ada_lin: {word}"):
                seam.ada_lin(*args)
        assert rec.calls == []


def test_documented_refusals_name_the_remedy_and_launch_nothing():
    f = seam.ada_lin
    with _recording() as rec:
        c, w, b = _ops()
        cases = [
            (lambda: f(_Fake(c.detach().double()), w, b), r"cond is torch.float64; .*pass cond.float\(\)"),
            (lambda: f(c, _Fake(w.detach().double()), b), r"weight is torch.float64; .*pass weight.float\(\)"),
            (lambda: f(c, w, _Fake(b.detach().double())), "bias is torch.float64"),
            (lambda: f(_Fake(torch.zeros(5, 64, dtype=torch.int32)), w, b), "cond is torch.int32"),
            (lambda: f(_Fake(c.detach().to(F16)), _Fake(w.detach().to(BF16)), b), "float16 mixed with bfloat16"),
            (lambda: f(c, _Fake(w.detach().to(F16)), b), r"weight is torch.float16 next to float32 arithmetic .*torch.autocast.*weight.float\(\)"),
            (lambda: f(c, _Fake(torch.zeros(96, 32)), b), r"shapes do not chain: cond \(5, 64\), weight \(96, 32\)"),
            (lambda: f(c, _Fake(torch.zeros(96, 64, 1)), b), "shapes do not chain"),
            (lambda: f(c, w, _Fake(torch.zeros(95))), r"bias has shape \(95,\), expected \(96,\)"),
            (lambda: f(_Fake(torch.zeros(65, 64)), w, b), r"cond has 65 rows; .*at most 64 rows.*linear_grad / linear_amp_grad"),
            (lambda: f(_Fake(torch.zeros(5, 13, 64)), w, b), "cond has 65 rows"),
            (lambda: f(_Fake(torch.zeros(5, 60)), _Fake(torch.zeros(96, 60)), None), "in_features 60 .*multiple of 8 in \\[8, 4096\\].*linear_grad"),
            (lambda: f(_Fake(torch.zeros(5, 4104)), _Fake(torch.zeros(8, 4104)), None), "in_features 4104"),
            (lambda: f(c, _Fake(torch.zeros(100, 64)), None), "out_features 100 .*multiple of 8.*linear_grad"),
        ]
        for call, words in cases:
            with pytest.raises(E.SdvarError, match=f"ada_lin: {words}"):
                call()
        assert rec.calls == []
    with _recording(autocast=F16) as rec:
        c, w, b = _ops()
        with pytest.raises(E.SdvarError, match="ada_lin: float16 mixed with bfloat16: weight is torch.bfloat16"):
            f(c, _Fake(w.detach().to(BF16)), b)          # the half dtype of the call is autocast's
        assert rec.calls == []


class _OtherDevice(_Fake):
    @property
    def device(self):
        return torch.device("meta")


def test_operands_on_different_devices_are_refused():
    with _recording() as rec, torch.no_grad():
        c, w, b = _ops(grad=(False,) * 3)
        with pytest.raises(E.SdvarError, match="ada_lin: operands live on different devices"):
            seam.ada_lin(c, _OtherDevice(torch.zeros(96, 64)), b)
        assert rec.calls == []


# ------------------------------------------------------------------------------------------------------------------ recorded launches
def test_fp32_call_reads_everything_in_place():
    with _recording() as rec:
        c, w, b = _ops(M=5, K=64, N=96)
        rec.name(cond=c, weight=w, bias=b)
        y = seam.ada_lin(c, w, b)
        assert y.shape == (5, 96) and y.dtype == F32
        assert rec.launches() == [(FWD, ["cond", 0, 64, "weight", 0, "bias", "new", 0, 5, 96, 64, None])]
        dy = torch.zeros(5, 96)
        rec.name(dy=dy)
        y.backward(_Fake(dy))
        assert rec.calls[1] == (WS, [5, 96, 64])
        assert rec.launches()[1] == (BWD, ["dy", "cond", 0, 64, "weight", 0, "new", "new", "new", None, 0, 5, 96, 64, None])     # the recorder's workspace has 0 bytes
        assert c.grad.shape == (5, 64) and w.grad.shape == (96, 64) and b.grad.shape == (96,)
        assert not seam._WEIGHT_PLANES and not seam._SKIP_MAPS


@pytest.mark.parametrize("half,code", [(F16, 1), (BF16, 2)])
def test_autocast_call_fp32_cond_half_result(half, code):
    """The head norm's case (a float32 cond under autocast): operands go to the kernel as they are, the codes say what they are; a frozen weight asks for no dW."""
    with _recording(autocast=half) as rec:
        c, w, b = _ops(M=8, K=128, N=256, grad=(True, False, True))
        rec.name(cond=c, weight=w, bias=b)
        y = seam.ada_lin(c, w, b)
        assert y.dtype == half
        assert rec.launches() == [(FWD, ["cond", 0, 128, "weight", 0, "bias", "new", code, 8, 256, 128, None])]
        y.backward(_Fake(torch.zeros(8, 256, dtype=half)))
        assert rec.launches()[1] == (BWD, ["new", "cond", 0, 128, "weight", 0, "new", None, "new", None, code, 8, 256, 128, None])
        assert c.grad.dtype == F32 and w.grad is None and b.grad.dtype == F32


def test_half_cond_sets_the_arithmetic_without_autocast():
    with _recording() as rec, torch.no_grad():
        c, w, b = _ops(M=3, K=64, N=96, cdt=BF16, grad=(False,) * 3)
        rec.name(cond=c, weight=w)
        assert seam.ada_lin(c, w, None).dtype == BF16
        assert rec.launches() == [(FWD, ["cond", 2, 64, "weight", 0, None, "new", 2, 3, 96, 64, None])]


def test_what_is_read_in_place_and_what_is_copied():
    with _recording() as rec, torch.no_grad():
        _, w, _ = _ops(K=64, N=96, grad=(False,) * 3)
        wide = _Fake(torch.zeros(6, 80))
        base = wide.data_ptr()
        strided = wide[:, 8:72]                     # row stride 80 floats, base + 32 bytes: inside the 16-byte rule
        shifted = wide[:, 1:65]                     # base + 4 bytes: copied once
        odd = _Fake(torch.zeros(6, 66))[:, :64]     # row stride 66 floats = 264 bytes: copied once
        one = wide[2:3, 8:72]                       # one row: its stride does not matter
        three_d = _Fake(torch.zeros(2, 3, 64))
        rec.name(weight=w)
        for t, ptr, ldc in ((strided, base + 32, 80), (shifted, None, 64), (odd, None, 64), (one, base + 2 * 320 + 32, 64), (three_d, three_d.data_ptr(), 64)):
            rec.calls.clear()
            rec.inputs.pop(ptr, None)
            if ptr is not None:
                rec.inputs[ptr] = "cond"
            y = seam.ada_lin(t, w, None)
            assert y.shape == tuple(t.shape[:-1]) + (96,)
            (name, args), = rec.launches()
            assert name == FWD and args[0] == ("cond" if ptr is not None else "new") and args[2] == ldc, (tuple(t.shape), tuple(t.stride()), args)
            rec.inputs.pop(ptr, None)


def test_stride0_and_misaligned_dy_are_copied_once():
    with _recording() as rec:
        c, w, b = _ops(M=4, K=64, N=96)
        dense = torch.zeros(4, 96)
        rec.name(cond=c, weight=w, dy=dense)
        seam.ada_lin(c, w, b).backward(_Fake(dense))
        assert rec.launches()[-1][1][0] == "dy"
        seam.ada_lin(c, w, b).backward(_Fake(dense[:1].expand(4, 96)))
        assert rec.launches()[-1][1][0] == "new"
        flat = torch.zeros(4 * 96 + 1)
        seam.ada_lin(c, w, b).backward(_Fake(flat[1:].view(4, 96)))
        assert rec.launches()[-1][1][0] == "new"


def test_no_grad_and_empty_batches():
    with _recording() as rec:
        c, w, b = _ops()
        with torch.no_grad():
            assert not seam.ada_lin(c, w, b).requires_grad
        assert [n for n, _ in rec.launches()] == [FWD]
        rec.calls.clear()
        y = seam.ada_lin(_Fake(torch.zeros(0, 64, requires_grad=True)), w, b)
        assert y.shape == (0, 96) and rec.calls == []
        y.sum().backward()
        assert rec.calls == []


# ------------------------------------------------------------------------------------------------------------------ installers
class _NS:
    pass


def _sequentials(m):
    return {n for n, q in m.named_modules() if isinstance(q, nn.Sequential) and "forward" in q.__dict__}


def test_install_cond_binds_exactly_the_plain_silu_linear_pairs():
    m = CM.Model()
    m.extra = nn.ModuleDict({
        "three": nn.Sequential(nn.SiLU(), nn.Linear(64, 64), nn.Identity()), "gelu": nn.Sequential(nn.GELU(), nn.Linear(64, 64)),
        "k_odd": nn.Sequential(nn.SiLU(), nn.Linear(60, 64)), "n_odd": nn.Sequential(nn.SiLU(), nn.Linear(64, 60)), "k_big": nn.Sequential(nn.SiLU(), nn.Linear(4104, 8)),
        "fits": nn.Sequential(nn.SiLU(), nn.Linear(4096, 8, bias=False)),
    })
    seam.install_cond(m)
    assert _sequentials(m) == {"block.ada_lin", "head_nm.ada_lin", "extra.fits"}
    assert not any("forward" in q.__dict__ for q in m.modules() if not isinstance(q, nn.Sequential)), "install_cond binds nothing but Sequentials"
    seam.uninstall_cond(m)
    assert not any("forward" in q.__dict__ for q in m.modules())


@pytest.mark.parametrize("installer", [seam.install_train, seam.install_train_amp])
def test_cond_keyword(installer, monkeypatch):
    with pytest.raises(E.SdvarError, match="cond=True .*pass the model"):
        installer(_NS(), None, cond=True)
    m = CM.Model()
    installer(_NS(), m)                               # the default binds nothing
    assert not any("forward" in q.__dict__ for q in m.modules())
    installer(_NS(), m, cond=True, linears=True)
    assert _sequentials(m) == {"block.ada_lin", "head_nm.ada_lin"}
    seen = []
    monkeypatch.setattr(seam, "ada_lin", lambda cond, weight, bias=None: seen.append((tuple(cond.shape), weight, bias)) or cond.new_zeros(cond.shape[:-1] + weight.shape[:1]))
    lin_calls = []
    monkeypatch.setattr(seam, "linear_grad", lambda x, weight, bias=None: lin_calls.append(weight) or x.new_zeros(x.shape[:-1] + weight.shape[:1]))
    with torch.no_grad():
        seq = m.head_nm.ada_lin
        assert seq(torch.zeros(64, CM.D)).shape == (64, 2 * CM.C) and seq(torch.zeros(2, 32, CM.D)).shape == (2, 32, 2 * CM.C)
        assert [s[0] for s in seen] == [(64, CM.D), (2, 32, CM.D)] and all(s[1] is seq[1].weight and s[2] is seq[1].bias for s in seen) and not lin_calls
        assert seq(torch.zeros(65, CM.D)).shape == (65, 2 * CM.C)            # nn.Sequential.forward: SiLU, then the Linear - through linears=True's forward
        assert len(seen) == 2 and len(lin_calls) == 1 and lin_calls[0] is seq[1].weight
    seam.uninstall_cond(m)
    assert not _sequentials(m) and "forward" in m.head_nm.ada_lin[1].__dict__, "uninstall_cond leaves the Linears' bound forwards to uninstall_linears"
    seam.uninstall_linears(m)
    assert not any("forward" in q.__dict__ for q in m.modules())


def test_wide_batches_are_served_up_to_2_23_weights_only(monkeypatch):
    assert seam.cond_serves(16, 11520, 1920) and not seam.cond_serves(17, 11520, 1920) and not seam.cond_serves(32, 11520, 1920)          # d30's ada_lin
    assert all(seam.cond_serves(32, n, k) for n, k in ((6144, 1024), (2048, 1024), (3840, 1920))) and seam.cond_serves(64, 2048, 4096)
    assert not seam.cond_serves(65, 8, 8) and not seam.cond_serves(17, 2056, 4096)
    seq = nn.Sequential(nn.SiLU(), nn.Linear(4096, 2056))          # 2^23 + 32768 weights
    seam.install_cond(seq)
    assert "forward" in seq.__dict__
    seen = []
    monkeypatch.setattr(seam, "ada_lin", lambda cond, weight, bias=None: seen.append(tuple(cond.shape)) or cond.new_zeros(cond.shape[:-1] + weight.shape[:1]))
    with torch.no_grad():
        assert seq(torch.zeros(16, 4096)).shape == (16, 2056) and seq(torch.zeros(17, 4096)).shape == (17, 2056)
    assert seen == [(16, 4096)], "17 rows into more than 2^23 weights: nn.Sequential.forward"
    seam.uninstall_cond(seq)


# ------------------------------------------------------------------------------------------------------------------ the library, no GPU
@pytest.mark.parametrize("M,N,K", [(1, 8, 8), (8, 768, 128), (8, 6144, 1024), (32, 11520, 1920), (64, 200, 4096), (33, 72, 136)])
def test_workspace_size(M, N, K):
    assert E.COND_SLAB == 64 and E.cond_lin_bwd_ws_bytes(M, N, K) == math.ceil(N / 64) * M * K * 4


def test_workspace_size_of_a_bad_shape_raises():
    lib = E.load_library()
    for bad in ((0, 8, 8), (65, 8, 8), (1, 12, 8), (1, 0, 8), (1, 8, 12), (1, 8, 0), (1, 8, 4104), (1, 1 << 20, 4096)):
        assert lib.sdvar_op_cond_lin_bwd_ws_bytes(*bad) == -1 and b"cond_lin_bwd_ws_bytes" in lib.sdvar_last_error()
        with pytest.raises(E.SdvarError):
            E.cond_lin_bwd_ws_bytes(*bad)
        assert not E.cond_lin_shape_ok(*bad)


def test_the_entries_report_argument_errors_before_any_launch():
    """The real library, no GPU: every refusal below is decided on the host before a launch (the pointers are made-up addresses that are never dereferenced)."""
    lib = E.load_library()
    P, odd = C.c_void_p(0x10000), C.c_void_p(0x10004)

    def fwd(c=P, cdt=0, ldc=64, w=P, wdt=0, b=P, y=P, dt=0, M=5, N=96, K=64):
        return lib.sdvar_op_cond_lin_fwd(c, cdt, ldc, w, wdt, b, y, dt, M, N, K, None)

    def bwd(dy=P, c=P, cdt=0, ldc=64, w=P, wdt=0, dc=P, dW=P, db=P, ws=P, dt=0, M=5, N=96, K=64):
        return lib.sdvar_op_cond_lin_bwd(dy, c, cdt, ldc, w, wdt, dc, dW, db, ws, dt, M, N, K, None)

    common = [(dict(M=0), b"M=0"), (dict(M=65), b"M=65"), (dict(K=60), b"K=60"), (dict(K=4104, ldc=4104), b"K=4104"), (dict(N=100), b"N=100"), (dict(N=0), b"N=0"),
              (dict(dt=3), b"dtype=3"), (dict(cdt=1), b"dtype codes"), (dict(wdt=2), b"dtype codes"), (dict(cdt=1, dt=2), b"dtype codes"), (dict(c=None), b"null"),
              (dict(w=None), b"null"), (dict(c=odd), b"16-byte"), (dict(w=odd), b"16-byte"), (dict(ldc=60), b"ldc=60"), (dict(ldc=66), b"ldc=66"),
              (dict(cdt=1, dt=1, ldc=68), b"ldc=68")]
    for name, f, more in (("cond_lin_fwd", fwd, [(dict(y=None), b"y must"), (dict(y=odd), b"16-byte"), (dict(b=odd), b"16-byte")]),
                          ("cond_lin_bwd", bwd, [(dict(dy=None), b"dy must"), (dict(dy=odd), b"16-byte"), (dict(dc=None, dW=None, db=None), b"no output"),
                                                 (dict(ws=None), b"workspace"), (dict(dW=odd), b"16-byte"), (dict(ws=odd), b"16-byte")])):
        for kw, word in common + more:
            assert f(**kw) == 1, (name, kw)
            msg = lib.sdvar_last_error()
            assert word in msg and name.encode() in msg, (name, kw, msg)
