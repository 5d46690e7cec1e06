"""sdvar_optim_grad_stats / sdvar_optim_adamw_step (csrc/optim.hip) and seam.AdamW / seam.install_optimizer without a GPU: exported and bound, every argument check
answers before any GPU call (the addresses below are never dereferenced: each call fails in the host-side checks), the Python layer's argument errors, the state_dict
round trips with torch.optim.AdamW and install_optimizer's bookkeeping."""
import ctypes as C
import types

import pytest
import torch

FAKE = 0x10000          # a 16-byte aligned, non-null address; never read
NAN = float("nan")


def _lib():
    from sdvar_amd import engine as E
    return E, E.load_library()


def _table(E, n=2, **kw):
    row = dict(param=FAKE, grad=FAKE, exp_avg=FAKE, exp_avg_sq=FAKE, step=FAKE, numel=1000, lr=1e-3, weight_decay=0.05)
    rows = [dict(row) for _ in range(n)]
    rows[-1].update(kw)          # the offending value sits in the LAST descriptor: the message must name that index
    keys = ("param", "grad", "exp_avg", "exp_avg_sq", "step", "numel", "lr", "weight_decay")
    return E.optim_table([tuple(r[k] for k in keys) for r in rows])


def _stats(E, lib, table="default", n=None, ws=FAKE, ws_bytes=1 << 20, beta1=0.9, beta2=0.95, max_norm=2.0, **kw):
    t = _table(E, **kw) if isinstance(table, str) else table
    return lib.sdvar_optim_grad_stats(t, (len(t) if t is not None else 1) if n is None else n, None, None, max_norm, beta1, beta2, ws, ws_bytes, None)


def _step(E, lib, table="default", n=None, ws=FAKE, ws_bytes=1 << 20, beta1=0.9, beta2=0.95, eps=1e-8, **kw):
    t = _table(E, **kw) if isinstance(table, str) else table
    return lib.sdvar_optim_adamw_step(t, (len(t) if t is not None else 1) if n is None else n, beta1, beta2, eps, ws, ws_bytes, None)


def test_entry_points_exported_and_bound():
    E, lib = _lib()
    for name, arity in (("sdvar_optim_grad_stats", 10), ("sdvar_optim_adamw_step", 8)):
        assert name in E._SIGNATURES and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.restype is C.c_int32 and len(fn.argtypes) == arity
    assert lib.sdvar_abi_version() == 5            # purely additive: no bump
    assert C.sizeof(E._OptimTensor) == 64
    assert E.OPTIM_CHUNK % 1024 == 0 and E.OPTIM_TENSORS_PER_LAUNCH >= 2
    assert E.optim_ws_bytes([1, E.OPTIM_CHUNK, E.OPTIM_CHUNK + 1]) == 16 + 8 * 3 + 8 * 4


@pytest.mark.parametrize("call", [_stats, _step])
def test_argument_errors_without_gpu(call):
    E, lib = _lib()
    who = b"optim_grad_stats" if call is _stats else b"optim_adamw_step"
    cases = [(dict(table=None), b"null tensor list"), (dict(n=0), b"n=0"), (dict(n=-3), b"n=-3"),
             (dict(param=None), b"tensor 1: null param"), (dict(grad=None), b"tensor 1: null grad"), (dict(exp_avg=None), b"tensor 1: null exp_avg pointer"),
             (dict(exp_avg_sq=None), b"tensor 1: null exp_avg_sq"), (dict(step=None), b"tensor 1: null step"), (dict(grad=FAKE + 2), b"tensor 1"),
             (dict(numel=-7), b"numel=-7"), (dict(beta1=1.0), b"beta1=1"), (dict(beta1=-0.1), b"beta1=-0.1"), (dict(beta2=1.5), b"beta2=1.5"), (dict(beta2=NAN), b"beta2"),
             (dict(lr=-1e-3), b"tensor 1: lr=-0.001"), (dict(lr=NAN), b"tensor 1: lr="), (dict(weight_decay=-0.5), b"tensor 1: weight_decay=-0.5"),
             (dict(weight_decay=NAN), b"weight_decay="), (dict(ws=None), b"null workspace"), (dict(ws=FAKE + 4), b"8-byte"),
             (dict(ws_bytes=16 + 8 * 2 + 8 * 2 - 1), b"workspace of 47 bytes is too small"), (dict(numel=3 * E.OPTIM_CHUNK + 1, ws_bytes=16 + 16 + 8 * 4), b"need 72")]
    if call is _stats:
        cases += [(dict(max_norm=NAN), b"max_norm")]
    else:
        cases += [(dict(eps=-1e-8), b"eps=-1e-08"), (dict(eps=NAN), b"eps=")]
    for kw, needle in cases:
        assert call(E, lib, **kw) == 1, kw
        err = lib.sdvar_last_error()
        assert needle in err and who in err, (kw, err)


def _params(dtype=torch.float32):
    torch.manual_seed(0)
    return [torch.nn.Parameter(torch.randn(5, dtype=dtype)), torch.nn.Parameter(torch.randn(3, 2, dtype=dtype))]


def _two_groups(ps, **kw):
    return [dict(params=ps[:1], lr_sc=1.0, wd_sc=1.0, **kw), dict(params=ps[1:], weight_decay=0.0, lr_sc=0.5, wd_sc=0.0, **kw)]


def test_python_argument_errors_without_gpu():
    from sdvar_amd import seam
    from sdvar_amd.engine import SdvarError
    assert "AdamW" in seam.__all__ and "install_optimizer" in seam.__all__
    assert issubclass(seam.AdamW, torch.optim.Optimizer) and seam.AdamW._step_supports_amp_scaling is True
    ps = _params()
    with pytest.raises(SdvarError, match="amsgrad"):
        seam.AdamW(ps, amsgrad=True)
    with pytest.raises(SdvarError, match="maximize"):
        seam.AdamW(ps, maximize=True)
    with pytest.raises(SdvarError, match="betas"):
        seam.AdamW(ps, betas=(0.9, 1.0))
    with pytest.raises(SdvarError, match="nesterov"):
        seam.AdamW(ps, nesterov=True)
    opt = seam.AdamW(ps, lr=1e-3, betas=(0.9, 0.95), fused=True, foreach=None, capturable=False, differentiable=False, grad_clip=2.0)          # train.py:118's keywords
    assert hasattr(opt, "global_grad_norm") and opt.grad_clip == 2.0
    opt.step()                                               # no gradient anywhere: nothing to do, no GPU needed
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(SdvarError, match="closure"):
        opt.step(lambda: 0.0)
    with pytest.raises(SdvarError, match="parameter 0 is on cpu"):
        opt.step()
    ps[0].grad = None
    with pytest.raises(SdvarError, match="parameter 1 is on cpu"):          # the index runs over all parameters, those without a gradient included
        opt.step()
    p64 = _params(torch.float64)
    o64 = seam.AdamW(p64)
    for p in p64:
        p.grad = torch.ones_like(p)
    with pytest.raises(SdvarError, match="parameter 0"):
        o64.step()


def _same_state(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for name in a["state"][k]:
            x, y = a["state"][k][name], b["state"][k][name]
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (k, name)


def test_state_dict_round_trips_with_torch():
    from sdvar_amd import seam
    ps = _params()
    topt = torch.optim.AdamW(_two_groups(ps), lr=2e-3, betas=(0.9, 0.95), weight_decay=0.05, foreach=False)
    for i in range(2):
        for p in ps:
            p.grad = torch.full_like(p, 0.1 * (i + 1))
        topt.step()
    sd = topt.state_dict()
    sopt = seam.AdamW(_two_groups(ps))
    sopt.load_state_dict(sd)
    sd2 = sopt.state_dict()
    _same_state(sd, sd2)
    assert sd2["param_groups"][1]["wd_sc"] == 0.0 and sd2["param_groups"][0]["betas"] == (0.9, 0.95)
    # and back: the seam's state loads into torch, which then steps from it
    tback = torch.optim.AdamW(_two_groups(ps), foreach=False)
    tback.load_state_dict(sd2)
    _same_state(sd, tback.state_dict())
    before = [p.detach().clone() for p in ps]
    tback.step()
    assert all(not torch.equal(a, p) for a, p in zip(before, ps))
    assert all(float(s["step"]) == 3.0 for s in tback.state.values())


def test_install_optimizer_bookkeeping():
    from sdvar_amd import seam
    from sdvar_amd.engine import SdvarError
    ps = _params()
    topt = torch.optim.AdamW(_two_groups(ps), lr=2e-3, betas=(0.9, 0.95), weight_decay=0.05, foreach=False)
    for p in ps:
        p.grad = torch.full_like(p, 0.3)
    topt.step()
    want = topt.state_dict()
    vo = types.SimpleNamespace(optimizer=topt, grad_clip=2.0, early_clipping=True, late_clipping=False)
    seam.install_optimizer(vo)
    assert type(vo.optimizer) is seam.AdamW and vo.optimizer.grad_clip == 2.0
    assert vo.early_clipping is False and vo.late_clipping is True
    assert hasattr(vo.optimizer, "global_grad_norm")          # what amp_sc.py:34-35 looks for
    _same_state(want, vo.optimizer.state_dict())
    g0, g1 = vo.optimizer.param_groups
    assert (g0["lr_sc"], g0["wd_sc"], g1["lr_sc"], g1["wd_sc"]) == (1.0, 1.0, 0.5, 0.0) and g1["weight_decay"] == 0.0 and g0["weight_decay"] == 0.05
    assert g0["params"][0] is ps[0] and g1["params"][0] is ps[1]
    assert all(vo.optimizer.state[p]["exp_avg"] is topt.state[p]["exp_avg"] for p in ps)          # the state tensors themselves, not copies
    g0["lr"] = 5e-4                                            # lr_wd_annealing writes the groups of var_opt.optimizer
    assert vo.optimizer.state_dict()["param_groups"][0]["lr"] == 5e-4

    vo0 = types.SimpleNamespace(optimizer=torch.optim.AdamW(_two_groups(ps), foreach=False), grad_clip=0, early_clipping=False, late_clipping=False)
    seam.install_optimizer(vo0)
    assert vo0.early_clipping is False and vo0.late_clipping is False and vo0.optimizer.grad_clip == 0.0

    with pytest.raises(SdvarError, match="SGD"):
        seam.install_optimizer(types.SimpleNamespace(optimizer=torch.optim.SGD(ps, lr=0.1), grad_clip=2.0, early_clipping=True, late_clipping=False))
    with pytest.raises(SdvarError, match="amsgrad"):
        seam.install_optimizer(types.SimpleNamespace(optimizer=torch.optim.AdamW(ps, amsgrad=True), grad_clip=2.0, early_clipping=True, late_clipping=False))
    with pytest.raises(SdvarError, match="L2"):
        seam.install_optimizer(types.SimpleNamespace(optimizer=torch.optim.Adam(ps, weight_decay=0.1), grad_clip=2.0, early_clipping=True, late_clipping=False))
