"""sdvar_xent_train_fwd / sdvar_xent_train_bwd without a GPU: exported, bound, and every argument check answers before any GPU call (the pointers below are never
dereferenced: each call fails in the host-side checks).  The Python layer's own argument errors that need no device are here too."""
import ctypes as C

import pytest
import torch

FAKE = 0x10000          # a 16-byte aligned, non-null address; never read


def _lib():
    from sdvar_amd import engine as E
    return E, E.load_library()


def _fwd(lib, logits=FAKE, ld=4096, targets=FAKE, rows=8, V=4096, eps=0.1, loss=FAKE, lse=FAKE, part=None, sums=None, reduced=None):
    return lib.sdvar_xent_train_fwd(logits, ld, targets, rows, V, eps, -100, loss, lse, part, sums, reduced, 0, None)


def _bwd(lib, logits=FAKE, ld=4096, targets=FAKE, lse=FAKE, grad=FAKE, reduction=0, sums=None, rows=8, V=4096, eps=0.1, dlogits=FAKE, flags=0):
    return lib.sdvar_xent_train_bwd(logits, ld, targets, lse, grad, reduction, sums, rows, V, eps, -100, dlogits, flags, None)


def test_entry_points_exported_and_bound():
    E, lib = _lib()
    for name in ("sdvar_xent_train_fwd", "sdvar_xent_train_bwd"):
        assert name in E._SIGNATURES and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.restype is C.c_int32 and len(fn.argtypes) == 14
    assert lib.sdvar_abi_version() == 5            # purely additive: no bump


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_argument_errors_without_gpu(call):
    E, lib = _lib()
    cases = [(dict(logits=None), b"null"), (dict(targets=None), b"null"), (dict(V=6, ld=8), b"V=6"), (dict(V=0, ld=8), b"V=0"), (dict(ld=4092), b"ld=4092"),
             (dict(ld=4098), b"ld=4098"), (dict(eps=1.5), b"label_smoothing=1.5"), (dict(eps=-0.1), b"label_smoothing"), (dict(eps=float("nan")), b"label_smoothing"),
             (dict(rows=0), b"rows=0"), (dict(rows=2 ** 31), b"rows=2147483648"), (dict(logits=FAKE + 4), b"16-byte")]
    if call is _fwd:
        cases += [(dict(loss=None), b"null loss"), (dict(sums=FAKE), b"both or neither"), (dict(reduced=FAKE), b"reduced")]
    else:
        cases += [(dict(lse=None), b"null"), (dict(grad=None), b"null"), (dict(dlogits=None), b"null"), (dict(dlogits=FAKE + 8), b"16-byte"), (dict(reduction=3), b"reduction=3"),
                  (dict(reduction=1), b"sums"), (dict(flags=2), b"flags=2")]
    for kw, needle in cases:
        assert call(lib, **kw) == 1, kw
        assert needle in lib.sdvar_last_error(), (kw, lib.sdvar_last_error())


def test_python_argument_errors_without_gpu():
    from sdvar_amd import seam
    from sdvar_amd.engine import SdvarError
    x, t = torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(SdvarError, match=r"\.float\(\)"):
        seam.cross_entropy(x.half(), t)
    with pytest.raises(SdvarError, match="weight=None"):
        seam.cross_entropy(x, t, weight=torch.ones(8))
    with pytest.raises(SdvarError, match=r"view\(-1, V\)"):
        seam.cross_entropy(x.view(2, 2, 8), t.view(2, 2))
    with pytest.raises(SdvarError, match="no CPU path"):
        seam.cross_entropy(x, t)
    with pytest.raises(SdvarError, match="reduction"):
        seam.CrossEntropyLoss(reduction="batchmean")
    loss = seam.CrossEntropyLoss(label_smoothing=0.1, reduction="none")
    assert (loss.label_smoothing, loss.reduction, loss.ignore_index) == (0.1, "none", -100) and "0.1" in repr(loss)
    d = seam.CrossEntropyLoss()
    assert (d.label_smoothing, d.reduction, d.ignore_index) == (0.0, "mean", -100)
