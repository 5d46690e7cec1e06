"""GPU: the kernels of masked sampling, every output inside guard canaries (as tests/test_gpu_row_params.py).
  1. cfg_sample_forced / cfg_sample_rows_forced (csrc/sampler.hip) against their unforced twins, bit for bit, on the hard rows of tests/sampler_hard_cases.py
     at V 4096 / 1000 / 8 / 4, with explicit q and with in-kernel Philox: a sampled token is the twin's token, a forced token is force_ids' and leaves its row
     of dbg_masked alone.
  2. sdvar_mask_tokens against the numpy restatement of tests/edit_cases.py, exactly.
  3. sdvar_img_composite against the two-rounding expression, bit for bit: the 16-byte path, the scalar path, out aliasing gen_img."""
import numpy as np
import pytest
import torch

import edit_cases as EC
import sampler_hard_cases as H
from sdvar_amd import engine as E
from sdvar_amd.ladder import LADDER_256, LADDER_512

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


class _Guarded:
    """A device tensor inside a larger buffer of sentinels: whatever a kernel writes outside its output is seen."""

    def __init__(self, dev, shape, dtype, fill, pad=64):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev)
        self.view = self.buf[pad:pad + n].view(*shape)
        self.fill, self.pad, self.n = fill, pad, n

    def intact(self):
        return bool((self.buf[:self.pad] == self.fill).all()) and bool((self.buf[self.pad + self.n:] == self.fill).all())


# ------------------------------------------------------------------------------------------------ 1. the forced sampler
GROUPS = {
    "v4096": ["b1024", "b1025", "g4096_k40", "g4096_none", "g4096_p_near0_full", "heavy4096_k900"],          # both sort paths (compact / full), top-k off, top-p off
    "v1000": [c.name for c in H.V1000 if c.l == 16][:4],
    "v8": [c.name for c in H.SMALL_V if c.V == 8][:3],
    "v4": [c.name for c in H.SMALL_V if c.V == 4][:3],
}
STRIDE, OFF = 23, 4            # ids land at ids[b * STRIDE + OFF + tok]: the columns around them are guards
FSTRIDE, FOFF = 29, 3          # gen and force_ids are read at [b * FSTRIDE + FOFF + tok]
SENT_ID, SENT_DBG = -7, 123.0
SEED, DRAW, IMG_OFF = 4321 + (9 << 33), 6, 3


def _inputs(names, sl, imgs):
    """Images of the named cases stacked into one batch: (cases per image, logits (2B, l, V), q (B, l, V))."""
    refs = [H.reference(n) for n in names]
    V = refs[0]["case"].V
    assert all(r["case"].V == V and r["case"].l == 16 and r["case"].B == 2 for r in refs)
    cond = torch.cat([r["logits"][:2][imgs, sl] for r in refs], 0)
    unc = torch.cat([r["logits"][2:][imgs, sl] for r in refs], 0)
    q = torch.cat([r["q"].view(2, 16, V)[imgs, sl] for r in refs], 0)
    per = cond.shape[0] // len(refs)
    return [r["case"] for r in refs for _ in range(per)], torch.cat([cond, unc], 0).contiguous(), q.contiguous()


def _tables(dev, cases):
    B = len(cases)
    ts = np.array([c.t for c in cases], np.float64)[None]
    fac = np.stack([(1.0 + ts).astype(np.float32), ts.astype(np.float32)], -1)
    img = np.zeros(B, E.ROW_IMAGE_DTYPE)
    img["top_k"] = [c.top_k for c in cases]
    img["use_top_p"] = [1 if c.top_p > 0.0 else 0 for c in cases]
    img["top_p_thr"] = [np.float32(1.0 - c.top_p) for c in cases]
    img["seed_lo"], img["seed_hi"] = [SEED & 0xFFFFFFFF] * B, [SEED >> 32] * B
    img["index"] = [IMG_OFF + b for b in range(B)]
    return E.RowParams.from_tables(fac, img, dev)


def _launch(dev, rows, cases, lg, q, philox, gen=None, force=None):
    """One launch, forced (gen / force (B, l) given) or the unforced twin.  Returns (ids (B, l), dbg (B, l, V)) on the host; canaries checked."""
    B, l, V = lg.shape[0] // 2, lg.shape[1], lg.shape[2]
    ids = _Guarded(dev, (B, STRIDE), torch.int64, SENT_ID)
    dbg = _Guarded(dev, (B, l, V), torch.float32, SENT_DBG)
    lgd, qd = lg.to(dev), None if philox else q.reshape(B * l, V).to(dev)
    tab = _tables(dev, cases) if rows else None
    c = cases[0]
    if gen is None:
        if rows:
            E.cfg_sample_rows(lgd, B, l, V, tab, 0, qd, DRAW, ids.view, OFF, STRIDE, dbg.view)
        else:
            E.cfg_sample(lgd, B, l, V, c.t, c.top_k, c.top_p, qd, SEED, DRAW, IMG_OFF, ids.view, OFF, STRIDE, dbg.view)
    else:
        g = _Guarded(dev, (B, FSTRIDE), torch.uint8, 1); f = _Guarded(dev, (B, FSTRIDE), torch.int64, 0)
        g.view[:, FOFF:FOFF + l] = gen.to(dev); f.view[:, FOFF:FOFF + l] = force.to(dev)
        g.view[:, :FOFF] = 0; g.view[:, FOFF + l:] = 0                     # the neighbours of the table say "forced": reading them instead would show
        before = (g.buf.clone(), f.buf.clone())
        if rows:
            E.cfg_sample_rows_forced(lgd, B, l, V, tab, 0, qd, DRAW, ids.view, OFF, STRIDE, g.view, f.view, FOFF, FSTRIDE, dbg.view)
        else:
            E.cfg_sample_forced(lgd, B, l, V, c.t, c.top_k, c.top_p, qd, SEED, DRAW, IMG_OFF, ids.view, OFF, STRIDE, g.view, f.view, FOFF, FSTRIDE, dbg.view)
        assert torch.equal(g.buf, before[0]) and torch.equal(f.buf, before[1])          # the tables are read-only
    got = ids.view.cpu()
    assert ids.intact() and dbg.intact()
    assert bool((got[:, :OFF] == SENT_ID).all()) and bool((got[:, OFF + l:] == SENT_ID).all()), "columns around the ids were written"
    return got[:, OFF:OFF + l].clone(), dbg.view.cpu()


def _patterns(B, l):
    alt = torch.zeros(B, l, dtype=torch.uint8); alt.view(-1)[::2] = 1
    if l % 2 == 0 and B > 1:
        alt[1::2] = 1 - alt[1::2]                                          # a checkerboard: every token index is sampled in one image and forced in another
    per_image = torch.zeros(B, l, dtype=torch.uint8); per_image[0::2] = 1  # image 0 fully sampled beside image 1 fully forced
    return {"ones": torch.ones(B, l, dtype=torch.uint8), "zeros": torch.zeros(B, l, dtype=torch.uint8), "alternating": alt, "per_image": per_image,
            "nonzero": torch.full((B, l), 200, dtype=torch.uint8)}       # any non-zero byte means "sample"


def _check_forced(dev, rows, names, philox, sl=slice(None), imgs=slice(None)):
    cases, lg, q = _inputs(names, sl, imgs)
    B, l, V = lg.shape[0] // 2, lg.shape[1], lg.shape[2]
    want_ids, want_dbg = _launch(dev, rows, cases, lg, q, philox)                                   # the unforced twin
    force = torch.from_numpy(np.random.Generator(np.random.Philox(key=[V, B * 100 + l])).integers(0, V, size=(B, l)))
    for pname, gen in _patterns(B, l).items():
        ids, dbg = _launch(dev, rows, cases, lg, q, philox, gen, force)
        g = gen != 0
        assert torch.equal(ids[g], want_ids[g]), f"{pname}: a sampled token differs from the unforced launch"
        assert torch.equal(ids[~g], force[~g]), f"{pname}: a forced token is not force_ids'"
        assert torch.equal(H.bits(dbg[g]), H.bits(want_dbg[g])), f"{pname}: masked logits of a sampled token differ from the unforced launch"
        assert bool((dbg[~g] == SENT_DBG).all()), f"{pname}: a forced token wrote its row of dbg_masked"
    return want_ids


@pytest.mark.parametrize("philox", [False, True], ids=["explicit_q", "philox"])
@pytest.mark.parametrize("group", list(GROUPS))
def test_rows_forced_is_the_rows_kernel_where_sampled(dev, group, philox):
    """Images of several cases in one launch (each with its case's t, top_k, top_p), under every gen pattern."""
    _check_forced(dev, True, GROUPS[group], philox)


@pytest.mark.parametrize("philox", [False, True], ids=["explicit_q", "philox"])
@pytest.mark.parametrize("group", list(GROUPS))
def test_scalar_forced_is_the_scalar_kernel_where_sampled(dev, group, philox):
    for name in GROUPS[group][:3]:
        _check_forced(dev, False, [name], philox)


@pytest.mark.parametrize("rows", [False, True], ids=["scalar", "rows"])
@pytest.mark.parametrize("philox", [False, True], ids=["explicit_q", "philox"])
def test_forced_one_token_and_one_image(dev, rows, philox):
    _check_forced(dev, rows, ["b1025"], philox, sl=slice(5, 6))                                     # l = 1
    _check_forced(dev, rows, ["g1000_k40"], philox, imgs=slice(1, 2))                               # B = 1
    _check_forced(dev, rows, ["g8_full"], philox, sl=slice(0, 1), imgs=slice(0, 1))                 # B = 1, l = 1
    _check_forced(dev, rows, [GROUPS["v4"][0]], philox, sl=slice(3, 4))                             # V = 4, l = 1


@pytest.mark.parametrize("rows", [False, True], ids=["scalar", "rows"])
def test_forced_ids_are_clamped_into_the_vocabulary(dev, rows):
    """Memory safety only (callers validate): the next kernel gathers codebook rows by the id."""
    cases, lg, q = _inputs(["g8_full"], slice(None), slice(None))
    B, l, V = 2, 16, 8
    force = torch.tensor([-5, -1, 0, 7, 8, 9, 2**40, -2**40] * 4).view(B, l)
    ids, _ = _launch(dev, rows, cases, lg, q, True, torch.zeros(B, l, dtype=torch.uint8), force)
    assert torch.equal(ids, force.clamp(0, V - 1))


# ------------------------------------------------------------------------------------------------ 2. mask_tokens
MASK_BATCHES = (("hole", "hole_inverse", "strip"), ("box", "empty", "full"), ("pixel", "half_plane", "speckle"))


@pytest.mark.parametrize("H_px, pns", [(256, LADDER_256), (512, LADDER_512), (512, LADDER_256)], ids=["256", "512", "512_ladder256"])
def test_mask_tokens_is_the_numpy_rule(dev, H_px, pns):
    ms = EC.masks(H_px)
    assert set(sum(MASK_BATCHES, ())) == set(ms)
    L = sum(p * p for p in pns)
    for names in MASK_BATCHES:                                             # B = 3
        m = np.stack([ms[n] for n in names])
        want = torch.from_numpy(EC.mask_tokens_np(m, pns))
        out = _Guarded(dev, (3, L), torch.uint8, 7)
        E.mask_tokens(torch.from_numpy(m).to(dev), pns, out=out.view)
        assert out.intact() and torch.equal(out.view.cpu(), want), names
        first = out.view.clone()
        E.mask_tokens(torch.from_numpy(m).to(dev), pns, out=out.view)      # no atomics: a repeat is bit-identical
        assert torch.equal(out.view, first)
        for b, n in enumerate(names):                                      # B = 1
            one = E.mask_tokens(torch.from_numpy(ms[n][None]).to(dev), pns)
            assert one.shape == (1, L) and one.dtype == torch.uint8 and torch.equal(one.cpu(), want[b:b + 1]), n


def test_mask_tokens_odd_sizes(dev):
    """Sizes that are no multiple of anything: H = 37 with stages 1, 2, 5, 7, 36, 37 (windows of 1 to 37 pixels, overlapping and not), B = 2."""
    pns = (1, 2, 5, 7, 36, 37)
    g = np.random.Generator(np.random.Philox(key=[37, 3]))
    m = (g.integers(0, 3, size=(2, 37, 37)) == 0).astype(np.uint8) * np.uint8(9)
    m[1, :, :19] = 1
    out = _Guarded(dev, (2, sum(p * p for p in pns)), torch.uint8, 7)
    E.mask_tokens(torch.from_numpy(m).to(dev), pns, out=out.view)
    assert out.intact() and torch.equal(out.view.cpu(), torch.from_numpy(EC.mask_tokens_np(m, pns)))


# ------------------------------------------------------------------------------------------------ 3. img_composite
def _composite_inputs(B, Hh, seed):
    g = np.random.Generator(np.random.Philox(key=[seed, 31]))
    gen_img = torch.from_numpy(g.uniform(-1, 1, size=(B, 3, Hh, Hh)).astype(np.float32))
    orig = torch.from_numpy(g.uniform(-1, 1, size=(B, 3, Hh, Hh)).astype(np.float32))
    gen_img.view(-1)[:6] = torch.tensor([-1.0, 1.0, 0.0, -0.0, 2.0 ** -25, -1.0 + 2.0 ** -24])          # the ends of the range and values whose + 1 rounds
    orig.view(-1)[:6] = torch.tensor([1.0, -1.0, 2.0 ** -30, 1.0 - 2.0 ** -24, -2.0 ** -25, 0.5])
    mask = torch.from_numpy((g.integers(0, 2, size=(B, Hh, Hh)) * g.integers(1, 256, size=(B, Hh, Hh))).astype(np.uint8))
    mask.view(-1)[:6] = torch.tensor([1, 0, 1, 0, 1, 0], dtype=torch.uint8)
    want = torch.where((mask != 0)[:, None], gen_img.add(1).mul(0.5), orig.add(1).mul(0.5))                 # torch on the CPU: two roundings each
    return gen_img, orig, mask, want


@pytest.mark.parametrize("B, Hh", [(1, 16), (3, 32)])
def test_img_composite_is_the_two_rounding_expression(dev, B, Hh):
    gen_img, orig, mask, want = _composite_inputs(B, Hh, 100 * B + Hh)
    out = _Guarded(dev, (B, 3, Hh, Hh), torch.float32, 55.0)
    assert out.view.data_ptr() % 16 == 0
    g_d, o_d, m_d = gen_img.to(dev), orig.to(dev), mask.to(dev)
    E.img_composite(g_d, o_d, m_d, out=out.view)
    assert out.intact() and torch.equal(H.bits(out.view.cpu()), H.bits(want))
    assert torch.equal(g_d.cpu(), gen_img) and torch.equal(o_d.cpu(), orig)
    got = E.img_composite(g_d, o_d, m_d)                                                                    # allocating form
    assert torch.equal(H.bits(got.cpu()), H.bits(want))
    # out aliasing gen_img
    alias = _Guarded(dev, (B, 3, Hh, Hh), torch.float32, 55.0)
    alias.view.copy_(g_d)
    ret = E.img_composite(alias.view, o_d, m_d, out=alias.view)
    assert ret.data_ptr() == alias.view.data_ptr() and alias.intact() and torch.equal(H.bits(alias.view.cpu()), H.bits(want))


@pytest.mark.parametrize("B, Hh", [(1, 16), (3, 32)])
@pytest.mark.parametrize("which", ["gen_img", "orig", "mask_px", "out"])
def test_img_composite_scalar_path_on_unaligned_views(dev, B, Hh, which):
    """Any operand off its alignment (floats 4 bytes off 16, the mask 1 byte off 4) sends the launch down the scalar path: the same bits."""
    gen_img, orig, mask, want = _composite_inputs(B, Hh, 7 * B + Hh)
    n = B * 3 * Hh * Hh

    def place(t, off):
        buf = torch.full((t.numel() + 64,), 55 if t.dtype == torch.uint8 else 55.0, dtype=t.dtype, device=dev)
        v = buf[16 + off:16 + off + t.numel()].view(t.shape)
        v.copy_(t.to(dev))
        return buf, v
    bufs = {k: place(t, 1 if k == which else 0) for k, t in (("gen_img", gen_img), ("orig", orig), ("mask_px", mask), ("out", torch.full((n,), 55.0).view(B, 3, Hh, Hh)))}
    views = {k: v for k, (_, v) in bufs.items()}
    align = 4 if which == "mask_px" else 16
    assert views[which].data_ptr() % align != 0 and all(v.data_ptr() % 16 == 0 for k, v in views.items() if k != which)
    E.img_composite(views["gen_img"], views["orig"], views["mask_px"], out=views["out"])
    buf, v = bufs["out"]
    off = 1 if which == "out" else 0
    assert bool((buf[:16 + off] == 55.0).all()) and bool((buf[16 + off + n:] == 55.0).all())
    assert torch.equal(H.bits(v.cpu()), H.bits(want))
    if which == "gen_img":                                                                                  # aliasing on the scalar path too
        E.img_composite(views["gen_img"], views["orig"], views["mask_px"], out=views["gen_img"])
        assert torch.equal(H.bits(views["gen_img"].cpu()), H.bits(want))
        b2 = bufs["gen_img"][0]
        assert bool((b2[:17] == 55.0).all()) and bool((b2[17 + n:] == 55.0).all())
