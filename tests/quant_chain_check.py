"""A per-scale fp64 check of the multi-scale residual quantisation (quant.py:135-166; csrc/quant.hip: quant_down_kernel / quant_rows_kernel ->
quant_nearest_kernel -> quant_up_kernel -> quant_phi_rest_kernel), for any implementation that returns its ids and its f_hat after every scale.  Test
infrastructure only (never imported by sdvar_amd/).

check_chain verifies scale s from the tested implementation's OWN state after scale s - 1 (its f_hat[s - 1]), so a legitimate near-tie that falls the
other way at one scale does not cascade into "every later id differs":

    f_rest64 = f64 - f_hat[s - 1]                      (f_hat[-1] = 0)
    z64      = area_down(f_rest64, pn_s)               (F.interpolate(mode="area") in double; the last scale takes f_rest64 itself)
    d64[n,v] = |z_n|^2 + |e_v|^2 - 2 z_n.e_v           in double, against every code

The bounds (derived, not measured; u = 2^-24, the unit round-off of float):

  b_v = gamma_36 (|z| + |e_v|)^2,  gamma_36 = 36 u / (1 - 36 u).   The tested formula is fl((|z|^2 + |e_v|^2) - 2 z.e_v) in float: two 32-term sums of squares,
        one 32-term dot product and three scalar operations (the add, the doubling, the subtract).  Every partial result is bounded in magnitude by
        |z|^2 + |e_v|^2 + 2 |z||e_v| = (|z| + |e_v|)^2 (Cauchy-Schwarz for the dot product), and no term passes through more than 32 + 1 + 3 = 36 roundings,
        so |fl(d_v) - d_v| <= gamma_36 (|z| + |e_v|)^2 in any summation order (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).
        Comparing two computed distances costs b_k + b_best.
  p_v = 2 |e_v - e_best| sqrt(32) delta,  delta = (s + 1) 2^-23 max|f|.   The device does not form f - f_hat[s - 1]: it keeps a running float f_rest, updated
        f_rest <- fl(f_rest - h) next to f_hat <- fl(f_hat + h).  Each scale adds at most half an ulp of |f_rest| and half an ulp of |f_hat| to the difference
        between the running f_rest and f - f_hat, together <= 2^-23 max|f| per element and scale, hence <= delta after s + 1 scales.  Area pooling is an average, so
        every channel of z moves by at most delta and |dz| <= sqrt(32) delta; d_v - d_best is linear in z with gradient -2 (e_v - e_best), which gives p_v.

  (a) near-optimal, every row:   the chosen code k has   d64_k - d64_best <= b_k + b_best + p_k.
  (b) exact where decidable:     a row is decidable if every other code v has d64_v - d64_best > b_v + b_best + p_v; there the id must be the fp64 argmin.
                                 Exact ties go to the lowest index: bit-identical codebook rows are one code for the margins (any formula gives them the
                                 same distance), and the id must be the lowest index of the winning group.
  (c) update:                    f_hat[s] - f_hat[s - 1] against h64 = Phi64(bicubic_up64(E[ids_s])) (F.interpolate in double; E[ids_s] itself at the last scale)
                                 within 2e-5 max(1, max|h64|), the bar of test_quant_next_* (the float restatement on the CPU stays at 2.5e-7 .. 3.9e-7).
  (d) outputs:                   ids in [0, V); f_hat_out bit-equal to the last per-scale tensor.
"""
import numpy as np
import torch
import torch.nn.functional as F

from torch_ref_encode import _phi

U = 2.0 ** -24
GAMMA36 = 36 * U / (1 - 36 * U)
UPDATE_BAR = 2e-5


class ChainReport:
    def __init__(self):
        self.scales, self.failures = [], []

    @property
    def ok(self):
        return not self.failures

    @property
    def rows(self):
        return sum(s["rows"] for s in self.scales)

    @property
    def decidable(self):
        """share of all rows that are decidable (a property of the inputs and the fp64 reference alone as long as the chain passes)"""
        return sum(s["n_decidable"] for s in self.scales) / max(1, self.rows)

    def __str__(self):
        out = ["scale  pn  rows  decidable  med|z|^2/best  worst excess/bound  wrong decidable  update err / bar"]
        for s in self.scales:
            out.append(f"{s['scale']:5d} {s['pn']:3d} {s['rows']:5d}  {100 * s['n_decidable'] / s['rows']:8.2f}%  {s['z2_over_best']:13.3g}  "
                       f"{s['worst_excess_over_bound']:18.3g}  {s['wrong_decidable']:15d}  {s['update_err']:.2e} / {s['update_bar']:.2e}")
        out.append(f"all: {self.rows} rows, {100 * self.decidable:.2f} % decidable; " + ("ok" if self.ok else "FAILED: " + "; ".join(self.failures)))
        return "\n".join(out)


def _canonical(E64):
    """canon[v] = the lowest index whose row is bit-identical to row v"""
    _, inv = torch.unique(E64, dim=0, return_inverse=True)
    first = torch.full((int(inv.max()) + 1,), E64.shape[0], dtype=torch.int64)
    first.scatter_reduce_(0, inv, torch.arange(E64.shape[0]), reduce="amin")
    return first[inv]


def nearest_report(z64, E64, ids, delta=0.0):
    """Rules (a) and (b) for rows z64 (N, 32) against the codebook E64 (V, 32), both double, and the tested ids (N,) already known to lie in [0, V).
    -> dict(excess_over_bound (N,), decidable (N,) bool, want (N,) the fp64 argmin (lowest index of its group), z2_over_best (N,))"""
    canon = _canonical(E64)
    e2 = (E64 * E64).sum(1)
    z2 = (z64 * z64).sum(1)
    d = z2[:, None] + e2[None, :] - 2 * z64 @ E64.T
    d = d[:, canon]                                               # identical rows: identical distances, whatever the matrix product's blocking
    best_d, _ = d.min(1)
    want = canon[(d == best_d[:, None]).int().argmax(1)]
    en, zn = e2.sqrt(), z2.sqrt()
    b = GAMMA36 * (zn[:, None] + en[None, :]) ** 2
    b_best = b.gather(1, want[:, None])
    p = 2 * np.sqrt(32.0) * delta * torch.cdist(E64[want], E64) if delta else 0.0
    bound = b + b_best + p
    gap = d - best_d[:, None]
    others = canon[None, :] != want[:, None]
    decidable = ((gap > bound) | ~others).all(1)
    k = ids.view(-1, 1)
    excess = gap.gather(1, k).view(-1)
    bk = bound.gather(1, k).view(-1)
    return dict(excess_over_bound=excess / bk, decidable=decidable, want=want, z2_over_best=z2 / best_d.clamp(min=1e-300))


@torch.no_grad()
def check_chain(f, ids, f_hat_per_scale, vae64, f_hat_out=None, patch_nums=None):
    """f (B, 32, HW, HW) float; ids (B, L) int64 or the list of per-scale (B, pn^2); f_hat_per_scale (S, B, 32, HW, HW) float or a list; vae64: a .double()
    sdvar_amd.vqvae.VQVAE on the CPU holding the codebook and the Phi convolutions; f_hat_out: the final f_hat where the implementation returns one.
    -> ChainReport (report.ok, report.failures, str(report) the per-scale table)."""
    q = vae64.quantize
    pns = tuple(patch_nums or q.v_patch_nums)
    S = len(pns)
    E64 = q.embedding.weight.data
    assert E64.dtype == torch.float64
    V = E64.shape[0]
    f64 = f.detach().cpu().double()
    B, C, H, W = f64.shape
    if not isinstance(ids, (list, tuple)):
        ids = ids.detach().cpu()
        ends = np.cumsum([p * p for p in pns])
        ids = [ids[:, e - p * p:e] for p, e in zip(pns, ends)]
    ids = [t.detach().cpu() for t in ids]
    fh = [t.detach().cpu() for t in f_hat_per_scale]
    rep = ChainReport()
    if len(ids) != S or len(fh) != S:
        rep.failures.append(f"{len(ids)} id tensors and {len(fh)} f_hat tensors for {S} scales")
        return rep
    fmax = f64.abs().max().item()
    prev = torch.zeros_like(f64)
    for s, pn in enumerate(pns):
        last = s == S - 1
        k = ids[s].reshape(-1).long()
        row = dict(scale=s, pn=pn, rows=B * pn * pn, n_decidable=0, z2_over_best=float("nan"), worst_excess_over_bound=float("nan"), wrong_decidable=0,
                   update_err=float("nan"), update_bar=float("nan"))
        rep.scales.append(row)
        if tuple(ids[s].shape) != (B, pn * pn) or ids[s].dtype != torch.int64 or tuple(fh[s].shape) != (B, C, H, W) or fh[s].dtype != torch.float32:
            rep.failures.append(f"scale {s}: ids {tuple(ids[s].shape)} {ids[s].dtype}, f_hat {tuple(fh[s].shape)} {fh[s].dtype}")
            return rep
        if k.min().item() < 0 or k.max().item() >= V:                                                       # (d)
            rep.failures.append(f"scale {s}: ids outside [0, {V}): {k.min().item()} .. {k.max().item()}")
            return rep
        f_rest = f64 - prev
        z = (f_rest if last else F.interpolate(f_rest, size=(pn, pn), mode="area")).permute(0, 2, 3, 1).reshape(-1, C)
        nr = nearest_report(z, E64, k, delta=(s + 1) * 2.0 ** -23 * fmax)
        row["n_decidable"] = int(nr["decidable"].sum())
        row["z2_over_best"] = nr["z2_over_best"].median().item()
        row["worst_excess_over_bound"] = nr["excess_over_bound"].max().item()
        if row["worst_excess_over_bound"] > 1.0:                                                           # (a)
            n = int(nr["excess_over_bound"].argmax())
            rep.failures.append(f"scale {s}: row {n} chose code {k[n].item()}, {row['worst_excess_over_bound']:.3g} x its bound above the fp64 best {nr['want'][n].item()} "
                                f"({int((nr['excess_over_bound'] > 1).sum())} rows over the bound)")
        wrong = nr["decidable"] & (k != nr["want"])                                                        # (b)
        row["wrong_decidable"] = int(wrong.sum())
        if row["wrong_decidable"]:
            n = int(wrong.int().argmax())
            rep.failures.append(f"scale {s}: {row['wrong_decidable']} decidable rows differ from the fp64 argmin (row {n}: {k[n].item()} for {nr['want'][n].item()})")
        hb = E64[ids[s].view(B, pn, pn)].permute(0, 3, 1, 2)                                                 # (c)
        h = _phi(q, s, S, hb.contiguous() if last else F.interpolate(hb, size=(H, W), mode="bicubic"))
        cur = fh[s].double()
        row["update_err"] = ((cur - prev) - h).abs().max().item()
        row["update_bar"] = UPDATE_BAR * max(1.0, h.abs().max().item())
        if not row["update_err"] <= row["update_bar"]:
            rep.failures.append(f"scale {s}: f_hat update differs from Phi64(up64(E[ids])) by {row['update_err']:.3g} (bar {row['update_bar']:.3g})")
        prev = cur
    if f_hat_out is not None and not torch.equal(f_hat_out.detach().cpu(), fh[-1]):                          # (d)
        rep.failures.append("f_hat_out is not bit-equal to the last per-scale f_hat")
    return rep


# ---------------------------------------------------------------------------------------------------- inputs
def _rng(seed):
    return np.random.Generator(np.random.Philox(key=[seed, 777]))


def checkpoint_like_f(B, HW, seed=0):
    """f (B, 32, HW, HW) float with the statistics tests/vae_ckpt_init.checkpoint_like_encoder_state_dict gives quant_conv's output: per-channel offsets ~ U(-3, 3),
    a per-pixel spread of 1 (half of it spatially smooth, so that the coarse scales see more than the offsets), max|f| <= 10."""
    g = _rng(seed)
    off = torch.from_numpy(g.uniform(-3, 3, size=(1, 32, 1, 1)).astype(np.float32))
    fine = torch.from_numpy(g.standard_normal(size=(B, 32, HW, HW), dtype=np.float32))
    coarse = F.interpolate(torch.from_numpy(g.standard_normal(size=(B, 32, 4, 4), dtype=np.float32)), size=(HW, HW), mode="bicubic")
    f = off + (fine + coarse) * 0.5 ** 0.5
    return f.clamp_(-10, 10).contiguous()


def three_decade_codebook(V, seed=0):
    """(V, 32) float: N(0, 1) rows scaled so that the row norms span three decades (0.03 .. 30 around sqrt(32)), the scales in a shuffled order"""
    g = _rng(seed + 1)
    e = g.standard_normal(size=(V, 32), dtype=np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    scale = 10.0 ** (-1.5 + 3.0 * g.permutation(V) / max(1, V - 1))
    return torch.from_numpy((e * scale[:, None]).astype(np.float32))


def quant_model(E, pns, share_quant_resi=4, seed=3, phi_bias_std=0.05):
    """A float VQVAE container (no encoder, a narrow decoder that nobody runs) around the codebook E (V, 32) with the stress init's Phi convolutions and
    N(0, phi_bias_std) Phi biases, in the Phi layout share_quant_resi selects (0: one per scale, 1: one for all, k: k partially shared)."""
    from sdvar_amd.vqvae import VQVAE
    from sdvar_amd.weights import vae_state_dict
    sd = vae_state_dict(tuple(pns), "stress", seed, V=E.shape[0], Cvae=32, ch=32, with_encoder=False, share_quant_resi=share_quant_resi)
    g = _rng(seed + 2)
    for k in sd:
        if "quant_resi" in k and k.endswith(".bias"):
            sd[k] = torch.from_numpy(g.standard_normal(size=tuple(sd[k].shape), dtype=np.float32) * np.float32(phi_bias_std))
    sd["quantize.embedding.weight"] = E.clone()
    vae = VQVAE(vocab_size=E.shape[0], z_channels=32, ch=32, v_patch_nums=tuple(pns), with_encoder=False, share_quant_resi=share_quant_resi)
    vae.load_state_dict(sd)
    return vae
