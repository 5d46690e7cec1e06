"""tests/quant_chain_check.py on the CPU: the harness accepts the PyTorch restatement of the residual quantisation (tests/torch_ref_encode.py) on
checkpoint-like f with an N(0, 1) codebook and with one whose row norms span three decades, on both ladders, and rejects seven mutants of it.

Conditions (from the inputs and the fp64 reference alone): at least 95 % of all rows are decidable; code V - 1 and a planted duplicate pair are decidable
winners of scale 0 (so that "the last code never considered" and "ties to the highest index" have something to get wrong)."""
import pytest
import torch
import torch.nn.functional as F

from quant_chain_check import check_chain, checkpoint_like_f, quant_model, three_decade_codebook
from sdvar_amd.ladder import LADDER_256, LADDER_512
from torch_ref_encode import _phi, f_to_idxBl_or_fhat_torch

V = 512
MUTANTS = ["skip_last_code", "ties_to_highest", "e2_of_other_codebook", "phi_bias_dropped", "f_rest_not_updated", "bilinear_down", "last_scale_transposed"]


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(16)
    yield
    torch.set_num_threads(n)


def _case(pns, book, B=2):
    """f, the float model, its .double() copy.  Planted from f alone: code V - 1 sits next to image 0's scale-0 row (the mean of f[0] over the pixels), codes 5
    and V - 2 are one vector next to image 1's."""
    f = checkpoint_like_f(B, pns[-1], seed=len(pns) + pns[-1])
    E = three_decade_codebook(V, 4) if book == "decades" else torch.randn(V, 32, generator=torch.Generator().manual_seed(9))
    z0 = f.double().mean((2, 3)).float()
    E[V - 1] = z0[0] + 1e-3
    E[5] = z0[1] - 1e-3
    E[V - 2] = E[5]
    vae = quant_model(E, pns)
    return f, vae, quant_model(E, pns).double()


@torch.no_grad()
def chain(vae, f, mutant=None):
    """f_to_idxBl_or_fhat_torch restated with one switch per mutant -> (ids per scale, f_hat per scale)"""
    q = vae.quantize
    pns = q.v_patch_nums
    B, C, H, W = f.shape
    E = q.embedding.weight.data
    f_rest, f_hat, ids, fhs = f.clone(), torch.zeros_like(f), [], []
    SN = len(pns)
    for si, pn in enumerate(pns):
        if si == SN - 1:
            z = f_rest.permute(0, 3, 2, 1) if mutant == "last_scale_transposed" else f_rest.permute(0, 2, 3, 1)
        elif mutant == "bilinear_down":
            z = F.interpolate(f_rest, size=(pn, pn), mode="bilinear").permute(0, 2, 3, 1)
        else:
            z = F.interpolate(f_rest, size=(pn, pn), mode="area").permute(0, 2, 3, 1)
        z = z.reshape(-1, C)
        E2 = E.flip(0) if mutant == "e2_of_other_codebook" else E
        d = torch.sum(z.square(), dim=1, keepdim=True) + torch.sum(E2.square(), dim=1, keepdim=False)
        d.addmm_(z, E.T, alpha=-2, beta=1)
        if mutant == "skip_last_code":
            d = d[:, :-1]
        idx = (d.shape[1] - 1 - torch.argmin(d.flip(1), dim=1)) if mutant == "ties_to_highest" else torch.argmin(d, dim=1)
        hb = E[idx.view(B, pn, pn)].permute(0, 3, 1, 2)
        h = F.interpolate(hb, size=(H, W), mode="bicubic") if si != SN - 1 else hb.contiguous()
        h = _phi(q, si, SN, h)
        if mutant == "phi_bias_dropped":
            from torch_ref_encode import _phis
            from sdvar_amd.ladder import phi_index
            phis = _phis(q)
            m = phis[phi_index(si, SN, len(phis))] if len(phis) > 1 else phis[0]
            h = h - 0.5 * m.bias.data.view(1, -1, 1, 1)
        f_hat.add_(h)
        if mutant != "f_rest_not_updated":
            f_rest.sub_(h)
        ids.append(idx.reshape(B, pn * pn))
        fhs.append(f_hat.clone())
    return ids, fhs


@pytest.mark.parametrize("book", ["normal", "decades"])
@pytest.mark.parametrize("pns", [LADDER_256, LADDER_512], ids=["ladder256", "ladder512"])
def test_harness_accepts_the_restatement(pns, book):
    f, vae, vae64 = _case(pns, book)
    ids = f_to_idxBl_or_fhat_torch(vae, f, False)
    fhs = f_to_idxBl_or_fhat_torch(vae, f, True)
    rep = check_chain(f, ids, fhs, vae64, f_hat_out=fhs[-1])
    print(f"\n{book} codebook, ladder {pns}\n{rep}")
    assert rep.decidable >= 0.95, rep.decidable
    assert rep.ok, rep.failures
    assert ids[0].view(-1).tolist() == [V - 1, 5]                                   # the planted winners, decidable
    assert rep.scales[0]["n_decidable"] == 2
    mine = chain(vae, f)                                                             # the mutants' base is the restatement, bit for bit
    assert all(torch.equal(a, b) for a, b in zip(mine[0], ids)) and all(torch.equal(a, b) for a, b in zip(mine[1], fhs))
    assert check_chain(f, torch.cat(ids, 1), torch.stack(fhs), vae64).ok            # the other accepted input form


@pytest.mark.parametrize("mutant", MUTANTS)
@pytest.mark.parametrize("book", ["normal", "decades"])
def test_harness_rejects_mutants(book, mutant):
    f, vae, vae64 = _case(LADDER_256, book)
    ids, fhs = chain(vae, f, mutant)
    rep = check_chain(f, ids, fhs, vae64, f_hat_out=fhs[-1])
    print(f"\n{mutant}: {rep.failures}")
    assert not rep.ok


def test_harness_rejects_bad_outputs():
    f, vae, vae64 = _case(LADDER_256, "normal")
    ids, fhs = chain(vae, f)
    bad = [t.clone() for t in ids]
    bad[3][0, 2] = V
    assert "outside" in check_chain(f, bad, fhs, vae64).failures[0]
    bad[3][0, 2] = -1
    assert "outside" in check_chain(f, bad, fhs, vae64).failures[0]
    out = fhs[-1].clone()
    out[0, 0, 0, 0] = torch.nextafter(out[0, 0, 0, 0], torch.tensor(100.0))
    assert "bit-equal" in check_chain(f, ids, fhs, vae64, f_hat_out=out).failures[-1]
    assert check_chain(f, ids[:-1], fhs[:-1], vae64).failures
