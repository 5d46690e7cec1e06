"""Teacher-forced VAR.forward without a GPU: its refusals, the PyTorch restatement (tests/torch_ref_tf.py) against the reference fixtures of
tests/golden/make_tf_golden.py, and the all-reduce of sdvar_amd.evaluate's validation sums over gloo with world size 2."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import golden, state_dicts

TF_CASES = ["tf_d4_256_stress", "tf_d4_256_uncond", "tf_d4_512_stress", "tf_d4_256_sharedaln", "tf_d4_256_nol2"]


def _small_var(**kw):
    from sdvar_amd import VAR, VQVAE
    vae = VQVAE(vocab_size=64, ch=32, with_encoder=False, v_patch_nums=(1, 2, 3))
    return VAR(vae, depth=2, embed_dim=128, num_heads=2, patch_nums=(1, 2, 3), **kw)


def test_forward_stores_the_reference_attributes():
    m = _small_var(cond_drop_rate=0.25, drop_path_rate=0.05)
    assert m.cond_drop_rate == 0.25 and m.drop_path_rate == 0.05 and m.drop_rate == 0.0 and m.attn_drop_rate == 0.0
    assert m.prog_si == -1


def test_forward_refuses_cpu_tensors():
    from sdvar_amd.engine import SdvarError
    m = _small_var().eval()
    with pytest.raises(SdvarError, match="cuda"):
        m(torch.tensor([1, 2]), torch.zeros(2, m.L - 1, m.Cvae))


@pytest.mark.parametrize("label_shape,x_shape", [((2,), (2, 14, 32)), ((2,), (3, 13, 32)), ((2,), (2, 13, 16)), ((2, 1), (2, 13, 32))])
def test_forward_refuses_wrong_shapes(label_shape, x_shape):
    from sdvar_amd.engine import SdvarError
    m = _small_var().eval()
    assert m.L - 1 == 13 and m.Cvae == 32
    with pytest.raises(SdvarError, match="must be"):
        m(torch.zeros(label_shape, dtype=torch.int64), torch.zeros(x_shape))


def test_forward_refuses_progressive_training():
    from sdvar_amd.engine import SdvarError
    m = _small_var().eval()
    m.prog_si = 0
    with pytest.raises(SdvarError, match="prog_si"):
        m(torch.tensor([1, 2]), torch.zeros(2, m.L - 1, m.Cvae))


@pytest.mark.parametrize("rate", ["drop_rate", "attn_drop_rate", "drop_path_rate"])
def test_forward_refuses_training_mode_with_dropout(rate):
    from sdvar_amd.engine import SdvarError
    m = _small_var(**{rate: 0.1})
    assert m.training
    with pytest.raises(SdvarError, match=r"\.eval\(\)"):
        m(torch.tensor([1, 2]), torch.zeros(2, m.L - 1, m.Cvae))
    m.eval()                                                     # past that check, the CPU model is refused for its device
    with pytest.raises(SdvarError, match="cuda"):
        m(torch.tensor([1, 2]), torch.zeros(2, m.L - 1, m.Cvae))


@pytest.mark.parametrize("name", TF_CASES)
def test_restatement_matches_reference_fixture(name):
    from oracle import var_oracle as orc
    from torch_ref_tf import tf_logits
    g = golden(name)
    pns, depth = tuple(int(p) for p in g["patch_nums"]), int(g["depth"])
    sd, _ = state_dicts(depth, pns, "stress", int(g["wseed"]), vae=False, shared_aln=bool(g["shared_aln"]), attn_l2_norm=bool(g["attn_l2_norm"]))
    e = golden(str(g["encode"]))
    labels = torch.from_numpy(g["labels"])
    B = labels.shape[0]
    lg = tf_logits(orc.OracleVAR(sd, depth, pns), labels, torch.from_numpy(e["var_input"][:B]))
    tol = 1e-4
    assert np.abs(np.take_along_axis(lg.numpy(), g["top_idx"].astype(np.int64), -1) - g["top_val"]).max() <= tol
    assert np.abs(np.take_along_axis(lg.numpy(), g["rand_idx"].astype(np.int64), -1) - g["rand_val"]).max() <= tol
    assert np.abs(np.stack([lg[b, t].numpy() for b, t in g["rows_bt"]]) - g["rows"]).max() <= tol
    assert np.abs(torch.logsumexp(lg.double(), -1).numpy() - g["lse"]).max() <= tol


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    from sdvar_amd import dist as D
    D.init_from_env("cpu")
    sums = torch.tensor([10.5 * (rank + 1), 2.25 * (rank + 1), 7.0 + rank, 3.0 * rank], dtype=torch.float64)
    out = D.allreduce_eval_sums(sums, 2 + rank)
    np.save(os.path.join(out_dir, f"rank{rank}.npy"), np.array(out))
    torch.distributed.destroy_process_group()


def test_eval_sums_allreduce_gloo(tmp_path):
    world = 2
    mp.start_processes(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True, start_method="spawn")
    for r in range(world):
        got = np.load(tmp_path / f"rank{r}.npy")
        assert np.array_equal(got, np.array([31.5, 6.75, 15.0, 3.0, 5.0])), got


def test_eval_sums_single_process():
    from sdvar_amd import dist as D
    assert D.allreduce_eval_sums(torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64), 3) == (1.0, 2.0, 3.0, 4.0, 3.0)
