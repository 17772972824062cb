"""Host-side pieces of the short last batch (no GPU): the CPU oracle against the reference's own 4 / 4 / 3 local update
(tests/golden/gs1_short_dat.npz, written by tools/make_shortbatch_golden.py), the --synthetic_last_batch option, and the new
bindings without a device.  (That the new symbols are declared, exported and bound is what tests/test_cabi_cpu.py checks for every
symbol of include/feddat_hip.h.)"""
import numpy as np
import pytest
import torch

from feddat_amd import lib as L
from oracle import feddat_oracle as O
from tests.golden_util import load, max_abs_diff_vs_golden
from tests.test_oracle_golden import TOL_W

torch.set_num_threads(8)
SIZES = (4, 4, 3)


def short_batches(seed0, sizes=SIZES, res=224):
    """Batch s = the first sizes[s] samples of O.synthetic_batch(4, res, seed0 + s) (tools/make_shortbatch_golden.py)."""
    return [{k: v[:n].clone() for k, v in O.synthetic_batch(4, res, seed0 + s).items()} for s, n in enumerate(sizes)]


def test_oracle_reproduces_the_reference_on_a_short_last_batch(golden_dir):
    """The bounds of test_g3_two_layer_forward_and_steps: losses rtol 2e-5 / atol 1e-4, every stored fp32 tensor (heads and
    adapters, whole or norm + 2048 samples) within TOL_W."""
    g = load(golden_dir, "gs1_short_dat.npz")
    assert g["sizes"].tolist() == list(SIZES)
    d = O.ViltDims(layers=2)
    P = O.make_params(d, ["art", "gqa"], bias_std=0.02)
    client = O.DatClient(P, d, "art", lr=1e-4, steps_per_epoch=3)
    losses = [float(client.train_step(b)[0]) for b in short_batches(int(g["seed0"]))]
    assert np.allclose(losses, g["losses"], rtol=2e-5, atol=1e-4), (losses, g["losses"])
    keys = [k[len("after3."):] for k in g if k.startswith("after3.") and "::" not in k]
    keys += [k.split("::", 1)[1][len("after3."):] for k in g if k.startswith("samp::after3.")]
    assert len(keys) == 6 + 16 and sum("adapter_0" in k or "adapter_1" in k for k in keys) == 16
    for k in keys:
        assert max_abs_diff_vs_golden(g, "after3." + k, P[k]) < TOL_W, k


def test_parser_accepts_synthetic_last_batch():
    from feddat_amd import train
    p = train.build_parser()
    assert p.parse_args([]).synthetic_last_batch == 0
    assert p.parse_args(["--synthetic_last_batch", "3"]).synthetic_last_batch == 3


def test_main_refuses_a_short_last_batch_where_it_cannot_run():
    from feddat_amd import train
    with pytest.raises(L.FeddatHipError, match="ViLT option"):
        train.main(["--encoder_name", "albef_no_distill", "--synthetic_last_batch", "3", "--batch_size", "4"])
    for n in ("5", "-1"):
        with pytest.raises(L.FeddatHipError, match="1 .. batch_size"):
            train.main(["--synthetic_last_batch", n, "--batch_size", "4"])


def test_short_batch_ops_need_a_device():
    """CPU tensors are refused before the library is touched: there is no host path."""
    z = torch.zeros(2, 3)
    with pytest.raises(L.FeddatHipError):
        L.dat_loss_fwd_bwd_rows(z, z, z, torch.zeros(2, 3), torch.zeros(4), 1)
    with pytest.raises(L.FeddatHipError):
        L.bce_loss_fwd_bwd_rows(z, z, torch.zeros(2, 3), torch.zeros(4), 1)
    inp = dict(input_ids=torch.zeros(2, 4, dtype=torch.int64), token_type_ids=torch.zeros(2, 4, dtype=torch.int64),
               attention_mask=torch.zeros(2, 4, dtype=torch.int64), patch_mask=torch.zeros(2, 1, 1, dtype=torch.int64),
               target=torch.zeros(2, 3))
    with pytest.raises(L.FeddatHipError):
        L.vilt_pad_batch(torch.zeros(2, 3072, dtype=torch.float16), inp, 1, 2)
    for name in ("feddat_vilt_pad_batch", "feddat_dat_loss_fwd_bwd_rows", "feddat_bce_loss_fwd_bwd_rows"):
        assert name in L.EXPORTED_SYMBOLS
    assert L.ABI_VERSION == 8
