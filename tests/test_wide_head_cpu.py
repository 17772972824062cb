"""Answer heads of more than 128 labels (the reference's `vqa` task: 3129) without a GPU: the C ABI of the any-width DAT loss
(declared = exported = bound; argument checks on never-dereferenced pointer values), the task table and what train.main does with
it, and the CPU oracle against the reference's own 3129-label runs (tests/golden/gw1_vilt2_c3129.npz, gw2_loss_c3129.npz, written
by tools/make_widehead_golden.py), so that fixture and oracle agree before any GPU is involved."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from feddat_amd import lib as L
from feddat_amd import vilt_spec
from oracle import feddat_oracle as O
from tests.golden_util import load, max_abs_diff_vs_golden
from tests.test_oracle_golden import TOL_W

torch.set_num_threads(8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("feddat_dat_loss_wide_workspace_elems", "feddat_dat_loss_fwd_bwd_wide")
EINVAL = 1
C = 3129
TASKS = ["art", "gqa"]


def wide_batches(seed0, sizes):
    """Batch s = the first sizes[s] samples of O.synthetic_batch(4, 224, seed0 + s, num_labels=3129)
    (tools/make_widehead_golden.py: batches)."""
    return [{k: v[:n].clone() for k, v in O.synthetic_batch(4, 224, seed0 + s, num_labels=C).items()}
            for s, n in enumerate(sizes)]


def wide_loss_inputs(B, Cn, seed):
    """(logits, teacher, target) of a gw2 case from its seed (tools/make_widehead_golden.py: wide_loss_inputs)."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, Cn, generator=g) * 2
    teacher = torch.randn(B, Cn, generator=g) * 2
    return logits, teacher, O.synthetic_batch(B, 32, seed, num_labels=Cn)["target_scores"]


@pytest.mark.parametrize("f16", [False, True])
def test_new_symbols_declared_exported_bound_and_checked(f16):
    from feddat_amd import build
    src = open(os.path.join(ROOT, "include", "feddat_hip.h")).read()
    lib = ctypes.CDLL(build.build(f16=f16))
    for n in NEW_SYMBOLS:
        assert re.search(rf"^(?:int|long) {n}\(", src, flags=re.M), n
        assert n in L.EXPORTED_SYMBOLS and hasattr(lib, n), n
    assert hasattr(L, "dat_loss_fwd_bwd_wide") and hasattr(L, "dat_loss_wide_workspace_elems")
    assert lib.feddat_abi_version() == 8 == L.ABI_VERSION
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    ws = lib.feddat_dat_loss_wide_workspace_elems
    ws.argtypes, ws.restype = [i32], i64
    assert [ws(b) for b in (1, 4, 32, 65, 4096)] == [2, 8, 64, 130, 8192] and ws(0) == 0 and ws(-3) == 0
    fn = lib.feddat_dat_loss_fwd_bwd_wide
    fn.argtypes, fn.restype = [vp, vp, vp, i32, i32, i32, f32, vp, vp, vp, vp, i64, vp], i32
    X, D, S, W = 0x1000, 0x2000, 0x3000, 0x4000      # never dereferenced: every call below is refused by the argument checks

    def call(x=X, t=X, y=X, n=4, B=4, Cn=C, temp=3.0, dl=D, sc=S, flag=None, w=W, elems=8):
        return fn(x, t, y, n, B, Cn, temp, dl, sc, flag, w, elems, None)
    for null in ("x", "t", "y", "dl", "sc", "w"):
        assert call(**{null: None}) == EINVAL, null
    assert call(n=0) == EINVAL and call(n=-1) == EINVAL
    assert call(n=5) == EINVAL                                     # n > B
    assert call(n=4, B=4097, elems=2 * 4097) == EINVAL             # B > 4096
    assert call(Cn=0) == EINVAL
    assert call(elems=7) == EINVAL                                 # a workspace one element short
    assert call(temp=0.0) == EINVAL


def test_wide_op_needs_a_device():
    """CPU tensors are refused before the library is touched: there is no host path."""
    z = torch.zeros(2, 300)
    with pytest.raises(L.FeddatHipError):
        L.dat_loss_fwd_bwd_wide(z, z, z, torch.zeros(2, 300), torch.zeros(4), torch.zeros(4))


def test_task_table_and_main():
    from feddat_amd import train
    assert vilt_spec.TASK_NUM_LABELS["vqa"] == 3129
    for t in [t for ts in train.TASK_SETS.values() for t in ts]:
        assert vilt_spec.TASK_NUM_LABELS[t] == 100, t
    assert vilt_spec.task_num_labels("some_new_task") == 100
    assert train.federation_num_labels(["vqa"]) == 3129 and train.federation_num_labels(["art", "gqa", "mine"]) == 100
    with pytest.raises(L.FeddatHipError, match="one engine has one width"):
        train.federation_num_labels(["art", "vqa"])
    with pytest.raises(L.FeddatHipError, match="one engine has one width"):      # refused before any device is touched
        train.main(["--ordered_cl_tasks", "vqa,art"])
    for mode in ("dat", "adapter", "bias", "norm"):
        P = vilt_spec.random_init(2, ["vqa"], seed=1, optimizer_mode=mode, num_labels=vilt_spec.task_num_labels("vqa"))
        assert tuple(P["task_layer.vqa.clf_fc1.weight"].shape) == (3129, 1536)
        assert tuple(P["task_layer.vqa.clf_fc1.bias"].shape) == (3129,)
    # the default width draws what it drew before the table existed
    a, b = vilt_spec.random_init(2, ["art"], seed=3), vilt_spec.random_init(2, ["art"], seed=3, num_labels=100)
    assert all(torch.equal(a[k], b[k]) for k in a) and tuple(a["task_layer.art.clf_fc1.bias"].shape) == (100,)
    bt = vilt_spec.synthetic_batch(2, 32, 5, num_labels=3129)
    assert tuple(bt["target_scores"].shape) == (2, 3129)


def test_flat_group_holds_whole_quads():
    """A 3129-label head has 5 993 529 floats: its flat buffers are padded to a whole number of 16-byte quads (the multi-group
    AdamW's unit); a 100-label head needs no padding and keeps its size."""
    from feddat_amd.local_update import FlatGroup
    from feddat_amd.vilt_backbone import HEAD_TENSORS
    for labels, numel, alloc in ((100, 1337956, 1337956), (3129, 5993529, 5993532)):
        shapes = {"clf_fc0.weight": (1536, 768), "clf_fc0.bias": (1536,), "clf_norm0.weight": (1536,), "clf_norm0.bias": (1536,),
                  "clf_fc1.weight": (labels, 1536), "clf_fc1.bias": (labels,)}
        g = FlatGroup([(n, shapes[n]) for n in HEAD_TENSORS], "cpu", True)
        assert g.numel == numel and g.p.numel() == alloc == g.g.numel() == g.m.numel() == g.v.numel()
        assert g.view("clf_fc1.bias").shape == (labels,) and int(g.seg_off[-1]) == numel
        assert g.offsets["clf_fc1.bias"] + labels == numel


def test_oracle_replays_gw2(golden_dir):
    """The bounds of test_g2_loss; the loss itself, ~1.7e3 at 3129 labels, to 2e-6 relative (fp32 resolution) on top."""
    g = load(golden_dir, "gw2_loss_c3129.npz")
    assert g["shapes"].tolist() == [[4, 3129, 31], [5, 129, 32]]
    for B, Cn, seed in g["shapes"].tolist():
        logits, teacher, target = wide_loss_inputs(B, Cn, seed)
        lg = logits.requires_grad_(True)
        loss = O.dat_loss(lg, target, teacher)
        loss.backward()
        p = f"{B}x{Cn}."
        assert abs(float(loss.detach()) - float(g[p + "L"])) < 1e-4 + 2e-6 * abs(float(g[p + "L"]))
        assert abs(float(O.kl_loss(lg.detach(), teacher)) - float(g[p + "kl"])) < 1e-5
        assert (lg.grad - torch.from_numpy(g[p + "dlogits"])).abs().max() < 1e-6


def _stored(g, pre):
    keys = [k[len(pre):] for k in g if k.startswith(pre) and "::" not in k]
    return keys + [k.split("::", 1)[1][len(pre):] for k in g if k.startswith("samp::" + pre)]


def test_oracle_replays_gw1(golden_dir):
    """The bounds of test_g3_two_layer_forward_and_steps: pooled 5e-6, logits 5e-5, losses rtol 2e-5 (the 3129-label BCE term is
    ~2e3, so the absolute allowance is immaterial), every stored fp32 tensor within TOL_W; the update stored as float16 of
    dW * 256 within TOL_W as well."""
    g = load(golden_dir, "gw1_vilt2_c3129.npz")
    assert int(g["num_labels"]) == C and g["tasks"].tolist() == TASKS
    d = O.ViltDims(layers=2, num_labels=C)
    P = O.make_params(d, TASKS, bias_std=0.02)
    P0 = {k: v.clone() for k, v in P.items()}
    b0 = O.synthetic_batch(4, 224, 1234, num_labels=C)
    with torch.no_grad():
        for mode in ("gating", "adapter_1", "adapter_0"):
            pooled, lg = O.vilt_forward(P, d, b0, mode, "art")
            assert tuple(lg.shape) == (4, C)
            assert (pooled - torch.from_numpy(g[f"fwd.{mode}.pooled"])).abs().max() < 5e-6
            assert (lg - torch.from_numpy(g[f"fwd.{mode}.logits"])).abs().max() < 5e-5
    for tag, sizes in (("full", (4, 4, 4, 4)), ("short", (4, 4, 3))):
        assert g[tag + ".sizes"].tolist() == list(sizes)
        P = {k: v.clone() for k, v in P0.items()}
        client = O.DatClient(P, d, "art", lr=1e-4, steps_per_epoch=len(sizes))
        losses, kls = [], []
        for s, b in enumerate(wide_batches(1234, sizes)):
            loss0, logits_all, logits_1, logits_0 = client.train_step(b)
            losses.append(float(loss0))
            kls.append([float(O.kl_loss(logits_1, logits_all)), float(O.kl_loss(logits_0, logits_1))])
            pre = f"{tag}.after{s + 1}."
            keys = _stored(g, pre)
            assert bool(keys) == (s + 1 == len(sizes) or (tag == "full" and s == 0))
            for k in keys:
                assert max_abs_diff_vs_golden(g, pre + k, P[k]) < TOL_W, (pre, k)
            for k in [k[len(pre + "dall::"):] for k in g if k.startswith(pre + "dall::")]:
                ref = torch.from_numpy(g[pre + "dall::" + k].astype(np.float32)) / 256.0
                assert float(((P[k] - P0[k]) - ref).abs().max()) < TOL_W, (pre, k)
        assert np.allclose(losses, g[tag + ".losses"], rtol=2e-5, atol=1e-4), (losses, g[tag + ".losses"])
        # the KL terms are ~5e-4 .. 2e-3 here (the two passes differ by a few adapter steps); two runs of the reference itself
        # differ by 1e-3 relative in them (HF permutes the image patches at random on every forward)
        assert np.allclose(kls, g[tag + ".kl"], rtol=2e-2, atol=2e-6), (kls, g[tag + ".kl"])
    assert len([k for k in g if k.startswith("full.after4.dall::")]) == 16
    assert len(_stored(g, "adapter.after4.")) == 6 + 8 and len(g["adapter.losses"]) == 4
