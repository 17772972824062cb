"""Generate the wide-head fixtures (tests/golden/gw1_vilt2_c3129.npz, gw2_loss_c3129.npz) by running the reference's own modules
with num_labels = 3129, the width of its `vqa` task (src/configs/task_configs_fed.py) on the same VQATrainerCross step as the
100-label tasks.

gw1: 2 layers, 224 x 224, B = 4, tasks ["art", "gqa"] with 3129-label heads.
  fwd.<mode>.{pooled,logits}       forward of the three adapter settings (gating, adapter_1, adapter_0) on batch 1234
  full.*                           optimizer_mode dat, one 4-step local update (seeds 1234 + s, poly schedule over 4 x 15 ticks):
                                   losses (loss_0 per step), kl ([step, {P1, P2}]: what the reference's kl_loss returned),
                                   after1.* / after4.* every trainable tensor
  short.*                          the same over batches of 4 / 4 / 3 samples (3 x 15 ticks): losses, kl, after3.*
  adapter.*                        optimizer_mode adapter (seeds 2000 + s), 4 steps: losses, after4.*
Adapters: full.after4 holds every element of the update as float16 of dW * 256 (`dall::`, ga1's encoding); the other snapshots
hold g3's form (norm + 2048 strided samples of the weights, biases whole) -- every element at every snapshot is 1.6 MB, more
than a committed file may have.  Heads: put()'s whole / sampled form (clf_fc1.weight is 4.8 M floats).

gw2: the reference's kl_loss and BCEWithLogits (task_trainer.py:299-301, 506-516) with their autograd dlogits at [4, 3129] and
[5, 129]; the inputs are stored as seeds (wide_loss_inputs below regenerates them).

The shims, model builders and storage helpers are imported read-only from oracle/make_golden.py, tools/make_adapter_golden.py and
tools/make_shortbatch_golden.py; this script writes numeric arrays and name lists to tests/golden/ only.

    python tools/make_widehead_golden.py [gw1 gw2]     (default: both)
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import make_golden as MG  # noqa: E402  (installs the shims on import)
from oracle import feddat_oracle as O  # noqa: E402
from oracle.make_golden import np_, put  # noqa: E402
import make_adapter_golden as MA  # noqa: E402
from make_shortbatch_golden import put_sampled  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
C = 3129
TASKS = ["art", "gqa"]
SIZES = (4, 4, 3)
GW2_SHAPES = ((4, 3129, 31), (5, 129, 32))      # (B, C, seed)


def dims():
    return O.ViltDims(layers=2, num_labels=C)


def batches(seed0, sizes):
    out = []
    for s, n in enumerate(sizes):
        b = O.synthetic_batch(4, 224, seed0 + s, num_labels=C)
        out.append({k: v[:n].clone() for k, v in b.items()})
    return out


def wide_loss_inputs(B, Cn, seed):
    """(logits, teacher, target) of a gw2 case from its seed."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, Cn, generator=g) * 2
    teacher = torch.randn(B, Cn, generator=g) * 2
    target = O.synthetic_batch(B, 32, seed, num_labels=Cn)["target_scores"]
    return logits, teacher, target


def store(rec, pre, model, init, whole):
    for k, v in model.state_dict().items():
        if "active_adapter" in k:
            continue
        if ("adapter_0" in k or "adapter_1" in k or ".adapter.adapter_down" in k or ".adapter.adapter_up" in k):
            if whole:
                rec[pre + "dall::" + k] = ((v.detach() - init[k]) * 256.0).to(torch.float16).numpy()
            else:
                put_sampled(rec, pre + k, v)
        elif k.startswith("task_layer.art."):
            put(rec, pre + k, v)


def dat_update(rec, tag, sizes):
    import src.train.visionlanguage_tasks.task_trainer as TT
    model = MG.build_reference_model(dims(), TASKS, bias_std=0.02)
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    kls, orig = [], TT.kl_loss

    def recording_kl(*a, **k):
        out = orig(*a, **k)
        kls.append(float(out.detach()))
        return out

    def cap(step, m):
        if step + 1 == len(sizes):
            store(rec, f"{tag}.after{step + 1}.", m, init, whole=tag == "full")
        elif step == 0 and tag == "full":
            store(rec, f"{tag}.after1.", m, init, whole=False)
    TT.kl_loss = recording_kl
    try:
        losses, _ = MG.ref_local_update(model, "art", batches(1234, sizes), lr=1e-4, capture=cap)
    finally:
        TT.kl_loss = orig
    assert len(kls) == 2 * len(sizes), len(kls)
    rec[tag + ".losses"] = np.array(losses, np.float32)
    rec[tag + ".kl"] = np.array(kls, np.float32).reshape(len(sizes), 2)
    rec[tag + ".sizes"] = np.array(sizes, np.int64)
    print(tag, "losses", losses, "kl", kls)


def golden_gw1():
    rec = {"num_labels": np.array(C), "tasks": np.array(TASKS)}
    model = MG.build_reference_model(dims(), TASKS, bias_std=0.02)
    b0 = O.synthetic_batch(4, 224, 1234, num_labels=C)
    with torch.no_grad():
        for mode in ("gating", "adapter_1", "adapter_0"):
            if mode == "gating":
                model.activate_gating()
            else:
                model.deactivate_gating()
                model.set_active_adapter(mode)
            pooled, lg = model(task_key="art", images=MG._enc_only(b0), texts=None)
            rec[f"fwd.{mode}.pooled"], rec[f"fwd.{mode}.logits"] = np_(pooled), np_(lg)
    dat_update(rec, "full", (4, 4, 4, 4))
    dat_update(rec, "short", SIZES)
    # optimizer_mode adapter
    am = MA.build_adapter_model(dims(), TASKS)
    init = {k: v.detach().clone() for k, v in am.state_dict().items()}
    losses, _ = MA.local_update(am, "art", batches(2000, (4, 4, 4, 4)))
    rec["adapter.losses"] = np.array(losses, np.float32)
    store(rec, "adapter.after4.", am, init, whole=False)
    print("adapter losses", losses)
    path = os.path.join(OUT, "gw1_vilt2_c3129.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")


def golden_gw2():
    rec = {"shapes": np.array(GW2_SHAPES, np.int64)}
    for B, Cn, seed in GW2_SHAPES:
        logits, teacher, target = wide_loss_inputs(B, Cn, seed)
        logits.requires_grad_(True)
        bce = nn.BCEWithLogitsLoss(reduction="mean")(logits, target) * target.shape[1]
        kl = MG.kl_loss(logits, teacher.clone().detach())
        L = (bce + kl) / 2
        L.backward()
        p = f"{B}x{Cn}."
        rec[p + "bce"], rec[p + "kl"], rec[p + "L"], rec[p + "dlogits"] = np_(bce), np_(kl), np_(L), np_(logits.grad)
        print("gw2", B, Cn, float(bce), float(kl))
    path = os.path.join(OUT, "gw2_loss_c3129.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    which = sys.argv[1:] or ["gw1", "gw2"]
    torch.manual_seed(0)
    for w in which:
        globals()["golden_" + w]()
