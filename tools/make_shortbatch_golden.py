"""Generate the short-last-batch fixtures (tests/golden/gs1_short_*.npz) by running the reference's own train_step over a
loader whose last batch is short, as its loaders yield whenever len(dataset) % batch_size != 0 (no drop_last:
vqa_dataset_crossvqa.py:509-515; the step is counted in max_steps, train_vqa_crossvqa.py:238).

Setup: 2 layers, 224 x 224, B = 4, tasks ["art", "gqa"], one local update (one pass over the loader, the poly schedule over
3 x 15 ticks as in g3 / ga1 / gv1) over batches of 4, 4 and 3 samples.  The last batch is the first three samples of its
seed's batch.  Seeds per mode as the mode's own 2-layer fixture uses them: dat 1234 + s (g3), adapter and bias / norm
2000 + s (ga1, gv1).

Stored per file: the three losses and every trainable tensor after step 3, in the packed forms of g3 / ga1 / gv1.  The dat
file holds its adapters twice: in g3's fp32 form (biases whole, weights as norm + 2048 strided samples: what the CPU oracle
is pinned to, at g3's bound) and every element of their update as ga1 stores it (float16 of dW * 256: what the engine is
compared with, element by element).  Every element in fp32 as well would make the file larger than 1 MiB.

The shims, model builders and storage helpers are imported read-only from oracle/make_golden.py,
tools/make_adapter_golden.py and tools/make_vector_golden.py; this script writes numeric arrays and name lists to
tests/golden/ only.

    python tools/make_shortbatch_golden.py [dat adapter bias norm]     (default: all four)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import make_golden as MG  # noqa: E402  (installs the shims on import)
from oracle import feddat_oracle as O  # noqa: E402
from oracle.make_golden import np_, put  # noqa: E402
import make_adapter_golden as MA  # noqa: E402
import make_vector_golden as MV  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
TASKS = ["art", "gqa"]
SIZES = (4, 4, 3)
SEED0 = {"dat": 1234, "adapter": 2000, "bias": 2000, "norm": 2000}


def short_batches(mode):
    """Batches of SIZES samples: batch s is the first SIZES[s] samples of O.synthetic_batch(4, 224, SEED0[mode] + s)."""
    out = []
    for s, n in enumerate(SIZES):
        b = O.synthetic_batch(4, 224, SEED0[mode] + s)
        out.append({k: v[:n].clone() for k, v in b.items()})
    return out


def header(mode, losses):
    return {"losses": np.array(losses, np.float32), "sizes": np.array(SIZES, np.int64), "seed0": np.array(SEED0[mode])}


def put_sampled(rec, key, t):
    """g3's form for large tensors (oracle/make_golden.py: put), also below put()'s size threshold."""
    flat = t.detach().float().flatten()
    if flat.numel() <= MG.N_SAMPLES:
        return put(rec, key, t)
    idx = torch.linspace(0, flat.numel() - 1, MG.N_SAMPLES).long()
    rec["samp::" + key] = np_(flat[idx])
    rec["norm::" + key] = np_(flat.norm())


def golden_dat():
    model = MG.build_reference_model(O.ViltDims(layers=2), TASKS, bias_std=0.02)
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    losses, _ = MG.ref_local_update(model, "art", short_batches("dat"), lr=1e-4)
    rec = header("dat", losses)
    for k, v in model.state_dict().items():
        if "adapter_0" in k or "adapter_1" in k:
            put_sampled(rec, "after3." + k, v)
            rec["after3.dall::" + k] = ((v.detach() - init[k]) * 256.0).to(torch.float16).numpy()
        elif k.startswith("task_layer.art."):
            put(rec, "after3." + k, v)
    return rec


def golden_adapter():
    model = MA.build_adapter_model(O.ViltDims(layers=2), TASKS)
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    losses, _ = MA.local_update(model, "art", short_batches("adapter"))
    rec = header("adapter", losses)
    for k, v in model.state_dict().items():
        if not MA.trainable(k):
            continue
        if "adapter" in k:      # every element of the update, as float16 of dW * 256 (ga1's encoding)
            rec["after3.dall::" + k] = ((v.detach() - init[k]) * 256.0).to(torch.float16).numpy()
        else:
            put(rec, "after3." + k, v)
    return rec


def golden_vector(mode):
    model = MV.build_model(O.ViltDims(layers=2), TASKS, mode)
    train = {n for n, p in model.named_parameters() if p.requires_grad}
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    losses = MV.local_update(model, mode, "art", short_batches(mode))
    rec = header(mode, losses)
    for k, v in model.state_dict().items():
        if k not in train:
            continue
        if k.startswith("task_layer."):
            if k.startswith("task_layer.art."):
                put(rec, "after3." + k, v)
            else:      # the other task's head is in the optimizer but gets no gradient: it must not have moved
                assert torch.equal(v, init[k]), k
        else:           # every element of the vector's update (gv1's encoding)
            rec["after3.d::" + k] = np_(v.detach() - init[k])
    return rec


if __name__ == "__main__":
    which = sys.argv[1:] or ["dat", "adapter", "bias", "norm"]
    torch.manual_seed(0)
    for w in which:
        rec = golden_dat() if w == "dat" else golden_adapter() if w == "adapter" else golden_vector(w)
        path = os.path.join(OUT, f"gs1_short_{w}.npz")
        np.savez_compressed(path, **rec)
        print(w, "losses", rec["losses"].tolist(), os.path.getsize(path), "bytes")
