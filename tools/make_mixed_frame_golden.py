"""Generate the mixed-frame fixture tests/golden/gm1_mixed_frame.npz by running the reference's own modules: one 384 x 384 frame
that holds a portrait, a landscape, a square and a small landscape image (pixel_mask with zeros) plus ragged questions.  HF
ViltEmbeddings.visual_embed, as the reference calls it, keeps only each sample's valid patches and pads the batch to its
largest valid count: the reference runs these batches at S = 40 + 1 + 84 = 125 where the grid frame holds 185 positions.

The shims, model builders, trainer set-up and storage helpers are imported read-only from oracle/make_golden.py and
tools/make_vector_golden.py; this script writes to tests/golden/ only, numeric arrays and name lists.

    python tools/make_mixed_frame_golden.py
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
import make_vector_golden as MV  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
GM1 = dict(res=384, batch=4, layers=2, seed0=7000, valid=[(384, 224), (224, 384), (288, 288), (160, 320)],
           text=[40, 31, 40, 12])


def gm1_batches():
    c = GM1
    return [O.pad_batch(O.synthetic_batch(c["batch"], c["res"], c["seed0"] + s), c["valid"], c["text"]) for s in range(2)]


def golden_gm1():
    """2 layers, B = 4.  dat (golden_g6's protocol): pooled and logits of the gating and adapter_1 passes on batch 0, the losses
    of two train_steps, the layer-1 adapter tensors after step 2.  bias (golden_gv1's protocol): pooled, logits, loss, the fp32
    gradient of every trainable tensor (g::) and its bf16-autocast twin (g16::) on batch 0, then four steps over the two batches
    (0, 1, 0, 1): every trainable tensor after steps 1 and 4.  Also the batches' patch masks and the valid patch counts."""
    c = GM1
    d = O.ViltDims(layers=c["layers"])
    batches = gm1_batches()
    pm = batches[0]["pixel_mask"][:, ::32, ::32]
    rec = {"patch_mask": pm.numpy().astype(np.int64), "valid": np.array(c["valid"]), "text": np.array(c["text"]),
           "seed0": np.array(c["seed0"]), "counts": pm.reshape(c["batch"], -1).sum(1).numpy().astype(np.int64)}
    assert rec["counts"].tolist() == [84, 84, 81, 50]
    # ---- dat
    model = MG.build_reference_model(d, ["art"], bias_std=0.02)
    seen = []
    hook = model.vilt_encoder.vilt.encoder.register_forward_pre_hook(lambda m, a: seen.append(tuple(a[0].shape)))
    with torch.no_grad():
        for mode in ("gating", "adapter_1"):
            if mode == "gating":
                model.activate_gating()
            else:
                model.deactivate_gating()
                model.set_active_adapter(mode)
            pooled, lg = model(task_key="art", images=MG._enc_only(batches[0]), texts=None)
            rec[f"dat.fwd.{mode}.pooled"], rec[f"dat.fwd.{mode}.logits"] = np_(pooled), np_(lg)
    hook.remove()
    print("GM1 encoder input", seen[0])
    assert seen and all(s == (c["batch"], 40 + 1 + 84, 768) for s in seen), seen
    rec["encoder_seq"] = np.array(seen[0][1])
    for n, p in model.named_parameters():
        if "adapter" in n:
            p.requires_grad = True
    losses, _ = MG.ref_local_update(model, "art", batches, lr=1e-4)
    rec["dat.losses"] = np.array(losses, np.float32)
    for k, v in model.state_dict().items():
        if ".layer.1." in k and ("adapter_0" in k or "adapter_1" in k):
            put(rec, "dat.after2." + k, v)
    print("GM1 dat losses", losses)
    # ---- bias
    pre = "bias."
    model = MV.build_model(d, ["art"], "bias")
    with torch.no_grad():
        pooled, logits = model(task_key="art", images=MG._enc_only(batches[0]), texts=None)
    rec[pre + "fwd.pooled"], rec[pre + "fwd.logits"] = np_(pooled), np_(logits)
    loss, g = MV.gradients(model, batches[0], False)
    _, g16 = MV.gradients(model, batches[0], True)
    rec[pre + "loss"] = np.array(loss, np.float32)
    for n in g:
        if n.startswith("task_layer."):
            put(rec, pre + "g::" + n, g[n])
            put(rec, pre + "g16::" + n, g16[n])
        else:
            rec[pre + "g::" + n], rec[pre + "g16::" + n] = np_(g[n]), np_(g16[n])
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    train = set(g)

    def cap(step, m):
        if step + 1 in (1, 4):
            for k, v in m.state_dict().items():
                if k not in train:
                    continue
                if k.startswith("task_layer."):
                    put(rec, pre + f"after{step + 1}." + k, v)
                else:
                    rec[pre + f"after{step + 1}.d::" + k] = np_(v.detach() - init[k])
    losses = MV.local_update(model, "bias", "art", [batches[0], batches[1], batches[0], batches[1]], cap)
    rec[pre + "losses"] = np.array(losses, np.float32)
    print("GM1 bias losses", losses)
    np.savez_compressed(os.path.join(OUT, "gm1_mixed_frame.npz"), **rec)


if __name__ == "__main__":
    torch.manual_seed(0)
    golden_gm1()
