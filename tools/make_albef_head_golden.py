"""Generate the ALBEF trainable-LM-head fixtures (tests/golden/gh*.npz) by running the reference's own modules with the head
made trainable the way the reference makes it: the statements of its own prepare_model (main.py:125-250, taken from the source
by ast and executed on the model with encoder_name = "albef_no_distill", optimizer_mode = "dat": requires_grad flags --
including main.py:247-250's `'.cls.' in n` -- comm_state_dict_names, personal_params_names), its TaskTrainer.train_step /
create_optimizer / kl_loss.  The shims, the model builder and the local-update driver are imported read-only from
oracle/make_albef_golden.py (the G10 / G11 fixtures were captured by the same driver with the head frozen); this script writes
to tests/golden/ only, numeric arrays and name lists.

    python tools/make_albef_head_golden.py [gh1 gh2]

Every run exists twice: in fp32, and with every forward under torch.autocast("cpu", bfloat16) (outputs converted back to fp32,
what accelerate's mixed precision does) -- the reference's own coarser arithmetic, the yardstick the head tensors are held to.
"""
import ast
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_albef_golden as MA  # noqa: E402  (installs the shims on import)
from oracle import albef_oracle as A  # noqa: E402
from oracle.make_albef_golden import np_  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CLS = "albef_model.albef.text_decoder.cls.predictions."
HEAD = [CLS + n for n in ("bias", "transform.dense.weight", "transform.dense.bias", "transform.LayerNorm.weight",
                          "transform.LayerNorm.bias")]
SAMPLE_ABOVE, N_SAMPLES = 4096, 4096


def put(rec, key, t):
    """Small tensors whole; large ones (transform.dense.weight) as L2 norm + N_SAMPLES strided samples."""
    t = t.detach().float()
    if t.numel() <= SAMPLE_ABOVE:
        rec[key] = np_(t)
    else:
        flat = t.flatten()
        idx = torch.linspace(0, flat.numel() - 1, N_SAMPLES).long()
        rec["samp::" + key] = np_(flat[idx])
        rec["norm::" + key] = np_(flat.norm())


def reference_prepare(model):
    """The part of the reference's prepare_model that follows the model's construction (main.py:125-250), executed on `model`.
    Returns args (personal_params_names)."""
    src = open(os.path.join(MA.REF, "src/train/main.py")).read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "prepare_model"][0]
    start = [i for i, s in enumerate(fn.body) if "comm_state_dict_names = []" in ast.unparse(s)][0]
    stop = [i for i, s in enumerate(fn.body) if i > start and ast.unparse(s).startswith("print(")][0]
    args = types.SimpleNamespace(optimizer_mode="dat", encoder_name="albef_no_distill", layers_to_freeze=0)
    ns = {"model": model, "args": args, "torch": torch}
    exec(compile(ast.Module(body=fn.body[start:stop], type_ignores=[]), "main.py:prepare_model", "exec"), ns)
    return args


def build_model(d):
    model = MA.build_reference_model(d)
    model.args_ref = reference_prepare(model)
    return model


def name_lists(model):
    """What the reference's own objects say once TaskTrainer.train has frozen the teacher (task_trainer.py:36-45), i.e. what
    create_optimizer sees: trainable (requires_grad over named_parameters, which lists a tied tensor once, under its first
    name), communicated (comm_state_dict_names), personal (the personal_params_names substrings over state_dict keys,
    main.py:444-450 -- the tied aliases decoder.weight / decoder.bias are state_dict keys of their own), decayed
    (create_optimizer's first group)."""
    for n, p in model.named_parameters():
        if "adapter_2" in n:
            p.requires_grad = False
    tr = MA.TaskTrainer()
    tr.lr, tr.adam_epsilon, tr.weight_decay = 1e-4, 1e-8, 1e-2
    opt = tr.create_optimizer(model, "dat")
    decayed_ids = {id(p) for p in opt.param_groups[0]["params"]}
    return dict(
        trainable=[n for n, p in model.named_parameters() if p.requires_grad],
        communicated=list(model.comm_state_dict_names),
        personal=[n for n in model.state_dict() if any(pn in n for pn in model.args_ref.personal_params_names)],
        decayed=[n for n, p in model.named_parameters() if id(p) in decayed_ids])


class _AutocastWrap(MA._Wrap):
    """_Wrap whose forward runs under bf16 autocast, outputs back in fp32 (accelerate's convert_outputs_to_fp32)."""

    def __call__(self, *a, **k):
        with torch.autocast("cpu", dtype=torch.bfloat16):
            out = self.module(*a, **k)
        return [o.float() if torch.is_tensor(o) else o for o in out]


def local_update(model, batches, autocast, num_epochs, capture):
    """oracle/make_albef_golden.ref_local_update, its model wrapper swapped for the autocast one when asked."""
    keep = MA._Wrap
    MA._Wrap = _AutocastWrap if autocast else keep
    try:
        return MA.ref_local_update(model, batches, lr=1e-4, num_epochs=num_epochs, capture=capture)
    finally:
        MA._Wrap = keep


def head_gradients(model, batch, autocast):
    """Gradient of L_1 = (loss_1 + KL(logits_1 || logits_all)) / 2 (task_trainer.py:283-302: teacher = the gated logits, no
    grad) w.r.t. the five head tensors at the model's current weights."""
    w = (_AutocastWrap if autocast else MA._Wrap)(model)
    model.zero_grad()
    with torch.no_grad():
        MA.set_mode(model, "gating")
        _, logits_all = w("art", dict(batch, train=True))
    MA.set_mode(model, "adapter_1")
    loss_1, logits_1 = w("art", dict(batch, train=True))
    L_1 = (loss_1 + MA.kl_loss(logits_1, logits_all.clone().detach())) / 2
    L_1.backward()
    par = dict(model.named_parameters())
    g = {n: par[n].grad.detach().clone().float() for n in HEAD}
    model.zero_grad()
    return float(L_1), g


def run_records(rec, pre, d, batches, autocast, num_epochs, snaps, with_max, n_samp=512):
    """One local update from the initial weights: losses, the update of every head tensor after each step in `snaps`, and
    the dnorm / dmean / (dmax) / dsamp records of adapter_0 / adapter_1 that G10 / G11 store.  Returns the trained model."""
    model = build_model(d)
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}

    def cap(step, m):
        if step + 1 in snaps:
            sd = m.state_dict()
            for k in HEAD:
                put(rec, f"{pre}after{step + 1}.d::{k}", sd[k].detach() - init[k])
    rec[pre + "losses"] = np.array(local_update(model, batches, autocast, num_epochs, cap), np.float32)
    for k, v in model.state_dict().items():
        if "adapter_0" in k or "adapter_1" in k:
            dw = (v.detach() - init[k]).flatten()
            idx = torch.linspace(0, dw.numel() - 1, min(n_samp, dw.numel())).long()
            rec[pre + "dnorm::" + k], rec[pre + "dmean::" + k] = np_(dw.norm()), np_(dw.abs().mean())
            rec[pre + "dsamp::" + k] = np_(dw[idx])
            if with_max:
                rec[pre + "dmax::" + k] = np_(dw.abs().max())
    return model


def golden_gh1():
    """small_dims(), the G10 batch protocol (B = 3, k = [2, 1, 3], ragged, 4 steps, lr 1e-4, 15 epochs of 4), dropout 0."""
    d = MA.small_dims()
    rec = {}
    model = build_model(d)
    for k, v in name_lists(model).items():
        rec["names." + k] = np.array(v)
    assert [n for n in rec["names.trainable"] if ".cls." in n] == HEAD
    batches = [A.synthetic_batch(3, d, 510 + s, q_len=12, a_len=5, k=[2, 1, 3], ragged=True) for s in range(4)]
    L1, g = head_gradients(model, batches[0], False)
    _, g16 = head_gradients(model, batches[0], True)
    rec["L_1"] = np.array(L1, np.float32)
    for n in HEAD:
        put(rec, "g::" + n, g[n])
        put(rec, "g16::" + n, g16[n])
    trained = run_records(rec, "fp32.", d, batches, False, 15, (1, 4), False)
    run_records(rec, "ac.", d, batches, True, 15, (1, 4), False)
    # eval path on the TRAINED fp32 model: rank_answer over an 11-answer list, k = 4 (G10's eval.* protocol)
    b0 = A.synthetic_batch(3, d, 500, q_len=12, a_len=5, k=[2, 1, 3], ragged=True)
    ev = A.synthetic_batch(3, d, 501, q_len=12, a_len=5, k=[4, 4, 3], ragged=True)
    ns = types.SimpleNamespace
    with torch.no_grad():
        MA.set_mode(trained, "gating")
        ids, probs = trained.albef_model.albef(
            image=b0["image"], question=ns(input_ids=b0["question_ids"], attention_mask=b0["question_mask"]),
            answer=ns(input_ids=ev["answer_ids"], attention_mask=ev["answer_mask"]), train=False, k=4)
    rec["eval.topk_ids"], rec["eval.topk_probs"] = ids.numpy().astype(np.int64), np_(probs)
    np.savez_compressed(os.path.join(OUT, "gh1_albef_head_small.npz"), **rec)
    print("GH1 losses fp32", rec["fp32.losses"], "autocast", rec["ac.losses"])


def golden_gh2(steps=40):
    """G11's protocol (small configuration, `steps` train_steps, one epoch: the schedule runs past its warm-up) with the head
    trainable: gh1's records plus dmax."""
    d = MA.small_dims()
    rec = {"steps": np.array(steps, np.int64)}
    batches = [A.synthetic_batch(3, d, 700 + s, q_len=12, a_len=5, k=[2, 1, 3], ragged=True) for s in range(steps)]
    run_records(rec, "fp32.", d, batches, False, 1, (1, steps), True)
    run_records(rec, "ac.", d, batches, True, 1, (1, steps), True)
    np.savez_compressed(os.path.join(OUT, f"gh2_albef_head_round{steps}.npz"), **rec)
    print("GH2 losses fp32", rec["fp32.losses"][:3], rec["fp32.losses"][-3:], "autocast", rec["ac.losses"][-3:])


if __name__ == "__main__":
    torch.manual_seed(0)
    for w in sys.argv[1:] or ["gh1", "gh2"]:
        globals()["golden_" + w]()
