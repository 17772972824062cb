"""Generate the ALBEF single-adapter (FedAvg baseline, optimizer_mode 'adapter') fixtures tests/golden/gb*.npz by running the
reference's own modules built with adapter_config names = ["adapter"] (main.py:114-118): the statements of its own prepare_model
(main.py:125-250, taken from the source by ast and executed with encoder_name = "albef_no_distill", optimizer_mode = "adapter":
requires_grad flags, comm_state_dict_names, personal_params_names) and the non-dat branch of its TaskTrainer.train_step
(task_trainer.py:433-450) with its create_optimizer.  The shims, _Wrapper, _Wrap, _Acc, TaskTrainer, np_ and small_dims are
imported read-only from oracle/make_albef_golden.py; the module with a single adapter per site is built here.  This script
writes to tests/golden/ only, numeric arrays and name lists.

    python tools/make_albef_adapter_golden.py [gb1 gb2 gb3 gb4]

Every run exists twice: in fp32, and with every forward under torch.autocast("cpu", bfloat16) (outputs converted back to fp32,
what accelerate's mixed precision does) -- the reference's own coarser arithmetic, the yardstick the engine's gradients are held
to.  Prefix `head.`: the reference's flags (the five `.cls.` tensors train).  Prefix `nohead.`: the same run with requires_grad
of the `.cls.` tensors cleared -- that is the reference's MODULES under a flag setting its configuration never produces; it is
the counterpart of the engines' default train_lm_head=False.
"""
import ast
import os
import sys
import types
from functools import partial

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_albef_golden as MA  # noqa: E402  (installs the shims on import)
from oracle import albef_oracle as A  # noqa: E402
from oracle.make_albef_golden import np_  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SAMPLE_ABOVE, N_SAMPLES = 4096, 512


def put(rec, key, t):
    """Small tensors whole; large ones as L2 norm + mean |.| + max |.| + N_SAMPLES strided samples."""
    t = t.detach().float()
    if t.numel() <= SAMPLE_ABOVE:
        rec[key] = np_(t)
    else:
        flat = t.flatten()
        idx = torch.linspace(0, flat.numel() - 1, N_SAMPLES).long()
        rec["samp::" + key], rec["norm::" + key] = np_(flat[idx]), np_(flat.norm())
        rec["mean::" + key], rec["max::" + key] = np_(flat.abs().mean()), np_(flat.abs().max())


def build_module(d, dropout=0.0):
    """ALBEF with ONE adapter per site: oracle/make_albef_golden.build_albef_module with names = ["adapter"]."""
    xb, ac = MA.xb, {"names": ["adapter"], "device": "cpu"}
    cfgd = dict(hidden_size=d.hidden, intermediate_size=d.inter, num_attention_heads=d.heads, num_hidden_layers=d.enc_layers,
                vocab_size=d.vocab, max_position_embeddings=d.max_pos, type_vocab_size=2, layer_norm_eps=1e-12,
                hidden_act="gelu", hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout, pad_token_id=d.pad_id,
                fusion_layer=d.fusion_layer, encoder_width=d.hidden)
    ce = xb.BertConfig(**cfgd)
    ce.adapter_config = ac
    cd = xb.BertConfig(**cfgd)
    cd.fusion_layer, cd.num_hidden_layers, cd.adapter_config = 0, d.dec_layers, ac
    m = MA.ALBEF.__new__(MA.ALBEF)
    nn.Module.__init__(m)
    m.tokenizer = types.SimpleNamespace(pad_token_id=d.pad_id)
    m.distill = False
    m.visual_encoder = MA.VisionTransformer(img_size=d.image, patch_size=d.patch, embed_dim=d.hidden, depth=d.vit_depth,
                                            num_heads=d.heads, mlp_ratio=4, qkv_bias=True,
                                            norm_layer=partial(nn.LayerNorm, eps=1e-6), adapter_config=ac)
    m.text_encoder = xb.BertModel(config=ce, add_pooling_layer=False)
    m.text_decoder = xb.BertLMHeadModel(config=cd)
    m.text_decoder.cls.predictions.decoder.weight = m.text_decoder.bert.embeddings.word_embeddings.weight
    return m


def reference_prepare(model):
    """The part of the reference's prepare_model that follows the model's construction (main.py:125-250), executed on `model`
    for optimizer_mode = "adapter".  Returns args (personal_params_names)."""
    src = open(os.path.join(MA.REF, "src/train/main.py")).read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "prepare_model"][0]
    start = [i for i, s in enumerate(fn.body) if "comm_state_dict_names = []" in ast.unparse(s)][0]
    stop = [i for i, s in enumerate(fn.body) if i > start and ast.unparse(s).startswith("print(")][0]
    args = types.SimpleNamespace(optimizer_mode="adapter", encoder_name="albef_no_distill", layers_to_freeze=0)
    ns = {"model": model, "args": args, "torch": torch}
    exec(compile(ast.Module(body=fn.body[start:stop], type_ignores=[]), "main.py:prepare_model", "exec"), ns)
    return args


def build_model(d, head=True, dropout=0.0):
    """The continual learner around build_module, every tensor filled by name (seeded), the reference's flags set by its own
    prepare_model; head=False then clears requires_grad of the `.cls.` tensors."""
    CL = MA._load_continual_learner_class()
    cl = CL.__new__(CL)
    nn.Module.__init__(cl)
    cl.albef_model = MA._Wrapper(build_module(d, dropout))
    sd = cl.state_dict()
    with torch.no_grad():
        for k, v in sd.items():
            if "position_ids" in k or "decoder.weight" in k or "decoder.bias" in k:      # buffers / tied aliases
                continue
            v.copy_(A.O.seeded_value(k, tuple(v.shape), 0.02, 0.02))
    cl.args_ref = reference_prepare(cl)
    if not head:
        for n, p in cl.named_parameters():
            if ".cls." in n:
                p.requires_grad = False
    cl.eval()
    return cl


def trainer(lr=1e-4):
    tr = MA.TaskTrainer()
    tr.accelerator, tr.device, tr.task_key = MA._Acc(), torch.device("cpu"), "art"
    tr.args = types.SimpleNamespace(optimizer_mode="adapter", encoder_name="albef_no_distill", debug=0)
    tr.batch2inputs_converter = lambda batch: dict(batch)
    tr.lr, tr.adam_epsilon, tr.weight_decay, tr.warmup_ratio = lr, 1e-8, 1e-2, 0.1
    return tr


def name_lists(model):
    """What the reference's own objects say: trainable (requires_grad over named_parameters), communicated
    (comm_state_dict_names), personal (the personal_params_names substrings over state_dict keys, main.py:444-450 -- the tied
    aliases decoder.weight / decoder.bias are state_dict keys of their own), decayed (create_optimizer's first group)."""
    opt = trainer().create_optimizer(model, "adapter")
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


def local_update(model, batches, autocast, num_epochs, capture=None, lr=1e-4):
    """TaskTrainer.train's prologue for a non-dat mode (task_trainer.py:30-59: no teacher copy, fresh AdamW, linear warm-up /
    decay over len(batches) * num_epochs ticks) and its own train_step per batch."""
    from transformers import get_polynomial_decay_schedule_with_warmup
    tr = trainer(lr)
    tr.max_steps = len(batches) * num_epochs
    opt = tr.create_optimizer(model, "adapter")
    sch = get_polynomial_decay_schedule_with_warmup(opt, num_warmup_steps=int(tr.max_steps * tr.warmup_ratio),
                                                    num_training_steps=tr.max_steps, lr_end=0, power=1)
    model.zero_grad()
    w = (_AutocastWrap if autocast else MA._Wrap)(model)
    losses = []
    for s, b in enumerate(batches):
        losses.append(float(tr.train_step(w, s, dict(b), opt, sch)))
        if capture is not None:
            capture(s, model)
    return losses


def first_step(model, batch, autocast):
    """(loss, logits, {name: gradient of every trainable tensor}) of ALBEF.forward(train=True) at the model's current weights."""
    w = (_AutocastWrap if autocast else MA._Wrap)(model)
    model.zero_grad()
    model.set_active_adapter("adapter")
    loss, logits = w("art", dict(batch, train=True))
    loss.backward()
    g = {n: p.grad.detach().clone().float() for n, p in model.named_parameters() if p.requires_grad}
    model.zero_grad()
    return loss.detach(), logits.detach(), g


def run_records(rec, pre, d, batches, head, autocast, num_epochs, snaps, n_samp=512):
    """One local update from the initial weights: losses, the update of every head tensor after each step in `snaps` (head
    trained), and dnorm / dmean / dmax / dsamp of every adapter tensor after the steps in `snaps`.  Returns the trained model."""
    model = build_model(d, head)
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    last = max(snaps)

    def cap(step, m):
        if step + 1 not in snaps:
            return
        tag = "" if step + 1 == last else f"after{step + 1}."
        for k, v in m.state_dict().items():
            if ".cls." in k and head and "predictions.decoder." not in k:      # (not the tied aliases)
                put(rec, f"{pre}after{step + 1}.d::{k}", v.detach() - init[k])
            if "adapter" in k and k in init:      # (set_active_adapter adds `active_adapter_*` aliases of the same modules)
                dw = (v.detach() - init[k]).flatten()
                idx = torch.linspace(0, dw.numel() - 1, min(n_samp, dw.numel())).long()
                rec[pre + tag + "dnorm::" + k], rec[pre + tag + "dmean::" + k] = np_(dw.norm()), np_(dw.abs().mean())
                rec[pre + tag + "dsamp::" + k], rec[pre + tag + "dmax::" + k] = np_(dw[idx]), np_(dw.abs().max())
    rec[pre + "losses"] = np.array(local_update(model, batches, autocast, num_epochs, cap), np.float32)
    return model


def golden_gb1():
    """small_dims(), the G10 batch protocol (B = 3, k = [2, 1, 3], ragged, 4 steps, lr 1e-4, 15 epochs of 4), dropout 0."""
    d = MA.small_dims()
    rec = {}
    batches = [A.synthetic_batch(3, d, 510 + s, q_len=12, a_len=5, k=[2, 1, 3], ragged=True) for s in range(4)]
    for pre, head in (("head.", True), ("nohead.", False)):
        model = build_model(d, head)
        for k, v in name_lists(model).items():
            rec[pre + "names." + k] = np.array(v)
        keys, dims = list(model.state_dict()), [",".join(str(x) for x in v.shape) for v in model.state_dict().values()]
        loss, logits, g = first_step(model, batches[0], False)
        loss16, _, g16 = first_step(model, batches[0], True)
        rec[pre + "fwd.loss"], rec[pre + "fwd.loss16"] = np_(loss), np_(loss16)
        if head:
            rec["fwd.logits"] = np_(logits)
            rec["shapes.keys"], rec["shapes.dims"] = np.array(keys), np.array(dims)
        assert sorted(g) == sorted(rec[pre + "names.trainable"].tolist())
        for n in g:
            err = float((g16[n] - g[n]).abs().max())
            assert err > 0, n           # the yardstick of the engine's gradient error: never empty
            put(rec, pre + "g::" + n, g[n])
            put(rec, pre + "g16::" + n, g16[n])
        trained = run_records(rec, pre + "fp32.", d, batches, head, False, 15, (2, 4), n_samp=64)      # (file size: < 1 MiB)
        run_records(rec, pre + "ac.", d, batches, head, True, 15, (2, 4), n_samp=64)
        if head:
            # eval path on the TRAINED fp32 model: rank_answer over an 11-answer list, k = 4 (G10's eval.* protocol)
            b0 = A.synthetic_batch(3, d, 500, q_len=12, a_len=5, k=[2, 1, 3], ragged=True)
            ev = A.synthetic_batch(3, d, 501, q_len=12, a_len=5, k=[4, 4, 3], ragged=True)
            ns = types.SimpleNamespace
            with torch.no_grad():
                trained.set_active_adapter("adapter")
                ids, probs = trained.albef_model.albef(
                    image=b0["image"], question=ns(input_ids=b0["question_ids"], attention_mask=b0["question_mask"]),
                    answer=ns(input_ids=ev["answer_ids"], attention_mask=ev["answer_mask"]), train=False, k=4)
            rec["eval.topk_ids"], rec["eval.topk_probs"] = ids.numpy().astype(np.int64), np_(probs)
    np.savez_compressed(os.path.join(OUT, "gb1_albef_adapter_small.npz"), **rec)
    print("GB1 losses fp32", rec["head.fp32.losses"], "autocast", rec["head.ac.losses"], "no head", rec["nohead.fp32.losses"])


def golden_gb2(steps=40):
    """G11's protocol (small configuration, `steps` train_steps, one epoch: the schedule runs past its warm-up), head trainable."""
    d = MA.small_dims()
    rec = {"steps": np.array(steps, np.int64)}
    batches = [A.synthetic_batch(3, d, 700 + s, q_len=12, a_len=5, k=[2, 1, 3], ragged=True) for s in range(steps)]
    run_records(rec, "fp32.", d, batches, True, False, 1, (2, steps))
    run_records(rec, "ac.", d, batches, True, True, 1, (2, steps))
    np.savez_compressed(os.path.join(OUT, f"gb2_albef_adapter_round{steps}.npz"), **rec)
    print("GB2 losses fp32", rec["fp32.losses"][:3], rec["fp32.losses"][-3:], "autocast", rec["ac.losses"][-3:])


def install_pass0_dropout(model, seed):
    """nn.Dropout.forward replaced by the counter-based mask of oracle/albef_oracle.py (dropout_keys, dropout_keep,
    dropout_site), keyed on the module's own name, for the ONE forward a non-dat train_step makes: pass id 0, step = forwards
    done before this one.  (oracle/make_albef_golden.install_counter_dropout counts three forwards per step.)  As there, a
    dropout module that fires without being one of the six mapped kinds trips the assertion."""
    import re
    kinds = [("embeddings.dropout", "emb"), ("crossattention.self.dropout", "cross_probs"), ("attention.self.dropout", "self_probs"),
             ("crossattention.output.dropout", "cross_out"), ("attention.output.dropout", "self_out")]
    n_sites = 0
    for n, m in model.named_modules():
        if isinstance(m, nn.Dropout):
            kind = next((k for suf, k in kinds if n.endswith(suf)), None)
            if kind is None and re.search(r"layer\.\d+\.output\.dropout$", n):
                kind = "out"
            m._fd_name, m._fd_site = n, (A.dropout_site(n, kind) if kind else None)
            n_sites += kind is not None
    state = {"calls": 0, "fired": set()}
    model.albef_model.register_forward_pre_hook(lambda mod, inp: state.__setitem__("calls", state["calls"] + 1))

    def fwd(self, x):
        if not self.training or self.p == 0:
            return x
        assert self._fd_site is not None, "unmapped dropout module fired: " + self._fd_name
        k0, k1 = A.dropout_keys(seed, 0, self._fd_site)
        keep = A.dropout_keep(x.numel(), self.p, k0, k1, state["calls"] - 1).view(x.shape)
        scale = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(self.p, dtype=torch.float32))
        state["fired"].add(self._fd_name)
        return x * (keep.to(x.dtype) * scale)
    nn.Dropout.forward = fwd
    return state, n_sites


def golden_gb3(steps=3, p=0.1, seed=77):
    """G12's protocol for the single-adapter step: `steps` train_steps of the small configuration under model.train() with
    hidden / attention dropout p, the masks the counter-based ones (one forward per step, pass 0), head trained; one epoch."""
    d = MA.small_dims()
    model = build_model(d, True, dropout=p)
    keep = nn.Dropout.forward
    state, n_sites = install_pass0_dropout(model, seed)
    try:
        model.train()
        batches = [A.synthetic_batch(3, d, 900 + s, q_len=12, a_len=5, k=[2, 1, 3], ragged=True) for s in range(steps)]
        init = {k: v.detach().clone() for k, v in model.state_dict().items()}
        rec = {"losses": np.array(local_update(model, batches, False, 1), np.float32), "steps": np.array(steps, np.int64),
               "p": np.array(p, np.float32), "seed": np.array(seed, np.int64)}
    finally:
        nn.Dropout.forward = keep
    assert state["calls"] == steps and len(state["fired"]) == n_sites, (state["calls"], len(state["fired"]), n_sites)
    for k, v in model.state_dict().items():
        if k not in init:
            continue
        if "adapter" in k:
            dw = (v.detach() - init[k]).flatten()
            idx = torch.linspace(0, dw.numel() - 1, min(512, dw.numel())).long()
            rec["dnorm::" + k], rec["dmean::" + k], rec["dsamp::" + k] = np_(dw.norm()), np_(dw.abs().mean()), np_(dw[idx])
        elif ".cls." in k and "predictions.decoder." not in k:
            put(rec, "d::" + k, v.detach() - init[k])
    np.savez_compressed(os.path.join(OUT, "gb3_albef_adapter_dropout.npz"), **rec)
    print("GB3 losses", rec["losses"], "dropout sites fired", len(state["fired"]))


GB4 = dict(tasks=["art", "abstract"], steps=[3, 2], rounds=2, seed0=800)


def gb4_batches(d, ti, n):
    return [A.synthetic_batch(3, d, GB4["seed0"] + 100 * ti + s, q_len=12, a_len=5, k=[2, 1, 3], ragged=True) for s in range(n)]


def golden_gb4():
    """Two clients (3 and 2 steps) over two rounds of the reference's FL loop (main.py:440-510): deepcopy(server) + the client's
    personal tensors, local update (15 epochs' schedule), personal tensors back, its own get_average_net over
    comm_state_dict_names; head trained.  Stored: the server's adapter tensors after each round (dnorm / dmean / dsamp of the
    update), each client's head update after each round, the name lists."""
    import copy
    src = open(os.path.join(MA.REF, "src/train/main.py")).read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "get_average_net"][0]
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "main.py:get_average_net", "exec"), ns)
    get_average_net = ns["get_average_net"]
    d, c = MA.small_dims(), GB4
    server = build_model(d, True)
    names = name_lists(server)
    rec = {"names." + k: np.array(v) for k, v in names.items()}
    init = {k: v.detach().clone() for k, v in server.state_dict().items()}
    pers = [n for n in server.state_dict() if any(pn in n for pn in server.args_ref.personal_params_names)]
    personal = {t: {n: server.state_dict()[n].detach().clone() for n in pers} for t in c["tasks"]}
    data = {t: gb4_batches(d, ti, c["steps"][ti]) for ti, t in enumerate(c["tasks"])}
    for rnd in range(c["rounds"]):
        c_models = []
        for t in c["tasks"]:
            m = copy.deepcopy(server)
            with torch.no_grad():
                for n in pers:
                    m.state_dict()[n].copy_(personal[t][n])
            local_update(m, data[t], False, 15)
            personal[t] = {n: m.state_dict()[n].detach().clone() for n in pers}
            c_models.append({n: v.detach().clone() for n, v in m.state_dict().items() if n in server.comm_state_dict_names})
        server = get_average_net(server, c_models, [1 for _ in c["tasks"]], c["tasks"], torch.device("cpu"))
        for n in names["communicated"]:
            dw = (server.state_dict()[n].detach() - init[n]).flatten()
            idx = torch.linspace(0, dw.numel() - 1, min(256, dw.numel())).long()
            pre = f"r{rnd}.server."
            rec[pre + "dnorm::" + n], rec[pre + "dmean::" + n], rec[pre + "dsamp::" + n] = np_(dw.norm()), np_(dw.abs().mean()), np_(dw[idx])
        for t in c["tasks"]:
            for n in pers:
                if "predictions.decoder." not in n:
                    put(rec, f"r{rnd}.{t}.d::{n}", personal[t][n] - init[n])
    path = os.path.join(OUT, "gb4_albef_adapter_2clients.npz")
    np.savez_compressed(path, **rec)
    print("GB4 written;", len(names["communicated"]), "communicated keys;", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    torch.manual_seed(0)
    for w in sys.argv[1:] or ["gb1", "gb2", "gb3", "gb4"]:
        globals()["golden_" + w]()
