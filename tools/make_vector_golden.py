"""Generate the optimizer_mode 'bias' / 'norm' fixtures (tests/golden/gv*.npz) by running the reference's own modules: its
ViltContinualLearner without an adapter, made trainable by the statements of its own prepare_model (main.py:126-250, taken
from the source by ast and executed on the model: requires_grad flags, comm_state_dict_names, personal_params_names), its
non-dat train_step (task_trainer.py:433-450), create_optimizer and get_average_net.  The shims, trainer set-up and storage
helpers are imported read-only from oracle/make_golden.py and tools/make_adapter_golden.py; this script writes to
tests/golden/ only, numeric arrays and name lists.

    python tools/make_vector_golden.py [gv1 gv3 gv2:bias gv2:norm]     (default: gv1 gv3; the gv2 rounds are the long ones)
"""
import ast
import copy
import os
import re
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import make_golden as MG  # noqa: E402  (installs the shims on import)
from oracle import feddat_oracle as O  # noqa: E402
from oracle.make_golden import _Wrap, make_trainer, np_, put  # noqa: E402
from make_adapter_golden import pack_codes  # noqa: E402
from feddat_amd import vilt_spec  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MODES = ("bias", "norm")


def reference_prepare(model, mode):
    """The part of the reference's prepare_model that follows the model's construction (main.py:125-250), executed on
    `model` with args.optimizer_mode = mode.  Returns args (personal_params_names)."""
    src = open(os.path.join(MG.REF, "src/train/main.py")).read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "prepare_model"][0]
    start = [i for i, s in enumerate(fn.body) if "comm_state_dict_names = []" in ast.unparse(s)][0]
    stop = [i for i, s in enumerate(fn.body) if i > start and ast.unparse(s).startswith("print(")][0]
    args = types.SimpleNamespace(optimizer_mode=mode, encoder_name="vilt", layers_to_freeze=0)
    ns = {"model": model, "args": args, "torch": torch}
    exec(compile(ast.Module(body=fn.body[start:stop], type_ignores=[]), "main.py:prepare_model", "exec"), ns)
    return args


def plain_shapes(d: O.ViltDims, tasks):
    """O.param_shapes without the adapters (these modes add no parameters); without Adaptered_ViltOutput the FFN's second
    product keeps its HF key, output.dense (not output.layer.dense)."""
    shapes = {k.replace(".output.layer.dense.", ".output.dense."): s for k, s in O.param_shapes(d, tasks).items()
              if ".adapter." not in k}
    assert all(dat_key(k) in O.param_shapes(d, tasks) for k in shapes)
    return shapes


def dat_key(k):
    """The key the dat fixtures seed this tensor by (so the frozen backbone equals theirs): FFN2 lives under `.layer` there."""
    return re.sub(r"(encoder\.layer\.\d+\.output\.)dense\.", r"\1layer.dense.", k)


def build_model(d: O.ViltDims, tasks, mode, bias_std=0.02, values=None):
    from transformers import ViltConfig, ViltModel
    from src.modeling.vilt import ViltEncoderWrapper, ViltContinualLearner
    cfg = ViltConfig(num_hidden_layers=d.layers, image_size=d.image_size)
    enc = ViltEncoderWrapper.__new__(ViltEncoderWrapper)
    nn.Module.__init__(enc)
    enc.processor = None
    enc.vilt = ViltModel(cfg)
    enc.device = torch.device("cpu")
    enc.max_text_length = cfg.max_position_embeddings
    enc.encoder_dim = cfg.hidden_size
    enc.expand_modality_type_embeddings()
    enc.process_inputs = lambda images, texts: images
    task_cfg = {t: {"num_labels": d.num_labels, "num_images": 1, "model_type": "classification"} for t in tasks}
    model = ViltContinualLearner(list(tasks), enc, cfg.hidden_size, task_cfg, torch.device("cpu"), None)
    model.args_ref = reference_prepare(model, mode)
    sd = model.state_dict()
    shapes = plain_shapes(d, tasks)
    assert sorted(shapes) == sorted(k for k in sd if "position_ids" not in k and "token_type_ids" not in k)
    with torch.no_grad():
        for k, shp in shapes.items():
            sd[k].copy_(values[k] if values is not None else O.seeded_value(dat_key(k), shp, 0.02, bias_std))
    model.eval()
    return model


def name_lists(model):
    """What the reference's own objects say: trainable (requires_grad), communicated (comm_state_dict_names), personal
    (the personal_params_names substrings over state_dict keys, main.py:444-450), decayed (create_optimizer's first group)."""
    tr = make_trainer("art", 1e-4, 1)
    opt = tr.create_optimizer(model, "full")
    decayed_ids = {id(p) for p in opt.param_groups[0]["params"]}
    return dict(
        trainable=[n for n, p in model.named_parameters() if p.requires_grad],
        communicated=list(model.comm_state_dict_names),
        personal=[n for n in model.state_dict() if any(pn in n for pn in model.args_ref.personal_params_names)],
        decayed=[n for n, p in model.named_parameters() if id(p) in decayed_ids])


def local_update(model, mode, task, batches, capture=None, num_epochs=15):
    from transformers import get_polynomial_decay_schedule_with_warmup
    tr = make_trainer(task, 1e-4, len(batches), num_epochs)
    tr.args.optimizer_mode = mode
    opt = tr.create_optimizer(model, mode)
    sch = get_polynomial_decay_schedule_with_warmup(opt, num_warmup_steps=int(tr.max_steps * tr.warmup_ratio),
                                                    num_training_steps=tr.max_steps, lr_end=0, power=1)
    model.zero_grad()
    w = _Wrap(model)
    losses = []
    for step, b in enumerate(batches):
        losses.append(float(tr.train_step(w, step, dict(b), opt, sch)))
        if capture is not None:
            capture(step, model)
    return losses


def gradients(model, batch, autocast):
    """Gradient of the reference's loss (BCE_mean * C, task_trainer.py:440) w.r.t. every trainable tensor."""
    model.zero_grad()
    crit = nn.BCEWithLogitsLoss(reduction="mean")
    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            _, logits = model(task_key="art", images=MG._enc_only(batch), texts=None)
    else:
        _, logits = model(task_key="art", images=MG._enc_only(batch), texts=None)
    tgt = batch["target_scores"]
    loss = crit(logits.float(), tgt) * tgt.shape[1]
    loss.backward()
    g = {n: p.grad.detach().clone().float() for n, p in model.named_parameters() if p.requires_grad}
    model.zero_grad()
    return float(loss), g


GV1_VALID = [(224, 224), (160, 224), (224, 128), (96, 192)]
GV1_TEXT = [40, 31, 40, 12]


def gv1_batches(case, n, seed0=2000):
    bs = [O.synthetic_batch(4, 224, seed0 + s) for s in range(n)]
    return [O.pad_batch(b, GV1_VALID, GV1_TEXT) for b in bs] if case == "padded" else bs


def golden_gv1():
    """2 layers, B = 4, 224: per mode and case ("plain"; "padded" = padded images + ragged text): pooled, logits, loss, the fp32
    gradient of every trainable tensor (g::) and the same under bf16 autocast (g16::), then 4 steps: every trainable tensor
    after steps 1 and 4 (backbone vectors whole as the update dW, heads in put()'s whole / sampled form).  One file per mode."""
    d = O.ViltDims(layers=2)
    for mode in MODES:
        rec = {}
        for case in ("plain", "padded"):
            pre = f"{mode}.{case}."
            model = build_model(d, ["art"], mode)
            batches = gv1_batches(case, 4)
            with torch.no_grad():
                pooled, logits = model(task_key="art", images=MG._enc_only(batches[0]), texts=None)
            rec[pre + "fwd.pooled"], rec[pre + "fwd.logits"] = np_(pooled), np_(logits)
            loss, g = gradients(model, batches[0], False)
            _, g16 = gradients(model, batches[0], True)
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
            losses = local_update(model, mode, "art", batches, cap)
            rec[pre + "losses"] = np.array(losses, np.float32)
            kq = [(float(g[n].abs().max()), float(g[n.replace("key", "query")].abs().max())) for n in g if "key.bias" in n]
            print("GV1", mode, case, "losses", losses, "max|g key.bias| / max|g query.bias| per layer", kq)
        np.savez_compressed(os.path.join(OUT, f"gv1_vilt2_{mode}.npz"), **rec)


def golden_gv2(mode, steps=80, batch=32, snaps=(20, 40, 60, 80), seed0=8000):
    """12 layers, B = 32, 384 x 384, one 80-step local round (ga2's protocol and batches): per snapshot every element of the
    update of every trainable tensor as pack_codes() codes; the logits of the trained model on a held-out batch (seed0 - 1);
    the largest |d key.bias| and |d query.bias| of the fp32 reference after the round."""
    d = O.ViltDims(layers=12)
    model = build_model(d, ["art"], mode)
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    train = {n for n, p in model.named_parameters() if p.requires_grad}
    rec = {"steps": np.array(steps), "batch": np.array(batch), "snaps": np.array(snaps), "seed0": np.array(seed0)}

    def cap(step, m):
        n = step + 1
        print("GV2", mode, "step", n, flush=True)
        if n in snaps:
            pack_codes(rec, f"s{n}::dq::", {k: (v.detach() - init[k]) for k, v in m.state_dict().items() if k in train})
    batches = [O.synthetic_batch(batch, 384, seed0 + s) for s in range(steps)]
    losses = local_update(model, mode, "art", batches, cap)
    rec["losses"] = np.array(losses, np.float32)
    held = O.synthetic_batch(batch, 384, seed0 - 1)
    with torch.no_grad():
        pooled, logits = model(task_key="art", images=MG._enc_only(held), texts=None)
    rec["heldout.seed"], rec["heldout.pooled"], rec["heldout.logits"] = np.array(seed0 - 1), np_(pooled), np_(logits)
    sd = model.state_dict()
    for which in ("key", "query"):
        moves = [float((sd[k] - init[k]).abs().max()) for k in sd if f"attention.attention.{which}.bias" in k]
        rec[f"max_abs_d_{which}_bias"] = np.array(max(moves) if mode == "bias" else 0.0)
        print("GV2", mode, f"max |d {which}.bias| after {steps} steps:", max(moves))
    np.savez_compressed(os.path.join(OUT, f"gv2_round{steps}_b{batch}_{mode}.npz"), **rec)
    print("GV2", mode, "losses", losses[:3], "...", losses[-3:])


GV3 = dict(tasks=["art", "abstract"], steps=[3, 2], rounds=2, batch=4, res=224, seed=42, layers=2)


def golden_gv3():
    """Two clients x 3 / 2 steps, two rounds of the reference's FL loop per mode (main.py:440-510): deepcopy(server) + personal
    tensors, local update, personal tensors back, get_average_net over comm_state_dict_names.  Weights and batches are what
    `python -m feddat_amd.train --optimizer_mode <mode> --num_layers 2 --image_size 224 --batch_size 4 --ordered_cl_tasks
    art,abstract --synthetic_steps 3,2 --comm_rounds 2` builds (vilt_spec.random_init / synthetic_batch, seed 42).  Stored: the
    reference's name lists (trainable / communicated / personal / decayed) for the 2-layer and a 12-layer model, and after each
    round every communicated server tensor (the update dW) and every personal tensor of each client."""
    c = GV3
    rec = {}
    get_average_net = MG.load_get_average_net()
    for mode in MODES:
        for k, v in name_lists(build_model(O.ViltDims(layers=12), c["tasks"], mode)).items():
            rec[f"{mode}.names12.{k}"] = np.array(v)
        d = O.ViltDims(layers=c["layers"])
        params = vilt_spec.random_init(c["layers"], c["tasks"], seed=c["seed"], optimizer_mode=mode)
        server = build_model(d, c["tasks"], mode, values=params)
        names = name_lists(server)
        for k, v in names.items():
            rec[f"{mode}.names.{k}"] = np.array(v)
        personal = {t: {n: v.clone() for n, v in server.state_dict().items() if n in names["personal"]} for t in c["tasks"]}
        data = {t: [vilt_spec.synthetic_batch(c["batch"], c["res"], c["seed"] + 1000 * ti + s) for s in range(c["steps"][ti])]
                for ti, t in enumerate(c["tasks"])}
        for rnd in range(c["rounds"]):
            c_models = []
            for t in c["tasks"]:
                m = copy.deepcopy(server)
                with torch.no_grad():
                    for n, v in personal[t].items():
                        m.state_dict()[n].copy_(v)
                local_update(m, mode, t, data[t])
                personal[t] = {n: v.detach().clone() for n, v in m.state_dict().items() if n in names["personal"]}
                c_models.append({n: v.detach().clone() for n, v in m.state_dict().items() if n in server.comm_state_dict_names})
            server = get_average_net(server, c_models, [1.0] * len(c_models), c["tasks"], torch.device("cpu"))
            for n in names["communicated"]:
                rec[f"{mode}.r{rnd}.server.d::" + n] = np_(server.state_dict()[n] - params[n])
            for t in c["tasks"]:
                for n, v in personal[t].items():
                    if n.startswith(f"task_layer.{t}."):
                        put(rec, f"{mode}.r{rnd}.{t}." + n, v)
        print("GV3", mode, "written;", len(names["communicated"]), "communicated keys")
    np.savez_compressed(os.path.join(OUT, "gv3_round_2clients_vector.npz"), **rec)


if __name__ == "__main__":
    which = sys.argv[1:] or ["gv1", "gv3"]
    torch.manual_seed(0)
    for w in which:
        if ":" in w:
            name, arg = w.split(":")
            globals()["golden_" + name](arg)
        else:
            globals()["golden_" + w]()
