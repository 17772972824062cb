"""Generate the optimizer_mode 'adapter' fixtures (tests/golden/ga*.npz) by running the reference's own modules with
adapter_config {"names": ["adapter"]} and args.optimizer_mode = "adapter" (main.py:114-118,141-149,248-250; the non-dat
train_step, task_trainer.py:433-450).  The shims, trainer set-up and storage helpers are imported read-only from
oracle/make_golden.py; this script writes to tests/golden/ only.

    python tools/make_adapter_golden.py [ga1 ga2 ga3 ga4]     (default: all four; ga2 is the long one)
"""
import copy
import lzma
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as MG  # noqa: E402  (installs the shims on import)
from oracle import feddat_oracle as O  # noqa: E402
from oracle.make_golden import _Wrap, make_trainer, np_, put  # noqa: E402
from feddat_amd import vilt_spec  # noqa: E402
from feddat_amd.modes import mode_names  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
# every element of a whole round's update in one small file: dW rounded to multiples of Q_STEP (error <= Q_STEP / 2 = 6.1e-5),
# the int8 codes of all tensors back-to-back, LZMA-compressed (tests/test_adapter_mode_gpu.py: unpack_codes)
Q_STEP = 2.0 ** -13


def pack_codes(rec, prefix, updates):
    """updates: {key: dW}.  Stores <prefix>names / sizes / step and <prefix>lzma (uint8 bytes of the int8 codes)."""
    codes = [torch.round(dw.flatten().double() / Q_STEP) for dw in updates.values()]
    assert all(float(c.abs().max()) <= 127 for c in codes), "update out of the int8 code range"
    flat = torch.cat(codes).to(torch.int8).numpy()
    rec[prefix + "names"] = np.array(list(updates))
    rec[prefix + "sizes"] = np.array([c.numel() for c in codes], np.int64)
    rec[prefix + "step"] = np.array(Q_STEP)
    rec[prefix + "lzma"] = np.frombuffer(lzma.compress(flat.tobytes(), preset=9 | lzma.PRESET_EXTREME), np.uint8)


def adapter_shapes(d: O.ViltDims, tasks):
    """O.param_shapes with the three DAT adapters replaced by the single `adapter` (adapter.py:22-39)."""
    out = {}
    for k, shp in O.param_shapes(d, tasks).items():
        if ".adapter.adapter_0_" in k:
            out[k.replace(".adapter.adapter_0_", ".adapter.adapter_")] = shp
        elif ".adapter.adapter_" not in k:
            out[k] = shp
    return out


def build_adapter_model(d: O.ViltDims, tasks, bias_std=0.02, values=None):
    """The reference's ViltContinualLearner in optimizer_mode adapter: names = ['adapter'], everything frozen except the
    adapters and the task heads.  values: {key: tensor} to load instead of the name-seeded fill."""
    from transformers import ViltConfig, ViltModel
    from src.modeling.vilt import ViltEncoderWrapper, ViltContinualLearner
    from src.modeling.adaptered_output import Adaptered_ViltOutput
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
    model = ViltContinualLearner(list(tasks), enc, cfg.hidden_size, task_cfg, torch.device("cpu"),
                                 {"names": ["adapter"], "device": "cpu"})
    for p in model.parameters():
        p.requires_grad = False
    for i in range(d.layers):        # add_adapter() for d.layers (it hard-codes range(12))
        model.vilt_encoder.vilt.encoder.layer[i].output = Adaptered_ViltOutput(
            model.vilt_encoder.vilt.encoder.layer[i].output, model.adapter_config)
    for n, p in model.named_parameters():         # main.py:141-149, 248-250
        if "adapter" in n or "task" in n:
            p.requires_grad = True
    model.comm_state_dict_names = [n for n in model.state_dict() if "adapter" in n]
    sd = model.state_dict()
    shapes = adapter_shapes(d, tasks)
    assert sorted(shapes) == sorted(k for k in sd if "position_ids" not in k and "token_type_ids" not in k)
    with torch.no_grad():
        for k, shp in shapes.items():
            sd[k].copy_(values[k] if values is not None else O.seeded_value(k, shp, 0.02, bias_std))
    model.eval()
    model.set_active_adapter("adapter")
    return model


def adapter_trainer(task, steps, num_epochs=15):
    tr = make_trainer(task, 1e-4, steps, num_epochs)
    tr.args.optimizer_mode = "adapter"
    return tr


def local_update(model, task, batches, capture=None, num_epochs=15):
    """TaskTrainer.train for optimizer_mode adapter: no teacher copy, fresh AdamW + poly schedule, one step per batch."""
    from transformers import get_polynomial_decay_schedule_with_warmup
    tr = adapter_trainer(task, len(batches), num_epochs)
    opt = tr.create_optimizer(model, "adapter")
    sch = get_polynomial_decay_schedule_with_warmup(opt, num_warmup_steps=int(tr.max_steps * tr.warmup_ratio),
                                                    num_training_steps=tr.max_steps, lr_end=0, power=1)
    model.zero_grad()
    w = _Wrap(model)
    losses, lrs = [], []
    for step, b in enumerate(batches):
        losses.append(float(tr.train_step(w, step, dict(b), opt, sch)))
        lrs.append(opt.param_groups[0]["lr"])
        if capture is not None:
            capture(step, model)
    return losses, lrs


def trainable(k):
    """(set_active_adapter('adapter') also registers the adapter's modules as `active_adapter_{down,up}`: aliases, skipped)"""
    return ("adapter" in k and "active_adapter" not in k) or k.startswith("task_layer.art.")


def golden_ga1():
    """2 layers, B = 4, 224 and 384 (keys prefixed "224." / "384."): forward (pooled, logits) with the adapter, then 5 steps:
    losses, LR after each step, every trainable tensor after steps 1, 2 and 5 (adapters: the whole update as float16 of
    dW * 256; heads: put()'s whole / sampled form of the weights)."""
    d = O.ViltDims(layers=2)
    rec = {}
    for res in (224, 384):
        model = build_adapter_model(d, ["art", "gqa"])
        with torch.no_grad():
            pooled, logits = model(task_key="art", images=MG._enc_only(O.synthetic_batch(4, res, 1234)), texts=None)
        rec[f"{res}.fwd.pooled"], rec[f"{res}.fwd.logits"] = np_(pooled), np_(logits)
        batches = [O.synthetic_batch(4, res, 2000 + s) for s in range(5)]
        init = {k: v.detach().clone() for k, v in model.state_dict().items()}

        def cap(step, m):
            if step + 1 in (1, 2, 5):
                for k, v in m.state_dict().items():
                    if not trainable(k):
                        continue
                    if "adapter" in k:      # every element of the update, as float16 of dW * 256 (g8b's encoding)
                        rec[f"{res}.after{step + 1}.dall::" + k] = ((v.detach() - init[k]) * 256.0).to(torch.float16).numpy()
                    else:
                        put(rec, f"{res}.after{step + 1}." + k, v)
        losses, lrs = local_update(model, "art", batches, cap)
        rec[f"{res}.losses"], rec[f"{res}.lr"] = np.array(losses, np.float32), np.array(lrs, np.float64)
        print("GA1", res, "losses", losses, "lr", lrs)
    np.savez_compressed(os.path.join(OUT, "ga1_vilt2_adapter.npz"), **rec)


def golden_ga2(steps=80, batch=32, snaps=(20, 40, 60, 80), seed0=8000):
    """12 layers, B = 32, 384 x 384, one 80-step local round (1200 ticks, warm-up 120): the update dW at every snapshot as
    norm / mean / max / 1024 samples, and every element of the adapter and head updates at the last one as pack_codes()
    codes (2.2 M elements in 0.8 MB) in the _all file."""
    d = O.ViltDims(layers=12)
    model = build_adapter_model(d, ["art"])
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    rec = {"steps": np.array(steps), "batch": np.array(batch), "snaps": np.array(snaps), "seed0": np.array(seed0)}
    full = {"steps": np.array(steps), "batch": np.array(batch), "seed0": np.array(seed0), "snaps": np.array((snaps[-1],))}
    last = {}

    def cap(step, m):
        n = step + 1
        print("GA2 step", n, flush=True)
        if n not in snaps:
            return
        for k, v in m.state_dict().items():
            if trainable(k):
                dw = (v.detach() - init[k]).flatten()
                idx = torch.linspace(0, dw.numel() - 1, min(1024, dw.numel())).long()
                rec[f"s{n}::dnorm::" + k] = np_(dw.norm())
                rec[f"s{n}::dmean::" + k] = np_(dw.abs().mean())
                rec[f"s{n}::dmax::" + k] = np_(dw.abs().max())
                rec[f"s{n}::dsamp::" + k] = np_(dw[idx])
                if n == snaps[-1]:
                    last[k] = dw.clone()
    batches = [O.synthetic_batch(batch, 384, seed0 + s) for s in range(steps)]
    losses, _ = local_update(model, "art", batches, cap)
    rec["losses"] = np.array(losses, np.float32)
    pack_codes(full, f"s{snaps[-1]}::dq::", last)
    np.savez_compressed(os.path.join(OUT, f"ga2_round{steps}_b{batch}.npz"), **rec)
    np.savez_compressed(os.path.join(OUT, f"ga2_round{steps}_b{batch}_all.npz"), **full)
    print("GA2 losses", losses[:3], "...", losses[-3:])


GA3_OVERFLOW = (2, 5)


def golden_ga3():
    """accelerate's AcceleratedOptimizer / AcceleratedScheduler + torch.amp.GradScaler around the non-dat train_step
    (golden_g15's recipe), 2 layers, B = 4, 224, 7 steps; inf injected into one adapter gradient element at steps 2 and 5."""
    from accelerate import Accelerator
    from accelerate.optimizer import AcceleratedOptimizer
    from accelerate.scheduler import AcceleratedScheduler
    from transformers import get_polynomial_decay_schedule_with_warmup
    Accelerator(cpu=True)
    d = O.ViltDims(layers=2)
    model = build_adapter_model(d, ["art"])
    steps = 7
    batches = [O.synthetic_batch(4, 224, 1500 + s) for s in range(steps)]
    tr = adapter_trainer("art", steps)
    scaler = torch.amp.GradScaler("cpu")
    calls = {"n": 0}

    class Acc:
        device = torch.device("cpu")

        @staticmethod
        def backward(loss):
            scaler.scale(loss).backward()
            step = calls["n"]
            calls["n"] += 1
            if step in GA3_OVERFLOW:
                tgt = [p for n, p in model.named_parameters() if "adapter_up.weight" in n and p.grad is not None][0]
                tgt.grad.view(-1)[7] = float("inf")
    tr.accelerator = Acc()
    opt = tr.create_optimizer(model, "adapter")
    sch = get_polynomial_decay_schedule_with_warmup(opt, num_warmup_steps=int(tr.max_steps * tr.warmup_ratio),
                                                    num_training_steps=tr.max_steps, lr_end=0, power=1)
    aopt = AcceleratedOptimizer(opt, device_placement=False, scaler=scaler)
    asch = AcceleratedScheduler(sch, aopt, step_with_optimizer=True, split_batches=False)
    model.zero_grad()
    w = _Wrap(model)
    rec = {"losses": [], "scale": [], "sched_t": []}
    for step, b in enumerate(batches):
        rec["losses"].append(float(tr.train_step(w, step, dict(b), aopt, asch)))
        rec["scale"].append(scaler.get_scale())
        rec["sched_t"].append(sch.last_epoch)
    rec = {k: np.array(v, np.float32) for k, v in rec.items()}
    rec["overflow_steps"] = np.array(GA3_OVERFLOW, np.int64)
    for k, v in model.state_dict().items():
        if trainable(k):
            put(rec, "after." + k, v)
    np.savez_compressed(os.path.join(OUT, "ga3_scaler_skip.npz"), **rec)
    print("GA3 losses", rec["losses"], "scale", rec["scale"], "sched_t", rec["sched_t"])


GA4 = dict(tasks=["art", "abstract"], steps=[3, 2], rounds=2, batch=4, res=224, seed=42, layers=2)


def golden_ga4():
    """Two clients x 3 / 2 steps, two rounds of the reference's FL loop in optimizer_mode adapter (main.py:466-510):
    deepcopy(server) + personal 'task' tensors, local update, personal tensors back, get_average_net over the communicated
    'adapter' keys (clf keys skipped) with equal weights.  Weights and batches are what `python -m feddat_amd.train
    --optimizer_mode adapter --num_layers 2 --image_size 224 --batch_size 4 --ordered_cl_tasks art,abstract
    --synthetic_steps 3,2 --comm_rounds 2` builds (vilt_spec.random_init / synthetic_batch, seed 42).  Stored after each round:
    the server adapter's update as float16 of dW * 256 (every element), the heads in put()'s whole / sampled form."""
    c = GA4
    d = O.ViltDims(layers=c["layers"])
    params = vilt_spec.random_init(c["layers"], c["tasks"], seed=c["seed"], optimizer_mode="adapter")
    server = build_adapter_model(d, c["tasks"], values=params)
    get_average_net = MG.load_get_average_net()
    names = mode_names([k for k in server.state_dict() if "active_adapter" not in k], "adapter")
    assert names["communicated"] == server.comm_state_dict_names
    personal = {t: {n: v.clone() for n, v in server.state_dict().items() if n in names["personal"]} for t in c["tasks"]}
    data = {t: [vilt_spec.synthetic_batch(c["batch"], c["res"], c["seed"] + 1000 * ti + s) for s in range(c["steps"][ti])]
            for ti, t in enumerate(c["tasks"])}
    rec = {}
    for rnd in range(c["rounds"]):
        c_models = []
        for t in c["tasks"]:
            m = copy.deepcopy(server)
            with torch.no_grad():
                for n, v in personal[t].items():
                    m.state_dict()[n].copy_(v)
            local_update(m, t, data[t])
            personal[t] = {n: v.detach().clone() for n, v in m.state_dict().items() if n in names["personal"]}
            c_models.append({n: v.detach().clone() for n, v in m.state_dict().items() if n in server.comm_state_dict_names})
        server = get_average_net(server, c_models, [1.0] * len(c_models), c["tasks"], torch.device("cpu"))
        for n in names["communicated"]:      # the server adapter's update from the initial weights, every element
            rec[f"r{rnd}.server.dall::" + n] = ((server.state_dict()[n] - params[n]) * 256.0).to(torch.float16).numpy()
        for t in c["tasks"]:
            for n, v in personal[t].items():
                if n.startswith(f"task_layer.{t}."):
                    put(rec, f"r{rnd}.{t}." + n, v)
    np.savez_compressed(os.path.join(OUT, "ga4_round_2clients.npz"), **rec)
    print("GA4 written")


if __name__ == "__main__":
    which = sys.argv[1:] or ["ga1", "ga3", "ga4", "ga2"]
    torch.manual_seed(0)
    for w in which:
        globals()["golden_" + w]()
