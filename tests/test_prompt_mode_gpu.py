"""optimizer_mode 'prompt' on the MI355X: prompt_engine.ViltPromptEngine against the reference's fixtures tests/golden/gp*
(written by tools/make_prompt_golden.py) and the public calls train.main drives a federation with.

Tolerances are test_vector_mode_gpu.py's: pooled / logits 3e-2, losses 2e-3 relative + 2e-3, updates by assert_update_parity
(every element < 1e-3, mean error <= REL_MEAN of the mean update).  Gradients: next to the fp32 gradient g of every trainable
tensor the fixture stores g16, the gradient of the same reference modules under torch.autocast("cpu", bfloat16);
e16 = max|g16 - g| / max|g| is what a 16-bit implementation of this step costs by the reference's own account, and both operand
builds must stay within 2 x e16 per tensor."""
import numpy as np
import pytest
import torch

from oracle import feddat_oracle as O
from tests.golden_util import assert_update_parity, golden_tensor, load, sampled_update_parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL_MEAN = 0.1
MODE = "prompt"
PROMPT_SEED = 77      # tools/make_prompt_golden.py
GV1_VALID = [(224, 224), (160, 224), (224, 128), (96, 192)]
GV1_TEXT = [40, 31, 40, 12]
TASKS = ["art", "gqa"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def prompt_params(layers, tasks):
    """The fixtures' weights: the name-seeded fill of the dat fixtures on the plain backbone's keys (as gv1) plus
    vilt_spec.prompt_init(PROMPT_SEED)."""
    from feddat_amd import vilt_spec
    out = {}
    for k, shp in O.param_shapes(O.ViltDims(layers=layers), tasks).items():
        if ".adapter." not in k:
            out[k.replace(".output.layer.dense.", ".output.dense.")] = O.seeded_value(k, shp, 0.02, 0.02)
    out.update(vilt_spec.prompt_init(PROMPT_SEED))
    return out


def _dev(b):
    return {k: v.to(DEV) for k, v in b.items()}


def _engine(P, tasks, B=4, res=224, layers=2, **kw):
    from feddat_amd.prompt_engine import ViltPromptEngine
    return ViltPromptEngine(P, tasks, DEV, batch=B, res=res, layers=layers, **kw)


def _batches(case, n, seed0=2000):
    bs = [O.synthetic_batch(4, 224, seed0 + s) for s in range(n)]
    return [O.pad_batch(b, GV1_VALID, GV1_TEXT) for b in bs] if case == "padded" else bs


def _vis(sd):
    return [k for k in sd if "prompt_embedding_vis" in k]


def _golden_rule(g, key, got):
    """(reference, reference under bf16 autocast, ours) of one gradient: whole tensors or put()'s 2048 strided samples."""
    flat = got.flatten()
    if key[0] in g:
        return torch.from_numpy(g[key[0]]).flatten(), torch.from_numpy(g[key[1]]).flatten(), flat
    idx = torch.linspace(0, flat.numel() - 1, 2048).long()
    return torch.from_numpy(g["samp::" + key[0]]), torch.from_numpy(g["samp::" + key[1]]), flat[idx]


# ------------------------------------------------------------------------------------------------------- gp1: forward, gradients
@pytest.mark.parametrize("case", ["plain", "padded"])
@pytest.mark.parametrize("operands", ["bf16", "f16"])
def test_forward_and_gradient_of_every_trainable_tensor(golden_dir, operands, case):
    g = load(golden_dir, "gp1_vilt2_prompt.npz")
    pre = f"{case}."
    P = prompt_params(2, TASKS)
    eng = _engine(P, TASKS, operands=operands, dynamic_loss_scale=False)
    assert eng.S == 100 and eng.S0 == 90
    batch = _batches(case, 1)[0]
    pooled, logits = eng.forward(_dev(batch), "art")
    dp = float((pooled.cpu() - torch.from_numpy(g[pre + "fwd.pooled"])).abs().max())
    dl = float((logits.cpu() - torch.from_numpy(g[pre + "fwd.logits"])).abs().max())
    eng.begin_local_update("art", steps_per_epoch=4)
    loss = float(eng.train_step(_dev(batch), use_graph=False)[0])
    ref_loss = float(g[pre + "loss"])
    print(f"gp1 {operands} {case}: |pooled| {dp:.2e} |logits| {dl:.2e} loss {loss:.5f} (ref {ref_loss:.5f})")
    assert dp < 3e-2 and dl < 3e-2
    assert abs(loss - ref_loss) < 2e-3 * abs(ref_loss) + 2e-3
    torch.cuda.synchronize()
    hp = eng.head["art"]
    grads = {n: eng.text.view(n, eng.text.g).cpu() for n in eng.text.names}
    grads.update({n: hp.view(n, hp.g).cpu() for n in hp.names})
    stored = sorted({k.split("g::", 1)[1] for k in g if k.startswith((pre + "g::", "samp::" + pre + "g::"))})
    assert stored == sorted(grads)      # every tensor the reference gives a gradient: the text module and this task's head
    assert sorted(g[pre + "nograd"].tolist()) == sorted(_vis(eng.state_dict()) + [k for k in eng.state_dict()
                                                                                 if k.startswith("task_layer.gqa.")])
    fails = []
    for n in stored:
        ref, ref16, got = _golden_rule(g, (pre + "g::" + n, pre + "g16::" + n), grads[n])
        gmax = float(ref.abs().max())
        e16, err = float((ref16 - ref).abs().max()) / gmax, float((got - ref).abs().max()) / gmax
        print(f"   {n}: e16 {e16:.3e}  ours {err:.3e}  bound {2 * e16:.3e}  ours / e16 {err / e16:.2f}")
        if not err <= 2 * e16:
            fails.append((n, "err / max|g|", err, "e16", e16))
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------- gp1: four steps
@pytest.mark.parametrize("case", ["plain", "padded"])
@pytest.mark.parametrize("operands,use_graph", [("f16", False), ("f16", True), ("bf16", False), ("bf16", True)])
def test_two_layer_engine_vs_reference(golden_dir, operands, use_graph, case):
    from feddat_amd.modes import mode_names
    g = load(golden_dir, "gp1_vilt2_prompt.npz")
    pre = f"{case}."
    P = prompt_params(2, TASKS)
    P0 = {k: v.clone() for k, v in P.items()}
    eng = _engine(P, TASKS, operands=operands)
    batches = _batches(case, 4)
    eng.begin_local_update("art", steps_per_epoch=4)
    if use_graph:
        eng.set_batch(_dev(O.synthetic_batch(4, 224, 1)))
        eng.ensure_captured()
    for s in range(4):
        out = eng.train_step(_dev(batches[s]), use_graph=use_graph)
        ref = float(g[pre + "losses"][s])
        assert abs(float(out[0]) - ref) < 2e-3 * abs(ref) + 2e-3, (s, float(out[0]), ref)
        assert eng.text.state.tolist() == [s + 1, s + 1] == eng.head["art"].state.tolist()
        if s + 1 in (1, 4):
            sd = eng.state_dict()
            p = pre + f"after{s + 1}."
            whole = [k[len(p):] for k in g if k.startswith(p)]
            w2 = assert_update_parity(whole, sd, {k: golden_tensor(g, p + k).reshape(P0[k].shape) for k in whole}, P0, 1e-3,
                                      REL_MEAN, p)
            w3 = sampled_update_parity(g, p, sd, P0, 2048, 1e-3, REL_MEAN)
            sampled = [k[len("samp::") + len(p):] for k in g if k.startswith("samp::" + p)]
            assert sorted(whole + sampled) == sorted(eng.text.names + eng.head["art"].names)
            print(f"gp1 {operands} graph {use_graph} {case} after {s + 1}: worst max {max(w2[0], w3[0]):.2e} "
                  f"worst mean ratio {max(w2[1], w3[1]):.3f}")
    assert eng.scaler_state()["skipped_substeps"] == 0
    sd = eng.state_dict()
    assert all(torch.equal(sd[k].cpu(), P0[k]) for k in sd if k.startswith("task_layer.gqa."))
    vis = _vis(sd)
    assert len(vis) == 5 and all(torch.equal(sd[k].cpu(), P0[k]) for k in vis)      # inert payload: bit-equal to the initial values
    assert sorted(sd) == sorted(mode_names(list(P0), MODE)["trainable"])
    assert eng.comm_flat().numel() == 599424
    # comm_flat is the ten tensors in state-dict order, and the kernels read the text tensors in place
    comm = mode_names(list(P0), MODE)["communicated"]
    assert torch.equal(eng.comm_flat(), torch.cat([sd[k].flatten() for k in comm]))
    assert sd[comm[5]].data_ptr() == eng.comm_flat()[299712:].data_ptr()


def test_graph_replay_is_bit_identical_to_eager_and_to_itself():
    outs = []
    for use_graph in (False, True, True):
        eng = _engine(prompt_params(2, ["art"]), ["art"])
        eng.begin_local_update("art", steps_per_epoch=3)
        for s in range(3):
            eng.train_step(_dev(O.synthetic_batch(4, 224, 700 + s)), use_graph=use_graph)
        torch.cuda.synchronize()
        outs.append({k: v.clone() for k, v in eng.state_dict().items()})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]) and torch.equal(outs[1][k], outs[2][k]), k


# ------------------------------------------------------------------------------------------------------- skipped step
def test_injected_overflow_skips_the_step_and_halves_the_scale():
    """test_vector_mode_gpu.py's rig: a step whose overflow flag is set leaves parameters, Adam moments and the schedule
    untouched, halves the scale and clears the flag; the next step applies; a scale at which the 16-bit gradient operands
    overflow raises the flag through the gather kernel itself."""
    eng = _engine(prompt_params(2, ["art"]), ["art"])
    s0 = eng.loss_scale
    eng.begin_local_update("art", steps_per_epoch=4)
    hp = eng.head["art"]
    eng.train_step(_dev(O.synthetic_batch(4, 224, 1500)), use_graph=True)
    eng.train_step(_dev(O.synthetic_batch(4, 224, 1501)), use_graph=True)
    torch.cuda.synchronize()
    keep = [t.clone() for grp in (eng.text, hp) for t in (grp.p, grp.m, grp.v, grp.state)] + [eng.comm_flat().clone()]
    eng.ovf_flags[0] = 1
    eng.train_step(_dev(O.synthetic_batch(4, 224, 1502)), use_graph=True)
    torch.cuda.synchronize()
    now = [t for grp in (eng.text, hp) for t in (grp.p, grp.m, grp.v, grp.state)] + [eng.comm_flat()]
    assert all(torch.equal(a, b) for a, b in zip(keep, now))
    st = eng.scaler_state()
    assert st["scale"] == s0 / 2 and st["skipped_substeps"] == 1 and int(eng.ovf_flags[0]) == 0
    assert eng.text.state.tolist() == [2, 2] == hp.state.tolist()
    eng.train_step(_dev(O.synthetic_batch(4, 224, 1503)), use_graph=True)
    torch.cuda.synchronize()
    assert eng.text.state.tolist() == [3, 3] and not torch.equal(keep[0], eng.text.p)
    eng2 = _engine(prompt_params(2, ["art"]), ["art"])
    eng2.begin_local_update("art", steps_per_epoch=4)
    eng2.train_step(_dev(O.synthetic_batch(4, 224, 1500)), use_graph=False)
    p_before = eng2.comm_flat().clone()
    eng2.scaler_f.copy_(torch.tensor([2.0 ** 30, 2.0 ** -30]))
    eng2.train_step(_dev(O.synthetic_batch(4, 224, 1501)), use_graph=False)
    torch.cuda.synchronize()
    assert torch.equal(p_before, eng2.comm_flat()) and eng2.scaler_state()["scale"] == 2.0 ** 29
    assert bool(torch.isfinite(eng2.comm_flat()).all())
    eng2.assert_finite()


# ------------------------------------------------------------------------------------------------------- short last batch vs gp2
@pytest.mark.parametrize("operands", ["f16", "bf16"])
def test_short_last_batch_vs_reference(golden_dir, operands):
    g = load(golden_dir, "gp2_short_prompt.npz")
    P = prompt_params(2, TASKS)
    P0 = {k: v.clone() for k, v in P.items()}
    eng = _engine(P, TASKS, operands=operands)
    eng.begin_local_update("art", steps_per_epoch=3)
    sizes = g["sizes"].tolist()
    graph = None
    for s, n in enumerate(sizes):
        b = O.synthetic_batch(4, 224, int(g["seed0"]) + s)
        out = eng.train_step(_dev({k: v[:n] for k, v in b.items()}), use_graph=True)
        ref = float(g["losses"][s])
        assert abs(float(out[0]) - ref) < 2e-3 * abs(ref) + 2e-3, (s, float(out[0]), ref)
        if s == 0:
            graph = eng.graph
        assert eng.graph is graph and graph is not None      # the n = B path's graph is untouched by the short step
    assert eng.n_valid == 3 and eng.text.state.tolist() == [3, 3]
    sd = eng.state_dict()
    p = "after3."
    whole = [k[len(p):] for k in g if k.startswith(p)]
    w2 = assert_update_parity(whole, sd, {k: golden_tensor(g, p + k).reshape(P0[k].shape) for k in whole}, P0, 1e-3, REL_MEAN, p)
    w3 = sampled_update_parity(g, p, sd, P0, 2048, 1e-3, REL_MEAN)
    sampled = [k[len("samp::") + len(p):] for k in g if k.startswith("samp::" + p)]
    assert sorted(whole + sampled) == sorted(eng.text.names + eng.head["art"].names)
    assert all(torch.equal(sd[k].cpu(), P0[k]) for k in _vis(sd))
    print(f"gp2 {operands}: worst max {max(w2[0], w3[0]):.2e} worst mean ratio {max(w2[1], w3[1]):.3f}")
    # a full batch afterwards replays the same graph
    eng.train_step(_dev(O.synthetic_batch(4, 224, 2100)), use_graph=True)
    assert eng.graph is graph and eng.text.state.tolist() == [4, 4]


# ------------------------------------------------------------------------------------------------------- federation vs gp3
def test_two_clients_two_rounds_vs_reference_federation(golden_dir, tmp_path):
    """The two clients of gp3 driven by hand with the public calls train.main uses (which keeps refusing the mode on the command
    line): load_state_dict, TaskTrainer.train, lib.fedavg_accumulate on comm_flat()."""
    from feddat_amd import checkpoint, lib as L, train, vilt_spec
    from feddat_amd.modeling import create_vilt_continual_learner_model
    from feddat_amd.modes import averaged_names, mode_names
    g = load(golden_dir, "gp3_round_2clients_prompt.npz")
    tasks, steps, seed = ["art", "abstract"], [3, 2], 42
    P0 = vilt_spec.random_init(2, tasks, seed=seed, optimizer_mode=MODE)
    model = create_vilt_continual_learner_model({k: v.clone() for k, v in P0.items()}, tasks, DEV, 4, 224, 2, 1e-4,
                                                optimizer_mode=MODE)
    eng = model.engine
    assert model.comm_state_dict_names == g["names.communicated"].tolist() == averaged_names(list(P0), MODE)
    with pytest.raises(L.FeddatHipError, match="has no adapter"):
        model.set_active_adapter("adapter_0")
    args = train.build_parser().parse_args(["--optimizer_mode", MODE, "--num_layers", "2", "--image_size", "224", "--batch_size", "4"])
    keep = set(mode_names(list(model.state_dict()), MODE)["personal"])
    assert keep == set(g["names.personal"].tolist())
    personal = {t: {n: v.clone() for n, v in model.state_dict().items() if n in keep} for t in tasks}
    data = {t: [vilt_spec.synthetic_batch(4, 224, seed + 1000 * ti + s, device=DEV) for s in range(steps[ti])]
            for ti, t in enumerate(tasks)}
    server_flat = eng.comm_flat().clone()
    acc = torch.zeros_like(server_flat)
    vis = _vis(model.state_dict())
    for rnd in range(2):
        for k, t in enumerate(tasks):
            eng.comm_flat().copy_(server_flat)
            eng.comm_written()
            model.load_state_dict(personal[t])
            tr = train.TaskTrainer(args, t, data[t], data[t][:1])
            tr.train(model, rnd)
            personal[t] = {n: v.clone() for n, v in model.state_dict().items() if n in keep}
            L.fedavg_accumulate(acc, eng.comm_flat(), 1.0, float(len(tasks)), k == 0)
        server_flat.copy_(acc)
        eng.comm_flat().copy_(server_flat)
        sd = model.state_dict()
        p = f"r{rnd}.server."
        whole = [k[len(p):] for k in g if k.startswith(p)]
        w = assert_update_parity(whole, sd, {k: golden_tensor(g, p + k).reshape(P0[k].shape) for k in whole}, P0, 1e-3, REL_MEAN, p)
        w3 = sampled_update_parity(g, p, sd, P0, 2048, 1e-3, REL_MEAN)
        sampled = [k[len("samp::") + len(p):] for k in g if k.startswith("samp::" + p)]
        assert sorted(whole + sampled + vis) == sorted(model.comm_state_dict_names)
        assert all(torch.equal(sd[k].cpu(), P0[k]) for k in vis)      # averaged, still bit-equal to the initial values
        for t in tasks:      # the heads are personal: each client's own, never averaged
            pt = f"r{rnd}.{t}."
            names = [k[len(pt):] for k in g if k.startswith(pt)]
            assert_update_parity(names, personal[t], {k: golden_tensor(g, pt + k).reshape(P0[k].shape) for k in names}, P0,
                                 1e-3, REL_MEAN, pt)
            sampled_update_parity(g, pt, personal[t], P0, 2048, 1e-3, REL_MEAN)
            other = [k for k in personal[t] if not k.startswith(f"task_layer.{t}.")]
            assert other and all(torch.equal(personal[t][k].cpu(), P0[k]) for k in other)
        print(f"gp3 round {rnd}: server worst max {max(w[0], w3[0]):.2e} worst mean ratio {max(w[1], w3[1]):.3f}")
    # one score from eval (no adapter to switch)
    score = train.TaskTrainer(args, "art", data["art"], data["art"][:1]).eval(model)
    assert isinstance(score, float)
    # checkpoint round trip of the payload and the personal tensors
    sd = model.state_dict()
    out = str(tmp_path / "ck")
    checkpoint.save_federation(out, {n: sd[n] for n in model.comm_state_dict_names}, personal, 1)
    comm, pers, last, _ = checkpoint.load_federation(out, tasks)
    assert last == 1 and sorted(comm) == sorted(model.comm_state_dict_names)
    before = eng.comm_flat().clone()
    eng.comm_flat().zero_()
    model.load_state_dict(comm)
    assert torch.equal(eng.comm_flat(), before)
    assert all(torch.equal(pers[t][k], personal[t][k].cpu()) for t in tasks for k in personal[t])


# ------------------------------------------------------------------------------------------------------- images + strings
def test_learner_forward_from_images_and_strings_equals_the_engines(golden_dir):
    from feddat_amd.modeling import ViltContinualLearner
    from tests.test_weights_gpu import _raw_batch
    vocab, raw = _raw_batch(golden_dir, 2, 5)
    frame = (384, 640)
    model = ViltContinualLearner(["art"], prompt_params(2, ["art"]), DEV, batch_size=2, image_size=frame, num_layers=2,
                                 vocab=vocab, optimizer_mode=MODE)
    assert model.engine.S == 40 + 1 + 12 * 20 + 10
    pooled, logits = model("art", raw["images"], raw["raw_texts"])
    enc = model.process_inputs(raw["images"], raw["raw_texts"])
    assert enc["pixel_values"].shape == (2, 3) + frame
    p2, l2 = model.engine.forward(enc, "art")
    assert tuple(logits.shape) == (2, 100) and bool(torch.isfinite(logits).all())
    assert torch.equal(pooled, p2) and torch.equal(logits, l2)
