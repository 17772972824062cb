"""A short last batch (n < B samples) through the ViLT engines of all four optimizer modes, the trainer and train.main
(DESIGN.md section 5c): the step runs in the engine's static B-sample frame with samples [n, B) replicas of real ones and an
exactly zero loss gradient in their rows, is never captured, and leaves the full-batch path and its hipGraph as they are.

References: the live CPU oracle (O.DatClient) and the reference's own 4 / 4 / 3 local updates (tests/golden/gs1_short_*.npz,
tools/make_shortbatch_golden.py).  Tolerances are the ones the full-batch tests of each mode use: losses 2e-3 relative, logits
3e-2, every element of every update within 1e-3 and its mean error within REL_MEAN of the mean update."""
import functools

import numpy as np
import pytest
import torch

from oracle import feddat_oracle as O
from tests.golden_util import assert_update_parity, golden_tensor, load, sampled_update_parity
from tests.test_adapter_mode_gpu import adapter_params
from tests.test_short_batch_cpu import SIZES, short_batches
from tests.test_vector_mode_gpu import _is_key_bias, plain_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL_MEAN = 0.1
TASKS = ["art", "gqa"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _dev(b):
    return {k: v.to(DEV) for k, v in b.items()}


def _first(b, n):
    return {k: v[:n].clone() for k, v in b.items()}


def _engine(mode, P, B=4, tasks=TASKS, **kw):
    if mode == "dat":
        from feddat_amd.engine import ViltDatEngine
        return ViltDatEngine(P, tasks, DEV, batch=B, res=224, layers=2, **kw)
    if mode == "adapter":
        from feddat_amd.adapter_engine import ViltAdapterEngine
        return ViltAdapterEngine(P, tasks, DEV, batch=B, res=224, layers=2, **kw)
    from feddat_amd.vector_engine import ViltVectorEngine
    return ViltVectorEngine(P, tasks, DEV, batch=B, res=224, layers=2, mode=mode, **kw)


def _params(mode, tasks=TASKS):
    if mode == "dat":
        return O.make_params(O.ViltDims(layers=2), tasks, bias_std=0.02)
    return adapter_params(2, tasks) if mode == "adapter" else plain_params(2, tasks)


def _step_state(eng):
    """Every device tensor a train_step advances."""
    return [t for _, g in eng._named_groups() for t in (g.p, g.m, g.v, g.state)] + \
        [eng.scaler_f, eng.scaler_i, eng.ovf_flags] + eng._extra_step_state()


def _save(eng):
    return [t.clone() for t in _step_state(eng)]


def _load(eng, saved):
    for t, v in zip(_step_state(eng), saved):
        t.copy_(v)
    eng.repack()


def _trained(eng):
    torch.cuda.synchronize()
    return {f"{name}.{f}": getattr(g, f).clone() for name, g in eng._named_groups() for f in ("p", "m", "v")}


def _same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------------- dat vs the live oracle
@functools.lru_cache(maxsize=None)
def _oracle_dat():
    """O.DatClient over the 4 / 4 / 3 batches, once for all cases: per-step (loss_0, L0, L1), the tensors after step 3 and the
    autograd dL_0 / dlogits of the short step's P2 pass."""
    d = O.ViltDims(layers=2)
    P = O.make_params(d, TASKS, bias_std=0.02)
    client = O.DatClient(P, d, "art", lr=1e-4, steps_per_epoch=3)
    steps = []
    for b in short_batches(1234):
        loss0, _, logits_1, logits_0 = client.train_step(b)
        steps.append((float(loss0), client.last_L0, client.last_L1))
    lg = logits_0.clone().requires_grad_(True)
    O.dat_loss(lg, b["target_scores"], logits_1).backward()
    return steps, {k: v.detach().clone() for k, v in P.items()}, lg.grad.detach().clone()


def _golden_updates(g, sd, P0, pre="after3."):
    """Every tensor of a gs1_short fixture against the engine, on the update: adapters (dall::, float16 of dW * 256), backbone
    vectors (d::, dW), heads (whole or 2048 samples)."""
    worst = []
    for tag, scale in (("dall::", 256.0), ("d::", 1.0)):
        names = [k[len(pre + tag):] for k in g if k.startswith(pre + tag)]
        ref = {k: P0[k] + torch.from_numpy(g[pre + tag + k].astype(np.float32)) / scale for k in names}
        strict = [k for k in names if not _is_key_bias(k)]
        worst.append(assert_update_parity(strict, sd, ref, P0, 1e-3, REL_MEAN, pre))
        for k in names:
            if _is_key_bias(k):      # rounding noise normalised by Adam (tests/test_vector_mode_gpu.py): the element bound only
                assert float((sd[k].cpu() - ref[k]).abs().max()) < 1e-3, k
    whole = [k[len(pre):] for k in g if k.startswith(pre) and "::" not in k]
    worst.append(assert_update_parity(whole, sd, {k: golden_tensor(g, pre + k).reshape(P0[k].shape) for k in whole}, P0, 1e-3,
                                      REL_MEAN, pre))
    worst.append(sampled_update_parity(g, pre, sd, P0, 2048, 1e-3, REL_MEAN))
    assert len(whole) >= 4
    return max(w[0] for w in worst), max(w[1] for w in worst)


@pytest.mark.parametrize("operands", ["f16", "bf16"])
@pytest.mark.parametrize("use_graph", [False, True])
def test_dat_short_last_batch_vs_oracle_and_reference(golden_dir, use_graph, operands):
    g = load(golden_dir, "gs1_short_dat.npz")
    steps, P_ref, dl_ref = _oracle_dat()
    P = _params("dat")
    P0 = {k: v.clone() for k, v in P.items()}
    eng = _engine("dat", P, operands=operands)
    eng.begin_local_update("art", steps_per_epoch=3)
    for s, b in enumerate(short_batches(1234)):
        out = eng.train_step(_dev(b), use_graph=use_graph)
        torch.cuda.synchronize()
        ref_loss, ref_L0, ref_L1 = steps[s]
        print(f"step {s + 1} ({SIZES[s]} samples): loss {float(out[0]):.5f} oracle {ref_loss:.5f} reference {float(g['losses'][s]):.5f}")
        assert abs(float(out[0]) - ref_loss) < 2e-3 * abs(ref_loss) + 2e-3, (s, float(out[0]), ref_loss)
        assert abs(float(out[0]) - float(g["losses"][s])) < 2e-3 * abs(ref_loss) + 2e-3
        assert abs(float(out[2]) - ref_L0) < 2e-3 * abs(ref_L0) + 2e-3
        assert abs(float(eng.loss_buf["p1"][2]) - ref_L1) < 2e-3 * abs(ref_L1) + 2e-3
        assert eng.n_valid == SIZES[s]
    # counters: a short step is one step
    assert eng.head["art"].state.tolist() == [6, 6] and eng.ad[1].state.tolist() == [6, 3] and eng.ad[0].state.tolist() == [7, 3]
    assert eng.scaler_state()["skipped_substeps"] == 0
    # the divisor of the short step's gradient is n, not B (AdamW's normalisation would hide a factor on the update)
    got, want = float(eng.dlogits[:3].abs().sum()), float(dl_ref.abs().sum())
    print(f"sum |dlogits[:3]| of P2: {got:.6f}, oracle autograd {want:.6f}")
    assert abs(got - want) <= 0.1 * want
    assert torch.equal(eng.dlogits[3:], torch.zeros_like(eng.dlogits[3:]))
    names = O.trainable_names(P, "art", 0) + [n for n in O.trainable_names(P, "art", 1) if "adapter_1" in n]
    sd = eng.state_dict()
    w = assert_update_parity(names, sd, P_ref, P0, 1e-3, REL_MEAN, "oracle step 3")
    wg = _golden_updates(g, sd, P0)
    print(f"dat {operands} graph {use_graph}: worst (max |ddW|, mean ratio) vs oracle {w}, vs the reference {wg}")
    # adapter_2 is the frozen teacher = adapter_1 at the start of the local update; nothing may have touched it or the other head
    assert all(torch.equal(sd[n].cpu(), P0[n.replace("adapter_2", "adapter_1")]) for n in sd if "adapter_2" in n)
    assert all(torch.equal(sd[n].cpu(), P0[n]) for n in sd if n.startswith("task_layer.gqa."))


# ------------------------------------------------------------------------------------------------------- adapter / bias / norm
@pytest.mark.parametrize("operands,use_graph", [("f16", True), ("f16", False), ("bf16", True)])
@pytest.mark.parametrize("mode", ["adapter", "bias", "norm"])
def test_single_pass_modes_short_last_batch_vs_reference(golden_dir, mode, operands, use_graph):
    g = load(golden_dir, f"gs1_short_{mode}.npz")
    P = _params(mode)
    P0 = {k: v.clone() for k, v in P.items()}
    eng = _engine(mode, P, operands=operands)
    eng.begin_local_update("art", steps_per_epoch=3)
    trained = eng.ad[0] if mode == "adapter" else eng.vec
    for s, b in enumerate(short_batches(int(g["seed0"]))):
        out = eng.train_step(_dev(b), use_graph=use_graph)
        ref = float(g["losses"][s])
        print(f"{mode} step {s + 1} ({SIZES[s]} samples): loss {float(out[0]):.5f} reference {ref:.5f}")
        assert abs(float(out[0]) - ref) < 2e-3 * abs(ref) + 2e-3, (s, float(out[0]), ref)
        assert trained.state.tolist() == [s + 1, s + 1] == eng.head["art"].state.tolist()
    assert eng.scaler_state()["skipped_substeps"] == 0
    assert torch.equal(eng.dlogits[3:], torch.zeros_like(eng.dlogits[3:]))
    sd = eng.state_dict()
    stored = [k.split("::")[-1] for k in g if k.startswith("after3.") and "::" in k]
    if mode == "adapter":
        assert len(stored) == 8
    else:
        assert sorted(stored) == sorted(eng.vec.names)
    w = _golden_updates(g, sd, P0)
    print(f"{mode} {operands} graph {use_graph}: worst max |ddW| {w[0]:.2e}, worst mean ratio {w[1]:.3f}")
    assert all(torch.equal(sd[k].cpu(), P0[k]) for k in sd if k.startswith("task_layer.gqa."))


# ------------------------------------------------------------------------------------------------------- the tail of the frame
@pytest.mark.parametrize("mode", ["dat", "adapter", "bias", "norm"])
def test_the_tail_of_the_frame_is_fully_overwritten(mode):
    """"full batch X, then short batch s" twice from one state, X differing between the runs and the trained state restored
    after X: whatever X leaves in the frame (its samples, its dlogits) must not reach the short step."""
    B, n = 5, 2
    eng = _engine(mode, _params(mode, ["art"]), B=B, tasks=["art"])
    eng.begin_local_update("art", steps_per_epoch=4)
    state0 = _save(eng)
    short = _dev(_first(O.synthetic_batch(B, 224, 77), n))
    runs = []
    for seed in (500, 600):
        _load(eng, state0)
        eng.train_step(_dev(O.synthetic_batch(B, 224, seed)))
        _load(eng, state0)
        eng.train_step(short)
        runs.append(_trained(eng))
        assert eng.n_valid == n
        for k, v in list(eng.inp.items()) + [("patches", eng.patches.view(B, -1))]:
            for j in range(n, B):
                assert torch.equal(v[j], v[j % n]), (k, j)
        assert torch.equal(eng.inp["input_ids"][:n], short["input_ids"])
        assert torch.equal(eng.inp["target"][:n], short["target_scores"])
        assert torch.equal(eng.dlogits[n:], torch.zeros_like(eng.dlogits[n:]))
    _same_bits(runs[0], runs[1])
    assert all(bool(torch.isfinite(t).all()) for t in runs[0].values())
    assert any(not torch.equal(t, s) for t, s in zip(_step_state(eng), state0))


# ------------------------------------------------------------------------------------------------------- the graph
def test_a_short_step_leaves_the_captured_graph_alone():
    """use_graph=True: full (captures), short (eager, same stream), full (replay) == the same three steps run eagerly."""
    batches = [_dev(O.synthetic_batch(4, 224, 40)), _dev(_first(O.synthetic_batch(4, 224, 41), 3)),
               _dev(O.synthetic_batch(4, 224, 42))]
    out = {}
    for use_graph in (True, False):
        eng = _engine("dat", _params("dat", ["art"]), tasks=["art"])
        eng.begin_local_update("art", steps_per_epoch=3)
        eng.train_step(batches[0], use_graph=use_graph)
        graph, sig = eng.graph, eng._graph_sig
        assert (graph is not None) == use_graph
        eng.train_step(batches[1], use_graph=use_graph)
        assert eng.graph is graph and eng._graph_sig == sig and eng.n_valid == 3
        eng.train_step(batches[2], use_graph=use_graph)
        assert eng.graph is graph and eng.n_valid == 4
        out[use_graph] = _trained(eng)
    _same_bits(out[True], out[False])


@pytest.mark.parametrize("mode", ["dat", "bias"])
def test_capture_with_a_short_batch_staged_captures_the_full_step(mode):
    """A loader whose first (or only) batch is short: ensure_captured() still captures the full-batch launch list and puts
    the staged row count back; a full batch replayed on that graph equals an engine that never saw the short one."""
    full = _dev(O.synthetic_batch(4, 224, 50))
    out = []
    for stage_short in (True, False):
        eng = _engine(mode, _params(mode, ["art"]), tasks=["art"])
        eng.begin_local_update("art", steps_per_epoch=2)
        if stage_short:
            eng.set_batch(_dev(_first(O.synthetic_batch(4, 224, 51), 1)))
            before = _save(eng)
            eng.ensure_captured()
            assert eng.n_valid == 1 and eng.graph is not None
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(_step_state(eng), before))      # capturing does not train
        eng.train_step(full, use_graph=True)
        out.append(_trained(eng))
    _same_bits(out[0], out[1])


# ------------------------------------------------------------------------------------------------------- eval
def test_eval_scores_the_samples_of_a_short_last_batch():
    import types
    from feddat_amd import lib as L, modeling, train
    d = O.ViltDims(layers=2)
    P = O.make_params(d, ["art"], bias_std=0.02)
    m = modeling.create_vilt_continual_learner_model(P, ["art"], DEV, batch_size=4, image_size=224, num_layers=2)
    args = types.SimpleNamespace(local_epochs=1, num_epochs=15, lr=1e-4, optimizer_mode="dat", debug=0, hip_graph=False)
    host = short_batches(900)
    loader = [_dev(b) for b in host]
    trainer = train.TaskTrainer(args, "art", [], loader)
    for mode in ("gating", "adapter_0", "adapter_1"):
        if mode == "gating":
            m.activate_gating()
        else:
            m.deactivate_gating()
            m.set_active_adapter(mode)
        acc, host_score = torch.zeros(2, device=DEV), 0.0
        for hb, b in zip(host, loader):
            pooled, logits = m(task_key="art", images=b, texts=None)
            n = hb["input_ids"].shape[0]
            assert logits.shape == (n, 100) and pooled.shape == (n, 768)
            L.vqa_score_accumulate(logits, b["target_scores"], acc)
            host_score += float(hb["target_scores"].gather(1, logits.cpu().argmax(1, keepdim=True)).sum())
        with torch.no_grad():
            _, ref = O.vilt_forward(P, d, host[2], mode, "art")
        assert (logits.cpu() - ref).abs().max() < 3e-2, mode
        score, seen = acc.tolist()
        assert seen == 11.0 and score == pytest.approx(host_score, abs=1e-4)
        assert trainer.eval_one_loader(m, loader) == pytest.approx(100.0 * host_score / 11, abs=1e-3)
    assert len(trainer.eval(m)) == 3


@pytest.mark.parametrize("mode", ["adapter", "bias", "norm"])
def test_single_pass_modes_forward_and_eval_on_a_short_last_batch(golden_dir, mode):
    """engine.forward of the single-pass engines returns the n real rows, equal (3e-2, the forward tolerance) to the same
    samples inside a full batch, whose samples do not interact; TaskTrainer.eval over 4 / 4 / 3 scores 11 samples."""
    import types
    from feddat_amd import lib as L, modeling, train
    P = _params(mode, ["art"])
    m = modeling.create_vilt_continual_learner_model(P, ["art"], DEV, batch_size=4, image_size=224, num_layers=2,
                                                     optimizer_mode=mode)
    full = _dev(O.synthetic_batch(4, 224, 902))
    p4, l4 = m.engine.forward(full, "art")
    assert p4.shape == (4, 768) and l4.shape == (4, 100)
    for n in (3, 1):
        pn, ln = m.engine.forward(_first(full, n), "art")
        assert pn.shape == (n, 768) and ln.shape == (n, 100) and m.engine.n_valid == n
        assert (pn - p4[:n]).abs().max() < 3e-2 and (ln - l4[:n]).abs().max() < 3e-2
    if mode == "adapter":      # the reference's own forward of this model (ga1) on the first three samples of its batch
        g = load(golden_dir, "ga1_vilt2_adapter.npz")
        eng = _engine(mode, _params(mode))
        _, lg = eng.forward(_dev(_first(O.synthetic_batch(4, 224, 1234), 3)), "art")
        assert (lg.cpu() - torch.from_numpy(g["224.fwd.logits"])[:3]).abs().max() < 3e-2
    args = types.SimpleNamespace(local_epochs=1, num_epochs=15, lr=1e-4, optimizer_mode=mode, debug=0, hip_graph=False)
    host = short_batches(900)
    loader = [_dev(b) for b in host]
    acc, host_score = torch.zeros(2, device=DEV), 0.0
    for hb, b in zip(host, loader):
        _, logits = m(task_key="art", images=b, texts=None)
        assert logits.shape == (hb["input_ids"].shape[0], 100)
        L.vqa_score_accumulate(logits, b["target_scores"], acc)
        host_score += float(hb["target_scores"].gather(1, logits.cpu().argmax(1, keepdim=True)).sum())
    score, seen = acc.tolist()
    assert seen == 11.0 and score == pytest.approx(host_score, abs=1e-4)
    assert train.TaskTrainer(args, "art", [], loader).eval(m) == pytest.approx(100.0 * host_score / 11, abs=1e-3)


# ------------------------------------------------------------------------------------------------------- trainer
def test_trainer_trains_a_loader_whose_last_batch_is_short():
    """TaskTrainer.train over host batches of 4 / 4 / 3 (upload worker + prefetch stream, hipGraph for the full steps, the short
    one eager): max_steps counts the short step, and the trained state carries the bits of the same three steps issued
    directly on an engine."""
    import types
    from feddat_amd import modeling, train
    host = short_batches(700)
    m = modeling.create_vilt_continual_learner_model(_params("dat", ["art"]), ["art"], DEV, batch_size=4, image_size=224,
                                                     num_layers=2)
    args = types.SimpleNamespace(local_epochs=1, num_epochs=15, lr=1e-4, optimizer_mode="dat", debug=0, hip_graph=True)
    trainer = train.TaskTrainer(args, "art", host)
    assert trainer.max_steps == 3 * 15
    trainer.train(m)
    assert m.engine.n_valid == 3 and m.engine.graph is not None
    eng = _engine("dat", _params("dat", ["art"]), tasks=["art"])
    eng.begin_local_update("art", steps_per_epoch=3)
    for b in host:
        eng.train_step(_dev(b))
    _same_bits(_trained(m.engine), _trained(eng))


def test_raw_batches_with_a_short_last_batch_through_the_trainer(golden_dir):
    """The reference's batch schema ({"images", "raw_texts", "target_scores"}) with 4 and then 3 samples: encode_batch ->
    process_inputs (device image processor + tokenizer) gives n-row encodings equal to the host oracle's, and TaskTrainer.train
    (upload worker + prefetch stream) / eval over that loader follow the oracle client on the host-processed batches."""
    import types
    from feddat_amd import modeling, train
    from tests.test_weights_gpu import _oracle_encodings, _raw_batch
    B, frame = 4, (384, 640)
    d = O.ViltDims(layers=2)
    P = O.make_params(d, ["art"], bias_std=0.02)
    P0 = {k: v.clone() for k, v in P.items()}
    vocab, raw4 = _raw_batch(golden_dir, B, 5)
    _, raw = _raw_batch(golden_dir, B, 9)
    raw3 = {"images": raw["images"][:3], "raw_texts": raw["raw_texts"][:3], "target_scores": raw["target_scores"][:3].clone()}
    raws = [raw4, raw3]
    model = modeling.create_vilt_continual_learner_model(P, ["art"], DEV, B, frame, 2, vocab=vocab)
    args = types.SimpleNamespace(local_epochs=1, num_epochs=15, lr=1e-4, optimizer_mode="dat", debug=0, hip_graph=True,
                                 prefetch=True)
    tr = train.TaskTrainer(args, "art", raws, raws)
    enc, ref = tr.encode_batch(model, raw3), _oracle_encodings(vocab, raw3, frame)
    assert enc["pixel_values"].shape == (3, 3) + frame
    for k in ("pixel_values", "pixel_mask", "input_ids", "attention_mask", "token_type_ids", "target_scores"):
        assert enc[k].dtype == ref[k].dtype and torch.equal(enc[k].cpu(), ref[k]), k
    tr.train(model)
    torch.cuda.synchronize()
    assert model.engine.n_valid == 3
    client = O.DatClient(P, d, "art", lr=1e-4, steps_per_epoch=2)
    for r in raws:
        client.train_step(_oracle_encodings(vocab, r, frame))
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    assert_update_parity([n for n in sd if "adapter_2" not in n], sd, P, P0, 1e-3, REL_MEAN, "raw short batch")
    scores = tr.eval(model)
    assert len(scores) == 3 and all(0.0 <= x <= 100.0 for x in scores)
    acc = torch.zeros(2, device=DEV)
    from feddat_amd import lib as L
    for r in raws:
        b = tr.encode_batch(model, r)
        _, logits = model(task_key="art", images=b, texts=None)
        L.vqa_score_accumulate(logits, b["target_scores"], acc)
    assert acc.tolist()[1] == 7.0


# ------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from feddat_amd import lib as L
    P = _params("dat", ["art"])
    eng = _engine("dat", P, tasks=["art"])
    b4 = O.synthetic_batch(4, 224, 3)
    with pytest.raises(L.FeddatHipError):
        eng.set_batch(_dev(_first(b4, 0)))
    with pytest.raises(L.FeddatHipError):
        eng.set_batch(_dev(O.synthetic_batch(5, 224, 3)))
    with pytest.raises(L.FeddatHipError):      # the other dimensions stay what the engine was built for
        eng.set_batch(_dev(_first(O.synthetic_batch(4, 256, 3), 3)))
    assert eng.n_valid == 4
    eng8 = _engine("dat", P, tasks=["art"], fp8=True)
    with pytest.raises(L.FeddatHipError, match="fp8"):
        eng8.set_batch(_dev(_first(b4, 3)))
    with pytest.raises(L.FeddatHipError, match="fp8"):
        eng8.train_step(_dev(_first(b4, 3)))
    eng8.set_batch(_dev(b4))
    assert eng8.n_valid == 4


# ------------------------------------------------------------------------------------------------------- train.main
@pytest.mark.parametrize("mode", ["dat", "bias"])
def test_main_with_a_short_last_batch(mode):
    from feddat_amd import train
    common = ["--optimizer_mode", mode, "--batch_size", "4", "--num_layers", "2", "--image_size", "224", "--comm_rounds", "2",
              "--ordered_cl_tasks", "art,gqa", "--synthetic_steps", "3"]
    short = ["--synthetic_last_batch", "3"]
    a = train.main(common + short).engine.comm_flat().clone()
    b = train.main(common + short).engine.comm_flat().clone()
    full = train.main(common).engine.comm_flat().clone()
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a, b)
    assert not torch.equal(a, full)
