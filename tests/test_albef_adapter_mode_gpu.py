"""AlbefAdapterEngine (ALBEF optimizer_mode 'adapter', the single-adapter FedAvg baseline) against the reference's own runs with
adapter_config names = ["adapter"] (tests/golden/gb1_albef_adapter_small.npz .. gb4_albef_adapter_2clients.npz;
tools/make_albef_adapter_golden.py), head trained (`head.`: the reference's flags) and frozen (`nohead.`).  Every fixture run
exists in fp32 and under torch.autocast("cpu", bfloat16); the autocast run is the reference's own coarser arithmetic.

Bounds.  Forward: logits 5e-2, loss 3e-3 relative (G10's).  First-step gradient of EVERY trainable tensor: max-abs error to the
fp32 gradient at most the reference's own autocast error of that tensor, factor 1.0 (on the stored strided samples for the large
tensors, both sides).  Losses of the 4-step run 3e-3, of the 40-step run 1e-2 relative; per adapter tensor |ddW|.max < 1e-3,
|ddW|.mean <= 0.1 |dW_ref|.mean (+ norm within 5 % at 40 steps); head updates max(1e-3, autocast max) and
max(0.1 mean |dW_ref|, autocast mean), as tests/test_albef_head_gpu.py holds them.  rank_answer: probabilities 2e-2, top-k id sets."""
import numpy as np
import pytest
import torch

from oracle import albef_oracle as A
from tests.golden_util import load

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = dict(vit_depth=2, enc_layers=3, fusion_layer=1, dec_layers=2, image=64, vocab=3072, max_pos=64)
CLS = "albef_model.albef.text_decoder.cls.predictions."
HEAD = [CLS + n for n in ("bias", "transform.dense.weight", "transform.dense.bias", "transform.LayerNorm.weight",
                          "transform.LayerNorm.bias")]


def _dev(b):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in b.items()}


@pytest.fixture(scope="module")
def mod():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import albef_adapter_engine
    return albef_adapter_engine


@pytest.fixture(scope="module")
def gb1(golden_dir):
    return load(golden_dir, "gb1_albef_adapter_small.npz")


def _params():
    """The fixtures' name-seeded fill of the single-adapter model."""
    from feddat_amd import albef_spec
    return {k: A.O.seeded_value(k, s, 0.02, 0.02) for k, s in albef_spec.param_shapes(optimizer_mode="adapter", **SMALL).items()}


def _engine(mod, P, head, B=3, N=6, **kw):
    return mod.AlbefAdapterEngine(P, DEV, batch=B, n_answers=N, q_len=12, a_len=5, vit_depth=SMALL["vit_depth"],
                                  enc_layers=SMALL["enc_layers"], fusion_layer=SMALL["fusion_layer"], dec_layers=SMALL["dec_layers"],
                                  image=SMALL["image"], vocab=SMALL["vocab"], train_lm_head=head, **kw)


def _batches(seed0, n):
    d = A.AlbefDims(**SMALL)
    return [A.synthetic_batch(3, d, seed0 + s, q_len=12, a_len=5, k=[2, 1, 3], ragged=True) for s in range(n)]


def _stored(g, key, t):
    """(engine values, stored values) of tensor `t` for fixture key `key`: whole, or on the stored strided samples."""
    if key in g:
        return t.flatten().float(), torch.from_numpy(g[key]).flatten()
    samp = torch.from_numpy(g["samp::" + key])
    idx = torch.linspace(0, t.numel() - 1, samp.numel()).long()
    return t.flatten().float()[idx], samp


def _grad_of(eng, n):
    grp = eng.lm if n in HEAD else eng.ad[0]
    return grp.view(n, grp.g).cpu()


def _check_adapters(g, pre, eng, P0, with_norm):
    sd = eng.state_dict()
    keys = [k.split("::", 1)[1] for k in g if k.startswith(pre + "dsamp::")]
    assert len(keys) == 28
    worst_max, worst_ratio = 0.0, 0.0
    for k in keys:
        dw = (sd[k].cpu() - P0[k]).flatten()
        ref = torch.from_numpy(g[pre + "dsamp::" + k])
        idx = torch.linspace(0, dw.numel() - 1, ref.numel()).long()
        err = (dw[idx] - ref).abs()
        move = float(g[pre + "dmean::" + k])
        assert float(err.max()) < 1e-3, (k, float(err.max()))
        assert float(err.mean()) <= 0.1 * move, (k, float(err.mean()), move)
        assert float(dw.abs().max()) > 0, k
        if with_norm:
            nerr = abs(float(dw.norm()) - float(g[pre + "dnorm::" + k])) / float(g[pre + "dnorm::" + k])
            assert nerr < 0.05, (k, nerr)
        worst_max, worst_ratio = max(worst_max, float(err.max())), max(worst_ratio, float(err.mean()) / move)
    return worst_max, worst_ratio


def _check_head(g, pre, eng, P0, step, tag):
    """pre: "head." (gb1) or "" (gb2); the fp32 run is the reference, the autocast run its own distance."""
    sd = eng.state_dict()
    bad = []
    for n in HEAD:
        key = f"after{step}.d::{n}"
        got, ref = _stored(g, pre + "fp32." + key, sd[n].cpu() - P0[n])
        _, ac = _stored(g, pre + "ac." + key, sd[n].cpu() - P0[n])
        err, err_ac = (got - ref).abs(), (ac - ref).abs()
        b_max, b_mean = max(1e-3, float(err_ac.max())), max(0.1 * float(ref.abs().mean()), float(err_ac.mean()))
        print(f"head update {tag} step {step} {n[len(CLS):]}: max {float(err.max()):.3e} (autocast {float(err_ac.max()):.3e}), "
              f"mean {float(err.mean()):.3e} (autocast {float(err_ac.mean()):.3e}, move {float(ref.abs().mean()):.3e})")
        # (the early snapshot is after step 2: the first optimizer step of a local update runs at the warm-up's learning rate 0)
        if not (float(err.max()) <= b_max and float(err.mean()) <= b_mean and float(got.abs().max()) > 0 and float(ref.abs().max()) > 0):
            bad.append((n, step, float(err.max()), b_max, float(err.mean()), b_mean))
    return bad


# ------------------------------------------------------------------------------------------------ 1. forward and first step
def test_forward_vs_reference(mod, gb1):
    P = _params()
    for operands in ("f16", "bf16"):
        eng = _engine(mod, P, False, operands=operands)
        loss, logits = eng.forward_train_logits(_dev(_batches(510, 1)[0]), "adapter")
        torch.cuda.synchronize()
        ref = torch.from_numpy(gb1["fwd.logits"])
        assert tuple(logits.shape) == tuple(ref.shape)
        assert float((logits.cpu() - ref).abs().max()) < 5e-2
        assert abs(float(loss) - float(gb1["head.fwd.loss"])) < 3e-3 * float(gb1["head.fwd.loss"])


# bf16 operands miss the factor-1.0 bound on a few adapter tensors (measured on an MI355X, worst engine / autocast error ratio: head
# trained 1.050 on text_encoder layer 2's adapter_down.bias, head frozen 1.325 on text_encoder layer 0's adapter_down.bias; the
# default fp16 build: 0.953 / 0.946, both on the first ViT block's adapter_down.bias).  The bound stays: strict xfail, as
# tests/test_round_b32_gpu.py does for bf16 operands.
_BF16 = pytest.mark.xfail(strict=True, reason="bf16 operands: worst gradient error 1.05x (head) / 1.33x (no head) the reference's autocast error")
GRAD_CASES = [("f16", True), ("f16", False), pytest.param("bf16", True, marks=_BF16), pytest.param("bf16", False, marks=_BF16)]


@pytest.mark.parametrize("operands,head", GRAD_CASES)
def test_first_step_gradients(mod, gb1, operands, head):
    """The gradient of every trainable tensor at the initial weights (the first train_step's, read from the groups' gradient
    buffers: unscaled), per tensor against gb1's fp32 gradient: no worse than the reference's own bf16-autocast gradient.
    Measured on an MI355X, worst engine / autocast error ratio over all trainable tensors: fp16 operands
    0.953 (head trained) / 0.946 (frozen); bf16 operands 1.050 / 1.325 -- those two parametrisations are strict xfails."""
    pre = "head." if head else "nohead."
    P = _params()
    eng = _engine(mod, P, head, operands=operands)
    eng.begin_local_update(steps_per_epoch=4)
    out = eng.train_step(_dev(_batches(510, 1)[0]))
    torch.cuda.synchronize()
    ref_loss = float(gb1[pre + "fwd.loss"])
    assert abs(float(out[0]) - ref_loss) < 3e-3 * ref_loss and float(out[2]) == float(out[0]) and float(out[1]) == 0.0
    names = gb1[pre + "names.trainable"].tolist()
    assert sorted(names) == sorted(n for _, grp in eng._named_groups() for n in grp.names)
    bad, worst = [], (0.0, "")
    for n in names:
        got, ref = _stored(gb1, pre + "g::" + n, _grad_of(eng, n))
        _, ref16 = _stored(gb1, pre + "g16::" + n, _grad_of(eng, n))
        e_eng, e_ac = float((got - ref).abs().max()), float((ref16 - ref).abs().max())
        assert e_ac > 0
        worst = max(worst, (e_eng / e_ac, n))
        if not e_eng <= e_ac:
            bad.append((n, e_eng, e_ac, e_eng / e_ac))
    print(f"first-step gradients {operands} head={head}: worst engine / autocast error ratio {worst[0]:.3f} ({worst[1]})")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 2. trajectories
@pytest.mark.parametrize("operands", ["f16", "bf16"])
@pytest.mark.parametrize("head", [True, False])
def test_four_steps_vs_reference(mod, gb1, operands, head):
    """gb1: 4 train_steps, eager then hipGraph replay (captured at step 3): losses, adapter updates, head updates after steps 2
    and 4, counters [4, 4] for every group."""
    pre = "head." if head else "nohead."
    P = _params()
    P0 = {k: v.clone() for k, v in P.items()}
    eng = _engine(mod, P, head, operands=operands)
    eng.begin_local_update(steps_per_epoch=4)
    bad = []
    for s, b in enumerate(_batches(510, 4)):
        out = eng.train_step(_dev(b), use_graph=(s >= 2))
        torch.cuda.synchronize()
        ref = float(gb1[pre + "fp32.losses"][s])
        assert abs(float(out[0]) - ref) < 3e-3 * ref, (s, float(out[0]), ref)
        if head and s + 1 in (2, 4):
            bad += _check_head(gb1, pre, eng, P0, s + 1, operands)
    assert not bad, bad
    wm, wr = _check_adapters(gb1, pre + "fp32.", eng, P0, False)
    print(f"adapter {operands} head={head}, 4 steps: worst max |ddW| {wm:.2e}, worst mean ratio {wr:.3f}")
    groups = eng._named_groups()
    assert [n for n, _ in groups] == (["adapter", "lm_head"] if head else ["adapter"])
    assert all(grp.state.tolist() == [4, 4] for _, grp in groups)
    if not head:
        assert eng.lm is None and not any(".cls." in k for k in eng.state_dict())
    assert eng.comm_flat().numel() == 7 * eng.ad_numel and eng.comm_flat().data_ptr() == eng.ad[0].p.data_ptr()
    eng.assert_finite()


@pytest.mark.parametrize("operands", ["f16", "bf16"])
def test_round_of_40_steps_vs_reference(mod, golden_dir, operands):
    """gb2: G11's 40-step protocol under hipGraph replay (the schedule runs past its warm-up), head trained."""
    g = load(golden_dir, "gb2_albef_adapter_round40.npz")
    steps = int(g["steps"])
    P = _params()
    P0 = {k: v.clone() for k, v in P.items()}
    eng = _engine(mod, P, True, operands=operands)
    eng.begin_local_update(steps_per_epoch=steps, num_epochs=1)
    worst_loss, bad = 0.0, []
    for s, b in enumerate(_batches(700, steps)):
        out = eng.train_step(_dev(b), use_graph=True)
        torch.cuda.synchronize()
        ref = float(g["fp32.losses"][s])
        worst_loss = max(worst_loss, abs(float(out[0]) - ref) / ref)
        if s + 1 in (2, steps):
            bad += _check_head(g, "", eng, P0, s + 1, operands)
    print(f"loss trajectory {operands}, {steps} steps: within {worst_loss:.2e}")
    assert worst_loss < 1e-2, worst_loss
    assert not bad, bad
    wm, wr = _check_adapters(g, "fp32.", eng, P0, True)
    print(f"adapter {operands}, {steps} steps: worst max |ddW| {wm:.2e}, worst mean ratio {wr:.3f}")
    assert eng.lm.state.tolist() == [steps, steps] == eng.ad[0].state.tolist()


# ------------------------------------------------------------------------------------------------ 3. graph replay, dropout = 0
@pytest.mark.parametrize("head", [True, False])
def test_graph_replay_is_bit_identical_to_eager_and_to_itself(mod, head):
    bs = [_dev(b) for b in _batches(510, 3)]
    outs = []
    for use_graph, kw in ((False, {}), (True, {}), (True, {}), (False, dict(dropout=0.0))):
        eng = _engine(mod, _params(), head, **kw)
        eng.begin_local_update(steps_per_epoch=3)
        losses = []
        for b in bs:
            losses.append(eng.train_step(b, use_graph=use_graph)[:3].clone())
        torch.cuda.synchronize()
        outs.append(({k: v.clone() for k, v in eng.state_dict().items()}, torch.stack(losses)))
        assert eng.side is None                      # one pass: no second stream was ever made
    assert any(".cls." in k for k in outs[0][0]) == head
    for sd, losses in outs[1:]:
        assert torch.equal(losses, outs[0][1])
        for k in outs[0][0]:
            assert torch.equal(sd[k], outs[0][0][k]), k


# ------------------------------------------------------------------------------------------------ 4. dynamic loss scale
@pytest.mark.parametrize("use_graph", [False, True])
def test_injected_overflow_skips_the_step(mod, use_graph):
    """The overflow flag forced before a step: nothing moves, no counter ticks, the scale backs off 16384 -> 8192, the flag is
    cleared -- and the next clean step moves adapter and head."""
    eng = _engine(mod, _params(), True, operands="f16")
    assert eng.scaler_state()["dynamic"]
    bs = [_dev(b) for b in _batches(510, 3)]
    eng.begin_local_update(steps_per_epoch=5)
    eng.train_step(bs[0], use_graph=use_graph)
    torch.cuda.synchronize()
    lm, ad = eng.lm, eng.ad[0]
    watched = (lm.p, lm.m, lm.v, lm.state, ad.p, ad.m, ad.v, ad.state)
    before = [t.clone() for t in watched]
    assert lm.state.tolist() == [1, 1] == ad.state.tolist() and eng.scaler_state()["scale"] == 16384.0
    eng.ovf_flags[0] = 1
    eng.train_step(bs[1], use_graph=use_graph)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, watched))
    st = eng.scaler_state()
    assert st["scale"] == 8192.0 and st["skipped_batches"] == 1 and eng.ovf_flags.tolist() == [0, 0]
    eng.train_step(bs[2], use_graph=use_graph)
    torch.cuda.synchronize()
    assert lm.state.tolist() == [2, 2] == ad.state.tolist()
    assert not torch.equal(before[0], lm.p) and not torch.equal(before[4], ad.p)
    eng.assert_finite()


# ------------------------------------------------------------------------------------------------ 5. evaluation, refusals
def test_rank_answer_after_training(mod, gb1):
    """rank_answer(mode="adapter") on the engine that trained gb1's four `head.` steps: the reference's trained model at G10's
    eval bounds; the slab path (this engine's frame is 6 answers for 3 x 4 candidates) and a short last batch of one question
    give the one-frame engine's rows; every other mode string is refused."""
    from feddat_amd import lib as L
    P = _params()
    bs = [_dev(b) for b in _batches(510, 4)]
    engines = {N: _engine(mod, {k: v.clone() for k, v in P.items()}, True, N=N) for N in (6, 12, 3)}
    for eng in engines.values():
        eng.begin_local_update(steps_per_epoch=4)
    for b in bs:
        engines[6].train_step(b)
    trained = {k: v.clone() for k, v in engines[6].state_dict().items()}
    for N in (12, 3):
        engines[N].load_tensors(trained)
    d = A.AlbefDims(**SMALL)
    b0 = A.synthetic_batch(3, d, 500, q_len=12, a_len=5, k=[2, 1, 3], ragged=True)
    ev = A.synthetic_batch(3, d, 501, q_len=12, a_len=5, k=[4, 4, 3], ragged=True)
    qb = _dev({kk: b0[kk] for kk in ("image", "question_ids", "question_mask")})
    ref_ids, ref_probs = gb1["eval.topk_ids"], torch.from_numpy(gb1["eval.topk_probs"])
    res = {N: eng.rank_answer(qb, ev["answer_ids"], ev["answer_mask"], 4, "adapter") for N, eng in engines.items()}
    torch.cuda.synchronize()
    for N, (ids, probs) in res.items():          # N = 12: one frame; 6: slabs; 3: the slab path at n_answers = B
        assert (probs.cpu().sort(1, descending=True).values - ref_probs).abs().max() < 2e-2, N
        assert np.array_equal(np.sort(ids.cpu().numpy(), 1), np.sort(ref_ids, 1)), N
        assert float((probs - res[12][1]).abs().max()) < 1e-5 and torch.equal(ids, res[12][0]), N
    # a short last batch: the first question alone gives its row
    q1 = {k: v[:1] for k, v in qb.items()}
    ids1, probs1 = engines[6].rank_answer(q1, ev["answer_ids"], ev["answer_mask"], 4, "adapter")
    assert torch.equal(ids1, res[6][0][:1]) and float((probs1 - res[6][1][:1]).abs().max()) < 1e-5
    for mode in ("gating", "adapter_0", "adapter_1", "both", ""):
        with pytest.raises(L.FeddatHipError):
            engines[6].rank_answer(qb, ev["answer_ids"], ev["answer_mask"], 4, mode)
        with pytest.raises(L.FeddatHipError):
            engines[6].forward_train_logits(bs[0], mode)
    with pytest.raises(L.FeddatHipError):
        engines[6].copy_global_to_teacher()
    with pytest.raises(L.FeddatHipError):
        _engine(mod, P, False, stack_text=True)


# ------------------------------------------------------------------------------------------------ 6. dropout
def test_engine_with_dropout_vs_the_reference_in_train_mode(mod, golden_dir):
    """gb3 = the reference's single-adapter modules under model.train() with p = 0.1, their nn.Dropout masks the shared counter-based
    ones (one forward per step: pass 0, step = forwards done): 3 train_steps, head trained.  The engine (eager for 2 steps, then a
    captured hipGraph whose masks come from the device-side step counter) at the bounds of
    tests/test_dropout_gpu.py::test_engine_with_dropout_vs_the_reference_in_train_mode: losses 3e-3, every adapter tensor
    |ddW|.max < 1e-3 and |ddW|.mean <= 0.1 |dW_ref|.mean."""
    g = load(golden_dir, "gb3_albef_adapter_dropout.npz")
    steps, p, seed = int(g["steps"]), float(g["p"]), int(g["seed"])
    P = _params()
    P0 = {k: v.clone() for k, v in P.items()}
    eng = _engine(mod, P, True, dropout=p, seed=seed)
    eng.begin_local_update(steps_per_epoch=steps, num_epochs=1)
    d = A.AlbefDims(**SMALL)
    for s in range(steps):
        b = A.synthetic_batch(3, d, 900 + s, q_len=12, a_len=5, k=[2, 1, 3], ragged=True)
        out = eng.train_step(_dev(b), use_graph=(s >= 2))
        torch.cuda.synchronize()
        ref = float(g["losses"][s])
        assert abs(float(out[0]) - ref) < 3e-3 * ref, (s, float(out[0]), ref)
    assert int(eng.drop_ctr[0]) == steps and eng.side is None
    wm, wr = _check_adapters(g, "", eng, P0, False)
    sd = eng.state_dict()
    for n in HEAD:
        got, ref = _stored(g, "d::" + n, sd[n].cpu() - P0[n])
        err = (got - ref).abs()
        assert float(err.max()) < 1e-3 and float(err.mean()) <= 0.1 * float(ref.abs().mean()) and float(got.abs().max()) > 0, n
    print(f"single adapter with dropout 0.1, 3 steps vs the reference: worst max |ddW| {wm:.2e}, mean ratio {wr:.3f}")


# ------------------------------------------------------------------------------------------------ 7. federation
def _args(**kw):
    import types
    return types.SimpleNamespace(**dict(dict(local_epochs=1, num_epochs=15, lr=1e-4, optimizer_mode="adapter", debug=0, hip_graph=True), **kw))


def _learner(P, **kw):
    from feddat_amd import albef_modeling
    return albef_modeling.create_albef_continual_learner_model(
        P, DEV, 3, 6, q_len=12, a_len=5, optimizer_mode="adapter", **dict({k: v for k, v in SMALL.items() if k != "max_pos"}, **kw))


def test_two_clients_two_rounds_vs_reference_federation(mod, golden_dir, tmp_path):
    """gb4's two clients (3 and 2 steps) over two rounds, driven by hand with the public calls train.main uses (which keeps refusing
    the combination on the command line): load_state_dict, AlbefTaskTrainer.train, lib.fedavg_accumulate on comm_flat()."""
    from feddat_amd import checkpoint, lib as L, train
    from feddat_amd.modes import mode_names
    g = load(golden_dir, "gb4_albef_adapter_2clients.npz")
    tasks, steps = ["art", "abstract"], [3, 2]
    P0 = _params()
    model = _learner({k: v.clone() for k, v in P0.items()}, train_lm_head=True)
    eng = model.engine
    assert isinstance(eng, mod.AlbefAdapterEngine) and model.optimizer_mode == "adapter" and model.optimizer_adapters() == (0,)
    names = mode_names(list(model.state_dict()), "adapter", albef=True)
    assert model.comm_state_dict_names == g["names.communicated"].tolist() == names["communicated"]
    assert sorted(names["trainable"]) == sorted(g["names.trainable"].tolist())
    keep = set(names["personal"])
    assert keep == {n for n in g["names.personal"].tolist() if "predictions.decoder." not in n} == set(HEAD)
    assert not keep & set(model.comm_state_dict_names)
    personal = {t: {n: v.clone() for n, v in model.state_dict().items() if n in keep} for t in tasks}
    d = A.AlbefDims(**SMALL)
    data = {t: [_dev(A.synthetic_batch(3, d, 800 + 100 * ti + s, q_len=12, a_len=5, k=[2, 1, 3], ragged=True)) for s in range(steps[ti])]
            for ti, t in enumerate(tasks)}
    server_flat = eng.comm_flat().clone()
    acc = torch.zeros_like(server_flat)
    args = _args()
    for rnd in range(2):
        for k, t in enumerate(tasks):
            eng.comm_flat().copy_(server_flat)
            eng.comm_written()
            model.load_state_dict(personal[t])
            train.AlbefTaskTrainer(args, t, data[t], []).train(model, rnd)
            personal[t] = {n: v.clone() for n, v in model.state_dict().items() if n in keep}
            L.fedavg_accumulate(acc, eng.comm_flat(), 1.0, float(len(tasks)), k == 0)
        server_flat.copy_(acc)
        eng.comm_flat().copy_(server_flat)
        eng.comm_written()
        wm, wr = _check_adapters(g, f"r{rnd}.server.", eng, P0, False)
        for t in tasks:          # the heads are personal: each client's own, never averaged
            for n in HEAD:
                got, ref = _stored(g, f"r{rnd}.{t}.d::{n}", personal[t][n].cpu() - P0[n])
                err = (got - ref).abs()
                assert float(err.max()) < 1e-3 and float(err.mean()) <= 0.1 * float(ref.abs().mean()), (rnd, t, n)
        assert all(not torch.equal(personal["art"][n], personal["abstract"][n]) for n in HEAD)
        print(f"gb4 round {rnd}: server worst max {wm:.2e} worst mean ratio {wr:.3f}")
    # eval: one score
    from feddat_amd import albef_spec
    ans_ids, ans_mask = albef_spec.synthetic_answer_list(11, a_len=5, vocab=SMALL["vocab"], seed=3)
    loader = albef_spec.synthetic_eval_loader(5, 3, 7, ans_ids, ans_mask, 4, image=SMALL["image"], q_len=12, vocab=SMALL["vocab"], device=DEV)
    score = train.AlbefTaskTrainer(args, "art", data["art"], loader).eval(model)
    assert isinstance(score, float) and 0.0 <= score <= 100.0
    # checkpoint round trip of the payload and the personal tensors, bit for bit
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
    model.load_state_dict(pers["abstract"])
    assert all(torch.equal(model.state_dict()[n], personal["abstract"][n]) for n in HEAD)


# ------------------------------------------------------------------------------------------------ 8. the learner
def test_learner_from_strings_and_an_image_list_equals_the_engine(mod, golden_dir):
    """ALBEFContinualLearner(optimizer_mode="adapter") on question / answer strings and a list of decoded images: what its engine
    gives on the tokenised batch; the dat-only switches are refused."""
    from feddat_amd import albef_spec, lib as L, train
    g9 = load(golden_dir, "g9_wordpiece.npz")
    vocab = str(g9["vocab"]).split("\n")
    texts = [t for t in str(g9["texts"]).split("\x1e") if t.isascii() and 0 < len(t) < 120]
    dims = dict(SMALL, vocab=max(SMALL["vocab"], len(vocab)))
    P = {k: A.O.seeded_value(k, s, 0.02, 0.02) for k, s in albef_spec.param_shapes(optimizer_mode="adapter", **dims).items()}
    from feddat_amd import albef_modeling
    model = albef_modeling.ALBEFContinualLearner(P, DEV, 3, 8, q_len=25, a_len=16, tokenizer_vocab=vocab, optimizer_mode="adapter",
                                                 **{k: v for k, v in dims.items() if k != "max_pos"})
    assert isinstance(model.engine, mod.AlbefAdapterEngine)
    assert all("adapter" in n for n in model.comm_state_dict_names) and len(model.comm_state_dict_names) == 28
    with pytest.raises(L.FeddatHipError):
        model.activate_gating()
    for name in ("adapter_0", "adapter_1", "gating"):
        with pytest.raises(L.FeddatHipError):
            model.set_active_adapter(name)
    model.set_active_adapter("adapter")
    assert model.optimizer_adapters() == (0,)
    gen = torch.Generator().manual_seed(4)
    raw = {"images": albef_spec.synthetic_raw_images(3, 11, image=dims["image"]), "questions": [texts[j] for j in range(3)],
           "answers": [" ".join(texts[7 + j].split()[:2]) or "yes" for j in range(6)], "weights": torch.rand(6, generator=gen) + 0.5,
           "n": [2, 1, 3], "alpha": 0.0}
    loss, logits = model("art", dict(raw, train=True))
    enc = model.process_inputs(dict(raw, train=True))
    enc = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in enc.items()}
    loss_e, logits_e = model.engine.forward_train_logits(enc, "adapter")
    torch.cuda.synchronize()
    assert torch.equal(loss, loss_e) and torch.equal(logits, logits_e) and bool(torch.isfinite(logits).all())
    # eval from strings: one ranking in mode "adapter"
    ev = {"images": raw["images"][:2], "questions": raw["questions"][:2], "answer_list": ["yes", "no", "two", "red", "a dog"], "k": 3,
          "train": False}
    ids, probs = model("art", ev)
    enc = model.process_inputs(ev)
    enc = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in enc.items()}
    ids_e, probs_e = model.engine.rank_answer(enc, enc["answer_list_ids"], enc["answer_list_mask"], 3, "adapter")
    assert tuple(ids.shape) == (2, 3) and torch.equal(ids, ids_e) and torch.equal(probs, probs_e)
    # one train_step through the trainer from the collated list: the gate is never touched
    tr = train.AlbefTaskTrainer(_args(), "art", [[raw["images"], raw["questions"], raw["answers"], raw["weights"], raw["n"], 0.0]], [])
    tr.train(model)
    assert model.engine.ad[0].state.tolist() == [1, 1] and model.gating is False
