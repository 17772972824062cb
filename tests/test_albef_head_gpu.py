"""AlbefDatEngine(train_lm_head=True): the decoder's LM head text_decoder.cls.predictions.* trained per client as the reference
trains it (main.py:247-250), against the reference's own runs with the head trainable (tests/golden/gh1_albef_head_small.npz,
gh2_albef_head_round40.npz; tools/make_albef_head_golden.py).  Every fixture run exists twice, in fp32 and with the forward
under torch.autocast("cpu", bfloat16): the autocast run is the reference's own coarser arithmetic and the yardstick for the head.

Bounds.  Losses and adapter records: the ones tests/test_albef_gpu.py uses for G10 / G11 (loss 3e-3 resp. 1e-2 relative; per
adapter tensor |ddW|.max < 1e-3, |ddW|.mean <= 0.1 |dW_ref|.mean, norm within 5 % at 40 steps).  Head gradients of the first step,
per tensor: max-abs error to the fp32 gradient over the tensor's max |g| at most that of the reference's autocast gradient (factor
1.0).  Head updates: the engine's distance to the fp32 run at most the larger of the adapter bound and the autocast run's own
distance (max: max(1e-3, autocast max); mean: max(0.1 mean |dW_ref|, autocast mean)).  transform.dense.weight is stored as 4096
strided samples: both sides of its comparisons are taken on those samples."""
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
# the step forms: the default two-stream form, the stacked text towers, and the separate form that dropout > 0 selects (three text
# forwards; the masks themselves switched off, so the reference's dropout-free run is what it must reproduce)
FORMS = ("default", "stacked", "separate")


def _dev(b):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in b.items()}


@pytest.fixture(scope="module")
def eng_mod():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import albef_engine
    return albef_engine


def _engine(eng_mod, P, form="default", B=3, N=6, **kw):
    if form == "stacked":
        kw["stack_text"] = True
    if form == "separate":
        kw["dropout"] = 0.1
    eng = eng_mod.AlbefDatEngine(P, DEV, batch=B, n_answers=N, q_len=12, a_len=5, vit_depth=SMALL["vit_depth"],
                                 enc_layers=SMALL["enc_layers"], fusion_layer=SMALL["fusion_layer"],
                                 dec_layers=SMALL["dec_layers"], image=SMALL["image"], vocab=SMALL["vocab"], train_lm_head=True, **kw)
    if form == "separate":
        eng._drop = lambda *a, **k: None        # every site without a mask; the schedule stays the three-forward one
        assert eng.dropout > 0 and not eng.batch_text
    if form == "stacked":
        assert eng.batch_text
    return eng


def _stored(g, key, t):
    """(engine values, stored values) of tensor `t` for fixture key `key`: whole, or on the stored strided samples."""
    if key in g:
        return t.flatten().float(), torch.from_numpy(g[key]).flatten()
    samp = torch.from_numpy(g["samp::" + key])
    idx = torch.linspace(0, t.numel() - 1, samp.numel()).long()
    return t.flatten().float()[idx], samp


def _batches(d, seed0, n):
    return [A.synthetic_batch(3, d, seed0 + s, q_len=12, a_len=5, k=[2, 1, 3], ragged=True) for s in range(n)]


# ------------------------------------------------------------------------------------------------ 1. the refresh kernel
@pytest.mark.parametrize("operands", ["bf16", "f16"])
@pytest.mark.parametrize("V", [3072, 30522])
def test_lm_head_refresh_kernel(eng_mod, operands, V):
    """feddat_lm_head_refresh on a 768 x 768 group: the 16-bit W and W^T bit-equal to cvt_f32_bf16 / transpose_f32_bf16 and to
    a float64 -> operand-format rounding in torch; the bias copied exactly and zero-padded to Vp (V = 30 522: not a multiple
    of 8, Vp = 30 592; the bias at an offset of the flat buffer that is not 16-byte aligned)."""
    from feddat_amd import lib as L
    H, Vp = 768, (V + 127) // 128 * 128
    gen = torch.Generator().manual_seed(V)
    flat = torch.randn(H * H + 4 + 1 + V, generator=gen).to(DEV)
    w, bias = flat[:H * H].view(H, H), flat[H * H + 5:H * H + 5 + V]
    assert bias.data_ptr() % 16 != 0
    with L.operands(operands):
        dt = L.OPERAND_DTYPE[operands]
        w16, wT16 = torch.zeros(H, H, dtype=dt, device=DEV), torch.zeros(H, H, dtype=dt, device=DEV)
        bpad = torch.full((Vp,), 7.0, device=DEV)
        L.lm_head_refresh(w, bias, w16, wT16, bpad)
        c16, cT16 = torch.empty_like(w16), torch.empty_like(wT16)
        L.cvt_f32_bf16(w.contiguous(), c16)
        L.transpose_f32_bf16(w.contiguous(), cT16, H, H)
    torch.cuda.synchronize()
    assert torch.equal(w16, c16) and torch.equal(wT16, cT16)
    assert torch.equal(w16, w.double().to(dt)) and torch.equal(wT16, w.double().t().contiguous().to(dt))
    assert torch.equal(bpad[:V], bias) and float(bpad[V:].abs().max() if Vp > V else 0.0) == 0.0


# ------------------------------------------------------------------------------------------------ 2. first-step gradients
@pytest.mark.parametrize("operands", ["bf16", "f16"])
@pytest.mark.parametrize("form", FORMS)
def test_first_step_head_gradients(eng_mod, golden_dir, operands, form):
    """The head's gradient of L_1 at the initial weights (sub-step A of the first train_step), per tensor against gh1's fp32
    gradient: no worse than the reference's own bf16-autocast gradient (factor 1.0).
    Measured on an MI355X, engine error / autocast error, the same in the three step forms --
      fp16 operands (the default): bias 0.135, dense.weight 0.889, dense.bias 0.772, LayerNorm.weight 0.618, LayerNorm.bias 0.706
      bf16 operands:               bias 0.496, dense.weight 0.967, dense.bias 0.883, LayerNorm.weight 0.800, LayerNorm.bias 0.784
    (errors: autocast 7.30e-4 / 3.58e-3 / 5.29e-3 / 6.17e-3 / 3.41e-3; bf16 engine 3.62e-4 / 3.46e-3 / 4.67e-3 / 4.93e-3 / 2.67e-3).
    About 3e-3 of every transform tensor's error arrives with the decoder rows and the teacher logits and is the same in both
    builds (an exact float64 head on the engine's own decoder rows: 3.4e-3 / 4.2e-3 / 5.2e-3 / 2.4e-3); the head's own share is
    what its fp32 transform forward and the two-product dlogits W_emb keep small."""
    g = load(golden_dir, "gh1_albef_head_small.npz")
    d = A.AlbefDims(**SMALL)
    P = A.make_params(d)
    eng = _engine(eng_mod, P, form, operands=operands)
    eng.grad_a_probe = torch.zeros_like(eng.lm.g)
    eng.begin_local_update(steps_per_epoch=4)
    eng.train_step(_dev(_batches(d, 510, 1)[0]))
    torch.cuda.synchronize()
    L1 = float(eng.acts["adapter_1"]["loss"][2])
    assert abs(L1 - float(g["L_1"])) < 3e-3 * float(g["L_1"]), (L1, float(g["L_1"]))
    bad = []
    for n in HEAD:
        got, ref = _stored(g, "g::" + n, eng.lm.view(n, eng.grad_a_probe).cpu())
        _, ref16 = _stored(g, "g16::" + n, eng.lm.view(n, eng.grad_a_probe).cpu())
        scale = float(ref.abs().max())
        e_eng, e_ac = float((got - ref).abs().max()) / scale, float((ref16 - ref).abs().max()) / scale
        print(f"head gradient {form} {operands} {n[len(CLS):]}: engine {e_eng:.3e}, autocast {e_ac:.3e}, ratio {e_eng / e_ac:.3f}")
        if not e_eng <= e_ac:
            bad.append((n, e_eng, e_ac))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 3. trajectories
def _check_head(g, pre, eng, P0, step, tag):
    sd = eng.state_dict()
    bad = []
    for n in HEAD:
        key = f"after{step}.d::{n}"
        got, ref = _stored(g, pre + key, sd[n].cpu() - P0[n])
        _, ac = _stored(g, "ac." + key, sd[n].cpu() - P0[n])
        err, err_ac = (got - ref).abs(), (ac - ref).abs()
        b_max, b_mean = max(1e-3, float(err_ac.max())), max(0.1 * float(ref.abs().mean()), float(err_ac.mean()))
        print(f"head update {tag} step {step} {n[len(CLS):]}: max {float(err.max()):.3e} (autocast {float(err_ac.max()):.3e}), "
              f"mean {float(err.mean()):.3e} (autocast {float(err_ac.mean()):.3e}, move {float(ref.abs().mean()):.3e})")
        if not (float(err.max()) <= b_max and float(err.mean()) <= b_mean and float(got.abs().max()) > 0):
            bad.append((n, step, float(err.max()), b_max, float(err.mean()), b_mean))
    return bad


def _check_adapters(g, pre, eng, P0, with_norm):
    sd = eng.state_dict()
    keys = [k.split("::", 1)[1] for k in g if k.startswith(pre + "dsamp::")]
    assert keys
    worst_max, worst_ratio = 0.0, 0.0
    for k in keys:
        dw = (sd[k].cpu() - P0[k]).flatten()
        idx = torch.linspace(0, dw.numel() - 1, min(512, dw.numel())).long()
        err = (dw[idx] - torch.from_numpy(g[pre + "dsamp::" + k])).abs()
        move = float(g[pre + "dmean::" + k])
        assert float(err.max()) < 1e-3, (k, float(err.max()))
        assert float(err.mean()) <= 0.1 * move, (k, float(err.mean()), move)
        if with_norm:
            nerr = abs(float(dw.norm()) - float(g[pre + "dnorm::" + k])) / float(g[pre + "dnorm::" + k])
            assert nerr < 0.05, (k, nerr)
        worst_max, worst_ratio = max(worst_max, float(err.max())), max(worst_ratio, float(err.mean()) / move)
    return worst_max, worst_ratio


@pytest.mark.parametrize("operands", ["bf16", "f16"])
@pytest.mark.parametrize("form", FORMS)
def test_four_steps_vs_reference(eng_mod, golden_dir, operands, form):
    """gh1: 4 train_steps (eager, then hipGraph replay) with the head trainable: losses, head updates after steps 1 and 4,
    adapter records, the Adam step counters (head 2 x steps, adapters steps)."""
    g = load(golden_dir, "gh1_albef_head_small.npz")
    d = A.AlbefDims(**SMALL)
    P = A.make_params(d)
    P0 = {k: v.clone() for k, v in P.items()}
    eng = _engine(eng_mod, P, form, operands=operands)
    eng.begin_local_update(steps_per_epoch=4)
    bad = []
    for s, b in enumerate(_batches(d, 510, 4)):
        out = eng.train_step(_dev(b), use_graph=(s >= 2))
        torch.cuda.synchronize()
        ref = float(g["fp32.losses"][s])
        print(f"loss {form} {operands} step {s + 1}: {float(out[0]):.4f} (reference {ref:.4f})")
        assert abs(float(out[0]) - ref) < 3e-3 * ref, (s, float(out[0]), ref)
        if s + 1 in (1, 4):
            bad += _check_head(g, "fp32.", eng, P0, s + 1, f"{form} {operands}")
    assert not bad, bad
    wm, wr = _check_adapters(g, "fp32.", eng, P0, False)
    print(f"adapters {form} {operands}, 4 steps: worst max |ddW| {wm:.2e}, worst mean ratio {wr:.3f}")
    assert eng.lm.state.tolist() == [8, 8] and eng.ad[1].state.tolist() == [8, 4] and eng.ad[0].state.tolist() == [9, 4]
    eng.assert_finite()


@pytest.mark.parametrize("form,operands", [("default", "f16"), ("default", "bf16"), ("stacked", "f16"), ("separate", "f16")])
def test_round_of_40_steps_vs_reference(eng_mod, golden_dir, form, operands):
    """gh2: G11's 40-step protocol (hipGraph replay, schedule past its warm-up) with the head trainable."""
    g = load(golden_dir, "gh2_albef_head_round40.npz")
    steps = int(g["steps"])
    d = A.AlbefDims(**SMALL)
    P = A.make_params(d)
    P0 = {k: v.clone() for k, v in P.items()}
    eng = _engine(eng_mod, P, form, operands=operands)
    eng.begin_local_update(steps_per_epoch=steps, num_epochs=1)
    worst_loss, bad = 0.0, []
    for s, b in enumerate(_batches(d, 700, steps)):
        out = eng.train_step(_dev(b), use_graph=True)
        torch.cuda.synchronize()
        ref = float(g["fp32.losses"][s])
        worst_loss = max(worst_loss, abs(float(out[0]) - ref) / ref)
        if s + 1 in (1, steps):
            bad += _check_head(g, "fp32.", eng, P0, s + 1, f"{form} {operands}")
    print(f"loss trajectory {form} {operands}, {steps} steps: within {worst_loss:.2e}")
    assert worst_loss < 1e-2, worst_loss
    assert not bad, bad
    wm, wr = _check_adapters(g, "fp32.", eng, P0, True)
    print(f"adapters {form} {operands}, {steps} steps: worst max |ddW| {wm:.2e}, worst mean ratio {wr:.3f}")
    assert eng.lm.state.tolist() == [2 * steps, 2 * steps] and eng.ad[1].state.tolist() == [2 * steps, steps]


# ------------------------------------------------------------------------------------------------ 4. evaluation
def test_rank_answer_after_training(eng_mod, golden_dir):
    """rank_answer on the engine that trained (4 steps of gh1, head included) reads the trained head: top-k ids and
    probabilities of the reference's trained model, at G10's eval tolerance."""
    g = load(golden_dir, "gh1_albef_head_small.npz")
    d = A.AlbefDims(**SMALL)
    P = A.make_params(d)
    eng = _engine(eng_mod, P)
    eng.begin_local_update(steps_per_epoch=4)
    for b in _batches(d, 510, 4):
        eng.train_step(_dev(b))
    b0 = A.synthetic_batch(3, d, 500, q_len=12, a_len=5, k=[2, 1, 3], ragged=True)
    ev = A.synthetic_batch(3, d, 501, q_len=12, a_len=5, k=[4, 4, 3], ragged=True)
    qb = {kk: b0[kk] for kk in ("image", "question_ids", "question_mask")}
    ids, probs = eng.rank_answer(_dev(qb), ev["answer_ids"], ev["answer_mask"], 4)
    ref_ids, ref_probs = g["eval.topk_ids"], torch.from_numpy(g["eval.topk_probs"])
    gaps = (ref_probs[:, :-1] - ref_probs[:, 1:]).min()
    assert (probs.cpu().sort(1, descending=True).values - ref_probs).abs().max() < 2e-2
    if float(gaps) > 4e-2:
        assert np.array_equal(ids.cpu().numpy(), ref_ids)
    else:
        assert np.array_equal(np.sort(ids.cpu().numpy(), 1), np.sort(ref_ids, 1))


# ------------------------------------------------------------------------------------------------ 5. dynamic loss scale
@pytest.mark.parametrize("use_graph", [False, True])
def test_overflow_in_substep_a_restores_the_head(eng_mod, use_graph):
    """The overflow flag of sub-step A forced before a step (tests/test_dynscale_gpu.py's injection): the batch is void -- the
    head's p | m | v are bit-equal to their state before the step although sub-step A had no way to know of the overflow that
    adapter_1's backward reports later, no counter ticks, the scale backs off -- and the next clean step proceeds."""
    d = A.AlbefDims(**SMALL)
    eng = _engine(eng_mod, A.make_params(d), operands="f16")
    assert eng.scaler_state()["dynamic"]
    bs = [_dev(b) for b in _batches(d, 510, 3)]
    eng.begin_local_update(steps_per_epoch=5)
    eng.train_step(bs[0], use_graph=use_graph)
    torch.cuda.synchronize()
    lm = eng.lm
    before = [t.clone() for t in (lm.p, lm.m, lm.v, lm.state, eng.ad[0].p, eng.ad[1].p, eng.ad[0].state, eng.ad[1].state)]
    assert lm.state.tolist() == [2, 2] and eng.scaler_state()["scale"] == 16384.0
    eng.ovf_flags[1] = 1
    eng.train_step(bs[1], use_graph=use_graph)
    torch.cuda.synchronize()
    after = (lm.p, lm.m, lm.v, lm.state, eng.ad[0].p, eng.ad[1].p, eng.ad[0].state, eng.ad[1].state)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    st = eng.scaler_state()
    assert st["scale"] == 8192.0 and st["skipped_batches"] == 1 and eng.ovf_flags.tolist() == [0, 0]
    # the operand copies are those of the restored head
    w16 = torch.empty_like(eng.head["t"]["w"])
    from feddat_amd import lib as L
    with L.operands("f16"):
        L.cvt_f32_bf16(lm.view(HEAD[1]).contiguous(), w16)
    assert torch.equal(w16, eng.head["t"]["w"])
    eng.train_step(bs[2], use_graph=use_graph)
    torch.cuda.synchronize()
    assert lm.state.tolist() == [4, 4] and not torch.equal(before[0], lm.p) and not torch.equal(before[5], eng.ad[1].p)
    eng.assert_finite()


# ------------------------------------------------------------------------------------------------ 6. graph vs eager
@pytest.mark.parametrize("form", FORMS)
def test_captured_graph_equals_eager(eng_mod, form):
    d = A.AlbefDims(**SMALL)
    bs = [_dev(b) for b in _batches(d, 510, 3)]
    outs = []
    for use_graph in (False, True):
        eng = _engine(eng_mod, A.make_params(d), form)
        eng.begin_local_update(steps_per_epoch=3)
        for b in bs:
            eng.train_step(b, use_graph=use_graph)
        torch.cuda.synchronize()
        outs.append({k: v.clone() for k, v in eng.state_dict().items()})
    assert any(".cls." in k for k in outs[0])
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


# ------------------------------------------------------------------------------------------------ 7. train.main
def test_train_main_keeps_the_head_personal(tmp_path):
    """feddat_amd.train.main --albef_train_lm_head, 2 clients x 2 rounds (the second round's optimizers no longer hold
    adapter_0 -- the server flags after round 0's evaluation slot -- and still step the head): each client's .cls. tensors ride
    in its personal parameters, differ between the clients and moved; the FedAvg payload is what it is without the option; one
    round + --checkpoint resume equals two rounds bit for bit."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import albef_spec, train
    dims = dict(vit_depth=2, enc_layers=3, fusion_layer=1, dec_layers=2, vocab=3072, max_pos=64)
    common = ["--encoder_name", "albef_no_distill", "--ordered_cl_tasks", "art,gqa", "--image_size", "64", "--batch_size", "2",
              "--synthetic_steps", "2", "--albef_dims", ",".join(f"{k}={v}" for k, v in dims.items()), "--save_every", "1"]
    two = train.main(common + ["--albef_train_lm_head", "--comm_rounds", "2", "--output_dir", str(tmp_path / "two")])
    init = albef_spec.random_init(seed=42, image=64, **dims)
    pers = two.personal_params
    for t in ("art", "gqa"):
        assert sorted(k for k in pers[t] if ".cls." in k) == sorted(HEAD)
        assert not any("decoder.weight" in k or "decoder.bias" in k for k in pers[t])
        for n in HEAD:
            assert float((pers[t][n].cpu() - init[n]).abs().max()) > 0, (t, n)
    for n in HEAD:
        assert not torch.equal(pers["art"][n], pers["gqa"][n]), n
    assert not any(".cls." in n for n in two.comm_state_dict_names)
    off = train.main(common + ["--comm_rounds", "1", "--output_dir", str(tmp_path / "off")])
    assert two.engine.comm_flat().numel() == off.engine.comm_flat().numel() == 7 * two.engine.ad_numel
    assert not any(".cls." in k for k in off.state_dict()) and not any(".cls." in k for k in off.personal_params["art"])
    train.main(common + ["--albef_train_lm_head", "--comm_rounds", "1", "--output_dir", str(tmp_path / "one")])
    res = train.main(common + ["--albef_train_lm_head", "--comm_rounds", "2", "--output_dir", str(tmp_path / "one"),
                               "--checkpoint", str(tmp_path / "one")])
    assert torch.equal(res.engine.comm_flat(), two.engine.comm_flat())
    for t in ("art", "gqa"):
        assert sorted(res.personal_params[t]) == sorted(pers[t])
        for k, v in pers[t].items():
            assert torch.equal(res.personal_params[t][k], v), (t, k)


# ------------------------------------------------------------------------------------------------ 8. option off
def test_option_off_is_the_engine_without_the_argument(eng_mod):
    """train_lm_head=False: no .cls. key in state_dict(), no head group, and the trained state after 3 steps bit-equal to an
    engine built without the argument (the parent's constructor call)."""
    d = A.AlbefDims(**SMALL)
    bs = [_dev(b) for b in _batches(d, 510, 3)]
    outs = []
    for kw in ({}, {"train_lm_head": False}):
        eng = eng_mod.AlbefDatEngine(A.make_params(d), DEV, batch=3, n_answers=6, q_len=12, a_len=5, vit_depth=SMALL["vit_depth"],
                                     enc_layers=SMALL["enc_layers"], fusion_layer=SMALL["fusion_layer"],
                                     dec_layers=SMALL["dec_layers"], image=SMALL["image"], vocab=SMALL["vocab"], **kw)
        assert eng.lm is None and [n for n, _ in eng._named_groups()] == ["adapter_0", "adapter_1"]
        eng.begin_local_update(steps_per_epoch=3)
        for b in bs:
            eng.train_step(b, use_graph=True)
        torch.cuda.synchronize()
        outs.append({k: v.clone() for k, v in eng.state_dict().items()})
    assert not any(".cls." in k for k in outs[0]) and sorted(outs[0]) == sorted(outs[1])
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
