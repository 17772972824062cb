"""Patch slots through the 2-layer ViLT engines (ViltBackbone max_patches): the image half of the sequence holds each sample's
valid patches compacted into max_patches slots instead of one position per cell of the pixel frame.

References: the reference's own numbers on a mixed portrait / landscape / square batch (tests/golden/gm1_mixed_frame.npz,
tools/make_mixed_frame_golden.py: it ran these batches at 125 positions), its padded-image fixture g6_padded.npz in a larger
frame, and the same mode's grid-frame engine (the code path every other test covers) on the same batch.

Tolerances are the grid frame's own: pooled / logits 3e-2, losses 2e-3 |ref| + 2e-3, updates by
tests/test_engine_gpu.py::_golden_update_parity (every element < 1e-3, mean error <= REL_MEAN of the mean update; key.bias excused
from the mean rule by name as in tests/test_vector_mode_gpu.py), gradients within 2 x the fixture's own bf16-autocast cost."""
import hashlib
import re

import pytest
import torch

from feddat_amd import vilt_spec
from oracle import feddat_oracle as O
from tests.golden_util import assert_update_parity, golden_tensor, load, sampled_update_parity
from tests.test_adapter_mode_gpu import adapter_params
from tests.test_engine_gpu import G6_TEXT, G6_VALID, REL_MEAN, _golden_update_parity
from tests.test_vector_mode_gpu import KEY_RATIO_MULT, _is_key_bias, plain_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
GM1_VALID = [(384, 224), (224, 384), (288, 288), (160, 320)]
GM1_TEXT = [40, 31, 40, 12]
# a 224 x 224 frame (49 cells) with 35 slots: 35, 28, 18 and 35 valid patches
SMALL_VALID = [(160, 224), (224, 128), (96, 192), (224, 160)]
SMALL_TEXT = [40, 31, 40, 12]
# trained state after `python -m feddat_amd.train` with MAIN_COMMON and no mixed-frame flag, at the parent commit
PARENT_MAIN_HASH = "65c14ee6fc4c91de"
MAIN_COMMON = ["--num_layers", "2", "--batch_size", "4", "--comm_rounds", "1", "--ordered_cl_tasks", "art,abstract",
               "--synthetic_steps", "2"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _dev(b):
    return {k: v.to(DEV) for k, v in b.items()}


def _first(b, n):
    return {k: v[:n].clone() for k, v in b.items()}


def _gm1_batches(g):
    return [O.pad_batch(O.synthetic_batch(4, 384, int(g["seed0"]) + s), GM1_VALID, GM1_TEXT) for s in range(2)]


def _engine(mode, P, tasks, B, res, **kw):
    if mode == "dat":
        from feddat_amd.engine import ViltDatEngine
        return ViltDatEngine(P, tasks, DEV, batch=B, res=res, layers=2, **kw)
    if mode == "adapter":
        from feddat_amd.adapter_engine import ViltAdapterEngine
        return ViltAdapterEngine(P, tasks, DEV, batch=B, res=res, layers=2, **kw)
    from feddat_amd.vector_engine import ViltVectorEngine
    return ViltVectorEngine(P, tasks, DEV, batch=B, res=res, layers=2, mode=mode, **kw)


def _params(mode, tasks):
    if mode == "dat":
        return O.make_params(O.ViltDims(layers=2), tasks, bias_std=0.02)
    return adapter_params(2, tasks) if mode == "adapter" else plain_params(2, tasks)


def _step_state(eng):
    return [t for _, g in eng._named_groups() for t in (g.p, g.m, g.v, g.state)] + \
        [eng.scaler_f, eng.scaler_i, eng.ovf_flags] + eng._extra_step_state()


def _trained(eng):
    torch.cuda.synchronize()
    return {f"{name}.{f}": getattr(g, f).clone() for name, g in eng._named_groups() for f in ("p", "m", "v")}


# ------------------------------------------------------------------------------------------------------- gm1: dat
@pytest.mark.parametrize("use_graph", [False, True])
def test_gm1_dat_engine_in_a_slot_frame(golden_dir, use_graph):
    """The reference's mixed batch (84, 84, 81, 50 valid patches) in a 384 x 384 frame with 84 slots: S = 125 like the
    reference's, eager and through a hipGraph captured on a batch WITHOUT padding (every sample over the budget there: capturing
    leaves neither the trained state nor the budget flag behind)."""
    g = load(golden_dir, "gm1_mixed_frame.npz")
    batches = _gm1_batches(g)
    P = _params("dat", ["art"])
    P0 = {k: v.clone() for k, v in P.items()}
    eng = _engine("dat", P, ["art"], 4, 384, max_patches=84)
    assert eng.S == 125 == int(g["encoder_seq"]) and eng.np == 84 and eng.patches.shape == (4 * 84, 3072)
    assert eng.key_mask2.shape == (2 * 4, 125) and eng.h0.shape == (4 * 125, 768)
    for mode in ("gating", "adapter_1"):
        pooled, logits = eng.forward(_dev(batches[0]), mode, "art")
        dp = float((pooled.cpu() - torch.from_numpy(g[f"dat.fwd.{mode}.pooled"])).abs().max())
        dl = float((logits.cpu() - torch.from_numpy(g[f"dat.fwd.{mode}.logits"])).abs().max())
        print(f"gm1 dat {mode}: |pooled| {dp:.2e} |logits| {dl:.2e}")
        assert dp < 3e-2 and dl < 3e-2
    # the key mask of the staged batch: text by attention_mask, CLS, then exactly `count` valid slots per sample
    km = eng.key_mask2.cpu()
    for b, (n_text, n_patch) in enumerate(zip(GM1_TEXT, g["counts"].tolist())):
        want = [1] * n_text + [0] * (40 - n_text) + [1] + [1] * n_patch + [0] * (84 - n_patch)
        assert km[b].tolist() == want == km[b + 4].tolist(), b
    eng.begin_local_update("art", steps_per_epoch=2)
    if use_graph:
        eng.set_batch(_dev(O.synthetic_batch(4, 384, 1)))
        eng._capture()
        assert int(eng.slot_overflow.item()) == 0
    for s, b in enumerate(batches):
        out = eng.train_step(_dev(b), use_graph=use_graph)
        ref = float(g["dat.losses"][s])
        print(f"gm1 dat graph {use_graph} step {s + 1}: loss {float(out[0]):.5f} reference {ref:.5f}")
        assert abs(float(out[0]) - ref) < 2e-3 * ref + 2e-3, (use_graph, s, float(out[0]), ref)
    w = _golden_update_parity(g, "dat.after2.", eng.state_dict(), P0)
    print(f"gm1 dat graph {use_graph}: worst (max |ddW|, mean ratio) vs the reference {w}")
    eng.assert_finite()


# ------------------------------------------------------------------------------------------------------- gm1: bias
@pytest.mark.parametrize("operands", ["bf16", "f16"])
def test_gm1_bias_gradients_in_a_slot_frame(golden_dir, operands):
    """tests/test_vector_mode_gpu.py::test_gradient_of_every_trainable_tensor's rule on the mixed batch: per tensor within
    2 x e16 = 2 max|g16 - g| / max|g| of the fixture; key.bias by its ratio to query.bias."""
    g = load(golden_dir, "gm1_mixed_frame.npz")
    pre = "bias."
    eng = _engine("bias", plain_params(2, ["art"]), ["art"], 4, 384, max_patches=84, operands=operands, dynamic_loss_scale=False)
    batch = _gm1_batches(g)[0]
    pooled, logits = eng.forward(_dev(batch), "art")
    dp = float((pooled.cpu() - torch.from_numpy(g[pre + "fwd.pooled"])).abs().max())
    dl = float((logits.cpu() - torch.from_numpy(g[pre + "fwd.logits"])).abs().max())
    eng.begin_local_update("art", steps_per_epoch=4)
    loss = float(eng.train_step(_dev(batch), use_graph=False)[0])
    ref_loss = float(g[pre + "loss"])
    print(f"gm1 bias {operands}: |pooled| {dp:.2e} |logits| {dl:.2e} loss {loss:.5f} (ref {ref_loss:.5f})")
    assert dp < 3e-2 and dl < 3e-2
    assert abs(loss - ref_loss) < 2e-3 * abs(ref_loss) + 2e-3
    torch.cuda.synchronize()
    grads = {n: eng.vec.view(n, eng.vec.g).cpu() for n in eng.vec.names}
    hp = eng.head["art"]
    grads.update({n: hp.view(n, hp.g).cpu() for n in hp.names})
    names = [k[len(pre) + 3:] for k in g if k.startswith(pre + "g::") and "task_layer." not in k]
    assert sorted(names) == sorted(n for n in grads if not n.startswith("task_layer."))
    worst, fails = {}, []
    for n in names:
        ref, ref16, got = torch.from_numpy(g[pre + "g::" + n]), torch.from_numpy(g[pre + "g16::" + n]), grads[n]
        gmax = float(ref.abs().max())
        e16, err = float((ref16 - ref).abs().max()) / gmax, float((got - ref).abs().max()) / gmax
        kind = re.sub(r"layer\.\d+\.", "layer.*.", n)
        w = worst.setdefault(kind, [0.0, 0.0])
        w[0], w[1] = max(w[0], e16), max(w[1], err)
        if _is_key_bias(n):
            q = n.replace("key.bias", "query.bias")
            r16 = float(ref16.abs().max()) / float(torch.from_numpy(g[pre + "g16::" + q]).abs().max())
            ours = float(got.abs().max()) / float(grads[q].abs().max())
            print(f"   {n}: max|g key| / max|g query|  bf16-autocast ref {r16:.2e}  ours {ours:.2e}")
            if not ours < KEY_RATIO_MULT * r16:
                fails.append((n, "key / query ratio", ours, "reference bf16", r16))
            continue
        if not err <= 2 * e16:
            fails.append((n, "err / max|g|", err, "e16", e16))
    for n in hp.names:
        flat = grads[n].flatten()
        if pre + "g::" + n in g:
            ref, ref16 = torch.from_numpy(g[pre + "g::" + n]).flatten(), torch.from_numpy(g[pre + "g16::" + n]).flatten()
        else:
            idx = torch.linspace(0, flat.numel() - 1, 2048).long()
            flat, ref, ref16 = flat[idx], torch.from_numpy(g["samp::" + pre + "g::" + n]), torch.from_numpy(g["samp::" + pre + "g16::" + n])
        gmax = float(ref.abs().max())
        e16, err = float((ref16 - ref).abs().max()) / gmax, float((flat - ref).abs().max()) / gmax
        worst[n] = [e16, err]
        if not err <= 2 * e16:
            fails.append((n, "err / max|g|", err, "e16", e16))
    for kind, (e16, err) in worst.items():
        print(f"   {kind}: e16 {e16:.3e}  ours {err:.3e}  bound {2 * e16:.3e}")
    assert not fails, fails


def test_gm1_bias_four_steps_in_a_slot_frame(golden_dir):
    g = load(golden_dir, "gm1_mixed_frame.npz")
    pre = "bias."
    P = plain_params(2, ["art"])
    P0 = {k: v.clone() for k, v in P.items()}
    eng = _engine("bias", P, ["art"], 4, 384, max_patches=84)
    b = _gm1_batches(g)
    eng.begin_local_update("art", steps_per_epoch=4)
    for s, batch in enumerate([b[0], b[1], b[0], b[1]]):
        out = eng.train_step(_dev(batch), use_graph=True)
        ref = float(g[pre + "losses"][s])
        print(f"gm1 bias step {s + 1}: loss {float(out[0]):.5f} reference {ref:.5f}")
        assert abs(float(out[0]) - ref) < 2e-3 * abs(ref) + 2e-3, (s, float(out[0]), ref)
        if s + 1 in (1, 4):
            sd = eng.state_dict()
            p = pre + f"after{s + 1}."
            vecs = [k[len(p) + 3:] for k in g if k.startswith(p + "d::")]
            assert sorted(vecs) == sorted(eng.vec.names)
            ref_sd = {k: P0[k] + torch.from_numpy(g[p + "d::" + k]) for k in vecs}
            w = assert_update_parity([k for k in vecs if not _is_key_bias(k)], sd, ref_sd, P0, 1e-3, REL_MEAN, p)
            for k in vecs:
                if _is_key_bias(k):
                    assert float((sd[k].cpu() - ref_sd[k]).abs().max()) < 1e-3, k
            whole = [k[len(p):] for k in g if k.startswith(p) and "::" not in k]
            w2 = assert_update_parity(whole, sd, {k: golden_tensor(g, p + k).reshape(P0[k].shape) for k in whole}, P0, 1e-3,
                                      REL_MEAN, p)
            w3 = sampled_update_parity(g, p, sd, P0, 2048, 1e-3, REL_MEAN)
            assert len(whole) >= 4
            print(f"gm1 bias after {s + 1}: worst max {max(w[0], w2[0], w3[0]):.2e} worst mean ratio {max(w[1], w2[1], w3[1]):.3f}")
    assert eng.scaler_state()["skipped_substeps"] == 0
    eng.assert_finite()


# ------------------------------------------------------------------------------------------------------- g6 in a larger frame
def test_g6_padded_fixture_in_a_448_frame_with_144_slots(golden_dir):
    """The existing padded-image fixture, its batches zero-extended to a 448 x 448 frame (196 cells): with 144 slots S = 185 as
    in the 384 frame the fixture was made in, and sample 0 (384 x 384) fills every slot -- count == max_patches through whole
    steps.  The bounds of tests/test_engine_gpu.py::test_padded_images_vs_reference_golden."""
    g = load(golden_dir, "g6_padded.npz")
    batches = [vilt_spec.extend_frame(O.pad_batch(O.synthetic_batch(4, 384, 6000 + s), G6_VALID, G6_TEXT), (448, 448))
               for s in range(2)]
    for use_graph in (False, True):
        P = _params("dat", ["art"])
        P0 = {k: v.clone() for k, v in P.items()}
        eng = _engine("dat", P, ["art"], 4, 448, max_patches=144)
        assert eng.S == 185 and (eng.gh, eng.gw, eng.g0) == (14, 14, 12)
        for mode in ("gating", "adapter_1"):
            pooled, logits = eng.forward(_dev(batches[0]), mode, "art")
            assert (pooled.cpu() - torch.from_numpy(g[f"fwd.{mode}.pooled"])).abs().max() < 3e-2
            assert (logits.cpu() - torch.from_numpy(g[f"fwd.{mode}.logits"])).abs().max() < 3e-2
        assert int(eng.key_mask2[0, 41:].sum()) == 144
        eng.begin_local_update("art", steps_per_epoch=2)
        if use_graph:
            eng.set_batch(_dev(vilt_spec.extend_frame(O.synthetic_batch(4, 384, 1), (448, 448))))
            eng._capture()
        for s, b in enumerate(batches):
            out = eng.train_step(_dev(b), use_graph=use_graph)
            ref = float(g["losses"][s])
            assert abs(float(out[0]) - ref) < 2e-3 * ref + 2e-3, (use_graph, s, float(out[0]), ref)
        _golden_update_parity(g, "after2.", eng.state_dict(), P0)
        eng.assert_finite()


# ------------------------------------------------------------------------------------------------------- all four modes vs the grid frame
@pytest.mark.parametrize("mode", ["dat", "adapter", "bias", "norm"])
def test_every_mode_agrees_with_its_grid_frame_engine(mode):
    """A full mixed batch, then a short one (3 of 4 samples) through the slot frame (35 slots in a 224 x 224 frame) and through
    the same mode's grid-frame engine: losses and updates agree within the bounds above, and the replica row's loss gradient
    is exactly zero."""
    tasks = ["art", "gqa"]
    full = vilt_spec.pad_to_valid(O.synthetic_batch(4, 224, 3100), SMALL_VALID, SMALL_TEXT)
    short = _first(vilt_spec.pad_to_valid(O.synthetic_batch(4, 224, 3101), SMALL_VALID[::-1], SMALL_TEXT), 3)
    engines = {}
    for frame in ("slots", "grid"):
        P = _params(mode, tasks)
        P0 = {k: v.clone() for k, v in P.items()}
        eng = _engine(mode, P, tasks, 4, 224, **({"max_patches": 35} if frame == "slots" else {}))
        eng.begin_local_update("art", steps_per_epoch=2)
        losses = []
        for b in (full, short):
            losses.append(float(eng.train_step(_dev(b), use_graph=True)[0]))
        torch.cuda.synchronize()
        assert eng.n_valid == 3 and torch.equal(eng.dlogits[3:], torch.zeros_like(eng.dlogits[3:]))
        assert float(eng.dlogits[:3].abs().max()) > 0
        engines[frame] = (eng, losses, {k: v.detach().cpu().clone() for k, v in eng.state_dict().items()})
    (es, ls, sds), (eg, lg, sdg) = engines["slots"], engines["grid"]
    assert es.S == 41 + 35 and eg.S == 41 + 49 and es.max_patches == 35 and eg.max_patches is None
    # the replicas of the short batch: sample 3 is sample 0 in every slot-frame input
    assert torch.equal(es.patches.view(4, -1)[3], es.patches.view(4, -1)[0])
    assert torch.equal(es.inp["patch_mask"][3], es.inp["patch_mask"][0]) and torch.equal(es.key_mask2[3], es.key_mask2[0])
    for s, (a, b) in enumerate(zip(ls, lg)):
        print(f"{mode} step {s + 1}: loss slots {a:.5f} grid {b:.5f}")
        assert abs(a - b) < 2e-3 * abs(b) + 2e-3, (s, a, b)
    names = [k for k in sds if "adapter_2" not in k and not k.startswith("task_layer.gqa.")]
    w = assert_update_parity([k for k in names if not _is_key_bias(k)], sds, sdg, P0, 1e-3, REL_MEAN, f"{mode} slots vs grid")
    for k in names:
        if _is_key_bias(k):
            assert float((sds[k] - sdg[k]).abs().max()) < 1e-3, k
    print(f"{mode}: slots vs grid after 2 steps, worst (max |ddW|, mean ratio) {w}")
    assert all(torch.equal(sds[k], P0[k]) for k in sds if k.startswith("task_layer.gqa."))
    es.assert_finite()


# ------------------------------------------------------------------------------------------------------- overflow
def test_a_sample_over_the_slot_budget_raises_and_training_goes_on():
    from feddat_amd import lib as L
    ok = vilt_spec.pad_to_valid(O.synthetic_batch(4, 224, 3200), SMALL_VALID, SMALL_TEXT)
    over = vilt_spec.pad_to_valid(O.synthetic_batch(4, 224, 3201), [(160, 224), (224, 224), (96, 192), (224, 160)])
    eng = _engine("dat", _params("dat", ["art"]), ["art"], 4, 224, max_patches=35)
    eng.begin_local_update("art", steps_per_epoch=3)
    state0 = [t.clone() for t in _step_state(eng)]
    # a host batch: the masks are read where they are
    staged = eng.patches.view(torch.int16).clone()      # (bits: the buffer is uninitialised memory before the first batch)
    with pytest.raises(L.FeddatHipError, match="sample 1 has 49 valid patches"):
        eng.set_batch(over)
    assert torch.equal(eng.patches.view(torch.int16), staged)
    # a device batch: nobody reads the masks on the host; the step's own kernel raises the flag, the end-of-update check reports it
    eng.train_step(_dev(over))
    torch.cuda.synchronize()
    assert int(eng.slot_overflow.item()) == 1
    # the sample kept its first 35 cells (5 rows of the 7 x 7 grid): all 35 slots are valid keys, the state is finite
    assert eng.key_mask2[1, 41:].tolist() == [1] * 35
    assert all(bool(torch.isfinite(t).all()) for t in _trained(eng).values())
    with pytest.raises(L.FeddatHipError, match="max_patches = 35"):
        eng.assert_finite()
    eng.assert_finite()          # reported once: the flag is cleared
    # ... and a later in-budget batch trains as on an engine that never saw the other one
    for t, v in zip(_step_state(eng), state0):
        t.copy_(v)
    eng.repack()
    eng.train_step(_dev(ok))
    got = _trained(eng)
    fresh = _engine("dat", _params("dat", ["art"]), ["art"], 4, 224, max_patches=35)
    fresh.begin_local_update("art", steps_per_epoch=3)
    fresh.train_step(_dev(ok))
    want = _trained(fresh)
    assert got.keys() == want.keys() and all(torch.equal(got[k], want[k]) for k in got)
    eng.assert_finite()


def test_trainer_reports_the_budget_at_the_end_of_the_local_update():
    import types
    from feddat_amd import lib as L, modeling, train
    over = vilt_spec.pad_to_valid(O.synthetic_batch(4, 224, 3201), [(160, 224), (224, 224), (96, 192), (224, 160)])
    m = modeling.create_vilt_continual_learner_model(_params("dat", ["art"]), ["art"], DEV, batch_size=4, image_size=224,
                                                     num_layers=2, max_patches=35)
    assert m.engine.max_patches == 35 and m.image_processor.pad_to == (224, 224)
    args = types.SimpleNamespace(local_epochs=1, num_epochs=15, lr=1e-4, optimizer_mode="dat", debug=0, hip_graph=True)
    with pytest.raises(L.FeddatHipError, match="max_patches = 35"):
        train.TaskTrainer(args, "art", [_dev(over)]).train(m)
    # raw images: the ViLT size rule says how many patches an image becomes before anything is resized or tokenised
    import numpy as np
    with pytest.raises(L.FeddatHipError, match="image 0 .* 144 patches"):
        m.process_inputs([np.zeros((100, 100, 3), np.uint8)], ["what is this"])


# ------------------------------------------------------------------------------------------------------- raw images, both orientations
def test_raw_portrait_and_landscape_images_through_the_model(golden_dir):
    """model(task_key, images=[uint8 arrays], texts=[str]) in a 640 x 640 frame with 240 slots: a landscape, a portrait, a square
    and a small portrait image go through the learner's own image processor (pad_to = the engine's frame) unchanged -- 209, 209,
    144 and 216 valid patches, S = 281 where the grid frame would need 441 -- and the logits follow the CPU oracle on the
    host-processed batch (HF visual_embed semantics at the full 640 x 640 grid)."""
    from feddat_amd import modeling
    from oracle import image_oracle as IO
    from tests.test_weights_gpu import _oracle_encodings, _raw_batch
    frame = (640, 640)
    vocab, raw = _raw_batch(golden_dir, 4, 3)
    raw["images"] = IO.synthetic_images([(300, 500), (500, 300), (384, 384), (500, 333)], seed=3)
    d = O.ViltDims(layers=2)
    P = O.make_params(d, ["art"], bias_std=0.02)
    m = modeling.create_vilt_continual_learner_model(P, ["art"], DEV, 4, frame, 2, vocab=vocab, max_patches=240)
    assert m.engine.S == 281 and m.image_processor.pad_to == frame
    enc, ref = m.process_inputs(raw["images"], raw["raw_texts"]), _oracle_encodings(vocab, raw, frame)
    for k in ("pixel_values", "pixel_mask", "input_ids", "attention_mask", "token_type_ids"):
        assert torch.equal(enc[k].cpu(), ref[k]), k
    _, counts, over = vilt_spec.patch_slot_plan(ref["pixel_mask"][:, ::32, ::32], 240)
    assert counts.tolist() == [209, 209, 144, 216] and not over.any()      # 352 x 608, 608 x 352, 384 x 384, 576 x 384
    m.activate_gating()
    pooled, logits = m(task_key="art", images=raw["images"], texts=raw["raw_texts"])
    with torch.no_grad():
        rp, rl = O.vilt_forward(P, d, {k: v for k, v in ref.items() if k != "target_scores"}, "gating", "art")
    dp, dl = float((pooled.cpu() - rp).abs().max()), float((logits.cpu() - rl).abs().max())
    print(f"raw mixed batch: |pooled| {dp:.2e} |logits| {dl:.2e}")
    assert dp < 3e-2 and dl < 3e-2
    m.engine.assert_finite()


# ------------------------------------------------------------------------------------------------------- train.main
def _state_hash(model):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for _, grp in model.engine._named_groups():
        h.update(grp.p.cpu().numpy().tobytes())
    h.update(model.engine.comm_flat().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def test_main_in_a_mixed_frame_and_the_default_run_is_the_parents():
    from feddat_amd import train
    mixed = MAIN_COMMON + ["--image_frame", "384,384", "--max_image_patches", "84", "--synthetic_orientations"]
    a, b = train.main(mixed), train.main(mixed)
    assert a.engine.max_patches == 84 and a.engine.S == 125 and a.engine.res == (384, 384)
    fa = a.engine.comm_flat()
    assert bool(torch.isfinite(fa).all()) and _state_hash(a) == _state_hash(b)
    plain = train.main(MAIN_COMMON)
    assert plain.engine.max_patches is None and plain.engine.S == 185
    hp = _state_hash(plain)
    print("state hash of the default run:", hp, "mixed frame:", _state_hash(a))
    assert hp == PARENT_MAIN_HASH and hp != _state_hash(a)
