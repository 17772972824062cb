"""The reference's whole image transform on the device, bit for bit: stage 1 (the image datasets' bilinear Resize(size, max_size),
feddat_image_resample_u8 / DatasetResize), stage 2 for ALBEF (bicubic Resize((R, R)) + ToTensor + Normalize,
feddat_albef_image_preprocess / AlbefImageTransform), stage 1 in front of the existing ViLT processor, and both model classes
and feddat_amd.train.main on lists of decoded uint8 images.

Everything is compared with np.array_equal / torch.equal / CRC32 against tests/image_path_ref.py (pinned to Pillow by
tests/test_image_path_cpu.py) and against tests/golden/gi1_image_path.npz (written from Pillow): bit-exactness is the claim, so
there is no tolerance.  The kernels' logic does not depend on the sizes, so most cases use size = 64, max_size = 96, R = 64; one
case each runs at the sizes of real use (384 / 640 / 384)."""
import numpy as np
import pytest
import torch

from oracle import image_oracle as IO
from tests import image_path_ref as R
from tests.golden_util import load

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = dict(vit_depth=2, enc_layers=3, fusion_layer=1, dec_layers=2, image=64, vocab=3072, max_pos=64)   # tests/test_albef_gpu.py's


@pytest.fixture(scope="module")
def IP():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import image_processing
    return image_processing


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load(golden_dir, "gi1_image_path.npz")


_REF = {}


def _ref(name):
    """(sources, stage-1 bytes, both stages' float32 tensors) of one shared case, computed once."""
    if name not in _REF:
        par, _ = R.CASES[name]
        imgs = R.case_images(name)
        s1 = [R.dataset_resize(im, par["size"], par["max_size"]) for im in imgs]
        both = [R.to_tensor_normalize(IO.pil_bicubic_resize(im, par["R"], par["R"])) for im in s1]
        _REF[name] = (imgs, s1, both)
    return _REF[name]


def _check_stage1(packed, name, golden):
    imgs, s1, _ = _ref(name)
    assert len(packed) == len(imgs)
    got = [packed.image(i).cpu().numpy() for i in range(len(imgs))]
    assert np.array_equal(np.array([g.shape[:2] for g in got], np.int32), golden[f"{name}.s1_shape"])
    for i, (g, want) in enumerate(zip(got, s1)):
        assert np.array_equal(g, want), (name, i, imgs[i].shape)
    assert [R.crc(g) for g in got] == golden[f"{name}.s1_crc"].tolist()


# ------------------------------------------------------------------------------------------------ 1. stage 1 alone
def test_stage1_bilinear(IP, golden):
    """Down-scales, up-scales, the cap, a 1-pixel-high and a 3-row result, and the two sources the rule leaves unchanged
    ((64, 200): short == size with long > max_size; (96, 64)): those keep their uploaded bytes at their uploaded offsets."""
    par, shapes = R.CASES["small"]
    imgs = R.case_images("small")
    resize = IP.DatasetResize(DEV, par["size"], par["max_size"])
    packed = resize(imgs)
    _check_stage1(packed, "small", golden)
    plain = IP.pack_images(imgs, DEV)
    for i in (2, 5):
        assert packed.offsets[i] == plain.offsets[i] and (packed.heights[i], packed.widths[i]) == shapes[i]
    moved = [i for i in range(len(imgs)) if i not in (2, 5)]
    assert all(packed.offsets[i] >= plain.data.numel() for i in moved)
    for i in R.STORED:
        assert np.array_equal(packed.image(i).cpu().numpy(), golden[f"small.{i}.s1"])
    # torch tensors and a second call on the same object (its workspace is reused) give the same bytes
    again = resize([torch.from_numpy(im) for im in imgs])
    assert torch.equal(again.data, packed.data) and np.array_equal(again.offsets, packed.offsets)
    # the ViLT gate: only images with min(h, w) > size pass stage 1
    gated = resize(imgs, larger_only=True)
    for i, im in enumerate(imgs):
        want = R.dataset_resize(im, par["size"], par["max_size"], larger_only=True)
        assert np.array_equal(gated.image(i).cpu().numpy(), want), i
    assert [i for i, im in enumerate(imgs) if gated.image(i).shape != im.shape] == [6]          # (300, 90) alone


def test_heavy_downscale_both_filters_and_an_unchanged_axis(IP, golden):
    """feddat_image_resample_u8 itself: 1600 -> 64 bilinear (51 taps per output pixel), the same with the bicubic filter, and
    resamples that change one axis only (Pillow skips the other pass; here its unit-scale table is the identity)."""
    from feddat_amd import lib as L
    src = R.case_images("heavy")[0]
    (oh, ow) = R.HEAVY[1]
    dst = np.array([0, oh * ow * 3, 2 * oh * ow * 3, 2 * oh * ow * 3 + 400 * 64 * 3], np.int64)
    total = int(dst[3]) + 64 * 1600 * 3
    data = torch.from_numpy(src.reshape(-1)).to(DEV)
    out = torch.full((total + 32,), 0xA5, dtype=torch.uint8, device=DEV)
    L.image_resample_u8(data, [0], [400], [1600], [oh], [ow], out, dst[:1], L.FILTER_BILINEAR)
    L.image_resample_u8(data, [0], [400], [1600], [oh], [ow], out, dst[1:2], L.FILTER_BICUBIC)
    L.image_resample_u8(data, [0, 0], [400, 400], [1600, 1600], [400, 64], [64, 1600], out, dst[2:], L.FILTER_BILINEAR)
    o = out.cpu().numpy()
    bil = o[:oh * ow * 3].reshape(oh, ow, 3)
    assert R.crc(bil) == int(golden["heavy.crc"][0]) and np.array_equal(bil, R.pil_bilinear_resize(src, oh, ow))
    assert np.array_equal(o[dst[1]:dst[2]].reshape(oh, ow, 3), IO.pil_bicubic_resize(src, oh, ow))
    assert np.array_equal(o[dst[2]:dst[3]].reshape(400, 64, 3), R.pil_bilinear_resize(src, 400, 64))
    assert np.array_equal(o[dst[3]:total].reshape(64, 1600, 3), R.pil_bilinear_resize(src, 64, 1600))
    assert (o[total:] == 0xA5).all()
    with pytest.raises(L.FeddatHipError, match="past the end"):
        L.image_resample_u8(data, [1], [400], [1600], [oh], [ow], out, [0])
    with pytest.raises(L.FeddatHipError, match="past the end"):
        L.image_resample_u8(data, [0], [400], [1600], [oh], [ow], out, [total + 32 - oh * ow * 3 + 1])


def test_offsets_past_two_gib(IP):
    """Byte offsets are 64-bit end to end: a source and a result that both sit behind 2^31 bytes of one buffer (what a packed
    batch of large photographs reaches) -- the buffer is allocated, not filled."""
    from feddat_amd import lib as L
    im = IO.synthetic_images([(37, 53)], seed=31)[0]
    big = (1 << 31) + (1 << 20)
    buf = torch.empty(big, dtype=torch.uint8, device=DEV)
    so, do = (1 << 31) + 7, (1 << 31) + 40000
    buf[so:so + im.size].copy_(torch.from_numpy(im.reshape(-1)))
    L.image_resample_u8(buf, [so], [37], [53], [64], [91], buf, [do])
    assert np.array_equal(buf[do:do + 64 * 91 * 3].cpu().numpy().reshape(64, 91, 3), R.pil_bilinear_resize(im, 64, 91))
    out = torch.empty(1, 3, 64, 64, device=DEV)
    L.albef_image_preprocess(buf, [so], [37], [53], out, R.ALBEF_MEAN, R.ALBEF_STD)
    assert np.array_equal(out[0].cpu().numpy(), R.albef_transform(im, 64, dataset_resize_first=False))
    del buf
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ 2. stage 2 alone
def test_stage2_bicubic_to_tensor_normalize(IP, golden):
    """The same sources straight to [n, 3, 64, 64] float32, plus (64, 64): the identity on both axes, where the floats are
    ToTensor + Normalize of the source bytes themselves."""
    imgs = R.case_images("stage2")
    out = IP.AlbefImageTransform(DEV, image=64)(imgs, dataset_resize=False)
    assert out.dtype == torch.float32 and tuple(out.shape) == (len(imgs), 3, 64, 64) and out.is_contiguous()
    got = out.cpu().numpy()
    for i, im in enumerate(imgs):
        assert np.array_equal(got[i], R.albef_transform(im, 64, dataset_resize_first=False)), (i, im.shape)
    assert [R.crc(g) for g in got] == golden["stage2.crc"].tolist()
    assert imgs[-1].shape == (64, 64, 3) and np.array_equal(got[-1], R.to_tensor_normalize(imgs[-1]))
    # other statistics travel by value: the ViLT processor's 0.5 / 0.5 on the same bytes
    half = IP.AlbefImageTransform(DEV, image=64, mean=(0.5, 0.5, 0.5), std=(0.5, 0.25, 2.0))(imgs[:2], dataset_resize=False)
    for i in range(2):
        want = R.to_tensor_normalize(IO.pil_bicubic_resize(imgs[i], 64, 64), (0.5, 0.5, 0.5), (0.5, 0.25, 2.0))
        assert np.array_equal(half[i].cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ 3. both stages
def test_both_stages_small_and_out_slice(IP, golden):
    """Both stages back to back, into a caller's slice: the samples around it keep their bytes."""
    par, _ = R.CASES["small"]
    imgs, _, both = _ref("small")
    n = len(imgs)
    tr = IP.AlbefImageTransform(DEV, image=par["R"], size=par["size"], max_size=par["max_size"])
    frame = torch.full((n + 3, 3, 64, 64), -7.25, device=DEV)
    ret = tr(imgs, out=frame[2:2 + n])
    assert ret.data_ptr() == frame[2].data_ptr()
    got = frame.cpu().numpy()
    for i in range(n):
        assert np.array_equal(got[2 + i], both[i]), (i, imgs[i].shape)
    assert [R.crc(got[2 + i]) for i in range(n)] == golden["small.both_crc"].tolist()
    for i in R.STORED:
        assert np.array_equal(got[2 + i], golden[f"small.{i}.both"])
    assert (got[:2] == -7.25).all() and (got[2 + n:] == -7.25).all()
    from feddat_amd import lib as L
    with pytest.raises(L.FeddatHipError, match="out is"):
        tr(imgs, out=frame[:n + 1])
    # dataset_resize=False on stage-1 results == both stages; a PackedImages goes in as it is
    resized = IP.DatasetResize(DEV, par["size"], par["max_size"])(imgs)
    assert torch.equal(tr(resized), frame[2:2 + n])


def test_both_stages_full_size(IP, golden):
    """The sizes of real use: (480, 640) and (640, 427) -> Resize(384, max_size=640) -> [2, 3, 384, 384]."""
    imgs, _, both = _ref("full")
    resize = IP.DatasetResize(DEV)
    _check_stage1(resize(imgs), "full", golden)
    out = IP.AlbefImageTransform(DEV)(imgs).cpu().numpy()
    assert out.shape == (2, 3, 384, 384)
    for i in range(2):
        assert np.array_equal(out[i], both[i]), i
    assert [R.crc(o) for o in out] == golden["full.both_crc"].tolist()


def test_many_images_cross_the_descriptor_group(IP, golden):
    """53 tiny images: two launches of 48 + 5 descriptors in every kernel, the second group's workspace behind the first's."""
    par, _ = R.CASES["many"]
    imgs, _, both = _ref("many")
    assert len(imgs) == 53
    _check_stage1(IP.DatasetResize(DEV, par["size"], par["max_size"])(imgs), "many", golden)
    out = IP.AlbefImageTransform(DEV, image=par["R"], size=par["size"], max_size=par["max_size"])(imgs).cpu().numpy()
    for i in range(53):
        assert np.array_equal(out[i], both[i]), (i, imgs[i].shape)
    assert [R.crc(o) for o in out] == golden["many.both_crc"].tolist()


# ------------------------------------------------------------------------------------------------ 4. ViLT
def _vilt_model(golden_dir, dataset_resize):
    from feddat_amd import modeling
    from oracle import feddat_oracle as O
    g9 = load(golden_dir, "g9_wordpiece.npz")
    vocab = str(g9["vocab"]).split("\n")
    P = O.make_params(O.ViltDims(layers=2), ["art"], bias_std=0.02)
    return modeling.create_vilt_continual_learner_model(P, ["art"], DEV, 2, (384, 640), 2, vocab=vocab, dataset_resize=dataset_resize)


def test_vilt_stage1_then_the_processor(IP, golden, golden_dir):
    """(600, 800) -> bilinear (384, 512) -> the existing processor == Pillow's stage-1 bytes through the oracle's processor; with
    dataset_resize=False the model gives the processor's own pixels on the unresized photograph (the behaviour before there
    was a stage 1), and dataset_resize=True leaves an image with min(h, w) <= 384 alone."""
    imgs, s1, _ = _ref("vilt")
    small = IO.synthetic_images([(333, 500)], seed=2)
    proc = IP.ViltImageProcessor(DEV, pad_to=(384, 640))
    packed = IP.DatasetResize(DEV)(imgs, larger_only=True)
    _check_stage1(packed, "vilt", golden)
    enc = proc(packed)
    rpx, rpm = IO.vilt_image_processor(s1)
    H, W = rpx.shape[2:]
    assert (H, W) == (384, 512)
    px, pm = enc["pixel_values"].cpu().numpy(), enc["pixel_mask"].cpu().numpy()
    assert np.array_equal(px[:, :, :H, :W], rpx) and np.array_equal(pm[:, :H, :W], rpm) and not px[:, :, :, W:].any()
    parent = proc(imgs + small)                                   # the processor alone, as before
    parent_crc = [R.crc(parent["pixel_values"][i].cpu().numpy()) for i in range(2)]
    assert parent_crc[0] != R.crc(px[0])                          # stage 1 changes the photograph's pixels
    texts = ["what is in the picture?", "how many are there?"]
    off = _vilt_model(golden_dir, False).process_inputs(imgs + small, texts)
    assert [R.crc(off["pixel_values"][i].cpu().numpy()) for i in range(2)] == parent_crc
    on = _vilt_model(golden_dir, True).process_inputs(imgs + small, texts)
    assert R.crc(on["pixel_values"][0].cpu().numpy()) == R.crc(px[0])
    assert R.crc(on["pixel_values"][1].cpu().numpy()) == parent_crc[1]
    assert torch.equal(on["pixel_mask"][1], parent["pixel_mask"][1]) and torch.equal(on["input_ids"], off["input_ids"])


def test_vilt_checks_use_the_sizes_after_stage1(IP, golden_dir):
    """A 640 x 427 portrait: the processor alone resizes it to 576 x 384 (int(575.55 + 0.5) = 576: 18 x 12 = 216 patches); stage 1
    truncates to 575 x 384 first, which the processor floors to 544 x 384 (17 x 12 = 204 patches).  A slot budget of 210 therefore
    takes the image with dataset_resize=True and refuses it without."""
    from feddat_amd import lib as L, modeling
    from oracle import feddat_oracle as O
    g9 = load(golden_dir, "g9_wordpiece.npz")
    vocab = str(g9["vocab"]).split("\n")
    P = O.make_params(O.ViltDims(layers=2), ["art"], bias_std=0.02)
    img = IO.synthetic_images([(640, 427)], seed=6)
    assert IO.resize_output_size(640, 427) == (576, 384) and IO.resize_output_size(575, 384) == (544, 384)
    models = {on: modeling.create_vilt_continual_learner_model(P, ["art"], DEV, 1, (640, 640), 2, vocab=vocab, max_patches=210,
                                                               dataset_resize=on) for on in (False, True)}
    with pytest.raises(L.FeddatHipError, match="216 patches"):
        models[False].process_inputs(img, ["what?"])
    enc = models[True].process_inputs(img, ["what?"])
    want = IO.vilt_image_processor([R.dataset_resize(img[0], larger_only=True)])[0]
    assert want.shape == (1, 3, 544, 384)
    px = enc["pixel_values"].cpu().numpy()
    assert np.array_equal(px[:, :, :544, :384], want) and not px[:, :, 544:].any() and not px[:, :, :, 384:].any()
    assert int(enc["pixel_mask"].sum()) == 544 * 384


# ------------------------------------------------------------------------------------------------ 5. ALBEF end to end
def _albef_model(B=3, N=4, **kw):
    from feddat_amd import albef_modeling
    from oracle import albef_oracle as A
    P = A.make_params(A.AlbefDims(**SMALL))
    return albef_modeling.create_albef_continual_learner_model(P, DEV, B, N, q_len=12, a_len=5, dropout=0.0,
                                                               **{k: v for k, v in SMALL.items() if k != "max_pos"}, **kw)


def _train_batches(IP, steps=2, B=3):
    from feddat_amd import albef_spec
    tr = IP.AlbefImageTransform(DEV, image=64)
    out = []
    for s in range(steps):
        b = albef_spec.synthetic_batch(B, 40 + s, image=64, q_len=12, a_len=5, k=[2, 1, 1], vocab=SMALL["vocab"], device=DEV)
        raw = albef_spec.synthetic_raw_images(B, 70 + s, image=64)
        out.append((dict(b, image=tr(raw).clone()), dict(b, image=raw)))
    return out


def test_albef_trains_on_image_lists_bit_for_bit(IP):
    """A SMALL model given lists of uint8 images: train_step losses and state_dict() equal those of the same model given the
    transform's float tensor; the list is transformed into the engine's own image buffer."""
    import types
    from feddat_amd import lib as L, train
    args = types.SimpleNamespace(local_epochs=1, num_epochs=15, lr=1e-4, optimizer_mode="dat", debug=0, hip_graph=False)
    batches = _train_batches(IP)
    losses, states = [], []
    for which in (0, 1):
        model = _albef_model()
        init = {k: v.clone().cpu() for k, v in model.state_dict().items()}
        trainer = train.AlbefTaskTrainer(args, "art", [b[which] for b in batches], [])
        eng = model.engine
        eng.begin_local_update(steps_per_epoch=2, num_epochs=1, warmup_ratio=0.1, opt_adapters=(0, 1))
        ls = []
        for step, b in enumerate(trainer.vqa_train_dataloader):
            ls.append(trainer.train_step(model, step, b).clone())
            if which == 1:
                assert torch.equal(eng.inp["image"], batches[step][0]["image"])
        losses.append(torch.stack(ls).cpu())
        states.append({k: v.clone().cpu() for k, v in model.state_dict().items()})
        if which == 1:
            enc = model.process_inputs(dict(batches[0][1], train=True))
            assert enc["image"].data_ptr() == eng.inp["image"].data_ptr() and torch.equal(enc["question_ids"], batches[0][1]["question_ids"])
            with pytest.raises(L.FeddatHipError, match="training batches bring exactly 3"):
                model.process_inputs(dict(batches[0][1], image=batches[0][1]["image"][:2], train=True))
            # "images", the reference's key, and dataset_resize=False on images that already passed stage 1
            same = model.process_inputs({**{k: v for k, v in batches[0][1].items() if k != "image"}, "images": batches[0][1]["image"]})
            assert torch.equal(same["image"], batches[0][0]["image"]) and "images" not in same
    assert torch.isfinite(losses[0]).all() and torch.equal(losses[0], losses[1])
    assert states[0].keys() == states[1].keys() and all(torch.equal(states[0][k], states[1][k]) for k in states[0])
    assert any(not torch.equal(states[0][k], init[k]) for k in init)          # and the steps did train


def test_albef_ranks_a_short_batch_of_image_lists(IP):
    """rank_answer on 2 questions in a frame of 3, images as a list == the same on the transform's float tensor."""
    from feddat_amd import albef_spec, lib as L
    model = _albef_model(dataset_resize=False)
    a_ids, a_mask = albef_spec.synthetic_answer_list(20, 5, SMALL["vocab"], seed=3)
    loader = albef_spec.synthetic_eval_loader(2, 2, 9, a_ids, a_mask, 6, image=64, q_len=12, vocab=SMALL["vocab"], device=DEV)
    raw = albef_spec.synthetic_raw_images(2, 11, image=64)
    x = IP.AlbefImageTransform(DEV, image=64)(raw, dataset_resize=False).clone()
    ids_t, probs_t = model("art", dict(loader[0], image=x, train=False))
    ids_t, probs_t = ids_t.clone(), probs_t.clone()
    ids_l, probs_l = model("art", dict(loader[0], image=raw, train=False))
    assert tuple(ids_l.shape) == (2, 6) and torch.equal(ids_l, ids_t) and torch.equal(probs_l, probs_t)
    assert torch.equal(model.engine.inp["image"][:2], x)
    for bad in ([], raw + raw):
        with pytest.raises(L.FeddatHipError):
            model("art", dict(loader[0], image=bad, train=False))


def test_train_main_with_raw_images_is_reproducible(tmp_path):
    """train.main --synthetic_raw_images: two rounds with training and evaluation batches of decoded images run, and a second run
    gives the same bits; without the option the batches carry N(0, 1) tensors as before."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import train
    argv = ["--encoder_name", "albef_no_distill", "--ordered_cl_tasks", "art,gqa", "--image_size", "64", "--batch_size", "2",
            "--synthetic_steps", "2", "--comm_rounds", "2", "--albef_dims",
            "vit_depth=2,enc_layers=3,fusion_layer=1,dec_layers=2,vocab=3072,max_pos=64", "--output_dir", str(tmp_path / "raw"),
            "--synthetic_answer_list", "12", "--synthetic_eval_questions", "3", "--val_batch_size", "2", "--synthetic_raw_images"]
    runs = []
    for _ in range(2):
        model = train.main(argv)
        assert sorted(model.eval_scores) == [0, 1]
        for t in ("art", "gqa"):
            assert [len(b["image"]) for b in model.eval_data[t]] == [2, 1]
            assert all(isinstance(b["image"], list) and b["image"][0].dtype == np.uint8 for b in model.eval_data[t])
        runs.append(({k: v.clone().cpu() for k, v in model.state_dict().items()},
                     {t: {k: v.clone().cpu() for k, v in p.items()} for t, p in model.personal_params.items()}, model.eval_scores))
    (sd0, pp0, sc0), (sd1, pp1, sc1) = runs
    assert all(torch.equal(sd0[k], sd1[k]) for k in sd0) and sc0 == sc1
    assert all(torch.equal(pp0[t][k], pp1[t][k]) for t in pp0 for k in pp0[t])
    assert all(torch.isfinite(v).all() for v in sd0.values())
