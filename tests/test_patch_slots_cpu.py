"""Patch slots without a GPU: the slot mapping (vilt_spec.patch_slot_plan) against HF's own ViltEmbeddings.visual_embed from the
installed transformers on the masks of the mixed-frame fixture (gm1, tools/make_mixed_frame_golden.py), the overflow report, the
C ABI of the two slot kernels (declared = exported = bound; argument checks), the host helpers that build mixed batches, and what
train.main and the engines refuse."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from feddat_amd import lib as L
from feddat_amd import vilt_spec
from oracle import feddat_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("feddat_im2col_patches_slots", "feddat_image_embed_assemble_slots")
EINVAL = 1
GM1_VALID = [(384, 224), (224, 384), (288, 288), (160, 320)]
GM1_TEXT = [40, 31, 40, 12]


@pytest.fixture(scope="module")
def gm1(golden_dir):
    return np.load(os.path.join(golden_dir, "gm1_mixed_frame.npz"))


def test_fixture_is_the_reference_at_125_positions(gm1):
    """What the fixture says about itself: the four rectangles' patch counts, and that the reference ran its encoder on
    40 + 1 + 84 positions (the grid frame would hold 185)."""
    assert gm1["counts"].tolist() == [84, 84, 81, 50] and int(gm1["encoder_seq"]) == 125
    b = O.pad_batch(O.synthetic_batch(4, 384, int(gm1["seed0"])), GM1_VALID, GM1_TEXT)
    assert np.array_equal(b["pixel_mask"][:, ::32, ::32].numpy(), gm1["patch_mask"])
    assert gm1["dat.losses"].shape == (2,) and gm1["bias.losses"].shape == (4,)


def test_plan_is_hf_visual_embed_order(gm1):
    """HF visual_embed (max_image_length = -1, as the reference calls it) returns the grid cell of every sequence position:
    for a sample with fewer valid patches than the batch maximum its valid cells come first, in valid_row_idx order = the plan's;
    the largest samples are drawn as a random permutation of their valid cells: equal as sets."""
    from transformers import ViltConfig
    from transformers.models.vilt.modeling_vilt import ViltEmbeddings
    pm = torch.from_numpy(gm1["patch_mask"])
    B, gh, gw = pm.shape
    cells, counts, over = vilt_spec.patch_slot_plan(pm, 84)
    assert counts.tolist() == [84, 84, 81, 50] and not over.any()
    torch.manual_seed(5)
    emb = ViltEmbeddings(ViltConfig(hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64,
                                    image_size=384)).eval()
    pixel_mask = pm.repeat_interleave(32, 1).repeat_interleave(32, 2)
    with torch.no_grad():
        x, x_mask, (patch_index, (h, w)) = emb.visual_embed(torch.zeros(B, 3, 384, 384), pixel_mask, max_image_length=-1)
    assert (h, w) == (gh, gw) and x.shape[1] == 1 + 84 and patch_index.shape == (B, 84, 2)
    hf_cells = patch_index[..., 0] * gw + patch_index[..., 1]
    most = int(counts.max())
    for b in range(B):
        n = int(counts[b])
        if n < most:
            assert hf_cells[b, :n].tolist() == cells[b, :n].tolist(), b
            assert x_mask[b, 1:1 + n].all() and not x_mask[b, 1 + n:].any()
        else:
            assert sorted(hf_cells[b].tolist()) == sorted(cells[b].tolist()), b
        assert (cells[b, n:] == -1).all()


def test_plan_counts_overflow_and_empty():
    pm = torch.zeros(4, 3, 5, dtype=torch.int64)
    pm[0, :2, :3] = 1            # 6 patches: count == max_patches is no overflow
    pm[1] = 1                    # 15 patches: overflow, the first 6 cells stay
    pm[2, :3, :1] = 1            # one column
    cells, counts, over = vilt_spec.patch_slot_plan(pm, 6)      # sample 3: no valid patch
    assert counts.tolist() == [6, 15, 3, 0] and over.tolist() == [False, True, False, False]
    assert cells[0].tolist() == [0, 1, 2, 5, 6, 7]
    assert cells[1].tolist() == [0, 1, 2, 3, 4, 5]
    assert cells[2].tolist() == [0, 5, 10, -1, -1, -1]
    assert cells[3].tolist() == [-1] * 6
    for bad in (0, 16):
        with pytest.raises(ValueError):
            vilt_spec.patch_slot_plan(pm, bad)


def test_host_helpers_build_mixed_batches():
    """pad_to_valid is the oracle's pad_batch; extend_frame zero-extends pixels and mask; synthetic_mixed_batch is seeded, keeps
    synthetic_batch's text and targets, and zero-pads outside each sample's rectangle."""
    b = O.synthetic_batch(4, 384, 7000)
    want, got = O.pad_batch(b, GM1_VALID, GM1_TEXT), vilt_spec.pad_to_valid(b, GM1_VALID, GM1_TEXT)
    assert want.keys() == got.keys() and all(torch.equal(want[k], got[k]) for k in want)
    ext = vilt_spec.extend_frame(got, (448, 416))
    assert ext["pixel_values"].shape == (4, 3, 448, 416) and ext["pixel_mask"].shape == (4, 448, 416)
    assert torch.equal(ext["pixel_values"][:, :, :384, :384], got["pixel_values"]) and int(ext["pixel_mask"].sum()) == int(got["pixel_mask"].sum())
    assert float(ext["pixel_values"][:, :, 384:].abs().max()) == 0 and float(ext["pixel_values"][:, :, :, 384:].abs().max()) == 0
    assert vilt_spec.orientation_sizes((384, 384)) == [(224, 384), (384, 224), (288, 288), (96, 288)]
    assert vilt_spec.orientation_sizes((640, 640))[:2] == [(384, 640), (640, 384)]
    m1, m2 = (vilt_spec.synthetic_mixed_batch(8, (384, 384), 11) for _ in range(2))
    assert all(torch.equal(m1[k], m2[k]) for k in m1)
    plain = vilt_spec.synthetic_batch(8, 384, 11)
    assert all(torch.equal(m1[k], plain[k]) for k in ("input_ids", "target_scores", "attention_mask"))
    _, counts, _ = vilt_spec.patch_slot_plan(m1["pixel_mask"][:, ::32, ::32], 84)
    assert set(counts.tolist()) <= {84, 81, 27} and len(set(counts.tolist())) > 1
    assert float((m1["pixel_values"] * (1 - m1["pixel_mask"][:, None]).float()).abs().max()) == 0
    wide = vilt_spec.synthetic_mixed_batch(2, (384, 640), 3, sizes=[(384, 640)])
    assert wide["pixel_values"].shape == (2, 3, 384, 640) and bool(wide["pixel_mask"].all())


@pytest.mark.parametrize("f16", [False, True])
def test_new_symbols_declared_exported_bound_and_checked(f16):
    from feddat_amd import build
    src = open(os.path.join(ROOT, "include", "feddat_hip.h")).read()
    lib = ctypes.CDLL(build.build(f16=f16))
    for n in NEW_SYMBOLS:
        assert re.search(rf"^(?:int|long) {n}\(", src, flags=re.M), n
        assert n in L.EXPORTED_SYMBOLS and hasattr(lib, n), n
    assert lib.feddat_abi_version() == 8
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    X = 0x1000          # never dereferenced: every call below is refused by the argument checks
    ga = lib.feddat_im2col_patches_slots
    ga.argtypes, ga.restype = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp], i32
    # (pixels, patch_mask, patches, n, B, C, Hi, Wi, P, max_patches, stream); the frame is 96 x 160: 3 x 5 cells
    assert ga(None, X, X, 3, 3, 3, 96, 160, 32, 6, None) == EINVAL
    assert ga(X, None, X, 3, 3, 3, 96, 160, 32, 6, None) == EINVAL
    assert ga(X, X, None, 3, 3, 3, 96, 160, 32, 6, None) == EINVAL
    assert ga(X, X, X, 3, 3, 3, 96, 160, 32, 0, None) == EINVAL               # max_patches < 1
    assert ga(X, X, X, 3, 3, 3, 96, 160, 32, 16, None) == EINVAL              # max_patches > gh * gw
    assert ga(X, X, X, 0, 3, 3, 96, 160, 32, 6, None) == EINVAL               # n < 1
    assert ga(X, X, X, 4, 3, 3, 96, 160, 32, 6, None) == EINVAL               # n > B
    assert ga(X, X, X, 3, 3, 3, 100, 160, 32, 6, None) == EINVAL              # Hi % P
    assert ga(X, X, X, 3, 3, 3, 60, 90, 30, 6, None) == EINVAL                # P % 4
    asm = lib.feddat_image_embed_assemble_slots
    asm.argtypes, asm.restype = [vp] * 10 + [i32] * 8 + [vp], i32
    # (proj, cls, pos0, pos_grid, patch_mask, attention_mask, modality1, h, key_mask, overflow, B, Lt, gh, gw, max_patches, g, H,
    #  nrep, stream); attention_mask, key_mask and overflow are optional
    ok = [X, X, X, X, X, None, X, X, None, None]
    for k in (0, 1, 2, 3, 4, 6, 7):
        ptrs = list(ok)
        ptrs[k] = None
        assert asm(*ptrs, 3, 3, 3, 5, 6, 12, 64, 1, None) == EINVAL, k
    assert asm(*ok, 3, 3, 3, 5, 0, 12, 64, 1, None) == EINVAL                 # max_patches < 1
    assert asm(*ok, 3, 3, 3, 5, 16, 12, 64, 1, None) == EINVAL                # max_patches > gh * gw
    assert asm(*ok, 3, 3, 3, 5, 6, 12, 66, 1, None) == EINVAL                 # H % 4 != 0
    assert asm(*ok, 0, 3, 3, 5, 6, 12, 64, 1, None) == EINVAL                 # B < 1
    assert asm(*ok, 3, 3, 3, 5, 6, 12, 64, 0, None) == EINVAL                 # nrep < 1
    assert asm(*ok, 3, 3, 65, 5, 6, 12, 64, 1, None) == EINVAL                # more than 64 cell rows


def test_slot_kernels_need_a_device():
    """Host tensors are refused: there is no CPU path."""
    pm = torch.ones(3, 3, 5, dtype=torch.int64)
    with pytest.raises(L.FeddatHipError):
        L.im2col_patches_slots(torch.zeros(3, 3, 96, 160), pm, torch.zeros(18, 3072, dtype=torch.float16), 3, 3, 3, 96, 160, 32, 6)
    z = torch.zeros(64)
    with pytest.raises(L.FeddatHipError):
        L.image_embed_assemble_slots(torch.zeros(18, 64), z, z, torch.zeros(144, 64), pm, None, z, torch.zeros(3, 10, 64),
                                     torch.zeros(3, 10, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), 3, 3, 3, 5, 6, 12, 64)


def test_main_refuses_the_flags_for_albef_and_long_sequences():
    from feddat_amd import train
    for flags in (["--image_frame", "384,384"], ["--max_image_patches", "84"], ["--synthetic_orientations"]):
        with pytest.raises(L.FeddatHipError, match="ViLT options"):
            train.main(["--encoder_name", "albef_no_distill"] + flags)
    with pytest.raises(L.FeddatHipError, match="at most 320"):      # 40 + 1 + 280 = 321
        train.main(["--image_frame", "640,640", "--max_image_patches", "280"])
    with pytest.raises(L.FeddatHipError, match="must lie in 1 .. 144"):
        train.main(["--max_image_patches", "145"])
    with pytest.raises(L.FeddatHipError, match="must lie in 1 .. 144"):
        train.main(["--max_image_patches", "0"])
    with pytest.raises(L.FeddatHipError, match="multiples of 32"):
        train.main(["--image_frame", "384,400"])
    with pytest.raises(L.FeddatHipError, match="multiples of 32"):
        train.main(["--image_frame", "384"])


def test_engines_refuse_fp8_and_bad_slot_counts():
    from feddat_amd.adapter_engine import ViltAdapterEngine
    from feddat_amd.engine import ViltDatEngine
    from feddat_amd.vector_engine import ViltVectorEngine
    with pytest.raises(L.FeddatHipError, match="grid frame only"):
        ViltDatEngine({}, ["art"], "cpu", 2, 224, fp8=True, max_patches=20)
    with pytest.raises(L.FeddatHipError):
        ViltAdapterEngine({}, ["art"], "cpu", 2, 224, fp8=True, max_patches=20)
    with pytest.raises(L.FeddatHipError):
        ViltVectorEngine({}, ["art"], "cpu", 2, 224, mode="bias", fp8=True, max_patches=20)
    for make in (ViltDatEngine, ViltAdapterEngine, lambda *a, **k: ViltVectorEngine(*a, mode="norm", **k)):
        with pytest.raises(L.FeddatHipError, match="must lie in 1 .. 49"):
            make({}, ["art"], "cpu", 2, 224, max_patches=0)
        with pytest.raises(L.FeddatHipError, match="must lie in 1 .. 49"):
            make({}, ["art"], "cpu", 2, 224, max_patches=50)
        with pytest.raises(L.FeddatHipError, match="at most 320"):      # 40 + 1 + 280
            make({}, ["art"], "cpu", 2, (640, 640), max_patches=280)
