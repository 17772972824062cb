"""Host-side pieces of the device image path (no GPU): the restatement tests/image_path_ref.py against Pillow itself and against the
fixture tests/golden/gi1_image_path.npz (written from Pillow by tools/make_image_path_golden.py); torchvision's size rule; the four
entry points (include/feddat_hip.h: feddat_image_resample_u8, feddat_albef_image_preprocess and their workspace functions) are
declared, exported, bound and check their arguments; the wrappers raise without a device; train.main's new option."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from feddat_amd import lib as L
from oracle import image_oracle as IO
from tests import image_path_ref as R
from tests.golden_util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("feddat_image_resample_workspace_bytes", "feddat_image_resample_u8", "feddat_albef_image_workspace_bytes",
               "feddat_albef_image_preprocess")
EINVAL = 1


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load(golden_dir, "gi1_image_path.npz")


def _ref_case(name):
    par, _ = R.CASES[name]
    imgs = R.case_images(name)
    s1 = [R.dataset_resize(im, par["size"], par["max_size"]) for im in imgs]
    both = [R.to_tensor_normalize(IO.pil_bicubic_resize(im, par["R"], par["R"])) for im in s1]
    return imgs, s1, both


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_matches_the_fixture(golden, name):
    _, s1, both = _ref_case(name)
    assert np.array_equal(np.array([im.shape[:2] for im in s1], np.int32), golden[f"{name}.s1_shape"])
    assert [R.crc(im) for im in s1] == golden[f"{name}.s1_crc"].tolist()
    assert [R.crc(t) for t in both] == golden[f"{name}.both_crc"].tolist()
    if name == "small":
        for i in R.STORED:
            assert np.array_equal(s1[i], golden[f"small.{i}.s1"]) and np.array_equal(both[i], golden[f"small.{i}.both"])
            assert both[i].dtype == np.float32 and both[i].shape == (3, 64, 64)


def test_restatement_matches_the_fixture_stage2_and_heavy(golden):
    got = [R.crc(R.albef_transform(im, R.SMALL["R"], dataset_resize_first=False)) for im in R.case_images("stage2")]
    assert got == golden["stage2.crc"].tolist()
    assert R.bilinear_coeffs(1600, 64)[1].shape[1] == 51          # the heavy down-scale's tap count
    assert R.crc(R.pil_bilinear_resize(R.case_images("heavy")[0], *R.HEAVY[1])) == int(golden["heavy.crc"][0])


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_matches_pillow_live(name):
    Image = pytest.importorskip("PIL.Image")
    par, _ = R.CASES[name]
    imgs, s1, both = _ref_case(name)
    for im, a, b in zip(imgs, s1, both):
        nh, nw = R.dataset_resize_size(im.shape[0], im.shape[1], par["size"], par["max_size"])
        p = im if (nh, nw) == im.shape[:2] else np.asarray(Image.fromarray(im).resize((nw, nh), resample=Image.BILINEAR))
        assert np.array_equal(a, p), im.shape
        q = np.asarray(Image.fromarray(p).resize((par["R"], par["R"]), resample=Image.BICUBIC))
        assert np.array_equal(b, R.to_tensor_normalize(q)), im.shape


def test_restatement_matches_pillow_live_upscale_identity_and_heavy():
    Image = pytest.importorskip("PIL.Image")
    (src, (oh, ow)) = R.HEAVY
    cases = [(R.case_images("heavy")[0], oh, ow)]
    for im in IO.synthetic_images([(30, 50), (64, 20), (1, 9), (9, 1)], seed=4):
        cases += [(im, 64, 64), (im, im.shape[0], 77), (im, 45, im.shape[1])]      # up-scales; one axis unchanged
    for im, h, w in cases:
        p = np.asarray(Image.fromarray(im).resize((w, h), resample=Image.BILINEAR))
        assert np.array_equal(R.pil_bilinear_resize(im, h, w), p), (im.shape, h, w)
    # the unit-scale tables are the identity for both filters: what lets the kernels run the pass Pillow skips
    for n in (1, 2, 7, 64):
        for bounds, kk in (R.bilinear_coeffs(n, n), IO.precompute_coeffs(n, n)):
            for xx in range(n):
                xmin, cnt = bounds[xx]
                row = np.zeros(n, np.int64)
                row[xmin:xmin + cnt] = kk[xx, :cnt]
                assert row[xx] == 1 << R.PRECISION_BITS and row.sum() == 1 << R.PRECISION_BITS


SIZE_RULE = [  # (h, w) -> (new_h, new_w) at size = 384, max_size = 640
    ((480, 640), (384, 512)), ((640, 480), (512, 384)),            # both orientations
    ((384, 1000), (384, 1000)), ((1000, 384), (1000, 384)),        # short == size: unchanged even with long > max_size
    ((384, 384), (384, 384)),
    ((400, 1000), (256, 640)), ((1000, 400), (640, 256)),          # the cap: int(640 * 384 / 960)
    ((333, 500), (384, 576)), ((500, 333), (576, 384)),            # truncation: int(384 * 500 / 333) = 576 (576.58)
    ((427, 640), (384, 575)), ((640, 427), (575, 384)),            # int(384 * 640 / 427) = 575 (575.55)
    ((600, 800), (384, 512)), ((100, 150), (384, 576)),            # an up-scale
    ((1, 40), (16, 640)), ((375, 500), (384, 512)),
]


@pytest.mark.parametrize("src,want", SIZE_RULE)
def test_size_rule_table(src, want):
    from feddat_amd.image_processing import dataset_resize_size
    assert dataset_resize_size(*src) == want == R.dataset_resize_size(*src)


def test_size_rule_scaled_down_and_against_pillow_sizes():
    from feddat_amd.image_processing import dataset_resize_size
    want = {(50, 70): (64, 89), (23, 37): (60, 96), (64, 200): (64, 200), (7, 200): (3, 96), (1, 40): (2, 96), (96, 64): (96, 64),
            (300, 90): (96, 28)}
    for src in R.SMALL_SOURCES:
        assert dataset_resize_size(*src, size=64, max_size=96) == want[src] == R.dataset_resize_size(*src, 64, 96), src
    rng = np.random.default_rng(0)
    for _ in range(2000):          # the product's rule and the restatement agree everywhere
        h, w = int(rng.integers(1, 3000)), int(rng.integers(1, 3000))
        assert dataset_resize_size(h, w) == R.dataset_resize_size(h, w)


@pytest.mark.parametrize("f16", [False, True])
def test_new_symbols_declared_exported_bound_and_checked(f16):
    """Every refusal below happens in the argument checks: the pointers are never dereferenced and no kernel is launched."""
    from feddat_amd import build
    src = open(os.path.join(ROOT, "include", "feddat_hip.h")).read()
    lib = ctypes.CDLL(build.build(f16=f16))
    for n in NEW_SYMBOLS:
        ret = "long" if n.endswith("_workspace_bytes") else "int"
        assert re.search(rf"^{ret} {n}\(", src, flags=re.M), n
        assert n in L.EXPORTED_SYMBOLS and hasattr(lib, n), n
        getattr(lib, n).argtypes = L._SIGS[n]
        getattr(lib, n).restype = ctypes.c_long if ret == "long" else ctypes.c_int
    assert re.search(r"^#define FEDDAT_FILTER_BILINEAR 2\b", src, flags=re.M) and L.FILTER_BILINEAR == 2
    assert re.search(r"^#define FEDDAT_FILTER_BICUBIC 3\b", src, flags=re.M) and L.FILTER_BICUBIC == 3
    assert lib.feddat_abi_version() == 8 == L.ABI_VERSION
    assert len(L.EXPORTED_SYMBOLS) == 115
    i32 = lambda *v: np.array(v, np.int32)          # noqa: E731
    i64 = lambda *v: np.array(v, np.int64)          # noqa: E731
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    h, w, oh, ow, off = i32(50, 7), i32(70, 200), i32(64, 3), i32(89, 96), i64(0, 10500)
    wsb = lib.feddat_image_resample_workspace_bytes
    assert wsb(p(h), p(w), p(oh), p(ow), 2, 2) > 0 and wsb(p(h), p(w), p(oh), p(ow), 2, 3) > wsb(p(h), p(w), p(oh), p(ow), 2, 2)
    for bad in ((None, p(w), p(oh), p(ow), 2, 2), (p(h), p(w), p(oh), p(ow), 0, 2), (p(h), p(w), p(oh), p(ow), 2, 1),
                (p(h), p(w), p(oh), p(ow), 2, 4), (p(i32(50, 0)), p(w), p(oh), p(ow), 2, 2),
                (p(h), p(w), p(oh), p(i32(89, -1)), 2, 2)):
        assert wsb(*bad) == -1, bad
    # the workspace: per image the [h][ow][3] intermediate and two tables of [out][2 + ksize] int32, each rounded up to 16 bytes
    al = lambda v: (v + 15) & ~15                    # noqa: E731
    want = sum(al(hh * o_w * 3) + al(o_w * (2 + R.bilinear_coeffs(ww, o_w)[1].shape[1]) * 4)
               + al(o_h * (2 + R.bilinear_coeffs(hh, o_h)[1].shape[1]) * 4) for hh, ww, o_h, o_w in zip(h, w, oh, ow))
    assert wsb(p(h), p(w), p(oh), p(ow), 2, 2) == want
    X = 0x1000                                      # never dereferenced
    rs = lib.feddat_image_resample_u8
    need = wsb(p(h), p(w), p(oh), p(ow), 2, 2)
    ok = [X, p(off), p(h), p(w), p(oh), p(ow), p(off), 2, 2, X, X, need, None]
    for i in (0, 1, 2, 3, 4, 5, 6, 9, 10):
        assert rs(*[None if j == i else a for j, a in enumerate(ok)]) == EINVAL, i
    for i, v in ((7, 0), (8, 1), (8, 0), (11, need - 1), (1, p(i64(0, -1))), (6, p(i64(-5, 0))), (4, p(i32(64, 0)))):
        assert rs(*[v if j == i else a for j, a in enumerate(ok)]) == EINVAL, (i, v)
    awb, ap = lib.feddat_albef_image_workspace_bytes, lib.feddat_albef_image_preprocess
    assert awb(p(h), p(w), 2, 64) == lib.feddat_vilt_image_workspace_bytes(p(h), p(w), p(i32(64, 64)), p(i32(64, 64)), 2)
    for bad in ((None, p(w), 2, 64), (p(h), None, 2, 64), (p(h), p(w), 0, 64), (p(h), p(w), 2, 0), (p(i32(0, 1)), p(w), 2, 64)):
        assert awb(*bad) == -1, bad
    mean, std = np.array(R.ALBEF_MEAN, np.float32), np.array(R.ALBEF_STD, np.float32)
    need = awb(p(h), p(w), 2, 64)
    ok = [X, p(off), p(h), p(w), 2, 64, p(mean), p(std), X, X, need, None]
    for i in (0, 1, 2, 3, 6, 7, 8, 9):
        assert ap(*[None if j == i else a for j, a in enumerate(ok)]) == EINVAL, i
    zero_std = np.array([0.5, 0.0, 0.5], np.float32)
    for i, v in ((4, 0), (5, 0), (10, need - 1), (7, p(zero_std)), (1, p(i64(0, -1))), (2, p(i32(50, 0)))):
        assert ap(*[v if j == i else a for j, a in enumerate(ok)]) == EINVAL, (i, v)


def test_image_ops_need_a_device():
    """CPU tensors are refused before the library is touched: there is no host path."""
    buf = torch.zeros(50 * 70 * 3 + 64 * 89 * 3, dtype=torch.uint8)
    with pytest.raises(L.FeddatHipError, match="no CPU path"):
        L.image_resample_u8(buf, [0], [50], [70], [64], [89], buf, [10500])
    with pytest.raises(L.FeddatHipError, match="no CPU path"):
        L.albef_image_preprocess(buf, [0], [50], [70], torch.zeros(1, 3, 64, 64), R.ALBEF_MEAN, R.ALBEF_STD)


def test_transforms_refuse_what_is_not_a_decoded_image_before_any_device():
    from feddat_amd import image_processing as IP
    words = "images must be decoded RGB uint8 arrays of shape \\[H, W, 3\\]"
    for bad in ([np.zeros((8, 8, 3), np.float32)], [np.zeros((8, 8), np.uint8)], [np.zeros((8, 8, 4), np.uint8)],
                [torch.zeros(3, 8, 8, dtype=torch.uint8)], []):
        with pytest.raises(L.FeddatHipError, match=words):
            IP.decoded_images(bad)
    ok = IP.decoded_images([np.zeros((8, 9, 3), np.uint8), torch.zeros(4, 5, 3, dtype=torch.uint8)])
    assert [a.shape for a in ok] == [(8, 9, 3), (4, 5, 3)]
    assert IP.ALBEF_MEAN == R.ALBEF_MEAN and IP.ALBEF_STD == R.ALBEF_STD


def test_main_refuses_raw_images_for_vilt_before_any_device():
    from feddat_amd import train
    with pytest.raises(L.FeddatHipError, match="dataset_resize=True"):
        train.main(["--encoder_name", "vilt", "--synthetic_raw_images"])
    p = train.build_parser()
    base, on = vars(p.parse_args([])), vars(p.parse_args(["--synthetic_raw_images"]))
    assert base["synthetic_raw_images"] is False and on["synthetic_raw_images"] is True
    assert {k: v for k, v in base.items() if k != "synthetic_raw_images"} == \
        {k: v for k, v in on.items() if k != "synthetic_raw_images"}


def test_synthetic_raw_images_are_seeded_and_mixed():
    from feddat_amd import albef_spec
    a, b = albef_spec.synthetic_raw_images(12, 5, image=64), albef_spec.synthetic_raw_images(12, 5, image=64)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(a, albef_spec.synthetic_raw_images(12, 6, image=64)))
    assert all(x.dtype == np.uint8 and x.ndim == 3 and x.shape[2] == 3 for x in a)
    shapes = {x.shape[:2] for x in a}
    assert any(h > w for h, w in shapes) and any(h < w for h, w in shapes) and len(shapes) >= 3
    assert {x.shape[:2] for x in albef_spec.synthetic_raw_images(40, 1)} <= {(480, 640), (640, 427), (384, 384), (427, 640), (240, 320)}
