"""TEST INFRASTRUCTURE ONLY: numpy / torch-CPU restatement of the two image stages the reference runs around the ViLT processor,
and the cases the image-path tests and tools/make_image_path_golden.py share.

Stage 1: the image datasets' torchvision `Resize(size=384, max_size=640)` on the PIL image (cocoimages_dataset_crossvqas.py:83,
108-109), default interpolation BILINEAR: the size rule of torchvision 0.11.3's functional_pil.resize, then Pillow's 8-bit
`ImagingResample` with the triangle filter (support 1.0) -- the same separable, 22-bit fixed-point scheme that
oracle/image_oracle.py restates for the bicubic filter.
Stage 2 (ALBEF, vqa_dataset_crossvqa.py:533-572): `Resize((R, R), BICUBIC)` (oracle.image_oracle.pil_bicubic_resize), `ToTensor`
(float32 x.div(255)) and `Normalize` (float32 x.sub_(mean).div_(std)) as torch float32 ops on the CPU.

Pinned: tests/test_image_path_cpu.py checks this file bit for bit against Pillow itself and against the committed fixture
tests/golden/gi1_image_path.npz, which tools/make_image_path_golden.py wrote from Pillow."""
import math
import zlib

import numpy as np
import torch

from oracle import image_oracle as IO

PRECISION_BITS = IO.PRECISION_BITS
ALBEF_MEAN = (0.48145466, 0.4578275, 0.40821073)
ALBEF_STD = (0.26862954, 0.26130258, 0.27577711)

# scaled-down parameters (the kernels' logic does not depend on the sizes) and the sizes of real use
SMALL = dict(size=64, max_size=96, R=64)
FULL = dict(size=384, max_size=640, R=384)
SMALL_SOURCES = [(50, 70), (23, 37), (64, 200), (7, 200), (1, 40), (96, 64), (300, 90)]


def _many_shapes():
    rng = np.random.default_rng(53)
    return [(int(rng.integers(1, 40)), int(rng.integers(1, 40))) for _ in range(53)]


# name -> (parameters, source shapes): stage 1 and both stages
CASES = {"small": (SMALL, SMALL_SOURCES), "full": (FULL, [(480, 640), (640, 427)]), "vilt": (FULL, [(600, 800)]),
         "many": (SMALL, _many_shapes())}
STAGE2_SOURCES = SMALL_SOURCES + [(64, 64)]          # stage 2 alone; the last one is the identity on both axes
HEAVY = ((400, 1600), (64, 64))                      # one heavy bilinear down-scale: 1600 -> 64 has 51 taps
STORED = (1, 4)                                      # the images of "small" whose arrays the fixture holds in full


def case_images(name):
    shapes = {"stage2": STAGE2_SOURCES, "heavy": [HEAVY[0]]}.get(name) or CASES[name][1]
    return IO.synthetic_images(shapes, seed=zlib.crc32(name.encode()))


def crc(a) -> int:
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def dataset_resize_size(h, w, size=384, max_size=640):
    """torchvision 0.11.3 functional_pil.resize with an int size and max_size: -> (new_h, new_w)."""
    short, long = (w, h) if w <= h else (h, w)
    if short == size:
        return h, w
    new_short, new_long = size, int(size * long / short)
    if new_long > max_size:
        new_short, new_long = int(max_size * new_short / new_long), max_size
    new_w, new_h = (new_short, new_long) if w <= h else (new_long, new_short)
    return new_h, new_w


def _triangle(x: float) -> float:
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


def bilinear_coeffs(in_size: int, out_size: int):
    """Resample.c precompute_coeffs + normalize_coeffs_8bpc for the BILINEAR filter -> (bounds [out, 2], coeffs [out, ksize])."""
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [_triangle((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        for x in range(xmax):
            v = k[x] / ww if ww != 0.0 else k[x]
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _pass(img: np.ndarray, out_size: int) -> np.ndarray:
    """One horizontal bilinear pass over a [rows, in_size, C] uint8 array -> [rows, out_size, C] uint8."""
    rows, in_size, C = img.shape
    bounds, kk = bilinear_coeffs(in_size, out_size)
    out = np.empty((rows, out_size, C), np.uint8)
    src = img.astype(np.int64)
    for xx in range(out_size):
        xmin, n = bounds[xx]
        acc = (1 << (PRECISION_BITS - 1)) + (src[:, xmin:xmin + n, :] * kk[xx, :n, None].astype(np.int64)).sum(1)
        out[:, xx, :] = np.clip(acc.astype(np.int32) >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def pil_bilinear_resize(img: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """== np.asarray(PIL.Image.fromarray(img).resize((out_w, out_h), BILINEAR)): horizontal pass first; an axis whose size does
    not change is skipped."""
    h, w, _ = img.shape
    t = img
    if out_w != w:
        t = _pass(t, out_w)
    if out_h != h:
        t = _pass(t.transpose(1, 0, 2), out_h).transpose(1, 0, 2)
    return np.ascontiguousarray(t)


def dataset_resize(img: np.ndarray, size=384, max_size=640, larger_only=False) -> np.ndarray:
    """Stage 1 on one image; larger_only = the ViLT gate min(h, w) > size (cocoimages_dataset_crossvqas.py:108)."""
    h, w = img.shape[:2]
    if larger_only and min(h, w) <= size:
        return img
    nh, nw = dataset_resize_size(h, w, size, max_size)
    return img if (nh, nw) == (h, w) else pil_bilinear_resize(img, nh, nw)


def to_tensor_normalize(u8: np.ndarray, mean=ALBEF_MEAN, std=ALBEF_STD) -> np.ndarray:
    """ToTensor + Normalize as torchvision writes them, torch float32 on the CPU: [H, W, 3] uint8 -> [3, H, W] float32."""
    x = torch.from_numpy(np.array(u8)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    m = torch.as_tensor(mean, dtype=torch.float32)[:, None, None]
    s = torch.as_tensor(std, dtype=torch.float32)[:, None, None]
    return x.sub_(m).div_(s).numpy()


def albef_transform(img: np.ndarray, R=384, size=384, max_size=640, dataset_resize_first=True) -> np.ndarray:
    """Both ALBEF stages on one image -> [3, R, R] float32."""
    if dataset_resize_first:
        img = dataset_resize(img, size, max_size)
    return to_tensor_normalize(IO.pil_bicubic_resize(img, R, R))
