"""Device-side mirror of the image half of the reference's input pipeline: HF `ViltImageProcessor` as called by
`ViltEncoderWrapper.process_inputs` (src/modeling/vilt.py:87-100; ViltProcessor(images=..., return_tensors='pt')).

    proc = ViltImageProcessor(device)
    enc = proc(images)          # list of [H, W, 3] uint8 arrays / tensors (decoded RGB) -> {'pixel_values', 'pixel_mask'}

Same defaults (shorter edge 384, longer <= 640, size_divisor 32, PIL BICUBIC, 1/255, mean = std = 0.5, zero padding) and
the same output dict, produced by `feddat_vilt_image_preprocess` (bit-exact with Pillow + transformers); the reference
runs this on the host three times per batch.  The text half (BertTokenizerFast WordPiece) needs the vocabulary file the
reference loads from ./models/bert-base-uncased and stays with the caller.

The two stages the reference runs around that processor are here as well:

    resize = DatasetResize(device)              # the image datasets' T.Resize(size=384, max_size=640), PIL BILINEAR
    packed = resize(images)                     # (cocoimages_dataset_crossvqas.py:83,108-109) -> PackedImages on the device
    enc = proc(packed)                          # ViLT: stage 1 -> the processor, without leaving the device
    x = AlbefImageTransform(device)(images)     # ALBEF: stage 1 -> Resize((384, 384), BICUBIC), ToTensor, Normalize
                                                # (vqa_dataset_crossvqa.py:533-572) -> [n, 3, 384, 384] float32"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import lib as L

MAX_SHORTER, MAX_LONGER = 800, 1333


def resize_output_size(h: int, w: int, shorter: int = 384, size_divisor: int = 32):
    """transformers' get_resize_output_image_size for ViLT (python float arithmetic, int(x + 0.5), floor to divisor)."""
    longer = int(MAX_LONGER / MAX_SHORTER * shorter)
    scale = shorter / min(h, w)
    if h < w:
        nh, nw = shorter, scale * w
    else:
        nh, nw = scale * h, shorter
    if max(nh, nw) > longer:
        scale = longer / max(nh, nw)
        nh, nw = scale * nh, scale * nw
    nh, nw = int(nh + 0.5), int(nw + 0.5)
    return nh // size_divisor * size_divisor, nw // size_divisor * size_divisor


# vqa_dataset_crossvqa.py:533-572: T.Normalize of the ALBEF transform (the CLIP statistics)
ALBEF_MEAN = (0.48145466, 0.4578275, 0.40821073)
ALBEF_STD = (0.26862954, 0.26130258, 0.27577711)


def dataset_resize_size(h: int, w: int, size: int = 384, max_size: int = 640):
    """(h, w) -> (new_h, new_w) of torchvision 0.11.3's Resize(size, max_size=max_size) on a PIL image (the version the
    reference pins, requirements.txt:3): restated from transforms/functional_pil.py `resize` by reading it -- torchvision is
    not a dependency here.  Python int arithmetic with true division and truncation, as there.  An image whose shorter side
    already equals `size` comes back unchanged even when its longer side exceeds max_size (that version's behaviour)."""
    short, long = (w, h) if w <= h else (h, w)
    if short == size:
        return h, w
    new_short, new_long = size, int(size * long / short)
    if new_long > max_size:
        new_short, new_long = int(max_size * new_short / new_long), max_size
    new_w, new_h = (new_short, new_long) if w <= h else (new_long, new_short)
    return new_h, new_w


class PackedImages:
    """n decoded images in one uint8 device buffer: image i is [heights[i]][widths[i]][3] at byte offsets[i] of `data`
    (host int arrays).  What DatasetResize returns and ViltImageProcessor / AlbefImageTransform take."""

    def __init__(self, data: torch.Tensor, offsets, heights, widths):
        self.data = data
        self.offsets = np.ascontiguousarray(offsets, np.int64)
        self.heights = np.ascontiguousarray(heights, np.int32)
        self.widths = np.ascontiguousarray(widths, np.int32)

    def __len__(self):
        return int(self.heights.shape[0])

    def image(self, i: int) -> torch.Tensor:
        """[h, w, 3] uint8 view of image i."""
        h, w, o = int(self.heights[i]), int(self.widths[i]), int(self.offsets[i])
        return self.data[o:o + h * w * 3].view(h, w, 3)


def decoded_images(images: Sequence) -> List[np.ndarray]:
    """uint8 [H, W, 3] arrays / tensors / PIL images -> contiguous host arrays; anything else is refused."""
    arrs: List[np.ndarray] = []
    for im in images:
        if hasattr(im, "convert"):            # a PIL image (the datasets' image.convert('RGB'))
            im = im.convert("RGB")
        a = im.cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise L.FeddatHipError("images must be decoded RGB uint8 arrays of shape [H, W, 3]")
        arrs.append(np.ascontiguousarray(a))
    if not arrs:
        raise L.FeddatHipError("images must be decoded RGB uint8 arrays of shape [H, W, 3] (got an empty list)")
    return arrs


def pack_images(images: Sequence, device, reserve: int = 0) -> PackedImages:
    """One packed host buffer, one H2D copy; `reserve` more bytes are left free behind the images."""
    arrs = decoded_images(images)
    sizes = np.array([a.size for a in arrs], np.int64)
    offs = np.zeros(len(arrs), np.int64)
    offs[1:] = np.cumsum(sizes)[:-1]
    host = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs]))
    if reserve:
        data = torch.empty(host.numel() + int(reserve), dtype=torch.uint8, device=device)
        data[:host.numel()].copy_(host, non_blocking=True)
    else:
        data = host.to(device, non_blocking=True)
    return PackedImages(data, offs, [a.shape[0] for a in arrs], [a.shape[1] for a in arrs])


class DatasetResize:
    """Stage 1: the image datasets' `pil_transform = T.Resize(size=384, max_size=640)` (cocoimages_dataset_crossvqas.py:83; the
    same line in the VG, VizWiz and COCO datasets), PIL BILINEAR, on the device: feddat_image_resample_u8.

        packed = DatasetResize(device)(images)                    # ALBEF: every image (the datasets' `use_albef` gate, :108)
        packed = DatasetResize(device)(images, larger_only=True)  # ViLT: only images with min(h, w) > size (:108)

    Images the rule leaves as they are (shorter side == size; with larger_only, shorter side <= size) are not resampled:
    their bytes are the uploaded ones.  The only host work is the size arithmetic and the one packed H2D copy."""

    def __init__(self, device, size: int = 384, max_size: int = 640):
        if not 0 < size < max_size:
            raise L.FeddatHipError(f"DatasetResize needs 0 < size < max_size, got {size}, {max_size}")
        L.load()
        self.device = torch.device(device)
        self.size, self.max_size = int(size), int(max_size)
        self._ws = None

    def output_size(self, h: int, w: int, larger_only: bool = False):
        if larger_only and min(h, w) <= self.size:
            return h, w
        oh, ow = dataset_resize_size(h, w, self.size, self.max_size)
        if oh < 1 or ow < 1:          # PIL raises "height and width must be > 0"
            raise L.FeddatHipError(f"a {h}x{w} image resizes to {oh}x{ow}: the reference's Resize refuses it as well")
        return oh, ow

    def __call__(self, images: Sequence, larger_only: bool = False) -> PackedImages:
        arrs = decoded_images(images)
        out = [self.output_size(a.shape[0], a.shape[1], larger_only) for a in arrs]
        move = [i for i, (a, o) in enumerate(zip(arrs, out)) if tuple(a.shape[:2]) != o]
        src = pack_images(arrs, self.device, reserve=sum(out[i][0] * out[i][1] * 3 for i in move))
        if not move:
            return src
        # the results sit behind the sources in the same buffer; an untouched image keeps its offset
        offs, hs, ws = src.offsets.copy(), src.heights.copy(), src.widths.copy()
        end = int(src.offsets[-1]) + arrs[-1].size
        dst = np.zeros(len(move), np.int64)
        for j, i in enumerate(move):
            dst[j] = end
            end += out[i][0] * out[i][1] * 3
        oh, ow = np.array([out[i][0] for i in move], np.int32), np.array([out[i][1] for i in move], np.int32)
        self._ws = L.image_resample_u8(src.data, src.offsets[move], src.heights[move], src.widths[move], oh, ow, src.data, dst,
                                       L.FILTER_BILINEAR, self._ws)
        offs[move], hs[move], ws[move] = dst, oh, ow
        return PackedImages(src.data, offs, hs, ws)


class AlbefImageTransform:
    """Stage 1 + stage 2 of the ALBEF image path, back to back on the current stream:

        T.Resize(384, max_size=640)                       cocoimages_dataset_crossvqas.py:83,108-109 (BILINEAR; DatasetResize)
        T.Resize((384, 384), interpolation=BICUBIC)       vqa_dataset_crossvqa.py:533-572
        T.ToTensor()                                      uint8 HWC -> float32 CHW, x.div(255)
        T.Normalize(ALBEF_MEAN, ALBEF_STD)                x.sub_(mean).div_(std), float32

    transform(images, out=None, dataset_resize=True) -> float32 [n, 3, image, image] on the device; `out` (contiguous, that
    shape) is written in place -- the engine's static image buffer or its first n samples."""

    def __init__(self, device, image: int = 384, mean=ALBEF_MEAN, std=ALBEF_STD, size: int = 384, max_size: int = 640):
        L.load()
        self.device = torch.device(device)
        self.image = int(image)
        self.mean, self.std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
        self.resize = DatasetResize(device, size, max_size)
        self._ws = None

    def __call__(self, images, out: Optional[torch.Tensor] = None, dataset_resize: bool = True) -> torch.Tensor:
        if isinstance(images, PackedImages):
            packed = images
        elif dataset_resize:
            packed = self.resize(images)
        else:
            packed = pack_images(images, self.device)
        n, R = len(packed), self.image
        if out is None:
            out = torch.empty(n, 3, R, R, device=self.device)
        elif tuple(out.shape) != (n, 3, R, R):
            raise L.FeddatHipError(f"{n} images transform to {(n, 3, R, R)}, out is {tuple(out.shape)}")
        self._ws = L.albef_image_preprocess(packed.data, packed.offsets, packed.heights, packed.widths, out, self.mean, self.std,
                                            self._ws)
        return out


class ViltImageProcessor:
    model_input_names = ["pixel_values", "pixel_mask"]

    def __init__(self, device, shortest_edge: int = 384, size_divisor: int = 32, pad_to=None):
        """pad_to=(H, W): pad every batch to a fixed frame (the static shape the engine was built for) instead of the
        batch maximum."""
        L.load()
        self.device = torch.device(device)
        self.shortest_edge, self.size_divisor, self.pad_to = shortest_edge, size_divisor, pad_to
        self._ws = None

    def __call__(self, images: Sequence, return_tensors: str = "pt") -> Dict[str, torch.Tensor]:
        """images: a list of decoded images, or the PackedImages DatasetResize left on the device."""
        pk = images if isinstance(images, PackedImages) else pack_images(images, self.device)
        n, hs, ws, offs, packed = len(pk), pk.heights, pk.widths, pk.offsets, pk.data
        out = [resize_output_size(int(h), int(w), self.shortest_edge, self.size_divisor) for h, w in zip(hs, ws)]
        oh = np.array([o[0] for o in out], np.int32)
        ow = np.array([o[1] for o in out], np.int32)
        Hm, Wm = (int(oh.max()), int(ow.max())) if self.pad_to is None else self.pad_to
        if int(oh.max()) > Hm or int(ow.max()) > Wm:
            raise L.FeddatHipError(f"resized image {int(oh.max())}x{int(ow.max())} exceeds the pad_to frame {Hm}x{Wm}")
        ip = lambda a: a.ctypes.data_as(C.c_void_p)
        need = int(L.load().feddat_vilt_image_workspace_bytes(ip(hs), ip(ws), ip(oh), ip(ow), n))
        if need < 0:
            raise L.FeddatHipError("feddat_vilt_image_workspace_bytes rejected the image sizes")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        px = torch.empty(n, 3, Hm, Wm, device=self.device)
        pm = torch.empty(n, Hm, Wm, dtype=torch.int64, device=self.device)
        rc = L.load().feddat_vilt_image_preprocess(packed.data_ptr(), ip(offs), ip(hs), ip(ws), ip(oh), ip(ow), n, Hm, Wm,
                                                   px.data_ptr(), pm.data_ptr(), self._ws.data_ptr(), self._ws.numel(),
                                                   torch.cuda.current_stream().cuda_stream)
        if rc:
            raise L.FeddatHipError(f"feddat_vilt_image_preprocess failed with code {rc}")
        return {"pixel_values": px, "pixel_mask": pm}
