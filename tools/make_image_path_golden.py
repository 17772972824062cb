"""Writes tests/golden/gi1_image_path.npz: what Pillow itself (Image.resize) produces for the two stages of the reference's image
transform on seeded uint8 images -- the image datasets' bilinear Resize(size, max_size=...) and ALBEF's bicubic Resize((R, R)) +
ToTensor + Normalize (the last two as torch float32 CPU ops on Pillow's bytes).  Per case: the stage-1 shapes, one CRC32 per
image of the stage-1 bytes and of the final float32 tensors, and the full arrays of the two smallest images.  The cases and
their seeds live in tests/image_path_ref.py; nothing of that file's resampling is used here.
Run where Pillow is installed: python tools/make_image_path_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import image_path_ref as R  # noqa: E402


def pil_resize(img, oh, ow, resample):
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((ow, oh), resample=resample))


def pil_stage1(img, size, max_size):
    """torchvision 0.11.3 functional_pil.resize: an image the rule leaves unchanged is returned as it is."""
    from PIL import Image
    h, w = img.shape[:2]
    nh, nw = R.dataset_resize_size(h, w, size, max_size)
    return img if (nh, nw) == (h, w) else pil_resize(img, nh, nw, Image.BILINEAR)


def pil_stage2(img, res):
    from PIL import Image
    return R.to_tensor_normalize(pil_resize(img, res, res, Image.BICUBIC))


def main():
    from PIL import Image
    rec = {}
    for name, (par, _) in R.CASES.items():
        imgs = R.case_images(name)
        s1 = [pil_stage1(im, par["size"], par["max_size"]) for im in imgs]
        both = [pil_stage2(im, par["R"]) for im in s1]
        rec[f"{name}.s1_shape"] = np.array([im.shape[:2] for im in s1], np.int32)
        rec[f"{name}.s1_crc"] = np.array([R.crc(im) for im in s1], np.int64)
        rec[f"{name}.both_crc"] = np.array([R.crc(t) for t in both], np.int64)
        if name == "small":
            for i in R.STORED:
                rec[f"small.{i}.s1"], rec[f"small.{i}.both"] = s1[i], both[i]
        print(name, len(imgs), "images", rec[f"{name}.s1_shape"][:4].tolist())
    rec["stage2.crc"] = np.array([R.crc(pil_stage2(im, R.SMALL["R"])) for im in R.case_images("stage2")], np.int64)
    (oh, ow) = R.HEAVY[1]
    rec["heavy.crc"] = np.array([R.crc(pil_resize(R.case_images("heavy")[0], oh, ow, Image.BILINEAR))], np.int64)
    path = os.path.join(ROOT, "tests", "golden", "gi1_image_path.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
