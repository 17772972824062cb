"""What the device image path costs, on one GPU: B = 32 seeded decoded images of 480 x 640 and of 1000 x 1500,
  albef   stage 1 (bilinear Resize(384, max_size=640)) + stage 2 (bicubic 384 x 384, ToTensor, Normalize);
  vilt    stage 1 + the ViLT processor into the (384, 640) frame;
each as (a) the kernels alone on an uploaded batch, stage by stage (HIP events) and (b) the whole call a trainer makes -- host
packing, the one H2D copy, both stages (host clock around a device synchronise); then the full-size ALBEF train_step (B = 32,
hipGraph) on tensor batches and on raw-image batches (the transform runs outside the captured step), and, where Pillow is
importable, the same batches through Pillow in this one process, for scale.  Medians of 5 repetitions of 10 batches, with
min .. max.
python tools/image_path_bench.py [--batch B] [--skip_step]     (figures: DESIGN.md section 19)"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from feddat_amd import albef_spec, image_processing as IP, lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--skip_step", action="store_true", help="leave out the full-size ALBEF train_step")
args = ap.parse_args()
dev = torch.device("cuda", 0)
B, REPS, STEPS = args.batch, 5, 10
SIZES = [(480, 640), (1000, 1500)]


def images(h, w, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(B)]


def device_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(STEPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / STEPS


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(STEPS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / STEPS


def report(name, xs):
    print(f"  {name:58s} {statistics.median(xs):9.3f} ms / batch   ({min(xs):.3f} .. {max(xs):.3f})", flush=True)


print(torch.cuda.get_device_name(0), f"-- image path, B = {B}, medians of {REPS} x {STEPS} batches")
for h, w in SIZES:
    imgs = images(h, w, 7)
    oh, ow = IP.dataset_resize_size(h, w)
    vh, vw = IP.resize_output_size(oh, ow)
    print(f"{h} x {w} uint8 -> stage 1 {oh} x {ow} -> albef 384 x 384 | vilt {vh} x {vw} in (384, 640)")
    # (a) kernels alone: the batch and the stage-1 results live in one device buffer, as DatasetResize lays them out
    n_src, n_dst = h * w * 3, oh * ow * 3
    buf = torch.empty(B * (n_src + n_dst), dtype=torch.uint8, device=dev)
    buf[:B * n_src].copy_(torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])))
    so, do = np.arange(B, dtype=np.int64) * n_src, B * n_src + np.arange(B, dtype=np.int64) * n_dst
    hs, ws, ohs, ows = (np.full(B, v, np.int32) for v in (h, w, oh, ow))
    out = torch.empty(B, 3, 384, 384, device=dev)
    proc = IP.ViltImageProcessor(dev, pad_to=(384, 640))
    resized = IP.PackedImages(buf, do, ohs, ows)
    state = {"ws": None, "ws2": None}

    def stage1():
        state["ws"] = L.image_resample_u8(buf, so, hs, ws, ohs, ows, buf, do, L.FILTER_BILINEAR, state["ws"])

    def stage2():
        state["ws2"] = L.albef_image_preprocess(buf, do, ohs, ows, out, IP.ALBEF_MEAN, IP.ALBEF_STD, state["ws2"])

    albef_tr, resize = IP.AlbefImageTransform(dev), IP.DatasetResize(dev)
    cases = {"kernels: stage 1 (bilinear)": (device_ms, stage1), "kernels: stage 2 albef (bicubic + normalize)": (device_ms, stage2),
             "kernels: vilt processor on the stage-1 result": (device_ms, lambda: proc(resized)),
             "call: albef transform (pack + H2D + both stages)": (host_ms, lambda: albef_tr(imgs, out=out)),
             "call: vilt stage 1 + processor (pack + H2D + both)": (host_ms, lambda: proc(resize(imgs, larger_only=True)))}
    for _, fn in cases.values():          # warm-up
        fn()
    torch.cuda.synchronize()
    res = {n: [] for n in cases}
    for _ in range(REPS):
        for n, (timer, fn) in cases.items():
            res[n].append(timer(fn))
    for n in cases:
        report(n, res[n])
    try:
        from PIL import Image
    except ImportError:
        print("  Pillow is not importable here: no host figure")
    else:
        m = torch.tensor(IP.ALBEF_MEAN)[:, None, None]
        s = torch.tensor(IP.ALBEF_STD)[:, None, None]

        def pillow_albef():
            for a in imgs:
                im = Image.fromarray(a).resize((ow, oh), resample=Image.BILINEAR).resize((384, 384), resample=Image.BICUBIC)
                torch.from_numpy(np.array(im)).permute(2, 0, 1).contiguous().to(torch.float32).div(255).sub_(m).div_(s)
        xs = []
        for _ in range(3):
            t = time.perf_counter()
            pillow_albef()
            xs.append((time.perf_counter() - t) * 1e3)
        report("host: Pillow + torch CPU, albef chain, 1 process", xs)
    del buf, out

if not args.skip_step:
    from feddat_amd.albef_modeling import create_albef_continual_learner_model
    model = create_albef_continual_learner_model(albef_spec.random_init(seed=0), dev, B, B, operands="f16")
    eng = model.engine
    eng.begin_local_update(steps_per_epoch=80)
    tens = [albef_spec.synthetic_batch(B, 100 + i, device=dev) for i in range(4)]
    raws = [dict(tens[i], image=albef_spec.synthetic_raw_images(B, 100 + i)) for i in range(4)]
    state = {"i": 0}

    def step(batches):
        b = batches[state["i"] % 4]
        state["i"] += 1
        if isinstance(b["image"], list):
            b = model.process_inputs(dict(b, train=True))
        eng.train_step(b, use_graph=True)

    for bs in (tens, raws):               # warm-up: capture, every batch once
        for _ in range(4):
            step(bs)
    torch.cuda.synchronize()
    res = {"tensor batches": [], "raw-image batches (mixed sizes)": []}
    for _ in range(REPS):
        res["tensor batches"].append(host_ms(lambda: step(tens)))
        res["raw-image batches (mixed sizes)"].append(host_ms(lambda: step(raws)))
    print(f"ALBEF train_step, full size, B = {B}, fp16 operands, hipGraph")
    for n, xs in res.items():
        report(n, xs)
