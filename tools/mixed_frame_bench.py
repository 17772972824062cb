"""What the patch-slot frame costs next to the grid frame, in one process on one GPU: the 12-layer B = 32 DAT train_step (default
fp16 engine, hipGraph replay) on
  grid    ViltDatEngine(res=(384, 640)):                    landscape-only batches, S = 40 + 1 + 240 = 281;
  slots   ViltDatEngine(res=(640, 640), max_patches=240):   the same landscape images zero-extended to the square frame (S = 281),
          and a half-portrait batch (even samples 384 x 640, odd samples 640 x 384), which only this frame can run.
Both run the same sequence length, so the difference is set_batch (the slot gather reads the masks and writes only the slot
patches of a 640 x 640 frame; im2col walks the whole 384 x 640 frame) and the slot assembly.  Two figures per case: the captured
step alone (replay on the staged batch) and set_batch + step on a device-resident batch; five repetitions of ten steps each, the
cases interleaved, HIP events around each repetition.
python tools/mixed_frame_bench.py [--layers N] [--batch B]     (figures: DESIGN.md section 17)"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from feddat_amd import engine, vilt_spec

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=12)
ap.add_argument("--batch", type=int, default=32)
args = ap.parse_args()
dev = torch.device("cuda", 0)
B, NL = args.batch, args.layers
REPS, STEPS = 5, 10


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n       # ms per call


def batch(seed, frame, valid):
    """A device-resident batch in `frame` whose sample b holds N(0, 1) pixels in its top-left valid[b % len(valid)] rectangle."""
    b = vilt_spec.synthetic_batch(B, 32, seed, device=dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    px = torch.zeros(B, 3, frame[0], frame[1], device=dev)
    pm = torch.zeros(B, frame[0], frame[1], dtype=torch.long, device=dev)
    for i in range(B):
        h, w = valid[i % len(valid)]
        px[i, :, :h, :w] = torch.randn(3, h, w, generator=g, device=dev)
        pm[i, :h, :w] = 1
    b["pixel_values"], b["pixel_mask"] = px, pm
    return b


def make(res, **kw):
    e = engine.ViltDatEngine(vilt_spec.random_init(NL, ["c0"], seed=0), ["c0"], dev, batch=B, res=res, layers=NL, **kw)
    e.begin_local_update("c0", steps_per_epoch=80)
    return e


LAND, PORT = (384, 640), (640, 384)
grid, slots = make(LAND), make((640, 640), max_patches=240)
cases = {
    "grid 384x640, landscape": (grid, [batch(1234 + i, LAND, [LAND]) for i in range(4)]),
    "slots 640x640 / 240, landscape": (slots, [batch(1234 + i, (640, 640), [LAND]) for i in range(4)]),
    "slots 640x640 / 240, half portrait": (slots, [batch(1234 + i, (640, 640), [LAND, PORT]) for i in range(4)]),
}
print(torch.cuda.get_device_name(0), f"-- DAT train_step, {NL} layers, B = {B}, fp16 operands, hipGraph; S = {grid.S} / {slots.S}")
assert grid.S == slots.S == 281
for e, bs in cases.values():      # warm-up: capture, every batch once
    for b in bs:
        e.train_step(b, use_graph=True)
torch.cuda.synchronize()
replay, staged = {n: [] for n in cases}, {n: [] for n in cases}
for _ in range(REPS):
    for n, (e, bs) in cases.items():
        e.set_batch(bs[0])
        replay[n].append(timed(lambda i: e.train_step(None, use_graph=True), STEPS))
        staged[n].append(timed(lambda i: e.train_step(bs[i % 4], use_graph=True), STEPS))
for n, (e, _) in cases.items():
    e.assert_finite()
    r, s = replay[n], staged[n]
    print(f"{n:38s} step alone: median {statistics.median(r):7.3f} ms (min {min(r):7.3f}, max {max(r):7.3f})   "
          f"set_batch + step: median {statistics.median(s):7.3f} ms (min {min(s):7.3f}, max {max(s):7.3f})")
