"""Cost of training the ALBEF LM head (AlbefDatEngine(train_lm_head=True)): the full-size B = 32 ALBEF train_step (ViT-B/16 at
384, BERT-base 12 + 6 layers, vocabulary 30 522, one 4-token answer per question; default operand format, dropout 0) with the
option off and on, in the same process on the same box.  hipGraph replay; per engine 5 repeats of 10 steps, the median repeat's
ms / step.  The two engines are timed in turn, repeat by repeat, so that drift of the box hits both alike.  Prints one JSON line.

    python tools/albef_head_bench.py [--batch 32] [--repeats 5] [--steps 10]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feddat_amd import albef_engine, albef_spec  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
args = ap.parse_args()
B = args.batch
params = albef_spec.random_init(seed=0, image=384)
batches = [albef_spec.synthetic_batch(B, 1234 + i, image=384, device="cuda") for i in range(2)]
engines = {}
for name, on in (("off", False), ("on", True)):
    eng = albef_engine.AlbefDatEngine(params, "cuda", batch=B, n_answers=B, image=384, train_lm_head=on)
    eng.begin_local_update(steps_per_epoch=1000)
    for i in range(5):          # capture + warm-up
        eng.train_step(batches[i % 2], use_graph=True)
    torch.cuda.synchronize()
    engines[name] = eng
times = {name: [] for name in engines}
for _ in range(args.repeats):
    for name, eng in engines.items():
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(args.steps):
            eng.train_step(batches[i % 2], use_graph=True)
        torch.cuda.synchronize()
        times[name].append((time.perf_counter() - t) / args.steps * 1e3)
off, on = statistics.median(times["off"]), statistics.median(times["on"])
for eng in engines.values():
    eng.assert_finite()
print(json.dumps({"tool": "albef_head_bench", "batch": B, "repeats": args.repeats, "steps": args.steps,
                  "ms_per_step_off": round(off, 3), "ms_per_step_on": round(on, 3), "on_over_off": round(on / off, 4),
                  "all_off": [round(x, 3) for x in times["off"]], "all_on": [round(x, 3) for x in times["on"]],
                  "lm_rows": engines["on"].R, "head_floats": engines["on"].lm.numel}))
