#!/usr/bin/env python
"""Throughput of the prompt-tuning step (optimizer_mode prompt, feddat_amd.prompt_engine, S = 195) next to the bias-only step
(feddat_amd.vector_engine, S = 185), both at configs[1]'s size (B = 32, 384 x 384, 12 layers, f16 operands, dynamic loss scale),
in one process and alternated: each engine is warmed up and its hipGraph captured, then R rounds of K replays each, timed with
device events.
python tools/prompt_step_bench.py [--steps K] [--rounds R]  -> one JSON line (medians of the R rounds and every round's value).
--eager-once: instead, run ONE eager step per mode after the warm-up (for a kernel trace of its own: the profiler names the
kernels of an eager step, a graph replay is one opaque launch)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feddat_amd import vilt_spec  # noqa: E402
from feddat_amd.prompt_engine import ViltPromptEngine  # noqa: E402
from feddat_amd.vector_engine import ViltVectorEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--eager-once", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, res, layers = 32, 384, 12
    batches = [vilt_spec.synthetic_batch(B, res, 1234 + i, device=dev) for i in range(4)]
    engs = {
        "bias": ViltVectorEngine(vilt_spec.random_init(layers, ["c0"], seed=0, optimizer_mode="bias"), ["c0"], dev, batch=B,
                                 res=res, layers=layers, mode="bias"),
        "prompt": ViltPromptEngine(vilt_spec.random_init(layers, ["c0"], seed=0, optimizer_mode="prompt"), ["c0"], dev, batch=B,
                                   res=res, layers=layers)}
    total = (a.warmup + a.rounds * a.steps) * 15
    for e in engs.values():
        e.begin_local_update("c0", steps_per_epoch=total)
        e.set_batch(batches[0])
        if a.eager_once:
            for i in range(a.warmup):
                e.train_step(batches[i % 4], use_graph=False)
            continue
        e.ensure_captured()
        for i in range(a.warmup):
            e.train_step(batches[i % 4], use_graph=True)
    torch.cuda.synchronize()
    if a.eager_once:
        print(json.dumps({k: float(e.train_step(batches[0], use_graph=False)[0]) for k, e in engs.items()}))
        torch.cuda.synchronize()
        return
    ms = {k: [] for k in engs}
    for r in range(a.rounds):
        for k, e in engs.items():
            e.set_batch(batches[r % 4])
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                e.graph.replay()
            t1.record()
            torch.cuda.synchronize()
            ms[k].append(t0.elapsed_time(t1) / a.steps)
    out = {}
    for k, v in ms.items():
        med = sorted(v)[len(v) // 2]
        out[k] = dict(seq=engs[k].S, ms_per_step=round(med, 4), samples_per_s=round(B / med * 1e3, 1), min_ms=round(min(v), 4),
                      max_ms=round(max(v), 4), rounds_ms=[round(x, 4) for x in v])
    out["ratio_prompt_over_bias"] = round(out["prompt"]["ms_per_step"] / out["bias"]["ms_per_step"], 4)
    out["seq_ratio"] = round(engs["prompt"].S / engs["bias"].S, 4)
    for k, e in engs.items():
        e.assert_finite()
        out[k]["skipped_batches"] = e.scaler_state()["skipped_batches"]
        out[k]["comm_bytes"] = e.comm_flat().numel() * 4
    print(json.dumps(dict(config="B=32 384x384 12 layers f16", steps=a.steps, rounds=a.rounds, **out)))


if __name__ == "__main__":
    main()
