#!/usr/bin/env python
"""Throughput of the single-adapter step (optimizer_mode adapter, feddat_amd.adapter_engine) next to the DAT step, both at
configs[1]'s size (B = 32, 384 x 384, 12 layers, f16 operands, dynamic loss scale), in one process and alternated: each
engine is warmed up and its hipGraph captured, then R rounds of K replays each, timed with device events.
Fraction of the MFMA peak at 6.548e10 FLOP per sample for the adapter step (SURVEY: fwd_single 3.3698e10 + bwd_single
3.1782e10).  python tools/adapter_step_bench.py [--steps K] [--rounds R]  -> one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feddat_amd import engine, vilt_spec  # noqa: E402
from feddat_amd.adapter_engine import ViltAdapterEngine  # noqa: E402

PEAK = 2.5e15                  # dense 16-bit MFMA peak of gfx950
FLOP_ADAPTER = 6.548e10        # per sample: single-adapter forward + backward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, res, layers = 32, 384, 12
    batches = [vilt_spec.synthetic_batch(B, res, 1234 + i, device=dev) for i in range(4)]
    engs = {"adapter": ViltAdapterEngine(vilt_spec.random_init(layers, ["c0"], seed=0, optimizer_mode="adapter"), ["c0"], dev,
                                         batch=B, res=res, layers=layers),
            "dat": engine.ViltDatEngine(vilt_spec.random_init(layers, ["c0"], seed=0), ["c0"], dev, batch=B, res=res,
                                        layers=layers)}
    total = (a.warmup + a.rounds * a.steps) * 15
    for e in engs.values():
        e.begin_local_update("c0", steps_per_epoch=total)
        e.set_batch(batches[0])
        e.ensure_captured()
        for i in range(a.warmup):
            e.train_step(batches[i % 4], use_graph=True)
    torch.cuda.synchronize()
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
        out[k] = dict(ms_per_step=round(med, 4), samples_per_s=round(B / med * 1e3, 1), rounds_ms=[round(x, 4) for x in v])
    out["adapter"]["mfma_peak_fraction"] = round(FLOP_ADAPTER * B / (out["adapter"]["ms_per_step"] * 1e-3) / PEAK, 4)
    out["ratio_adapter_over_dat"] = round(out["adapter"]["ms_per_step"] / out["dat"]["ms_per_step"], 4)
    for k, e in engs.items():
        e.assert_finite()
        out[k]["skipped_batches"] = e.scaler_state()["skipped_batches"]
    print(json.dumps(dict(config="B=32 384x384 12 layers f16", steps=a.steps, rounds=a.rounds, **out)))


if __name__ == "__main__":
    main()
