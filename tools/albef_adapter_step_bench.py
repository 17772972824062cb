#!/usr/bin/env python
"""Throughput of the ALBEF single-adapter step (optimizer_mode adapter, feddat_amd.albef_adapter_engine) next to the DAT step
(feddat_amd.albef_engine), each with the LM head frozen and trained, at the full-size model (ViT-B/16 at 384, BERT-base 12 + 6
layers, vocabulary 30 522), B = 32, one answer per question, f16 operands, dynamic loss scale -- in one process and alternated:
each engine is warmed up and its hipGraph captured, then R rounds of K replays each, timed with device events.
python tools/albef_adapter_step_bench.py [--steps K] [--rounds R] [--batch B]  -> one JSON line: per engine the median ms/step
with min .. max over the rounds, samples/s, the FedAvg payload in bytes, memory allocated by its construction; and the ratios
adapter / dat."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feddat_amd import albef_spec  # noqa: E402
from feddat_amd.albef_adapter_engine import AlbefAdapterEngine  # noqa: E402
from feddat_amd.albef_engine import AlbefDatEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B = a.batch
    batches = [albef_spec.synthetic_batch(B, 1234 + i, image=384, device=dev) for i in range(4)]
    P = {"dat": albef_spec.random_init(seed=0, image=384), "adapter": albef_spec.random_init(seed=0, image=384, optimizer_mode="adapter")}
    engs, mem = {}, {}
    for name, cls, head in (("dat", AlbefDatEngine, False), ("adapter", AlbefAdapterEngine, False), ("dat-head", AlbefDatEngine, True),
                            ("adapter-head", AlbefAdapterEngine, True)):
        before = torch.cuda.memory_allocated()
        engs[name] = cls(P[name.split("-")[0]], dev, batch=B, n_answers=B, image=384, train_lm_head=head)
        mem[name] = torch.cuda.memory_allocated() - before
    total = (a.warmup + a.rounds * a.steps) * 15
    for e in engs.values():
        e.begin_local_update(steps_per_epoch=total)
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
        e = engs[k]
        e.assert_finite()
        out[k] = dict(ms_per_step=round(med, 4), samples_per_s=round(B / med * 1e3, 1), min_ms=round(min(v), 4), max_ms=round(max(v), 4),
                      rounds_ms=[round(x, 4) for x in v], skipped_batches=e.scaler_state()["skipped_batches"],
                      comm_bytes=e.comm_flat().numel() * 4, construction_bytes=mem[k], loss=round(float(e._loss_tensor()[0]), 4))
    out["ratio_adapter_over_dat"] = round(out["adapter"]["ms_per_step"] / out["dat"]["ms_per_step"], 4)
    out["ratio_adapter_over_dat_head"] = round(out["adapter-head"]["ms_per_step"] / out["dat-head"]["ms_per_step"], 4)
    print(json.dumps(dict(config=f"ALBEF full size, B={B}, 384x384, f16, hipGraph", steps=a.steps, rounds=a.rounds, **out)))


if __name__ == "__main__":
    main()
