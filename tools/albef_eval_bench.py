#!/usr/bin/env python
"""Time of one AlbefDatEngine.rank_answer call at the reference's evaluation size on one box: the real architecture (AlbefDims():
ViT-B/16 at 384 x 384, BERT-base 12 + 6 layers, 30 522-way LM head), B = 32 questions, k = 64 of M = 3128 answers of 5 tokens,
random-init weights (the time does not depend on them), fp16 operands (the engines' default).

  (a) slabs: the engine a federation trains with (n_answers = B = 32): the 2048 candidates in 64 slabs of 32;
  (b) frame: an engine built with n_answers = B * k = 2048: each decoder pass in one frame (rank_answer's one-frame path).

Both are warmed up (one call each), then timed alternately, `--calls` calls each: wall clock around a call that ends in a device
synchronise, median and min / max printed, with how far the two paths' results are apart; `*_enqueue_ms` is the part of the call
the host spends issuing launches (the clock when rank_answer returns, before the synchronise): a call whose enqueue time is its
whole time is bound by the host's launch rate, not by the kernels.
python tools/albef_eval_bench.py [--calls 5] [--batch 32] [--k 64] [--answers 3128]
Results: DESIGN.md section 11."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from feddat_amd import albef_spec  # noqa: E402
from feddat_amd.albef_engine import AlbefDatEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--k", type=int, default=64)
ap.add_argument("--answers", type=int, default=3128)
ap.add_argument("--a_len", type=int, default=5)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("albef_eval_bench needs the GPU: there is no host path to time")
dev = torch.device("cuda", 0)
B, k, M, La = args.batch, args.k, args.answers, args.a_len
params = albef_spec.random_init(seed=0)
alist, amask = albef_spec.synthetic_answer_list(M, La, seed=1)
b = albef_spec.synthetic_batch(B, 2, device=dev)
qb = {kk: b[kk] for kk in ("image", "question_ids", "question_mask")}
alist, amask = alist.to(dev), amask.to(dev)
engines = {"slabs": AlbefDatEngine(params, dev, batch=B, n_answers=B, a_len=La),
           "frame": AlbefDatEngine(params, dev, batch=B, n_answers=B * k, a_len=La)}
del params


def one_call(name):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ids, probs = engines[name].rank_answer(qb, alist, amask, k)
    t1 = time.perf_counter()          # every launch is enqueued: the host's share of the call
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, ids, probs, (t1 - t0) * 1e3


out = {}
for name in engines:          # warm-up: code objects, function attributes, the slab maps
    _, out[name + "_ids"], out[name + "_probs"], _ = one_call(name)
times, enqueue = {name: [] for name in engines}, {name: [] for name in engines}
for _ in range(args.calls):
    for name in engines:
        r = one_call(name)
        times[name].append(r[0])
        enqueue[name].append(r[3])
# what the two paths agree on (16-bit operands on different tile shapes: not bit-identical)
same = float((out["slabs_ids"].sort(1).values == out["frame_ids"].sort(1).values).float().mean())
dprob = float((out["slabs_probs"] - out["frame_probs"]).abs().max())
res = {"B": B, "k": k, "answers": M, "a_len": La, "calls": args.calls, "operands": engines["slabs"].operands,
       "shortlists_equal_fraction": same, "max_abs_prob_diff": dprob}
for name, ts in times.items():
    res[name + "_ms_median"] = round(statistics.median(ts), 2)
    res[name + "_ms_min"], res[name + "_ms_max"] = round(min(ts), 2), round(max(ts), 2)
    res[name + "_enqueue_ms_median"] = round(statistics.median(enqueue[name]), 2)
res["slabs_over_frame"] = round(res["slabs_ms_median"] / res["frame_ms_median"], 3)
res["slabs"] = engines["slabs"]._rank_maps(B, k)["slabs"]
print(json.dumps(res))
