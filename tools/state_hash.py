#!/usr/bin/env python
"""Hash of the trained state of a full ViLT-B/32 engine after 12 hipGraph-replayed train_steps at configs[1]'s size, default
settings: every group the step updates (_named_groups(), in that order: adapter_0, adapter_1, head for the dat engine).  Two builds
with the same hash run the same arithmetic: at 80 steps the AdamW trajectory is chaotic enough that a last-bit change moves the
round-length parity draws ("draws"), so a change meant to be arithmetic-neutral -- a kernel, or the host
sequencing of an engine -- is checked with this before the 80-step tests are trusted.
python tools/state_hash.py [repo root] [--engine dat | dat-fp8 | adapter | bias | norm | prompt | albef | albef-head | albef-dropout | albef-stack | albef_adapter | albef_adapter-head] [--layers N]
(albef: the full-size AlbefDatEngine at B = 4, default settings -- the LM head frozen --, 12 replayed steps; albef-head: train_lm_head=True, albef-dropout: dropout=0.1, albef-stack: stack_text=True, each otherwise the same; albef_adapter / albef_adapter-head: the single-adapter AlbefAdapterEngine, head frozen / trained, same protocol; the albef lines end with torch.cuda.max_memory_allocated() after the engine's construction; the repo root is the tree whose feddat_amd is hashed, so one copy of this tool compares two trees)
dat, round 6 HEAD (= round 5's arithmetic): cb900273526616cd; the other engines: DESIGN.md sections 13, 14 and 21 (prompt, and --layers 1)"""
import argparse, sys, os, hashlib, torch
ap = argparse.ArgumentParser()
ap.add_argument("root", nargs="?", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ALBEF = {"albef": {}, "albef-head": dict(train_lm_head=True), "albef-dropout": dict(dropout=0.1), "albef-stack": dict(stack_text=True),
         "albef_adapter": {}, "albef_adapter-head": dict(train_lm_head=True)}
ap.add_argument("--engine", choices=("dat", "dat-fp8", "adapter", "bias", "norm", "prompt") + tuple(ALBEF), default="dat")
ap.add_argument("--layers", type=int, default=12, help="encoder layers of the ViLT engines (1: the top layer is layer 0)")
args = ap.parse_args()
root = args.root
sys.path.insert(0, root)
from feddat_amd import engine, vilt_spec
dev = torch.device("cuda", 0)
if args.engine in ALBEF:
    from feddat_amd import albef_engine, albef_spec
    if args.engine.startswith("albef_adapter"):
        from feddat_amd.albef_adapter_engine import AlbefAdapterEngine
        e = AlbefAdapterEngine(albef_spec.random_init(seed=0, image=384, optimizer_mode="adapter"), dev, batch=4, n_answers=4,
                               image=384, **ALBEF[args.engine])
    else:
        e = albef_engine.AlbefDatEngine(albef_spec.random_init(seed=0, image=384), dev, batch=4, n_answers=4, image=384,
                                        **ALBEF[args.engine])
    mem = torch.cuda.max_memory_allocated()
    batches = [albef_spec.synthetic_batch(4, 1234 + i, image=384, device=dev) for i in range(4)]
    e.begin_local_update(steps_per_epoch=80)
    for i in range(12):
        e.train_step(batches[i % 4], use_graph=True)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for _, grp in e._named_groups():
        h.update(grp.p.cpu().numpy().tobytes())
    print(os.path.basename(root), args.engine, h.hexdigest()[:16], float(e.comm_flat().double().abs().sum()), float(e._loss_tensor()[0]),
          "max_memory_allocated after construction", mem)
    sys.exit(0)
mode = "dat" if args.engine.startswith("dat") else args.engine
params = vilt_spec.random_init(args.layers, ["c0"], seed=0, optimizer_mode=mode)
batches = [vilt_spec.synthetic_batch(32, 384, 1234 + i, device=dev) for i in range(4)]
size = dict(batch=32, res=384, layers=args.layers)
if mode == "dat":
    e = engine.ViltDatEngine(params, ["c0"], dev, fp8=args.engine == "dat-fp8", **size)
    e.top_q_cls = False
elif mode == "adapter":
    from feddat_amd.adapter_engine import ViltAdapterEngine
    e = ViltAdapterEngine(params, ["c0"], dev, **size)
elif mode == "prompt":
    from feddat_amd.prompt_engine import ViltPromptEngine
    e = ViltPromptEngine(params, ["c0"], dev, **size)
else:
    from feddat_amd.vector_engine import ViltVectorEngine
    e = ViltVectorEngine(params, ["c0"], dev, mode=mode, **size)
e.begin_local_update("c0", steps_per_epoch=80)
for i in range(12):
    e.train_step(batches[i % 4], use_graph=True)
torch.cuda.synchronize()
h = hashlib.sha256()
for _, grp in e._named_groups():
    h.update(grp.p.cpu().numpy().tobytes())
print(os.path.basename(root), args.engine, h.hexdigest()[:16], float(e.comm_flat().double().abs().sum()),
      float(e._loss_tensor()[0]))
