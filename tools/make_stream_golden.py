#!/usr/bin/env python
"""Write tests/golden/stream_kernels.json: sha256 digests of what the LayerNorm, multi-group AdamW, im2col, embedding and adapter-pack kernels produce on the seeded
cases of tests/test_stream_kernels_gpu.py (which defines the cases and compares against this file).

The fixture is a REFERENCE for kernels that are rewritten to move the same bits faster, so it is generated from the libraries of
the commit BEFORE such a rewrite, on a GPU box:

    git stash / git worktree the parent commit, python -m feddat_amd.build there, then here:
    python tools/make_stream_golden.py --lib-dir <parent tree>/feddat_amd

--lib-dir: directory holding libfeddat_hip.so and libfeddat_hip_f16.so to run (default: this tree's own).  The case list comes
from THIS tree's test module; the kernels from --lib-dir."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--lib-dir", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "stream_kernels.json"))
args = ap.parse_args()

import torch  # noqa: E402
from feddat_amd import lib  # noqa: E402

if args.lib_dir:
    lib.LIB_PATH = os.path.join(os.path.abspath(args.lib_dir), "libfeddat_hip.so")
    lib.LIB_PATH_F16 = os.path.join(os.path.abspath(args.lib_dir), "libfeddat_hip_f16.so")
lib.load()
with lib.operands("f16"):
    lib.load()

from tests import test_stream_kernels_gpu as T  # noqa: E402

torch.manual_seed(0)
digests = T.all_digests(lib)
# compute_units fixes the two grid-dependent LayerNorm row counts
meta = {"libraries": "the parent of the commit that made the H = 768 LayerNorm kernels persistent",
        "compute_units": torch.cuda.get_device_properties(0).multi_processor_count}
with open(args.out, "w") as f:
    json.dump({"meta": meta, "digests": digests}, f, indent=0, sort_keys=True)
print(f"{len(digests)} cases, {sum(len(v) for v in digests.values())} digests -> {args.out} ({os.path.getsize(args.out)} bytes)")
