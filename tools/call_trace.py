#!/usr/bin/env python
"""Record every call an engine makes into the HIP library, in a form that two source trees can be compared by: a change meant to
leave the launch list alone -- a refactor of an engine's host sequencing -- gives the same call count and the same hash before
and after.  The recorder stands between feddat_amd.lib and the loaded libraries (what lib.load() returns) and only reads the
arguments on their way through: it changes none and adds no launch.  Per call it logs
  the entry point's name,
  every scalar argument,
  the stream as the ordinal of its first appearance (s0, s1, ...),
  every pointer as the ordinal of its first appearance in the trace (p1, p2, ...; 0 = NULL) -- addresses differ from run to run,
    which buffer is which does not,
  and for arrays of AdapterSeg, WgradSeg, HtJob and AdamwGroup their fields the same way; the device-resident VgradJob table of
    feddat_vector_grad_reduce is read back once where lib.make_vgrad_jobs builds it and logged with every reduce that takes it.
The trace starts with the engine's construction and prints the call count and the sha256 of the log; --dump FILE writes the log
itself, one call per line, so that two trees' traces can be diffed.

python tools/call_trace.py [repo root] --engine albef [--head] [--dropout P] [--stack-text] [--opt-adapters 1] [--static-scale]
                           [--operands bf16] [--eval] [--dump FILE]
The repo root is the tree whose feddat_amd is traced (as in tools/state_hash.py: one copy of this tool traces two trees).
albef: the small model of tests/test_albef_gpu.py (SMALL), B = 3, N = 9, q_len 16, a_len 7.  A training run is two eager
train_steps on full frames and one on a batch inside the frame (12-token questions, k = [2, 1, 3]: 6 answers of 5 tokens).
--eval instead runs forward_train_logits in "gating" and "adapter_0" and rank_answer twice: through the slabs (2 questions, k = 4,
on the N = 9 engine) and as one frame (an engine with n_answers = B * k).  Each run takes a few seconds."""
import argparse
import ctypes as C
import hashlib
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("root", nargs="?", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--engine", choices=("albef",), default="albef")
ap.add_argument("--head", action="store_true", help="train_lm_head=True")
ap.add_argument("--dropout", type=float, default=0.0)
ap.add_argument("--stack-text", action="store_true")
ap.add_argument("--opt-adapters", type=int, nargs="+", default=[0, 1], help="begin_local_update's opt_adapters")
ap.add_argument("--static-scale", action="store_true", help="dynamic_loss_scale=False")
ap.add_argument("--operands", choices=("f16", "bf16"), default="f16")
ap.add_argument("--eval", action="store_true", help="the evaluation paths instead of train_steps")
ap.add_argument("--dump", metavar="FILE")
args = ap.parse_args()
sys.path.insert(0, args.root)
from feddat_amd import lib as L  # noqa: E402


class Stream(C.c_void_p):
    """lib._stream()'s handle, told apart from the data pointers by its type."""


class Recorder:
    def __init__(self):
        self.lines, self.ptrs, self.streams, self.tables = [], {}, {}, {}

    def ptr(self, v):
        v = getattr(v, "value", v)
        return "0" if not v else "p%d" % self.ptrs.setdefault(v, len(self.ptrs) + 1)

    def scalar(self, v):
        return repr(getattr(v, "value", v))

    def struct(self, s):
        out = []
        for name, typ in s._fields_:
            v = getattr(s, name)
            if isinstance(v, C.Array):
                one = self.ptr if v._type_ is C.c_void_p else self.scalar
                out.append("%s=(%s)" % (name, ",".join(one(x) for x in v)))
            else:
                out.append("%s=%s" % (name, self.ptr(v) if typ is C.c_void_p else self.scalar(v)))
        return "{" + " ".join(out) + "}"

    def arg(self, a, typ):
        if isinstance(a, Stream):
            return "s%d" % self.streams.setdefault(a.value or 0, len(self.streams))
        if isinstance(a, C.Array):
            if issubclass(a._type_, C.Structure):
                return "[" + " ".join(self.struct(s) for s in a) + "]"
            return "[" + ",".join((self.ptr if a._type_ is C.c_void_p else self.scalar)(x) for x in a) + "]"
        if a is None or isinstance(a, C.c_void_p) or (typ is C.c_void_p and isinstance(a, int)):
            v = getattr(a, "value", a)
            table = self.tables.get(v)
            return self.ptr(v) + ("[" + " ".join(self.struct(s) for s in table) + "]" if table else "")
        if isinstance(a, (int, float)):
            return repr(a)
        return "<%s>" % type(a).__name__          # byref() results of the query entry points, strings

    def wrap(self, lib):
        rec = self

        class Traced:
            def __getattr__(self, name):
                fn = getattr(lib, name)
                types = fn.argtypes or ()

                def call(*a):
                    rec.lines.append(name + " " + " ".join(rec.arg(x, t) for x, t in zip(a, types)))
                    return fn(*a)
                setattr(self, name, call)
                return call
        return Traced()


rec = Recorder()
L.load()
with L.operands("f16"):
    L.load()
L._lib, L._lib_f16 = rec.wrap(L._lib), rec.wrap(L._lib_f16)
L._stream = lambda: Stream(torch.cuda.current_stream().cuda_stream)
_make_vgrad_jobs, _p, _seen = L.make_vgrad_jobs, L._p, {}


def p(t):
    """lib._p, holding on to the tensor: no address the trace has seen is freed and handed out again under another ordinal's
    name while it runs (which temporary lands in which freed block depends on the order of the engine's allocations)."""
    if t is not None:
        _seen[t.data_ptr()] = t
    return _p(t)


def make_vgrad_jobs(jobs, device):
    table, n, max_n = _make_vgrad_jobs(jobs, device)
    rec.tables[table.data_ptr()] = (L.VgradJob * n).from_buffer_copy(table.cpu().numpy().tobytes())
    return table, n, max_n


L.make_vgrad_jobs, L._p = make_vgrad_jobs, p

from feddat_amd import albef_engine, albef_spec  # noqa: E402

dev = torch.device("cuda", 0)
SMALL = dict(vit_depth=2, enc_layers=3, fusion_layer=1, dec_layers=2, image=64, vocab=3072, max_pos=64)
B, N, LQ, LA = 3, 9, 16, 7
params = albef_spec.random_init(seed=0, **SMALL)


def engine(n_answers, **kw):
    dims = {k: v for k, v in SMALL.items() if k != "max_pos"}
    return albef_engine.AlbefDatEngine(params, dev, batch=B, n_answers=n_answers, q_len=LQ, a_len=LA, max_pos=SMALL["max_pos"],
                                       operands=args.operands, **dims, **kw)


def batch(seed, q_len=LQ, a_len=LA, k=(3, 3, 3)):
    return albef_spec.synthetic_batch(B, seed, image=SMALL["image"], q_len=q_len, a_len=a_len, k=k, vocab=SMALL["vocab"], device=dev)


if args.eval:
    e = engine(N)
    for mode in ("gating", "adapter_0"):
        e.forward_train_logits(batch(20, 12, 5, (2, 1, 3)), mode)
    k = 4
    ids, mask = albef_spec.synthetic_answer_list(11, a_len=5, vocab=SMALL["vocab"], seed=3)
    b = batch(21, 12)
    e.rank_answer({n: b[n][:2] for n in ("image", "question_ids", "question_mask")}, ids, mask, k)          # slabs
    e = engine(B * k)
    ids, mask = albef_spec.synthetic_answer_list(11, a_len=LA, vocab=SMALL["vocab"], seed=4)
    b = batch(22)
    e.rank_answer({n: b[n] for n in ("image", "question_ids", "question_mask")}, ids, mask, k)              # one frame
else:
    e = engine(N, dropout=args.dropout, stack_text=args.stack_text, train_lm_head=args.head,
               dynamic_loss_scale=False if args.static_scale else None)
    e.begin_local_update(steps_per_epoch=4, opt_adapters=tuple(args.opt_adapters))
    for b in (batch(10), batch(11), batch(12, 12, 5, (2, 1, 3))):
        e.train_step(b)
torch.cuda.synchronize()
log = "\n".join(rec.lines) + "\n"
print(os.path.basename(os.path.abspath(args.root)), " ".join(sys.argv[2 if sys.argv[1:2] == [args.root] else 1:]) or "default",
      "calls", len(rec.lines), "sha256", hashlib.sha256(log.encode()).hexdigest()[:16])
if args.dump:
    with open(args.dump, "w") as f:
        f.write(log)
