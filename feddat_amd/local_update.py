"""Host-side protocol that every local-update engine shares around its HIP step (the ViLT engines on vilt_backbone.ViltBackbone --
ViltDatEngine, ViltAdapterEngine, ViltVectorEngine -- and albef_engine.AlbefDatEngine on albef_backbone.AlbefBackbone): the flat trainable groups, the device-side loss scaler
(GradScaler on the device), the AdamW launches and the DAT optimizer tail, the start of a local update,
hipGraph capture, and the trainable state.

An engine derived from LocalUpdateEngine supplies its step (`_step_kernels`), its adapters (`ad`, `repack_adapter`; an engine
without adapters: `ad = []`), the (name, group) pairs a train_step updates (`_named_groups`), the host-side switches frozen into a
captured step (`_graph_switches`) and the tensor train_step returns (`_loss_tensor`)."""
from __future__ import annotations

import functools
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import lib as L


def _no_decay(name: str) -> bool:  # task_trainer.py:478
    return ("bias" in name) or ("LayerNorm.weight" in name)


def _bound(fn):
    """Run a public engine method with the calling thread bound to the library of the engine's operand format
    (lib.operands): engines of both formats can live in one process."""
    @functools.wraps(fn)
    def wrapped(self, *a, **kw):
        with L.operands(self.operands):
            return fn(self, *a, **kw)
    return wrapped


class FlatGroup:
    """A set of named fp32 tensors living back-to-back in one flat device buffer (+ grad, Adam m/v, segment table)."""

    def __init__(self, names_shapes: Sequence, device, with_opt: bool, pad: int = 0):
        """pad: floats kept behind the last tensor besides the quad padding (they belong to no name and stay 0.0f like it): the
        ALBEF LM head's vocabulary bias, last in its group, is followed by the padding of the vocabulary axis, so that its
        gradient can be reduced at the padded width."""
        self.names = [n for n, _ in names_shapes]
        self.shapes = {n: tuple(s) for n, s in names_shapes}
        self.offsets = {}
        off = 0
        for n, s in names_shapes:
            self.offsets[n] = off
            off += int(math.prod(s))
        self.numel = off
        # the buffers hold a whole number of quads (the multi-group AdamW moves 16 bytes per lane: feddat_adamw_multi wants
        # n % 4 == 0); up to 3 floats behind the last tensor (a head of 3129 labels: 5 993 529 floats) stay 0.0f for good --
        # zero gradient, zero moments, and they belong to no name
        alloc = (off + int(pad) + 3) // 4 * 4
        self.p = torch.zeros(alloc, device=device)
        if with_opt:
            self.g = torch.zeros(alloc, device=device)
            self.m = torch.zeros(alloc, device=device)
            self.v = torch.zeros(alloc, device=device)
            offs = [self.offsets[n] for n in self.names] + [off]
            self.seg_off = torch.tensor(offs, dtype=torch.int64, device=device)
            self.seg_wd = torch.tensor([0.0 if _no_decay(n) else 1.0 for n in self.names], device=device)
            self.state = torch.zeros(2, dtype=torch.int32, device=device)  # {sched_t, adam_t}

    def view(self, name: str, buf: Optional[torch.Tensor] = None) -> torch.Tensor:
        buf = self.p if buf is None else buf
        o = self.offsets[name]
        return buf[o:o + int(math.prod(self.shapes[name]))].view(self.shapes[name])


class LocalUpdateEngine:
    # the adapter slot whose tensors the federation averages (comm_flat)
    COMM_ADAPTER = 1
    # samples of the engine's static B-sample frame that the staged batch really holds (the ViLT engines' set_batch records
    # it: a short last batch has n_valid < B); None: the engine takes full batches only
    n_valid: Optional[int] = None

    # ------------------------------------------------------------------------------------------ loss scale
    def _init_loss_scale(self, operands: str, loss_scale: Optional[float], dynamic_loss_scale: Optional[bool],
                         scale_growth_interval: int):
        """Operand format and loss scale: a power of two (it is removed exactly), default 2^14 for "f16" and 1 for "bf16";
        dynamic (GradScaler on the device) by default for "f16"."""
        if operands not in L.OPERAND_DTYPE:
            raise L.FeddatHipError(f"operands must be 'bf16' or 'f16', got {operands!r}")
        self.operands, self.op_dtype = operands, L.OPERAND_DTYPE[operands]
        self.loss_scale = float(loss_scale if loss_scale is not None else (16384.0 if operands == "f16" else 1.0))
        if self.loss_scale <= 0 or math.frexp(self.loss_scale)[0] != 0.5:
            raise L.FeddatHipError("loss_scale must be a power of two (it is removed exactly)")
        self.dynamic_scale = bool(operands == "f16" if dynamic_loss_scale is None else dynamic_loss_scale)
        self.scale_growth, self.scale_backoff, self.scale_growth_interval = 2.0, 0.5, int(scale_growth_interval)

    def _alloc_scaler(self):
        """The dynamic loss scale's device state: {scale, 1 / scale}; {growth tracker, skipped sub-steps, batches with a skip,
        -}; overflow flags {sub-step B = adapter_0's pass, sub-step A = adapter_1's pass}."""
        self.scaler_f = torch.tensor([self.loss_scale, 1.0 / self.loss_scale], dtype=torch.float32, device=self.dev)
        self.scaler_i = torch.zeros(4, dtype=torch.int32, device=self.dev)
        self.ovf_flags = torch.zeros(2, dtype=torch.int32, device=self.dev)
        self._no_head = torch.zeros(2, dtype=torch.int32, device=self.dev)      # feddat_dat_step_finish's head counters, no head

    def _dyn(self) -> bool:
        """Dynamic loss scale in effect."""
        return self.dynamic_scale

    def _scale_out(self):
        """How the loss scale leaves, where the adapter weight gradients are formed (feddat_wgrad_seg)."""
        return dict(grad_unscale=1.0, grad_unscale_dev=self.scaler_f[1:2]) if self._dyn() else \
            dict(grad_unscale=1.0 / self.loss_scale)

    def scaler_state(self) -> Dict[str, float]:
        """Host copy of the loss scaler (one device read-back): current scale, growth tracker, skipped sub-steps / batches."""
        f, i = self.scaler_f.tolist(), self.scaler_i.tolist()
        return dict(scale=f[0], growth_tracker=i[0], skipped_substeps=i[1], skipped_batches=i[2], dynamic=self._dyn())

    def _wgrad_desc(self, key: Tuple, segs):
        """Weight-gradient descriptor (lib.make_wgrad_segs) of the segment dicts `segs()` returns, built once per key; None when
        there is no segment.  The scale mode is appended to every key and its unscale fields to every segment here, so a
        descriptor built under one mode is never launched under the other."""
        key = key + (self._dyn(),)
        if key not in self._segs_cache:
            s = segs()
            self._segs_cache[key] = L.make_wgrad_segs([dict(d, **self._scale_out()) for d in s]) if s else None
        return self._segs_cache[key]

    def _reduce_wgrads(self, grads_dev, n, nseg, partials, stride, flags):
        """feddat_adapter_wgrad_reduce; with the dynamic scale its checked form, which ORs GradScaler's inf check of segment k
        into flags[k]."""
        if self._dyn():
            L.adapter_wgrad_reduce_checked(grads_dev, n, nseg, partials, stride, flags)
        else:
            L.adapter_wgrad_reduce(grads_dev, n, nseg, partials, stride)

    # ------------------------------------------------------------------------------------------ optimizer
    def _wd_vec(self, grp: FlatGroup):
        if not hasattr(grp, "_wdv") or grp._wdv_val != self.wd:
            grp._wdv = grp.seg_wd * self.wd
            grp._wdv_val = self.wd
        return grp._wdv

    def _adamw_group(self, grp: FlatGroup, d_sched: int = 0, d_adam: int = 0, **kw):
        return L.adamw_group(grp.p, grp.g, grp.m, grp.v, grp.seg_off, self._wd_vec(grp), grp.state, d_sched, d_adam, **kw)

    def _adamw_many(self, groups):
        L.adamw_multi(groups, self.lr, self.sched["warmup"], self.sched["total"], 0.9, 0.98, self.eps)

    def _dat_tail(self, head: Optional[FlatGroup] = None, head_bak: Optional[torch.Tensor] = None):
        """End of a DAT train_step: adapter_1 (tick 2b), the head if there is one (2b + 1: it reads its counters one ahead) and
        adapter_0 (2b + 1) in ONE AdamW launch, the 16-bit operand copies of the updated adapters, then ONE launch for all
        counters.  Under the dynamic scale GradScaler's skips are device predicates: flag A (adapter_1's pass overflowed) voids
        the batch -- adapter_1 and adapter_0 stay, the head returns to its state before sub-step A (head_bak); flag B alone skips
        the head's second update and adapter_0's.  feddat_dat_step_finish then ticks the counters by what was applied (a
        skipped optimizer step skips its scheduler tick), updates the scale and clears the flags."""
        dyn = self._dyn()
        fB, fA = self.ovf_flags[0:1], self.ovf_flags[1:2]
        groups = []
        if 1 in self.opt_adapters:
            groups.append(self._adamw_group(self.ad[1], **(dict(skip_if=(fA,)) if dyn else {})))
        if head is not None:
            groups.append(self._adamw_group(head, 1, 1, **(dict(skip_if=(fB,), bak=head_bak, bak_mode=2, restore_if=fA)
                                                           if dyn else {})))
        if 0 in self.opt_adapters:
            groups.append(self._adamw_group(self.ad[0], **(dict(skip_if=(fA, fB)) if dyn else {})))
        if groups:
            self._adamw_many(groups)
        for a in (1, 0):
            if a in self.opt_adapters:
                self.repack_adapter(a)
        if dyn:
            L.dat_step_finish(self._no_head if head is None else head.state, self.ad[1].state, self.ad[0].state, self.ovf_flags,
                              self.scaler_f, self.scaler_i, self.scale_growth, self.scale_backoff, self.scale_growth_interval)
        elif head is None:
            L.step_tick_multi([self.ad[1].state, self.ad[0].state], [2, 2], [1, 1])
        else:
            L.step_tick_multi([head.state, self.ad[1].state, self.ad[0].state], [2, 2, 2], [2, 1, 1])

    # ------------------------------------------------------------------------------------------ local update
    def _start_local_update(self, steps_per_epoch: int, num_epochs: int, warmup_ratio: float,
                            counters: Dict[str, Tuple[int, int]]):
        """Fresh AdamW state and poly schedule over steps_per_epoch * num_epochs ticks; counters: the initial
        {schedule index, Adam step} of the named groups that do not start at {0, 0}."""
        total = steps_per_epoch * num_epochs
        self.sched = dict(total=total, warmup=int(total * warmup_ratio))
        for name, grp in self._named_groups():
            grp.m.zero_()
            grp.v.zero_()
            grp.g.zero_()
            grp.state.copy_(torch.tensor(counters.get(name, (0, 0)), dtype=torch.int32))
        # a fresh GradScaler per local update (the reference builds a fresh Accelerator per round: main.py:435)
        self.scaler_f.copy_(torch.tensor([self.loss_scale, 1.0 / self.loss_scale], dtype=torch.float32))
        self.scaler_i.zero_()
        self.ovf_flags.zero_()
        # a captured step stays valid across local updates as long as everything it froze into kernel arguments or into its
        # launch list is unchanged (all mutable state -- weights, moments, counters -- lives in device buffers)
        sig = (total, self.sched["warmup"], self.opt_adapters, self.lr, self.wd, self.eps, self.operands, self.loss_scale,
               self._dyn(), self.scale_growth_interval) + self._graph_switches()
        if getattr(self, "_graph_sig", None) != sig:
            self.graph = None
            self._graph_sig = sig

    def _graph_switches(self) -> Tuple:
        """The engine's host-side switches that change the launch list of a step (part of the graph signature)."""
        return ()

    def _named_groups(self) -> List[Tuple[str, FlatGroup]]:
        """(name, group) of every group a train_step updates."""
        raise NotImplementedError

    def _extra_step_state(self) -> List[torch.Tensor]:
        """Device tensors besides the trained groups and the scaler that a train_step advances."""
        return []

    @_bound
    def copy_global_to_teacher(self):
        """adapter_1 -> adapter_2 at the start of every local update (task_trainer.py:36-41)."""
        self.ad[2].p.copy_(self.ad[1].p)
        self.repack_adapter(2)

    # ------------------------------------------------------------------------------------------ train step
    @_bound
    def train_step(self, batch: Optional[Dict] = None, use_graph: bool = False):
        """One local-update step on `batch` (None: the batch already staged); use_graph: replay the step as one hipGraph
        (captured on first use).  Returns the engine's loss tensor (_loss_tensor)."""
        if batch is not None:
            self.set_batch(batch)
        if not use_graph or self._short_batch():
            # a short batch is never captured or replayed: its launch list differs (the loss kernels with a row count), and it
            # comes once per epoch; the captured full-batch graph and its signature stay as they are
            self._step_kernels()
        else:
            self.ensure_captured()
            self.graph.replay()
        return self._loss_tensor()

    def _short_batch(self) -> bool:
        """The staged batch holds fewer samples than the engine's static frame."""
        return self.n_valid is not None and self.n_valid < self.B

    @_bound
    def ensure_captured(self):
        """Capture the step graph now if it is not there yet (TaskTrainer.train calls this before it starts the upload
        worker, so no capture ever overlaps a prefetch)."""
        if self.graph is None:
            self._capture()

    @_bound
    def _capture(self):
        """Capture the whole step into one hipGraph (all launches are on static buffers; the LR schedule and Adam
        step counts live on the device).  The trained state, the scaler and the engine's other step state are saved /
        restored around the warm-up + capture run so that capturing does not advance training."""
        groups = [grp for _, grp in self._named_groups()]
        state = [t for g in groups for t in (g.p, g.m, g.v, g.state)] + [self.scaler_f, self.scaler_i, self.ovf_flags] + \
            self._extra_step_state()
        saved = [t.clone() for t in state]
        # the graph is ALWAYS the full-batch launch list, whatever is staged (a loader whose only batch is short): the tail of
        # the frame holds finite replicas then, and the staged row count comes back below
        staged = self.n_valid
        if staged is not None:
            self.n_valid = self.B
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._step_kernels()      # warm-up (sets function attributes, allocates lazily created scratch)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        # thread_local: other host threads (feddat_amd.data.DevicePrefetcher's upload worker) may allocate and copy on their
        # own streams while this thread captures; the default global mode would turn their hipMalloc / hipMemcpy into
        # hipErrorStreamCaptureUnsupported
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            self._step_kernels()
        torch.cuda.synchronize()
        for t, v in zip(state, saved):
            t.copy_(v)
        for a, ad in enumerate(self.ad):
            if any(ad is g for g in groups):
                self.repack_adapter(a)
        torch.cuda.synchronize()
        if staged is not None:
            self.n_valid = staged
        self.graph = graph

    # ------------------------------------------------------------------------------------------ state
    def _state_groups(self) -> List[FlatGroup]:
        """The groups whose tensors make up state_dict."""
        return list(self.ad)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """Trainable tensors under the reference's state-dict keys (views into the flat buffers)."""
        return {n: grp.view(n) for grp in self._state_groups() for n in grp.names}

    @_bound
    def load_tensors(self, tensors: Dict[str, torch.Tensor]):
        """Copy tensors in under their state-dict keys; the 16-bit operand copies of every adapter touched are rebuilt."""
        sd = self.state_dict()
        touched = set()
        for n, v in tensors.items():
            sd[n].copy_(v.to(self.dev, torch.float32))
            touched.update(a for a, grp in enumerate(self.ad) if n in grp.offsets)
        for a in sorted(touched):
            self.repack_adapter(a)

    def comm_flat(self) -> torch.Tensor:
        """The FedAvg payload: every tensor of the averaged adapter back-to-back in state-dict order (main.py:154-163,499-503)."""
        grp = self.ad[self.COMM_ADAPTER]
        return grp.p[:grp.numel]      # without FlatGroup's quad padding (the adapters' sizes are multiples of 4: the whole buffer)

    def comm_written(self):
        """To be called after comm_flat() was overwritten (a server copy, the FedAvg write-back): rebuilds what the step derives
        from it, the averaged adapter's 16-bit operand copies."""
        self.repack_adapter(self.COMM_ADAPTER)

    def repack(self):
        """Rebuild the 16-bit operand copies of every adapter (after tensors were written into state_dict()'s views)."""
        for a in range(len(self.ad)):
            self.repack_adapter(a)

    def nonfinite_groups(self) -> List[str]:
        """Names of the trainable groups holding an inf / NaN (one host read-back each); [] = all finite (train.main agrees on
        this across ranks before the FedAvg collective)."""
        return [name for name, grp in self._named_groups() if not bool(torch.isfinite(grp.p).all())]

    def assert_finite(self):
        """Last line of defence.  With the dynamic loss scale (the default for fp16 operands) an overflowed sub-step is skipped
        on the device like GradScaler does (task_trainer.py:302 via accelerate) and this never fires; with a STATIC scale
        a gradient operand that left fp16's range turns the update non-finite.  One host read-back of the trainable state,
        meant to be called once per local update (TaskTrainer.train does; train.main agrees on the outcome across ranks BEFORE
        the FedAvg collective); raises with what to change."""
        bad = self.nonfinite_groups()
        if bad:
            raise L.FeddatHipError(
                f"non-finite values in {', '.join(bad)} after the local update: with operands={self.operands!r} the backward "
                f"carries a {'dynamic' if self._dyn() else 'static'} loss scale (initial value {self.loss_scale:g}); "
                + ("the scaler skips overflowed steps, so the non-finite values entered through the inputs or the weights"
                   if self._dyn() else
                   "this model's gradients leave fp16's range at that scale -- construct the engine with "
                   "dynamic_loss_scale=True, a smaller power of two (loss_scale=...) or operands='bf16'"))
