"""ViLT-B/32 single-adapter (FedAvg baseline, optimizer_mode 'adapter') local-update engine on MI355X.

The reference's non-dat train_step (src/train/visionlanguage_tasks/task_trainer.py:433-450 around src/modeling/vilt.py:244-264
with adapter_config {"names": ["adapter"]}, main.py:114-118,141-149,248-250): ONE forward through the backbone with one bottleneck
adapter per layer, loss = BCEWithLogits_mean(logits, target) * C, one backward, one AdamW step over adapter + task head, one
scheduler tick.  It is the DAT step (engine.ViltDatEngine) with a single pass: the same kernels, the same static-buffer layout at
B samples (R = B * S rows) instead of 2 B, the same dynamic loss scale, and one hipGraph per step.  The adapter's tensors are
`...output.adapter.adapter_{down,up}.{weight,bias}`; the FedAvg payload (comm_flat) is all of them, back-to-back.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from . import lib as L
from .engine import ViltDatEngine
from .local_update import _bound


class ViltAdapterEngine(ViltDatEngine):
    NPASS = 1
    ADAPTER_STEMS = ("adapter_",)
    COMM_ADAPTER = 0

    def __init__(self, params: Dict[str, torch.Tensor], tasks: Sequence[str], device, batch: int, res: int, fp8: bool = False,
                 **kw):
        """Arguments as ViltDatEngine (operands "f16" -- the default, dynamic loss scale -- or "bf16"); fp8 is not supported."""
        if fp8:
            raise L.FeddatHipError("optimizer_mode adapter runs with 16-bit operands only (fp8=True is a dat configuration)")
        super().__init__(params, tasks, device, batch, res, fp8=False, **kw)
        self.opt_adapters = (0,)
        self.loss_out = torch.zeros(4, device=self.dev)

    # ------------------------------------------------------------------------------------------ segment descriptors
    def _segs(self, layer: int, first: bool, bwd: bool):
        """One segment: rows [0, R), the adapter with scale 1 (its own weight-gradient slot in the backward)."""
        key = (layer, bwd)
        if key not in self._segs_cache:
            self._segs_cache[key] = L.make_segs([dict(row_begin=0, row_end=self.R, train_slot=0 if bwd else -1, x_row_delta=0,
                                                      adapters=[dict(self.ad16[0][layer], scale=1.0)])])
        return self._segs_cache[key]

    def _top_segs(self, bwd: bool):
        key = ("top", bwd)
        if key not in self._segs_cache:
            self._segs_cache[key] = L.make_segs([dict(row_begin=0, row_end=self.B, train_slot=0 if bwd else -1,
                                                      adapters=[dict(self.ad16[0][self.nl - 1], scale=1.0)])])
        return self._segs_cache[key]

    def _single_segs(self, layer: int, mode: str, rows: int):
        return L.make_segs([dict(row_begin=0, row_end=rows, adapters=[dict(self.ad16[0][layer], scale=1.0)])])

    def _wgrad_segs(self, layer: int, x, x_delta_s: int, dy):
        n = self.ad_layer_numel
        return self._wgrad_desc(("wg", layer, x.data_ptr(), dy.data_ptr()), lambda: [
            dict(x=x, dy=dy, z=self.z, dz=self.dz, grad=self.ad[0].g[layer * n:(layer + 1) * n], rows=self.R, scale=1.0)])

    def _top_wgrad_segs(self):
        i, n = self.nl - 1, self.ad_layer_numel
        return self._wgrad_desc(("wg-top",), lambda: [
            dict(x=self.top["h3"], dy=self.dcls, z=self.z, dz=self.dz, grad=self.ad[0].g[i * n:(i + 1) * n], rows=self.B,
                 scale=1.0)])

    def _named_groups(self):
        return [("adapter", self.ad[0]), ("head", self.head[self.task])]

    # ------------------------------------------------------------------------------------------ train step
    @_bound
    def begin_local_update(self, task: str, steps_per_epoch: int, num_epochs: int = 15, warmup_ratio: float = 0.1,
                           opt_adapters: Sequence[int] = (0,)):
        """TaskTrainer.train prologue for optimizer_mode adapter (task_trainer.py:36-59): no teacher copy; a fresh AdamW over
        adapter + head and a fresh poly schedule over steps_per_epoch * num_epochs ticks (one tick per batch)."""
        self.task = task
        self._start_local_update(steps_per_epoch, num_epochs, warmup_ratio, {})

    @_bound
    def _step_kernels(self):
        B, task = self.B, self.task
        hp = self.head[task]
        if not self.fused_tail:
            raise L.FeddatHipError("the single-adapter step runs on the fused step tail only")
        self._forward_dual()                       # embed, layers at R rows, token-0 top layer, pooler (B rows)
        logits = self._head_fwd(self.pooled[:B], "all", task)
        flag = self.ovf_flags[0:1]
        if self.n_valid < B:      # a short batch: the loss of the n valid rows, zero gradient in the replica rows
            L.bce_loss_fwd_bwd_rows(logits, self.inp["target"], self.dlogits, self.loss_out, self.n_valid,
                                    flag if self._dyn() else None)
        else:
            L.bce_loss_fwd_bwd(logits, self.inp["target"], self.dlogits, self.loss_out, flag if self._dyn() else None)
        self._head_bwd(self.pooled[:B], "all", task, self.dpooled[:B])
        self._backward_dual()                      # layers L-1 .. 1, layer-0 weight gradients, one reduce (+ inf check)
        skip = dict(skip_if=(flag,)) if self._dyn() else {}
        self._adamw_many([self._adamw_group(self.ad[0], **skip), self._adamw_group(hp, **skip)])
        self.repack_adapter(0)
        if self._dyn():
            L.single_step_finish([self.ad[0].state, hp.state], flag, self.scaler_f, self.scaler_i, self.scale_growth,
                                 self.scale_backoff, self.scale_growth_interval)
        else:
            L.step_tick_multi([self.ad[0].state, hp.state], [1, 1], [1, 1])

    def _loss_tensor(self):
        """What train_step returns (task_trainer.py:433-450): the device tensor whose [0] is the reference's loss =
        BCE_mean * num_labels."""
        return self.loss_out

    # ------------------------------------------------------------------------------------------ inference / state
    def forward(self, batch: Dict[str, torch.Tensor], task: Optional[str] = None):
        """model(task_key, images, texts) -> (pooled, logits) with set_active_adapter('adapter') (vilt.py:244-264)."""
        return super().forward(batch, "adapter", task)
