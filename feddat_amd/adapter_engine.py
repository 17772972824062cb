"""ViLT-B/32 single-adapter (FedAvg baseline, optimizer_mode 'adapter') local-update engine on MI355X.

The reference's non-dat train_step (src/train/visionlanguage_tasks/task_trainer.py:433-450 around src/modeling/vilt.py:244-264
with adapter_config {"names": ["adapter"]}, main.py:114-118,141-149,248-250): ONE forward through the backbone with one bottleneck
adapter per layer, loss = BCEWithLogits_mean(logits, target) * C, one backward, one AdamW step over adapter + task head, one
scheduler tick.  The step itself is single_pass.SinglePassStep, shared with the bias / norm / prompt engines; forward and backward
are the dual-adapter engine's (engine.ViltDatEngine) with a single pass: the same kernels, the same static-buffer layout at
B samples (R = B * S rows) instead of 2 B, the same dynamic loss scale, and one hipGraph per step.  The adapter's tensors are
`...output.adapter.adapter_{down,up}.{weight,bias}`; the FedAvg payload (comm_flat) is all of them, back-to-back.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from . import lib as L
from .engine import ViltDatEngine
from .single_pass import SinglePassStep


class ViltAdapterEngine(SinglePassStep, ViltDatEngine):
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
        self._init_single_pass()

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

    # ------------------------------------------------------------------------------------------ train step (SinglePassStep)
    def _trained(self):
        return "adapter", self.ad[0]

    def _step_refusal(self):
        if not self.fused_tail:
            return "the single-adapter step runs on the fused step tail only"

    def _forward_train(self):
        self._forward_dual()                       # embed, layers at R rows, token-0 top layer, pooler (B rows)

    def _backward_train(self):
        self._backward_dual()                      # layers L-1 .. 1, layer-0 weight gradients, one reduce (+ inf check)

    def _after_adamw(self):
        self.repack_adapter(0)

    # ------------------------------------------------------------------------------------------ inference / state
    def forward(self, batch: Dict[str, torch.Tensor], task: Optional[str] = None):
        """model(task_key, images, texts) -> (pooled, logits) with set_active_adapter('adapter') (vilt.py:244-264)."""
        return super().forward(batch, "adapter", task)
