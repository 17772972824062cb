"""ALBEF single-adapter (FedAvg baseline, optimizer_mode 'adapter') local-update engine on MI355X -- the ALBEF counterpart of
adapter_engine.ViltAdapterEngine.

The reference's non-dat train_step (src/train/visionlanguage_tasks/task_trainer.py:433-450 around ALBEF.forward(train=True),
src/modeling/models/albef_model.py:69-145, with adapter_config {"names": ["adapter"]}: main.py:114-118,141-149,247-250): ONE
forward through the three towers with one bottleneck adapter per module, loss = the weighted LM loss alone (no KL, no factor
1/2), one backward, one AdamW step over the adapter (+ the decoder's LM head when train_lm_head), one scheduler tick.  Forward,
backward and weight gradients are the dual-adapter engine's (albef_backbone.AlbefBackbone, albef_engine.AlbefDatEngine) in the
one mode "adapter": the same kernels on ONE activation set, ONE scratch set and ONE weight-gradient workspace, on one stream.
The loss is feddat_lm_ce_loss_fwd_bwd (include/feddat_hip_albef.h).  The adapter's tensors are
`...adapter.adapter_{down,up}.{weight,bias}`; the FedAvg payload (comm_flat) is all of them back-to-back (2 236 320 floats at
full size, as many as DAT's adapter_1); the head is personal and never part of it.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from . import lib as L
from .albef_engine import AlbefDatEngine
from .local_update import _bound

MODE = "adapter"


class AlbefAdapterEngine(AlbefDatEngine):
    ADAPTER_STEMS = ("adapter_",)
    FROZEN_ADAPTERS = ()
    ACT_SETS = (MODE,)
    COMM_ADAPTER = 0

    def __init__(self, params: Dict[str, torch.Tensor], device, batch: int, n_answers: int, q_len: int = 25, a_len: int = 4,
                 vit_depth: int = 12, enc_layers: int = 12, fusion_layer: int = 6, dec_layers: int = 6, image: int = 384,
                 vocab: int = 30522, lr: float = 1e-4, weight_decay: float = 1e-2, adam_eps: float = 1e-8, pad_id: int = 0,
                 max_pos: int = 512, dropout: float = 0.0, seed: int = 0, stack_text: bool = False,
                 operands: str = "f16", loss_scale: Optional[float] = None, dynamic_loss_scale: Optional[bool] = None,
                 scale_growth_interval: int = 2000, train_lm_head: bool = False):
        """Arguments as AlbefDatEngine (operands "f16" -- the default, dynamic loss scale -- or "bf16"; train_lm_head with the same
        meaning and default: the reference's own behaviour is True).  stack_text is refused: one pass has nothing to stack."""
        if stack_text:
            raise L.FeddatHipError("optimizer_mode adapter runs one pass per step: there is nothing to stack (stack_text)")
        super().__init__(params, device, batch, n_answers, q_len, a_len, vit_depth, enc_layers, fusion_layer, dec_layers, image,
                         vocab, lr, weight_decay, adam_eps, pad_id, max_pos, dropout, seed, False, operands, loss_scale,
                         dynamic_loss_scale, scale_growth_interval, train_lm_head)

    def _alloc_head_grads(self):
        super()._alloc_head_grads()
        self.head_bak = None          # one sub-step: a skipped head update is simply not applied, nothing to restore

    # ------------------------------------------------------------------------------------------ train step
    @_bound
    def begin_local_update(self, steps_per_epoch: int, num_epochs: int = 15, warmup_ratio: float = 0.1,
                           opt_adapters: Sequence[int] = (), dropout_epoch: int = 0):
        """TaskTrainer.train prologue (task_trainer.py:30-59) of the non-dat mode: no teacher copy; a fresh AdamW over {adapter,
        head if trained} and a fresh poly schedule over steps_per_epoch * num_epochs ticks, one tick per batch.  opt_adapters
        (the dat engine's signature): () or (0,), the one adapter there is; dropout_epoch as there."""
        if tuple(opt_adapters) not in ((), (0,)):
            raise L.FeddatHipError(f"optimizer_mode adapter trains adapter 0 alone, got opt_adapters={tuple(opt_adapters)}")
        self.drop_ctr.copy_(torch.tensor([(int(dropout_epoch) << 16) & 0x7FFFFFFF, 0], dtype=torch.int32))
        self._start_local_update(steps_per_epoch, num_epochs, warmup_ratio, {})

    def copy_global_to_teacher(self):
        raise L.FeddatHipError("optimizer_mode adapter has no teacher adapter")

    def _graph_switches(self):
        return (self.dropout, self.train_lm_head, MODE)

    def _named_groups(self):
        groups = [(MODE, self.ad[0])]
        return groups + [("lm_head", self.lm)] if self.train_lm_head else groups

    @_bound
    def _step_kernels(self):
        """1. ViT, text encoder, decoder, LM head forward (dropout pass 0)   2. L = sum_r w_r ce_r and dL/dlogits, scaled
        3. LM-head backward (+ the head's gradients)   4. towers and ViT backward, one weight-gradient reduce (+ inf check)
        5. one AdamW launch over the groups, skipped on the flag   6. operand copies   7. counters / scaler   8. dropout counter."""
        dyn, pid = self._dyn(), (0 if self.dropout > 0 else None)
        S, g = self.acts[MODE], self.gs[MODE]
        flag = self.ovf_flags[0:1] if dyn else None
        logits = self._forward(MODE, pid)
        L.lm_ce_loss_fwd_bwd(logits, self.labels, self.row_w, self.V, g["dlogits"], S["loss"], **self._scale_in(MODE))
        self._lm_head_bwd(S, g, 0, self.R, self.train_lm_head, flag)
        self._towers_bwd(MODE, pid)
        self._vit_bwd(S, MODE, g["d_img"])
        self._wgrad_reduce(MODE)
        trained = [grp for _, grp in self._named_groups()]
        skip = dict(skip_if=(flag,)) if dyn else {}
        self._adamw_many([self._adamw_group(grp, **skip) for grp in trained])
        self.repack_adapter(0)
        if self.train_lm_head:
            self._refresh_head()
        states = [grp.state for grp in trained]
        if dyn:
            L.single_step_finish(states, flag, self.scaler_f, self.scaler_i, self.scale_growth, self.scale_backoff,
                                 self.scale_growth_interval)
        else:
            L.step_tick_multi(states, [1] * len(states), [1] * len(states))
        if pid is not None:
            L.step_tick(self.drop_ctr, 1, 0)                 # the next train_step draws fresh masks (also under graph replay)

    def _loss_tensor(self):
        """What train_step returns: the device buffer whose [0] (= [2]) is the reference's loss, ALBEF.forward's output."""
        return self.acts[MODE]["loss"]

    # ------------------------------------------------------------------------------------------ inference
    @staticmethod
    def _only_mode(mode: str):
        if mode != MODE:
            raise L.FeddatHipError(f"a single-adapter ALBEF runs in mode {MODE!r} only (set_active_adapter('adapter')), got {mode!r}")

    def forward_train_logits(self, batch: Dict, mode: str = MODE):
        self._only_mode(mode)
        return super().forward_train_logits(batch, mode)

    def rank_answer(self, batch: Dict, answer_ids: torch.Tensor, answer_mask: torch.Tensor, k: int, mode: str = MODE):
        self._only_mode(mode)
        return super().rank_answer(batch, answer_ids, answer_mask, k, mode)

    def image_embeds(self, mode_key: str = MODE):
        self._only_mode(mode_key)
        return super().image_embeds(mode_key)
