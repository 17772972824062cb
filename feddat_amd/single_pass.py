"""What the four single-pass ViLT baselines (optimizer_mode 'adapter', 'bias', 'norm', 'prompt') share, each once.

SinglePassStep is the reference's non-dat train_step (src/train/visionlanguage_tasks/task_trainer.py:433-450): one forward, loss =
BCEWithLogits_mean * C, one backward, one AdamW step over {the mode's group, task head}, one scheduler tick.  An engine mixes it
in ahead of its backbone class and supplies what differs: `_forward_train`, `_backward_train`, the trained group (`_trained`),
when it refuses to run (`_step_refusal`) and, with 16-bit operand copies to rebuild, `_after_adamw`.

ViltFrozenEngine is the base of the engines with no adapter in the backbone (vector_engine.ViltVectorEngine,
prompt_engine.ViltPromptEngine): the activations kept for a backward that runs through layer 0, the frozen forward behind the
embeddings, and the ONE dX chain from dpooled to d h0 (`_backward_kept`), which offers the gradient tensors it passes to two
optional taps -- the bias / norm engine's column sums and LayerNorm parameter gradients; the prompt engine takes none.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from . import lib as L
from .local_update import FlatGroup, _bound
from .vilt_backbone import ViltBackbone


class SinglePassStep:
    """Mixin over a LocalUpdateEngine on vilt_backbone.ViltBackbone; list it first among the bases."""

    def _init_single_pass(self):
        self.loss_out = torch.zeros(4, device=self.dev)

    # ------------------------------------------------------------------------------------------ what an engine supplies
    def _trained(self) -> Tuple[str, FlatGroup]:
        """(name, group) of the mode's trainable group; the task head is the step's other one."""
        raise NotImplementedError

    def _forward_train(self):
        """Inputs staged -> self.pooled[:B], everything the backward reads kept."""
        raise NotImplementedError

    def _backward_train(self):
        """self.dpooled[:B] -> the gradient of the trained group (unscaled, overflow-checked under the dynamic scale)."""
        raise NotImplementedError

    def _step_refusal(self) -> Optional[str]:
        """Why the step cannot run under the engine's current host switches; None when it can."""
        return None

    def _after_adamw(self):
        """Between the AdamW launch and the counters' launch: whatever the next forward derives from the updated group."""

    # ------------------------------------------------------------------------------------------ train step
    def _named_groups(self):
        return [self._trained(), ("head", self.head[self.task])]

    @_bound
    def begin_local_update(self, task: str, steps_per_epoch: int, num_epochs: int = 15, warmup_ratio: float = 0.1,
                           opt_adapters: Sequence[int] = ()):
        """TaskTrainer.train prologue (task_trainer.py:36-59) of a non-dat mode: no teacher copy; a fresh AdamW over {the mode's
        group, head} and a fresh poly schedule over steps_per_epoch * num_epochs ticks (one tick per batch).  opt_adapters is
        accepted for the dat engine's signature and ignored."""
        self.task = task
        self._start_local_update(steps_per_epoch, num_epochs, warmup_ratio, {})

    @_bound
    def _step_kernels(self):
        B, task = self.B, self.task
        grp, hp = self._trained()[1], self.head[task]
        why = self._step_refusal()
        if why:
            raise L.FeddatHipError(why)
        self._forward_train()
        logits = self._head_fwd(self.pooled[:B], "all", task)
        flag = self.ovf_flags[0:1]
        if self.n_valid < B:      # a short batch: the loss of the n valid rows, zero gradient in the replica rows
            L.bce_loss_fwd_bwd_rows(logits, self.inp["target"], self.dlogits, self.loss_out, self.n_valid,
                                    flag if self._dyn() else None)
        else:
            L.bce_loss_fwd_bwd(logits, self.inp["target"], self.dlogits, self.loss_out, flag if self._dyn() else None)
        self._head_bwd(self.pooled[:B], "all", task, self.dpooled[:B])
        self._backward_train()
        skip = dict(skip_if=(flag,)) if self._dyn() else {}
        self._adamw_many([self._adamw_group(grp, **skip), self._adamw_group(hp, **skip)])
        self._after_adamw()
        if self._dyn():
            L.single_step_finish([grp.state, hp.state], flag, self.scaler_f, self.scaler_i, self.scale_growth,
                                 self.scale_backoff, self.scale_growth_interval)
        else:
            L.step_tick_multi([grp.state, hp.state], [1, 1], [1, 1])

    def _loss_tensor(self):
        """What train_step returns (task_trainer.py:433-450): the device tensor whose [0] is the reference's loss =
        BCE_mean * num_labels."""
        return self.loss_out


class ViltFrozenEngine(SinglePassStep, ViltBackbone):
    def __init__(self, params: Dict[str, torch.Tensor], tasks: Sequence[str], device, batch: int, res: int, mode: str,
                 fp8: bool = False, **kw):
        """mode: the optimizer_mode the subclass runs; other arguments as ViltBackbone (operands "f16" -- the default, dynamic
        loss scale -- or "bf16"); fp8 is not supported."""
        if fp8:
            raise L.FeddatHipError(f"optimizer_mode {mode} runs with 16-bit operands only (fp8=True is a dat configuration)")
        self.mode = mode
        super().__init__(params, tasks, device, batch, res, **kw)
        self._init_single_pass()

    def _step_refusal(self):
        if not (self.fused_tail and self.cls_attention):
            return f"the {self.mode} step runs on the fused step tail and the token-0 top layer only"

    def _graph_switches(self) -> Tuple:
        return super()._graph_switches() + (self.mode,)

    # ------------------------------------------------------------------------------------------ forward
    def _alloc_kept(self) -> List[dict]:
        """The activations an adapter-less engine keeps for its backward: every layer at R rows, layer 0 included; no adapter
        between the layers, so layer i reads layer i - 1's output in place."""
        act: List[dict] = []
        for i in range(self.nl):
            act.append(self._kept_layer(h_in=self.h0 if i == 0 else act[i - 1]["h3"]))
        return act

    def _forward_kept(self):
        """Behind the embeddings (self.h0, self.key_mask2): layers 0 .. L-2 at R rows (activations kept in self.act), the top
        layer on its token-0 rows, LayerNorm + pooler."""
        R, B, H = self.R, self.B, self.H
        m1 = self.key_mask2[:B]
        top = self.nl - 1
        for i in range(top):
            a = self.act[i]
            self._layer_body(i, a["h_in"], R, B, a["qkv"], a["ctx"], a["lse"], a["h2"], a["h3"], st1=a["st1"], st2=a["st2"],
                             u=a["u"], mask=m1, ln1_done=False)
        a, W, t = self.act[top], self.layers[top], self.top
        x16 = self.x16[:R]
        L.layernorm_fwd(a["h_in"], W["ln1g"], W["ln1b"], self.ln_eps, R, H, y_bf16=x16, stats=a["st1"])
        L.gemm_bf16_nt(x16, W["wqkv"], L.EPI_BF16, bias=W["bqkv"], out_bf16=a["qkv"])
        L.attn_cls_fwd(a["qkv"], a["ctx"], a["lse"], B, self.S, self.heads, key_mask=m1)
        self._top_token0_fwd(a, W, B)
        self._pool(t["h3"], B, x_stride=H)

    # ------------------------------------------------------------------------------------------ backward
    def _backward_kept(self, colsum: Optional[Callable] = None, ln: Optional[Callable] = None, need_dh0: bool = True):
        """The dX chain through the frozen backbone: dpooled [B, H] -> the gradient of the residual stream entering layer 0
        (d h0, returned).  Each gradient tensor a per-column vector is trained from is offered to a tap as soon as it exists:
        colsum(key, x) for a bias behind x, ln(key, dy, x, stats) for a LayerNorm's parameters; keys (layer, "b2" | "b1" | "ln2" |
        "bo" | "bqkv" | "ln1") and "lnf".  need_dh0=False leaves out the last launch, layer 0's layernorm_before backward (nothing
        trainable below it): the returned buffer does not hold d h0 then."""
        colsum = colsum or (lambda key, x: None)
        ln = ln or (lambda key, dy, x, stats: None)
        R, B, H = self.R, self.B, self.H
        m1 = self.key_mask2[:B]
        top = self.nl - 1
        a, W, t = self.act[top], self.layers[top], self.top
        ws = self._skinny_ws()
        L.head_gemm(L.ht_job(self.dpooled, H, 1, self.pool_w, H, 1, B, H, H, self.dcls_ln, pro=L.HT_PRO_TANH_BWD,
                             pro_a=self.pooled, **self._scale_in()))
        ln("lnf", self.dcls_ln[:B], t["h3"], self.cls_st)
        dcls = self.dcls[:B]
        L.layernorm_bwd_dx(self._pool_src, self.cls_st, self.lnf_g, B, H, dy_f32=self.dcls_ln, x_stride=self._pool_stride,
                           out_f32=dcls)
        # ---- top layer: FFN, LN2 and the attention-output projection on the B token-0 rows
        colsum((top, "b2"), dcls)
        L.cvt_f32_bf16(dcls, t["dh316"][:B])
        L.gemm_bf16_nt(t["dh316"][:B], W["w2T"], L.EPI_MUL_DGELU, aux=t["u"], out_bf16=t["dU"], skinny_workspace=ws)
        colsum((top, "b1"), t["dU"][:B])
        L.gemm_bf16_nt(t["dU"], W["w1T"], L.EPI_BF16, out_bf16=t["dx2"], skinny_workspace=ws)
        ln((top, "ln2"), t["dx2"][:B], t["h2"], t["st2"])
        L.layernorm_bwd_dx(t["h2"], t["st2"], W["ln2g"], B, H, dy_bf16=t["dx2"], dres=dcls, out_f32=t["dh2"],
                           out_bf16=t["dh216"])
        colsum((top, "bo"), t["dh2"][:B])
        L.gemm_bf16_nt(t["dh216"], W["woT"], L.EPI_F32, out_f32=t["dctx"], skinny_workspace=ws)
        L.attn_cls_bwd(a["qkv"], a["ctx"], a["lse"], t["dctx"], self.dqkv, B, self.S, self.heads, key_mask=m1)
        dqkv, dx16, dh16 = self.dqkv[:R], self.dx16[:R], self.dh16[:R]
        colsum((top, "bqkv"), dqkv)
        L.gemm_bf16_nt(dqkv, W["wqkvT"], L.EPI_BF16, out_bf16=dx16)
        ln((top, "ln1"), dx16, a["h_in"], a["st1"])
        cur, oth = self.dh[0][:R], self.dh[1][:R]
        if top > 0 or need_dh0:
            L.layernorm_bwd_dx(a["h_in"], a["st1"], W["ln1g"], R, H, dy_bf16=dx16, dres=t["dh2"], dres_every=self.S, out_f32=cur)
        # ---- layers L-2 .. 0 at R rows; `cur` = gradient of the residual stream leaving layer i
        for i in range(top - 1, -1, -1):
            a, W = self.act[i], self.layers[i]
            colsum((i, "b2"), cur)
            L.cvt_f32_bf16(cur, dh16)
            L.gemm_bf16_nt(dh16, W["w2T"], L.EPI_MUL_G8 if self.g8u else L.EPI_MUL_DGELU, aux=a["u"], out_bf16=self.dU[:R])
            colsum((i, "b1"), self.dU[:R])
            L.gemm_bf16_nt(self.dU[:R], W["w1T"], L.EPI_BF16, out_bf16=dx16)
            ln((i, "ln2"), dx16, a["h2"], a["st2"])
            L.layernorm_bwd_dx(a["h2"], a["st2"], W["ln2g"], R, H, dy_bf16=dx16, dres=cur, out_f32=oth, out_bf16=dh16)
            colsum((i, "bo"), oth)
            L.gemm_bf16_nt(dh16, W["woT"], L.EPI_BF16, out_bf16=self.dctx[:R])
            L.attn_bwd(a["qkv"], a["ctx"], a["lse"], self.dctx[:R], dqkv, B, self.S, self.heads, key_mask=m1)
            colsum((i, "bqkv"), dqkv)
            L.gemm_bf16_nt(dqkv, W["wqkvT"], L.EPI_BF16, out_bf16=dx16)
            ln((i, "ln1"), dx16, a["h_in"], a["st1"])
            if i > 0 or need_dh0:
                L.layernorm_bwd_dx(a["h_in"], a["st1"], W["ln1g"], R, H, dy_bf16=dx16, dres=oth, out_f32=cur)
        return cur

    # ------------------------------------------------------------------------------------------ inference / state
    @_bound
    @torch.no_grad()
    def forward(self, batch: Dict[str, torch.Tensor], task: Optional[str] = None):
        """model(task_key, images, texts) -> (pooled, logits) of the engine's model (vilt.py:244-264): the step's own forward."""
        task = task or self.task
        self.set_batch(batch)
        self._forward_train()
        logits = self._head_fwd(self.pooled[:self.B], "all", task)
        return self.pooled[:self.n_valid].clone(), logits[:self.n_valid].clone()

    def comm_written(self):
        """Nothing to rebuild: the kernels read the fp32 tensors in place."""
