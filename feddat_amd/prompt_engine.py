"""ViLT-B/32 prompt-tuning FedAvg baseline (optimizer_mode 'prompt') on MI355X.

The reference (src/train/main.py:198-245, src/modeling/prompted_output.py:218-278) adds two modules to
vilt_encoder.vilt.embeddings, prompt_embedding_vis and prompt_embedding_text, each
Sequential(Embedding(5, 768), Linear(768, 192), Tanh(), Linear(192, 768)), and inserts the five rows
P = prompt_embedding_text(arange(5)) behind row 0 of the text embeddings AND behind row 0 (CLS) of the image embeddings -- the
image side reads the TEXT module too (prompted_output.py:254), prompt_embedding_vis is never read.  Masks get ones at the inserted
rows, the token-type embeddings are added afterwards.  The backbone is frozen, there is no adapter; trainable are every 'prompt'
key and the task heads.  The step is the non-dat train_step (task_trainer.py:433-450): one forward, loss = BCEWithLogits_mean * C,
one backward, one AdamW step over {prompt, head}, one scheduler tick.

Sequence frame (S = Lt + Np + 11 rows per sample; lib.prompt_row_map):
  0 text token 0 | 1..5 P[j] + type0 | 6..Lt+4 text tokens 1..Lt-1 | Lt+5 image CLS | Lt+6..Lt+10 P[j] + type1 | Lt+11.. patches

Launch list of a step (what differs from the bias step, vector_engine.ViltVectorEngine, at a 10-row longer sequence):
  forward   2 x feddat_head_gemm (the MLP: t = tanh(E W1^T + b1), P = t W2^T + b2), the backbone's embedding launches into
            staging buffers of S0 = Lt + 1 + Np rows, feddat_prompt_frame_assemble -> h0 / key mask at S rows, then the frozen
            forward of the vector engine (vector_engine.forward_kept_layers)
  backward  the vector engine's dX chain with no vector-gradient job, ALWAYS through layer 0's layernorm_before to d h0, then
            feddat_prompt_grad_gather (10 B rows -> G = dL/dP, unscaled, overflow-checked) and 2 x feddat_head_gemm of two
            products each (the MLP backward, written into the AdamW group's gradient slices)
  tail      the vector engine's: one multi-group AdamW, single_step_finish / step_tick_multi
Six launches more than a vector step without its column-sum jobs.

State: ONE allocation holds the ten prompt tensors in the reference's state-dict order (vis first); comm_flat() is that buffer
(599 424 floats).  The AdamW FlatGroup spans the five text tensors (its p is the second half of the buffer).  The vis tensors
never get a gradient in the reference, AdamW skips them entirely (weight decay included): they are inert payload here and stay
bit-identical to their initial values.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import lib as L
from .local_update import FlatGroup, _bound
from .modes import PROMPT_MODE
from .vector_engine import alloc_kept_layers, forward_kept_layers
from .vilt_backbone import ENC, ViltBackbone

PROMPT_LEN, PROMPT_DIM = L.PROMPT_ROWS, 192


def prompt_names(which: str, hidden: int = 768) -> List[Tuple[str, Tuple[int, ...]]]:
    """(state-dict key, shape) of the five tensors of prompt_embedding_<which> ("vis" | "text") in state-dict order."""
    p = ENC + f"embeddings.prompt_embedding_{which}."
    H, D, n = hidden, PROMPT_DIM, PROMPT_LEN
    return [(p + "0.weight", (n, H)), (p + "1.weight", (D, H)), (p + "1.bias", (D,)), (p + "3.weight", (H, D)),
            (p + "3.bias", (H,))]


class ViltPromptEngine(ViltBackbone):
    EXTRA_TOKENS = 2 * PROMPT_LEN

    def __init__(self, params: Dict[str, torch.Tensor], tasks: Sequence[str], device, batch: int, res: int,
                 mode: str = PROMPT_MODE, fp8: bool = False, max_patches: Optional[int] = None, **kw):
        """Arguments as ViltBackbone (operands "f16" -- the default, dynamic loss scale -- or "bf16"); fp8 and patch slots
        (max_patches) are not supported with prompts."""
        if mode != PROMPT_MODE:
            raise L.FeddatHipError(f"ViltPromptEngine runs optimizer_mode {PROMPT_MODE!r}, got {mode!r}")
        if fp8:
            raise L.FeddatHipError("optimizer_mode prompt runs with 16-bit operands only (fp8=True is a dat configuration)")
        if max_patches is not None:
            raise L.FeddatHipError("optimizer_mode prompt runs in the grid frame only (max_patches is not supported with prompts)")
        self.mode = mode
        super().__init__(params, tasks, device, batch, res, extra_tokens=self.EXTRA_TOKENS, **kw)
        self._init_prompt(params)

    @_bound
    def _init_prompt(self, params):
        dev, H, B = self.dev, self.H, self.B
        self.loss_out = torch.zeros(4, device=dev)
        # ---------------- the ten prompt tensors in one allocation, state-dict order (vis first): the FedAvg payload
        vis, text = prompt_names("vis", H), prompt_names("text", H)
        self.vis = FlatGroup(vis, dev, False)
        self.text = FlatGroup(text, dev, True)
        n = self.text.numel
        assert self.vis.numel == n and n % 4 == 0      # no quad padding: the two groups lie back to back
        self.comm = torch.zeros(2 * n, device=dev)
        self.vis.p, self.text.p = self.comm[:n], self.comm[n:]
        for grp in (self.vis, self.text):
            for k in grp.names:
                grp.view(k).copy_(params[k].to(dev, torch.float32))
        t = [k for k, _ in text]
        self._w = [self.text.view(k) for k in t]                       # E, W1, b1, W2, b2
        self._g = [self.text.view(k, self.text.g) for k in t]          # dE, dW1, db1, dW2, db2
        # ---------------- staging: the embeddings' own S0-row frame and key mask; the MLP's activations
        self.h_stage = self._f32(B * self.S0, H)
        self.mask_stage = torch.ones(self.NPASS * B, self.S0, dtype=torch.uint8, device=dev)
        self.pt = self._f32(PROMPT_LEN, PROMPT_DIM)      # t = tanh(E W1^T + b1), kept for the backward
        self.pP = self._f32(PROMPT_LEN, H)               # P
        self.pG = self._f32(PROMPT_LEN, H)               # dL/dP
        self.pdt = self._f32(PROMPT_LEN, PROMPT_DIM)
        self.act: List[dict] = alloc_kept_layers(self)

    # ------------------------------------------------------------------------------------------ forward
    def _forward_prompt(self):
        """Prompt MLP, embeddings into staging, the prompted frame, then the frozen forward."""
        E, W1, b1, W2, b2 = self._w
        L.prompt_mlp_fwd(E, W1, b1, W2, b2, self.pt, self.pP)
        self._embed(self.h_stage, self.mask_stage)
        L.prompt_frame_assemble(self.h_stage, self.mask_stage, self.pP, self.mod0, self.mod1, self.h0, self.key_mask2, self.B,
                                self.Lt, self.np, self.H, nrep=self.NPASS)
        forward_kept_layers(self)

    # ------------------------------------------------------------------------------------------ backward
    def _backward_prompt(self):
        """dpooled [B, H] -> d h0 (the vector engine's dX chain, no vector job, through layer 0) -> the gradient of the five
        text tensors (self.text.g)."""
        R, B, H = self.R, self.B, self.H
        m1 = self.key_mask2[:B]
        top = self.nl - 1
        a, W, t = self.act[top], self.layers[top], self.top
        ws = self._skinny_ws()
        L.head_gemm(L.ht_job(self.dpooled, H, 1, self.pool_w, H, 1, B, H, H, self.dcls_ln, pro=L.HT_PRO_TANH_BWD,
                             pro_a=self.pooled, **self._scale_in()))
        dcls = self.dcls[:B]
        L.layernorm_bwd_dx(self._pool_src, self.cls_st, self.lnf_g, B, H, dy_f32=self.dcls_ln, x_stride=self._pool_stride,
                           out_f32=dcls)
        # ---- top layer: FFN, LN2 and the attention-output projection on the B token-0 rows
        L.cvt_f32_bf16(dcls, t["dh316"][:B])
        L.gemm_bf16_nt(t["dh316"][:B], W["w2T"], L.EPI_MUL_DGELU, aux=t["u"], out_bf16=t["dU"], skinny_workspace=ws)
        L.gemm_bf16_nt(t["dU"], W["w1T"], L.EPI_BF16, out_bf16=t["dx2"], skinny_workspace=ws)
        L.layernorm_bwd_dx(t["h2"], t["st2"], W["ln2g"], B, H, dy_bf16=t["dx2"], dres=dcls, out_f32=t["dh2"],
                           out_bf16=t["dh216"])
        L.gemm_bf16_nt(t["dh216"], W["woT"], L.EPI_F32, out_f32=t["dctx"], skinny_workspace=ws)
        L.attn_cls_bwd(a["qkv"], a["ctx"], a["lse"], t["dctx"], self.dqkv, B, self.S, self.heads, key_mask=m1)
        dqkv, dx16, dh16 = self.dqkv[:R], self.dx16[:R], self.dh16[:R]
        L.gemm_bf16_nt(dqkv, W["wqkvT"], L.EPI_BF16, out_bf16=dx16)
        cur, oth = self.dh[0][:R], self.dh[1][:R]
        L.layernorm_bwd_dx(a["h_in"], a["st1"], W["ln1g"], R, H, dy_bf16=dx16, dres=t["dh2"], dres_every=self.S, out_f32=cur)
        # ---- layers L-2 .. 0 at R rows; `cur` = gradient of the residual stream leaving layer i
        for i in range(top - 1, -1, -1):
            a, W = self.act[i], self.layers[i]
            L.cvt_f32_bf16(cur, dh16)
            L.gemm_bf16_nt(dh16, W["w2T"], L.EPI_MUL_G8 if self.g8u else L.EPI_MUL_DGELU, aux=a["u"], out_bf16=self.dU[:R])
            L.gemm_bf16_nt(self.dU[:R], W["w1T"], L.EPI_BF16, out_bf16=dx16)
            L.layernorm_bwd_dx(a["h2"], a["st2"], W["ln2g"], R, H, dy_bf16=dx16, dres=cur, out_f32=oth, out_bf16=dh16)
            L.gemm_bf16_nt(dh16, W["woT"], L.EPI_BF16, out_bf16=self.dctx[:R])
            L.attn_bwd(a["qkv"], a["ctx"], a["lse"], self.dctx[:R], dqkv, B, self.S, self.heads, key_mask=m1)
            L.gemm_bf16_nt(dqkv, W["wqkvT"], L.EPI_BF16, out_bf16=dx16)
            L.layernorm_bwd_dx(a["h_in"], a["st1"], W["ln1g"], R, H, dy_bf16=dx16, dres=oth, out_f32=cur)
        # ---- cur = d h0: the ten prompt rows of every sample -> dL/dP (the loss scale leaves here), then the MLP backward
        if self._dyn():
            L.prompt_grad_gather(cur, B, self.S, self.Lt, H, self.pG, 1.0, self.scaler_f[1:2], self.ovf_flags[0:1])
        else:
            L.prompt_grad_gather(cur, B, self.S, self.Lt, H, self.pG, 1.0 / self.loss_scale)
        E, W1, _, W2, _ = self._w
        dE, dW1, db1, dW2, db2 = self._g
        L.prompt_mlp_bwd(self.pG, self.pt, E, W1, W2, self.pdt, dE, dW1, db1, dW2, db2)

    # ------------------------------------------------------------------------------------------ train step
    def _named_groups(self):
        return [(self.mode, self.text), ("head", self.head[self.task])]

    def _state_groups(self):
        return [self.vis, self.text] + list(self.head.values())

    def _graph_switches(self) -> Tuple:
        return super()._graph_switches() + (self.mode,)

    @_bound
    def begin_local_update(self, task: str, steps_per_epoch: int, num_epochs: int = 15, warmup_ratio: float = 0.1,
                           opt_adapters: Sequence[int] = ()):
        """TaskTrainer.train prologue (task_trainer.py:36-59 without the teacher copy): a fresh AdamW over {text prompt, head}
        and a fresh poly schedule over steps_per_epoch * num_epochs ticks (one tick per batch)."""
        self.task = task
        self._start_local_update(steps_per_epoch, num_epochs, warmup_ratio, {})

    @_bound
    def _step_kernels(self):
        B, task = self.B, self.task
        hp = self.head[task]
        if not (self.fused_tail and self.cls_attention):
            raise L.FeddatHipError("the prompt step runs on the fused step tail and the token-0 top layer only")
        self._forward_prompt()
        logits = self._head_fwd(self.pooled[:B], "all", task)
        flag = self.ovf_flags[0:1]
        if self.n_valid < B:      # a short batch: the loss of the n valid rows, zero gradient in the replica rows
            L.bce_loss_fwd_bwd_rows(logits, self.inp["target"], self.dlogits, self.loss_out, self.n_valid,
                                    flag if self._dyn() else None)
        else:
            L.bce_loss_fwd_bwd(logits, self.inp["target"], self.dlogits, self.loss_out, flag if self._dyn() else None)
        self._head_bwd(self.pooled[:B], "all", task, self.dpooled[:B])
        self._backward_prompt()
        skip = dict(skip_if=(flag,)) if self._dyn() else {}
        self._adamw_many([self._adamw_group(self.text, **skip), self._adamw_group(hp, **skip)])
        if self._dyn():
            L.single_step_finish([self.text.state, hp.state], flag, self.scaler_f, self.scaler_i, self.scale_growth,
                                 self.scale_backoff, self.scale_growth_interval)
        else:
            L.step_tick_multi([self.text.state, hp.state], [1, 1], [1, 1])

    def _loss_tensor(self):
        """What train_step returns (task_trainer.py:433-450): the device tensor whose [0] is loss = BCE_mean * num_labels."""
        return self.loss_out

    # ------------------------------------------------------------------------------------------ inference / state
    @_bound
    @torch.no_grad()
    def forward(self, batch: Dict[str, torch.Tensor], task: Optional[str] = None):
        """model(task_key, images, texts) -> (pooled, logits) of the prompted model: the step's own forward."""
        task = task or self.task
        self.set_batch(batch)
        self._forward_prompt()
        logits = self._head_fwd(self.pooled[:self.B], "all", task)
        return self.pooled[:self.n_valid].clone(), logits[:self.n_valid].clone()

    def load_state_dict(self, tensors: Dict[str, torch.Tensor]):
        """Copy tensors in under their state-dict keys (load_tensors: the kernels read the fp32 tensors in place)."""
        self.load_tensors(tensors)

    def comm_flat(self) -> torch.Tensor:
        """The FedAvg payload: all ten 'prompt' tensors back-to-back in state-dict order, vis first (main.py:243-245; no
        'prompt' key contains 'clf', so get_average_net averages every one of them)."""
        return self.comm

    def comm_written(self):
        """Nothing to rebuild: the kernels read the fp32 tensors in place."""
