"""ViLT-B/32 prompt-tuning FedAvg baseline (optimizer_mode 'prompt') on MI355X.

The reference (src/train/main.py:198-245, src/modeling/prompted_output.py:218-278) adds two modules to
vilt_encoder.vilt.embeddings, prompt_embedding_vis and prompt_embedding_text, each
Sequential(Embedding(5, 768), Linear(768, 192), Tanh(), Linear(192, 768)), and inserts the five rows
P = prompt_embedding_text(arange(5)) behind row 0 of the text embeddings AND behind row 0 (CLS) of the image embeddings -- the
image side reads the TEXT module too (prompted_output.py:254), prompt_embedding_vis is never read.  Masks get ones at the inserted
rows, the token-type embeddings are added afterwards.  The backbone is frozen, there is no adapter; trainable are every 'prompt'
key and the task heads.  The step is the non-dat train_step (task_trainer.py:433-450): one forward, loss = BCEWithLogits_mean * C,
one backward, one AdamW step over {prompt, head}, one scheduler tick (single_pass.SinglePassStep, shared with the adapter and
bias / norm engines).

Sequence frame (S = Lt + Np + 11 rows per sample; lib.prompt_row_map):
  0 text token 0 | 1..5 P[j] + type0 | 6..Lt+4 text tokens 1..Lt-1 | Lt+5 image CLS | Lt+6..Lt+10 P[j] + type1 | Lt+11.. patches

Launch list of a step (what differs from the bias step, vector_engine.ViltVectorEngine, at a 10-row longer sequence):
  forward   2 x feddat_head_gemm (the MLP: t = tanh(E W1^T + b1), P = t W2^T + b2), the backbone's embedding launches into
            staging buffers of S0 = Lt + 1 + Np rows, feddat_prompt_frame_assemble -> h0 / key mask at S rows, then the frozen
            forward both engines inherit (single_pass.ViltFrozenEngine._forward_kept)
  backward  the shared dX chain (ViltFrozenEngine._backward_kept) with no tap, ALWAYS through layer 0's layernorm_before to
            d h0, then feddat_prompt_grad_gather (10 B rows -> G = dL/dP, unscaled, overflow-checked) and 2 x feddat_head_gemm
            of two products each (the MLP backward, written into the AdamW group's gradient slices)
  tail      the shared step's: one multi-group AdamW, one launch for the counters (and the dynamic scale)
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
from .single_pass import ViltFrozenEngine
from .vilt_backbone import ENC

PROMPT_LEN, PROMPT_DIM = L.PROMPT_ROWS, 192


def prompt_names(which: str, hidden: int = 768) -> List[Tuple[str, Tuple[int, ...]]]:
    """(state-dict key, shape) of the five tensors of prompt_embedding_<which> ("vis" | "text") in state-dict order."""
    p = ENC + f"embeddings.prompt_embedding_{which}."
    H, D, n = hidden, PROMPT_DIM, PROMPT_LEN
    return [(p + "0.weight", (n, H)), (p + "1.weight", (D, H)), (p + "1.bias", (D,)), (p + "3.weight", (H, D)),
            (p + "3.bias", (H,))]


class ViltPromptEngine(ViltFrozenEngine):
    EXTRA_TOKENS = 2 * PROMPT_LEN

    def __init__(self, params: Dict[str, torch.Tensor], tasks: Sequence[str], device, batch: int, res: int,
                 mode: str = PROMPT_MODE, fp8: bool = False, max_patches: Optional[int] = None, **kw):
        """Arguments as single_pass.ViltFrozenEngine; patch slots (max_patches) are not supported with prompts."""
        if mode != PROMPT_MODE:
            raise L.FeddatHipError(f"ViltPromptEngine runs optimizer_mode {PROMPT_MODE!r}, got {mode!r}")
        if max_patches is not None:
            raise L.FeddatHipError("optimizer_mode prompt runs in the grid frame only (max_patches is not supported with prompts)")
        super().__init__(params, tasks, device, batch, res, mode, fp8, extra_tokens=self.EXTRA_TOKENS, **kw)
        self._init_prompt(params)

    @_bound
    def _init_prompt(self, params):
        dev, H, B = self.dev, self.H, self.B
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
        self.act: List[dict] = self._alloc_kept()

    # ------------------------------------------------------------------------------------------ forward / backward
    def _forward_train(self):
        """Prompt MLP, embeddings into staging, the prompted frame, then the frozen forward."""
        E, W1, b1, W2, b2 = self._w
        L.prompt_mlp_fwd(E, W1, b1, W2, b2, self.pt, self.pP)
        self._embed(self.h_stage, self.mask_stage)
        L.prompt_frame_assemble(self.h_stage, self.mask_stage, self.pP, self.mod0, self.mod1, self.h0, self.key_mask2, self.B,
                                self.Lt, self.np, self.H, nrep=self.NPASS)
        self._forward_kept()

    def _backward_train(self):
        """dpooled [B, H] -> d h0 (the frozen dX chain, no tap, through layer 0) -> the gradient of the five text tensors
        (self.text.g)."""
        B, H = self.B, self.H
        cur = self._backward_kept()
        # ---- cur = d h0: the ten prompt rows of every sample -> dL/dP (the loss scale leaves here), then the MLP backward
        if self._dyn():
            L.prompt_grad_gather(cur, B, self.S, self.Lt, H, self.pG, 1.0, self.scaler_f[1:2], self.ovf_flags[0:1])
        else:
            L.prompt_grad_gather(cur, B, self.S, self.Lt, H, self.pG, 1.0 / self.loss_scale)
        E, W1, _, W2, _ = self._w
        dE, dW1, db1, dW2, db2 = self._g
        L.prompt_mlp_bwd(self.pG, self.pt, E, W1, W2, self.pdt, dE, dW1, db1, dW2, db2)

    # ------------------------------------------------------------------------------------------ state
    def _trained(self):
        return self.mode, self.text

    def _state_groups(self):
        return [self.vis, self.text] + list(self.head.values())

    def load_state_dict(self, tensors: Dict[str, torch.Tensor]):
        """Copy tensors in under their state-dict keys (load_tensors: the kernels read the fp32 tensors in place)."""
        self.load_tensors(tensors)

    def comm_flat(self) -> torch.Tensor:
        """The FedAvg payload: all ten 'prompt' tensors back-to-back in state-dict order, vis first (main.py:243-245; no
        'prompt' key contains 'clf', so get_average_net averages every one of them)."""
        return self.comm
