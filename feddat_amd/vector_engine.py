"""ViLT-B/32 bias-only (BitFit) and LayerNorm-only FedAvg baselines (optimizer_mode 'bias' / 'norm') on MI355X.

The reference's non-dat train_step (src/train/visionlanguage_tasks/task_trainer.py:433-450) on the plain HF backbone -- no adapter
anywhere -- with requires_grad on every parameter whose name contains 'bias' resp. 'norm' plus the task head (main.py:176-196,
246-250): one forward, loss = BCEWithLogits_mean * C, one backward, one AdamW step over {vectors, head}, one scheduler tick.

The step (single_pass.SinglePassStep), the frozen forward at R = B * S rows and the dX chain of the backward THROUGH layer 0
(single_pass.ViltFrozenEngine: the dual-adapter engine's kernels without the adapter) are shared with the prompt engine; this
engine owns the vectors and hangs its taps into the chain, so that after each gradient tensor exists its per-column vector
gradient is taken
(csrc/vector_grad.hip: feddat_colsum_partial / feddat_ln_param_grad_partial into per-vector partial buffers, then ONE
feddat_vector_grad_reduce per step that unscales by the device-side 1 / loss-scale and feeds the overflow flag):

  gradient tensor (per layer)                                vector
  d h3       residual stream entering the layer, fp32        output.dense.bias
  dU         at FFN1's pre-activation, 16-bit                intermediate.dense.bias
  dx16       at LN2's output (FFN1^T), with h2, st2          layernorm_after   (beta; gamma in 'norm')
  d h2       residual stream after the LN2 backward, fp32    attention.output.dense.bias
  dqkv       dq | dk | dv, 16-bit [R, 2304]                  query | key | value .bias (adjacent in the group: one sum)
  dx16       at LN1's output (QKV^T), with h_in, st1         layernorm_before
  and once: dcls_ln -> vilt.layernorm; the pooler's pre-tanh gradient -> pooler.dense.bias (formed above the point where the
  loss scale enters the backward: FEDDAT_VGRAD_UNSCALED); in 'bias' mode d h0 -> text_embeddings.LayerNorm.bias (text-token
  rows) and patch_embeddings.projection.bias (image-patch rows; every patch row of h0 is proj + position + type, padded ones
  included, and a padded row's gradient is exactly zero because it is masked as a key and never pooled).

The last layer runs the backbone's token-0 path with no adapter behind it (only token 0 reaches the pooler): its FFN / LN2 /
attention-output gradients live on the B token-0 rows and are summed over those rows only.  'norm' mode stops after layer
0's layernorm_before (nothing trainable below).

The trainable vectors live in ONE FlatGroup; the frozen-weight entries the kernels read (layers[i]["bqkv"], ["bo"], ["b1"],
["b2"], ["ln1g"] ..., the embedding / pooler entries) are VIEWS into that group's p, so AdamW updates them in place and the
GEMM epilogues read the new values with no repack.  comm_flat() is that group: 0.42 MB ('bias') / 0.15 MB ('norm').
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import torch

from . import lib as L
from .local_update import FlatGroup, _bound
from .modes import VECTOR_MODES
from .single_pass import ViltFrozenEngine
from .vilt_backbone import ENC


def vector_names(mode: str, layers: int, hidden: int = 768, inter: int = 3072) -> List[Tuple[str, Tuple[int, ...]]]:
    """(state-dict key, shape) of the trainable backbone vectors of `mode`, in the order they lie in the engine's group
    (query | key | value adjacent: the kernels read them as one [2304] bias)."""
    H, I = hidden, inter
    out: List[Tuple[str, Tuple[int, ...]]] = []
    e = ENC + "embeddings."
    if mode == "bias":
        out += [(e + "text_embeddings.LayerNorm.bias", (H,)), (e + "patch_embeddings.projection.bias", (H,))]
    for i in range(layers):
        Lp = ENC + f"encoder.layer.{i}."
        if mode == "bias":
            out += [(Lp + f"attention.attention.{n}.bias", (H,)) for n in ("query", "key", "value")]
            out += [(Lp + "attention.output.dense.bias", (H,)), (Lp + "intermediate.dense.bias", (I,)),
                    (Lp + "output.dense.bias", (H,)), (Lp + "layernorm_before.bias", (H,)), (Lp + "layernorm_after.bias", (H,))]
        else:
            out += [(Lp + f"{ln}.{t}", (H,)) for ln in ("layernorm_before", "layernorm_after") for t in ("weight", "bias")]
    if mode == "bias":
        out += [(ENC + "layernorm.bias", (H,)), (ENC + "pooler.dense.bias", (H,))]
    else:
        out += [(ENC + "layernorm.weight", (H,)), (ENC + "layernorm.bias", (H,))]
    return out


class ViltVectorEngine(ViltFrozenEngine):
    def __init__(self, params: Dict[str, torch.Tensor], tasks: Sequence[str], device, batch: int, res: int, mode: str = "bias",
                 fp8: bool = False, **kw):
        """mode: "bias" | "norm"; other arguments as single_pass.ViltFrozenEngine."""
        if mode not in VECTOR_MODES:
            raise L.FeddatHipError(f"ViltVectorEngine runs optimizer_mode {VECTOR_MODES}, got {mode!r}")
        super().__init__(params, tasks, device, batch, res, mode, fp8, **kw)
        self._init_vectors(params)

    @_bound
    def _init_vectors(self, params):
        dev, H, I, R, B, nl = self.dev, self.H, self.I, self.R, self.B, self.nl
        bias = self.mode == "bias"
        # ---------------- the trainable vectors: one flat group, the kernels' frozen entries become views into it
        self.vec = FlatGroup(vector_names(self.mode, nl, H, I), dev, True)
        for n in self.vec.names:
            self.vec.view(n).copy_(params[n].to(dev, torch.float32))
        v = self.vec.view

        def span(first, n):      # n floats of the group's p starting at tensor `first`
            o = self.vec.offsets[first]
            return self.vec.p[o:o + n]
        for i, W in enumerate(self.layers):
            Lp = ENC + f"encoder.layer.{i}."
            if bias:
                W["bqkv"] = span(Lp + "attention.attention.query.bias", 3 * H)
                W["bo"], W["b1"], W["b2"] = v(Lp + "attention.output.dense.bias"), v(Lp + "intermediate.dense.bias"), \
                    v(Lp + "output.dense.bias")
            else:
                W["ln1g"], W["ln2g"] = v(Lp + "layernorm_before.weight"), v(Lp + "layernorm_after.weight")
            W["ln1b"], W["ln2b"] = v(Lp + "layernorm_before.bias"), v(Lp + "layernorm_after.bias")
        self.lnf_b = v(ENC + "layernorm.bias")
        if bias:
            e = ENC + "embeddings."
            self.emb["text_embeddings.LayerNorm.bias"] = v(e + "text_embeddings.LayerNorm.bias")
            self.emb["patch_embeddings.projection.bias"] = v(e + "patch_embeddings.projection.bias")
            self.pool_b = v(ENC + "pooler.dense.bias")
        else:
            self.lnf_g = v(ENC + "layernorm.weight")
        self.act: List[dict] = self._alloc_kept()
        # static row masks of h0's [text | cls | patches] rows
        s = torch.arange(self.S, device=dev).repeat(B)
        self.text_rows = (s < self.Lt).to(torch.uint8).contiguous()
        self.patch_rows = (s > self.Lt).to(torch.uint8).contiguous()
        # ---------------- vector-gradient jobs: one partial buffer per (gradient tensor -> vector), one reduce per step
        self._jobs: List[tuple] = []
        self._part: Dict[tuple, tuple] = {}
        top = nl - 1

        def job(key, rows, first, n, gamma=None, flags=0):
            """Partial buffer(s) of the sum over `rows` rows into the n floats of the group's g at tensor `first` (and, for a
            LayerNorm in 'norm' mode, the dgamma partials into tensor `gamma`)."""
            elems = L.vector_grad_workspace_elems(rows, n)
            o = self.vec.offsets[first]
            pb = torch.zeros(elems, device=dev)
            self._jobs.append((pb, elems // n, self.vec.g[o:o + n], flags))
            pg = None
            if gamma is not None:
                og = self.vec.offsets[gamma]
                pg = torch.zeros(elems, device=dev)
                self._jobs.append((pg, elems // n, self.vec.g[og:og + n], flags))
            self._part[key] = (pb, pg)
        for i in range(nl):
            Lp = ENC + f"encoder.layer.{i}."
            rows_top = B if i == top else R      # the top layer's FFN / LN2 / attention-output gradients: token-0 rows only
            if bias:
                job((i, "b2"), rows_top, Lp + "output.dense.bias", H)
                job((i, "b1"), rows_top, Lp + "intermediate.dense.bias", I)
                job((i, "bo"), rows_top, Lp + "attention.output.dense.bias", H)
                job((i, "bqkv"), R, Lp + "attention.attention.query.bias", 3 * H)
            job((i, "ln2"), rows_top, Lp + "layernorm_after.bias", H, None if bias else Lp + "layernorm_after.weight")
            job((i, "ln1"), R, Lp + "layernorm_before.bias", H, None if bias else Lp + "layernorm_before.weight")
        job("lnf", B, ENC + "layernorm.bias", H, None if bias else ENC + "layernorm.weight")
        if bias:
            job("pool", B, ENC + "pooler.dense.bias", H, flags=L.VGRAD_UNSCALED)
            job("text", R, ENC + "embeddings.text_embeddings.LayerNorm.bias", H)
            job("patch", R, ENC + "embeddings.patch_embeddings.projection.bias", H)
        self._job_table = L.make_vgrad_jobs(self._jobs, dev)

    # ------------------------------------------------------------------------------------------ vector gradients
    def _colsum(self, key, x, row_mask=None):
        L.colsum_partial(x, self._part[key][0], row_mask=row_mask)

    def _ln_grads(self, key, dy, x, stats):
        pb, pg = self._part[key]
        L.ln_param_grad_partial(dy, x, stats, pb, pg)

    def _reduce_vectors(self):
        table, n, max_n = self._job_table
        if self._dyn():
            L.vector_grad_reduce(table, n, max_n, 1.0, self.scaler_f[1:2], self.ovf_flags[0:1])
        else:
            L.vector_grad_reduce(table, n, max_n, 1.0 / self.loss_scale)

    # ------------------------------------------------------------------------------------------ forward / backward
    def _forward_train(self):
        """Embeddings, layers 0 .. L-2 at R rows (activations kept), the top layer on its token-0 rows, LayerNorm + pooler."""
        self._embed()
        self._forward_kept()

    def _backward_train(self):
        """dpooled [B, H] -> the gradient of every trainable vector (self.vec.g)."""
        B = self.B
        bias = self.mode == "bias"
        if bias:      # the pooler's pre-tanh gradient (the loss scale enters below it)
            L.tanh_bwd(self.pooled[:B], self.dpooled[:B], self.dpre[:B])
            self._colsum("pool", self.dpre[:B])
        # 'norm': no bias to sum for, and nothing trainable below layer 0's layernorm_before
        cur = self._backward_kept(self._colsum if bias else None, self._ln_grads, need_dh0=bias)
        if bias:      # cur = d h0: the text LayerNorm's beta over the text rows, the patch projection's bias over the patch rows
            self._colsum("text", cur, row_mask=self.text_rows)
            self._colsum("patch", cur, row_mask=self.patch_rows)
        self._reduce_vectors()

    # ------------------------------------------------------------------------------------------ state
    def _trained(self):
        return self.mode, self.vec

    def _state_groups(self):
        return [self.vec] + list(self.head.values())

    def comm_flat(self) -> torch.Tensor:
        """The FedAvg payload: every trainable backbone vector back-to-back (the heads' own 'bias' / 'norm' keys are in the
        reference's communicated list too, but get_average_net skips every 'clf' key: main.py:54)."""
        return self.vec.p[:self.vec.numel]      # without FlatGroup's quad padding (none at these sizes)
