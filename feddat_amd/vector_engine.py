"""ViLT-B/32 bias-only (BitFit) and LayerNorm-only FedAvg baselines (optimizer_mode 'bias' / 'norm') on MI355X.

The reference's non-dat train_step (src/train/visionlanguage_tasks/task_trainer.py:433-450) on the plain HF backbone -- no adapter
anywhere -- with requires_grad on every parameter whose name contains 'bias' resp. 'norm' plus the task head (main.py:176-196,
246-250): one forward, loss = BCEWithLogits_mean * C, one backward, one AdamW step over {vectors, head}, one scheduler tick.

The frozen forward is vilt_backbone.ViltBackbone's at R = B * S rows and the dX chain of the backward is the dual-adapter
engine's kernels (engine.py) without the adapter; what is new is that the backward runs THROUGH layer 0 and that after each
gradient tensor exists its per-column vector gradient is taken
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

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import lib as L
from .local_update import FlatGroup, _bound
from .modes import VECTOR_MODES
from .vilt_backbone import ENC, ViltBackbone


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


def alloc_kept_layers(eng: ViltBackbone) -> List[dict]:
    """The activations an adapter-less engine keeps for its backward: every layer at R rows, layer 0 included; no adapter
    between the layers, so layer i reads layer i - 1's output in place (shared with prompt_engine.ViltPromptEngine)."""
    act: List[dict] = []
    for i in range(eng.nl):
        act.append(eng._kept_layer(h_in=eng.h0 if i == 0 else act[i - 1]["h3"]))
    return act


def forward_kept_layers(eng: ViltBackbone):
    """Behind the embeddings (eng.h0, eng.key_mask2): layers 0 .. L-2 at R rows (activations kept in eng.act), the top layer on
    its token-0 rows, LayerNorm + pooler (shared with prompt_engine.ViltPromptEngine)."""
    R, B, H = eng.R, eng.B, eng.H
    m1 = eng.key_mask2[:B]
    top = eng.nl - 1
    for i in range(top):
        a = eng.act[i]
        eng._layer_body(i, a["h_in"], R, B, a["qkv"], a["ctx"], a["lse"], a["h2"], a["h3"], st1=a["st1"], st2=a["st2"],
                        u=a["u"], mask=m1, ln1_done=False)
    a, W, t = eng.act[top], eng.layers[top], eng.top
    x16 = eng.x16[:R]
    L.layernorm_fwd(a["h_in"], W["ln1g"], W["ln1b"], eng.ln_eps, R, H, y_bf16=x16, stats=a["st1"])
    L.gemm_bf16_nt(x16, W["wqkv"], L.EPI_BF16, bias=W["bqkv"], out_bf16=a["qkv"])
    L.attn_cls_fwd(a["qkv"], a["ctx"], a["lse"], B, eng.S, eng.heads, key_mask=m1)
    eng._top_token0_fwd(a, W, B)
    eng._pool(t["h3"], B, x_stride=H)


class ViltVectorEngine(ViltBackbone):
    def __init__(self, params: Dict[str, torch.Tensor], tasks: Sequence[str], device, batch: int, res: int, mode: str = "bias",
                 fp8: bool = False, **kw):
        """mode: "bias" | "norm"; other arguments as ViltBackbone (operands "f16" -- the default, dynamic loss scale -- or
        "bf16"); fp8 is not supported."""
        if mode not in VECTOR_MODES:
            raise L.FeddatHipError(f"ViltVectorEngine runs optimizer_mode {VECTOR_MODES}, got {mode!r}")
        if fp8:
            raise L.FeddatHipError(f"optimizer_mode {mode} runs with 16-bit operands only (fp8=True is a dat configuration)")
        self.mode = mode
        super().__init__(params, tasks, device, batch, res, **kw)
        self._init_vectors(params)

    @_bound
    def _init_vectors(self, params):
        dev, H, I, R, B, nl = self.dev, self.H, self.I, self.R, self.B, self.nl
        bias = self.mode == "bias"
        self.loss_out = torch.zeros(4, device=dev)
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
        # ---------------- activations kept for the backward: every layer at R rows, layer 0 included; no adapter between the
        # layers, so layer i reads layer i - 1's output in place
        self.act: List[dict] = alloc_kept_layers(self)
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

    # ------------------------------------------------------------------------------------------ forward
    def _forward_plain(self):
        """Embeddings, layers 0 .. L-2 at R rows (activations kept), the top layer on its token-0 rows, LayerNorm + pooler."""
        self._embed()
        forward_kept_layers(self)

    # ------------------------------------------------------------------------------------------ backward
    def _backward_plain(self):
        """dpooled [B, H] -> the gradient of every trainable vector (self.vec.g)."""
        R, B, H = self.R, self.B, self.H
        bias = self.mode == "bias"
        m1 = self.key_mask2[:B]
        top = self.nl - 1
        a, W, t = self.act[top], self.layers[top], self.top
        ws = self._skinny_ws()
        if bias:      # the pooler's pre-tanh gradient (the loss scale enters below it)
            L.tanh_bwd(self.pooled[:B], self.dpooled[:B], self.dpre[:B])
            self._colsum("pool", self.dpre[:B])
        L.head_gemm(L.ht_job(self.dpooled, H, 1, self.pool_w, H, 1, B, H, H, self.dcls_ln, pro=L.HT_PRO_TANH_BWD,
                             pro_a=self.pooled, **self._scale_in()))
        self._ln_grads("lnf", self.dcls_ln[:B], t["h3"], self.cls_st)
        dcls = self.dcls[:B]
        L.layernorm_bwd_dx(self._pool_src, self.cls_st, self.lnf_g, B, H, dy_f32=self.dcls_ln, x_stride=self._pool_stride,
                           out_f32=dcls)
        # ---- top layer: FFN, LN2 and the attention-output projection on the B token-0 rows
        if bias:
            self._colsum((top, "b2"), dcls)
        L.cvt_f32_bf16(dcls, t["dh316"][:B])
        L.gemm_bf16_nt(t["dh316"][:B], W["w2T"], L.EPI_MUL_DGELU, aux=t["u"], out_bf16=t["dU"], skinny_workspace=ws)
        if bias:
            self._colsum((top, "b1"), t["dU"][:B])
        L.gemm_bf16_nt(t["dU"], W["w1T"], L.EPI_BF16, out_bf16=t["dx2"], skinny_workspace=ws)
        self._ln_grads((top, "ln2"), t["dx2"][:B], t["h2"], t["st2"])
        L.layernorm_bwd_dx(t["h2"], t["st2"], W["ln2g"], B, H, dy_bf16=t["dx2"], dres=dcls, out_f32=t["dh2"],
                           out_bf16=t["dh216"])
        if bias:
            self._colsum((top, "bo"), t["dh2"][:B])
        L.gemm_bf16_nt(t["dh216"], W["woT"], L.EPI_F32, out_f32=t["dctx"], skinny_workspace=ws)
        L.attn_cls_bwd(a["qkv"], a["ctx"], a["lse"], t["dctx"], self.dqkv, B, self.S, self.heads, key_mask=m1)
        dqkv, dx16, dh16 = self.dqkv[:R], self.dx16[:R], self.dh16[:R]
        if bias:
            self._colsum((top, "bqkv"), dqkv)
        L.gemm_bf16_nt(dqkv, W["wqkvT"], L.EPI_BF16, out_bf16=dx16)
        self._ln_grads((top, "ln1"), dx16, a["h_in"], a["st1"])
        cur, oth = self.dh[0][:R], self.dh[1][:R]
        if top > 0 or bias:
            L.layernorm_bwd_dx(a["h_in"], a["st1"], W["ln1g"], R, H, dy_bf16=dx16, dres=t["dh2"], dres_every=self.S, out_f32=cur)
        # ---- layers L-2 .. 0 at R rows; `cur` = gradient of the residual stream leaving layer i
        for i in range(top - 1, -1, -1):
            a, W = self.act[i], self.layers[i]
            if bias:
                self._colsum((i, "b2"), cur)
            L.cvt_f32_bf16(cur, dh16)
            L.gemm_bf16_nt(dh16, W["w2T"], L.EPI_MUL_G8 if self.g8u else L.EPI_MUL_DGELU, aux=a["u"], out_bf16=self.dU[:R])
            if bias:
                self._colsum((i, "b1"), self.dU[:R])
            L.gemm_bf16_nt(self.dU[:R], W["w1T"], L.EPI_BF16, out_bf16=dx16)
            self._ln_grads((i, "ln2"), dx16, a["h2"], a["st2"])
            L.layernorm_bwd_dx(a["h2"], a["st2"], W["ln2g"], R, H, dy_bf16=dx16, dres=cur, out_f32=oth, out_bf16=dh16)
            if bias:
                self._colsum((i, "bo"), oth)
            L.gemm_bf16_nt(dh16, W["woT"], L.EPI_BF16, out_bf16=self.dctx[:R])
            L.attn_bwd(a["qkv"], a["ctx"], a["lse"], self.dctx[:R], dqkv, B, self.S, self.heads, key_mask=m1)
            if bias:
                self._colsum((i, "bqkv"), dqkv)
            L.gemm_bf16_nt(dqkv, W["wqkvT"], L.EPI_BF16, out_bf16=dx16)
            self._ln_grads((i, "ln1"), dx16, a["h_in"], a["st1"])
            if i > 0 or bias:      # 'norm': nothing trainable below layer 0's layernorm_before
                L.layernorm_bwd_dx(a["h_in"], a["st1"], W["ln1g"], R, H, dy_bf16=dx16, dres=oth, out_f32=cur)
        if bias:      # cur = d h0: the text LayerNorm's beta over the text rows, the patch projection's bias over the patch rows
            self._colsum("text", cur, row_mask=self.text_rows)
            self._colsum("patch", cur, row_mask=self.patch_rows)
        self._reduce_vectors()

    # ------------------------------------------------------------------------------------------ train step
    def _named_groups(self):
        return [(self.mode, self.vec), ("head", self.head[self.task])]

    def _state_groups(self):
        return [self.vec] + list(self.head.values())

    def _graph_switches(self) -> Tuple:
        return super()._graph_switches() + (self.mode,)

    @_bound
    def begin_local_update(self, task: str, steps_per_epoch: int, num_epochs: int = 15, warmup_ratio: float = 0.1,
                           opt_adapters: Sequence[int] = ()):
        """TaskTrainer.train prologue (task_trainer.py:36-59 without the teacher copy): a fresh AdamW over {vectors, head} and a
        fresh poly schedule over steps_per_epoch * num_epochs ticks (one tick per batch)."""
        self.task = task
        self._start_local_update(steps_per_epoch, num_epochs, warmup_ratio, {})

    @_bound
    def _step_kernels(self):
        B, task = self.B, self.task
        hp = self.head[task]
        if not (self.fused_tail and self.cls_attention):
            raise L.FeddatHipError(f"the {self.mode} step runs on the fused step tail and the token-0 top layer only")
        self._forward_plain()
        logits = self._head_fwd(self.pooled[:B], "all", task)
        flag = self.ovf_flags[0:1]
        if self.n_valid < B:      # a short batch: the loss of the n valid rows, zero gradient in the replica rows
            L.bce_loss_fwd_bwd_rows(logits, self.inp["target"], self.dlogits, self.loss_out, self.n_valid,
                                    flag if self._dyn() else None)
        else:
            L.bce_loss_fwd_bwd(logits, self.inp["target"], self.dlogits, self.loss_out, flag if self._dyn() else None)
        self._head_bwd(self.pooled[:B], "all", task, self.dpooled[:B])
        self._backward_plain()
        skip = dict(skip_if=(flag,)) if self._dyn() else {}
        self._adamw_many([self._adamw_group(self.vec, **skip), self._adamw_group(hp, **skip)])
        if self._dyn():
            L.single_step_finish([self.vec.state, hp.state], flag, self.scaler_f, self.scaler_i, self.scale_growth,
                                 self.scale_backoff, self.scale_growth_interval)
        else:
            L.step_tick_multi([self.vec.state, hp.state], [1, 1], [1, 1])

    def _loss_tensor(self):
        """What train_step returns (task_trainer.py:433-450): the device tensor whose [0] is loss = BCE_mean * num_labels."""
        return self.loss_out

    # ------------------------------------------------------------------------------------------ inference / state
    @_bound
    @torch.no_grad()
    def forward(self, batch: Dict[str, torch.Tensor], task: Optional[str] = None):
        """model(task_key, images, texts) -> (pooled, logits) of the adapter-less model (vilt.py:244-264): the step's own forward."""
        task = task or self.task
        self.set_batch(batch)
        self._forward_plain()
        logits = self._head_fwd(self.pooled[:self.B], "all", task)
        return self.pooled[:self.n_valid].clone(), logits[:self.n_valid].clone()

    def comm_flat(self) -> torch.Tensor:
        """The FedAvg payload: every trainable backbone vector back-to-back (the heads' own 'bias' / 'norm' keys are in the
        reference's communicated list too, but get_average_net skips every 'clf' key: main.py:54)."""
        return self.vec.p[:self.vec.numel]      # without FlatGroup's quad padding (none at these sizes)

    def comm_written(self):
        """Nothing to rebuild: the kernels read the fp32 vectors in place."""
