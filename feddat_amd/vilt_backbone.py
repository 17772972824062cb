"""The frozen ViLT-B/32 backbone and the task head, as every ViLT local-update engine uses them on MI355X.

What the dual-adapter engine (engine.ViltDatEngine), the single-adapter engine (adapter_engine.ViltAdapterEngine), the bias /
LayerNorm-only engine (vector_engine.ViltVectorEngine) and the prompt engine (prompt_engine.ViltPromptEngine) share INSIDE a train_step: the geometry, the frozen weights as 16-bit MFMA
operands (+ transposes for the dX products), the task heads, the static input buffers, the embeddings, the body of one HF ViltLayer,
the token-0 block of the top layer, LayerNorm + pooler, the head's forward / backward, and the workspace all of this runs on.
What they share AROUND the step is local_update.LocalUpdateEngine.  An engine derived from ViltBackbone adds its own trainable
groups, says which layers' activations it keeps (_kept_layer), and sequences its own forward, backward and step.

No arithmetic happens in Python/PyTorch here: torch only owns the device buffers and the stream; every launch goes through the C ABI,
on static buffers, so a whole train_step can be captured into one hipGraph (torch.cuda.CUDAGraph stream capture) and replayed.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import lib as L
from .local_update import FlatGroup, LocalUpdateEngine, _bound

ENC = "vilt_encoder.vilt."
# longest sequence the attention kernels take (csrc/attention.hip, csrc/attention_cls.hip)
MAX_SEQ = 320
HEAD_TENSORS = ("clf_fc0.weight", "clf_fc0.bias", "clf_norm0.weight", "clf_norm0.bias", "clf_fc1.weight",
                "clf_fc1.bias")


class ViltBackbone(LocalUpdateEngine):
    # passes per sample batched through the backbone: sizes the shared workspace (NPASS * B samples, NPASS * R rows)
    NPASS = 1
    # state-dict stem of the FFN's second product: the plain HF ViltOutput key
    FFN2_STEM = "output.dense."

    def __init__(self, params: Dict[str, torch.Tensor], tasks: Sequence[str], device, batch: int, res: int,
                 text_len: int = 40, layers: int = 12, num_labels: int = 100, lr: float = 1e-4,
                 weight_decay: float = 1e-2, adam_eps: float = 1e-8, gelu_codes: bool = True, operands: Optional[str] = None,
                 loss_scale: Optional[float] = None, dynamic_loss_scale: Optional[bool] = None,
                 scale_growth_interval: int = 2000, max_patches: Optional[int] = None, extra_tokens: int = 0):
        """operands ("f16", the default, or "bf16"), loss_scale, dynamic_loss_scale, scale_growth_interval and gelu_codes: see
        engine.ViltDatEngine.
        max_patches (None: the grid frame, every cell of the res frame is a sequence position): the image half of the sequence
        holds max_patches PATCH SLOTS per sample, S = text_len + 1 + max_patches.  Each sample's valid patches (pixel_mask) are
        compacted into its slots in row-major order, as HF visual_embed does with max_image_length = -1, so a frame that holds
        portrait and landscape images (res up to 640 x 640) runs at the longest image's patch count (240).  A sample with more
        valid patches than slots raises FeddatHipError: in set_batch for a host pixel_mask, at the end-of-update check
        (assert_finite) for a device-resident one.
        extra_tokens (0: none): rows per sample that the engine itself inserts into the sequence behind the embeddings (prompt
        tuning: 10), S = text_len + 1 + patches + extra_tokens; self.S0 stays the embeddings' own row count."""
        self._init_loss_scale(operands or "f16", loss_scale, dynamic_loss_scale, scale_growth_interval)
        self._init_backbone(params, tasks, device, batch, res, text_len, layers, num_labels, lr, weight_decay, adam_eps,
                            gelu_codes, max_patches, extra_tokens)

    def _param(self, params, name):
        return params[name].to(self.dev, torch.float32).contiguous()

    def _f32(self, *s):
        return torch.empty(*s, device=self.dev)

    def _b16(self, *s):
        return torch.empty(*s, dtype=self.op_dtype, device=self.dev)

    @_bound
    def _init_backbone(self, params, tasks, device, batch, res, text_len, layers, num_labels, lr, weight_decay, adam_eps,
                       gelu_codes, max_patches=None, extra_tokens=0):
        L.load()
        self.dev = torch.device(device)
        self.tasks = list(tasks)
        self.B, self.Lt, self.nl = batch, text_len, layers
        self.res = (res, res) if isinstance(res, int) else tuple(res)      # (height, width), multiples of 32
        self.H, self.I, self.heads, self.C = 768, 3072, 12, num_labels
        self.P = 32
        self.gh, self.gw = self.res[0] // self.P, self.res[1] // self.P
        self.np = self.gh * self.gw
        # patch slots: self.np is the slot count (the patch matrix, the projection, the activations and the key mask shrink
        # with it); None: one sequence position per grid cell
        self.max_patches = None if max_patches is None else int(max_patches)
        if self.max_patches is not None:
            if not 1 <= self.max_patches <= self.gh * self.gw:
                raise L.FeddatHipError(f"max_patches must lie in 1 .. {self.gh * self.gw} (the {self.gh} x {self.gw} cells of "
                                       f"the {self.res[0]} x {self.res[1]} frame), got {max_patches}")
            if text_len + 1 + self.max_patches > MAX_SEQ:
                raise L.FeddatHipError(f"max_patches = {self.max_patches} makes sequences of {text_len + 1 + self.max_patches} "
                                       f"tokens; the attention kernels take at most {MAX_SEQ}")
            if max(self.gh, self.gw) > 64:
                raise L.FeddatHipError("a patch-slot frame holds at most 64 x 64 cells")
            self.np = self.max_patches
        # S0: the rows the embeddings write ([text | CLS | patches]); S: the sequence the layers run on
        self.extra_tokens = int(extra_tokens)
        self.S0 = text_len + 1 + self.np
        self.S = self.S0 + self.extra_tokens
        if self.extra_tokens < 0 or (self.extra_tokens and self.S > MAX_SEQ):
            raise L.FeddatHipError(f"extra_tokens = {extra_tokens} makes sequences of {self.S} tokens; the attention kernels "
                                   f"take at most {MAX_SEQ}")
        self.R = batch * self.S
        self.lr, self.wd, self.eps = lr, weight_decay, adam_eps
        self.ln_eps = 1e-12
        dev = self.dev
        H, I = self.H, self.I

        def P(name):
            return self._param(params, name)

        def bf16_of(w):
            out = torch.empty(w.shape, dtype=self.op_dtype, device=dev)
            L.cvt_f32_bf16(w, out)
            return out

        def bf16_T(w):  # [R,C] fp32 -> [C,R] bf16
            out = torch.empty(w.shape[1], w.shape[0], dtype=self.op_dtype, device=dev)
            L.transpose_f32_bf16(w, out, w.shape[0], w.shape[1])
            return out

        # ---------------- frozen backbone (bf16 weights + their transposes for the dX products) --------------
        e = ENC + "embeddings."
        self.emb = {k: P(e + k) for k in (
            "text_embeddings.word_embeddings.weight", "text_embeddings.position_embeddings.weight",
            "text_embeddings.token_type_embeddings.weight", "text_embeddings.LayerNorm.weight",
            "text_embeddings.LayerNorm.bias", "patch_embeddings.projection.bias")}
        tok = P(e + "token_type_embeddings.weight")
        self.mod0, self.mod1 = tok[0].contiguous(), tok[1].contiguous()
        self.cls = P(e + "cls_token").reshape(H).contiguous()
        pos = P(e + "position_embeddings")[0]
        self.pos0 = pos[0].contiguous()
        # per-sample position grids: the 12 x 12 table resized to each sample's valid patch rectangle (pixel_mask)
        self.pos_grid = pos[1:].contiguous()
        self.g0 = int(round(math.sqrt(pos.shape[0] - 1)))
        if self.max_patches is None:
            self.pos_img = torch.empty(batch, self.np, H, device=dev)
        self.w_patch = bf16_of(P(e + "patch_embeddings.projection.weight").reshape(H, 3 * self.P * self.P))
        self.layers: List[dict] = []
        for i in range(layers):
            Lp = ENC + f"encoder.layer.{i}."
            wq, wk, wv = (P(Lp + f"attention.attention.{n}.weight") for n in ("query", "key", "value"))
            wqkv = torch.cat([wq, wk, wv], 0).contiguous()
            bqkv = torch.cat([P(Lp + f"attention.attention.{n}.bias") for n in ("query", "key", "value")]).contiguous()
            wo, w1, w2 = P(Lp + "attention.output.dense.weight"), P(Lp + "intermediate.dense.weight"), \
                P(Lp + self.FFN2_STEM + "weight")
            self.layers.append(dict(
                wqkv=bf16_of(wqkv), wqkvT=bf16_T(wqkv), bqkv=bqkv,
                wo=bf16_of(wo), woT=bf16_T(wo), bo=P(Lp + "attention.output.dense.bias"),
                w1=bf16_of(w1), w1T=bf16_T(w1), b1=P(Lp + "intermediate.dense.bias"),
                w2=bf16_of(w2), w2T=bf16_T(w2), b2=P(Lp + self.FFN2_STEM + "bias"),
                ln1g=P(Lp + "layernorm_before.weight"), ln1b=P(Lp + "layernorm_before.bias"),
                ln2g=P(Lp + "layernorm_after.weight"), ln2b=P(Lp + "layernorm_after.bias")))
        self.lnf_g, self.lnf_b = P(ENC + "layernorm.weight"), P(ENC + "layernorm.bias")
        self.pool_w, self.pool_b = P(ENC + "pooler.dense.weight"), P(ENC + "pooler.dense.bias")

        # ---------------- trainable state every engine has: one head per task (an engine's adapters, if any, go into self.ad) ----
        self.ad: List[FlatGroup] = []
        self.opt_adapters: Tuple[int, ...] = ()
        head_shapes = {"clf_fc0.weight": (2 * H, H), "clf_fc0.bias": (2 * H,), "clf_norm0.weight": (2 * H,),
                       "clf_norm0.bias": (2 * H,), "clf_fc1.weight": (num_labels, 2 * H), "clf_fc1.bias": (num_labels,)}
        self.head = {t: FlatGroup([(f"task_layer.{t}.{n}", head_shapes[n]) for n in HEAD_TENSORS], dev, True)
                     for t in self.tasks}
        for grp in self.head.values():
            for n in grp.names:
                grp.view(n).copy_(params[n].to(dev, torch.float32))

        # ---------------- workspace (static: a whole step is graph-capturable) ----------------
        R, R2, B = self.R, self.NPASS * self.R, batch
        f32, b16 = self._f32, self._b16
        self._px_shape = (B, 3, self.res[0], self.res[1])
        self.inp = dict(input_ids=torch.zeros(B, text_len, dtype=torch.int64, device=dev),
                        token_type_ids=torch.zeros(B, text_len, dtype=torch.int64, device=dev),
                        target=f32(B, num_labels),
                        attention_mask=torch.ones(B, text_len, dtype=torch.int64, device=dev),
                        # pixel_mask sampled at the patch origins (all that HF's visual_embed looks at): [B, gh, gw]
                        patch_mask=torch.ones(B, self.gh, self.gw, dtype=torch.int64, device=dev))
        # attention key masks of the [text | CLS | patches] sequence, derived on the device from the two HF masks
        # inside the step (no host sync, valid for every batch under one captured graph); rows [B, 2B) repeat [0, B)
        self.key_mask2 = torch.ones(self.NPASS * B, self.S, dtype=torch.uint8, device=dev)
        self.patches = b16(B * self.np, 3 * self.P * self.P)
        if self.max_patches is not None:
            # raised by the slot kernel inside the step when a sample has more valid patches than slots (device-resident masks:
            # nobody reads them on the host); read and cleared by assert_finite
            self.slot_overflow = torch.zeros(1, dtype=torch.int32, device=dev)
            # what feddat_vilt_pad_batch moves in the patch matrix' place: the slot gather reads a short batch's replicas itself
            self._pad_stub = torch.zeros(B * self.gh * self.gw, 2, dtype=self.op_dtype, device=dev)
        self.proj = f32(B * self.np, H)
        self.h0 = f32(R, H)
        self.x16 = b16(R2, H)          # LN output (GEMM operand), transient
        self.f16 = b16(R2, I)          # gelu(u), transient
        # what FFN2^T needs of the pre-GELU u: 8-bit gelu'(u) codes where the persistent GEMM applies (FEDDAT_EPI_GELU_G8 /
        # _MUL_G8, M >= 1024: 25 % fewer bytes through the two HBM-bound epilogues), else u itself in bf16
        self.g8u = R2 >= 1024 and bool(gelu_codes)
        # top layer: only token 0 of each sample feeds the pooler, so everything after its attention runs on NPASS * B rows
        nb2 = self.NPASS * B
        self.top = dict(h2=f32(nb2, H), st2=f32(nb2, 2), u=b16(nb2, I), h3=f32(nb2, H), x16=b16(nb2, H),
                        f16=b16(nb2, I), dh316=b16(nb2, H), dU=b16(nb2, I), dx2=b16(nb2, H), dh2=f32(nb2, H),
                        dh216=b16(nb2, H), dctx=f32(nb2, H))
        # head / pooler
        self.cls_ln = f32(2 * B, H)
        self.cls_st = f32(2 * B, 2)
        self.pooled = f32(2 * B, H)
        # task-head activations: "both" = a 2B-row pass, "all" = its rows [0,B), "p1" = its rows [B,2B)
        both = dict(a0=f32(2 * B, 2 * H), n0=f32(2 * B, 2 * H), st=f32(2 * B, 2), g0=f32(2 * B, 2 * H),
                    logits=f32(2 * B, num_labels))
        self.hd = {"both": both, "all": {k: v[:B] for k, v in both.items()}, "p1": {k: v[B:] for k, v in both.items()}}
        self.dlogits = f32(B, num_labels)
        self.dg0, self.dn0, self.da0 = f32(B, 2 * H), f32(B, 2 * H), f32(B, 2 * H)
        self.dpooled = f32(2 * B, H)
        self.dpre = f32(2 * B, H)
        self.dcls_ln = f32(2 * B, H)
        self.dcls = f32(2 * B, H)
        # backward streams
        self.dh = [f32(R2, H), f32(R2, H)]       # ping-pong residual-gradient stream
        self.dh16 = b16(R2, H)
        self.dU = b16(R2, I)
        self.dx16 = b16(R2, H)
        self.dctx = b16(R2, H)
        self.dqkv = b16(R2, 3 * H)
        self.graph = None
        # samples of the B-sample frame that the staged batch really holds (set_batch); B = a full batch
        self.n_valid = batch
        self.ctx = L.Context(self.dev.index if self.dev.index is not None else torch.cuda.current_device())
        # True: the serial tail (token-0 LayerNorm + pooler, task head forward / backward, loss, optimizer bookkeeping) on the
        # fused kernels of csrc/head_tail.hip (20 launches); False: the round-3 sequence of 46 single-purpose launches (same
        # arithmetic up to fp32 summation order; tools/step_breakdown.py --unfused-tail, and the tests compare the two)
        self.fused_tail = True
        # True: the last layer's attention computes the ONE query per (sample, head) the pooler consumes (token 0) and its
        # rank-1 backward (feddat_attn_cls_fwd / _bwd); False: the dense kernels on all S queries (184 of 185 never read)
        self.cls_attention = True
        self.sched = dict(warmup=1, total=2)
        self.task = self.tasks[0]
        # dynamic loss scale (GradScaler on the device)
        self._alloc_scaler()

    def _kept_layer(self, h_in=None):
        """The buffers of ONE layer's activations that its backward reads, NPASS * R rows each.  h_in: the layer's input where it
        already lives somewhere (the previous layer's h3); None: a buffer of the layer's own.  FFN2^T needs of the pre-GELU u
        only what self.g8u says: the 8-bit gelu' codes, else u itself in 16 bits."""
        R2, H, I = self.NPASS * self.R, self.H, self.I
        f32, b16 = self._f32, self._b16
        return dict(h_in=f32(R2, H) if h_in is None else h_in, st1=f32(R2, 2), qkv=b16(R2, 3 * H), ctx=b16(R2, H),
                    lse=f32(self.NPASS * self.B, self.heads, self.S), h2=f32(R2, H), st2=f32(R2, 2),
                    u=torch.empty(R2, I, dtype=torch.uint8, device=self.dev) if self.g8u else b16(R2, I), h3=f32(R2, H))

    # ------------------------------------------------------------------------------------------ inputs
    @_bound
    def set_batch(self, batch: Dict[str, torch.Tensor]):
        """Copy one batch (reference schema: HF ViLT encodings + target_scores) into the static input buffers.  A batch of
        n < B samples (the last batch of a loader that does not drop it) is staged into samples [0, n) of the B-sample frame and
        samples [n, B) become copies of samples j mod n; self.n_valid = n."""
        px = batch["pixel_values"]
        n = int(px.shape[0]) if px.dim() == 4 else 0
        if px.dim() != 4 or tuple(px.shape[1:]) != self._px_shape[1:] or not 1 <= n <= self.B:
            raise L.FeddatHipError(f"engine built for pixel_values {self._px_shape} (or fewer samples: a short last batch), "
                                   f"got {tuple(px.shape)}")
        # the pixels are consumed right here, from the caller's tensor: patch extraction (im2col + bf16) is the only reader of
        # pixel_values, so it runs ahead of the captured step instead of a 57 MB device-to-device copy into a static buffer
        # followed by the same read inside the graph (stream-ordered with the replay that follows)
        if not px.is_cuda:
            px = px.to(self.dev, non_blocking=True)
        if self.max_patches is not None:
            self._set_batch_slots(batch, px, n)
            return
        L.im2col_patches(px.to(torch.float32).contiguous(), self.patches, n, 3, self.res[0], self.res[1], self.P)
        self._stage_small_inputs(batch, n)
        if n < self.B:
            L.vilt_pad_batch(self.patches, self.inp, n, self.B)
        self.n_valid = n

    def _set_batch_slots(self, batch, px, n: int):
        """set_batch in a patch-slot frame: the masks first (the gather needs every sample's valid rectangle, the replicas'
        too), then only the slot patches leave the pixels.  A host pixel_mask is checked against the slot budget here; a
        device-resident one by the step's own kernel (self.slot_overflow)."""
        pm = batch.get("pixel_mask")
        if pm is not None and not pm.is_cuda:
            from .vilt_spec import patch_slot_plan
            _, counts, over = patch_slot_plan(pm[:, ::self.P, ::self.P], self.max_patches)
            if bool(over.any()):
                b = int(over.nonzero()[0])
                raise L.FeddatHipError(f"sample {b} has {int(counts[b])} valid patches; the engine was built with max_patches = "
                                       f"{self.max_patches} slots per sample")
        self._stage_small_inputs(batch, n)
        if n < self.B:
            L.vilt_pad_batch(self._pad_stub, self.inp, n, self.B)
        L.im2col_patches_slots(px.to(torch.float32).contiguous(), self.inp["patch_mask"], self.patches, n, self.B, 3, self.res[0],
                               self.res[1], self.P, self.max_patches)
        self.n_valid = n

    def check_patch_slots(self):
        """Raise if a batch since the last check held a sample with more valid patches than slots (one 4-byte read-back; the
        flag is cleared, so training can go on with in-budget batches).  No-op in the grid frame."""
        if self.max_patches is not None and int(self.slot_overflow.item()) != 0:
            self.slot_overflow.zero_()
            raise L.FeddatHipError(f"a sample had more valid patches than the engine's max_patches = {self.max_patches} slots: its "
                                   "patches behind the budget were dropped from the sequence -- build the engine with more slots "
                                   "(the ViLT size rule yields at most 240 patches)")

    def _extra_step_state(self) -> List[torch.Tensor]:
        """The slot-budget flag is raised inside the step: capturing (a warm-up and a capture run on whatever is staged) puts it
        back like the rest of the step's state."""
        return super()._extra_step_state() + ([self.slot_overflow] if self.max_patches is not None else [])

    def assert_finite(self):
        self.check_patch_slots()
        super().assert_finite()

    def nonfinite_groups(self) -> List[str]:
        """LocalUpdateEngine.nonfinite_groups; a sample over the slot budget is reported here too (and the flag cleared), so
        that the ranks of train.main agree on it before the FedAvg collective like on a non-finite group."""
        bad = super().nonfinite_groups()
        if self.max_patches is not None and int(self.slot_overflow.item()) != 0:
            self.slot_overflow.zero_()
            bad.append(f"patch slots (a sample had more valid patches than max_patches = {self.max_patches})")
        return bad

    def _stage_small_inputs(self, batch, n: int):
        """input_ids, token_type_ids, attention_mask, target_scores and pixel_mask of n samples -> samples [0, n) of self.inp."""
        ids, tts, am, tg, pm = (batch.get(k) for k in ("input_ids", "token_type_ids", "attention_mask", "target_scores",
                                                        "pixel_mask"))

        def dev_ok(t, dt, shape):
            return t is None or (t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == shape)
        Lt = self.Lt
        if (ids is not None and tts is not None and dev_ok(ids, torch.int64, (n, Lt)) and dev_ok(tts, torch.int64, (n, Lt))
                and dev_ok(am, torch.int64, (n, Lt)) and dev_ok(tg, torch.float32, (n, self.C))
                and dev_ok(pm, torch.int64, (n, self.res[0], self.res[1]))):
            # the usual case (device-resident batch in the reference's dtypes): one launch for all five
            L.vilt_stage_inputs(ids, tts, am, tg, pm, self.inp, n, Lt, self.C, self.res[0], self.res[1], self.P)
            return
        inp = {k: v[:n] for k, v in self.inp.items()}
        for k in ("input_ids", "token_type_ids", "attention_mask", "target_scores", "pixel_mask"):
            if batch.get(k) is not None and batch[k].shape[0] != n:
                raise L.FeddatHipError(f"pixel_values has {n} samples but {k} has {batch[k].shape[0]}")
        inp["input_ids"].copy_(batch["input_ids"], non_blocking=True)
        inp["token_type_ids"].copy_(batch["token_type_ids"], non_blocking=True)
        if "target_scores" in batch:
            inp["target"].copy_(batch["target_scores"], non_blocking=True)
        if batch.get("attention_mask") is not None:     # absent = all valid
            inp["attention_mask"].copy_(batch["attention_mask"], non_blocking=True)
        else:
            inp["attention_mask"].fill_(1)
        if batch.get("pixel_mask") is not None:
            inp["patch_mask"].copy_(batch["pixel_mask"][:, ::self.P, ::self.P], non_blocking=True)
        else:
            inp["patch_mask"].fill_(1)

    # ------------------------------------------------------------------------------------------ forward
    def _embed(self, h=None, key_mask=None):
        """The embeddings' [text | CLS | patches] rows (S0 per sample) and their key mask, into the sequence frame itself
        (extra_tokens = 0) or into the staging buffers `h` [B * S0, H] / `key_mask` [NPASS * B, S0] of an engine that inserts rows."""
        B, H, S, Lt = self.B, self.H, self.S0, self.Lt
        h = self.h0 if h is None else h
        key_mask = self.key_mask2 if key_mask is None else key_mask
        e = self.emb
        L.text_embed(self.inp["input_ids"], self.inp["token_type_ids"], e["text_embeddings.word_embeddings.weight"],
                     e["text_embeddings.position_embeddings.weight"], e["text_embeddings.token_type_embeddings.weight"],
                     e["text_embeddings.LayerNorm.weight"], e["text_embeddings.LayerNorm.bias"], self.ln_eps,
                     self.mod0, h, B, Lt, S, H)
        # (self.patches was filled by set_batch: im2col of the caller's pixel_values)
        L.gemm_bf16_nt(self.patches, self.w_patch, L.EPI_F32, bias=e["patch_embeddings.projection.bias"],
                       out_f32=self.proj)
        if self.max_patches is not None:      # patch slots: key mask + position value at each slot's cell + assembly + budget check
            L.image_embed_assemble_slots(self.proj, self.cls, self.pos0, self.pos_grid, self.inp["patch_mask"],
                                         self.inp["attention_mask"], self.mod1, h, key_mask, self.slot_overflow, B,
                                         Lt, self.gh, self.gw, self.max_patches, self.g0, H, nrep=self.NPASS)
            return
        if self.fused_tail:      # key mask + per-sample position grid + assembly in one launch (bit-identical)
            L.image_embed_assemble_masked(self.proj, self.cls, self.pos0, self.pos_grid, self.inp["patch_mask"],
                                          self.inp["attention_mask"], self.mod1, h, key_mask, B, Lt, self.gh,
                                          self.gw, self.g0, H, nrep=self.NPASS)
            return
        L.vilt_key_mask(self.inp["attention_mask"], self.inp["patch_mask"], key_mask, B, Lt, self.gh, self.gw, 1,
                        nrep=self.NPASS)
        L.pos_embed_resize_masked(self.pos_grid, self.inp["patch_mask"], self.pos_img, self.g0, B, self.gh, self.gw, 1,
                                  H)
        L.image_embed_assemble(self.proj, self.cls, self.pos0, self.pos_img, self.mod1, h, B, Lt, self.np, S, H,
                               pos_batch_stride=self.np * H)

    def _layer_body(self, i: int, h_in, rows: int, nb: int, qkv, ctx, lse, h2, h3, st1=None, st2=None, u=None,
                    mask=None, ln1_done=False):
        """LN -> QKV -> attention -> out-proj(+res) -> LN -> FFN1(gelu) -> FFN2(+res): HF ViltLayer (with an adapter behind it,
        the Adaptered_ViltOutput dense+residual: adaptered_output.py:74-76, and h3 is the adapter's input)."""
        W, H = self.layers[i], self.H
        x16, f16 = self.x16[:rows], self.f16[:rows]
        g8 = u is not None and u.dtype == torch.uint8
        if not ln1_done:     # otherwise x16 / st1 were written by the previous layer's fused adapter + LN kernel
            L.layernorm_fwd(h_in, W["ln1g"], W["ln1b"], self.ln_eps, rows, H, y_bf16=x16, stats=st1)
        L.gemm_bf16_nt(x16, W["wqkv"], L.EPI_BF16, bias=W["bqkv"], out_bf16=qkv)
        L.attn_fwd(qkv, ctx, lse, nb, self.S, self.heads, key_mask=mask)
        L.gemm_bf16_nt(ctx, W["wo"], L.EPI_RESID_F32, bias=W["bo"], resid=h_in, out_f32=h2)
        L.layernorm_fwd(h2, W["ln2g"], W["ln2b"], self.ln_eps, rows, H, y_bf16=x16, stats=st2)
        L.gemm_bf16_nt(x16, W["w1"], L.EPI_GELU_G8 if g8 else L.EPI_GELU, bias=W["b1"], out_bf16=f16, out2_bf16=u)
        L.gemm_bf16_nt(f16, W["w2"], L.EPI_RESID_F32, bias=W["b2"], resid=h2, out_f32=h3)

    def _sg(self, A, sa_i, sa_k, Bm, sb_k, sb_j, I, J, K, out, ksplit=1, bias_j=None, alpha=1.0):
        """Skinny exact-fp32 product; long contractions are split over the grid and reduced deterministically."""
        if ksplit <= 1:
            L.sgemm_f32(A, sa_i, sa_k, Bm, sb_k, sb_j, I, J, K, out, bias_j=bias_j, alpha=alpha)
            return
        part = self._scratch1(ksplit * I * J)
        L.sgemm_f32(A, sa_i, sa_k, Bm, sb_k, sb_j, I, J, K, part, ksplit=ksplit, bias_j=bias_j,
                    out_split_stride=I * J, alpha=alpha)
        L.reduce_partials(part, I * J, ksplit, I * J, out)

    def _scratch1(self, n):
        if not hasattr(self, "_scr") or self._scr.numel() < n:
            self._scr = torch.empty(n, device=self.dev)
        return self._scr

    def _cls_rows(self, t, nb: int):
        """Strided view of token 0 of every sample: [nb, width] with row stride S * width (no copy)."""
        w = t.shape[1]
        return t.view(nb, self.S * w)[:, :w]

    def _top_token0_fwd(self, a, W, nb: int):
        """The top layer behind its attention, on the nb token-0 rows (only token 0 of each sample reaches the pooler: HF
        ViltPooler takes hidden_states[:, 0]; vilt.py:127), read in place through strided GEMM operands: attention-output
        projection (+ residual), LN2, FFN1 + GELU, FFN2 (+ residual) -> self.top["h3"]."""
        H, t = self.H, self.top
        L.gemm_bf16_nt(self._cls_rows(a["ctx"], nb), W["wo"], L.EPI_RESID_F32, bias=W["bo"],
                       resid=self._cls_rows(a["h_in"], nb), out_f32=t["h2"], skinny_workspace=self._skinny_ws())
        L.layernorm_fwd(t["h2"], W["ln2g"], W["ln2b"], self.ln_eps, nb, H, y_bf16=t["x16"], stats=t["st2"])
        L.gemm_bf16_nt(t["x16"], W["w1"], L.EPI_GELU, bias=W["b1"], out_bf16=t["f16"], out2_bf16=t["u"],
                       skinny_workspace=self._skinny_ws())
        L.gemm_bf16_nt(t["f16"], W["w2"], L.EPI_RESID_F32, bias=W["b2"], resid=t["h2"], out_f32=t["h3"],
                       skinny_workspace=self._skinny_ws())

    def _skinny_ws(self):
        """fp32 split-K partials of the top layer's 2B-row GEMMs (largest: 2B x 3072 x 768)."""
        if getattr(self, "_skws", None) is None:
            nb, H, I = self.NPASS * self.B, self.H, self.I
            n = max(L.gemm_skinny_workspace_elems(nb, I, H), L.gemm_skinny_workspace_elems(nb, H, I),
                    L.gemm_skinny_workspace_elems(nb, H, H), L.gemm_skinny_workspace_elems(nb, H, 3 * H)) if nb <= 64 else 0
            self._skws = torch.empty(max(n, 1), device=self.dev) if n else False
        return self._skws if self._skws is not False else None

    def _pool(self, h_last, nb: int, x_stride: int = None):
        """ViltModel.layernorm on token 0 + ViltPooler (dense + tanh) -> self.pooled[:nb]."""
        H = self.H
        self._pool_src, self._pool_stride = h_last, (self.S * H if x_stride is None else x_stride)
        if self.fused_tail:      # LayerNorm (statistics in the block) -> dense -> tanh in one launch
            L.head_gemm(L.ht_job(h_last, self._pool_stride, 1, self.pool_w, 1, H, nb, H, H, self.pooled, bias_j=self.pool_b,
                                 pro=L.HT_PRO_LN, pro_a=self.lnf_g, pro_b=self.lnf_b, pro_eps=self.ln_eps,
                                 stats_out=self.cls_st, epi=L.HT_EPI_TANH))
            return
        L.layernorm_fwd(h_last, self.lnf_g, self.lnf_b, self.ln_eps, nb, H, x_stride=self._pool_stride,
                        y_f32=self.cls_ln, stats=self.cls_st)
        self._sg(self.cls_ln, H, 1, self.pool_w, 1, H, nb, H, H, self.pooled, ksplit=4, bias_j=self.pool_b)
        L.tanh_fwd(self.pooled[:nb])

    def _head_fwd(self, pooled, slot: str, task: str):
        """vilt.py:202-209: fc0 -> LayerNorm(1536, eps 1e-5) -> GELU -> fc1 on the rows of `pooled` (B, or 2B for the
        joint P0 + P1 pass)."""
        B, H, C = pooled.shape[0], self.H, self.C
        hp, s = self.head[task], self.hd[slot]
        pre = f"task_layer.{task}."
        if self.fused_tail:
            L.head_gemm(L.ht_job(pooled, H, 1, hp.view(pre + "clf_fc0.weight"), 1, H, B, 2 * H, H, s["a0"],
                                 bias_j=hp.view(pre + "clf_fc0.bias")))
            L.head_ln_gelu(s["a0"], hp.view(pre + "clf_norm0.weight"), hp.view(pre + "clf_norm0.bias"), 1e-5, s["n0"], s["st"],
                           s["g0"])
            L.head_gemm(L.ht_job(s["g0"], 2 * H, 1, hp.view(pre + "clf_fc1.weight"), 1, 2 * H, B, C, 2 * H, s["logits"],
                                 bias_j=hp.view(pre + "clf_fc1.bias")))
            return s["logits"]
        self._sg(pooled, H, 1, hp.view(pre + "clf_fc0.weight"), 1, H, B, 2 * H, H, s["a0"], ksplit=4,
                 bias_j=hp.view(pre + "clf_fc0.bias"))
        L.layernorm_fwd(s["a0"], hp.view(pre + "clf_norm0.weight"), hp.view(pre + "clf_norm0.bias"), 1e-5, B, 2 * H,
                        y_f32=s["n0"], stats=s["st"])
        L.gelu_fwd(s["n0"], s["g0"])
        self._sg(s["g0"], 2 * H, 1, hp.view(pre + "clf_fc1.weight"), 1, 2 * H, B, C, 2 * H, s["logits"], ksplit=16,
                 bias_j=hp.view(pre + "clf_fc1.bias"))
        return s["logits"]

    def _head_bwd(self, pooled, slot: str, task: str, dpooled_out):
        """Gradients of the task head (all six tensors, fp32) and d(pooled) for B rows."""
        B, H, C = self.B, self.H, self.C
        hp, s = self.head[task], self.hd[slot]
        pre = f"task_layer.{task}."

        def G(n):
            return hp.view(pre + n, hp.g)
        dl = self.dlogits
        if self.fused_tail:
            # {dW_fc1 = dl^T g0, db_fc1} next to {dn0 = (dl W_fc1) * gelu'(n0)}; LayerNorm backward (dx, dgamma, dbeta);
            # {dW_fc0 = da0^T pooled, db_fc0} next to {dpooled = da0 W_fc0}: three launches
            L.head_gemm(L.ht_job(dl, 1, C, s["g0"], 2 * H, 1, C, 2 * H, B, G("clf_fc1.weight"), mode=1, colsum=G("clf_fc1.bias")),
                        L.ht_job(dl, C, 1, hp.view(pre + "clf_fc1.weight"), 2 * H, 1, B, 2 * H, C, self.dn0,
                                 epi=L.HT_EPI_MUL_DGELU, aux=s["n0"], ld_aux=2 * H))
            L.head_ln_bwd_full(self.dn0, s["a0"], s["st"], hp.view(pre + "clf_norm0.weight"), self.da0, G("clf_norm0.weight"),
                               G("clf_norm0.bias"))
            L.head_gemm(L.ht_job(self.da0, 1, 2 * H, pooled, H, 1, 2 * H, H, B, G("clf_fc0.weight"), mode=1,
                                 colsum=G("clf_fc0.bias")),
                        L.ht_job(self.da0, 2 * H, 1, hp.view(pre + "clf_fc0.weight"), H, 1, B, H, 2 * H, dpooled_out))
            return
        L.sgemm_f32(dl, 1, C, s["g0"], 2 * H, 1, C, 2 * H, B, G("clf_fc1.weight"), colsum=G("clf_fc1.bias"))
        L.sgemm_f32(dl, C, 1, hp.view(pre + "clf_fc1.weight"), 2 * H, 1, B, 2 * H, C, self.dg0)
        L.gelu_bwd(s["n0"], self.dg0, self.dn0)
        L.layernorm_bwd_full(self.dn0, s["a0"], s["st"], hp.view(pre + "clf_norm0.weight"), B, 2 * H, self.da0,
                             G("clf_norm0.weight"), G("clf_norm0.bias"))
        L.sgemm_f32(self.da0, 1, 2 * H, pooled, H, 1, 2 * H, H, B, G("clf_fc0.weight"), colsum=G("clf_fc0.bias"))
        self._sg(self.da0, 2 * H, 1, hp.view(pre + "clf_fc0.weight"), H, 1, B, H, 2 * H, dpooled_out, ksplit=8)

    def _adamw(self, grp: FlatGroup):
        """One group's AdamW as its own launch (the unfused tail)."""
        L.adamw_flat(grp.p, grp.g, grp.m, grp.v, grp.seg_off, self._wd_vec(grp), grp.state, self.lr,
                     self.sched["warmup"], self.sched["total"], 0.9, 0.98, self.eps)

    def _dyn(self) -> bool:
        """Dynamic loss scale in effect (it rides on the fused tail's multi-group AdamW launch)."""
        return self.dynamic_scale and self.fused_tail

    def _scale_in(self):
        """How the loss scale enters the backbone's backward (factor of the pooler-backward product); it leaves through
        _scale_out."""
        return dict(alpha=1.0, alpha_dev=self.scaler_f[0:1]) if self._dyn() else dict(alpha=self.loss_scale)

    def _graph_switches(self) -> Tuple:
        return (self.task, self.fused_tail, self.cls_attention)

    def _state_groups(self):
        return self.ad + list(self.head.values())
