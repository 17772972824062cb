"""ViLT-B/32 dual-adapter (DAT) local-update engine on MI355X.

Host-side sequencing of the HIP kernels in libfeddat_hip.so for the reference's hot path
(src/train/visionlanguage_tasks/task_trainer.py:266-330 around src/modeling/vilt.py:244-264 and
src/modeling/models/adapter.py:124-163).  No arithmetic happens in Python/PyTorch here: torch only owns the
device buffers and the stream; every launch goes through the C ABI, on static buffers, so a whole train_step
can be captured into one hipGraph (torch.cuda.CUDAGraph stream capture) and replayed.

Restructuring relative to the reference (same results, fewer FLOPs -- DESIGN.md "step algebra"):
  * P0 (no-grad gated forward) and P2 (gated forward with grad) see identical backbone inputs and identical
    adapter_0/adapter_2 weights (P1 only updates adapter_1 and the task head), so the gated backbone forward is
    run ONCE and its pooled output feeds both the P0 logits (old head) and the P2 logits (updated head).
  * Embeddings and the body of layer 0 (everything below the first adapter) are shared by the gated and the
    adapter_1 pass; from the layer-0 adapter on, the two passes ride in ONE batch of 2*B*S rows through the
    frozen GEMMs / attention (rows [0,R) gated, rows [R,2R) adapter_1).
  * Nothing trainable lies below the layer-0 adapter, so the backward stops there.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from . import lib as L
from .local_update import FlatGroup, _bound
from .vilt_backbone import ENC, HEAD_TENSORS, ViltBackbone  # noqa: F401 -- ENC / HEAD_TENSORS are imported from here

ADAPTER_TENSORS = ("down.weight", "down.bias", "up.weight", "up.bias")


class ViltDatEngine(ViltBackbone):
    # passes per sample through the backbone: the DAT step runs the gated and the adapter_1 pass as one batch of 2 B samples
    NPASS = 2
    # state-dict stems of the engine's adapters (adapter.py:22-58): slot a <-> "...output.adapter.<stem>{down,up}.{weight,bias}"
    ADAPTER_STEMS = ("adapter_0_", "adapter_1_", "adapter_2_")
    # state-dict stem of the FFN's second product: Adaptered_ViltOutput keeps the HF ViltOutput as `.layer` (adaptered_output.py)
    FFN2_STEM = "output.layer.dense."

    def __init__(self, params: Dict[str, torch.Tensor], tasks: Sequence[str], device, batch: int, res: int,
                 text_len: int = 40, layers: int = 12, num_labels: int = 100, lr: float = 1e-4,
                 weight_decay: float = 1e-2, adam_eps: float = 1e-8, wgrad_splits: int = 16, fp8: bool = False,
                 fp8_ffn_chain: bool = True, gelu_codes: bool = True, operands: Optional[str] = None,
                 loss_scale: Optional[float] = None, fp8_mx_dqkv: bool = True, dynamic_loss_scale: Optional[bool] = None,
                 scale_growth_interval: int = 2000, max_patches: Optional[int] = None):
        """operands: "f16" (the default) or "bf16" (the default with fp8=True, configs[4]).  "f16": every 16-bit MFMA operand of the step -- frozen weights and their transposes, LayerNorm outputs,
        qkv, probabilities, ctx, gelu(u), the adapters' operand copies, and every gradient operand of the dX products and of
        the attention backward -- is IEEE half instead of bf16 (libfeddat_hip_f16.so: v_mfma_f32_16x16x32_f16, the same MFMA
        rate and the same bytes; 10 instead of 7 mantissa bits, i.e. the reference's own GPU arithmetic, fp16 autocast:
        accelerate_config.yaml:8).  The backward then carries a power-of-two `loss_scale` (default 2^14; 1 for bf16): the
        gradient entering the backbone (d pooler-input) is multiplied by it where it is produced, every kernel of the backward
        is linear in the gradient, and the factor leaves exactly where the adapter weight gradients are formed
        (feddat_wgrad_seg.scale); the task head's own gradients never see it.  The scaled gradients of this path span
        1e-4 .. 1e1 at the default, eleven binades inside either end of fp16's range.
        dynamic_loss_scale (default: on with "f16" operands): the reference's GradScaler (accelerate, mixed_precision fp16:
        accelerate_config.yaml:8; task_trainer.py:302-308,323-328) ON THE DEVICE, inside the captured step -- `loss_scale` is
        only the initial value (GradScaler's own is 65536); a non-finite adapter gradient (the checked weight-gradient reduce)
        or loss (feddat_dat_loss_fwd_bwd_checked) skips that sub-step's optimizer AND scheduler step and halves the scale,
        `scale_growth_interval` clean sub-steps double it (feddat_dat_step_finish; DESIGN.md section 5b says where this
        differs from GradScaler: an overflow in sub-step A voids the whole batch).  With no overflow the step is bit-identical
        to the static scale.  A fresh scaler per local update, like the reference's fresh Accelerator per round (main.py:435).
        fp8=True (BASELINE.json configs[4]): four frozen products per layer run on the block-scaled fp8 MFMA with e4m3
        operands -- forward QKV and FFN1 (activations quantised per token row by the LayerNorm kernel that produces them) and
        the dX products FFN2^T and attention-output^T (the gradient rows quantised per row: by feddat_quant_rows_fp8 behind the
        adapter backward, by the LayerNorm backward itself); weights quantised once here per output channel of each product.
        Everything else -- adapters, attention, the products whose A operand comes out of a GEMM or attention epilogue --
        stays bf16 / fp32.
        gelu_codes=False: the backward of FFN2 reads the pre-GELU activation u in bf16 instead of the 8-bit gelu' codes
        (FEDDAT_EPI_GELU / _MUL_DGELU instead of _GELU_G8 / _MUL_G8; middle layers issued op by op).  25 % more bytes through
        the two heaviest epilogues (+0.14 ms/step at configs[1]); at B = 32 it takes the worst adapter element after an 80-step
        round from 1.31e-3 to 1.00e-3 and the worst update-norm error from 2.9 % to 1.6 % -- for callers
        that trade 2 % of throughput for that.
        max_patches: patch slots instead of the grid frame (vilt_backbone.ViltBackbone); 16-bit operands only."""
        if fp8 and max_patches is not None:
            raise L.FeddatHipError("fp8=True takes the grid frame only (max_patches=None): configs[4] is a B = 64 configuration "
                                   "with sequence limits of its own")
        operands = operands or ("bf16" if fp8 else "f16")
        if fp8 and operands != "bf16":
            raise L.FeddatHipError("fp8=True (configs[4]) pairs the e4m3 products with bf16 operands")
        # fp8 (round 5): the attention backward writes dq | dk | dv as MX-scaled e4m3 (one E8M0 scale per (row, 32 columns):
        # feddat_attn_bwd_fp8mx) and QKV^T runs on the block-scaled fp8 MFMA with those scales (feddat_gemm_fp8mx_nt): the seventh
        # of the eight frozen products per layer, and half the bytes of the backward's largest write
        self.fp8_mx_dqkv = bool(fp8) and bool(fp8_mx_dqkv)
        super().__init__(params, tasks, device, batch, res, text_len, layers, num_labels, lr, weight_decay, adam_eps, gelu_codes,
                         operands, loss_scale, dynamic_loss_scale, scale_growth_interval, max_patches)
        self._init_dat(params, wgrad_splits, fp8, fp8_ffn_chain, gelu_codes)

    @_bound
    def _init_dat(self, params, wgrad_splits, fp8, fp8_ffn_chain, gelu_codes):
        """What the dual-adapter step owns on top of the backbone: the adapters, their workspace, the fp8 copies."""
        dev, H, I, layers = self.dev, self.H, self.I, self.nl
        self.r = 48
        self.fp8 = bool(fp8)
        self.fp8_ffn_chain = bool(fp8_ffn_chain)      # fp8: also FFN2 forward and FFN1^T (their A operands leave as e4m3)
        # fp8 attribution switches (tools/fp8_noise_attribution.py; production = both True): the backward's dX products on e4m3
        # gradient rows / the forward's products on e4m3 activations
        self.fp8_backward = True
        self.fp8_forward = True
        self.ksplit = wgrad_splits
        if self.fp8:
            self._init_fp8_weights(params)

        # ---------------- trainable state: three adapters (flat per adapter); the heads are the backbone's ----------
        def adapter_names(a):
            return [(ENC + f"encoder.layer.{i}.output.adapter.{self.ADAPTER_STEMS[a]}{t}",
                     {"down.weight": (self.r, H), "down.bias": (self.r,), "up.weight": (H, self.r),
                      "up.bias": (H,)}[t]) for i in range(layers) for t in ADAPTER_TENSORS]
        self.ad = [FlatGroup(adapter_names(a), dev, with_opt=(a != 2)) for a in range(len(self.ADAPTER_STEMS))]
        self.ad_layer_numel = self.r * H + self.r + H * self.r + H
        for grp in self.ad:
            for n in grp.names:
                grp.view(n).copy_(params[n].to(dev, torch.float32))
        # bf16 operand copies of the adapters: [a][layer] -> dict(wd, wdT, wu, wuT, bd, bu)
        self._pack16 = {}
        self.ad16 = [[self._alloc_pack(a, i) for i in range(layers)] for a in range(len(self.ad))]
        for a in range(len(self.ad)):
            self.repack_adapter(a)

        # ---------------- workspace (static: a whole step is graph-capturable) ----------------
        R, R2, B = self.R, self.NPASS * self.R, self.B
        f32, b16 = self._f32, self._b16
        if self.fp8:                   # LN output as e4m3 + per-row scale (operand of the fp8 products)
            self.x8 = torch.empty(R2, H, dtype=torch.uint8, device=dev)
            self.xs = f32(R2)
            self.g8 = torch.empty(R2, H, dtype=torch.uint8, device=dev)     # gradient rows as e4m3 + per-row scale
            self.gsc = f32(R2)
            self.f8 = torch.empty(R2, I, dtype=torch.uint8, device=dev)     # gelu(u) as e4m3, fixed scale
            self.f8s = torch.full((R2,), L.F8_ACT_SCALE, dtype=torch.float32, device=dev)
            self.dU8 = torch.empty(R2, I, dtype=torch.uint8, device=dev)    # dU rows as e4m3, row scale = headroom x gsc
            if self.fp8_mx_dqkv:
                if self.S > 192:
                    raise L.FeddatHipError("fp8_mx_dqkv needs sequences of at most 192 tokens (feddat_attn_bwd_fp8mx)")
                self.dqkv8 = torch.empty(R2, 3 * H, dtype=torch.uint8, device=dev)        # dq | dk | dv as e4m3 ...
                self.dqkv_sc = torch.empty(R2, 3 * H // 32, dtype=torch.uint8, device=dev)   # ... + E8M0 per (row, 32 columns)
        # layer 0 (shared body, R rows): only h3 is kept
        self.l0 = dict(qkv=b16(R, 3 * H), ctx=b16(R, H), lse=f32(B, self.heads, self.S), h2=f32(R, H), h3=f32(R, H))
        # layers 1 .. L-1 (both passes, R2 rows): kept for the backward, each with its own input buffer (the adapter's output)
        self.act = [None] + [self._kept_layer() for _ in range(1, layers)]
        self.h_out = f32(R2, H)        # output of the last adapter (dense path: single-layer models only)
        nb2 = self.NPASS * B
        self.top.update(h_out=f32(nb2, H), dh3=f32(nb2, H))
        self.st0 = f32(R, 2)
        # task-head activations.  P0 (gated rows, old head) and P1 (adapter_1 rows, same old head) run as ONE 2B-row
        # pass ("all" = rows [0,B), "p1" = rows [B,2B) of the "both" buffers); P2 uses the updated head.
        self.hd["p2"] = dict(a0=f32(B, 2 * H), n0=f32(B, 2 * H), st=f32(B, 2), g0=f32(B, 2 * H), logits=f32(B, self.C))
        self.loss_buf = {k: f32(4 + 2 * B) for k in ("p1", "p2")}
        # row terms of the any-width DAT loss (heads of more than 128 labels: feddat_dat_loss_fwd_bwd_wide), at a static address
        self.loss_ws = f32(L.dat_loss_wide_workspace_elems(B))
        self.z = f32(R2, self.r)
        self.dz = f32(R2, self.r)
        # relu(W_down h3 + b_down) of every adapter slot, saved by the adapter forward of each layer for its backward
        # (fp32 [rows, 2, 48]: 384 B per token instead of re-reading the 3 KB row and repeating the down-projection)
        self.zsave = [f32(R2, 2, self.r) for _ in range(layers - 1)] + [f32(nb2 if layers > 1 else R2, 2, self.r)]
        # token-split partial sums of the adapter weight gradients: one slot per layer, folded into the flat gradient
        # buffers by ONE reduction at the end of the backward (feddat_adapter_wgrad_reduce) instead of one per layer
        self.wpart_stride = L.adapter_wgrad_workspace_elems(2)
        self.wpart_all = f32(layers * self.wpart_stride)
        self.wpart = self.wpart_all[:self.wpart_stride]
        self._segs_cache: Dict = {}
        self._layer_structs: Dict = {}
        # True: one composite C-ABI call per middle layer (feddat_vilt_layer_fwd / _bwd); False: the same kernel sequence
        # issued op by op from here (what tools/step_breakdown.py brackets with events)
        self.use_layer_calls = bool(gelu_codes) or R2 < 1024      # (the composite layer calls take the code epilogues at M >= 1024)
        # True: with the token-0-only attention the last layer's QKV product computes K | V for every row and Q for the 2B token-0
        # rows only, and QKV^T contracts dK | dV densely + the token-0 rows' dQ as a skinny product (a third of both products:
        # -0.03 ms/step, ratio 0.996).  OFF by default: equally accurate, but not bit-identical on the 2B token-0 rows, and at 80
        # steps the AdamW trajectory is chaotic enough that this moves the draw of the round-length parity tests (DESIGN.md
        # section 5, "draws"): the default keeps round 5's arithmetic, whose draws on both reference rounds are pinned.
        self.top_q_cls = False
        self.opt_adapters = (0, 1)
        # the head's p | m | v before its sub-step-A update (restored when A turns out to have overflowed in the backbone's
        # backward under the dynamic loss scale)
        self.head_bak = {t: torch.empty(3 * self.head[t].p.numel(), device=dev) for t in self.tasks} if self.dynamic_scale else {}

    def _init_fp8_weights(self, params):
        """e4m3 copies of the frozen weights of the fp8 products, quantised once per output channel of each product."""
        dev = self.dev

        def fp8_of(w):  # [N,K] fp32 -> e4m3 [N,K] + per-output-channel scale [N]
            w8 = torch.empty(w.shape, dtype=torch.uint8, device=dev)
            sc = torch.empty(w.shape[0], device=dev)
            L.quant_rows_fp8(w.contiguous(), w8, sc)
            return w8, sc

        for i, W in enumerate(self.layers):
            Lp = ENC + f"encoder.layer.{i}."
            wqkv = torch.cat([self._param(params, Lp + f"attention.attention.{n}.weight") for n in ("query", "key", "value")],
                             0).contiguous()
            wo, w1, w2 = (self._param(params, Lp + n + "weight") for n in ("attention.output.dense.", "intermediate.dense.",
                                                                            self.FFN2_STEM))
            W["wqkv8"], W["sqkv"] = fp8_of(wqkv)
            W["w18"], W["s1"] = fp8_of(w1)
            # dX products whose A operand (a gradient) is produced by a row kernel: FFN2^T and attention-output^T
            W["w2T8"], W["s2T"] = fp8_of(w2.t().contiguous())
            W["woT8"], W["soT"] = fp8_of(wo.t().contiguous())
            # the FFN chain: FFN1's epilogue leaves gelu(u) as e4m3 (fixed scale) for an fp8 FFN2; FFN2^T's leaves dU as
            # e4m3 rows that keep the incoming gradient's row scale x FEDDAT_F8_GRAD_HEADROOM (folded into W1^T's
            # channel scales here) for an fp8 FFN1^T
            W["w28"], W["s2"] = fp8_of(w2)
            W["w1T8"], s1T = fp8_of(w1.t().contiguous())
            W["s1T4"] = s1T * L.F8_GRAD_HEADROOM
            if self.fp8_mx_dqkv:      # QKV^T: [768, 2304], per output channel
                W["wqkvT8"], W["sqkvT"] = fp8_of(wqkv.t().contiguous())

    # ------------------------------------------------------------------------------------------ inputs
    def set_batch(self, batch: Dict[str, torch.Tensor]):
        """ViltBackbone.set_batch; fp8=True takes full batches only: its gradient-row quantisers take row maxima and are not
        verified on the all-zero gradient rows of a short batch."""
        px = batch["pixel_values"]
        if self.fp8 and px.dim() == 4 and 1 <= px.shape[0] < self.B:
            raise L.FeddatHipError(f"fp8=True runs full batches only (got {px.shape[0]} of {self.B} samples): its gradient-row "
                                   "quantisers are not verified on the all-zero rows of a short batch")
        super().set_batch(batch)

    # ------------------------------------------------------------------------------------------ adapters
    def _alloc_pack(self, a, i):
        H, r = self.H, self.r
        base = ENC + f"encoder.layer.{i}.output.adapter.{self.ADAPTER_STEMS[a]}"
        if a not in self._pack16:       # bf16 operand copies of all layers of adapter a: [layer][wd | wdT | wu | wuT]
            self._pack16[a] = torch.empty(self.nl, 4, r * H, dtype=self.op_dtype, device=self.dev)
        c = self._pack16[a][i]
        return dict(wd=c[0].view(r, H), wdT=c[1].view(H, r), wu=c[2].view(H, r), wuT=c[3].view(r, H),
                    bd=self.ad[a].view(base + "down.bias"), bu=self.ad[a].view(base + "up.bias"),
                    wd32=self.ad[a].view(base + "down.weight"), wu32=self.ad[a].view(base + "up.weight"))

    @_bound
    def repack_adapter(self, a: int):
        """fp32 masters -> bf16 MFMA operand copies (after every optimizer step / load / FedAvg): one launch for all
        layers when the flat fp32 layout is regular (it is: four tensors per layer, fixed order)."""
        packs = self.ad16[a]
        offs = [p["wd32"].data_ptr() for p in packs]
        stride = (offs[1] - offs[0]) // 4 if len(offs) > 1 else 0
        regular = all(offs[i] - offs[0] == 4 * stride * i for i in range(len(offs))) and all(
            p["wu32"].data_ptr() - p["wd32"].data_ptr() == packs[0]["wu32"].data_ptr() - packs[0]["wd32"].data_ptr()
            for p in packs)
        if regular:
            p0 = packs[0]
            L.adapter_pack_strided(p0["wd32"], p0["wu32"], stride, p0["wd"], p0["wdT"], p0["wu"], p0["wuT"],
                                   4 * self.r * self.H, len(packs))
        else:
            for p in packs:
                L.adapter_pack(p["wd32"], p["wu32"], p["wd"], p["wdT"], p["wu"], p["wuT"])

    def _segs(self, layer: int, first: bool, bwd: bool):
        """Two-segment descriptor: rows [0,R) gated (adapter_0 + adapter_2, 0.5 each), rows [R,2R) adapter_1."""
        key = (layer, first, bwd)
        if key not in self._segs_cache:
            a0, a1, a2 = (self.ad16[a][layer] for a in range(3))
            R = self.R
            self._segs_cache[key] = L.make_segs([
                dict(row_begin=0, row_end=R, train_slot=0 if bwd else -1, x_row_delta=0,
                     adapters=[dict(a0, scale=0.5), dict(a2, scale=0.5)]),
                dict(row_begin=R, row_end=2 * R, train_slot=0 if bwd else -1, x_row_delta=-R if first else 0,
                     adapters=[dict(a1, scale=1.0)]),
            ])
        return self._segs_cache[key]

    def _single_segs(self, layer: int, mode: str, rows: int):
        if mode == "gating":
            ads = [dict(self.ad16[0][layer], scale=0.5), dict(self.ad16[2][layer], scale=0.5)]
        else:
            ads = [dict(self.ad16[int(mode.split("_")[1])][layer], scale=1.0)]
        return L.make_segs([dict(row_begin=0, row_end=rows, adapters=ads)])

    # ------------------------------------------------------------------------------------------ forward
    def _layer_body(self, i: int, h_in, rows: int, nb: int, qkv, ctx, lse, h2, h3, st1=None, st2=None, u=None,
                    mask=None, ln1_done=False):
        """The backbone's layer body; where the fp8 products apply (_fp8_rows), the two products fed by a LayerNorm -- and with
        fp8_ffn_chain FFN2 -- run on the fp8 MFMA."""
        if not self._fp8_rows(rows):
            return super()._layer_body(i, h_in, rows, nb, qkv, ctx, lse, h2, h3, st1=st1, st2=st2, u=u, mask=mask,
                                       ln1_done=ln1_done)
        W, H = self.layers[i], self.H
        f16 = self.f16[:rows]
        g8 = u is not None and u.dtype == torch.uint8
        x8, xs = self.x8[:rows], self.xs[:rows]
        L.layernorm_fwd_fp8(h_in, W["ln1g"], W["ln1b"], self.ln_eps, rows, H, x8, xs, stats=st1)
        L.gemm_fp8_nt(x8, xs, W["wqkv8"], W["sqkv"], L.EPI_BF16, bias=W["bqkv"], out_bf16=qkv)
        L.attn_fwd(qkv, ctx, lse, nb, self.S, self.heads, key_mask=mask)
        L.gemm_bf16_nt(ctx, W["wo"], L.EPI_RESID_F32, bias=W["bo"], resid=h_in, out_f32=h2)
        L.layernorm_fwd_fp8(h2, W["ln2g"], W["ln2b"], self.ln_eps, rows, H, x8, xs, stats=st2)
        if self.fp8_ffn_chain:      # FFN1 -> e4m3 gelu(u) (+ gelu' codes) -> fp8 FFN2
            codes = u if g8 else self.dU.view(torch.uint8)[:rows, :self.I]       # (no backward through this call: scratch)
            L.gemm_fp8_nt(x8, xs, W["w18"], W["s1"], L.EPI_GELU_G8_F8, bias=W["b1"], out_bf16=self.f8[:rows], out2_bf16=codes)
            L.gemm_fp8_nt_f32(self.f8[:rows], self.f8s[:rows], W["w28"], W["s2"], bias=W["b2"], resid=h2, out_f32=h3)
            return
        L.gemm_fp8_nt(x8, xs, W["w18"], W["s1"], L.EPI_GELU_G8 if g8 else L.EPI_GELU, bias=W["b1"], out_bf16=f16,
                      out2_bf16=u if u is not None else self.dU[:rows])
        L.gemm_bf16_nt(f16, W["w2"], L.EPI_RESID_F32, bias=W["b2"], resid=h2, out_f32=h3)

    def _fp8_rows(self, rows: int, bwd: bool = False) -> bool:
        """fp8 products are used where feddat_gemm_fp8_nt applies (M >= 1024); smaller launches stay bf16."""
        return self.fp8 and rows >= 1024 and (self.fp8_backward if bwd else self.fp8_forward)

    @_bound
    def _forward_dual(self):
        """Shared embeddings + layer-0 body, then both passes (gated | adapter_1) batched through layers 1..L-1."""
        R, R2, B = self.R, self.NPASS * self.R, self.B
        nb = self.NPASS * B
        self._embed()
        l0 = self.l0
        m1 = self.key_mask2[:self.B]
        m2 = self.key_mask2
        self._layer_body(0, self.h0, R, B, l0["qkv"], l0["ctx"], l0["lse"], l0["h2"], l0["h3"], st1=self.st0,
                         st2=self.st0, mask=m1)
        def adapter_then_ln1(x, i, first):
            """Adapter of layer i fused with layer i+1's layernorm_before (its bf16 output and row statistics go
            where that layer's LN kernel would have put them)."""
            nx, Wn = self.act[i + 1], self.layers[i + 1]
            if self._fp8_rows(R2):      # the next layer quantises its own LayerNorm output (feddat_layernorm_fwd_fp8)
                L.adapter_fwd(x, nx["h_in"], self._segs(i, first, False), R2, z_save=self.zsave[i])
                return
            L.adapter_fwd_ln(x, nx["h_in"], self._segs(i, first, False), R2, Wn["ln1g"], Wn["ln1b"], self.ln_eps,
                             self.x16[:R2], nx["st1"], z_save=self.zsave[i])
        if self.nl > 1:
            adapter_then_ln1(l0["h3"], 0, True)
        else:
            L.adapter_fwd(l0["h3"], self.h_out, self._segs(0, True, False), R2, z_save=self.zsave[0])
        for i in range(1, self.nl - 1):
            # one C-ABI call per layer (feddat_vilt_layer_fwd): ViltLayer body + adapter + the next layer's layernorm_before
            if not self.use_layer_calls or self.fp8:
                a = self.act[i]
                self._layer_body(i, a["h_in"], R2, nb, a["qkv"], a["ctx"], a["lse"], a["h2"], a["h3"], st1=a["st1"],
                                 st2=a["st2"], u=a["u"], mask=m2, ln1_done=True)
                adapter_then_ln1(a["h3"], i, False)
                continue
            Wn = self.layers[i + 1]
            W, A, _ = self._layer_struct(i)
            L.vilt_layer_fwd(self.ctx, W, A, nb, self.S, self.heads, self._segs(i, False, False), key_mask=m2,
                             ln1_done=True, next_ln_g=Wn["ln1g"], next_ln_b=Wn["ln1b"])
        if self.nl > 1:
            self._top_layer_fwd(m2)
            self._pool(self.top["h_out"], nb, x_stride=self.H)
        else:
            self._pool(self.h_out, nb)

    def _top_layer_fwd(self, mask):
        """Last layer.  LN1 / QKV / attention see every token (keys and values of all tokens feed token 0), but only
        token 0 of each sample reaches the pooler (HF ViltPooler takes hidden_states[:, 0]; vilt.py:127), so the
        attention-output projection, LN2, FFN and the adapter run on the 2B token-0 rows, read in place through
        strided GEMM operands."""
        i = self.nl - 1
        a, W, H, t = self.act[i], self.layers[i], self.H, self.top
        R2, nb = self.NPASS * self.R, self.NPASS * self.B
        x16 = self.x16[:R2]       # LN1 of this layer: written by the previous layer's fused adapter + LN kernel
        if self._fp8_rows(R2):
            L.layernorm_fwd_fp8(a["h_in"], W["ln1g"], W["ln1b"], self.ln_eps, R2, H, self.x8[:R2], self.xs[:R2],
                                stats=a["st1"])
            L.gemm_fp8_nt(self.x8[:R2], self.xs[:R2], W["wqkv8"], W["sqkv"], L.EPI_BF16, bias=W["bqkv"], out_bf16=a["qkv"])
        elif self.cls_attention and self.top_q_cls:
            # (round 6) token 0 is the only QUERY of this layer that anything reads (step algebra item 6): K | V for every row
            # (N = 1536: two exact rounds of tiles at configs[1]), Q for the 2B token-0 rows as one skinny product
            L.gemm_bf16_nt(x16, W["wqkv"][H:], L.EPI_BF16, bias=W["bqkv"][H:], out_bf16=a["qkv"][:, H:])
            L.gemm_bf16_nt(self._cls_rows(x16, nb), W["wqkv"][:H], L.EPI_BF16, bias=W["bqkv"][:H],
                           out_bf16=self._cls_rows(a["qkv"], nb)[:, :H], skinny_workspace=self._skinny_ws())
        else:
            L.gemm_bf16_nt(x16, W["wqkv"], L.EPI_BF16, bias=W["bqkv"], out_bf16=a["qkv"])
        (L.attn_cls_fwd if self.cls_attention else L.attn_fwd)(a["qkv"], a["ctx"], a["lse"], nb, self.S, self.heads,
                                                                key_mask=mask)
        self._top_token0_fwd(a, W, nb)
        L.adapter_fwd(t["h3"], t["h_out"], self._top_segs(False), nb, z_save=self.zsave[i])

    def _top_segs(self, bwd: bool):
        key = ("top", bwd)
        if key not in self._segs_cache:
            i, B = self.nl - 1, self.B
            a0, a1, a2 = (self.ad16[a][i] for a in range(3))
            self._segs_cache[key] = L.make_segs([
                dict(row_begin=0, row_end=B, train_slot=0 if bwd else -1,
                     adapters=[dict(a0, scale=0.5), dict(a2, scale=0.5)]),
                dict(row_begin=B, row_end=2 * B, train_slot=0 if bwd else -1, adapters=[dict(a1, scale=1.0)]),
            ])
        return self._segs_cache[key]

    # ------------------------------------------------------------------------------------------ backward
    @_bound
    def _backward_dual(self):
        """dpooled [2B,H] -> adapter_0 grads (rows [0,R)) and adapter_1 grads (rows [R,2R))."""
        R, R2, B, H = self.R, self.NPASS * self.R, self.B, self.H
        nb = self.NPASS * B
        # the gradient entering the frozen backbone carries the loss scale from here on (alpha of this product; 1 for bf16
        # operands): every kernel below is linear in it, and feddat_wgrad_seg.grad_unscale takes it out again
        if self.fused_tail:      # d(pooler input) = (dpooled * (1 - pooled^2)) W_pool in one launch
            L.head_gemm(L.ht_job(self.dpooled, H, 1, self.pool_w, H, 1, nb, H, H, self.dcls_ln, pro=L.HT_PRO_TANH_BWD,
                                 pro_a=self.pooled, **self._scale_in()))
        else:
            L.tanh_bwd(self.pooled, self.dpooled, self.dpre)
            self._sg(self.dpre, H, 1, self.pool_w, H, 1, nb, H, H, self.dcls_ln, ksplit=4, alpha=self.loss_scale)
        L.layernorm_bwd_dx(self._pool_src, self.cls_st, self.lnf_g, nb, H, dy_f32=self.dcls_ln,
                           x_stride=self._pool_stride, out_f32=self.dcls)
        cur, oth = self.dh
        m2 = self.key_mask2
        top = self.nl - 1 if self.nl > 1 else 0
        if self.nl > 1:
            self._top_layer_bwd(cur, oth, m2)      # leaves d(h_in of the top layer) in `oth`
            cur, oth = oth, cur
        else:
            L.scatter_cls_rows(self.dcls, cur, None, nb, self.S, H)
        for i in range(top - 1, 0, -1):
            # one C-ABI call per layer (feddat_vilt_layer_bwd): adapter backward + its weight gradients, FFN2^T (. gelu'),
            # FFN1^T, LN2 backward (+ residual), attention-out^T, attention backward, QKV^T, LN1 backward (+ residual)
            if self._fp8_rows(R2, bwd=True):      # configs[4]: FFN2^T and attention-output^T on the fp8 MFMA, e4m3 gradient rows
                a, W = self.act[i], self.layers[i]
                L.adapter_bwd_fp8(cur, oth, self.g8, self.gsc, self._segs(i, False, True), R2, z_saved=self.zsave[i],
                                  z_out=self.z, dz_out=self.dz)
                self._adapter_wgrads(i, a["h3"], 0, cur)
                if self.fp8_ffn_chain and self.g8u:
                    L.gemm_fp8_nt(self.g8, self.gsc, W["w2T8"], W["s2T"], L.EPI_MUL_G8_F8, aux=a["u"], out_bf16=self.dU8)
                    L.gemm_fp8_nt(self.dU8, self.gsc, W["w1T8"], W["s1T4"], L.EPI_BF16, out_bf16=self.dx16)
                else:
                    L.gemm_fp8_nt(self.g8, self.gsc, W["w2T8"], W["s2T"], L.EPI_MUL_G8 if self.g8u else L.EPI_MUL_DGELU,
                                  aux=a["u"], out_bf16=self.dU)
                    L.gemm_bf16_nt(self.dU, W["w1T"], L.EPI_BF16, out_bf16=self.dx16)
                L.layernorm_bwd_dx_fp8(a["h2"], a["st2"], W["ln2g"], R2, H, self.g8, self.gsc, dy_bf16=self.dx16, dres=oth,
                                       out_f32=cur)
                L.gemm_fp8_nt(self.g8, self.gsc, W["woT8"], W["soT"], L.EPI_BF16, out_bf16=self.dctx)
                if self.fp8_mx_dqkv:
                    L.attn_bwd_fp8mx(a["qkv"], a["ctx"], a["lse"], self.dctx, self.dqkv8, self.dqkv_sc, nb, self.S, self.heads,
                                     key_mask=m2)
                    L.gemm_fp8mx_nt(self.dqkv8, self.dqkv_sc, W["wqkvT8"], W["sqkvT"], out_bf16=self.dx16)
                else:
                    L.attn_bwd(a["qkv"], a["ctx"], a["lse"], self.dctx, self.dqkv, nb, self.S, self.heads, key_mask=m2)
                    L.gemm_bf16_nt(self.dqkv, W["wqkvT"], L.EPI_BF16, out_bf16=self.dx16)
                L.layernorm_bwd_dx(a["h_in"], a["st1"], W["ln1g"], R2, H, dy_bf16=self.dx16, dres=cur, out_f32=oth)
                cur, oth = oth, cur
                continue
            if not self.use_layer_calls or self.fp8:
                a, W = self.act[i], self.layers[i]
                L.adapter_bwd(None, cur, oth, self._segs(i, False, True), R2, dx_bf16=self.dh16, z_out=self.z,
                              dz_out=self.dz, z_saved=self.zsave[i])
                self._adapter_wgrads(i, a["h3"], 0, cur)
                L.gemm_bf16_nt(self.dh16, W["w2T"], L.EPI_MUL_G8 if self.g8u else L.EPI_MUL_DGELU, aux=a["u"], out_bf16=self.dU)
                L.gemm_bf16_nt(self.dU, W["w1T"], L.EPI_BF16, out_bf16=self.dx16)
                L.layernorm_bwd_dx(a["h2"], a["st2"], W["ln2g"], R2, H, dy_bf16=self.dx16, dres=oth, out_f32=cur,
                                   out_bf16=self.dh16)
                L.gemm_bf16_nt(self.dh16, W["woT"], L.EPI_BF16, out_bf16=self.dctx)
                L.attn_bwd(a["qkv"], a["ctx"], a["lse"], self.dctx, self.dqkv, nb, self.S, self.heads, key_mask=m2)
                L.gemm_bf16_nt(self.dqkv, W["wqkvT"], L.EPI_BF16, out_bf16=self.dx16)
                L.layernorm_bwd_dx(a["h_in"], a["st1"], W["ln1g"], R2, H, dy_bf16=self.dx16, dres=cur, out_f32=oth)
                cur, oth = oth, cur
                continue
            W, A, _ = self._layer_struct(i)
            G = self._grad_struct(cur, oth)
            L.vilt_layer_bwd(self.ctx, W, A, G, nb, self.S, self.heads, self._segs(i, False, True),
                             self._wgrad_segs(i, self.act[i]["h3"], 0, cur), self._wpart(i), key_mask=m2,
                             wgrad_reduce_now=False)
            cur, oth = oth, cur
        # layer 0: weight gradients only (nothing trainable below)
        L.adapter_bwd(None, cur, None, self._segs(0, True, True), R2, z_out=self.z, dz_out=self.dz,
                      z_saved=self.zsave[0])
        self._adapter_wgrads(0, self.l0["h3"], -R, cur)
        self._wgrad_reduce_all()

    def _top_layer_bwd(self, cur, oth, mask):
        """Backward of the last layer: the incoming gradient is non-zero only on the 2B token-0 rows, so the adapter,
        FFN, LN2 and attention-output backward run on those rows; from the attention backward on every token is live."""
        i = self.nl - 1
        a, W, H, t = self.act[i], self.layers[i], self.H, self.top
        R2, nb = self.NPASS * self.R, self.NPASS * self.B
        L.adapter_bwd(None, self.dcls, t["dh3"], self._top_segs(True), nb, dx_bf16=t["dh316"], z_out=self.z,
                      dz_out=self.dz, z_saved=self.zsave[i])
        segs = self._top_wgrad_segs()
        if segs is not None:
            L.adapter_wgrad_partial(segs, self._wpart(i))
        ws = self._skinny_ws()
        L.gemm_bf16_nt(t["dh316"], W["w2T"], L.EPI_MUL_DGELU, aux=t["u"], out_bf16=t["dU"], skinny_workspace=ws)
        L.gemm_bf16_nt(t["dU"], W["w1T"], L.EPI_BF16, out_bf16=t["dx2"], skinny_workspace=ws)
        L.layernorm_bwd_dx(t["h2"], t["st2"], W["ln2g"], nb, H, dy_bf16=t["dx2"], dres=t["dh3"], out_f32=t["dh2"],
                           out_bf16=t["dh216"])
        L.gemm_bf16_nt(t["dh216"], W["woT"], L.EPI_F32, out_f32=t["dctx"], skinny_workspace=ws)
        # the token-0 rows' residual gradient t["dh2"] reaches the LN1 backward below compact (dres_every = S); only the dense
        # attention path needs its own operand scattered into a dense buffer
        if self.cls_attention:       # rank-1 backward straight from the fp32 token-0 gradient rows
            L.attn_cls_bwd(a["qkv"], a["ctx"], a["lse"], t["dctx"], self.dqkv, nb, self.S, self.heads, key_mask=mask)
        else:
            L.scatter_cls_rows(t["dctx"], None, self.dctx, nb, self.S, H)
            L.attn_bwd(a["qkv"], a["ctx"], a["lse"], self.dctx, self.dqkv, nb, self.S, self.heads, key_mask=mask)
        if self.cls_attention and self.top_q_cls and nb <= 64:
            # dQ is non-zero on the token-0 rows only: the dense product contracts dK | dV alone (K = 1536: the zero third of
            # the contraction is not read or multiplied -- bit-identical on those rows), and the 2B token-0 rows are
            # overwritten by the full contraction as one skinny product
            L.gemm_bf16_nt(self.dqkv[:, H:], W["wqkvT"][:, H:], L.EPI_BF16, out_bf16=self.dx16)
            L.gemm_bf16_nt(self._cls_rows(self.dqkv, nb), W["wqkvT"], L.EPI_BF16, out_bf16=self._cls_rows(self.dx16, nb),
                           skinny_workspace=self._skinny_ws())
        else:
            L.gemm_bf16_nt(self.dqkv, W["wqkvT"], L.EPI_BF16, out_bf16=self.dx16)
        L.layernorm_bwd_dx(a["h_in"], a["st1"], W["ln1g"], R2, H, dy_bf16=self.dx16, dres=t["dh2"], dres_every=self.S, out_f32=oth)

    def _top_wgrad_segs(self):
        """Weight-gradient descriptor of the top layer's adapters (2B token-0 rows: adapter_0 | adapter_1)."""
        i, t, B, n = self.nl - 1, self.top, self.B, self.ad_layer_numel
        return self._wgrad_desc(("wg-top", self.opt_adapters), lambda: [
            dict(x=t["h3"][r0:], dy=self.dcls[r0:], z=self.z[r0:], dz=self.dz[r0:], grad=self.ad[ad].g[i * n:(i + 1) * n],
                 rows=B, scale=sc) for ad, r0, sc in ((0, 0, 0.5), (1, B, 1.0)) if ad in self.opt_adapters])

    def _layer_struct(self, i: int):
        """ctypes views of layer i's frozen weights and static activation buffers for the composite entry points."""
        if i not in self._layer_structs:
            Wd, a = self.layers[i], self.act[i]
            R2 = self.NPASS * self.R
            W = L._fill(L.ViltLayerWeights, wqkv=Wd["wqkv"], wo=Wd["wo"], w1=Wd["w1"], w2=Wd["w2"], wqkvT=Wd["wqkvT"],
                        woT=Wd["woT"], w1T=Wd["w1T"], w2T=Wd["w2T"], bqkv=Wd["bqkv"], bo=Wd["bo"], b1=Wd["b1"], b2=Wd["b2"],
                        ln1_g=Wd["ln1g"], ln1_b=Wd["ln1b"], ln2_g=Wd["ln2g"], ln2_b=Wd["ln2b"])
            W.ln_eps = self.ln_eps
            nxt = self.act[i + 1] if i + 1 < self.nl else None
            A = L._fill(L.ViltLayerActs, h_in=a["h_in"], st1=a["st1"], qkv=a["qkv"], ctx=a["ctx"], lse=a["lse"], h2=a["h2"],
                        st2=a["st2"], u=a["u"], h3=a["h3"], z_save=self.zsave[i], h_out=nxt["h_in"] if nxt else self.h_out,
                        x16=self.x16[:R2], f16=self.f16[:R2], st1_next=nxt["st1"] if nxt else None)
            self._layer_structs[i] = (W, A, None)
        return self._layer_structs[i]

    def _grad_struct(self, cur, oth):
        key = ("G", cur.data_ptr())
        if key not in self._layer_structs:      # dh3 and dh_in share `oth`: dh3 is dead before dh_in is written
            self._layer_structs[key] = L._fill(L.ViltLayerGrads, dh_out=cur, dh_in=oth, dh3=oth, dh16=self.dh16, dU=self.dU,
                                               dx16=self.dx16, dctx=self.dctx, dqkv=self.dqkv, z=self.z, dz=self.dz)
        return self._layer_structs[key]

    def _wgrad_segs(self, layer: int, x, x_delta_s: int, dy):
        R, n = self.R, self.ad_layer_numel
        return self._wgrad_desc(("wg", layer, x.data_ptr(), dy.data_ptr(), self.opt_adapters), lambda: [
            dict(x=x[xrow0:], dy=dy[row0:], z=self.z[row0:], dz=self.dz[row0:], grad=self.ad[a].g[layer * n:(layer + 1) * n],
                 rows=R, scale=sc)
            for a, row0, xrow0, sc in ((0, 0, 0, 0.5), (1, R, R + x_delta_s, 1.0)) if a in self.opt_adapters])

    def _wpart(self, layer: int):
        return self.wpart_all[layer * self.wpart_stride:(layer + 1) * self.wpart_stride]

    def _wgrad_reduce_all(self):
        """Fold every layer's partial sums into the adapters' flat gradient buffers (one launch)."""
        ads = [a for a in (0, 1) if a in self.opt_adapters]
        if not ads:
            return
        key = ("wg-reduce", self.opt_adapters)
        if key not in self._segs_cache:
            n = self.ad_layer_numel
            ptrs = [self.ad[a].g[i * n:(i + 1) * n].data_ptr() for i in range(self.nl) for a in ads]
            assert all(p % 16 == 0 for p in ptrs)      # feddat_adapter_wgrad_reduce moves float4 (it cannot check a device table)
            self._segs_cache[key] = torch.tensor(ptrs, dtype=torch.int64, device=self.dev)
        # flags[a] for adapter a
        self._reduce_wgrads(self._segs_cache[key], self.nl, len(ads), self.wpart_all, self.wpart_stride, self.ovf_flags[ads[0]:])

    def _adapter_wgrads(self, layer: int, x, x_delta_s: int, dy):
        """dW_up = s dy^T z, db_up = s sum_t dy, dW_down = dz^T x, db_down = sum_t dz (autograd of adapter.py:125-146)
        for adapter_0 (rows [0,R)) and adapter_1 (rows [R,2R)): exact fp32 MFMA, split over tokens, deterministic
        reduction straight into the flat gradient buffers."""
        segs = self._wgrad_segs(layer, x, x_delta_s, dy)
        if segs is not None:
            L.adapter_wgrad_partial(segs, self._wpart(layer))

    # ------------------------------------------------------------------------------------------ train step
    @_bound
    def begin_local_update(self, task: str, steps_per_epoch: int, num_epochs: int = 15, warmup_ratio: float = 0.1,
                           opt_adapters: Sequence[int] = (0, 1)):
        """TaskTrainer.train prologue (task_trainer.py:36-59): teacher snapshot, fresh AdamW state and schedule."""
        self.task = task
        self.copy_global_to_teacher()
        self.opt_adapters = tuple(opt_adapters)
        # scheduler index / Adam step count per group: adapter_1 is stepped at 2b, adapter_0 at 2b+1, head at both
        self._start_local_update(steps_per_epoch, num_epochs, warmup_ratio, {"adapter_0": (1, 0)})

    def _graph_switches(self) -> Tuple:
        return super()._graph_switches() + (self.use_layer_calls, self.fp8, self.fp8_ffn_chain, self.fp8_mx_dqkv, self.top_q_cls)

    def _named_groups(self):
        return [("adapter_0", self.ad[0]), ("adapter_1", self.ad[1]), ("head", self.head[self.task])]

    def _loss(self, logits, teacher, slot):
        if self.C > 128:      # the one-launch forms below hold a row in two elements per lane; wider heads (vqa: 3129 labels)
            flag = (self.ovf_flags[1:2] if slot == "p1" else self.ovf_flags[0:1]) if self._dyn() else None
            L.dat_loss_fwd_bwd_wide(logits, teacher, self.inp["target"], self.dlogits, self.loss_buf[slot], self.loss_ws,
                                    n=self.n_valid, nonfinite=flag)
        elif self.n_valid < self.B:      # a short batch: the loss of the n valid rows, zero gradient in the replica rows
            flag = self.ovf_flags[1:2] if slot == "p1" else self.ovf_flags[0:1]
            L.dat_loss_fwd_bwd_rows(logits, teacher, self.inp["target"], self.dlogits, self.loss_buf[slot], self.n_valid,
                                    flag if self._dyn() else None)
        elif self._dyn():      # + non-finite loss -> the sub-step's overflow flag (p1 = sub-step A, p2 = B)
            flag = self.ovf_flags[1:2] if slot == "p1" else self.ovf_flags[0:1]
            L.dat_loss_fwd_bwd_checked(logits, teacher, self.inp["target"], self.dlogits, self.loss_buf[slot], flag)
        elif self.fused_tail:
            L.dat_loss_fwd_bwd_single(logits, teacher, self.inp["target"], self.dlogits, self.loss_buf[slot])
        else:
            L.dat_loss_fwd_bwd(logits, teacher, self.inp["target"], self.dlogits, self.loss_buf[slot])

    @_bound
    def _step_kernels(self):
        B, task = self.B, self.task
        hp = self.head[task]
        self._forward_dual()
        pooled_g, pooled_s = self.pooled[:B], self.pooled[B:]
        # P0: logits of the gated pass with the current head (no grad)          task_trainer.py:283-287
        # P1: adapter_1 pass, KL to P0                                           task_trainer.py:290-308
        # same head weights for both -> one 2B-row pass over [pooled_g; pooled_s]
        logits_both = self._head_fwd(self.pooled[:2 * B], "both", task)
        logits_all, logits_1 = logits_both[:B], logits_both[B:]
        self._loss(logits_1, logits_all, "p1")
        self._head_bwd(pooled_s, "p1", task, self.dpooled[B:])
        if self._dyn():      # sub-step A's head update: skipped on a non-finite loss; the old p | m | v are kept for the restore below
            fA = self.ovf_flags[1:2]
            self._adamw_many([self._adamw_group(hp, skip_if=(fA,), bak=self.head_bak[task], bak_mode=1)])
        elif self.fused_tail:
            self._adamw_many([self._adamw_group(hp)])       # sub-step 2b; its counters are ticked once, at the end of the step
        else:
            self._adamw(hp)
            L.step_tick(hp.state, 1, 1)
        # P2: gated pass again -- same pooled features, UPDATED head, KL to logits_1     task_trainer.py:311-328
        logits_0 = self._head_fwd(pooled_g, "p2", task)
        self._loss(logits_0, logits_1, "p2")
        self._head_bwd(pooled_g, "p2", task, self.dpooled[:B])
        # one backward for both passes, then the deferred adapter_1 step (lr index 2b) and the P2 steps (2b+1)
        self._backward_dual()
        if self.fused_tail:      # the shared DAT tail, with the head (restored from head_bak when sub-step A overflowed)
            self._dat_tail(hp, self.head_bak.get(task))
            return
        if 1 in self.opt_adapters:
            self._adamw(self.ad[1])
            self.repack_adapter(1)
        L.step_tick(self.ad[1].state, 2, 1)
        self._adamw(hp)
        L.step_tick(hp.state, 1, 1)
        if 0 in self.opt_adapters:
            self._adamw(self.ad[0])
            self.repack_adapter(0)
        L.step_tick(self.ad[0].state, 2, 1)

    def _loss_tensor(self):
        """What train_step returns: the device tensor holding what the reference returns, loss_0 = BCE * num_labels of the
        P2 pass (loss_buf['p2'][0]); [1] = KL, [2] = L_0."""
        return self.loss_buf["p2"]

    # ------------------------------------------------------------------------------------------ inference
    @_bound
    @torch.no_grad()
    def forward(self, batch: Dict[str, torch.Tensor], mode: str, task: Optional[str] = None):
        """model(task_key, images, texts) -> (pooled, logits) in adapter mode `mode` ('gating' | 'adapter_k')
        (vilt.py:244-264 with the adapter switches of vilt.py:363-373).  Single pass over B*S rows."""
        task = task or self.task
        self.set_batch(batch)
        R, B = self.R, self.B
        self._embed()
        l0 = self.l0
        m1 = self.key_mask2[:self.B]
        h = self.h0
        for i in range(self.nl):
            self._layer_body(i, h, R, B, l0["qkv"], l0["ctx"], l0["lse"], l0["h2"], l0["h3"], st1=self.st0,
                             st2=self.st0, mask=m1)
            h = self.dh[i & 1][:R]
            L.adapter_fwd(l0["h3"], h, self._single_segs(i, mode, R), R)
        self._pool(h, B)
        logits = self._head_fwd(self.pooled[:B], "all", task)
        return self.pooled[:self.n_valid].clone(), logits[:self.n_valid].clone()
