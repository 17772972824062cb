"""ALBEF dual-adapter (DAT + MKD) local-update engine on MI355X -- BASELINE.json configs[3]: the backward, the weight
gradients, the trainable LM head and the train step on top of the frozen model and forward of albef_backbone.AlbefBackbone;
the evaluation (forward_train_logits, rank_answer) comes from albef_rank.AlbefRank.

Host-side sequencing of the HIP kernels in libfeddat_hip.so for the reference's two-stream path: ALBEF.forward(train=True)
inside the dat branch of TaskTrainer.train_step (src/train/visionlanguage_tasks/task_trainer.py:280-330, ALBEF wiring
:296-297,316-317, vocabulary-axis KL :506-516).  The step algebra (which of the reference's three passes P0 / P1 / P2 share
what, with the LM head frozen or trained) and the dropout scheme are described in albef_backbone's module docstring.

A step comes in two schedules, _step_kernels (LM head frozen) and _step_kernels_head (train_lm_head=True), and each of them
in two forms: the two passes' text towers side by side on two streams, or stacked on 2x the rows (stack_text).  The halves the
schedules share are written once: _forward_stacked and _image_bwd_stacked for the stacked form, _forward_two_passes for the
two-stream form; a schedule keeps what happens between the logits and the towers' backward.  Nothing trainable lies below the
first ViT block's adapter, so the backward stops there.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from . import lib as L
from .albef_backbone import ADAPTER_TENSORS, LM_HEAD, PRE, AlbefBackbone, lm_head_group_spec  # noqa: F401
from .albef_rank import AlbefRank, rank_slab_plan, slab_question_of_row  # noqa: F401
from .local_update import _bound


class AlbefDatEngine(AlbefRank, AlbefBackbone):
    def __init__(self, params: Dict[str, torch.Tensor], device, batch: int, n_answers: int, q_len: int = 25, a_len: int = 4,
                 vit_depth: int = 12, enc_layers: int = 12, fusion_layer: int = 6, dec_layers: int = 6, image: int = 384,
                 vocab: int = 30522, lr: float = 1e-4, weight_decay: float = 1e-2, adam_eps: float = 1e-8, pad_id: int = 0,
                 max_pos: int = 512, dropout: float = 0.0, seed: int = 0, stack_text: bool = False,
                 operands: str = "f16", loss_scale: Optional[float] = None, dynamic_loss_scale: Optional[bool] = None,
                 scale_growth_interval: int = 2000, train_lm_head: bool = False):
        """train_lm_head: train text_decoder.cls.predictions.* as the reference does (albef_backbone's docstring); off by default.
        operands="f16": every 16-bit MFMA operand in IEEE half (libfeddat_hip_f16.so) with a power-of-two loss scale on
        dL/dlogits (feddat_lm_loss_fwd_bwd's grad_scale, default 2^14) that leaves through feddat_wgrad_seg.grad_unscale -- the
        ViLT engine's scheme (engine.ViltDatEngine), with the same device-side dynamic scaler (dynamic_loss_scale, default on for
        "f16").  The default operand format is fp16 -- in this class, in train.main (--encoder_name albef_no_distill without
        --mixed_precision) and in bench.py --workload albef alike, the same as the ViLT engine's and the reference's own setting
        (accelerate_config.yaml:8): against the reference's own full-size 40-step rounds (tests/golden/g11b_albef_full_round40.npz
        and ..._seed8800.npz) fp16 operands land at 3.2e-4 / 2.6e-4 on the worst adapter element (mean ratio 0.005 / 0.003), bf16
        operands at 7.6e-4 / 8.4e-4 (0.024 / 0.028): both inside north_star's 1e-3, bf16 with a fifth of it to spare, for 1.5 % of
        the step (tests/test_sizes_gpu.py::test_albef_full_size_round_of_40_steps_vs_reference_golden asserts all four)."""
        # fp16 operands: the loss scale is dynamic by default -- LocalUpdateEngine's GradScaler on the device, as in ViltDatEngine
        # (DESIGN.md section 5b).  With the LM head frozen the two sub-steps share no trainable tensor: flag B (adapter_0's
        # pass) skips adapter_0's step alone; flag A (adapter_1's pass) voids the batch like in the ViLT engine (one finish kernel).
        # A trainable head is shared by the two sub-steps exactly like the ViLT task head: _dat_tail's restore / skip predicates.
        self._init_loss_scale(operands, loss_scale, dynamic_loss_scale, scale_growth_interval)
        self.train_lm_head = bool(train_lm_head)
        with L.operands(operands):
            self._init_backbone(params, device, batch, n_answers, q_len, a_len, vit_depth, enc_layers, fusion_layer, dec_layers,
                                image, vocab, lr, weight_decay, adam_eps, pad_id, max_pos, dropout, seed, stack_text)
            self._init_rank()
            # the weight-gradient workspaces come ahead of the backbone's buffers, as they always have: which freed block of the
            # caching allocator a buffer lands in, and with it the allocator's accounting, follows the order of the allocations
            self._alloc_wgrad()
            self._alloc()
            self._alloc_step()

    def _alloc_wgrad(self):
        """Weight-gradient partial sums: one slot per adapter module and pass; ONE batched reduction per backward pass folds them
        into the flat gradient buffers (feddat_adapter_wgrad_partial / _reduce) instead of one reduce launch per module.  A slot
        holds the partial sums of the pass's segments: one, or two for the stacked pair."""
        modes = self.ACT_SETS + (("both",) if self.batch_text else ())
        ws = {n: L.adapter_wgrad_workspace_elems(n) for n in ((1, 2) if self.batch_text else (1,))}
        self.wpart_stride = {m: ws[2 if m == "both" else 1] for m in modes}
        self.wpart = {m: torch.empty(len(self.modules) * self.wpart_stride[m], device=self.dev) for m in modes}
        self._wg_done = {m: [] for m in self.ACT_SETS + ("both",)}

    def _alloc_step(self):
        """What the backward and the step need besides: the schedule's host state, the loss scaler, one scratch set per pass
        (and per stacked pair), P0's teacher logits, the head's gradients."""
        dev, H, I = self.dev, self.H, self.I
        f32, b16 = self._f32, self._b16
        B, N, Lq, La = self.B, self.N, self.Lq, self.La
        self.sched = dict(warmup=1, total=2)
        self.opt_adapters = tuple(a for a in range(len(self.ad)) if a not in self.FROZEN_ADAPTERS)
        self.graph = None
        self.side = None           # second stream of train_step (created lazily on the engine's device)
        self._alloc_scaler()
        # backward scratch: one set per pass (their text-side backward passes run on two streams)
        Mtext = max(self.Mq, self.Ma, N * Lq, self.R)

        def scratch(k):
            """Scratch of k passes stacked.  The image encoder's backward always runs per pass, in the passes' own sets, so only
            the single set's row buffers hold its Mi rows."""
            M = max(self.Mi, Mtext) if k == 1 else k * Mtext
            return dict(dlogits=b16(k * self.R, self.Vp), d1=f32(M, H), d2=f32(M, H), d3=f32(M, H), d4=f32(M, H),
                        b1=b16(M, H), b2=b16(M, H), bI=b16(M, I), b3=b16(M, 3 * H),
                        bkv=b16(k * max(self.Mi, N * Lq), max(self.el - self.fl, self.dl) * 2 * H),
                        z=f32(M, self.r), dz=f32(M, self.r), dsum=f32(k * max(B, N), self.heads, max(self.Ni, Lq, La)),
                        d_img=f32(k * self.Mi, H), d_qs=f32(k * self.Mq, H), d_rep=f32(k * N * Lq, H), d_dec=f32(k * self.Ma, H))
        self.gs = {m: scratch(2 if m == "both" else 1) for m in self.wpart}
        if self.dropout > 0 and len(self.ACT_SETS) > 1:       # teacher logits of P0: the gated text pass is re-run (other masks) for P2
            self.logits_all = torch.empty(self.R, self.Vp, device=dev)
        if self.train_lm_head:
            self._alloc_head_grads()

    # ------------------------------------------------------------------------------------------ weight gradients
    def _wgrad(self, m: int, mode: str, x, dy, rows: int):
        """Partial sums of module m's weight gradient from the pass's rows: per segment, the gradient of the adapter the
        segment trains (its first; scale 0.5 on the gated rows, where it is one of two)."""
        segments = [(lo, hi) + ads[0] for lo, hi, ads in self._mode_segments(mode, rows)]
        if any(a not in self.opt_adapters for _, _, a, _ in segments):      # (the stacked pair runs only when both are optimised)
            return
        n, g = self.ad_numel, self.gs[mode]
        segs = self._wgrad_desc(("wg", m, mode, x.data_ptr(), dy.data_ptr(), rows), lambda: [
            dict(x=x[lo:], dy=dy[lo:], z=g["z"][lo:], dz=g["dz"][lo:], grad=self.ad[a].g[m * n:(m + 1) * n], rows=hi - lo, scale=s)
            for lo, hi, a, s in segments])
        ws = self.wpart_stride[mode]
        L.adapter_wgrad_partial(segs, self.wpart[mode][m * ws:(m + 1) * ws])
        self._wg_done[mode].append(m)

    def _wgrad_reduce(self, mode: str):
        """Fold the partial sums of every module this backward pass produced into the adapters' gradient buffers (one launch)."""
        done, self._wg_done[mode] = self._wg_done[mode], []
        if not done:
            return
        ms = tuple(sorted(done))
        trained = [ads[0][0] for _, _, ads in self._mode_segments(mode, 2)]      # gating: [0]; adapter_1: [1]; both: [0, 1]
        nseg = len(trained)
        key = ("wg-reduce", mode, ms)
        if key not in self._segs_cache:
            n = self.ad_numel
            contiguous = ms == tuple(range(ms[0], ms[0] + len(ms)))
            ptrs = [self.ad[a].g[m * n:(m + 1) * n].data_ptr() for m in ms for a in trained]
            assert all(p % 16 == 0 for p in ptrs)      # feddat_adapter_wgrad_reduce moves float4
            self._segs_cache[key] = (torch.tensor(ptrs, dtype=torch.int64, device=self.dev), contiguous)
        ptrs, contiguous = self._segs_cache[key]
        # the overflow flag of adapter a's pass is ovf_flags[a] (flag B = adapter_0's, flag A = adapter_1's): segment j's is flags[j]
        ws, flags = self.wpart_stride[mode], self.ovf_flags[trained[0]:trained[0] + nseg]
        if contiguous:       # the usual case (all 30 modules): slots m0 .. m0 + len - 1 are one strided batch
            self._reduce_wgrads(ptrs, len(ms), nseg, self.wpart[mode][ms[0] * ws:], ws, flags)
        else:
            for j, m in enumerate(ms):
                self._reduce_wgrads(ptrs[j * nseg:(j + 1) * nseg], 1, nseg, self.wpart[mode][m * ws:], ws, flags)

    def _scale_in(self, mode: str):
        """How the loss scale enters, on dL/dlogits of the pass `mode` (+ that pass's overflow flag for a non-finite loss); it
        leaves through LocalUpdateEngine._scale_out."""
        if not self._dyn():
            return dict(grad_scale=self.loss_scale)
        a = self._mode_segments(mode, 2)[0][2][0][0]      # the adapter the pass trains: its flag ("gating": 0, "adapter_1": 1)
        return dict(grad_scale=1.0, grad_scale_dev=self.scaler_f[0:1], nonfinite=self.ovf_flags[a:a + 1])

    # ------------------------------------------------------------------------------------------ trainable LM head
    def _alloc_head_grads(self):
        """Partial-sum buffers and the reduce table of the head's four vector gradients (a sub-step has R rows, whatever the
        step form), and the head's p | m | v backup of sub-step A under the dynamic loss scale."""
        dev, H, Vp, g = self.dev, self.H, self.Vp, self.lm
        slabs = L.vector_grad_workspace_elems(self.R, H) // H
        self.hg = dict(bias=torch.empty(slabs * Vp, device=dev), db=torch.empty(slabs * H, device=dev),
                       gamma=torch.empty(slabs * H, device=dev), beta=torch.empty(slabs * H, device=dev))
        ob = g.offsets[g.names[4]]
        assert ob % 4 == 0 and g.g.numel() >= ob + Vp
        self.hg_table = L.make_vgrad_jobs([(self.hg["bias"], slabs, g.g[ob:ob + Vp]), (self.hg["db"], slabs, g.view(g.names[1], g.g)),
                                           (self.hg["gamma"], slabs, g.view(g.names[2], g.g)),
                                           (self.hg["beta"], slabs, g.view(g.names[3], g.g))], dev)
        self.head_bak = torch.empty(3 * g.p.numel(), device=dev) if self.dynamic_scale else None
        # diagnostics: a tensor of the gradient buffer's size set here receives the head's gradient of sub-step A (L_1), which
        # sub-step B's otherwise overwrites within the step
        self.grad_a_probe: Optional[torch.Tensor] = None

    def _head_step_a(self):
        """Sub-step A's optimizer step on the head (tick 2b).  Dynamic scale: skipped on flag A as far as it is known here (the
        loss, the head's own gradients); the old p | m | v are kept for _dat_tail's restore, should adapter_1's backward raise
        the flag later.  The counters are ticked once, at the end of the step."""
        if self.grad_a_probe is not None:
            self.grad_a_probe.copy_(self.lm.g)
        if self._dyn():
            self._adamw_many([self._adamw_group(self.lm, skip_if=(self.ovf_flags[1:2],), bak=self.head_bak, bak_mode=1)])
        else:
            self._adamw_many([self._adamw_group(self.lm)])
        self._refresh_head()

    # ------------------------------------------------------------------------------------------ backward
    def _bert_bwd(self, T, S, m0: int, mode: str, M, nb, Sq, self_mask, causal, enc16, enc_rows, Skv, enc_mask, d_out,
                  d_enc, pass_id=None, tower: int = 0):
        """d_out: fp32 [M,768] gradient of the tower's output (consumed); d_enc: fp32 gradient of the encoder-side states
        (written: one product over all cross-attention layers' dK | dV); returns the gradient wrt the tower's embedding output
        (unused: embeddings frozen)."""
        H, g = self.H, self.gs[mode]
        cross0 = T["cross_layers"][0] if T["cross_layers"] else 0
        for i in range(len(T["layers"]) - 1, -1, -1):
            W, A = T["layers"][i], S["layers"][i]
            dk = lambda kind: self._drop(pass_id, tower, i, kind)      # noqa: E731

            def ln_bwd_to_operand(x, st, gam, dy, dres, out, kind):
                """LayerNorm backward whose fp32 result also becomes the bf16 dY operand of the dense layer ahead of it --
                through that layer's dropout mask when the pass has one (d dense = mask / (1 - p) . d out)."""
                d = dk(kind)
                if d is None:
                    L.layernorm_bwd_dx(x, st, gam, M, H, dy_f32=dy, dres=dres, out_f32=out, out_bf16=g["b1"][:M])
                else:
                    L.layernorm_bwd_dx(x, st, gam, M, H, dy_f32=dy, dres=dres, out_f32=out)
                    L.dropout(out, d, out_bf16=g["b1"][:M])
            ds2, dxf, dx, ds1 = g["d1"][:M], g["d2"][:M], g["d3"][:M], g["d4"][:M]
            L.layernorm_bwd_dx(A["s2"], A["st_o"], W["lng"], M, H, dy_f32=d_out, out_f32=ds2)
            L.adapter_bwd(None, ds2, dxf, self._segs(m0 + i, mode, M, True), M, z_out=g["z"], dz_out=g["dz"],
                          z_saved=A["zs"])
            self._wgrad(m0 + i, mode, A["x"], ds2, M)
            L.axpby3(dxf, 1.0, ds2, -1.0, out_f32=dx)                      # d x = Wd^T dz (the adapter's residual is r, not x)
            ln_bwd_to_operand(A["s1"], A["st_x"], W["lng"], dx, ds2, ds1, "out")
            L.gemm_bf16_nt(g["b1"][:M], W["fc2"]["wT"], L.EPI_MUL_DGELU, aux=A["u"], out_bf16=g["bI"][:M])
            dc = d_out                                                      # reuse: d_out is dead
            L.gemm_bf16_nt(g["bI"][:M], W["fc1"]["wT"], L.EPI_RESID_F32, resid=ds1, out_f32=dc)
            if W["cross"] is not None:
                Wc = W["cross"]
                dt2 = ds2
                ln_bwd_to_operand(A["t2"], A["st_c"], Wc["lng"], dc, None, dt2, "cross_out")
                L.gemm_bf16_nt(g["b1"][:M], Wc["o"]["wT"], L.EPI_BF16, out_bf16=g["b2"][:M])
                kv_rows, j = A["kvc"].shape[0], i - cross0
                dq, dkv = g["b1"][:M], g["bkv"][:kv_rows, j * 2 * H:(j + 1) * 2 * H]
                L.attn2_bwd(A["qc"], A["kvc"][:, :H], A["kvc"][:, H:], A["ctx2"], A["lse2"], g["b2"][:M], g["dsum"], dq,
                            dkv[:, :H], dkv[:, H:], nb, Sq, Skv, self.heads, key_mask=enc_mask, q_rows=Sq, kv_rows=enc_rows,
                            drop=dk("cross_probs"))
                da = dc
                L.gemm_bf16_nt(dq, Wc["q"]["wT"], L.EPI_RESID_F32, resid=dt2, out_f32=da)
            else:
                da = dc
            dt1 = ds2
            ln_bwd_to_operand(A["t1"], A["st_a"], W["att"]["lng"], da, None, dt1, "self_out")
            L.gemm_bf16_nt(g["b1"][:M], W["att"]["o"]["wT"], L.EPI_BF16, out_bf16=g["b2"][:M])
            dqkv = g["b3"][:M]
            L.attn2_bwd(A["qkv"][:, :H], A["qkv"][:, H:2 * H], A["qkv"][:, 2 * H:], A["ctx"], A["lse"], g["b2"][:M],
                        g["dsum"], dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:], nb, Sq, Sq, self.heads, key_mask=self_mask,
                        causal=causal, drop=dk("self_probs"))
            L.gemm_bf16_nt(dqkv, W["att"]["qkv"]["wT"], L.EPI_RESID_F32, resid=dt1, out_f32=d_out)
        if T["cross_layers"]:         # d(encoder-side states) = sum over the layers of [dK | dV]_l Wkv_l: one product, K = n 1536
            nc = len(T["cross_layers"])
            L.gemm_bf16_nt(g["bkv"][:enc16.shape[0], :nc * 2 * H], T["kv_all"]["wT"], L.EPI_F32, out_f32=d_enc)
        return d_out

    def _vit_bwd(self, S, mode: str, d_img):
        """d_img: fp32 [Mi,768] gradient wrt image_embeds (the final norm's output)."""
        H, g, vt, Mi = self.H, self.gs[mode], self.vit, self.Mi
        V = S["vit"]
        cur, oth = g["d1"][:Mi], g["d2"][:Mi]
        L.layernorm_bwd_dx(V["out"], V["stf"], vt["ng"], Mi, H, dy_f32=d_img, out_f32=cur)
        for i in range(self.vd - 1, -1, -1):
            W, A = vt["blocks"][i], V["blocks"][i]
            if i == 0:       # nothing trainable below the first adapter: weight gradients only
                L.adapter_bwd(None, cur, None, self._segs(0, mode, Mi, True), Mi, z_out=g["z"], dz_out=g["dz"],
                              z_saved=A["zs"])
                self._wgrad(0, mode, A["h3"], cur, Mi)
                break
            L.adapter_bwd(None, cur, oth, self._segs(i, mode, Mi, True), Mi, dx_bf16=g["b1"][:Mi], z_out=g["z"],
                          dz_out=g["dz"], z_saved=A["zs"])
            self._wgrad(i, mode, A["h3"], cur, Mi)
            L.gemm_bf16_nt(g["b1"][:Mi], W["fc2"]["wT"], L.EPI_MUL_G8 if A["u"].dtype == torch.uint8 else L.EPI_MUL_DGELU,
                           aux=A["u"], out_bf16=g["bI"][:Mi])
            L.gemm_bf16_nt(g["bI"][:Mi], W["fc1"]["wT"], L.EPI_BF16, out_bf16=g["b2"][:Mi])
            L.layernorm_bwd_dx(A["h2"], A["st2"], W["n2g"], Mi, H, dy_bf16=g["b2"][:Mi], dres=oth, out_f32=cur,
                               out_bf16=g["b1"][:Mi])
            L.gemm_bf16_nt(g["b1"][:Mi], W["proj"]["wT"], L.EPI_BF16, out_bf16=g["b2"][:Mi])
            dqkv = g["b3"][:Mi]
            L.attn2_bwd(A["qkv"][:, :H], A["qkv"][:, H:2 * H], A["qkv"][:, 2 * H:], A["ctx"], A["lse"], g["b2"][:Mi],
                        g["dsum"], dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:], self.B, self.Ni, self.Ni, self.heads)
            L.gemm_bf16_nt(dqkv, W["qkv"]["wT"], L.EPI_BF16, out_bf16=g["b2"][:Mi])
            L.layernorm_bwd_dx(A["h_in"], A["st1"], W["n1g"], Mi, H, dy_bf16=g["b2"][:Mi], dres=cur, out_f32=oth)
            cur, oth = oth, cur

    def _backward(self, mode: str, teacher_logits, pass_id=None):
        """L = (loss + kl) / 2 of the pass `mode` (task_trainer.py:300-302 / 320-323) -> gradients of its trainable adapter."""
        self._backward_text(mode, teacher_logits, pass_id)
        self._vit_bwd(self.acts[mode], mode, self.gs[mode]["d_img"])
        self._wgrad_reduce(mode)

    def _loss(self, logits, teacher, dlogits, own: str):
        """L = (loss + KL(logits || teacher)) / 2 of the R rows of the pass `own` ("gating" | "adapter_1") and dL/dlogits, scaled."""
        L.lm_loss_fwd_bwd(logits, teacher, self.labels, self.row_w, self.V, 3.0, 9.0 / self.N, dlogits, self.acts[own]["loss"],
                          row_kl=self.row_kl, **self._scale_in(own))

    def _backward_text(self, mode: str, teacher_logits, pass_id=None):
        """Loss, LM head, decoder and text encoder backward of the pass `mode`; leaves d(image_embeds) in its scratch set.
        mode "both": the two passes stacked, each half's MKD teacher the OTHER half's logits (teacher_logits unused)."""
        S, g = self.acts[mode], self.gs[mode]
        R = self.R
        if mode == "both":       # L_0 = (loss_0 + KL(logits_0 || logits_1)) / 2 on rows [0, R), L_1 likewise on rows [R, 2R)
            lg = S["logits"]
            for half, own in ((0, "gating"), (1, "adapter_1")):
                self._loss(lg[half * R:(half + 1) * R], lg[(1 - half) * R:(2 - half) * R], g["dlogits"][half * R:(half + 1) * R], own)
        else:
            self._loss(S["logits"], teacher_logits, g["dlogits"], mode)
        self._lm_head_bwd(S, g, 0, self.tx["both" if mode == "both" else "single"]["R"])
        self._towers_bwd(mode, pass_id)

    def _lm_head_bwd(self, S, g, lo: int, hi: int, grads: bool = False, flag=None):
        """LM head backward of rows [lo, hi): logits = LN(gelu(dense(h))) W_emb^T; dlogits -> d(selected decoder rows) in
        g["d1"][lo:hi].  grads (a sub-step of a step that trains the head; flag: that sub-step's overflow flag under the dynamic
        scale): the gradients of the head's five tensors go into the head group's gradient buffer, unscaled --
          d bias        column sums of the 16-bit dlogits [rows, Vp]                      feddat_colsum_partial
          d gamma, beta sum_r dy xhat, sum_r dy of the transform LayerNorm (dy fp32)      feddat_ln_param_grad_partial
          d dense.bias  column sums of d2 = d(dense output), fp32                         feddat_colsum_partial
            (the four folded, unscaled and inf-checked in ONE feddat_vector_grad_reduce)
          d dense.W     d2^T x over the rows, x = the fp32 selected decoder rows          feddat_head_gemm (fp32 MFMA, unscaled by alpha)
        all fixed-order sums.  d dense.W has no inf check of its own: it is non-finite only where d2 is (x is a LayerNorm
        output), and then so are d2's column sums, which are checked."""
        hd, H, n = self.head, self.H, hi - lo
        train = bool(grads)
        dl, b1, d1, d2 = g["dlogits"][lo:hi], g["b1"][lo:hi], g["d1"][lo:hi], g["d2"][lo:hi]
        if train:
            # dy = d(LayerNorm output) stays fp32 here (the frozen-head path rounds it to the operand format) and is formed with
            # the decoder weight to about twice the operand's mantissa (two products): it feeds the sums for gamma / beta and,
            # through d2, those for transform.dense
            dy = g["d3"][lo:hi]
            L.gemm_bf16_nt(dl, hd["wT"], L.EPI_F32, out_f32=g["d4"][lo:hi])
            L.gemm_bf16_nt(dl, hd["wT_lo"], L.EPI_RESID_F32, resid=g["d4"][lo:hi], out_f32=dy)       # + dlogits (W_emb - W_emb16)
            L.colsum_partial(dl, self.hg["bias"])
            L.ln_param_grad_partial(dy, S["tg"][lo:hi], S["tst"][lo:hi], self.hg["beta"], self.hg["gamma"])
            L.layernorm_bwd_dx(S["tg"][lo:hi], S["tst"][lo:hi], hd["lng"], n, H, dy_f32=dy, out_f32=d1)
        else:
            L.gemm_bf16_nt(dl, hd["wT"], L.EPI_BF16, out_bf16=b1)
            L.layernorm_bwd_dx(S["tg"][lo:hi], S["tst"][lo:hi], hd["lng"], n, H, dy_bf16=b1, out_f32=d1)
        L.gelu_bwd(S["tu"][lo:hi], d1, d2)
        if train:
            L.colsum_partial(d2, self.hg["db"])
            key = ("head-wgrad", d2.data_ptr(), S["hsel"].data_ptr(), lo, self._dyn())
            if key not in self._segs_cache:
                gw = self.lm.view(self.lm.names[0], self.lm.g)
                us = dict(alpha=1.0, alpha_dev=self.scaler_f[1:2]) if self._dyn() else dict(alpha=1.0 / self.loss_scale)
                # out[i, j] = sum_r d2[r, i] x[r, j]: A[i, k] = d2[k, i], B[k, j] = x[k, j]
                self._segs_cache[key] = L.ht_job(d2, 1, H, S["hsel"][lo:hi], H, 1, H, H, n, gw, **us)
            L.head_gemm(self._segs_cache[key])
        L.cvt_f32_bf16(d2, b1)
        L.gemm_bf16_nt(b1, hd["t"]["wT"], L.EPI_F32, out_f32=d1)
        if train:
            table, njobs, max_n = self.hg_table
            us = dict(unscale=1.0, unscale_dev=self.scaler_f[1:2]) if self._dyn() else dict(unscale=1.0 / self.loss_scale)
            L.vector_grad_reduce(table, njobs, max_n, nonfinite=flag, **us)

    def _towers_bwd(self, mode: str, pass_id=None):
        """From the gradient of the selected decoder rows (g["d1"], left by _lm_head_bwd) down: decoder and text encoder
        backward of the pass `mode`; leaves d(image_embeds) in its scratch set."""
        S, g, H = self.acts[mode], self.gs[mode], self.H
        t = self.tx["both" if mode == "both" else "single"]
        R = t["R"]
        L.gather_rows(g["d1"][:R], t["unsel_idx"], dst_f32=g["d_dec"])          # zero rows at the last position of each answer
        emb16 = self.emb16_both if mode == "both" else S["vit"]["emb16"]
        self._bert_bwd(self.dec, S["dec"], self.vd + self.el, mode, t["Ma"], t["na"], self.La, t["amask8"], True,
                       S["enc_rep16"], self.Lq, self.Lq, t["qmask8_rep"], g["d_dec"], g["d_rep"], pass_id, 1)
        # question states were repeated per answer: sum the answers of each question back (rows = [N, Lq * H])
        L.segment_sum_rows(g["d_rep"].view(t["na"], self.Lq * H), t["seg_off"], g["d_qs"].view(t["nq"], self.Lq * H))
        self._bert_bwd(self.enc, S["enc"], self.vd, mode, t["Mq"], t["nq"], self.Lq, t["qmask8"], False, emb16,
                       self.Ni, self.Ni, None, g["d_qs"], g["d_img"], pass_id, 0)

    # ------------------------------------------------------------------------------------------ train step
    @_bound
    def begin_local_update(self, steps_per_epoch: int, num_epochs: int = 15, warmup_ratio: float = 0.1,
                           opt_adapters: Sequence[int] = (0, 1), dropout_epoch: int = 0):
        """TaskTrainer.train prologue (task_trainer.py:36-59): teacher snapshot, fresh AdamW state and schedule.
        dropout_epoch: which local update this is, federation-wide (train.main passes round * n_clients + client index).  The
        masks are a function of (seed, site, step counter): the counter starts at dropout_epoch * 2^16, so every round and
        every client draws its own masks -- like the reference's nn.Dropout, which keeps consuming the global RNG across
        rounds and clients -- and a resumed run reproduces them without any saved RNG state."""
        self.copy_global_to_teacher()
        self.opt_adapters = tuple(opt_adapters)
        self.drop_ctr.copy_(torch.tensor([(int(dropout_epoch) << 16) & 0x7FFFFFFF, 0], dtype=torch.int32))
        # adapter_1 is stepped at tick 2b, adapter_0 at tick 2b + 1
        self._start_local_update(steps_per_epoch, num_epochs, warmup_ratio, {"adapter_0": (1, 0)})

    def _graph_switches(self):
        return (self.dropout, self.batch_text, self.train_lm_head)

    def _named_groups(self):
        groups = [("adapter_0", self.ad[0]), ("adapter_1", self.ad[1])]
        return groups + [("lm_head", self.lm)] if self.train_lm_head else groups

    def _state_groups(self):
        return list(self.ad) + ([self.lm] if self.train_lm_head else [])

    def _extra_step_state(self):
        return [self.drop_ctr]

    @_bound
    def _capture(self):
        super()._capture()
        if self.train_lm_head:      # the head's tensors are back at their state before the capture: so are its operand copies
            self._refresh_head()
            torch.cuda.synchronize()

    @_bound
    def load_tensors(self, tensors: Dict[str, torch.Tensor]):
        super().load_tensors(tensors)
        if self.train_lm_head and any(n in self.lm.offsets for n in tensors):
            self._refresh_head()

    def repack(self):
        super().repack()
        if self.train_lm_head:
            self._refresh_head()

    # The two passes are independent up to the loss and from the loss down to their adapters, so they run side by side on two
    # streams (separate activation, scratch and weight-gradient workspaces per pass; inside a captured step the fork / join
    # become graph edges): the text towers' launches are small (25-token questions, 4-token answers: 24-156 workgroups) and
    # overlap each other, and the other pass's kernels fill the CUs that the last, partial round of an image-encoder GEMM
    # leaves idle (388 tiles on 256 CUs at N = 768).
    def _streams(self):
        """(the current stream, the step's second stream)."""
        if self.side is None:
            self.side = torch.cuda.Stream(device=self.dev)
        return torch.cuda.current_stream(), self.side

    def _stacked(self) -> bool:
        """The step runs in its stacked form (dropout = 0, stack_text, both adapters optimised)."""
        return self.batch_text and self.opt_adapters == (0, 1)

    def _forward_stacked(self):
        """Forward of the stacked form: the image encoder ahead of block 0's adapter once, the rest of the two passes' image
        encoders side by side, then ONE text-side forward over both passes' rows.  -> logits [2R, Vp]: rows [0, R) gated,
        [R, 2R) adapter_1."""
        cur, side = self._streams()
        self._vit_fwd(self.acts["gating"], "gating", "prefix")
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            self._vit_fwd(self.acts["gating"], "gating", "suffix")
        self._vit_fwd(self.acts["adapter_1"], "adapter_1", "suffix")
        cur.wait_stream(side)
        return self._forward_text("both")

    def _image_bwd_stacked(self, d_img):
        """Image-encoder backward of the stacked form, the two passes side by side.  d_img: fp32 [2 Mi, 768], the gradient wrt
        the stacked image_embeds that the text-side backward left."""
        cur, side = self._streams()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            self._vit_bwd(self.acts["gating"], "gating", d_img[:self.Mi])
            self._wgrad_reduce("gating")
        self._vit_bwd(self.acts["adapter_1"], "adapter_1", d_img[self.Mi:])
        self._wgrad_reduce("adapter_1")
        self._wgrad_reduce("both")
        cur.wait_stream(side)

    def _forward_two_passes(self):
        """Forward of the two-stream form: the image encoder ahead of block 0's adapter once for both passes (frozen,
        adapter-free, no dropout), then the gated pass on the second stream and the adapter_1 pass (P1, task_trainer.py:290-295)
        on the current one, joined.  -> (teacher logits, logits_1).  The teacher is the gated forward: P0 == P2
        (task_trainer.py:283-287,311-315) -- except under dropout, where P0 is the no-grad gated forward under its own masks,
        copied to logits_all: the image encoder has no dropout, so its gated forward is still shared with P2, but the gated
        text towers run again for P2 (other masks), in the schedule."""
        cur, side = self._streams()
        drop = self.dropout > 0
        self._vit_fwd(self.acts["gating"], "gating", "prefix")
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            self._vit_fwd(self.acts["gating"], "gating", "suffix")
            if drop:
                self.logits_all.copy_(self._forward_text("gating", 0))
                teacher = self.logits_all
            else:
                teacher = self._forward_text("gating")
        self._vit_fwd(self.acts["adapter_1"], "adapter_1", "suffix")
        logits_1 = self._forward_text("adapter_1", 1 if drop else None)
        cur.wait_stream(side)
        return teacher, logits_1

    def _step_kernels_head(self):
        """The step with a trainable LM head (task_trainer.py:280-330; the head is in the optimizer of BOTH sub-steps):
          1. towers of both passes up to the decoder output, LM head with the OLD head -> logits_all (P0), logits_1 (P1)
          2. L_1; LM-head backward of the P1 rows through the old head; the head's gradients; AdamW on the head at tick 2b
          3. the head's operand copies rebuilt (feddat_lm_head_refresh)
          4. the LM head AGAIN on the gated pass's decoder output -- only the head changed, the towers are not re-run (with
             dropout P2's text towers are a pass of their own anyway: it simply runs here, after the update) -> logits_0
          5. L_0 against the PRE-update logits_1; LM-head backward of the gated rows through the UPDATED head; its gradients
          6. the towers' backward of both passes (adapter_1's starts on the second stream as soon as 2. is done)
          7. _dat_tail with the head: adapter_1 (2b), head (2b + 1), adapter_0 (2b + 1), GradScaler's predicates; operands again.
        An adapter_0 that left the optimizer (server flags after an eval) drops its towers' backward only: the reference's
        optimizer holds the head either way, so 5. still runs."""
        cur, side = self._streams()
        drop = self.dropout > 0
        fB, fA = (self.ovf_flags[0:1], self.ovf_flags[1:2]) if self._dyn() else (None, None)
        R = self.R
        Sg, S1, gg, g1 = self.acts["gating"], self.acts["adapter_1"], self.gs["gating"], self.gs["adapter_1"]
        if self._stacked():
            # the stacked form: rows [0, R) gated, [R, 2R) adapter_1 of one text-side pass
            lg = self._forward_stacked()
            S, g = self.acts["both"], self.gs["both"]
            self._loss(lg[R:], lg[:R], g["dlogits"][R:], "adapter_1")
            self._lm_head_bwd(S, g, R, 2 * R, True, fA)
            self._head_step_a()
            self._lm_head_fwd(S, 0, R)
            self._loss(lg[:R], lg[R:], g["dlogits"][:R], "gating")
            self._lm_head_bwd(S, g, 0, R, True, fB)
            self._towers_bwd("both")
            self._image_bwd_stacked(g["d_img"])
        else:
            teacher, logits_1 = self._forward_two_passes()
            self._loss(logits_1, teacher, g1["dlogits"], "adapter_1")
            self._lm_head_bwd(S1, g1, 0, R, True, fA)
            self._head_step_a()
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                self._towers_bwd("adapter_1", 1 if drop else None)
                self._vit_bwd(S1, "adapter_1", g1["d_img"])
                self._wgrad_reduce("adapter_1")
            if drop:       # the gated text towers again, under P2's masks
                logits_0 = self._forward_text("gating", 2)
            else:
                self._lm_head_fwd(Sg, 0, R)
                logits_0 = Sg["logits"]
            self._loss(logits_0, logits_1, gg["dlogits"], "gating")
            self._lm_head_bwd(Sg, gg, 0, R, True, fB)
            if 0 in self.opt_adapters:
                self._towers_bwd("gating", 2 if drop else None)
                self._vit_bwd(Sg, "gating", gg["d_img"])
                self._wgrad_reduce("gating")
            cur.wait_stream(side)
        self._dat_tail(self.lm, self.head_bak)
        self._refresh_head()
        if drop:
            L.step_tick(self.drop_ctr, 1, 0)

    @_bound
    def _step_kernels(self):
        if self.train_lm_head:
            return self._step_kernels_head()
        drop = self.dropout > 0
        if self._stacked():
            # dropout = 0: the image encoders of the two passes side by side, then ONE text-side forward / backward over both
            # passes' rows, then the two image-encoder backward passes side by side
            self._forward_stacked()
            self._backward_text("both", None)
            self._image_bwd_stacked(self.gs["both"]["d_img"])
        else:
            cur, side = self._streams()
            logits_teacher, logits_1 = self._forward_two_passes()
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                logits_g = self._forward_text("gating", 2) if drop else logits_teacher
                if 0 in self.opt_adapters:
                    self._backward("gating", logits_1, 2 if drop else None)   # L_0 = (loss_0 + KL(logits_0 || logits_1)) / 2
                else:        # adapter_0 left the optimizer (server flags after the first eval): only the loss values are needed
                    L.lm_loss_fwd_bwd(logits_g, logits_1, self.labels, self.row_w, self.V, 3.0, 9.0 / self.N, None,
                                      self.acts["gating"]["loss"], row_kl=self.row_kl)
            self._backward("adapter_1", logits_teacher, 1 if drop else None)  # L_1 = (loss_1 + KL(logits_1 || logits_all)) / 2
            cur.wait_stream(side)
        self._dat_tail()        # the DAT tail without a head
        if drop:
            L.step_tick(self.drop_ctr, 1, 0)                 # the next train_step draws fresh masks (also under graph replay)

    def _loss_tensor(self):
        """What train_step returns: the device buffer {loss_0, kl_0, L_0} of the P2 pass (the reference returns loss_0).  A
        step is ~3000 launches (the BERT towers' are tiny: without use_graph the step is host-bound)."""
        return self.acts["gating"]["loss"]
