"""ALBEF (ViT-B/16 + BERT-base encoder + 6-layer decoder) dual-adapter (DAT + MKD) local-update engine on MI355X --
BASELINE.json configs[3].

Host-side sequencing of the HIP kernels in libfeddat_hip.so for the reference's two-stream path: ALBEF.forward(train=True)
(src/modeling/models/albef_model.py:69-145) inside the dat branch of TaskTrainer.train_step
(src/train/visionlanguage_tasks/task_trainer.py:280-330, ALBEF wiring :296-297,316-317, vocabulary-axis KL :506-516), with
the adapters of vit.py:99-110 (after the MLP residual) and xbert.py:438-445 / adapter.py:97-116 (BertOutput, same LayerNorm
before and after the adapter).  As in the ViLT engine, no arithmetic happens in Python / PyTorch: torch owns device
buffers and the stream, every launch goes through the C ABI.

Step algebra.  The reference trains the adapters (main.py:138-159) AND the decoder's LM head: prepare_model ends by making every
parameter whose name contains `.cls.` trainable (main.py:247-250 -- text_decoder.cls.predictions.{bias, transform.dense.weight,
transform.dense.bias, transform.LayerNorm.weight, transform.LayerNorm.bias}; the tied decoder.weight is listed under the word
embeddings and stays frozen), and `.cls.` is personal (main.py:127-128): per client, never averaged.  Here that is the opt-in
`train_lm_head=True`; the DEFAULT (False) still keeps the head frozen, which is what the fixtures G10 - G12 were captured with.
With the head frozen the no-grad gated pass P0 and the gated pass P2 of one train_step are the same computation (P1 updates
adapter_1 only, the gated passes read adapter_0 / adapter_2) -> the gated forward runs ONCE; its logits serve as the teacher of
P1 and as the student of P2.  With the head trainable the towers of P0 and P2 are still the same computation, but P1's optimizer
step moves the head between them (create_optimizer takes every requires_grad parameter, so the head is stepped in BOTH sub-steps:
task_trainer.py:302-308,323-328): the gated decoder output is kept and only the LM head runs again on it with the updated
tensors (_step_kernels_head).  Nothing trainable lies below the first ViT block's adapter, so the backward stops there.

Dropout.  The reference trains under model.train() (task_trainer.py:75) with hidden_dropout_prob =
attention_probs_dropout_prob = 0.1 (src/configs/model_configs.py:44-46) in the two BERT towers -- after the embedding
LayerNorm (xbert.py:216), on the attention probabilities (:333), on BertSelfOutput's dense output (:360) and on BertOutput's
dense output ahead of the adapter (:440); the ViT has none (vit.py:120).  `dropout=p` reproduces that with counter-based
masks (seed, train step, pass, site, element -> bit; include/feddat_hip.h) that the backward regenerates.  With p > 0 the P0
and P2 forwards draw DIFFERENT masks (three independent forwards in the reference), so the "gated forward once" identity
only holds for the image encoder: the text towers then run three times (P0 no-grad, P1, P2).  dropout=0 (the default) is
the deterministic configuration every parity fixture except g12 is captured in; feddat_amd.train.main passes the
reference's 0.1 (--albef_dropout).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from . import lib as L
from .local_update import FlatGroup, LocalUpdateEngine, _bound

PRE = "albef_model.albef."
ADAPTER_TENSORS = ("down.weight", "down.bias", "up.weight", "up.bias")


def rank_slab_plan(nq: int, k: int, N: int, B: int) -> List[List[int]]:
    """rank_answer on a frame of N answers: the nq * k candidates (candidate c = b * k + j, question b's j-th shortlisted answer)
    go through the decoder in slabs of N, slab s = the candidates [s N, min((s + 1) N, nq k)) -- a slab may straddle questions and
    the last one may be partial.  Returns, per slab, ks[b] = how many of the slab's rows belong to question b (length B; sum <= N;
    over the slabs, k for b < nq and 0 for the replicas b >= nq).  Pure host arithmetic: needs no device."""
    if not (1 <= nq <= B and k >= 1 and N >= B):
        raise L.FeddatHipError(f"rank_slab_plan: need 1 <= nq <= B <= N and k >= 1, got nq={nq}, k={k}, N={N}, B={B}")
    plan = []
    for first in range(0, nq * k, N):
        ks = [0] * B
        for c in range(first, min(first + N, nq * k)):
            ks[c // k] += 1
        plan.append(ks)
    return plan


def slab_question_of_row(ks: Sequence[int], N: int) -> List[int]:
    """Question whose states row i of an N-answer frame reads: the rows of question b are consecutive, ks[b] of them, in question
    order; rows behind the last candidate ride with the last question that has one (they carry no loss)."""
    q = [b for b, n in enumerate(ks) for _ in range(n)]
    return q + [q[-1]] * (N - len(q))


LM_HEAD = PRE + "text_decoder.cls.predictions."


def lm_head_group_spec(vocab: int, H: int = 768):
    """(names and shapes, padding) of the flat group that holds the trainable LM head: the five tensors main.py:247-250 makes
    trainable on ALBEF (622 650 floats at a vocabulary of 30 522), transform.dense.weight first (16-byte aligned for the refresh
    kernel), the vocabulary bias last and followed by the padding of the vocabulary axis to a multiple of 128.  Weight decay
    follows the names (local_update._no_decay): transform.dense.weight alone is decayed."""
    spec = [(LM_HEAD + "transform.dense.weight", (H, H)), (LM_HEAD + "transform.dense.bias", (H,)),
            (LM_HEAD + "transform.LayerNorm.weight", (H,)), (LM_HEAD + "transform.LayerNorm.bias", (H,)),
            (LM_HEAD + "bias", (vocab,))]
    return spec, (vocab + 127) // 128 * 128 - vocab


class AlbefDatEngine(LocalUpdateEngine):
    def __init__(self, params: Dict[str, torch.Tensor], device, batch: int, n_answers: int, q_len: int = 25, a_len: int = 4,
                 vit_depth: int = 12, enc_layers: int = 12, fusion_layer: int = 6, dec_layers: int = 6, image: int = 384,
                 vocab: int = 30522, lr: float = 1e-4, weight_decay: float = 1e-2, adam_eps: float = 1e-8, pad_id: int = 0,
                 max_pos: int = 512, dropout: float = 0.0, seed: int = 0, stack_text: bool = False,
                 operands: str = "f16", loss_scale: Optional[float] = None, dynamic_loss_scale: Optional[bool] = None,
                 scale_growth_interval: int = 2000, train_lm_head: bool = False):
        """train_lm_head: train text_decoder.cls.predictions.* as the reference does (module docstring); off by default.
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
            self._init(params, device, batch, n_answers, q_len, a_len, vit_depth, enc_layers, fusion_layer, dec_layers, image, vocab,
                       lr, weight_decay, adam_eps, pad_id, max_pos, dropout, seed, stack_text)

    def _init(self, params, device, batch, n_answers, q_len, a_len, vit_depth, enc_layers, fusion_layer, dec_layers, image, vocab, lr,
              weight_decay, adam_eps, pad_id, max_pos, dropout, seed, stack_text):
        L.load()
        if not 0.0 <= dropout < 1.0:
            raise L.FeddatHipError("dropout must be in [0, 1)")
        self.dropout, self.seed = float(dropout), int(seed)
        self.dev = dev = torch.device(device)
        self.B, self.N, self.Lq, self.La = batch, n_answers, q_len, a_len
        self.vd, self.el, self.fl, self.dl = vit_depth, enc_layers, fusion_layer, dec_layers
        self.H, self.I, self.heads, self.r, self.P = 768, 3072, 12, 48, 16
        self.img = image
        self.gp = image // self.P
        self.Ni = self.gp * self.gp + 1
        self.V, self.Vp = vocab, ((vocab + 127) // 128) * 128
        self.pad_id = pad_id
        self.lr, self.wd, self.eps = lr, weight_decay, adam_eps
        H, I = self.H, self.I
        self.Mi, self.Mq, self.Ma, self.R = batch * self.Ni, batch * q_len, n_answers * a_len, n_answers * (a_len - 1)

        def Pm(name):
            return params[PRE + name].to(dev, torch.float32).contiguous()

        def bf16_of(w):
            out = torch.empty(w.shape, dtype=self.op_dtype, device=dev)
            L.cvt_f32_bf16(w.contiguous(), out)
            return out

        def bf16_T(w):
            out = torch.empty(w.shape[1], w.shape[0], dtype=self.op_dtype, device=dev)
            L.transpose_f32_bf16(w.contiguous(), out, w.shape[0], w.shape[1])
            return out

        def lin(prefix):          # forward operand, transposed operand (dX), bias
            w = Pm(prefix + ".weight")
            return dict(w=bf16_of(w), wT=bf16_T(w), b=Pm(prefix + ".bias"))

        # ---------------- frozen ViT-B/16 ----------------
        v = "visual_encoder."
        self.vit = dict(cls=Pm(v + "cls_token").reshape(H), pos=Pm(v + "pos_embed")[0].contiguous(),
                        wp=bf16_of(Pm(v + "patch_embed.proj.weight").reshape(H, 3 * self.P * self.P)),
                        bp=Pm(v + "patch_embed.proj.bias"), ng=Pm(v + "norm.weight"), nb=Pm(v + "norm.bias"), blocks=[])
        for i in range(vit_depth):
            b = f"{v}blocks.{i}."
            self.vit["blocks"].append(dict(qkv=lin(b + "attn.qkv"), proj=lin(b + "attn.proj"), fc1=lin(b + "mlp.fc1"),
                                           fc2=lin(b + "mlp.fc2"), n1g=Pm(b + "norm1.weight"), n1b=Pm(b + "norm1.bias"),
                                           n2g=Pm(b + "norm2.weight"), n2b=Pm(b + "norm2.bias")))
        self.zero_h = torch.zeros(H, device=dev)

        # ---------------- frozen BERT towers ----------------
        def attn_block(prefix, cross):
            wq, wk, wv = (Pm(f"{prefix}self.{n}.weight") for n in ("query", "key", "value"))
            bq, bk, bv = (Pm(f"{prefix}self.{n}.bias") for n in ("query", "key", "value"))
            d = dict(o=lin(prefix + "output.dense"), lng=Pm(prefix + "output.LayerNorm.weight"),
                     lnb=Pm(prefix + "output.LayerNorm.bias"))
            if cross:          # Q from the text stream, K | V fused from the other stream
                d.update(q=dict(w=bf16_of(wq), wT=bf16_T(wq), b=bq),
                         kv=dict(w=bf16_of(torch.cat([wk, wv], 0)), wT=bf16_T(torch.cat([wk, wv], 0)), b=torch.cat([bk, bv])))
            else:
                w = torch.cat([wq, wk, wv], 0)
                d.update(qkv=dict(w=bf16_of(w), wT=bf16_T(w), b=torch.cat([bq, bk, bv])))
            return d

        def tower(prefix, layers, fusion):
            e = prefix + "embeddings."
            t = dict(word=Pm(e + "word_embeddings.weight"), pos=Pm(e + "position_embeddings.weight"),
                     typ=Pm(e + "token_type_embeddings.weight"), lng=Pm(e + "LayerNorm.weight"), lnb=Pm(e + "LayerNorm.bias"),
                     layers=[])
            for i in range(layers):
                Lp = f"{prefix}encoder.layer.{i}."
                t["layers"].append(dict(att=attn_block(Lp + "attention.", False),
                                        cross=attn_block(Lp + "crossattention.", True) if i >= fusion else None,
                                        fc1=lin(Lp + "intermediate.dense"), fc2=lin(Lp + "output.dense"),
                                        lng=Pm(Lp + "output.LayerNorm.weight"), lnb=Pm(Lp + "output.LayerNorm.bias")))
            # The cross-attention K | V projections of ALL fusion layers read the same encoder-side states (image_embeds for
            # the text encoder, the repeated question states for the decoder): ONE product with the layers' weights stacked
            # along N in the forward ([rows, n_cross * 1536], each layer's K | V a column slice), and ONE product over the
            # stacked dK | dV columns (K = n_cross * 1536) for the gradient of those states in the backward -- instead of six
            # 18 464-row launches of N = 1536 and six read-modify-write passes over the fp32 gradient.
            cross = [i for i, Ly in enumerate(t["layers"]) if Ly["cross"] is not None]
            t["cross_layers"] = cross
            if cross:
                t["kv_all"] = dict(w=torch.cat([t["layers"][i]["cross"]["kv"]["w"] for i in cross], 0).contiguous(),
                                   b=torch.cat([t["layers"][i]["cross"]["kv"]["b"] for i in cross], 0).contiguous(),
                                   wT=torch.cat([t["layers"][i]["cross"]["kv"]["wT"] for i in cross], 1).contiguous())
                for i in cross:          # the per-layer copies are not used any more
                    t["layers"][i]["cross"]["kv"] = None
            return t
        self.enc = tower("text_encoder.", enc_layers, fusion_layer)
        self.dec = tower("text_decoder.bert.", dec_layers, 0)
        c = "text_decoder.cls.predictions."
        wemb = torch.zeros(self.Vp, H, device=dev)
        wemb[:vocab] = self.dec["word"]                      # tied LM-head weight, vocabulary padded to a multiple of 128
        bpad = torch.zeros(self.Vp, device=dev)
        bpad[:vocab] = Pm(c + "bias")
        self.head = dict(t=lin(c + "transform.dense"), lng=Pm(c + "transform.LayerNorm.weight"),
                         lnb=Pm(c + "transform.LayerNorm.bias"), w=bf16_of(wemb), wT=bf16_T(wemb), b=bpad)
        del wemb
        self.lm = None
        if self.train_lm_head:
            # the five trainable head tensors in one flat fp32 group (AdamW state; weight decay on transform.dense.weight alone:
            # local_update._no_decay).  The vocabulary bias comes last, followed by the Vp - V floats of vocabulary padding, so that
            # its gradient -- the column sums of the [R, Vp] dlogits -- is reduced at the padded width.  The kernels read the fp32
            # vectors (dense bias, LayerNorm gamma / beta) straight from the group; W, W^T and the padded bias are operand copies
            # that feddat_lm_head_refresh rewrites after every head update.
            c_ = PRE + c
            spec, pad = lm_head_group_spec(vocab, H)
            self.lm = FlatGroup(spec, dev, with_opt=True, pad=pad)
            for n in self.lm.names:
                self.lm.view(n).copy_(params[n].to(dev, torch.float32))
            self.head["t"]["b"] = self.lm.view(c_ + "transform.dense.bias")
            self.head["lng"] = self.lm.view(c_ + "transform.LayerNorm.weight")
            self.head["lnb"] = self.lm.view(c_ + "transform.LayerNorm.bias")
            # the tied decoder weight a second time: the 16-bit REMAINDER of its 16-bit copy (W_emb - fp32(operand(W_emb)), frozen,
            # formed once here).  dy = dlogits W_emb is dominated by the rows of the label tokens, so the operand rounding of those
            # embedding rows goes straight into the head's gradients; a second product with the remainder removes it.
            wemb = torch.zeros(self.Vp, H, device=dev)
            wemb[:vocab] = self.dec["word"]
            self.head["wT_lo"] = bf16_T(wemb - self.head["w"].float())
            del wemb
            self._refresh_head()

        # ---------------- trainable state: three adapters over the 30 modules, flat per adapter ----------------
        self.modules: List[str] = [f"visual_encoder.blocks.{i}.adapter." for i in range(vit_depth)] + \
            [f"text_encoder.encoder.layer.{i}.output.adapter." for i in range(enc_layers)] + \
            [f"text_decoder.bert.encoder.layer.{i}.output.adapter." for i in range(dec_layers)]
        shp = {"down.weight": (self.r, H), "down.bias": (self.r,), "up.weight": (H, self.r), "up.bias": (H,)}
        self.ad = [FlatGroup([(PRE + m + f"adapter_{a}_{t}", shp[t]) for m in self.modules for t in ADAPTER_TENSORS], dev,
                             with_opt=(a != 2)) for a in range(3)]
        for grp in self.ad:
            for n in grp.names:
                grp.view(n).copy_(params[n].to(dev, torch.float32))
        self.ad_numel = self.r * H + self.r + H * self.r + H
        nm = len(self.modules)
        self._pack16 = [torch.empty(nm, 4, self.r * H, dtype=self.op_dtype, device=dev) for _ in range(3)]
        for a in range(3):
            self.repack_adapter(a)
        self.sched = dict(warmup=1, total=2)
        self.opt_adapters = (0, 1)
        self.graph = None
        self._segs_cache: Dict = {}
        self._rank_cache: Dict = {}          # rank_answer's slab maps per (nq, k)
        # weight-gradient partial sums: one slot per adapter module and pass; ONE batched reduction per backward pass folds them
        # into the flat gradient buffers (feddat_adapter_wgrad_partial / _reduce) instead of one reduce launch per module
        self.wpart_stride = L.adapter_wgrad_workspace_elems(1)
        self.wpart = {m: torch.empty(len(self.modules) * self.wpart_stride, device=dev) for m in ("gating", "adapter_1")}
        self._wg_done = {m: [] for m in ("gating", "adapter_1", "both")}
        # stack_text (round 4, OFF by default -- measured slower): with dropout = 0 the text towers of the gated and the
        # adapter_1 pass are the same launches on different rows, so they can run ONCE on 2x the rows (rows [0, M) gated,
        # [M, 2M) adapter_1 -- the ViLT engine's 2R-row batching; adapters, weight gradients and the two losses take
        # two-segment descriptors): 366 -> 183 text-side GEMM launches per step, results equal to the two-pass form
        # (tests/test_albef_gpu.py::test_stacked_text_towers_equal_the_two_separate_passes).  Under hipGraph replay it LOSES:
        # 34.6 against 32.6 ms / step at B = 32 in round 4, 31.2 against 30.4 in round 5 once its 1600-row products left the
        # persistent GEMM kernels (36 tiles = 36 CUs) for the small-tile one (same box, tools/albef_stack_ab.py) -- the two passes' small kernels already
        # overlap each other on two streams, and a stacked launch of twice the rows costs more than one of the pair.  It
        # stays as a switch because it halves the host launches of the eager (no-graph) step.
        self.batch_text = bool(stack_text) and self.dropout <= 0
        if self.batch_text:
            self.wpart_stride2 = L.adapter_wgrad_workspace_elems(2)
            self.wpart["both"] = torch.empty(len(self.modules) * self.wpart_stride2, device=dev)
        self.side = None           # second stream of train_step (created lazily on the engine's device)
        self._alloc_scaler()
        self.drop_ctr = torch.zeros(2, dtype=torch.int32, device=dev)      # [0] = train_steps since begin_local_update
        self._alloc()
        if self.dropout > 0:       # teacher logits of P0: the gated text pass is re-run (other masks) for P2
            self.logits_all = torch.empty(self.R, self.Vp, device=dev)
        if self.train_lm_head:
            self._alloc_head_grads()

    # ------------------------------------------------------------------------------------------ buffers
    def _alloc(self):
        dev, H, I = self.dev, self.H, self.I

        def f32(*s):
            return torch.empty(*s, device=dev)

        def b16(*s):
            return torch.empty(*s, dtype=self.op_dtype, device=dev)
        B, N, Lq, La = self.B, self.N, self.Lq, self.La
        self.inp = dict(image=f32(B, 3, self.img, self.img), question_ids=torch.zeros(B, Lq, dtype=torch.int64, device=dev),
                        question_mask=torch.ones(B, Lq, dtype=torch.int64, device=dev),
                        answer_ids=torch.zeros(N, La, dtype=torch.int64, device=dev),
                        answer_mask=torch.ones(N, La, dtype=torch.int64, device=dev), weights=f32(N))
        self.zero_tt_q = torch.zeros(B, Lq, dtype=torch.int64, device=dev)
        self.zero_tt_a = torch.zeros(N, La, dtype=torch.int64, device=dev)
        self.qmask8 = torch.ones(B, Lq, dtype=torch.uint8, device=dev)
        self.amask8 = torch.ones(N, La, dtype=torch.uint8, device=dev)
        self.qmask8_rep = torch.ones(N, Lq, dtype=torch.uint8, device=dev)
        self.rep_idx = torch.zeros(N * Lq, dtype=torch.int32, device=dev)       # (answer, token) -> question-state row
        self.seg_off = torch.zeros(B + 1, dtype=torch.int32, device=dev)        # answers of question b: [off[b], off[b+1])
        self.sel_idx = torch.zeros(self.R, dtype=torch.int32, device=dev)       # LM rows: (answer, t < La-1) -> decoder row
        self.unsel_idx = torch.full((self.Ma,), -1, dtype=torch.int32, device=dev)
        self.labels = torch.zeros(self.R, dtype=torch.int64, device=dev)
        self.row_w = f32(self.R)
        self.row_kl = torch.ones(self.R, device=dev)      # per-row factor on the MKD term (0 on rows that only padding created)

        def vit_set():
            Mi = self.Mi

            def u_img():     # what fc2^T needs of the pre-GELU u: 8-bit gelu' codes where FEDDAT_EPI_GELU_G8 applies, else bf16 u
                return torch.empty(Mi, I, dtype=torch.uint8, device=dev) if Mi >= 1024 else b16(Mi, I)
            return dict(patches=b16(B * (self.Ni - 1), 3 * self.P * self.P), proj=f32(B * (self.Ni - 1), H),
                        h0=f32(Mi, H), st0=f32(Mi, 2), x16=b16(Mi, H), f16=b16(Mi, I),
                        blocks=[dict(h_in=f32(Mi, H) if i else None, st1=f32(Mi, 2), qkv=b16(Mi, 3 * H), ctx=b16(Mi, H),
                                     lse=f32(self.B, self.heads, self.Ni), h2=f32(Mi, H), st2=f32(Mi, 2), u=u_img(),
                                     h3=f32(Mi, H), zs=f32(Mi, 2, self.r)) for i in range(self.vd)],
                        out=f32(Mi, H), stf=f32(Mi, 2), emb16=b16(Mi, H))

        def bert_set(M, nb, Sq, layers, cross_from, kv_rows):
            nc = max(layers - cross_from, 0)
            kvc_all = b16(kv_rows, nc * 2 * H) if nc else None      # K | V of every cross-attention layer, one product

            def layer(i):
                d = dict(qkv=b16(M, 3 * H), ctx=b16(M, H), lse=f32(nb, self.heads, Sq), t1=f32(M, H), st_a=f32(M, 2),
                         a=f32(M, H), a16=b16(M, H), u=b16(M, I), s1=f32(M, H), st_x=f32(M, 2), x=f32(M, H),
                         zs=f32(M, 2, self.r), s2=f32(M, H), st_o=f32(M, 2), out=f32(M, H), out16=b16(M, H))
                if i >= cross_from:
                    j = i - cross_from
                    d.update(qc=b16(M, H), kvc=kvc_all[:, j * 2 * H:(j + 1) * 2 * H], ctx2=b16(M, H),
                             lse2=f32(nb, self.heads, Sq), t2=f32(M, H), st_c=f32(M, 2), c=f32(M, H), c16=b16(M, H))
                return d
            return dict(h=f32(M, H), h16=b16(M, H), f16=b16(M, I), tA=f32(M, H), td=f32(M, H), kvc_all=kvc_all,
                        layers=[layer(i) for i in range(layers)])

        def act_set():
            return dict(vit=vit_set(), enc=bert_set(self.Mq, B, Lq, self.el, self.fl, self.Mi),
                        dec=bert_set(self.Ma, N, La, self.dl, 0, N * Lq), enc_rep16=b16(N * Lq, H),
                        hsel=f32(self.R, H), hsel16=b16(self.R, H), tu=f32(self.R, H), tg=f32(self.R, H), tst=f32(self.R, 2),
                        ty16=b16(self.R, H), logits=f32(self.R, self.Vp), loss=f32(4 + 2 * self.R))
        self.acts = {"gating": act_set(), "adapter_1": act_set()}
        # Everything in the image encoder AHEAD of block 0's adapter (patch embedding, block 0's attention and MLP) is frozen
        # and sees the same image in both passes: train_step computes it once (_vit_fwd(..., part="prefix")), both activation
        # sets point at the same buffers (read-only in the backward: block 0's adapter input h3 for its weight gradient).
        vg, v1 = self.acts["gating"]["vit"], self.acts["adapter_1"]["vit"]
        for k in ("patches", "proj", "h0", "st0"):
            v1[k] = vg[k]
        for k in ("st1", "qkv", "ctx", "lse", "h2", "st2", "u", "h3"):
            v1["blocks"][0][k] = vg["blocks"][0][k]
        # image_embeds of the two passes back to back: one K / V source for the batched text encoder's cross-attention
        self.emb16_both = b16(2 * self.Mi, H)
        self.acts["gating"]["vit"]["emb16"] = self.emb16_both[:self.Mi]
        self.acts["adapter_1"]["vit"]["emb16"] = self.emb16_both[self.Mi:]
        if self.batch_text:
            R2 = 2 * self.R
            self.acts["both"] = dict(enc=bert_set(2 * self.Mq, 2 * B, Lq, self.el, self.fl, 2 * self.Mi),
                                     dec=bert_set(2 * self.Ma, 2 * N, La, self.dl, 0, 2 * N * Lq), enc_rep16=b16(2 * N * Lq, H),
                                     hsel=f32(R2, H), hsel16=b16(R2, H), tu=f32(R2, H), tg=f32(R2, H), tst=f32(R2, 2),
                                     ty16=b16(R2, H), logits=f32(R2, self.Vp))
        # backward scratch: one set per pass (their text-side backward passes run on two streams)
        Mmax = max(self.Mi, self.Mq, self.Ma, N * Lq, self.R)

        def scratch():
            return dict(dlogits=b16(self.R, self.Vp), d1=f32(Mmax, H), d2=f32(Mmax, H), d3=f32(Mmax, H), d4=f32(Mmax, H),
                      b1=b16(Mmax, H), b2=b16(Mmax, H), bI=b16(Mmax, I), b3=b16(Mmax, 3 * H),
                      bkv=b16(max(self.Mi, N * Lq), max(self.el - self.fl, self.dl) * 2 * H),
                      z=f32(Mmax, self.r), dz=f32(Mmax, self.r), dsum=f32(max(B, N), self.heads, max(self.Ni, Lq, La)),
                      d_img=f32(self.Mi, H), d_qs=f32(self.Mq, H), d_rep=f32(N * Lq, H), d_dec=f32(self.Ma, H))
        self.gs = {"gating": scratch(), "adapter_1": scratch()}
        if self.batch_text:
            M2 = 2 * max(self.Mq, self.Ma, N * Lq, self.R)
            self.gs["both"] = dict(dlogits=b16(2 * self.R, self.Vp), d1=f32(M2, H), d2=f32(M2, H), d3=f32(M2, H), d4=f32(M2, H),
                                   b1=b16(M2, H), b2=b16(M2, H), bI=b16(M2, I), b3=b16(M2, 3 * H),
                                   bkv=b16(2 * max(self.Mi, N * Lq), max(self.el - self.fl, self.dl) * 2 * H),
                                   z=f32(M2, self.r), dz=f32(M2, self.r),
                                   dsum=f32(2 * max(B, N), self.heads, max(self.Ni, Lq, La)), d_img=f32(2 * self.Mi, H),
                                   d_qs=f32(2 * self.Mq, H), d_rep=f32(2 * N * Lq, H), d_dec=f32(2 * self.Ma, H))
        # text-side inputs / index maps, per form: "single" = one pass (B questions, N answers), "both" = the two passes stacked
        self.tx = {"single": dict(nq=B, na=N, Mq=self.Mq, Ma=self.Ma, R=self.R, q_ids=self.inp["question_ids"], q_tt=self.zero_tt_q,
                                  a_ids=self.inp["answer_ids"], a_tt=self.zero_tt_a, qmask8=self.qmask8, amask8=self.amask8,
                                  qmask8_rep=self.qmask8_rep, rep_idx=self.rep_idx, seg_off=self.seg_off, sel_idx=self.sel_idx,
                                  unsel_idx=self.unsel_idx)}
        if self.batch_text:
            i64 = lambda *s_: torch.zeros(*s_, dtype=torch.int64, device=dev)      # noqa: E731
            u8 = lambda *s_: torch.ones(*s_, dtype=torch.uint8, device=dev)        # noqa: E731
            i32 = lambda *s_: torch.zeros(*s_, dtype=torch.int32, device=dev)      # noqa: E731
            self.tx["both"] = dict(nq=2 * B, na=2 * N, Mq=2 * self.Mq, Ma=2 * self.Ma, R=2 * self.R, q_ids=i64(2 * B, Lq),
                                   q_tt=i64(2 * B, Lq), a_ids=i64(2 * N, La), a_tt=i64(2 * N, La), qmask8=u8(2 * B, Lq),
                                   amask8=u8(2 * N, La), qmask8_rep=u8(2 * N, Lq), rep_idx=i32(2 * N * Lq), seg_off=i32(2 * B + 1),
                                   sel_idx=i32(2 * self.R), unsel_idx=i32(2 * self.Ma))

    # ------------------------------------------------------------------------------------------ adapters
    def _pack(self, a: int, m: int):
        c = self._pack16[a][m]
        H, r = self.H, self.r
        base = PRE + self.modules[m] + f"adapter_{a}_"
        return dict(wd=c[0].view(r, H), wdT=c[1].view(H, r), wu=c[2].view(H, r), wuT=c[3].view(r, H),
                    bd=self.ad[a].view(base + "down.bias"), bu=self.ad[a].view(base + "up.bias"),
                    wd32=self.ad[a].view(base + "down.weight"), wu32=self.ad[a].view(base + "up.weight"))

    @_bound
    def repack_adapter(self, a: int):
        p0 = self._pack(a, 0)
        L.adapter_pack_strided(p0["wd32"], p0["wu32"], self.ad_numel, p0["wd"], p0["wdT"], p0["wu"], p0["wuT"],
                               4 * self.r * self.H, len(self.modules))

    def _segs(self, m: int, mode: str, rows: int, bwd: bool):
        key = (m, mode, rows, bwd)
        if key not in self._segs_cache and mode == "both":       # rows [0, rows / 2) gated, [rows / 2, rows) adapter_1
            h = rows // 2
            ts = 0 if bwd else -1
            self._segs_cache[key] = L.make_segs([
                dict(row_begin=0, row_end=h, train_slot=ts, adapters=[dict(self._pack(0, m), scale=0.5), dict(self._pack(2, m), scale=0.5)]),
                dict(row_begin=h, row_end=rows, train_slot=ts, adapters=[dict(self._pack(1, m), scale=1.0)])])
        if key not in self._segs_cache:
            if mode == "gating":
                ads = [dict(self._pack(0, m), scale=0.5), dict(self._pack(2, m), scale=0.5)]
            else:
                ads = [dict(self._pack(int(mode.split("_")[1]), m), scale=1.0)]
            self._segs_cache[key] = L.make_segs([dict(row_begin=0, row_end=rows, train_slot=0 if bwd else -1, adapters=ads)])
        return self._segs_cache[key]

    def _wgrad(self, m: int, mode: str, x, dy, rows: int):
        if mode == "both":       # adapter_0 from the gated half (scale 0.5), adapter_1 from the other; both are optimised here
            n, h, g = self.ad_numel, rows // 2, self.gs["both"]
            segs = self._wgrad_desc(("wg2", m, x.data_ptr(), dy.data_ptr(), rows), lambda: [
                dict(x=x, dy=dy, z=g["z"], dz=g["dz"], grad=self.ad[0].g[m * n:(m + 1) * n], rows=h, scale=0.5),
                dict(x=x[h:], dy=dy[h:], z=g["z"][h:], dz=g["dz"][h:], grad=self.ad[1].g[m * n:(m + 1) * n], rows=h, scale=1.0)])
            ws = self.wpart_stride2
            L.adapter_wgrad_partial(segs, self.wpart["both"][m * ws:(m + 1) * ws])
            self._wg_done["both"].append(m)
            return
        a = 0 if mode == "gating" else int(mode.split("_")[1])
        if a not in self.opt_adapters:
            return
        n = self.ad_numel
        segs = self._wgrad_desc(("wg", m, a, x.data_ptr(), dy.data_ptr(), rows), lambda: [
            dict(x=x, dy=dy, z=self.gs[mode]["z"], dz=self.gs[mode]["dz"], grad=self.ad[a].g[m * n:(m + 1) * n], rows=rows,
                 scale=0.5 if mode == "gating" else 1.0)])
        ws = self.wpart_stride
        L.adapter_wgrad_partial(segs, self.wpart[mode][m * ws:(m + 1) * ws])
        self._wg_done[mode].append(m)

    def _wgrad_reduce(self, mode: str):
        """Fold the partial sums of every module this backward pass produced into the adapter's gradient buffer (one launch)."""
        done, self._wg_done[mode] = self._wg_done[mode], []
        if not done:
            return
        if mode == "both":
            ms = tuple(sorted(done))
            key = ("wg-reduce2", ms)
            if key not in self._segs_cache:
                n = self.ad_numel
                assert ms == tuple(range(ms[0], ms[0] + len(ms)))
                ptrs = [self.ad[a].g[m * n:(m + 1) * n].data_ptr() for m in ms for a in (0, 1)]
                assert all(p % 16 == 0 for p in ptrs)      # feddat_adapter_wgrad_reduce moves float4
                self._segs_cache[key] = torch.tensor(ptrs, dtype=torch.int64, device=self.dev)
            ws = self.wpart_stride2
            # segments (adapter_0, adapter_1) = flags (B, A)
            self._reduce_wgrads(self._segs_cache[key], len(ms), 2, self.wpart["both"][ms[0] * ws:], ws, self.ovf_flags)
            return
        a = 0 if mode == "gating" else int(mode.split("_")[1])
        ms = tuple(sorted(done))
        key = ("wg-reduce", mode, ms)
        if key not in self._segs_cache:
            n, ws = self.ad_numel, self.wpart_stride
            contiguous = ms == tuple(range(ms[0], ms[0] + len(ms)))
            ptrs = [self.ad[a].g[m * n:(m + 1) * n].data_ptr() for m in ms]
            assert all(p % 16 == 0 for p in ptrs)      # feddat_adapter_wgrad_reduce moves float4
            ptrs = torch.tensor(ptrs, dtype=torch.int64, device=self.dev)
            self._segs_cache[key] = (ptrs, contiguous)
        ptrs, contiguous = self._segs_cache[key]
        ws, flag = self.wpart_stride, self.ovf_flags[a:a + 1]
        if contiguous:       # the usual case (all 30 modules): slots m0 .. m0 + len - 1 are one strided batch
            self._reduce_wgrads(ptrs, len(ms), 1, self.wpart[mode][ms[0] * ws:], ws, flag)
        else:
            for j, m in enumerate(ms):
                self._reduce_wgrads(ptrs[j:j + 1], 1, 1, self.wpart[mode][m * ws:], ws, flag)

    def _scale_in(self, mode: str):
        """How the loss scale enters, on dL/dlogits of the pass `mode` (+ that pass's overflow flag for a non-finite loss); it
        leaves through LocalUpdateEngine._scale_out."""
        if not self._dyn():
            return dict(grad_scale=self.loss_scale)
        a = 0 if mode == "gating" else 1
        return dict(grad_scale=1.0, grad_scale_dev=self.scaler_f[0:1], nonfinite=self.ovf_flags[a:a + 1])

    _KINDS = {"emb": 0, "self_probs": 1, "self_out": 2, "cross_probs": 3, "cross_out": 4, "out": 5}

    def _drop(self, pass_id, tower: int, layer: int, kind: str):
        """(p, key0, key1, step counter) of one dropout site of pass `pass_id` (0 / 1 / 2 = P0 / P1 / P2), or None when the
        pass runs without dropout (pass_id None: eval / plain forwards, or dropout = 0).  Site numbering: (tower * 64 + layer) * 8 + kind
        (tower 0 = text encoder, 1 = decoder)."""
        if pass_id is None or self.dropout <= 0:
            return None
        key = (pass_id, tower, layer, kind)
        if key not in self._segs_cache:
            k0, k1 = L.dropout_keys(self.seed, pass_id, (tower * 64 + layer) * 8 + self._KINDS[kind])
            self._segs_cache[key] = (self.dropout, k0, k1, self.drop_ctr)
        return self._segs_cache[key]

    # ------------------------------------------------------------------------------------------ inputs
    @_bound
    def set_batch(self, batch: Dict):
        """Reference batch after tokenisation (albef.py:52-60): image [B,3,R,R] f32; question_ids / question_mask [B, lq];
        answer_ids / answer_mask [n, la]; weights [n]; k = answers per question (host list, sum = n).
        The reference pads to the LONGEST question / answer of the batch and has as many answers as the batch brings
        (vqa_dataset_crossvqa.py:377-422); the engine's buffers are one static frame [B, Lq], [N, La] (one captured graph).
        Any lq <= Lq, la <= La, n <= N is accepted and embedded in the frame so that the RESULT is the reference's on the
        unpadded batch: padded key positions are masked out of every attention; padded answer POSITIONS and padded ANSWERS get
        label -100, weight 0 and factor 0 on their MKD rows (row_kl), and the MKD's batchmean divides by n, not N -- the
        reference's KL runs over every row of logits[:, :-1] of ITS batch, i.e. [n, la - 1, V] (task_trainer.py:506-516)."""
        B, N, Lq, La = self.B, self.N, self.Lq, self.La
        img = batch["image"]
        if tuple(img.shape) != tuple(self.inp["image"].shape):
            raise L.FeddatHipError(f"engine built for image {tuple(self.inp['image'].shape)}, got {tuple(img.shape)}")
        if img.data_ptr() != self.inp["image"].data_ptr():      # (the image transform writes into this very buffer)
            self.inp["image"].copy_(img, non_blocking=True)
        qi, qm, ai, am, wt = (batch[k] for k in ("question_ids", "question_mask", "answer_ids", "answer_mask", "weights"))
        lq, n, la = qi.shape[1], ai.shape[0], ai.shape[1]
        if qi.shape[0] != B or tuple(qm.shape) != tuple(qi.shape) or tuple(am.shape) != tuple(ai.shape) or wt.shape[0] != n:
            raise L.FeddatHipError("question / answer tensors of one batch disagree in shape")
        if lq > Lq or la > La or n > N or n < 1 or la < 2:
            raise L.FeddatHipError(f"batch ({lq} question tokens, {n} answers of {la} tokens) exceeds the engine's frame "
                                   f"({Lq}, {N}, {La})")
        for k, t in (("question_ids", qi), ("answer_ids", ai)):      # an out-of-range id would fault in the embedding gather;
            if not t.is_cuda and int(t.max()) >= self.V:             # host batches are checked (device ones: no sync)
                raise L.FeddatHipError("token id outside the vocabulary")
        full = (lq, n, la) == (Lq, N, La)
        if full:
            for k, src in (("question_ids", qi), ("question_mask", qm), ("answer_ids", ai), ("answer_mask", am), ("weights", wt)):
                self.inp[k].copy_(src, non_blocking=True)
        else:
            self.inp["question_ids"].fill_(self.pad_id)
            self.inp["question_mask"].zero_()
            self.inp["question_ids"][:, :lq].copy_(qi, non_blocking=True)
            self.inp["question_mask"][:, :lq].copy_(qm, non_blocking=True)
            self.inp["answer_ids"].fill_(self.pad_id)
            self.inp["answer_mask"].zero_()
            self.inp["answer_ids"][:n, :la].copy_(ai, non_blocking=True)
            self.inp["answer_mask"][:n, :la].copy_(am, non_blocking=True)
            if n < N:       # padded answers: one live [CLS] key so that no attention row is empty; they carry no loss
                self.inp["answer_ids"][n:, 0] = self.inp["answer_ids"][0, 0]
                self.inp["answer_mask"][n:, 0] = 1
            self.inp["weights"].zero_()
            self.inp["weights"][:n].copy_(wt, non_blocking=True)
        ks = [int(x) for x in batch["k"]]
        if len(ks) != B or sum(ks) != n:
            raise L.FeddatHipError("k must list the answers per question and sum to the number of answers")
        ks[-1] += N - n                              # padded answers ride with the last question (zero gradient rows)
        shape_key = (tuple(ks), n, la)
        if getattr(self, "_k", None) != shape_key:   # index maps depend on the batch's shape only (host-built once per pattern)
            self._k = shape_key
            qof = torch.repeat_interleave(torch.arange(B), torch.tensor(ks))
            self.qof = qof.to(self.dev)
            self.rep_idx.copy_((qof[:, None] * Lq + torch.arange(Lq)[None]).reshape(-1).int())
            self.seg_off.copy_(torch.tensor([0] + list(torch.tensor(ks).cumsum(0)), dtype=torch.int32))
            sel = (torch.arange(N)[:, None] * La + torch.arange(La - 1)[None]).reshape(-1)
            self.sel_idx.copy_(sel.int())
            un = torch.full((self.Ma,), -1, dtype=torch.int32)
            un[sel] = torch.arange(self.R, dtype=torch.int32)
            self.unsel_idx.copy_(un)
            rk = torch.zeros(N, La - 1)
            rk[:n, :la - 1] = float(N) / float(n)
            self.row_kl.copy_(rk.reshape(-1))
            if self.batch_text:       # the same maps for the stacked passes: the second pass's rows sit behind the first's
                tb = self.tx["both"]
                rep, off = self.rep_idx.cpu(), self.seg_off.cpu()
                tb["rep_idx"].copy_(torch.cat([rep, rep + self.Mq]))
                tb["seg_off"].copy_(torch.cat([off[:B], off + N]))
                tb["sel_idx"].copy_(torch.cat([sel, sel + self.Ma]).int())
                tb["unsel_idx"].copy_(torch.cat([un, torch.where(un >= 0, un + self.R, un)]))
        # masks, labels and per-row weights of this batch (tiny integer work on the device tensors)
        self.qmask8.copy_(self.inp["question_mask"])
        self.amask8.copy_(self.inp["answer_mask"])
        self.qmask8_rep.copy_(self.qmask8[self.qof])
        if self.batch_text:
            tb = self.tx["both"]
            for dst, src in ((tb["q_ids"], self.inp["question_ids"]), (tb["a_ids"], self.inp["answer_ids"]), (tb["qmask8"], self.qmask8),
                             (tb["amask8"], self.amask8), (tb["qmask8_rep"], self.qmask8_rep)):
                dst.view(2, *src.shape).copy_(src.unsqueeze(0).expand(2, *src.shape))
        ids = self.inp["answer_ids"]
        lab = ids[:, 1:].masked_fill(ids[:, 1:] == self.pad_id, -100)
        if not full:
            lab[n:] = -100
            lab[:, la - 1:] = -100
        self.labels.copy_(lab.reshape(-1))
        self.row_w.copy_((self.inp["weights"] / self.B)[:, None].expand(self.N, self.La - 1).reshape(-1))

    # ------------------------------------------------------------------------------------------ forward
    def _vit_fwd(self, S, mode: str, part: str = "all"):
        """part: "prefix" = patch embedding + block 0 up to (not including) its adapter -- the same for every adapter mode;
        "suffix" = from block 0's adapter on; "all" = both."""
        B, H, Ni, vt = self.B, self.H, self.Ni, self.vit
        V = S["vit"]
        if part != "suffix":
            L.im2col_patches(self.inp["image"], V["patches"], B, 3, self.img, self.img, self.P)
            L.gemm_bf16_nt(V["patches"], vt["wp"], L.EPI_F32, bias=vt["bp"], out_f32=V["proj"])
            # x = cat(cls, patches) + pos_embed  (vit.py:179-184): row 0 = cls + pos[0], rows 1.. = proj + pos[1..]
            L.image_embed_assemble(V["proj"], vt["cls"], vt["pos"][0], vt["pos"][1:], self.zero_h, V["h0"], B, 0, Ni - 1, Ni, H)
            b0 = vt["blocks"][0]
            L.layernorm_fwd(V["h0"], b0["n1g"], b0["n1b"], 1e-6, self.Mi, H, y_bf16=V["x16"], stats=V["blocks"][0]["st1"])
        h = V["h0"]
        for i, W in enumerate(vt["blocks"]):
            A = V["blocks"][i]
            if i > 0 or part != "suffix":
                L.gemm_bf16_nt(V["x16"], W["qkv"]["w"], L.EPI_BF16, bias=W["qkv"]["b"], out_bf16=A["qkv"])
                q, k, v = A["qkv"][:, :H], A["qkv"][:, H:2 * H], A["qkv"][:, 2 * H:]
                L.attn2_fwd(q, k, v, A["ctx"], A["lse"], B, Ni, Ni, self.heads)
                L.gemm_bf16_nt(A["ctx"], W["proj"]["w"], L.EPI_RESID_F32, bias=W["proj"]["b"], resid=h, out_f32=A["h2"])
                L.layernorm_fwd(A["h2"], W["n2g"], W["n2b"], 1e-6, self.Mi, H, y_bf16=V["x16"], stats=A["st2"])
                L.gemm_bf16_nt(V["x16"], W["fc1"]["w"], L.EPI_GELU_G8 if A["u"].dtype == torch.uint8 else L.EPI_GELU,
                               bias=W["fc1"]["b"], out_bf16=V["f16"], out2_bf16=A["u"])
                L.gemm_bf16_nt(V["f16"], W["fc2"]["w"], L.EPI_RESID_F32, bias=W["fc2"]["b"], resid=A["h2"], out_f32=A["h3"])
            if part == "prefix":
                return
            last = i == self.vd - 1
            nxt = V["out"] if last else V["blocks"][i + 1]["h_in"]
            g_, b_ = (vt["ng"], vt["nb"]) if last else (vt["blocks"][i + 1]["n1g"], vt["blocks"][i + 1]["n1b"])
            # adapter (vit.py:107) fused with the NEXT LayerNorm: the next block's norm1, or the encoder's final norm whose
            # bf16 output is image_embeds, the K / V source of the text encoder's cross-attention
            L.adapter_fwd_ln(A["h3"], nxt, self._segs(i, mode, self.Mi, False), self.Mi, g_, b_, 1e-6,
                             V["emb16"] if last else V["x16"], V["stf"] if last else V["blocks"][i + 1]["st1"],
                             z_save=A["zs"])
            h = nxt

    def _embed(self, T, ids, tts, nb, Lt, out_f32, out_b16, drop=None):
        L.text_embed(ids, tts, T["word"], T["pos"], T["typ"], T["lng"], T["lnb"], 1e-12, self.zero_h, out_f32, nb, Lt, Lt,
                     self.H)
        if drop is not None:                 # embeddings = self.dropout(LayerNorm(...))   xbert.py:216
            L.dropout(out_f32, drop, out_f32=out_f32, out_bf16=out_b16)
        else:
            L.cvt_f32_bf16(out_f32, out_b16)

    def _dense_resid(self, x16, lin, resid, out, tmp, drop):
        """out = dropout(x W^T + b) + resid: one GEMM with the residual epilogue, or -- with dropout between the dense
        layer and the residual add (xbert.py:360,440) -- the plain product followed by the fused mask + add."""
        if drop is None:
            L.gemm_bf16_nt(x16, lin["w"], L.EPI_RESID_F32, bias=lin["b"], resid=resid, out_f32=out)
        else:
            L.gemm_bf16_nt(x16, lin["w"], L.EPI_F32, bias=lin["b"], out_f32=tmp)
            L.dropout(tmp, drop, resid=resid, out_f32=out)

    def _attn_out(self, W, ctx, resid, M, t_out, st, y, y16, tmp=None, drop=None):
        """BertSelfOutput: LN(dropout(dense(ctx)) + input) (xbert.py:356-362)."""
        self._dense_resid(ctx, W["o"], resid, t_out, tmp, drop)
        L.layernorm_fwd(t_out, W["lng"], W["lnb"], 1e-12, M, self.H, y_bf16=y16, y_f32=y, stats=st)

    def _bert_fwd(self, T, S, m0: int, mode: str, M, nb, Sq, self_mask, causal, enc16, enc_rows, Skv, enc_mask,
                  pass_id=None, tower: int = 0):
        H = self.H
        h, h16 = S["h"], S["h16"]
        if T["cross_layers"]:         # K | V of every cross-attention layer of the tower in one product (see tower())
            L.gemm_bf16_nt(enc16, T["kv_all"]["w"], L.EPI_BF16, bias=T["kv_all"]["b"], out_bf16=S["kvc_all"])
        for i, W in enumerate(T["layers"]):
            A = S["layers"][i]
            dk = lambda kind: self._drop(pass_id, tower, i, kind)      # noqa: E731
            L.gemm_bf16_nt(h16, W["att"]["qkv"]["w"], L.EPI_BF16, bias=W["att"]["qkv"]["b"], out_bf16=A["qkv"])
            L.attn2_fwd(A["qkv"][:, :H], A["qkv"][:, H:2 * H], A["qkv"][:, 2 * H:], A["ctx"], A["lse"], nb, Sq, Sq,
                        self.heads, key_mask=self_mask, causal=causal, drop=dk("self_probs"))
            self._attn_out(W["att"], A["ctx"], h, M, A["t1"], A["st_a"], A["a"], A["a16"], S["td"], dk("self_out"))
            c, c16 = A["a"], A["a16"]
            if W["cross"] is not None:
                Wc = W["cross"]
                L.gemm_bf16_nt(A["a16"], Wc["q"]["w"], L.EPI_BF16, bias=Wc["q"]["b"], out_bf16=A["qc"])
                L.attn2_fwd(A["qc"], A["kvc"][:, :H], A["kvc"][:, H:], A["ctx2"], A["lse2"], nb, Sq, Skv, self.heads,
                            key_mask=enc_mask, q_rows=Sq, kv_rows=enc_rows, drop=dk("cross_probs"))
                self._attn_out(Wc, A["ctx2"], A["a"], M, A["t2"], A["st_c"], A["c"], A["c16"], S["td"], dk("cross_out"))
                c, c16 = A["c"], A["c16"]
            L.gemm_bf16_nt(c16, W["fc1"]["w"], L.EPI_GELU, bias=W["fc1"]["b"], out_bf16=S["f16"], out2_bf16=A["u"])
            # BertOutput with the adapter (xbert.py:438-445 -> adapter.py:97-116): s1 = dropout(dense) + inp; x = LN(s1);
            # y + inp = s1 + (x + A(x)) - x; out = LN(y + inp), same LayerNorm twice
            self._dense_resid(S["f16"], W["fc2"], c, A["s1"], S["td"], dk("out"))
            L.layernorm_fwd(A["s1"], W["lng"], W["lnb"], 1e-12, M, H, y_f32=A["x"], stats=A["st_x"])
            L.adapter_fwd(A["x"], S["tA"], self._segs(m0 + i, mode, M, False), M, z_save=A["zs"])
            L.axpby3(A["s1"], 1.0, S["tA"], 1.0, A["x"], -1.0, out_f32=A["s2"])
            L.layernorm_fwd(A["s2"], W["lng"], W["lnb"], 1e-12, M, H, y_f32=A["out"], y_bf16=A["out16"], stats=A["st_o"])
            h, h16 = A["out"], A["out16"]
        return h, h16

    def _forward(self, mode: str, pass_id=None):
        """ALBEF.forward(train=True) up to logits[:, :-1] (albef_model.py:69-145), activations kept in self.acts[mode].
        pass_id (0 / 1 / 2): the train_step pass whose dropout masks apply; None = no dropout."""
        self._vit_fwd(self.acts[mode], mode)
        return self._forward_text(mode, pass_id)

    def _forward_text(self, mode: str, pass_id=None):
        """Everything behind the image encoder: text encoder with cross-attention, answer decoder, LM head.  mode "both":
        the gated and the adapter_1 pass stacked (rows of the gated pass first) over the stacked image_embeds."""
        t = self.tx["both" if mode == "both" else "single"]
        return self._text_answers(mode, self._text_questions(mode, t, pass_id), t, pass_id)

    def _text_questions(self, mode: str, t, pass_id=None):
        """The question half of _forward_text: the text encoder with cross-attention over image_embeds -> question states."""
        S = self.acts[mode]
        emb16 = self.emb16_both if mode == "both" else S["vit"]["emb16"]
        Lq, E = self.Lq, S["enc"]
        self._embed(self.enc, t["q_ids"], t["q_tt"], t["nq"], Lq, E["h"], E["h16"], self._drop(pass_id, 0, 0, "emb"))
        qs, _ = self._bert_fwd(self.enc, E, self.vd, mode, t["Mq"], t["nq"], Lq, t["qmask8"], False, emb16, self.Ni,
                               self.Ni, None, pass_id, 0)
        return qs

    def _text_answers(self, mode: str, qs, t, pass_id=None):
        """The answer half of _forward_text: question states repeated per answer (t["rep_idx"]), answer decoder, LM head.
        rank_answer's slabs call it once per slab on the same question states, with that slab's maps in `t`."""
        S = self.acts[mode]
        Lq, La, H = self.Lq, self.La, self.H
        D = S["dec"]
        # one question's states for each of its k answers (albef_model.py:93-98)
        L.gather_rows(qs, t["rep_idx"], dst_bf16=S["enc_rep16"])
        self._embed(self.dec, t["a_ids"], t["a_tt"], t["na"], La, D["h"], D["h16"], self._drop(pass_id, 1, 0, "emb"))
        out, _ = self._bert_fwd(self.dec, D, self.vd + self.el, mode, t["Ma"], t["na"], La, t["amask8"], True, S["enc_rep16"], Lq,
                                Lq, t["qmask8_rep"], pass_id, 1)
        # BertOnlyMLMHead on the positions that predict a next token (logits[:, :-1])
        L.gather_rows(out, t["sel_idx"], dst_f32=S["hsel"], dst_bf16=S["hsel16"])
        self._lm_head_fwd(S, 0, t["R"])
        return S["logits"]

    def _lm_head_fwd(self, S, lo: int, hi: int):
        """BertOnlyMLMHead (transform.dense, gelu, transform.LayerNorm, tied decoder + bias) on rows [lo, hi) of the selected
        decoder states S["hsel16"], with the head as it stands.  A train_step with a trainable head calls it a second time on the
        gated rows, after sub-step A's head update: the towers below did not change."""
        hd, H = self.head, self.H
        if self.train_lm_head:
            # transform.dense in fp32 from the group's master weight (fp32 MFMA, rows x 768 x 768: small): tu, gelu(tu) and the
            # LayerNorm statistics feed the head's own gradients
            key = ("head-dense", S["hsel"].data_ptr(), lo, hi)
            if key not in self._segs_cache:
                w32 = self.lm.view(self.lm.names[0])          # out[i, j] = sum_k x[i, k] W[j, k] + b[j]
                self._segs_cache[key] = L.ht_job(S["hsel"][lo:hi], H, 1, w32, 1, H, hi - lo, H, H, S["tu"][lo:hi], bias_j=hd["t"]["b"])
            L.head_gemm(self._segs_cache[key])
        else:
            L.gemm_bf16_nt(S["hsel16"][lo:hi], hd["t"]["w"], L.EPI_F32, bias=hd["t"]["b"], out_f32=S["tu"][lo:hi])
        L.gelu_fwd(S["tu"][lo:hi], S["tg"][lo:hi])
        L.layernorm_fwd(S["tg"][lo:hi], hd["lng"], hd["lnb"], 1e-12, hi - lo, H, y_bf16=S["ty16"][lo:hi], stats=S["tst"][lo:hi])
        L.gemm_bf16_nt(S["ty16"][lo:hi], hd["w"], L.EPI_F32, bias=hd["b"], out_f32=S["logits"][lo:hi])

    # ------------------------------------------------------------------------------------------ trainable LM head
    @_bound
    def _refresh_head(self):
        """The head's kernel operands from its fp32 group (one launch): 16-bit W and W^T of transform.dense, the padded bias."""
        g, hd = self.lm, self.head
        L.lm_head_refresh(g.view(g.names[0]), g.view(g.names[4]), hd["t"]["w"], hd["t"]["wT"], hd["b"])

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

    def _backward_text(self, mode: str, teacher_logits, pass_id=None):
        """Loss, LM head, decoder and text encoder backward of the pass `mode`; leaves d(image_embeds) in its scratch set.
        mode "both": the two passes stacked, each half's MKD teacher the OTHER half's logits (teacher_logits unused)."""
        S, g = self.acts[mode], self.gs[mode]
        t = self.tx["both" if mode == "both" else "single"]
        R, R1 = t["R"], self.R
        if mode == "both":       # L_0 = (loss_0 + KL(logits_0 || logits_1)) / 2 on rows [0, R), L_1 likewise on rows [R, 2R)
            lg = S["logits"]
            for half, own in ((0, "gating"), (1, "adapter_1")):
                L.lm_loss_fwd_bwd(lg[half * R1:(half + 1) * R1], lg[(1 - half) * R1:(2 - half) * R1], self.labels, self.row_w, self.V,
                                  3.0, 9.0 / self.N, g["dlogits"][half * R1:(half + 1) * R1], self.acts[own]["loss"],
                                  row_kl=self.row_kl, **self._scale_in(own))
        else:
            L.lm_loss_fwd_bwd(S["logits"], teacher_logits, self.labels, self.row_w, self.V, 3.0, 9.0 / self.N, g["dlogits"],
                              S["loss"], row_kl=self.row_kl, **self._scale_in(mode))
        self._lm_head_bwd(S, g, 0, R)
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
        cur = torch.cuda.current_stream()
        if self.side is None:
            self.side = torch.cuda.Stream(device=self.dev)
        side = self.side
        drop = self.dropout > 0
        dyn = self._dyn()
        fB, fA = (self.ovf_flags[0:1], self.ovf_flags[1:2]) if dyn else (None, None)
        R = self.R
        Sg, S1, gg, g1 = self.acts["gating"], self.acts["adapter_1"], self.gs["gating"], self.gs["adapter_1"]

        def loss(logits, teacher, dl, own):
            L.lm_loss_fwd_bwd(logits, teacher, self.labels, self.row_w, self.V, 3.0, 9.0 / self.N, dl, self.acts[own]["loss"],
                              row_kl=self.row_kl, **self._scale_in(own))
        self._vit_fwd(Sg, "gating", "prefix")
        side.wait_stream(cur)
        if self.batch_text and self.opt_adapters == (0, 1):
            # the stacked form: rows [0, R) gated, [R, 2R) adapter_1 of one text-side pass
            with torch.cuda.stream(side):
                self._vit_fwd(Sg, "gating", "suffix")
            self._vit_fwd(S1, "adapter_1", "suffix")
            cur.wait_stream(side)
            lg = self._forward_text("both")
            S, g = self.acts["both"], self.gs["both"]
            loss(lg[R:], lg[:R], g["dlogits"][R:], "adapter_1")
            self._lm_head_bwd(S, g, R, 2 * R, True, fA)
            self._head_step_a()
            self._lm_head_fwd(S, 0, R)
            loss(lg[:R], lg[R:], g["dlogits"][:R], "gating")
            self._lm_head_bwd(S, g, 0, R, True, fB)
            self._towers_bwd("both")
            d_img = g["d_img"]
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                self._vit_bwd(Sg, "gating", d_img[:self.Mi])
                self._wgrad_reduce("gating")
            self._vit_bwd(S1, "adapter_1", d_img[self.Mi:])
            self._wgrad_reduce("adapter_1")
            self._wgrad_reduce("both")
            cur.wait_stream(side)
        else:
            with torch.cuda.stream(side):
                self._vit_fwd(Sg, "gating", "suffix")
                if drop:       # P0 under its own masks; the gated text towers run again for P2 below
                    self.logits_all.copy_(self._forward_text("gating", 0))
                    teacher = self.logits_all
                else:
                    teacher = self._forward_text("gating")
            self._vit_fwd(S1, "adapter_1", "suffix")
            logits_1 = self._forward_text("adapter_1", 1 if drop else None)
            cur.wait_stream(side)
            loss(logits_1, teacher, g1["dlogits"], "adapter_1")
            self._lm_head_bwd(S1, g1, 0, R, True, fA)
            self._head_step_a()
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                self._towers_bwd("adapter_1", 1 if drop else None)
                self._vit_bwd(S1, "adapter_1", g1["d_img"])
                self._wgrad_reduce("adapter_1")
            if drop:
                logits_0 = self._forward_text("gating", 2)
            else:
                self._lm_head_fwd(Sg, 0, R)
                logits_0 = Sg["logits"]
            loss(logits_0, logits_1, gg["dlogits"], "gating")
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
        # The two passes are independent up to the loss and from the loss down to their adapters, so they run side by
        # side on two streams (separate activation, scratch and weight-gradient workspaces per pass; inside a captured
        # step the fork / join become graph edges): the text towers' launches are small (25-token questions, 4-token
        # answers: 24-156 workgroups) and overlap each other, and the other pass's kernels fill the CUs that the last,
        # partial round of an image-encoder GEMM leaves idle (388 tiles on 256 CUs at N = 768).
        cur = torch.cuda.current_stream()
        if self.side is None:
            self.side = torch.cuda.Stream(device=self.dev)
        side = self.side
        drop = self.dropout > 0
        if self.batch_text and self.opt_adapters == (0, 1):
            # dropout = 0: the image encoders of the two passes side by side, then ONE text-side forward / backward over both
            # passes' rows, then the two image-encoder backward passes side by side
            self._vit_fwd(self.acts["gating"], "gating", "prefix")
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                self._vit_fwd(self.acts["gating"], "gating", "suffix")
            self._vit_fwd(self.acts["adapter_1"], "adapter_1", "suffix")
            cur.wait_stream(side)
            self._forward_text("both")
            self._backward_text("both", None)
            d_img = self.gs["both"]["d_img"]
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                self._vit_bwd(self.acts["gating"], "gating", d_img[:self.Mi])
                self._wgrad_reduce("gating")
            self._vit_bwd(self.acts["adapter_1"], "adapter_1", d_img[self.Mi:])
            self._wgrad_reduce("adapter_1")
            self._wgrad_reduce("both")
            cur.wait_stream(side)
            self._optimizer_tail(False)
            return
        # the image encoder ahead of block 0's adapter: once for both passes (frozen, adapter-free, no dropout)
        self._vit_fwd(self.acts["gating"], "gating", "prefix")
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            self._vit_fwd(self.acts["gating"], "gating", "suffix")
            if drop:
                # P0 (task_trainer.py:283-287): no-grad gated forward under its own masks.  The image encoder has no dropout,
                # so its gated forward is shared with P2; the text towers run again for P2 below (other masks).
                self.logits_all.copy_(self._forward_text("gating", 0))
                logits_teacher = self.logits_all
            else:
                logits_teacher = self._forward_text("gating")     # P0 == P2 forward (task_trainer.py:283-287,311-315)
        self._vit_fwd(self.acts["adapter_1"], "adapter_1", "suffix")
        logits_1 = self._forward_text("adapter_1", 1 if drop else None)       # P1 (task_trainer.py:290-295)
        cur.wait_stream(side)
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
        self._optimizer_tail(drop)

    def _optimizer_tail(self, drop: bool):
        self._dat_tail()        # the DAT tail without a head
        if drop:
            L.step_tick(self.drop_ctr, 1, 0)                 # the next train_step draws fresh masks (also under graph replay)

    def _loss_tensor(self):
        """What train_step returns: the device buffer {loss_0, kl_0, L_0} of the P2 pass (the reference returns loss_0).  A
        step is ~3000 launches (the BERT towers' are tiny: without use_graph the step is host-bound)."""
        return self.acts["gating"]["loss"]

    # ------------------------------------------------------------------------------------------ inference
    @_bound
    @torch.no_grad()
    def forward_train_logits(self, batch: Dict, mode: str):
        """-> (loss, logits [N, La-1, V]) of ALBEF.forward(train=True) in adapter mode `mode` ('gating' | 'adapter_k')."""
        self.set_batch(batch)
        key = "gating" if mode == "gating" else "adapter_1"          # activation set whose buffers the pass uses
        S = self.acts[key]
        self.acts[mode] = S
        try:
            logits = self._forward(mode)
        finally:
            if mode != key:
                del self.acts[mode]
        L.lm_loss_fwd_bwd(logits, None, self.labels, self.row_w, self.V, 3.0, 0.0, None, S["loss"])
        _, n, la = self._k             # the batch's own answer count / length inside the engine's frame
        return S["loss"][0].clone(), logits[:, :self.V].reshape(self.N, self.La - 1, self.V)[:n, :la - 1].clone()

    @_bound
    @torch.no_grad()
    def rank_answer(self, batch: Dict, answer_ids: torch.Tensor, answer_mask: torch.Tensor, k: int, mode: str = "gating"):
        """ALBEF.forward(train=False) -> rank_answer (albef_model.py:147-156,171-228; eval loop task_trainer.py:159-204):
        first-token shortlist of k candidates per question out of the answer list, re-ranked by sequence likelihood.
        batch: image [nq, 3, R, R], question_ids / question_mask [nq, lq <= Lq] of 1 <= nq <= B questions; answer_ids / answer_mask
        [M, la <= La]: the tokenised answer list; 1 <= k <= M.  Any engine takes it (n_answers >= B); anything else is refused.
        Returns (topk_ids [nq, k] int64, topk_probs [nq, k]).  The decoder passes, the first-token softmax over the vocabulary
        (feddat_softmax_gather_rows) and both top-k selections (feddat_topk_rows) run on the HIP kernels.
        An engine built with n_answers = B * k takes a full batch (nq = B, la = La) as ONE frame -- two set_batch + forward
        passes, the form this method had before there were slabs, launch for launch.  Every other shape runs on the frame the engine
        has, in slabs of N candidates (_rank_answer_slabs): the engine a federation trains with scores itself."""
        B, N, La = self.B, self.N, self.La
        qi = batch["question_ids"]
        if answer_ids.dim() != 2 or tuple(answer_mask.shape) != tuple(answer_ids.shape) or qi.dim() != 2:
            raise L.FeddatHipError("rank_answer: question_ids [nq, lq] and answer_ids / answer_mask [M, la] expected")
        nq, (M, la) = qi.shape[0], answer_ids.shape
        if not (1 <= nq <= B and 2 <= la <= La and 1 <= k <= M and qi.shape[1] <= self.Lq):
            raise L.FeddatHipError(f"rank_answer: {nq} questions of {qi.shape[1]} tokens, k = {k} of {M} answers of {la} tokens do not "
                                   f"fit the engine's frame (B = {B}, Lq = {self.Lq}, La = {La}; 1 <= k <= answers)")
        if nq == B and la == La and N == B * k:
            return self._rank_answer_frame(batch, answer_ids, answer_mask, k, mode)
        return self._rank_answer_slabs(batch, answer_ids, answer_mask, k, mode)

    def _rank_maps(self, nq: int, k: int):
        """Index maps of rank_answer's slabs, built once per (nq, k) and kept on the device: entry 0 = pass 1 (one [BOS]-only answer
        per question, ks = [1] * B), entry 1 + s = slab s of rank_slab_plan.  rep: (answer, token) -> question-state row [N Lq];
        qof: answer -> question (the row of the question mask its cross-attention uses); sel: LM rows -> decoder rows.  (seg_off and
        unsel_idx, the other two maps of a train step, serve the backward pass only.)  They are tensors of their own: the maps
        set_batch keeps for the training batches, and its shape cache, stay as they are."""
        cache = self._rank_cache
        if (nq, k) not in cache:
            B, N, Lq, La = self.B, self.N, self.Lq, self.La
            plan = [[1] * B] + rank_slab_plan(nq, k, N, B)
            qof = torch.tensor([slab_question_of_row(ks, N) for ks in plan])
            rep = (qof[:, :, None] * Lq + torch.arange(Lq)[None, None]).reshape(len(plan), N * Lq).int()
            sel = (torch.arange(N)[:, None] * La + torch.arange(La - 1)[None]).reshape(-1).int()
            cache[(nq, k)] = dict(qof=qof.to(self.dev), rep=rep.to(self.dev), sel=sel.to(self.dev), slabs=len(plan) - 1)
        return cache[(nq, k)]

    def _rank_answer_slabs(self, batch: Dict, answer_ids: torch.Tensor, answer_mask: torch.Tensor, k: int, mode: str):
        """rank_answer at any shape the frame holds.  The nq questions are staged into samples [0, nq) of the static frame, samples
        [nq, B) become replicas (feddat_albef_pad_questions); the image encoder and the text encoder run ONCE.  Pass 1: the decoder
        on one [BOS]-only answer per question, first-token softmax over the list, top k -- the shortlist stays on the device.
        Pass 2: the nq * k candidates in slabs of N (rank_slab_plan); per slab feddat_rank_slab_gather writes the frame's answers,
        labels and row weights from the shortlist, the decoder and the LM head run as in a train step, and feddat_rank_slab_loss
        adds each candidate's CE terms into answer_loss.  No device-to-host read-back anywhere.
        The static buffers keep their addresses and the training maps are not written, so a train_step WITH A BATCH (eager or
        graph replay) afterwards is what it would have been without the evaluation; the staged training batch itself is gone
        (train_step(None) needs a set_batch first)."""
        B, N, Lq, La, V, dev = self.B, self.N, self.Lq, self.La, self.V, self.dev
        img, qi, qm = batch["image"], batch["question_ids"], batch["question_mask"]
        nq, lq = qi.shape
        (M, la) = answer_ids.shape
        if tuple(img.shape) != (nq,) + tuple(self.inp["image"].shape[1:]) or tuple(qm.shape) != (nq, lq):
            raise L.FeddatHipError(f"rank_answer: image {tuple(img.shape)} / question_mask {tuple(qm.shape)} do not match {nq} questions "
                                   f"of an engine built for images {tuple(self.inp['image'].shape[1:])}")
        if M > 8192:
            raise L.FeddatHipError("rank_answer: feddat_topk_rows sorts at most 8192 answers")
        for t_ in (qi, answer_ids):              # an out-of-range id would fault in the embedding gather (host tensors: no sync)
            if not t_.is_cuda and int(t_.max()) >= V:
                raise L.FeddatHipError("token id outside the vocabulary")
        answer_ids = answer_ids.to(dev, torch.int64).contiguous()
        answer_mask = answer_mask.to(dev, torch.int64).contiguous()
        inp = self.inp
        if img.data_ptr() != inp["image"].data_ptr():
            inp["image"][:nq].copy_(img, non_blocking=True)
        if lq < Lq:
            inp["question_ids"].fill_(self.pad_id)
            inp["question_mask"].zero_()
        inp["question_ids"][:nq, :lq].copy_(qi, non_blocking=True)
        inp["question_mask"][:nq, :lq].copy_(qm, non_blocking=True)
        L.albef_pad_questions(inp["image"], inp["question_ids"], inp["question_mask"], nq)
        self.qmask8.copy_(inp["question_mask"])
        maps = self._rank_maps(nq, k)
        qmask8_rep = self.qmask8[maps["qof"]]              # [1 + slabs, N, Lq]: each answer row's question mask

        def tx(i):
            return dict(self.tx["single"], rep_idx=maps["rep"][i], qmask8_rep=qmask8_rep[i], sel_idx=maps["sel"])
        key = "gating" if mode == "gating" else "adapter_1"
        S = self.acts[key]
        self.acts[mode] = S
        try:
            self._vit_fwd(S, mode)
            qs = self._text_questions(mode, self.tx["single"])
            # pass 1: [BOS] only (later positions are padding; the causal mask keeps position 0 blind to them)
            ai, am = inp["answer_ids"], inp["answer_mask"]
            ai.fill_(self.pad_id)
            ai[:, 0].copy_(answer_ids[0, 0])
            am.zero_()
            am[:, 0].fill_(1)
            self.amask8.copy_(am)
            lg = self._text_answers(mode, qs, tx(0))       # position 0 of question b's answer = row b (La - 1)
            prob_first = torch.empty(nq, M, device=dev)
            L.softmax_gather_rows(lg, nq, (La - 1) * lg.stride(0), V, answer_ids[:, 1], prob_first)
            topk_probs, topk_ids = L.topk_rows(prob_first, k)
            # pass 2: the shortlisted answers slab by slab, per-answer next-token loss
            answer_loss = torch.empty(nq * k, device=dev)
            for s in range(maps["slabs"]):
                L.rank_slab_gather(topk_ids, answer_ids, answer_mask, ai, am, self.amask8, self.labels, self.row_w, B, s, self.pad_id)
                lg = self._text_answers(mode, qs, tx(1 + s))
                L.lm_loss_fwd_bwd(lg, None, self.labels, self.row_w, V, 3.0, 0.0, None, S["loss"])
                L.rank_slab_loss(S["loss"], answer_loss, nq, k, B, N, La, s)
        finally:
            if mode != key:
                del self.acts[mode]
        # softmax(log(topk_probs) - answer_loss) over the k candidates, sorted (albef_model.py:223-226)
        probs, rerank = L.topk_rows(topk_probs, k, minus=answer_loss.view(nq, k), log_first=True, softmax=True)
        return torch.gather(topk_ids, 1, rerank), probs

    def _rank_answer_frame(self, batch: Dict, answer_ids: torch.Tensor, answer_mask: torch.Tensor, k: int, mode: str):
        """rank_answer of a full batch on an engine whose frame is B * k answers: both decoder passes in one frame each.  What
        is left to torch is index bookkeeping (index_select / gather of the shortlisted answers)."""
        B, N, La, V = self.B, self.N, self.La, self.V
        answer_ids, answer_mask = answer_ids.to(self.dev), answer_mask.to(self.dev)
        key = "gating" if mode == "gating" else "adapter_1"
        S = self.acts[key]
        self.acts[mode] = S
        try:
            # pass 1: [BOS] only (later positions are padding; the causal mask keeps position 0 blind to them)
            start = torch.full((N, La), self.pad_id, dtype=torch.int64, device=self.dev)
            start[:, 0] = answer_ids[0, 0]
            m0 = torch.zeros(N, La, dtype=torch.int64, device=self.dev)
            m0[:, 0] = 1
            self.set_batch(dict(batch, answer_ids=start, answer_mask=m0, weights=torch.ones(N, device=self.dev), k=[k] * B))
            lg = self._forward(mode)          # [N (La - 1), Vp] fp32; position 0 of one slot per question = row b k (La - 1)
            prob_first = torch.empty(B, answer_ids.shape[0], device=self.dev)
            L.softmax_gather_rows(lg, B, k * (La - 1) * lg.stride(0), V, answer_ids[:, 1], prob_first)
            topk_probs, topk_ids = L.topk_rows(prob_first, k)
            # pass 2: the shortlisted answers, per-answer next-token loss
            ids = answer_ids.index_select(0, topk_ids.reshape(-1))
            atts = answer_mask.index_select(0, topk_ids.reshape(-1))
            self.set_batch(dict(batch, answer_ids=ids, answer_mask=atts, weights=torch.full((N,), float(B), device=self.dev),
                                k=[k] * B))
            lg = self._forward(mode)
            L.lm_loss_fwd_bwd(lg, None, self.labels, self.row_w, V, 3.0, 0.0, None, S["loss"])
            answer_loss = S["loss"][4:4 + 2 * self.R:2].view(N, La - 1).sum(1)       # row_terms[2 r] = ce of row r (weight 1)
        finally:
            if mode != key:
                del self.acts[mode]
        # softmax(log(topk_probs) - answer_loss) over the k candidates, sorted (albef_model.py:223-226)
        probs, rerank = L.topk_rows(topk_probs, k, minus=answer_loss.view(B, k).contiguous(), log_first=True, softmax=True)
        return torch.gather(topk_ids, 1, rerank), probs

    @_bound
    def image_embeds(self, mode_key: str = "gating"):
        """fp32 image_embeds of the last forward in that activation set (final-norm output recomputed from its input)."""
        V = self.acts[mode_key]["vit"]
        out = torch.empty(self.Mi, self.H, device=self.dev)
        L.layernorm_fwd(V["out"], self.vit["ng"], self.vit["nb"], 1e-6, self.Mi, self.H, y_f32=out)
        return out.view(self.B, self.Ni, self.H)
