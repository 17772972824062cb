"""ALBEF (ViT-B/16 + BERT-base encoder + 6-layer decoder) with the three DAT adapters: the frozen model, its buffers and its
forward on MI355X -- what the training step (albef_engine.AlbefDatEngine) and the evaluation (albef_rank.AlbefRank) both run on.

Host-side sequencing of the HIP kernels in libfeddat_hip.so for ALBEF.forward(train=True) (src/modeling/models/albef_model.py:69-145)
with the adapters of vit.py:99-110 (after the MLP residual) and xbert.py:438-445 / adapter.py:97-116 (BertOutput, same LayerNorm
before and after the adapter).  As in the ViLT engine, no arithmetic happens in Python / PyTorch: torch owns device
buffers and the stream, every launch goes through the C ABI.  AlbefBackbone holds the frozen weights and their 16-bit operand
copies, the three adapter groups and their 16-bit packs, the LM head (frozen, or its trainable group and the operand copies
_refresh_head rebuilds from it), the activation sets, the staged batch with its index maps (set_batch), and the forward of the
three towers and of the LM head as it stands.  It keeps nothing a backward pass needs beyond the forward's activations.

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
tensors (_lm_head_fwd on rows [lo, hi); albef_engine._step_kernels_head).  Nothing trainable lies below the first ViT block's
adapter, so everything ahead of it runs once for both passes (_vit_fwd's "prefix").

Dropout.  The reference trains under model.train() (task_trainer.py:75) with hidden_dropout_prob =
attention_probs_dropout_prob = 0.1 (src/configs/model_configs.py:44-46) in the two BERT towers -- after the embedding
LayerNorm (xbert.py:216), on the attention probabilities (:333), on BertSelfOutput's dense output (:360) and on BertOutput's
dense output ahead of the adapter (:440); the ViT has none (vit.py:120).  `dropout=p` reproduces that with counter-based
masks (seed, train step, pass, site, element -> bit; include/feddat_hip.h; _drop) that the backward regenerates.  With p > 0
the P0 and P2 forwards draw DIFFERENT masks (three independent forwards in the reference), so the "gated forward once" identity
only holds for the image encoder: the text towers then run three times (P0 no-grad, P1, P2).  dropout=0 (the default) is
the deterministic configuration every parity fixture except g12 is captured in; feddat_amd.train.main passes the
reference's 0.1 (--albef_dropout).
"""
from __future__ import annotations

from typing import Dict, List

import torch

from . import lib as L
from .local_update import FlatGroup, LocalUpdateEngine, _bound

PRE = "albef_model.albef."
ADAPTER_TENSORS = ("down.weight", "down.bias", "up.weight", "up.bias")
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


class AlbefBackbone(LocalUpdateEngine):
    """The frozen ALBEF model with its adapters, buffers and forward.  A class on top sets the operand format
    (_init_loss_scale) and train_lm_head, then calls _init_backbone (the model) and _alloc (the buffers) inside
    `with lib.operands(...)`.

    ADAPTER_STEMS names the adapters every module carries, one flat group and one 16-bit pack each (slot a = stem a): the three of
    DAT here, ("adapter_",) in the single-adapter FedAvg engine (albef_adapter_engine.AlbefAdapterEngine).  What else depends on
    the adapter set follows from it: FROZEN_ADAPTERS (slots without optimizer state: DAT's teacher), ACT_SETS (the activation
    sets _alloc makes, named after the adapter modes whose forward they keep; a forward in any other mode borrows the last:
    albef_rank._as_mode) and the mode -> segment table (_mode_segments)."""
    ADAPTER_STEMS = ("adapter_0_", "adapter_1_", "adapter_2_")
    FROZEN_ADAPTERS = (2,)
    ACT_SETS = ("gating", "adapter_1")

    def _init_backbone(self, params, device, batch, n_answers, q_len, a_len, vit_depth, enc_layers, fusion_layer, dec_layers, image,
                       vocab, lr, weight_decay, adam_eps, pad_id, max_pos, dropout, seed, stack_text):
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
        H = self.H
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
        self.ad = [FlatGroup([(PRE + m + stem + t, shp[t]) for m in self.modules for t in ADAPTER_TENSORS], dev,
                             with_opt=(a not in self.FROZEN_ADAPTERS)) for a, stem in enumerate(self.ADAPTER_STEMS)]
        for grp in self.ad:
            for n in grp.names:
                grp.view(n).copy_(params[n].to(dev, torch.float32))
        self.ad_numel = self.r * H + self.r + H * self.r + H
        nm = len(self.modules)
        self._pack16 = [torch.empty(nm, 4, self.r * H, dtype=self.op_dtype, device=dev) for _ in self.ad]
        for a in range(len(self.ad)):
            self.repack_adapter(a)
        self._segs_cache: Dict = {}
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
        self.drop_ctr = torch.zeros(2, dtype=torch.int32, device=dev)      # [0] = train_steps since begin_local_update

    # ------------------------------------------------------------------------------------------ buffers
    def _b16(self, *s):
        return torch.empty(*s, dtype=self.op_dtype, device=self.dev)

    def _f32(self, *s):
        return torch.empty(*s, device=self.dev)

    def _alloc(self):
        dev, H, I = self.dev, self.H, self.I
        f32, b16 = self._f32, self._b16
        B, N, Lq, La = self.B, self.N, self.Lq, self.La

        def tx_set(k):
            """Text-side inputs and index maps of k passes stacked (k B questions, k N answers; k = 1: one pass)."""
            i64 = lambda *s_: torch.zeros(*s_, dtype=torch.int64, device=dev)      # noqa: E731
            u8 = lambda *s_: torch.ones(*s_, dtype=torch.uint8, device=dev)        # noqa: E731
            i32 = lambda *s_: torch.zeros(*s_, dtype=torch.int32, device=dev)      # noqa: E731
            return dict(nq=k * B, na=k * N, Mq=k * self.Mq, Ma=k * self.Ma, R=k * self.R, q_ids=i64(k * B, Lq), q_tt=i64(k * B, Lq),
                        a_ids=i64(k * N, La), a_tt=i64(k * N, La), qmask8=u8(k * B, Lq), amask8=u8(k * N, La),
                        qmask8_rep=u8(k * N, Lq),
                        rep_idx=i32(k * N * Lq),            # (answer, token) -> question-state row
                        seg_off=i32(k * B + 1),             # answers of question b: [off[b], off[b+1])
                        sel_idx=i32(k * self.R),            # LM rows: (answer, t < La-1) -> decoder row
                        unsel_idx=torch.full((k * self.Ma,), -1, dtype=torch.int32, device=dev))
        # text-side inputs / index maps, per form: "single" = one pass (B questions, N answers), "both" = the two passes stacked.
        # The staged batch (inp) and the maps set_batch writes ARE the single form's tensors.
        self.tx = {"single": tx_set(1)}
        t = self.tx["single"]
        self.inp = dict(image=f32(B, 3, self.img, self.img), question_ids=t["q_ids"],
                        question_mask=torch.ones(B, Lq, dtype=torch.int64, device=dev), answer_ids=t["a_ids"],
                        answer_mask=torch.ones(N, La, dtype=torch.int64, device=dev), weights=f32(N))
        self.zero_tt_q, self.zero_tt_a = t["q_tt"], t["a_tt"]
        self.qmask8, self.amask8, self.qmask8_rep = t["qmask8"], t["amask8"], t["qmask8_rep"]
        self.rep_idx, self.seg_off, self.sel_idx, self.unsel_idx = t["rep_idx"], t["seg_off"], t["sel_idx"], t["unsel_idx"]
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

        def text_set(k):
            """Text-side activations of k passes stacked: text encoder, decoder, LM head (k = 1: one pass)."""
            R = k * self.R
            return dict(enc=bert_set(k * self.Mq, k * B, Lq, self.el, self.fl, k * self.Mi),
                        dec=bert_set(k * self.Ma, k * N, La, self.dl, 0, k * N * Lq), enc_rep16=b16(k * N * Lq, H),
                        hsel=f32(R, H), hsel16=b16(R, H), tu=f32(R, H), tg=f32(R, H), tst=f32(R, 2), ty16=b16(R, H),
                        logits=f32(R, self.Vp))

        def act_set():
            return dict(vit=vit_set(), **text_set(1), loss=f32(4 + 2 * self.R))
        self.acts = {m: act_set() for m in self.ACT_SETS}
        if len(self.ACT_SETS) == 1:      # one pass per step: nothing to share between passes, nothing to stack
            return
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
            self.acts["both"] = text_set(2)
            self.tx["both"] = tx_set(2)

    # ------------------------------------------------------------------------------------------ adapters
    def _pack(self, a: int, m: int):
        c = self._pack16[a][m]
        H, r = self.H, self.r
        base = PRE + self.modules[m] + self.ADAPTER_STEMS[a]
        return dict(wd=c[0].view(r, H), wdT=c[1].view(H, r), wu=c[2].view(H, r), wuT=c[3].view(r, H),
                    bd=self.ad[a].view(base + "down.bias"), bu=self.ad[a].view(base + "up.bias"),
                    wd32=self.ad[a].view(base + "down.weight"), wu32=self.ad[a].view(base + "up.weight"))

    @_bound
    def repack_adapter(self, a: int):
        p0 = self._pack(a, 0)
        L.adapter_pack_strided(p0["wd32"], p0["wu32"], self.ad_numel, p0["wd"], p0["wdT"], p0["wu"], p0["wuT"],
                               4 * self.r * self.H, len(self.modules))

    @_bound
    def _refresh_head(self):
        """The trainable head's kernel operands from its fp32 group (one launch): 16-bit W and W^T of transform.dense, the
        padded bias -- to the LM head what repack_adapter is to an adapter."""
        g, hd = self.lm, self.head
        L.lm_head_refresh(g.view(g.names[0]), g.view(g.names[4]), hd["t"]["w"], hd["t"]["wT"], hd["b"])

    @classmethod
    def _mode_segments(cls, mode: str, rows: int):
        """The row segments of a pass over `rows` rows as [(row_begin, row_end, [(adapter, scale), ...])]; the FIRST adapter of
        a segment is the one that pass trains.  A single pass is one segment -- "gating": adapter_0 and the teacher adapter_2 at
        0.5 each, "adapter_k": adapter k alone; "both" is two: rows [0, rows / 2) gated, [rows / 2, rows) adapter_1.  With one
        adapter per module (ADAPTER_STEMS of one) the only mode is "adapter": that adapter alone at scale 1."""
        if len(cls.ADAPTER_STEMS) == 1:
            if mode != "adapter":
                raise L.FeddatHipError(f"a single-adapter model runs in mode 'adapter' only, got {mode!r}")
            return [(0, rows, [(0, 1.0)])]
        gated, h = [(0, 0.5), (2, 0.5)], rows // 2
        if mode == "both":
            return [(0, h, gated), (h, rows, [(1, 1.0)])]
        return [(0, rows, gated if mode == "gating" else [(int(mode.split("_")[1]), 1.0)])]

    def _segs(self, m: int, mode: str, rows: int, bwd: bool):
        key = (m, mode, rows, bwd)
        if key not in self._segs_cache:
            self._segs_cache[key] = L.make_segs([
                dict(row_begin=lo, row_end=hi, train_slot=0 if bwd else -1, adapters=[dict(self._pack(a, m), scale=s) for a, s in ads])
                for lo, hi, ads in self._mode_segments(mode, rows)])
        return self._segs_cache[key]

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
    def _check_ids(self, *ids):
        """An out-of-range token id would fault in the embedding gather: host tensors are checked (device ones: no sync)."""
        for t in ids:
            if not t.is_cuda and int(t.max()) >= self.V:
                raise L.FeddatHipError("token id outside the vocabulary")

    def _stage_questions(self, qi, qm, fill: bool):
        """Questions [nq <= B, lq <= Lq] into the top-left corner of the frame; fill: pad_id and mask 0 everywhere else first."""
        ids, mask = self.inp["question_ids"], self.inp["question_mask"]
        nq, lq = qi.shape
        if fill:
            ids.fill_(self.pad_id)
            mask.zero_()
        ids[:nq, :lq].copy_(qi, non_blocking=True)
        mask[:nq, :lq].copy_(qm, non_blocking=True)

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
        self._check_ids(qi, ai)
        full = (lq, n, la) == (Lq, N, La)
        self._stage_questions(qi, qm, fill=not full)
        if full:
            for k, src in (("answer_ids", ai), ("answer_mask", am), ("weights", wt)):
                self.inp[k].copy_(src, non_blocking=True)
        else:
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
        Lq, La = self.Lq, self.La
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

    @_bound
    def image_embeds(self, mode_key: str = "gating"):
        """fp32 image_embeds of the last forward in that activation set (final-norm output recomputed from its input)."""
        V = self.acts[mode_key]["vit"]
        out = torch.empty(self.Mi, self.H, device=self.dev)
        L.layernorm_fwd(V["out"], self.vit["ng"], self.vit["nb"], 1e-6, self.Mi, self.H, y_f32=out)
        return out.view(self.B, self.Ni, self.H)
