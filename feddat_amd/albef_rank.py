"""ALBEF evaluation on the training engine's frame: forward_train_logits and the reference's rank_answer
(ALBEF.forward(train=False), src/modeling/models/albef_model.py:147-156,171-228; eval loop task_trainer.py:159-204).

AlbefRank is a mixin over albef_backbone.AlbefBackbone; list it first among the bases (albef_engine.AlbefDatEngine does).  It
runs the backbone's forward only -- nothing of the backward, the optimizer or the step -- and writes none of the training maps,
so the engine a federation trains with scores itself between local updates.  rank_slab_plan and slab_question_of_row are the
pure host arithmetic behind the slabs.
"""
from __future__ import annotations

import contextlib
from typing import Dict, List, Sequence

import torch

from . import lib as L
from .local_update import _bound


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


class AlbefRank:
    """Mixin over albef_backbone.AlbefBackbone; list it first among the bases."""

    def _init_rank(self):
        self._rank_cache: Dict = {}          # rank_answer's slab maps per (nq, k)

    @contextlib.contextmanager
    def _as_mode(self, mode: str):
        """A forward in adapter mode `mode` ('gating' | 'adapter_k'; 'adapter' on a single-adapter engine) runs in the buffers of
        an activation set the engine has (the backbone's ACT_SETS: the mode's own, else the last): that set, registered under
        `mode` for the length of the block."""
        key = mode if mode in self.ACT_SETS else self.ACT_SETS[-1]
        S = self.acts[key]
        self.acts[mode] = S
        try:
            yield S
        finally:
            if mode != key:
                del self.acts[mode]

    @_bound
    @torch.no_grad()
    def forward_train_logits(self, batch: Dict, mode: str):
        """-> (loss, logits [N, La-1, V]) of ALBEF.forward(train=True) in adapter mode `mode` ('gating' | 'adapter_k')."""
        self.set_batch(batch)
        with self._as_mode(mode) as S:
            logits = self._forward(mode)
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
        self._check_ids(qi, answer_ids)
        answer_ids = answer_ids.to(dev, torch.int64).contiguous()
        answer_mask = answer_mask.to(dev, torch.int64).contiguous()
        inp = self.inp
        if img.data_ptr() != inp["image"].data_ptr():
            inp["image"][:nq].copy_(img, non_blocking=True)
        self._stage_questions(qi, qm, fill=lq < Lq)
        L.albef_pad_questions(inp["image"], inp["question_ids"], inp["question_mask"], nq)
        self.qmask8.copy_(inp["question_mask"])
        maps = self._rank_maps(nq, k)
        qmask8_rep = self.qmask8[maps["qof"]]              # [1 + slabs, N, Lq]: each answer row's question mask

        def tx(i):
            return dict(self.tx["single"], rep_idx=maps["rep"][i], qmask8_rep=qmask8_rep[i], sel_idx=maps["sel"])
        with self._as_mode(mode) as S:
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
        # softmax(log(topk_probs) - answer_loss) over the k candidates, sorted (albef_model.py:223-226)
        probs, rerank = L.topk_rows(topk_probs, k, minus=answer_loss.view(nq, k), log_first=True, softmax=True)
        return torch.gather(topk_ids, 1, rerank), probs

    def _rank_answer_frame(self, batch: Dict, answer_ids: torch.Tensor, answer_mask: torch.Tensor, k: int, mode: str):
        """rank_answer of a full batch on an engine whose frame is B * k answers: both decoder passes in one frame each.  What
        is left to torch is index bookkeeping (index_select / gather of the shortlisted answers)."""
        B, N, La, V = self.B, self.N, self.La, self.V
        answer_ids, answer_mask = answer_ids.to(self.dev), answer_mask.to(self.dev)
        with self._as_mode(mode) as S:
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
        # softmax(log(topk_probs) - answer_loss) over the k candidates, sorted (albef_model.py:223-226)
        probs, rerank = L.topk_rows(topk_probs, k, minus=answer_loss.view(B, k).contiguous(), log_first=True, softmax=True)
        return torch.gather(topk_ids, 1, rerank), probs
