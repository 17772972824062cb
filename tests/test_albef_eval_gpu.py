"""ALBEF's evaluation on the engine a federation trains with (AlbefDatEngine.rank_answer at any shape the training frame holds:
nq <= B questions, any k <= M, answer lists of la <= La tokens, the candidates in slabs of N): the three kernels the slabs add
against torch on the CPU, the reference's own ranking (tests/golden/g10_albef_small.npz) and the CPU oracle through slabs, the
slab path against the one-frame path, a train_step after an evaluation, and feddat_amd.train.main with --synthetic_answer_list.

Tolerances are tests/test_albef_gpu.py's for this quantity: re-ranked probabilities within 2e-2 of the reference / the oracle.
A shortlist is compared as a SET, and only where the oracle's k-th and (k + 1)-th first-token probabilities are more than 2e-1
apart (relative): 16-bit operands move a first-token probability by a few per cent, so a closer pair could swap.  The answer
lists are chosen for that on the CPU (seeds 523 and 603 of the oracle's generator; test 501, the golden file's, has pairs 3 %
apart, which is why its own test compares ids only under a gap condition) and the gap is asserted on the oracle's values."""
import types

import numpy as np
import pytest
import torch

from oracle import albef_oracle as A
from tests.golden_util import load

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = dict(vit_depth=2, enc_layers=3, fusion_layer=1, dec_layers=2, image=64, vocab=3072, max_pos=64)
QKEYS = ("image", "question_ids", "question_mask")


def _dev(b):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in b.items()}


def _small_engine(eng_mod, P, B, N, q_len, a_len, **kw):
    return eng_mod.AlbefDatEngine(P, DEV, batch=B, n_answers=N, q_len=q_len, a_len=a_len, vit_depth=SMALL["vit_depth"],
                                  enc_layers=SMALL["enc_layers"], fusion_layer=SMALL["fusion_layer"],
                                  dec_layers=SMALL["dec_layers"], image=SMALL["image"], vocab=SMALL["vocab"], **kw)


class Ctx:
    """Parameters, the golden test's batch and answer list, the lists with a clear shortlist, and engines by frame size -- built
    once for the module."""

    def __init__(self, eng_mod):
        self.eng_mod = eng_mod
        self.d = A.AlbefDims(**SMALL)
        self.P = A.make_params(self.d)
        b0 = A.synthetic_batch(3, self.d, 500, q_len=12, a_len=5, k=[2, 1, 3], ragged=True)
        self.qb = {kk: b0[kk] for kk in QKEYS}
        self.lists = {}
        for seed, la in ((501, 5), (523, 5), (603, 4)):
            ev = A.synthetic_batch(3, self.d, seed, q_len=12, a_len=la, k=[4, 4, 3], ragged=True)
            self.lists[seed] = (ev["answer_ids"], ev["answer_mask"])
        self._engines, self._full, self._pv = {}, {}, None

    def engine(self, N):
        if N not in self._engines:
            self._engines[N] = _small_engine(self.eng_mod, self.P, 3, N, 12, 5)
        return self._engines[N]

    def questions(self, nq):
        return {kk: v[:nq] for kk, v in self.qb.items()}

    def full(self, seed, k=4, N=5):
        """rank_answer of all three questions through slabs of N (computed once per list, left unchanged)."""
        if (seed, k, N) not in self._full:
            ids, probs = self.engine(N).rank_answer(_dev(self.qb), *self.lists[seed], k)
            self._full[(seed, k, N)] = (ids.cpu(), probs.cpu())
        return self._full[(seed, k, N)]

    def first_token_probs(self):
        """The oracle's softmax over the vocabulary behind [BOS], per question (oracle rank_answer's first step)."""
        if self._pv is None:
            with torch.no_grad():
                img = A.vit_forward(self.P, self.d, self.qb["image"], "gating")
                qs = A.text_encoder(self.P, self.d, self.qb["question_ids"], self.qb["question_mask"], img, "gating")
                start = torch.full((3, 1), 101)
                lg = A.text_decoder(self.P, self.d, start, torch.ones_like(start), qs, self.qb["question_mask"], "gating")[:, 0]
            self._pv = torch.softmax(lg, 1)
        return self._pv


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import albef_engine
    return Ctx(albef_engine)


def _check_vs_oracle(ctx, ids, probs, nq, alist, amask, k, what):
    """Case 3's criteria: the oracle on these nq questions alone; sorted probabilities within 2e-2; the same shortlist as a set,
    with the oracle's own k-th / (k + 1)-th first-token probabilities more than 2e-1 apart (relative)."""
    qb = ctx.questions(nq)
    with torch.no_grad():
        rids, rprobs = A.albef_eval_forward(ctx.P, ctx.d, dict(qb, answer_list_ids=alist, answer_list_mask=amask), k, "gating")
    ids, probs = ids.cpu(), probs.cpu()
    assert ids.shape == probs.shape == (nq, k)
    if k < alist.shape[0]:
        s = ctx.first_token_probs()[:nq].index_select(1, alist[:, 1]).sort(1, descending=True).values
        gap = float(((s[:, k - 1] - s[:, k]) / s[:, k - 1]).min())
        assert gap > 2e-1, (what, gap)
    err = float((probs.sort(1, descending=True).values - rprobs.sort(1, descending=True).values).abs().max())
    print(f"{what}: sorted re-ranked probabilities within {err:.2e} of the oracle")
    assert err < 2e-2, (what, err)
    assert np.array_equal(np.sort(ids.numpy(), 1), np.sort(rids.numpy(), 1)), what
    assert bool((probs[:, :-1] >= probs[:, 1:]).all()) and float((probs.sum(1) - 1).abs().max()) < 1e-4


# ------------------------------------------------------------------------------------------------ 1. the kernels
def _ragged_list(M, la, g):
    ids = torch.randint(1000, 3000, (M, la), generator=g)
    ids[:, 0], ids[:, -1] = 101, 102
    mask = torch.ones(M, la, dtype=torch.long)
    ids[1::3, -2], ids[1::3, -1], mask[1::3, -1] = 102, 0, 0
    return ids, mask


def _gather_ref(topk, lids, lmask, N, La, s, pad):
    (nq, k), la = topk.shape, lids.shape[1]
    live = max(0, min(N, nq * k - s * N))
    ids, mask = torch.full((N, La), pad, dtype=torch.int64), torch.zeros(N, La, dtype=torch.int64)
    pick = topk.reshape(-1)[s * N:s * N + live]
    ids[:live, :la], mask[:live, :la] = lids[pick], lmask[pick]
    ids[live:, 0], mask[live:, 0] = lids[0, 0], 1
    lab = ids[:, 1:].clone()
    lab[lab == pad] = -100
    lab[:, la - 1:] = -100
    lab[live:] = -100
    w = torch.zeros(N, La - 1)
    w[:live] = 1.0
    return ids, mask, lab.reshape(-1), w.reshape(-1)


@pytest.mark.parametrize("nq", [1, 2, 3])
def test_slab_gather_equals_torch(ctx, nq):
    """M = 11 answers of la = 4 tokens (every third one shorter) in a frame of N = 5 answers of La = 5, k = 4: every slab, the
    partial last one included (nq = 3: 5 / 5 / 2; nq = 2: 5 / 3; nq = 1: 4); all five outputs, exactly."""
    from feddat_amd import lib as L
    g = torch.Generator().manual_seed(40 + nq)
    M, la, k, N, La, B = 11, 4, 4, 5, 5, 3
    lids, lmask = _ragged_list(M, la, g)
    topk = torch.stack([torch.randperm(M, generator=g)[:k] for _ in range(nq)])
    for s in range((nq * k + N - 1) // N):
        out = dict(ids=torch.full((N, La), -7, dtype=torch.int64, device=DEV), mask=torch.full((N, La), -7, dtype=torch.int64, device=DEV),
                   m8=torch.full((N, La), 9, dtype=torch.uint8, device=DEV), lab=torch.full((N * (La - 1),), -7, dtype=torch.int64, device=DEV),
                   w=torch.full((N * (La - 1),), -7.0, device=DEV))
        L.rank_slab_gather(topk.to(DEV), lids.to(DEV), lmask.to(DEV), out["ids"], out["mask"], out["m8"], out["lab"], out["w"], B, s, 0)
        ids, mask, lab, w = _gather_ref(topk, lids, lmask, N, La, s, 0)
        assert torch.equal(out["ids"].cpu(), ids) and torch.equal(out["mask"].cpu(), mask), (nq, s)
        assert torch.equal(out["m8"].cpu(), mask.to(torch.uint8)) and torch.equal(out["lab"].cpu(), lab), (nq, s)
        assert torch.equal(out["w"].cpu(), w), (nq, s)
    with pytest.raises(L.FeddatHipError):          # one slab past the last
        L.rank_slab_gather(topk.to(DEV), lids.to(DEV), lmask.to(DEV), out["ids"], out["mask"], None, out["lab"], out["w"], B,
                           (nq * k + N - 1) // N, 0)


@pytest.mark.parametrize("nq,Lq", [(1, 12), (2, 12), (1, 13), (2, 13)])
def test_pad_questions_equals_torch(ctx, nq, Lq):
    """B = 3 samples of a 64 x 64 image: samples [nq, 3) become copies of j mod nq, samples below nq stay.  Lq = 13: question rows of
    104 bytes, every other one off the 16-byte grid (the 8-byte path)."""
    from feddat_amd import lib as L
    g = torch.Generator().manual_seed(50 + nq)
    img = torch.randn(3, 3, 64, 64, generator=g)
    qi, qm = torch.randint(0, 3000, (3, Lq), generator=g), torch.randint(0, 2, (3, Lq), generator=g)
    d_img, d_qi, d_qm = img.to(DEV), qi.to(DEV), qm.to(DEV)
    L.albef_pad_questions(d_img, d_qi, d_qm, nq)
    src = [j if j < nq else j % nq for j in range(3)]
    assert torch.equal(d_img.cpu(), img[src]) and torch.equal(d_qi.cpu(), qi[src]) and torch.equal(d_qm.cpu(), qm[src])
    with pytest.raises(L.FeddatHipError):
        L.albef_pad_questions(d_img, d_qi, d_qm, 4)


@pytest.mark.parametrize("nq,k,B,N,La", [(3, 4, 3, 5, 5), (2, 4, 3, 5, 5), (3, 128, 3, 300, 5), (1, 7, 1, 1, 2)])
def test_slab_loss_against_float64(ctx, nq, k, B, N, La):
    """Every slab of (nq, k, N): each candidate's sum within (La - 1) * 2^-24 * sum |term| of the float64 sum (La - 1 fp32
    additions in a fixed order); entries of other slabs and the KL halves of `scalars` are not touched / not read.
    N = 300: more than one block."""
    from feddat_amd import lib as L
    g = torch.Generator().manual_seed(60 + N)
    out = torch.full((nq * k,), -7.0, device=DEV)
    for s in range((nq * k + N - 1) // N):
        sc = (torch.randn(4 + 2 * N * (La - 1), generator=g) * 3).abs()
        sc[5::2] = 1e30                                             # the KL terms: a read of them would show
        L.rank_slab_loss(sc.to(DEV), out, nq, k, B, N, La, s)
        live = min(N, nq * k - s * N)
        terms = sc[4::2].view(N, La - 1)[:live].double()
        got = out.cpu()
        bound = (La - 1) * 2.0 ** -24 * terms.abs().sum(1)
        assert bool(((got[s * N:s * N + live].double() - terms.sum(1)).abs() <= bound).all()), (s,)
        assert bool((got[s * N + live:] == -7.0).all())
    assert bool((out != -7.0).all())


# ------------------------------------------------------------------------------------------------ 2. the reference through slabs
def test_reference_golden_through_slabs(ctx, golden_dir):
    """test_rank_answer_eval_vs_reference_golden's inputs and assertions on an engine with a frame of N = 5 answers: 12
    candidates in slabs of 5 / 5 / 2 that straddle the questions."""
    g = load(golden_dir, "g10_albef_small.npz")
    k = 4
    ids, probs = ctx.full(501, k, 5)
    ref_ids, ref_probs = g["eval.topk_ids"], torch.from_numpy(g["eval.topk_probs"])
    # ranks are only comparable where the reference's probabilities are separated by more than the bf16 noise
    gaps = (ref_probs[:, :-1] - ref_probs[:, 1:]).min()
    assert (probs.cpu().sort(1, descending=True).values - ref_probs).abs().max() < 2e-2
    if float(gaps) > 4e-2:
        assert np.array_equal(ids.cpu().numpy(), ref_ids)
    else:
        assert np.array_equal(np.sort(ids.cpu().numpy(), 1), np.sort(ref_ids, 1))      # same shortlist


# ------------------------------------------------------------------------------------------------ 3. short batches
@pytest.mark.parametrize("nq", [2, 1])
def test_short_batch_against_the_oracle_and_the_full_batch(ctx, nq):
    """The first nq questions alone in the B = 3 frame (samples [nq, 3) are replicas): against the oracle on those nq questions,
    and against rows [0, nq) of the three-question run -- expected equal, every kernel on the path being row- or
    sample-independent."""
    k = 4
    alist, amask = ctx.lists[523]
    ids, probs = ctx.engine(5).rank_answer(_dev(ctx.questions(nq)), alist, amask, k)
    _check_vs_oracle(ctx, ids, probs, nq, alist, amask, k, f"nq = {nq} of B = 3, k = 4 of 11")
    for seed in (523, 501):
        fids, fprobs = ctx.full(seed, k, 5)
        ids, probs = ctx.engine(5).rank_answer(_dev(ctx.questions(nq)), *ctx.lists[seed], k)
        diff = float((probs.cpu() - fprobs[:nq]).abs().max())
        print(f"nq = {nq}, list {seed}: largest difference to rows [0, {nq}) of the full batch {diff:.3e}, ids equal: "
              f"{torch.equal(ids.cpu(), fids[:nq])}")
        assert diff <= 2e-2


# ------------------------------------------------------------------------------------------------ 4. edges
def test_shorter_list_in_a_longer_frame(ctx):
    """Answers of la = 4 tokens in the La = 5 frame, and questions of lq = 9 tokens in the Lq = 12 frame."""
    alist, amask = ctx.lists[603]
    assert alist.shape == (11, 4)
    ids, probs = ctx.engine(5).rank_answer(_dev(ctx.qb), alist, amask, 4)
    _check_vs_oracle(ctx, ids, probs, 3, alist, amask, 4, "la = 4 in La = 5")
    q9 = {"image": ctx.qb["image"][:2], "question_ids": ctx.qb["question_ids"][:2, :9].clone(),
          "question_mask": ctx.qb["question_mask"][:2, :9].clone()}
    q9["question_ids"][0, 8], q9["question_mask"][0, 8] = 102, 1          # question 0 cut to 9 tokens: [CLS] ... [SEP]
    ids9, probs9 = ctx.engine(5).rank_answer(_dev(q9), alist, amask, 4)
    with torch.no_grad():
        rids, rprobs = A.albef_eval_forward(ctx.P, ctx.d, dict(q9, answer_list_ids=alist, answer_list_mask=amask), 4, "gating")
    assert float((probs9.cpu().sort(1, descending=True).values - rprobs.sort(1, descending=True).values).abs().max()) < 2e-2
    # question 1 is its 9-token self in both runs
    assert float((probs9[1].cpu() - probs[1].cpu()).abs().max()) <= 2e-2


@pytest.mark.parametrize("k", [11, 1])
def test_k_equal_to_the_list_and_k_one(ctx, k):
    alist, amask = ctx.lists[523]
    ids, probs = ctx.engine(5).rank_answer(_dev(ctx.qb), alist, amask, k)
    _check_vs_oracle(ctx, ids, probs, 3, alist, amask, k, f"k = {k} of 11")
    if k == 11:
        assert np.array_equal(np.sort(ids.cpu().numpy(), 1), np.tile(np.arange(11), (3, 1)))


def test_k64_of_100_on_the_training_frame(ctx):
    """train.main's shape: N = B = 3, k = 64 of M = 100, 64 slabs of 3 candidates.  No seeded list of 100 random first tokens has
    its 64th and 65th probabilities 20 % apart for three questions at once (neighbours in a sorted sample of 100 from a
    distribution of log-spread 0.56 are ~1.5 % apart), so the list is BUILT with that gap from the oracle's first-token
    probabilities: 64 first tokens that every question puts above the vocabulary's median by more than 0.25 in log, 36 that every
    question puts below it by more than 0.25 (a seeded draw among those); the gap is then asserted like any other."""
    M, k, la = 100, 64, 5
    lp = ctx.first_token_probs()[:, 1000:3000].log()
    med = lp.median()
    g = torch.Generator().manual_seed(64)
    hi, lo = torch.nonzero(lp.min(0).values > med + 0.25).flatten(), torch.nonzero(lp.max(0).values < med - 0.25).flatten()
    assert hi.numel() >= k and lo.numel() >= M - k
    first = torch.cat([hi[torch.randperm(hi.numel(), generator=g)[:k]], lo[torch.randperm(lo.numel(), generator=g)[:M - k]]]) + 1000
    alist, amask = _ragged_list(M, la, g)
    alist[:, 1] = first[torch.randperm(M, generator=g)]
    ids, probs = ctx.engine(3).rank_answer(_dev(ctx.qb), alist, amask, k)
    assert ctx.engine(3)._rank_maps(3, k)["slabs"] == 64
    _check_vs_oracle(ctx, ids, probs, 3, alist, amask, k, "k = 64 of 100, N = B = 3")


def test_rank_answer_refuses_what_the_frame_cannot_hold(ctx):
    from feddat_amd import lib as L
    eng = ctx.engine(5)
    alist, amask = ctx.lists[523]
    four = {kk: torch.cat([v, v[:1]]) for kk, v in ctx.qb.items()}
    long6 = torch.cat([alist, alist[:, -1:]], 1)
    wide = {"image": ctx.qb["image"], "question_ids": torch.cat([ctx.qb["question_ids"]] * 2, 1),
            "question_mask": torch.cat([ctx.qb["question_mask"]] * 2, 1)}
    for batch, al, am, k in ((four, alist, amask, 4), (ctx.qb, long6, torch.ones_like(long6), 4), (ctx.qb, alist, amask, 12),
                             (ctx.qb, alist, amask, 0), (wide, alist, amask, 4), (ctx.qb, alist, amask[:, :4], 4)):
        with pytest.raises(L.FeddatHipError):
            eng.rank_answer(_dev(batch), al, am, k)


# ------------------------------------------------------------------------------------------------ 5. slabs against one frame
def test_slab_path_against_the_one_frame_path(ctx):
    """The same questions and list on an engine built with N = B * k = 12 (one frame per decoder pass) and on N = 5."""
    k = 4
    for seed in (501, 523):
        ids12, probs12 = ctx.engine(12).rank_answer(_dev(ctx.qb), *ctx.lists[seed], k)
        ids5, probs5 = ctx.full(seed, k, 5)
        diff = float((probs12.cpu().sort(1, descending=True).values - probs5.sort(1, descending=True).values).abs().max())
        print(f"list {seed}: slabs of 5 against one frame of 12: sorted probabilities differ by at most {diff:.3e}; ids equal: "
              f"{torch.equal(ids12.cpu(), ids5)}")
        assert diff < 2e-2


# ------------------------------------------------------------------------------------------------ 6. training undisturbed
def test_evaluation_does_not_disturb_training(ctx):
    """Two engines from the same parameters, two graph-replayed train_steps each; the second engine ranks answers (slab path,
    nq = 2) between its steps.  Every trainable tensor and both passes' losses: bit-identical."""
    bs = [A.synthetic_batch(3, ctx.d, 510 + s, q_len=12, a_len=5, k=[2, 1, 3], ragged=True) for s in range(2)]
    engs = [_small_engine(ctx.eng_mod, ctx.P, 3, 6, 12, 5) for _ in range(2)]
    losses = []
    for e, evaluate in zip(engs, (False, True)):
        e.begin_local_update(steps_per_epoch=2)
        out = []
        for s, b in enumerate(bs):
            if evaluate and s == 1:
                addr = {kk: v.data_ptr() for kk, v in e.inp.items()}
                ids, probs = e.rank_answer(_dev(ctx.questions(2)), *ctx.lists[523], 4)
                assert ids.shape == (2, 4) and e._rank_maps(2, 4)["slabs"] == 2
                assert addr == {kk: v.data_ptr() for kk, v in e.inp.items()}
            o = e.train_step(_dev(b), use_graph=True)
            torch.cuda.synchronize()
            out.append((o[:3].clone(), e.acts["adapter_1"]["loss"][:3].clone()))
        losses.append(out)
    for s in range(2):
        for j in range(2):
            assert torch.equal(losses[0][s][j], losses[1][s][j]), (s, j, losses[0][s][j], losses[1][s][j])
    sa, sb = engs[0].state_dict(), engs[1].state_dict()
    moved = 0.0
    for n in sa:
        assert torch.equal(sa[n], sb[n]), n
        moved = max(moved, float((sa[n].cpu() - ctx.P[n]).abs().max()))
    assert moved > 0


def test_model_ranks_answer_strings_for_a_short_batch(golden_dir):
    """ALBEFContinualLearner.forward(train=False) on the reference's eval batch (albef.py:61-73: questions and the answer list as
    strings, k): 2 questions in a 3-question frame, a list whose longest entry ([CLS] pieces [SEP] [SEP]) is shorter than the
    engine's a_len, on the engine built for training (n_answers = batch).  The appended [SEP] is in place, and the result is
    rank_answer's on the same encodings."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import albef_modeling
    g9 = load(golden_dir, "g9_wordpiece.npz")
    vocab = str(g9["vocab"]).split("\n")
    dims = dict(SMALL, vocab=max(SMALL["vocab"], len(vocab)))
    P = A.make_params(A.AlbefDims(**dims))
    model = albef_modeling.create_albef_continual_learner_model(P, DEV, 3, 3, q_len=25, a_len=8, tokenizer_vocab=vocab,
                                                                **{k: v for k, v in dims.items() if k != "max_pos"})
    answers = ["yes", "no", "two dogs", "red", "a man", "on the table", "blue sky"]
    batch = {"images": torch.randn(2, 3, dims["image"], dims["image"], generator=torch.Generator().manual_seed(3)),
             "questions": ["what color is the sky?", "how many dogs are there?"], "answer_list": answers, "k": 4, "train": False}
    enc = model.process_inputs(batch)
    ids, msk = enc["answer_list_ids"].cpu(), enc["answer_list_mask"].cpu()
    la = ids.shape[1]
    assert ids.shape[0] == len(answers) and 4 <= la < model.engine.La and enc["question_ids"].shape[0] == 2
    lens = msk.sum(1)
    sep = model.tokenizer.sep_id
    assert int(lens.max()) == la and bool((ids.gather(1, (lens - 1)[:, None]) == sep).all())
    assert bool((ids.gather(1, (lens - 2)[:, None]) == sep).all()) and bool((ids[msk == 0] == model.tokenizer.pad_id).all())
    model.activate_gating()
    out_ids, out_probs = model("art", batch)
    assert out_ids.shape == out_probs.shape == (2, 4) and float((out_probs.sum(1) - 1).abs().max()) < 1e-4
    assert bool((out_probs[:, :-1] >= out_probs[:, 1:]).all()) and int(out_ids.max()) < len(answers) and int(out_ids.min()) >= 0
    assert all(len(set(r)) == 4 for r in out_ids.tolist())
    ref_ids, ref_probs = model.engine.rank_answer(enc, enc["answer_list_ids"], enc["answer_list_mask"], 4, "gating")
    assert torch.equal(out_ids, ref_ids) and torch.equal(out_probs, ref_probs)


# ------------------------------------------------------------------------------------------------ 7. train.main
def test_train_main_scores_the_federation(tmp_path):
    """feddat_amd.train.main --encoder_name albef_no_distill --synthetic_answer_list 20, one round, two clients: the evaluation
    runs on the engine the clients trained with (N = B = 2, k = 20: ten slabs per batch; eval batches of one question in the
    two-question frame), stores [gating, adapter_0, adapter_1] scores per client, and they are what AlbefTaskTrainer.eval gives on
    the returned model with that client's personal tensors.  Without the option nothing is scored."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from feddat_amd import train
    common = ["--encoder_name", "albef_no_distill", "--ordered_cl_tasks", "art,gqa", "--image_size", "64", "--batch_size", "2",
              "--synthetic_steps", "2", "--comm_rounds", "1", "--albef_dims",
              "vit_depth=2,enc_layers=3,fusion_layer=1,dec_layers=2,vocab=3072,max_pos=64", "--output_dir", str(tmp_path / "albef")]
    model = train.main(common + ["--synthetic_answer_list", "20"])
    assert list(model.eval_scores) == [0] and sorted(model.eval_scores[0]) == ["art", "gqa"]
    assert model.adapter_requires_grad == {0: False, 1: True, 2: False}
    args = types.SimpleNamespace(local_epochs=1, num_epochs=15, lr=1e-4, optimizer_mode="dat", debug=0, hip_graph=True)
    for task, scores in model.eval_scores[0].items():
        assert len(scores) == 3 and all(0.0 <= s <= 100.0 for s in scores), (task, scores)
        loader = model.eval_data[task]
        assert [b["question_ids"].shape[0] for b in loader] == [1, 1, 1] and loader[0]["k"] == 20
        model.load_state_dict(model.personal_params[task])
        model.after_load()
        again = train.AlbefTaskTrainer(args, task, [], loader).eval(model)
        assert again == scores, (task, again, scores)
    plain = train.main(common)
    assert plain.eval_scores == {}
