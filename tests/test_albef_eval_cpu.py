"""Host-side pieces of ALBEF's evaluation on the training engine (no GPU): the three entry points that rank_answer's slabs add
(include/feddat_hip.h: feddat_albef_pad_questions, feddat_rank_slab_gather, feddat_rank_slab_loss) are declared, exported, bound and
check their arguments; rank_slab_plan's arithmetic; train.main's new options and its synthetic answer list."""
import ctypes
import math
import os
import re

import pytest
import torch

from feddat_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("feddat_albef_pad_questions", "feddat_rank_slab_gather", "feddat_rank_slab_loss")
EINVAL = 1


@pytest.mark.parametrize("f16", [False, True])
def test_new_symbols_declared_exported_bound_and_checked(f16):
    """Every refusal below happens in the argument checks: the pointers are never dereferenced and no kernel is launched.  Each
    entry point is tried on the refusals its arguments can express: NULL pointers, nq = 0 and nq > B for all three; k > M and
    la > La for the gather (the only one that sees the list); a slab index past the last slab for the gather and the loss."""
    from feddat_amd import build
    src = open(os.path.join(ROOT, "include", "feddat_hip.h")).read()
    lib = ctypes.CDLL(build.build(f16=f16))
    for n in NEW_SYMBOLS:
        assert re.search(rf"^int {n}\(", src, flags=re.M), n
        assert n in L.EXPORTED_SYMBOLS and hasattr(lib, n), n
        getattr(lib, n).argtypes, getattr(lib, n).restype = L._SIGS[n], ctypes.c_int
    assert lib.feddat_abi_version() == 8 == L.ABI_VERSION
    X = 0x1000          # 16-byte aligned, never dereferenced
    pq = lib.feddat_albef_pad_questions
    for args in ((None, X, X, 2, 3, 12288, 12), (X, None, X, 2, 3, 12288, 12), (X, X, None, 2, 3, 12288, 12),
                 (X, X, X, 0, 3, 12288, 12),           # nq = 0
                 (X, X, X, 4, 3, 12288, 12),           # nq > B
                 (X + 4, X, X, 2, 3, 12288, 12),       # image not 16-byte aligned
                 (X, X + 4, X, 2, 3, 12288, 12),       # question ids not 8-byte aligned
                 (X, X, X + 4, 2, 3, 12288, 12),
                 (X, X, X, 2, 3, 12290, 12)):          # image rows that are no whole 16-byte words
        assert pq(*args, None) == EINVAL, args
    sg = lib.feddat_rank_slab_gather
    ok = dict(nq=3, k=4, M=11, la=4, B=3, N=5, La=5, slab=2)

    def gather(ptrs=(X,) * 8, **kw):
        a = dict(ok, **kw)
        return sg(*ptrs, a["nq"], a["k"], a["M"], a["la"], a["B"], a["N"], a["La"], a["slab"], 0, None)
    for i in (0, 1, 2, 3, 4, 6, 7):                   # (pointer 5, the uint8 mask, is optional)
        assert gather(tuple(None if j == i else X for j in range(8))) == EINVAL, i
    for bad in (dict(nq=0), dict(nq=4), dict(k=12), dict(k=0), dict(la=6), dict(la=1), dict(N=2), dict(slab=3), dict(slab=-1),
                dict(nq=1, slab=1)):                   # (1 question, k = 4, N = 5: one slab)
        assert gather(**bad) == EINVAL, bad
    sl = lib.feddat_rank_slab_loss
    assert sl(None, X, 3, 4, 3, 5, 5, 0, None) == EINVAL and sl(X, None, 3, 4, 3, 5, 5, 0, None) == EINVAL
    for nq, k, B, N, La, slab in ((0, 4, 3, 5, 5, 0), (4, 4, 3, 5, 5, 0), (3, 0, 3, 5, 5, 0), (3, 4, 3, 2, 5, 0), (3, 4, 3, 5, 1, 0),
                                  (3, 4, 3, 5, 5, 3), (3, 4, 3, 5, 5, -1), (3, 64, 3, 3, 5, 64)):
        assert sl(X, X, nq, k, B, N, La, slab, None) == EINVAL, (nq, k, B, N, La, slab)


def test_slab_ops_need_a_device():
    """CPU tensors are refused before the library is touched: there is no host path."""
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64)      # noqa: E731
    with pytest.raises(L.FeddatHipError):
        L.albef_pad_questions(torch.zeros(3, 3, 64, 64), i64(3, 12), i64(3, 12), 2)
    with pytest.raises(L.FeddatHipError):
        L.rank_slab_gather(i64(3, 4), i64(11, 4), i64(11, 4), i64(5, 5), i64(5, 5), None, i64(20), torch.zeros(20), 3, 0, 0)
    with pytest.raises(L.FeddatHipError):
        L.rank_slab_loss(torch.zeros(44), torch.zeros(12), 3, 4, 3, 5, 5, 0)


@pytest.mark.parametrize("nq,k,N,B", [(3, 4, 5, 3), (2, 4, 5, 3), (1, 64, 3, 3), (3, 1, 3, 3), (3, 11, 12, 3), (32, 64, 32, 32)])
def test_rank_slab_plan_properties(nq, k, N, B):
    from feddat_amd.albef_engine import rank_slab_plan, slab_question_of_row
    plan = rank_slab_plan(nq, k, N, B)
    assert len(plan) == math.ceil(nq * k / N)
    assert all(len(ks) == B for ks in plan)
    assert all(0 < sum(ks) <= N for ks in plan) and all(sum(ks) == N for ks in plan[:-1])
    assert [sum(ks[b] for ks in plan) for b in range(B)] == [k] * nq + [0] * (B - nq)
    # flat order: the rows of the slabs, read slab after slab, are the candidates c = 0, 1, ... , i.e. questions c // k
    flat = [b for ks in plan for b, n in enumerate(ks) for _ in range(n)]
    assert flat == [c // k for c in range(nq * k)]
    for s, ks in enumerate(plan):
        q = slab_question_of_row(ks, N)
        live = sum(ks)
        assert len(q) == N and q[:live] == [c // k for c in range(s * N, s * N + live)] and all(0 <= b < nq for b in q)


def test_rank_slab_plan_refuses_what_no_frame_holds():
    from feddat_amd.albef_engine import rank_slab_plan
    for bad in ((0, 4, 5, 3), (4, 4, 5, 3), (3, 0, 5, 3), (3, 4, 2, 3)):
        with pytest.raises(L.FeddatHipError):
            rank_slab_plan(*bad)


def test_main_refuses_bad_eval_options_before_any_device():
    from feddat_amd import train
    with pytest.raises(L.FeddatHipError, match="ALBEF option"):
        train.main(["--encoder_name", "vilt", "--synthetic_answer_list", "20"])
    with pytest.raises(L.FeddatHipError, match="synthetic_answer_list must be >= 0"):
        train.main(["--encoder_name", "albef_no_distill", "--synthetic_answer_list", "-1"])
    for q in ("0", "-3"):
        with pytest.raises(L.FeddatHipError, match="synthetic_eval_questions must be >= 1"):
            train.main(["--encoder_name", "albef_no_distill", "--synthetic_answer_list", "20", "--synthetic_eval_questions", q])


def test_parser_default_is_the_run_without_evaluation():
    from feddat_amd import train
    p = train.build_parser()
    base, zero = vars(p.parse_args([])), vars(p.parse_args(["--synthetic_answer_list", "0"]))
    assert zero == base and base["synthetic_answer_list"] == 0 and base["synthetic_eval_questions"] is None
    a = p.parse_args(["--synthetic_answer_list", "20", "--synthetic_eval_questions", "7"])
    assert (a.synthetic_answer_list, a.synthetic_eval_questions) == (20, 7)
    # nothing else moved: the options the parser had before keep their defaults
    assert {k: v for k, v in base.items() if not k.startswith("synthetic_")} == \
        {k: v for k, v in vars(a).items() if not k.startswith("synthetic_")}


def test_synthetic_answer_list_and_eval_loader():
    from feddat_amd import albef_spec
    ids, mask = albef_spec.synthetic_answer_list(100, 4, 3072, seed=5)
    ids2, mask2 = albef_spec.synthetic_answer_list(100, 4, 3072, seed=5)
    assert torch.equal(ids, ids2) and torch.equal(mask, mask2)
    assert not torch.equal(ids, albef_spec.synthetic_answer_list(100, 4, 3072, seed=6)[0])
    assert ids.shape == mask.shape == (100, 4) and ids.dtype == mask.dtype == torch.int64
    assert len(set(ids[:, 1].tolist())) == 100 and int(ids.max()) < 3072
    assert bool((ids[:, 0] == 101).all())
    lens = mask.sum(1)
    assert set(lens.tolist()) == {3, 4} and bool((ids.gather(1, (lens - 1)[:, None]) == 102).all())      # ends in [SEP]
    assert bool((ids[mask == 0] == 0).all())                                                             # [PAD] behind it
    with pytest.raises(ValueError):
        albef_spec.synthetic_answer_list(3000, 4, 3072)          # not that many distinct first tokens
    loader = albef_spec.synthetic_eval_loader(5, 2, 9, ids, mask, 64, image=64, q_len=10, vocab=3072)
    assert [b["question_ids"].shape[0] for b in loader] == [2, 2, 1]          # the last batch is short
    for b in loader:
        n = b["question_ids"].shape[0]
        assert b["image"].shape == (n, 3, 64, 64) and b["question_mask"].shape == (n, 10) and b["k"] == 64
        assert b["answer_list_ids"] is loader[0]["answer_list_ids"] and len(b["gts"]) == n
        assert all(1 <= len(g) <= 3 and len(set(g)) == len(g) and all(0 <= i < 100 for i in g) for g in b["gts"])
