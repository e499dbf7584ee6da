"""Host-side checks of the group-aware retrieval evaluation (csrc/eval_keys.hip, clipmi/evaluation.py) that need no
GPU: argument validation of the three C-ABI entry points before any HIP call, the Python argument checks, and the
keyed rank / precision / average-precision metrics on hand-written counts."""
import math
import os
import re

import numpy as np
import pytest
import torch

PTR = 4096  # a non-null pointer that validation must reject before anything dereferences it
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "clipmi.h")


def _lib():
    from clipmi import _lib as L
    from clipmi import evaluation  # noqa: F401  (declares the prototypes)
    return L


def test_version_is_at_least_8():
    assert _lib().lib().clipmi_version() >= 8


def test_prototypes_are_in_the_header_and_the_library():
    with open(HEADER, encoding="utf-8") as f:
        text = f.read()
    lib = _lib().lib()
    for name in ("clipmi_group_pick", "clipmi_group_count", "clipmi_topk_hits"):
        assert re.search(r"\bint " + name + r"\(void\* stream,", text), name
        assert getattr(lib, name) is not None
    assert re.search(r"\* 8: .*clipmi_group_pick", text)  # the version comment


def test_names_are_exported_from_the_package():
    import clipmi
    from clipmi import evaluation
    for name in ("GroupRankResult", "group_ranks", "topk_relevance", "precision_at_k", "average_precision_at_k"):
        assert getattr(clipmi, name) is getattr(evaluation, name)


def _pick(L, **kw):
    a = dict(S=PTR, lds=128, N=300, M=400, row0=128, rows=128, col0=256, cols=128, qkeys=PTR, ckeys=PTR, exclude=PTR,
             first=1, pos_score=PTR, pos_idx=PTR, n_pos=PTR)
    a.update(kw)
    return L.lib().clipmi_group_pick(None, a["S"], a["lds"], a["N"], a["M"], a["row0"], a["rows"], a["col0"],
                                     a["cols"], a["qkeys"], a["ckeys"], a["exclude"], a["first"], a["pos_score"],
                                     a["pos_idx"], a["n_pos"])


def _count(L, **kw):
    a = dict(S=PTR, lds=128, N=300, M=400, row0=128, rows=128, col0=256, cols=128, qkeys=PTR, ckeys=PTR, exclude=PTR,
             pos_score=PTR, n_pos=PTR, first=1, greater=PTR, equal=PTR, top1=PTR, top1_score=PTR)
    a.update(kw)
    return L.lib().clipmi_group_count(None, a["S"], a["lds"], a["N"], a["M"], a["row0"], a["rows"], a["col0"],
                                      a["cols"], a["qkeys"], a["ckeys"], a["exclude"], a["pos_score"], a["n_pos"],
                                      a["first"], a["greater"], a["equal"], a["top1"], a["top1_score"])


def _hits(L, **kw):
    a = dict(top_idx=PTR, N=300, k=10, M=400, qkeys=PTR, ckeys=PTR, hits=PTR)
    a.update(kw)
    return L.lib().clipmi_topk_hits(None, a["top_idx"], a["N"], a["k"], a["M"], a["qkeys"], a["ckeys"], a["hits"])


BLOCK_CASES = [dict(N=0), dict(N=-3), dict(M=0), dict(M=-1), dict(rows=0), dict(cols=0), dict(rows=-4),
               dict(lds=127), dict(lds=0), dict(row0=-1), dict(row0=200), dict(col0=-1), dict(col0=300), dict(S=None),
               dict(qkeys=None), dict(ckeys=None)]
IDS = dict(ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))


@pytest.mark.parametrize("kw", BLOCK_CASES + [dict(pos_score=None), dict(pos_idx=None), dict(n_pos=None)], **IDS)
def test_group_pick_rejects_bad_arguments_without_gpu(kw):
    L = _lib()
    st = _pick(L, **kw)
    assert st == -1 and b"clipmi_group_pick" in L.lib().clipmi_last_error()
    with pytest.raises(ValueError):
        L.check(st, "clipmi_group_pick")


@pytest.mark.parametrize("kw", BLOCK_CASES + [dict(pos_score=None), dict(n_pos=None), dict(greater=None),
                                              dict(equal=None), dict(top1=None), dict(top1_score=None)], **IDS)
def test_group_count_rejects_bad_arguments_without_gpu(kw):
    L = _lib()
    st = _count(L, **kw)
    assert st == -1 and b"clipmi_group_count" in L.lib().clipmi_last_error()
    with pytest.raises(ValueError):
        L.check(st, "clipmi_group_count")


@pytest.mark.parametrize("kw", [dict(N=0), dict(N=-1), dict(M=0), dict(M=-5), dict(k=0), dict(k=257), dict(k=-1),
                                dict(top_idx=None), dict(qkeys=None), dict(ckeys=None), dict(hits=None)], **IDS)
def test_topk_hits_rejects_bad_arguments_without_gpu(kw):
    L = _lib()
    st = _hits(L, **kw)
    assert st == -1 and b"clipmi_topk_hits" in L.lib().clipmi_last_error()
    with pytest.raises(ValueError):
        L.check(st, "clipmi_topk_hits")


def test_messages_name_the_fault():
    L = _lib()
    assert _pick(L, lds=100) == -1 and b"leading dimension" in L.lib().clipmi_last_error()
    assert _count(L, qkeys=None) == -1 and b"keys" in L.lib().clipmi_last_error()
    assert _hits(L, k=257) == -1 and b"CLIPMI_TOPK_MAX" in L.lib().clipmi_last_error()


# ------------------------------------------------------------------------------ Python argument checks
def test_group_ranks_argument_errors():
    from clipmi import evaluation as EV
    q, c = torch.zeros(5, 8), torch.zeros(7, 8)
    qk, ck = torch.arange(5), torch.arange(7)
    with pytest.raises(ValueError, match="query_keys must have length 5"):
        EV.group_ranks(q, c, torch.arange(4), ck)
    with pytest.raises(ValueError, match="candidate_keys must have length 7"):
        EV.group_ranks(q, c, qk, list(range(5)))
    with pytest.raises(ValueError, match="int32 or int64"):
        EV.group_ranks(q, c, qk.float(), ck)
    with pytest.raises(ValueError, match="sequence of ints"):
        EV.group_ranks(q, c, qk, [0.5] * 7)
    with pytest.raises(ValueError, match="sequence of ints"):
        EV.group_ranks(q, c, [True] * 5, ck)
    with pytest.raises(ValueError, match="exclude"):
        EV.group_ranks(q, c, qk, ck, exclude=torch.arange(7))
    with pytest.raises(ValueError, match="GPU tensors"):
        EV.group_ranks(q, c, qk, ck)  # CPU features: no fallback
    with pytest.raises(ValueError, match="query \\[N, E\\]"):
        EV.group_ranks(q[0], c, qk, ck)


def test_topk_relevance_argument_errors():
    from clipmi import evaluation as EV
    idx = torch.zeros(5, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU tensors"):
        EV.topk_relevance(idx, torch.arange(5), torch.arange(7))
    with pytest.raises(ValueError, match="query_keys must have length 5"):
        EV.topk_relevance(idx, torch.arange(6), torch.arange(7))
    with pytest.raises(ValueError, match="int32 or int64"):
        EV.topk_relevance(idx, torch.arange(5), torch.arange(7).double())
    with pytest.raises(ValueError, match="int32"):
        EV.topk_relevance(idx.long(), torch.arange(5), torch.arange(7))
    with pytest.raises(ValueError, match="no candidate keys"):
        EV.topk_relevance(idx, torch.arange(5), [])
    with pytest.raises(ValueError):
        EV.topk_relevance(torch.zeros(5, 300, dtype=torch.int32), torch.arange(5), torch.arange(7))


# ------------------------------------------------------------------------------ metrics on hand-written results
def test_recall_and_rank_summary_skip_rows_without_a_positive():
    from clipmi.evaluation import GroupRankResult, rank_summary, recall_at_k
    greater = np.array([0, -1, 0, 3, 4, -1, 9, 0, 1, 12], dtype=np.int32)
    equal = np.array([0, -1, 2, 0, 1, -1, 0, 5, 0, 0], dtype=np.int32)
    n_pos = np.array([1, 0, 3, 1, 2, 0, 1, 7, 1, 2], dtype=np.int32)
    for res in (GroupRankResult(greater=greater, equal=equal, n_pos=n_pos),
                GroupRankResult(greater=torch.from_numpy(greater), equal=torch.from_numpy(equal),
                                n_pos=torch.from_numpy(n_pos))):
        # the eight rows with a positive; optimistic ranks: 1 1 4 5 10 1 2 13
        assert recall_at_k(res, (1, 5, 10)) == {1: 3 / 8, 5: 6 / 8, 10: 7 / 8}
        assert rank_summary(res) == {"median_rank": 3.0, "mean_rank": 37 / 8}
        # pessimistic ranks: 1 3 4 6 10 6 2 13
        assert recall_at_k(res, (1, 5, 10), ties="pessimistic") == {1: 1 / 8, 5: 4 / 8, 10: 7 / 8}
        assert rank_summary(res, ties="pessimistic") == {"median_rank": 5.0, "mean_rank": 45 / 8}
    with pytest.raises(ValueError):
        recall_at_k(res, (1,), ties="random")


def test_precision_at_k_on_handwritten_hits():
    from clipmi.evaluation import precision_at_k
    hits = torch.tensor([[1, 1, 2, 2], [0, 0, 0, 1], [1, 2, 3, 4], [0, 0, 0, 0]], dtype=torch.int32)
    got = precision_at_k(hits, (1, 2, 4))
    assert got == {1: (1 + 0 + 1 + 0) / 4, 2: (1 / 2 + 0 + 2 / 2 + 0) / 4, 4: (2 / 4 + 1 / 4 + 4 / 4 + 0) / 4}
    assert precision_at_k(hits.numpy(), (3,)) == {3: (2 + 0 + 3 + 0) / 4 / 3}
    assert precision_at_k(hits, ()) == {}
    for bad in (0, 5):
        with pytest.raises(ValueError):
            precision_at_k(hits, (bad,))
    with pytest.raises(ValueError):
        precision_at_k(hits.float(), (1,))
    with pytest.raises(ValueError):
        precision_at_k(hits[0], (1,))


def test_average_precision_at_k_on_handwritten_hits():
    from clipmi.evaluation import average_precision_at_k
    one = torch.tensor([[1, 1, 2, 2]], dtype=torch.int32)
    assert average_precision_at_k(one, torch.tensor([3])) == (1 + 2 / 3) / 3
    assert average_precision_at_k(one, torch.tensor([2])) == (1 + 2 / 3) / 2
    assert average_precision_at_k(one, torch.tensor([9])) == (1 + 2 / 3) / 4  # min(n_pos, k) = k
    hits = torch.tensor([[1, 1, 2, 2], [0, 0, 0, 0], [0, 0, 0, 1], [1, 2, 3, 4], [0, 0, 0, 0]], dtype=torch.int32)
    n_pos = torch.tensor([3, 0, 1, 6, 2])
    # row 1 has no positive at all and is left out; row 4 has positives but retrieved none: AP 0
    want = ((1 + 2 / 3) / 3 + (1 / 4) / 1 + (1 + 1 + 1 + 1) / 4 + 0.0) / 4
    assert abs(average_precision_at_k(hits, n_pos) - want) < 1e-15
    assert abs(average_precision_at_k(hits.numpy(), n_pos.numpy()) - want) < 1e-15
    assert math.isnan(average_precision_at_k(hits[1:2], n_pos[1:2]))
    with pytest.raises(ValueError):
        average_precision_at_k(hits, n_pos[:3])
    with pytest.raises(ValueError):
        average_precision_at_k(hits, n_pos.float())
