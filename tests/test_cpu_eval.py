"""Host-side checks of the evaluation path (csrc/eval.hip, clipmi/evaluation.py) that need no GPU: argument
validation of the new C-ABI entry points before any HIP call, the sklearn-layout report and accuracy against
what the reference's evaluate_model computed (tests/golden/evaluation*.{npz,txt}, tools/gen_eval_golden.py),
and the rank metrics on hand-written counts."""
import ctypes
import os
import types

import numpy as np
import pytest

EMOTIONS = ["angry", "disgust", "fear", "happy", "neutral", "sad", "surprise"]  # reference constants.EMOTIONS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PTR = 4096  # a non-null pointer that validation must reject before anything dereferences it


def _lib():
    from clipmi import _lib as L
    from clipmi import evaluation  # noqa: F401  (declares the prototypes)
    return L


def test_version_is_at_least_3():
    assert _lib().lib().clipmi_version() >= 3


def _pick(L, **kw):
    a = dict(S=PTR, lds=128, N=300, M=400, row0=128, rows=128, col0=256, cols=128, target=PTR, target_score=PTR,
             bad=PTR)
    a.update(kw)
    return L.lib().clipmi_rank_pick(None, a["S"], a["lds"], a["N"], a["M"], a["row0"], a["rows"], a["col0"],
                                    a["cols"], a["target"], a["target_score"], a["bad"])


def _count(L, **kw):
    a = dict(S=PTR, lds=128, N=300, M=400, row0=128, rows=128, col0=256, cols=128, target=PTR, target_score=PTR,
             first=1, greater=PTR, equal=PTR, top1=PTR, top1_score=PTR)
    a.update(kw)
    return L.lib().clipmi_rank_count(None, a["S"], a["lds"], a["N"], a["M"], a["row0"], a["rows"], a["col0"],
                                     a["cols"], a["target"], a["target_score"], a["first"], a["greater"],
                                     a["equal"], a["top1"], a["top1_score"])


def _classify(L, **kw):
    a = dict(probs=PTR, labels=PTR, B=8, C=7, pred=PTR, conf=PTR, confusion=PTR, bad=PTR)
    a.update(kw)
    return L.lib().clipmi_classify_accumulate(None, a["probs"], a["labels"], a["B"], a["C"], a["pred"], a["conf"],
                                              a["confusion"], a["bad"])


BLOCK_CASES = [dict(N=0), dict(N=-3), dict(M=0), dict(M=-1), dict(rows=0), dict(cols=0), dict(rows=-4),
               dict(lds=127), dict(lds=0), dict(row0=-1), dict(row0=200), dict(col0=-1), dict(col0=300), dict(S=None),
               dict(target=None), dict(target_score=None)]  # target=None: paired needs N == M


@pytest.mark.parametrize("kw", BLOCK_CASES + [dict(bad=None)], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_rank_pick_rejects_bad_arguments_without_gpu(kw):
    L = _lib()
    st = _pick(L, **kw)
    assert st == -1 and b"clipmi_rank_pick" in L.lib().clipmi_last_error()
    with pytest.raises(ValueError):
        L.check(st, "clipmi_rank_pick")


@pytest.mark.parametrize("kw", BLOCK_CASES + [dict(greater=None), dict(equal=None), dict(top1=None),
                                              dict(top1_score=None)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_rank_count_rejects_bad_arguments_without_gpu(kw):
    L = _lib()
    st = _count(L, **kw)
    assert st == -1 and b"clipmi_rank_count" in L.lib().clipmi_last_error()
    with pytest.raises(ValueError):
        L.check(st, "clipmi_rank_count")


def test_rank_messages_name_the_fault():
    L = _lib()
    assert _pick(L, lds=100) == -1 and b"leading dimension" in L.lib().clipmi_last_error()
    assert _count(L, N=0) == -1 and b"positive" in L.lib().clipmi_last_error()
    assert _count(L, target=None) == -1 and b"N == M" in L.lib().clipmi_last_error()


@pytest.mark.parametrize("kw", [dict(B=0), dict(B=-1), dict(C=0), dict(C=-2), dict(C=50000), dict(probs=None),
                                dict(labels=None), dict(pred=None), dict(conf=None), dict(confusion=None),
                                dict(bad=None)], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_classify_accumulate_rejects_bad_arguments_without_gpu(kw):
    L = _lib()
    st = _classify(L, **kw)
    assert st == -1 and b"clipmi_classify_accumulate" in L.lib().clipmi_last_error()
    with pytest.raises(ValueError):
        L.check(st, "clipmi_classify_accumulate")


def test_classification_report_equals_the_reference_string(golden):
    from clipmi.evaluation import classification_report
    g = golden("evaluation.npz")
    with open(os.path.join(GOLDEN, "evaluation_report.txt"), encoding="utf-8") as f:
        want = f.read()
    cm = g["conf_matrix"]
    assert cm.shape == (7, 7) and cm[1].sum() == 0 and cm[:, 1].sum() > 0  # the zero-support row is in the fixture
    assert cm[2].sum() > 0 and cm[:, 2].sum() == 0                          # and the zero_division precision
    assert classification_report(cm, EMOTIONS) == want
    assert classification_report(cm, EMOTIONS, digits=4) == want
    assert classification_report(cm, EMOTIONS, digits=2) != want


def test_accuracy_equals_the_reference(golden):
    from clipmi.evaluation import accuracy
    g = golden("evaluation.npz")
    assert accuracy(g["conf_matrix"]) == float(g["accuracy"])
    assert accuracy(g["conf_matrix"]) == float(np.mean(g["preds"] == g["labels"]))
    assert accuracy(np.zeros((3, 3), np.int64)) == 0.0


def test_golden_is_self_consistent(golden):
    g = golden("evaluation.npz")
    assert g["probs"].shape == (37, 7) and g["probs"].dtype == np.float32
    assert np.array_equal(g["preds"], g["probs"].argmax(1))
    assert np.array_equal(g["confidences"], g["probs"].max(1))
    cm = np.zeros((7, 7), np.int64)
    np.add.at(cm, (g["labels"], g["preds"]), 1)
    assert np.array_equal(cm, g["conf_matrix"])


def test_report_rejects_a_name_count_mismatch():
    from clipmi.evaluation import classification_report
    with pytest.raises(ValueError):
        classification_report(np.eye(3, dtype=np.int64), ["a", "b"])


def test_recall_and_rank_summary_under_both_tie_policies():
    from clipmi.evaluation import RankResult, rank_summary, recall_at_k
    greater = np.array([0, 0, 3, 4, 9, 0, 1, 12], dtype=np.int32)
    equal = np.array([0, 2, 0, 1, 0, 5, 0, 0], dtype=np.int32)
    for res in (RankResult(greater=greater, equal=equal), types.SimpleNamespace(greater=greater, equal=equal)):
        # optimistic ranks: 1 1 4 5 10 1 2 13
        assert recall_at_k(res, (1, 5, 10)) == {1: 3 / 8, 5: 6 / 8, 10: 7 / 8}
        assert recall_at_k(res, (1, 5, 10), ties="optimistic") == recall_at_k(res, (1, 5, 10))
        assert rank_summary(res) == {"median_rank": 3.0, "mean_rank": 37 / 8}
        # pessimistic ranks: 1 3 4 6 10 6 2 13
        assert recall_at_k(res, (1, 5, 10), ties="pessimistic") == {1: 1 / 8, 5: 4 / 8, 10: 7 / 8}
        assert rank_summary(res, ties="pessimistic") == {"median_rank": 5.0, "mean_rank": 45 / 8}
    with pytest.raises(ValueError):
        recall_at_k(res, (1,), ties="random")
    odd = RankResult(greater=np.array([4, 0, 2]), equal=np.array([0, 0, 0]))
    assert rank_summary(odd) == {"median_rank": 3.0, "mean_rank": 3.0}


def test_names_are_exported_from_the_package():
    import clipmi
    from clipmi import evaluation
    for name in ("RankResult", "target_ranks", "recall_at_k", "rank_summary", "evaluate_retrieval",
                 "ClassificationMeter", "classification_report", "accuracy", "evaluate_model",
                 "evaluate_enhanced_model"):
        assert getattr(clipmi, name) is getattr(evaluation, name)


def test_evaluation_imports_no_plotting_or_sklearn():
    import ast
    from clipmi import evaluation
    with open(evaluation.__file__, encoding="utf-8") as f:
        tree = ast.parse(f.read())
    roots = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            roots |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom) and node.level == 0:
            roots.add((node.module or "").split(".")[0])
    assert not roots & {"sklearn", "matplotlib", "seaborn", "pandas"}, roots
