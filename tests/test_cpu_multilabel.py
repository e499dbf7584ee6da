"""Host-side checks of the multi-label head and metrics (csrc/multilabel.hip, csrc/eval_multilabel.hip,
clipmi.heads / clipmi.evaluation) that need no GPU: argument validation of the entry points before any HIP call,
the float64 references of tests/multilabel_ref.py against torch and (where installed) sklearn, and the host
formulas on hand-written counts."""
import numpy as np
import pytest
import torch

import multilabel_ref as R

PTR = 4096  # a non-null pointer that validation must reject before anything dereferences it


def _lib():
    from clipmi import _lib as L
    from clipmi import evaluation, heads  # noqa: F401  (declare the prototypes)
    return L


def test_version_is_at_least_14():
    assert _lib().lib().clipmi_version() >= 14


def _bce(L, **kw):
    a = dict(img=PTR, B=4, E=64, desc=PTR, off=PTR, C=5, scale=100.0, bias=PTR, targets=PTR, pos_weight=PTR,
             scores=PTR, probs=PTR, loss_rows=PTR, dscore=PTR, bad=PTR)
    a.update(kw)
    return L.lib().clipmi_class_bce(None, a["img"], a["B"], a["E"], a["desc"], a["off"], a["C"], a["scale"],
                                    a["bias"], a["targets"], a["pos_weight"], a["scores"], a["probs"],
                                    a["loss_rows"], a["dscore"], a["bad"])


def _ap(L, **kw):
    a = dict(scores=PTR, targets=PTR, N=100, C=5, ld=100, ge_all=PTR, ge_pos=PTR, n_pos=PTR, bad=PTR)
    a.update(kw)
    return L.lib().clipmi_ap_count(None, a["scores"], a["targets"], a["N"], a["C"], a["ld"], a["ge_all"],
                                   a["ge_pos"], a["n_pos"], a["bad"])


def _acc(L, **kw):
    a = dict(probs=PTR, targets=PTR, B=8, C=5, thr=PTR, counts=PTR, exact_rows=PTR, bad=PTR)
    a.update(kw)
    return L.lib().clipmi_multilabel_accumulate(None, a["probs"], a["targets"], a["B"], a["C"], a["thr"],
                                                a["counts"], a["exact_rows"], a["bad"])


def _ids(kw):
    return "-".join(f"{k}={v}" for k, v in kw.items())


@pytest.mark.parametrize("kw", [dict(B=0), dict(B=-1), dict(E=0), dict(E=-8), dict(E=1025), dict(C=0), dict(C=-1),
                                dict(C=1025), dict(img=None), dict(desc=None), dict(off=None), dict(bad=None),
                                dict(targets=None)], ids=_ids)  # targets=None: pos_weight needs targets
def test_class_bce_rejects_bad_arguments_without_gpu(kw):
    L = _lib()
    st = _bce(L, **kw)
    assert st == -1 and b"clipmi_class_bce" in L.lib().clipmi_last_error()
    with pytest.raises(ValueError):
        L.check(st, "clipmi_class_bce")


@pytest.mark.parametrize("kw", [dict(N=0), dict(N=-5), dict(C=0), dict(C=-1), dict(C=70000), dict(ld=99), dict(ld=0),
                                dict(ld=-1), dict(scores=None), dict(targets=None), dict(ge_all=None),
                                dict(ge_pos=None), dict(n_pos=None), dict(bad=None)], ids=_ids)
def test_ap_count_rejects_bad_arguments_without_gpu(kw):
    L = _lib()
    st = _ap(L, **kw)
    assert st == -1 and b"clipmi_ap_count" in L.lib().clipmi_last_error()
    with pytest.raises(ValueError):
        L.check(st, "clipmi_ap_count")


@pytest.mark.parametrize("kw", [dict(B=0), dict(B=-1), dict(C=0), dict(C=-2), dict(C=1025), dict(probs=None),
                                dict(targets=None), dict(counts=None), dict(exact_rows=None), dict(bad=None)],
                         ids=_ids)
def test_multilabel_accumulate_rejects_bad_arguments_without_gpu(kw):
    L = _lib()
    st = _acc(L, **kw)
    assert st == -1 and b"clipmi_multilabel_accumulate" in L.lib().clipmi_last_error()
    with pytest.raises(ValueError):
        L.check(st, "clipmi_multilabel_accumulate")


def test_bias_grad_rejects_bad_arguments_without_gpu():
    L = _lib()
    f = L.lib().clipmi_class_bias_grad
    for args in ((PTR, 0, 5, None, PTR), (PTR, 4, 0, None, PTR), (None, 4, 5, None, PTR), (PTR, 4, 5, None, None)):
        assert f(None, *args) == -1 and b"clipmi_class_bias_grad" in L.lib().clipmi_last_error()


def test_messages_name_the_fault():
    L = _lib()
    assert _ap(L, ld=50) == -1 and b"leading dimension" in L.lib().clipmi_last_error()
    assert _ap(L, N=0) == -1 and b"positive" in L.lib().clipmi_last_error()
    assert _bce(L, bad=None) == -1 and b"targets need bad" in L.lib().clipmi_last_error()


@pytest.mark.parametrize("with_pw", [False, True])
@pytest.mark.parametrize("soft", [False, True])
def test_reference_bce_equals_torch(with_pw, soft):
    rng = np.random.default_rng(5 + 2 * with_pw + soft)
    B, C = 9, 26
    z = rng.normal(0, 8, (B, C))
    z[0, :4] = [100.0, -100.0, 0.0, -0.0]
    z[1, :2] = [100.0, -100.0]
    y = rng.random((B, C)) if soft else (rng.random((B, C)) < 0.3).astype(np.float64)
    y[0, :2], y[1, :2] = [1.0, 1.0], [0.0, 0.0]  # both saturations against both labels
    pw = rng.uniform(0.2, 30.0, C) if with_pw else None
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    pwt = None if pw is None else torch.tensor(pw, dtype=torch.float64)
    el = torch.nn.functional.binary_cross_entropy_with_logits(zt, torch.tensor(y), pos_weight=pwt, reduction="none")
    loss_rows, dscore, l = R.bce(z, y, pw)
    assert np.isfinite(l).all()
    np.testing.assert_allclose(l, el.detach().numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(loss_rows, el.mean(1).detach().numpy(), rtol=0, atol=1e-12)
    mean = torch.nn.functional.binary_cross_entropy_with_logits(zt, torch.tensor(y), pos_weight=pwt)
    assert abs(loss_rows.mean() - mean.item()) < 1e-12
    mean.backward()
    np.testing.assert_allclose(dscore / B, zt.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(R.sigmoid(z), torch.sigmoid(zt).detach().numpy(), rtol=0, atol=1e-12)


@pytest.mark.parametrize("N,C,levels", [(1, 3, 2), (2, 1, 2), (17, 3, 2), (64, 3, 5), (300, 5, 5), (1000, 4, 1000),
                                        (257, 26, 2)])
def test_sort_route_ap_equals_the_count_identity(N, C, levels):
    s, t = R.tie_heavy(N, C, levels, seed=N + C)
    ga, gp, npos = R.ap_counts(s, t)
    assert np.array_equal(npos, t.sum(0)) and (ga[t == 0] == 0).all() and (gp[t == 0] == 0).all()
    assert (gp[t == 1] >= 1).all() and (ga >= gp).all()
    a, b = R.ap_from_counts(ga, gp, npos), R.ap_sorted(s, t)
    assert np.array_equal(np.isnan(a), npos == 0) and np.array_equal(np.isnan(b), npos == 0)
    np.testing.assert_allclose(a[npos > 0], b[npos > 0], rtol=0, atol=1e-12)
    if C >= 3:
        assert a[0] == 1.0  # every sample positive: precision 1 at every threshold
        if npos[2]:
            assert abs(a[2] - npos[2] / N) < 1e-12  # all scores equal: one threshold, precision = prevalence
    # the library's host sum of the same integers (class-major) agrees
    from clipmi.evaluation import ap_from_counts
    c = ap_from_counts(ga.T, gp.T, npos)
    np.testing.assert_allclose(c[npos > 0], a[npos > 0], rtol=0, atol=1e-12)
    assert np.array_equal(np.isnan(c), npos == 0)


@pytest.mark.parametrize("N,levels", [(1, 2), (50, 2), (400, 5), (1000, 1000)])
def test_both_routes_equal_sklearn(N, levels):
    metrics = pytest.importorskip("sklearn.metrics")
    s, t = R.tie_heavy(N, 6, levels, seed=3 * N, inf=False)  # sklearn's input check refuses inf
    ga, gp, npos = R.ap_counts(s, t)
    a, b = R.ap_from_counts(ga, gp, npos), R.ap_sorted(s, t)
    for c in range(6):
        if npos[c]:
            want = metrics.average_precision_score(t[:, c], s[:, c])
            assert abs(a[c] - want) < 1e-12 and abs(b[c] - want) < 1e-12, (c, a[c], b[c], want)


def test_result_numbers_from_hand_written_counts():
    from clipmi.evaluation import MultiLabelResult
    #          tp fp fn tn
    counts = [[3, 1, 2, 4],   # p 3/4, r 3/5, f1 6/9
              [0, 0, 0, 10],  # nothing predicted, nothing there: all 0 (zero_division=0)
              [0, 2, 0, 8],   # p 0, r 0/0 -> 0
              [5, 0, 5, 0]]   # p 1, r 1/2, f1 2/3
    r = MultiLabelResult.from_counts(counts, exact_rows=4, n=10, ap=[0.5, np.nan, np.nan, 1.0])
    np.testing.assert_allclose(r.precision, [0.75, 0, 0, 1.0], atol=1e-15)
    np.testing.assert_allclose(r.recall, [0.6, 0, 0, 0.5], atol=1e-15)
    np.testing.assert_allclose(r.f1, [6 / 9, 0, 0, 2 / 3], atol=1e-15)
    assert r.support.tolist() == [5, 0, 0, 10] and r.counts.dtype == np.int64 and r.n == 10
    assert abs(r.micro_f1 - 16 / 26) < 1e-15          # 2 * 8 / (16 + 3 + 7)
    assert abs(r.macro_f1 - (6 / 9 + 2 / 3) / 4) < 1e-15
    assert r.subset_accuracy == 0.4 and abs(r.hamming_loss - 10 / 40) < 1e-15
    assert r.mAP == 0.75 and np.isnan(r.ap[1])         # the empty classes are left out of the mean
    empty = MultiLabelResult.from_counts(np.zeros((2, 4), np.int64), 0, 0, [np.nan, np.nan])
    assert np.isnan(empty.mAP) and empty.subset_accuracy == 0.0 and empty.hamming_loss == 0.0
    assert empty.micro_f1 == 0.0 and empty.macro_f1 == 0.0


def test_result_numbers_equal_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    from clipmi.evaluation import MultiLabelResult
    rng = np.random.default_rng(11)
    p = rng.random((200, 7)).astype(np.float32)
    t = (rng.random((200, 7)) < 0.2).astype(np.uint8)
    t[:, 3] = 0
    counts, exact = R.thresholded_counts(p, t, 0.5)
    r = MultiLabelResult.from_counts(counts, exact, 200, R.ap_sorted(p, t))
    pred = (p >= 0.5).astype(np.uint8)
    pr, rc, f1, sup = metrics.precision_recall_fscore_support(t, pred, average=None, zero_division=0)
    np.testing.assert_allclose(r.precision, pr, atol=1e-15)
    np.testing.assert_allclose(r.recall, rc, atol=1e-15)
    np.testing.assert_allclose(r.f1, f1, atol=1e-15)
    assert r.support.tolist() == sup.tolist()
    assert abs(r.micro_f1 - metrics.f1_score(t, pred, average="micro", zero_division=0)) < 1e-15
    assert abs(r.macro_f1 - metrics.f1_score(t, pred, average="macro", zero_division=0)) < 1e-15
    assert abs(r.subset_accuracy - metrics.accuracy_score(t, pred)) < 1e-15
    assert abs(r.hamming_loss - metrics.hamming_loss(t, pred)) < 1e-15


def test_pos_weight_from_counts():
    from clipmi.heads import pos_weight_from_counts
    w = pos_weight_from_counts([2, 0, 5, 10], 10)
    assert w.dtype == torch.float32 and w.tolist() == [4.0, 1.0, 1.0, 0.0]
    w = pos_weight_from_counts(torch.tensor([1, 3]), 4)
    assert w[0].item() == 3.0 and abs(w[1].item() - 1 / 3) < 1e-7
    for bad in (([11], 10), ([-1], 10), ([1], 0)):
        with pytest.raises(ValueError):
            pos_weight_from_counts(*bad)


def test_meter_and_functions_refuse_cpu_tensors_and_bad_shapes():
    from clipmi.evaluation import MultiLabelMeter, average_precision
    with pytest.raises(ValueError):
        MultiLabelMeter(0)
    with pytest.raises(ValueError):
        MultiLabelMeter(3, threshold=[0.5, 0.5])
    m = MultiLabelMeter(3)
    with pytest.raises(ValueError):
        m.update(torch.zeros(4, 3), torch.zeros(4, 3))  # no CPU fallback
    with pytest.raises(ValueError):
        m.update(torch.zeros(4, 2), torch.zeros(4, 2))
    with pytest.raises(ValueError):
        average_precision(torch.zeros(4, 3), torch.zeros(4, 3))
    with pytest.raises(ValueError):
        average_precision(torch.zeros(4, 3), torch.zeros(4, 2))
    r = m.result()  # nothing seen
    assert r.n == 0 and np.isnan(r.mAP) and r.counts.shape == (3, 4)


def test_names_are_exported_from_the_package():
    import clipmi
    from clipmi import evaluation, heads
    for name in ("average_precision", "MultiLabelMeter", "MultiLabelResult", "evaluate_multilabel"):
        assert getattr(clipmi, name) is getattr(evaluation, name)
    for name in ("class_bce", "MultiLabelCLIPAdapter", "pos_weight_from_counts"):
        assert getattr(clipmi, name) is getattr(heads, name)
