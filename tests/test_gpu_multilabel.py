"""The multi-label head and metrics on the GPU (clipmi.heads.class_bce / MultiLabelCLIPAdapter over
csrc/multilabel.hip; clipmi.evaluation.average_precision / MultiLabelMeter over csrc/eval_multilabel.hip) against
the float64 references of tests/multilabel_ref.py and torch restatements written here.

Tolerances.  The scores are pinned bit for bit to clipmi_class_scores', so the tail is compared with float64
computed from the kernel's own fp32 scores: a few ulp per transcendental (expf, log1pf, one division) gives
16 * 2^-23 * max(1, |ref|) for probs and C * dscore, and a C-term fp32 sum on top gives (C + 16) * 2^-23 *
max(1, max_c |l|) for loss_rows.  Gradients and the trained head use tests/test_gpu_heads.py's bounds for the
single-label head (1e-5 on gradients; 1e-4 on weights after 6 Adam steps and on the predictions, Adam's m / sqrt(v)
amplifying summation-order noise on near-zero gradient entries).  The AP counts and the thresholded tallies are
integers and must be exact; AP against the sort route to 1e-12."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from clipmi import evaluation as EV  # noqa: E402
from clipmi import heads as HD  # noqa: E402
from clipmi import synth  # noqa: E402
from oracle import heads_ref as H  # noqa: E402
import multilabel_ref as R  # noqa: E402

ULP = 2.0 ** -23
AP_ROWS, AP_COLS = 1024, 2048  # csrc/eval_multilabel.hip's row tile and staged column tile


def _unit(shape, seed):
    x = torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).cuda()
    return torch.nn.functional.normalize(x, dim=1)


def _offsets(C, ragged, seed):
    n = np.random.default_rng(seed).integers(1, 6, C) if ragged else np.ones(C, np.int64)
    return torch.from_numpy(np.r_[0, np.cumsum(n)].astype(np.int32)).cuda()


def test_version():
    assert HD._lib.lib().clipmi_version() >= 14


# ------------------------------------------------------------------------------------------ 1. scores
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("B,E,C", [(1, 64, 1), (3, 512, 7), (65, 768, 26), (40, 1024, 9)])
def test_scores_equal_class_scores_bit_for_bit(B, E, C, ragged):
    off = _offsets(C, ragged, B + C)
    img, desc = _unit((B, E), B), _unit((int(off[-1]), E), E + C)
    want, want_probs = HD.class_scores(img, desc, off, 100.0)[:2]
    got = HD.class_bce(img, desc, off, 100.0)[0]
    assert torch.equal(got, want)
    # the same with every output the tail has switched on
    y = (torch.rand(B, C, device="cuda") < 0.2).float()
    assert torch.equal(HD.class_bce(img, desc, off, 100.0, y, torch.full((C,), 3.0))[0], want)
    # and the softmax head itself is where it was: its probabilities are the softmax of those scores
    assert (want_probs - want.softmax(1)).abs().max().item() < 1e-5


# ------------------------------------------------------------------------------------------ 2. the tail
def _check_tail(out, y, pw, C):
    scores, probs, loss_rows, dscore, bad = out
    z = scores.double().cpu().numpy()
    want_rows, want_d, l = R.bce(z, y, pw)
    want_p = R.sigmoid(z)
    ep = np.abs(probs.double().cpu().numpy() - want_p) / np.maximum(1.0, np.abs(want_p))
    ed = np.abs(C * dscore.double().cpu().numpy() - C * want_d) / np.maximum(1.0, np.abs(C * want_d))
    el = np.abs(loss_rows.double().cpu().numpy() - want_rows) / np.maximum(1.0, np.abs(l).max(1))
    print(f"C={C}: probs {ep.max() / ULP:.2f} ulp, C*dscore {ed.max() / ULP:.2f} ulp, loss_rows {el.max() / ULP:.2f} ulp "
          f"(bounds 16, 16, {C + 16})")
    assert torch.isfinite(probs).all() and torch.isfinite(loss_rows).all() and torch.isfinite(dscore).all()
    assert ep.max() <= 16 * ULP and ed.max() <= 16 * ULP and el.max() <= (C + 16) * ULP
    assert bad.item() == 0


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("with_pw", [False, True], ids=["nopw", "pw"])
@pytest.mark.parametrize("B,E,C", [(5, 64, 26), (3, 96, 300)])  # C > 256: more than one class per thread
def test_tail_matches_float64_of_the_kernels_own_scores(B, E, C, with_pw, with_bias, soft):
    rng = np.random.default_rng(C + 4 * with_pw + 2 * with_bias + soft)
    off = _offsets(C, True, C)
    img, desc = _unit((B, E), 1), _unit((int(off[-1]), E), 2)
    y = rng.random((B, C)).astype(np.float32) if soft else (rng.random((B, C)) < 0.15).astype(np.float32)
    pw = rng.uniform(0.2, 30.0, C).astype(np.float32) if with_pw else None
    bias = torch.from_numpy(rng.uniform(-6, 6, C).astype(np.float32)).cuda() if with_bias else None
    out = HD.class_bce(img, desc, off, 40.0, torch.from_numpy(y), pw, bias)
    assert out[0].abs().max().item() > 5  # the logits reach both tails of the sigmoid
    if with_bias:
        assert torch.equal(out[0], HD.class_scores(img, desc, off, 40.0)[0] + bias[None, :])
    _check_tail(out, y, pw, C)


def test_tail_is_finite_at_saturation():
    """z = +-100 (scale 100, identical / opposite unit vectors) against both labels."""
    E = 64
    img = torch.zeros(4, E, device="cuda")
    img[:, 0] = 1.0
    desc = torch.zeros(2, E, device="cuda")
    desc[0, 0], desc[1, 0] = 1.0, -1.0
    off = torch.arange(3, dtype=torch.int32, device="cuda")
    y = np.array([[0, 0], [0, 1], [1, 0], [1, 1]], np.float32)
    for pw in (None, np.array([7.0, 0.5], np.float32)):
        out = HD.class_bce(img, desc, off, 100.0, torch.from_numpy(y), pw)
        assert out[0].cpu().tolist() == [[100.0, -100.0]] * 4
        _check_tail(out, y, pw, 2)  # finite everywhere; probs 0 / 1 or the denormal next to 0
    assert abs(out[2][1].item() - (100.0 + 0.5 * 100.0) / 2) < 1e-4  # y = (0, 1): l = z_0 + pw_1 * (-z_1)


@pytest.mark.parametrize("value", [1.5, -0.25, float("nan")])
def test_a_bad_target_sets_bad(value):
    off = _offsets(7, False, 0)
    img, desc = _unit((6, 64), 1), _unit((7, 64), 2)
    y = torch.zeros(6, 7)
    assert HD.class_bce(img, desc, off, 10.0, y)[4].item() == 0
    y[4, 5] = value
    scores, probs, loss_rows, dscore, bad = HD.class_bce(img, desc, off, 10.0, y)
    assert bad.item() == 1
    assert torch.isfinite(loss_rows).all() and torch.isfinite(dscore).all() and dscore[4, 5].item() == 0.0


# ------------------------------------------------------------------------------------------ 3. gradients
def _bias_grad(dscore):
    B, C = dscore.shape
    g = torch.empty(C, dtype=torch.float32, device="cuda")
    HD.call("clipmi_class_bias_grad", HD.T.K.stream(), dscore.data_ptr(), B, C, None, g.data_ptr())
    return g


@pytest.mark.parametrize("B,C,E", [(40, 9, 512), (300, 26, 512)])  # 300 rows: more than one row per thread
def test_gradients_match_torch_autograd(B, C, E):
    torch.manual_seed(3)
    img = torch.nn.functional.normalize(torch.randn(B, E, device="cuda"), dim=1).requires_grad_(True)
    P = torch.nn.functional.normalize(torch.randn(C, E, device="cuda"), dim=1).requires_grad_(True)
    bias = (0.5 * torch.randn(C, device="cuda")).requires_grad_(True)
    y = (torch.rand(B, C, device="cuda") < 0.2).float()
    pw = torch.rand(C, device="cuda") * 8 + 0.5
    off = torch.arange(C + 1, dtype=torch.int32, device="cuda")
    scores, probs, loss_rows, dscore, bad = HD.class_bce(img.detach(), P.detach(), off, 50.0, y, pw, bias.detach())
    logits = 50.0 * img @ P.T + bias
    assert (scores - logits).abs().max().item() < 1e-4
    loss = torch.nn.BCEWithLogitsLoss(pos_weight=pw)(logits, y)
    mean = torch.empty(1, device="cuda")
    HD.call("clipmi_row_mean", HD.T.K.stream(), loss_rows.data_ptr(), B, mean.data_ptr())
    assert abs(mean.item() - loss.item()) < 1e-5 and bad.item() == 0
    loss.backward()
    dimg, dP = torch.empty_like(img), torch.empty_like(P)
    HD.call("clipmi_class_ce_bwd", HD.T.K.stream(), dscore.data_ptr(), img.data_ptr(), P.data_ptr(), B, C, E, 50.0,
            None, dimg.data_ptr(), dP.data_ptr())
    assert (dimg - img.grad).abs().max().item() < 1e-5
    assert (dP - P.grad).abs().max().item() < 1e-5
    g1, g2 = _bias_grad(dscore), _bias_grad(dscore)
    assert (g1 - bias.grad).abs().max().item() < 1e-5
    assert bias.grad.abs().max().item() > 1e-4  # the comparison is not of zeros
    assert torch.equal(g1, g2)
    again = HD.class_bce(img.detach(), P.detach(), off, 50.0, y, pw, bias.detach())
    assert torch.equal(again[3], dscore) and torch.equal(again[2], loss_rows) and torch.equal(_bias_grad(again[3]), g1)


# ------------------------------------------------------------------------------------------ 4. the head
C26, NDESC, NIMG, DIM = 26, 5, 24, 512


class StubBackbone:
    """Frozen-backbone stand-in serving fixed feature tables, as tests/test_gpu_heads.py's: text ids index the
    description table; image ids below 1000 index the context images, the others the body crops."""
    projection_dim = DIM

    def __init__(self):
        self.desc = torch.from_numpy(synth.normal((C26 * NDESC, DIM), 17, "ml_desc")).cuda()
        self.img = torch.from_numpy(synth.normal((NIMG, DIM), 18, "ml_img")).cuda()
        self.body = torch.from_numpy(synth.normal((NIMG, DIM), 19, "ml_body")).cuda()
        self.logit_scale = torch.tensor(float(np.log(100.0)), device="cuda")

    def get_text_features(self, input_ids, attention_mask=None):
        return self.desc[input_ids[:, 0]]

    def get_image_features(self, pixel_values):
        idx = pixel_values.long()
        return torch.where((idx >= 1000)[:, None], self.body[idx % 1000], self.img[idx % 1000])


def _descs():
    return {f"cat{i:02d}": (torch.arange(i * NDESC, (i + 1) * NDESC, device="cuda").view(NDESC, 1), None)
            for i in range(C26)}


def _targets():
    rng = np.random.default_rng(21)
    y = (rng.random((NIMG, C26)) < 0.08).astype(np.float32)
    y[np.arange(NIMG), rng.integers(0, C26, NIMG)] = 1.0  # at least one category per person
    return torch.from_numpy(y)


def _loader(y):
    idx = torch.arange(NIMG, device="cuda")
    cont = torch.zeros(NIMG, 3)
    return [(idx[i:i + 8], idx[i:i + 8] + 1000, y[i:i + 8], cont[i:i + 8]) for i in range(0, NIMG, 8)]


def _w(ad):
    sd = ad.state_dict_()
    return [sd[k].clone() for k in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")]


def _torch_head(m, bb, y, pw, body, epochs, lr, alpha, beta):
    """The same training restated in torch on the CPU: same initial weights, torch.optim.Adam, BCEWithLogitsLoss.
    -> (visual, text, body weights, bias, predict, predict_all)."""
    img, bod, desc = bb.img.cpu(), bb.body.cpu(), bb.desc.cpu()
    desc_n, protos = H.encode(desc, NDESC)
    wv = [p.requires_grad_(True) for p in _w(m.visual_adapter)]
    wt = [p.requires_grad_(True) for p in _w(m.text_adapter)]
    wb = [p.requires_grad_(True) for p in _w(m.body_adapter)] if body else []
    bias = m.class_bias.detach().cpu().clone().requires_grad_(True)
    opt = torch.optim.Adam(wv + wt + wb + [bias], lr=lr)
    crit = torch.nn.BCEWithLogitsLoss(pos_weight=pw)

    def features(idx):
        f = H.blend(img[idx], wv, alpha, True)
        if body:
            f = (f + H.blend(bod[idx], wb, alpha, True)) / 2.0
            f = f / f.norm(dim=-1, keepdim=True)
        return f

    losses = []
    for _ in range(epochs):
        for i in range(0, NIMG, 8):
            idx = torch.arange(i, i + 8)
            loss = crit(100.0 * features(idx) @ H.blend(protos, wt, beta, False).T + bias, y[idx])
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.item())
    with torch.no_grad():
        f = features(torch.arange(NIMG))
        pred = torch.sigmoid(100.0 * f @ H.blend(protos, wt, beta, False).T + bias)
        s_all = (100.0 * f @ H.blend(desc_n, wt, beta, False).T).view(NIMG, C26, NDESC).amax(2)
        pred_all = torch.sigmoid(s_all + bias)
    return wv, wt, wb, bias.detach(), pred, pred_all, losses


@pytest.mark.parametrize("body", [False, True], ids=["context", "context+body"])
def test_head_training_matches_torch(body, tmp_path):
    bb, y = StubBackbone(), _targets()
    pw = HD.pos_weight_from_counts(y.sum(0), NIMG).clamp(max=20.0)
    m = HD.MultiLabelCLIPAdapter(bb, alpha=0.2, beta=0.2, bottleneck_dim=64, descriptions=_descs(), pos_weight=pw,
                                 class_bias=True, bias_init=-1.0, body=body, seed=5)
    wv, wt, wb, bias, pred, pred_all, losses = _torch_head(m, bb, y, pw, body, 2, 3e-4, 0.2, 0.2)
    hist = m.train(_loader(y), num_epochs=2, learning_rate=3e-4)
    assert len(hist) == 2 and all(np.isfinite(hist))
    assert abs(hist[0] - np.mean(losses[:3])) < 1e-4 and abs(hist[1] - np.mean(losses[3:])) < 1e-4
    pairs = [("visual", m.visual_adapter, wv), ("text", m.text_adapter, wt)] + \
        ([("body", m.body_adapter, wb)] if body else [])
    for nm, ad, ref in pairs:
        for k, got, r in zip(("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"), _w(ad), ref):
            err = (got - r.detach()).abs().max().item()
            assert err < 1e-4, (nm, k, err)
    assert (m.class_bias.cpu() - bias).abs().max().item() < 1e-4
    # the bias has trained (Adam moves an entry by up to lr per step; steps of opposite sign may cancel in one)
    assert (m.class_bias.cpu() + 1.0).abs().max().item() > 1e-3
    idx = torch.arange(NIMG, device="cuda")
    args = (idx, idx + 1000) if body else (idx,)
    p, p_all = m.predict(*args), m.predict_with_all_descriptions(*args)
    np.testing.assert_allclose(p.cpu().numpy(), pred.numpy(), atol=1e-4)
    np.testing.assert_allclose(p_all.cpu().numpy(), pred_all.numpy(), atol=1e-4)
    # save, then load into a freshly initialised head: the same bits
    path = str(tmp_path / "head.pt")
    m.save_adapter_weights(path)
    m2 = HD.MultiLabelCLIPAdapter(bb, alpha=0.2, beta=0.2, bottleneck_dim=64, descriptions=_descs(), pos_weight=pw,
                                  class_bias=True, body=body, seed=99)
    assert not torch.equal(m2.predict(*args), p)
    m2.load_adapter_weights(path)
    assert torch.equal(m2.predict(*args), p) and torch.equal(m2.predict_with_all_descriptions(*args), p_all)
    with pytest.raises(FileNotFoundError):
        m2.load_adapter_weights(str(tmp_path / "missing.pt"))


@pytest.mark.parametrize("value", [1.5, float("nan")])
def test_a_bad_batch_leaves_every_parameter_untouched(value):
    bb, y = StubBackbone(), _targets()
    m = HD.MultiLabelCLIPAdapter(bb, descriptions=_descs(), body=True, seed=5)
    before = [ad.flat.clone() for ad in m._adapters()] + [m.class_bias.clone()]
    y[3, 7] = value
    idx = torch.arange(8, device="cuda")
    with pytest.raises(ValueError):
        m.train_step(idx, y[:8], 3e-4, 100.0, idx + 1000)
    with pytest.raises(ValueError):
        m.train_step(idx, y[:8, :5], 3e-4, 100.0, idx + 1000)
    after = [ad.flat for ad in m._adapters()] + [m.class_bias]
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert all(ad.step_count == 0 for ad in m._adapters()) and m.bias_step_count == 0


# ------------------------------------------------------------------------------------------ 5. AP counts
AP_N = sorted({1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049,
               AP_ROWS - 1, AP_ROWS, AP_ROWS + 1, AP_COLS - 1, AP_COLS, AP_COLS + 1})


@pytest.mark.parametrize("C", [1, 3, 26])
@pytest.mark.parametrize("N", AP_N)
def test_ap_counts_are_exact(N, C):
    for levels in (2, 5, 1000):
        s, t = R.tie_heavy(N, C, levels, seed=7 * N + C + levels)
        ga, gp, npos = R.ap_counts(s, t)
        sd, td = torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda()
        out = EV._ap_counts(sd.t().contiguous(), td.t().contiguous())
        got_all, got_pos, got_n, bad = (x.cpu().numpy() for x in out)
        assert bad[0] == 0
        assert np.array_equal(got_n, npos)
        assert np.array_equal(got_all.T, ga), (levels, np.argwhere(got_all.T != ga)[:4])
        assert np.array_equal(got_pos.T, gp), (levels, np.argwhere(got_pos.T != gp)[:4])
        ap, n_pos = EV.average_precision(sd, td)
        want = R.ap_sorted(s, t)
        assert ap.dtype == np.float64 and n_pos.dtype == np.int64 and np.array_equal(n_pos, npos)
        assert np.array_equal(np.isnan(ap), npos == 0)
        np.testing.assert_allclose(ap[npos > 0], want[npos > 0], rtol=0, atol=1e-12)
        if C >= 3:
            assert np.isnan(ap[1]) and ap[0] == 1.0  # the empty class; the all-positive class
            # the empty class (and any other without positives at a small N) is not in the mean
            assert npos[1] == 0 and abs(np.nanmean(ap) - ap[npos > 0].mean()) < 1e-15
    # float and bool targets are read as 0 / 1 too
    assert np.array_equal(EV.average_precision(sd, td.float())[0], ap, equal_nan=True)
    assert np.array_equal(EV.average_precision(sd, td.bool())[0], ap, equal_nan=True)


def test_ap_count_with_a_padded_leading_dimension():
    """ld > N: the padding of every class row is neither read as a sample nor written."""
    N, C, ld = 1500, 5, 1536
    s, t = R.tie_heavy(N, C, 5, seed=1)
    ga, gp, npos = R.ap_counts(s, t)
    sp = torch.full((C, ld), float("nan"), device="cuda")
    tp = torch.full((C, ld), 7, dtype=torch.uint8, device="cuda")
    sp[:, :N], tp[:, :N] = torch.from_numpy(s.T.copy()).cuda(), torch.from_numpy(t.T.copy()).cuda()
    ge_all = torch.full((C, ld), -5, dtype=torch.int32, device="cuda")
    ge_pos = torch.full((C, ld), -5, dtype=torch.int32, device="cuda")
    n_pos = torch.full((C,), -5, dtype=torch.int32, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    EV.call("clipmi_ap_count", EV.T.K.stream(), sp.data_ptr(), tp.data_ptr(), N, C, ctypes.c_int64(ld),
            ge_all.data_ptr(), ge_pos.data_ptr(), n_pos.data_ptr(), bad.data_ptr())
    assert bad.item() == 0 and np.array_equal(n_pos.cpu().numpy(), npos)
    assert np.array_equal(ge_all[:, :N].cpu().numpy().T, ga) and np.array_equal(ge_pos[:, :N].cpu().numpy().T, gp)
    assert (ge_all[:, N:] == -5).all() and (ge_pos[:, N:] == -5).all()


def test_ap_refuses_nan_scores_and_non_binary_targets():
    s, t = R.tie_heavy(300, 4, 5, seed=2)
    sd, td = torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda()
    EV.average_precision(sd, td)
    s2 = sd.clone()
    s2[299, 3] = float("nan")
    with pytest.raises(ValueError):
        EV.average_precision(s2, td)
    for value in (2.0, 0.5, float("nan")):
        t2 = td.float()
        t2[0, 0] = value
        with pytest.raises(ValueError):
            EV.average_precision(sd, t2)
    m = EV.MultiLabelMeter(4)
    m.update(s2, td)
    with pytest.raises(ValueError):
        m.result()
    m = EV.MultiLabelMeter(4)
    t2 = td.clone()
    t2[5, 1] = 3
    m.update(sd, t2)
    with pytest.raises(ValueError):
        m.result()


# ------------------------------------------------------------------------------------------ 6. the meter
def _probs(B, C, seed):
    rng = np.random.default_rng(seed)
    p = (rng.integers(0, 9, (B, C)) / 8.0).astype(np.float32)  # a grid: probabilities exactly at a threshold occur
    t = (rng.random((B, C)) < 0.3).astype(np.uint8)
    return p, t


@pytest.mark.parametrize("per_class", [False, True], ids=["scalar", "per-class"])
@pytest.mark.parametrize("C", [1, 26])
@pytest.mark.parametrize("B", [1, 64, 65, 300])
def test_meter_counts_are_exact(B, C, per_class):
    p, t = _probs(B, C, B + C)
    thr = (np.random.default_rng(C).integers(1, 8, C) / 8.0).astype(np.float32) if per_class else 0.5
    m = EV.MultiLabelMeter(C, threshold=thr)
    m.update(torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda())
    r = m.result()
    counts, exact = R.thresholded_counts(p, t, thr)
    assert r.counts.dtype == np.int64 and np.array_equal(r.counts, counts) and r.exact_rows == exact
    assert (r.counts.sum(1) == B).all() and r.n == B
    assert r.subset_accuracy == exact / B and abs(r.hamming_loss - (counts[:, 1] + counts[:, 2]).sum() / (B * C)) < 1e-15
    assert np.array_equal(r.probs, p) and np.array_equal(r.targets, t)
    want = R.ap_sorted(p, t)
    assert np.array_equal(np.isnan(r.ap), np.isnan(want))
    np.testing.assert_allclose(r.ap[~np.isnan(want)], want[~np.isnan(want)], rtol=0, atol=1e-12)


def test_meter_in_batches_equals_one_update():
    p, t = _probs(300, 26, 5)
    pd, td = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
    one = EV.MultiLabelMeter(26, capacity=300)
    one.update(pd, td)
    r1 = one.result()
    many = EV.MultiLabelMeter(26)  # grows on demand
    for a, b in ((0, 7), (7, 71), (71, 300)):
        many.update(pd[a:b], td[a:b].float())
    r2 = many.result()
    assert np.array_equal(r1.counts, r2.counts) and r1.exact_rows == r2.exact_rows and r2.n == 300
    assert np.array_equal(r1.ap, r2.ap, equal_nan=True) and r1.mAP == r2.mAP
    assert np.array_equal(r2.probs, p) and np.array_equal(r2.targets, t)


def test_evaluate_multilabel_equals_the_meter_fed_by_hand():
    bb, y = StubBackbone(), _targets()
    for body in (False, True):
        m = HD.MultiLabelCLIPAdapter(bb, descriptions=_descs(), body=body, bias_init=-2.0, seed=5)
        for use_all in (False, True):
            res = EV.evaluate_multilabel(m, _loader(y), threshold=0.3, use_all_descriptions=use_all)
            meter = EV.MultiLabelMeter(C26, threshold=0.3)
            for context, bodies, cat, _ in _loader(y):
                args = (context, bodies) if body else (context,)
                meter.update(m.predict_with_all_descriptions(*args) if use_all else m.predict(*args), cat)
            want = meter.result()
            assert res.n == NIMG and np.array_equal(res.counts, want.counts) and res.exact_rows == want.exact_rows
            assert np.array_equal(res.ap, want.ap, equal_nan=True) and res.mAP == want.mAP
            assert np.array_equal(res.probs, want.probs) and np.array_equal(res.targets, y.numpy().astype(np.uint8))
            counts, exact = R.thresholded_counts(res.probs, res.targets, 0.3)
            assert np.array_equal(res.counts, counts) and res.exact_rows == exact
