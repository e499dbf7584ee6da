"""On-device evaluation (csrc/eval.hip through clipmi/evaluation.py) on the GPU.

Retrieval ranks: exact against an int64 numpy computation on integer-valued inputs (every dot product is exact
in fp32 in any summation order), within a derived bound against fp64 on unit vectors, in bounded memory, with
an out-of-range target reported; evaluate_retrieval and the trainer method over the tiny model.
Classification: the meter against what the reference's evaluate_model computed (tests/golden/evaluation.npz),
and the two evaluate_* drop-ins over the stub-backbone heads of tests/test_gpu_heads.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from clipmi import CLIPAdapterTrainer, CLIPWithAdapters, synth  # noqa: E402
from clipmi import evaluation as EV  # noqa: E402
from clipmi import heads as HD  # noqa: E402
from clipmi import towers as T  # noqa: E402
from heads_common import LN100, fixture, weights  # noqa: E402

EMOS = ["angry", "disgust", "fear", "happy", "neutral", "sad", "surprise"]  # reference constants.EMOTIONS
FIELDS = ("greater", "equal", "top1", "top1_score", "target_score")


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(res):
    res.check()
    return {f: getattr(res, f).cpu().numpy() for f in FIELDS}


def reference_ranks(S, target):
    """The five outputs from a full score matrix S [N, M] (any exact dtype) and targets [N]."""
    n = np.arange(S.shape[0])
    ts = S[n, target]
    return {"greater": (S > ts[:, None]).sum(1), "equal": (S == ts[:, None]).sum(1) - 1, "top1": S.argmax(1),
            "top1_score": S.max(1), "target_score": ts}


def assert_same(got, want, rows=None):
    for f in FIELDS:
        g, w = got[f], want[f]
        if rows is not None:
            g, w = g[rows], w[rows]
        assert np.array_equal(g.astype(np.float64), np.asarray(w).astype(np.float64)), f


def assert_bitwise(a, b):
    for f in FIELDS:
        assert a[f].dtype == b[f].dtype and a[f].tobytes() == b[f].tobytes(), f


# ------------------------------------------------------------------------------ 1. exact ranks
def integer_case(E, N, M, seed, paired=False):
    rng = np.random.default_rng(seed)
    q = rng.integers(-4, 5, (N, E)).astype(np.float32)
    c = rng.integers(-4, 5, (M, E)).astype(np.float32)
    target = np.arange(N) if paired else rng.integers(0, M, N)
    idx = rng.permutation(M)[:20]
    src, dst = idx[:10], idx[10:]
    c[dst] = c[src]  # ten duplicated candidate rows ...
    if not paired:
        target[:5] = src[:5]  # ... some of them targets (from either side of the copy)
        target[5:8] = dst[5:8]
    return q, c, target.astype(np.int64)


@pytest.mark.parametrize("E", [64, 200])
@pytest.mark.parametrize("N,M", [(257, 300), (65, 35), (130, 1030)])
def test_integer_ranks_are_exact_and_block_independent(E, N, M):
    q, c, target = integer_case(E, N, M, seed=E + N)
    want = reference_ranks(q.astype(np.int64) @ c.astype(np.int64).T, target)
    assert (want["equal"] > 0).sum() >= 8  # the duplicated targets tie
    got = host(EV.target_ranks(cuda(q), cuda(c), cuda(target), block=128))
    assert_same(got, want)
    whole = host(EV.target_ranks(cuda(q), cuda(c), cuda(target), block=2048))  # one block; M = 1030: one workgroup per row
    assert_bitwise(got, whole)


def test_paired_integer_ranks_are_exact():
    q, c, target = integer_case(64, 257, 257, seed=5, paired=True)
    want = reference_ranks(q.astype(np.int64) @ c.astype(np.int64).T, target)
    assert (want["equal"] > 0).sum() >= 10
    got = host(EV.target_ranks(cuda(q), cuda(c), block=128))  # only the diagonal blocks feed the first pass
    assert_same(got, want)
    assert_bitwise(got, host(EV.target_ranks(cuda(q), cuda(c), block=2048)))
    assert_bitwise(got, host(EV.target_ranks(cuda(q), cuda(c), cuda(target), block=128)))  # explicit t_i = i
    with pytest.raises(ValueError):
        EV.target_ranks(cuda(q), cuda(c[:100]))  # paired needs N == M


# the (rows, cols, E) of every GEMM call, in order, at N = 40 and E = 8: block 16 cuts 40 into 16 + 16 + 8 and 24
# into 16 + 8, block 64 leaves one block
GEMM_SCHEDULE = {
    # paired, M = 40: per row range its diagonal block (pass 1), then the three column blocks (pass 2)
    ("paired", 16): [(16, 16, 8), (16, 16, 8), (16, 16, 8), (16, 8, 8),
                     (16, 16, 8), (16, 16, 8), (16, 16, 8), (16, 8, 8),
                     (8, 8, 8), (8, 16, 8), (8, 16, 8), (8, 8, 8)],
    # explicit targets, M = 24: per row range both column blocks in pass 1 and again in pass 2
    ("target", 16): [(16, 16, 8), (16, 8, 8), (16, 16, 8), (16, 8, 8),
                     (16, 16, 8), (16, 8, 8), (16, 16, 8), (16, 8, 8),
                     (8, 16, 8), (8, 8, 8), (8, 16, 8), (8, 8, 8)],
    # topk, M = 40: one pass
    ("topk", 16): [(16, 16, 8), (16, 16, 8), (16, 8, 8), (16, 16, 8), (16, 16, 8), (16, 8, 8),
                   (8, 16, 8), (8, 16, 8), (8, 8, 8)],
    # a single column block is computed once: pass 2 reads it from the scratch
    ("paired", 64): [(40, 40, 8)], ("target", 64): [(40, 24, 8)], ("topk", 64): [(40, 40, 8)],
}


@pytest.mark.parametrize("block", [16, 64])
def test_block_walk_gemm_schedule(block, monkeypatch):
    """The exact ordered list of GEMM calls behind target_ranks and topk (the walk's skip rules), and the results
    of those calls against numpy on the same integer inputs."""
    calls = []
    real = T._gemm_f32

    def recording(*a, **kw):
        calls.append(tuple(a[:3]))
        return real(*a, **kw)

    def run(fn):
        calls.clear()
        monkeypatch.setattr(T, "_gemm_f32", recording)
        out = fn()
        monkeypatch.setattr(T, "_gemm_f32", real)
        return out, list(calls)

    q, c, target = integer_case(8, 40, 40, seed=21, paired=True)
    S = q.astype(np.int64) @ c.astype(np.int64).T
    res, got = run(lambda: EV.target_ranks(cuda(q), cuda(c), block=block))
    assert got == GEMM_SCHEDULE["paired", block]
    assert_same(host(res), reference_ranks(S, target))

    top, got = run(lambda: EV.topk(cuda(q), cuda(c), 5, block=block))
    assert got == GEMM_SCHEDULE["topk", block]
    order = np.argsort(-S, axis=1, kind="stable")[:, :5]  # equal scores: the lower index first
    assert np.array_equal(top.indices.cpu().numpy(), order)
    assert np.array_equal(top.scores.cpu().numpy(), np.take_along_axis(S, order, 1))

    q, c, target = integer_case(8, 40, 24, seed=22)
    res, got = run(lambda: EV.target_ranks(cuda(q), cuda(c), cuda(target), block=block))
    assert got == GEMM_SCHEDULE["target", block]
    assert_same(host(res), reference_ranks(q.astype(np.int64) @ c.astype(np.int64).T, target))


# ------------------------------------------------------------------------------ 2. float ranks
def unit_case(E, N, M, seed):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((N, E))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    c = rng.standard_normal((M, E))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    target = rng.integers(0, M, N)
    planted = np.arange(N) % 2 == 0
    for i in np.nonzero(planted)[0]:
        c[target[i]] += 0.6 * q[i]
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    return q.astype(np.float32), c.astype(np.float32), target.astype(np.int64)


@pytest.mark.parametrize("E,N,M", [(64, 257, 300), (512, 257, 96), (768, 65, 35)])
def test_float_ranks_within_the_fp32_dot_product_bound(E, N, M):
    """tau = 2 E 2^-24: |fl(q.c) - q.c| <= gamma_E |q|.|c| <= ~E 2^-24 for unit vectors (any summation order,
    split-K included), applied to the target's score and to the compared score."""
    q, c, target = unit_case(E, N, M, seed=E)
    S = q.astype(np.float64) @ c.astype(np.float64).T
    tau = 2.0 * E * 2.0 ** -24
    n = np.arange(N)
    ts = S[n, target][:, None]
    other = np.ones_like(S, dtype=bool)
    other[n, target] = False
    lo = ((S > ts + tau) & other).sum(1)
    hi = ((S > ts - tau) & other).sum(1)
    exact_rows = np.where(other, np.abs(S - ts), np.inf).min(1) >= tau
    excluded = 1.0 - exact_rows.mean()
    print(f"\n[E={E} N={N} M={M}] rows within tau of a tie: {100 * excluded:.1f} %")
    assert exact_rows.mean() >= 0.9  # from the fp64 reference alone
    res = EV.target_ranks(cuda(q), cuda(c), cuda(target), block=128)
    got = host(res)
    assert np.all(lo <= got["greater"]) and np.all(got["greater"] <= hi)
    want = ((S > ts) & other).sum(1)
    assert np.array_equal(got["greater"][exact_rows], want[exact_rows])
    assert np.abs(got["target_score"] - ts[:, 0]).max() <= tau
    assert np.abs(got["top1_score"] - S.max(1)).max() <= tau


# ------------------------------------------------------------------------------ 3. bounded memory
def test_scratch_is_one_block():
    N = M = 4096
    g = torch.Generator(device="cuda").manual_seed(3)
    q = torch.nn.functional.normalize(torch.randn(N, 64, device="cuda", generator=g), dim=1)
    c = torch.nn.functional.normalize(torch.randn(M, 64, device="cuda", generator=g), dim=1)
    target = torch.randint(0, M, (N,), device="cuda", generator=g)
    EV.target_ranks(q[:300], c[:300], target[:300] % 300, block=256)  # library load, kernel modules
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = EV.target_ranks(q, c, target, block=256)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"\npeak rise {rise / 2**20:.2f} MiB (the score matrix is {N * M * 4 / 2**20:.0f} MiB)")
    assert rise < 8 * 2**20
    got = host(res)
    assert got["greater"].min() >= 0 and got["greater"].max() < M and (got["top1_score"] >= got["target_score"]).all()
    assert np.array_equal(got["greater"] == 0, got["top1_score"] == got["target_score"])


# ------------------------------------------------------------------------------ 4. bad target
@pytest.mark.parametrize("block", [128, 2048])
def test_out_of_range_target_is_reported(block):
    q, c, target = integer_case(64, 130, 1030, seed=11)
    good = host(EV.target_ranks(cuda(q), cuda(c), cuda(target), block=block))
    for bad_value in (1030, -1):
        t = target.copy()
        t[77] = bad_value
        res = EV.target_ranks(cuda(q), cuda(c), cuda(t), block=block)
        with pytest.raises(IndexError):
            res.check()
        with pytest.raises(IndexError):
            EV.recall_at_k(res, (1,))
        got = {f: getattr(res, f).cpu().numpy() for f in FIELDS}
        rows = np.arange(130) != 77
        assert_same(got, good, rows)
        assert all(got[f][77] == -1 for f in FIELDS)


# ------------------------------------------------------------------------------ 5. evaluate_retrieval
@pytest.mark.parametrize("pooling", ["eos", "first"])
def test_evaluate_retrieval_on_the_tiny_model(pooling, tmp_path):
    """pooling="first" is the reference's quirk Q1: every caption gets the same text feature, so every
    image->text score of a row ties and the optimistic rank is 1 with equal = n - 1."""
    m = CLIPWithAdapters("tiny", use_shared_adapters=False, device="cuda", precision="fp32", pooling=pooling)
    b_np = synth.synthetic_batch(m.config, 21, seed=7)
    loader = [{k: torch.from_numpy(v[i:j]) for k, v in b_np.items()} for i, j in ((0, 8), (8, 16), (16, 21))]
    m.train()
    out = EV.evaluate_retrieval(m, loader, ks=(1, 5, 10), block=16)
    assert m.training
    m.eval()
    assert EV.evaluate_retrieval(m, loader, ks=(1,))["n"] == 21 and not m.training
    txt, img = [], []
    with torch.no_grad():
        for b in loader:
            o = m(**{k: v.cuda() for k, v in b.items()}, return_loss=False)
            txt.append(EV.l2_normalize(o["text_features"]))
            img.append(EV.l2_normalize(o["image_features"]))
    txt, img = torch.cat(txt), torch.cat(img)
    assert out["n"] == 21
    for name, (a, b) in (("i2t", (img, txt)), ("t2i", (txt, img))):
        want = host(EV.target_ranks(a, b, block=16))
        assert_bitwise(host(out[name]), want)
        rank = want["greater"].astype(np.int64) + 1
        for k in (1, 5, 10):
            assert out[f"{name}_R@{k}"] == float(np.mean(rank <= k))
        assert out[f"{name}_median_rank"] == float(np.median(rank))
        assert out[f"{name}_mean_rank"] == float(np.mean(rank))
    if pooling == "first":
        i2t = host(out["i2t"])
        assert (i2t["greater"] == 0).all() and (i2t["equal"] == 20).all() and out["i2t_R@1"] == 1.0
    # the trainer method: the same numbers; evaluate() unchanged
    tr = CLIPAdapterTrainer(m, loader, val_dataloader=loader, output_dir=str(tmp_path))
    got = tr.evaluate_retrieval()
    assert {k: v for k, v in got.items() if k not in ("i2t", "t2i")} == \
        {k: v for k, v in out.items() if k not in ("i2t", "t2i")}
    assert_bitwise(host(got["i2t"]), host(out["i2t"]))
    with torch.no_grad():
        losses = [m(**{k: v.cuda() for k, v in b.items()}, return_loss=True)["loss"].item() for b in loader]
    assert tr.evaluate() == sum(losses) / 3
    with pytest.raises(AssertionError):
        CLIPAdapterTrainer(m, loader, output_dir=str(tmp_path)).evaluate_retrieval()


def test_feature_buffers_grow_or_are_presized():
    r = EV._Rows((3,), torch.float32, "cuda", 0)
    chunks = [torch.full((n, 3), float(n), device="cuda") for n in (2, 5, 1, 9)]
    for ch in chunks:
        r.take(ch.shape[0]).copy_(ch)
    assert torch.equal(r.rows(), torch.cat(chunks)) and r.n == 17
    p = EV._Rows((3,), torch.float32, "cuda", 17)
    base = p.buf.data_ptr()
    for ch in chunks:
        p.take(ch.shape[0]).copy_(ch)
    assert p.buf.data_ptr() == base and torch.equal(p.rows(), torch.cat(chunks))


# ------------------------------------------------------------------------------ 6. classification
def test_meter_reproduces_the_reference_run(golden):
    g = golden("evaluation.npz")
    probs, labels = g["probs"], g["labels"]
    meter = EV.ClassificationMeter(7)
    for i, j in ((0, 10), (10, 30), (30, 37)):
        meter.update(cuda(probs[i:j]), torch.from_numpy(labels[i:j]))
    r = meter.result()
    assert np.array_equal(r.preds, g["preds"]) and r.preds.dtype == np.int64
    assert np.array_equal(r.confidences, g["confidences"]) and r.confidences.dtype == np.float32
    assert np.array_equal(r.confusion, g["conf_matrix"]) and r.confusion.dtype == np.int64
    assert np.array_equal(r.labels, labels) and np.array_equal(r.probs, probs)
    assert EV.accuracy(r.confusion) == float(g["accuracy"])


def test_meter_ties_take_the_lower_index_and_bad_labels_raise():
    probs = np.full((3, 7), 0.05, np.float32)
    probs[0, [5, 2]] = 0.375  # two equal maxima
    probs[1, 6] = 0.7
    probs[2, :] = 1 / 7       # all equal
    meter = EV.ClassificationMeter(7)
    meter.update(cuda(probs), torch.tensor([2, 6, 3]).cuda())
    r = meter.result()
    assert r.preds.tolist() == [2, 6, 0] and r.confidences.tolist() == [probs[0, 2], probs[1, 6], probs[2, 0]]
    want = np.zeros((7, 7), np.int64)
    want[2, 2] = want[6, 6] = want[3, 0] = 1
    assert np.array_equal(r.confusion, want)
    for bad_label in (7, -1):
        meter = EV.ClassificationMeter(7)
        meter.update(cuda(probs), torch.tensor([2, bad_label, 3]))
        with pytest.raises(IndexError):
            meter.result()
        assert meter.confusion.sum().item() == 2  # the bad row is not counted
    with pytest.raises(ValueError):
        meter.update(cuda(probs[:, :5]), torch.tensor([0, 1, 2]))


@pytest.mark.parametrize("B,C", [(3000, 7), (300, 70), (70, 64), (5, 65)])
def test_classify_accumulate_matches_numpy(B, C):
    """Both tally paths (workgroup table up to C = 64, direct atomics above) with more rows than one grid
    pass covers (B = 3000) and accumulation over two updates."""
    rng = np.random.default_rng(B + C)
    probs = rng.random((B, C)).astype(np.float32)
    labels = rng.integers(0, C, B)
    meter = EV.ClassificationMeter(C)
    h = B // 3
    meter.update(cuda(probs[:h]), cuda(labels[:h]))
    meter.update(cuda(probs[h:]), cuda(labels[h:]))
    r = meter.result()
    want = np.zeros((C, C), np.int64)
    np.add.at(want, (labels, probs.argmax(1)), 1)
    assert np.array_equal(r.preds, probs.argmax(1)) and np.array_equal(r.confidences, probs.max(1))
    assert np.array_equal(r.confusion, want)


class StubBackbone:
    """Frozen-backbone stand-in serving the fixture's feature tables, as in tests/test_gpu_heads.py."""
    projection_dim = 512

    def __init__(self, desc, img):
        self.desc, self.img = torch.from_numpy(desc).cuda(), torch.from_numpy(img).cuda()
        self.logit_scale = torch.tensor(LN100, device="cuda")

    def get_text_features(self, input_ids, attention_mask=None):
        return self.desc[input_ids[:, 0]]

    def get_image_features(self, pixel_values):
        return self.img[pixel_values.long()]


def _descs():
    return {e: (torch.arange(i * 5, i * 5 + 5, device="cuda").view(5, 1), None) for i, e in enumerate(EMOS)}


def _loader(labels, extra=None):
    out = []
    for i, j in ((0, 10), (10, 20), (20, 24)):
        item = (torch.arange(i, j), torch.from_numpy(labels[i:j]), [f"img_{k}.jpg" for k in range(i, j)])
        out.append(item + extra(i, j) if extra else item)
    return out


def _check_tuple(res, probs, labels, n_fields):
    assert isinstance(res, tuple) and len(res) == n_fields
    acc, cm, report, preds, labs, paths, confs, sims = res[:8]
    want = np.zeros((7, 7), np.int64)
    np.add.at(want, (labels, probs.argmax(1)), 1)
    assert isinstance(acc, float) and acc == float(np.mean(probs.argmax(1) == labels))
    assert isinstance(cm, np.ndarray) and cm.dtype == np.int64 and np.array_equal(cm, want)
    assert isinstance(report, str) and report == EV.classification_report(want, EMOS, digits=4)
    assert isinstance(preds, list) and np.array_equal(preds, probs.argmax(1))
    assert isinstance(labs, list) and np.array_equal(labs, labels)
    assert paths == [f"img_{k}.jpg" for k in range(24)]
    assert isinstance(confs, list) and np.array_equal(confs, probs.max(1))
    assert isinstance(sims, np.ndarray) and sims.dtype == np.float32 and np.array_equal(sims, probs)


@pytest.mark.parametrize("kind", ["adapter", "zero_shot"])
@pytest.mark.parametrize("use_all", [False, True])
def test_evaluate_model_matches_batchwise_predict(golden, kind, use_all):
    g = golden("heads.npz")
    desc, img, labels = fixture()
    if kind == "adapter":
        model = HD.CLIPAdapter(StubBackbone(desc, img), alpha=0.2, beta=0.2, bottleneck_dim=64, descriptions=_descs())
        for nm, ad in (("visual", model.visual_adapter), ("text", model.text_adapter)):
            ad.load_state_dict_(dict(zip(("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"), weights(g, "init", nm))))
    else:
        model = HD.ZeroShotEmotionRecognition(StubBackbone(desc, img), descriptions=_descs())
    loader = _loader(labels)
    predict = model.predict_with_all_descriptions if use_all else model.predict
    probs = torch.cat([predict(b[0].cuda()) for b in loader]).cpu().numpy()
    _check_tuple(EV.evaluate_model(model, loader, use_all_descriptions=use_all), probs, labels, 8)


def test_evaluate_enhanced_model_gives_the_reference_tuple(golden):
    g = golden("heads.npz")
    desc, img, labels = fixture()
    m = HD.EnhancedCLIPAdapter(StubBackbone(desc, img), alpha=0.2, beta=0.2, gamma=0.3, bottleneck_dim=64,
                               descriptions=_descs(), seed=3)
    for nm, ad in (("visual", m.visual_adapter), ("text", m.text_adapter)):
        ad.load_state_dict_(dict(zip(("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"), weights(g, "init", nm))))
    ctx = torch.from_numpy(np.random.default_rng(4).standard_normal((24, 512)).astype(np.float32))
    m.eval()
    m.encode_emotion_descriptions()
    loader = _loader(labels, lambda i, j: (ctx[i:j], [f"context {k}" for k in range(i, j)]))
    probs = torch.cat([m.predict_probs(b[0].cuda(), b[3].cuda()) for b in loader]).cpu().numpy()
    m.train()
    res = EV.evaluate_enhanced_model(m, loader, EMOS)
    assert not m.training  # utils.py:26 leaves the model in eval mode
    _check_tuple(res, probs, labels, 9)
    assert res[8] == [f"context {k}" for k in range(24)]
    empty = EV.evaluate_enhanced_model(m, [], EMOS)
    assert len(empty) == 9 and empty[0] == 0.0 and empty[1].shape == (7, 7) and empty[2] == "No data to report."
