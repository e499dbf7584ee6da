"""Group-aware retrieval evaluation (csrc/eval_keys.hip through clipmi.evaluation and the C ABI) on the GPU.

The reference is numpy on the host over the full score matrix.  Exact on integer-valued inputs (every dot product
is exact in fp32 in any order) and on hand-made score blocks fed straight to clipmi_group_pick / clipmi_group_count
inside guard bands; bitwise the diagonal ranks when every key is distinct; consistent with target_ranks on float
inputs; within the fp32 dot-product bound of fp64 on unit vectors; clipmi_topk_hits against numpy; in bounded
memory; and through evaluate_retrieval on the tiny model."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_eval as GE  # noqa: E402  (integer_case, unit_case: the rank tests' inputs)
import test_gpu_topk as TK  # noqa: E402  (block_on_device: the two load paths)
from clipmi import CLIPAdapterTrainer, CLIPWithAdapters, synth  # noqa: E402
from clipmi import evaluation as EV  # noqa: E402
from clipmi import losses as LS  # noqa: E402
from clipmi import towers as T  # noqa: E402
from kernel_checks import guarded1d  # noqa: E402

FIELDS = ("greater", "equal", "n_pos", "pos_idx", "pos_score", "top1", "top1_score")
DTYPES = dict(greater=torch.int32, equal=torch.int32, n_pos=torch.int32, pos_idx=torch.int32,
              pos_score=torch.float32, top1=torch.int32, top1_score=torch.float32)
# seven keys: a negative one, and two pairs that differ only above bit 32
KEYS = np.array([-5, 0, 3, 3 + 2 ** 32, 7, 7 + 2 ** 40, 11], np.int64)
ABSENT = 12345  # a key no candidate carries
NEG_INF = -np.inf

cuda = GE.cuda


def host(res):
    return {f: getattr(res, f).cpu().numpy() for f in FIELDS}


def reference_group(S, qk, ck, exclude=None):
    """The seven outputs from a full score matrix S [N, M] of an exact dtype."""
    S = np.asarray(S).astype(np.float64)
    N, M = S.shape
    live = np.ones((N, M), bool)
    if exclude is not None:
        for i, e in enumerate(exclude):
            if 0 <= int(e) < M:
                live[i, int(e)] = False
    same = np.asarray(qk)[:, None] == np.asarray(ck)[None, :]
    pos, neg = live & same, live & ~same
    n_pos = pos.sum(1)
    ps = np.where(pos, S, NEG_INF)
    pos_score = ps.max(1)
    pos_idx = np.where(n_pos > 0, ps.argmax(1), -1)  # argmax: the lowest index on equal scores
    greater = np.where(n_pos > 0, (neg & (S > pos_score[:, None])).sum(1), -1)
    equal = np.where(n_pos > 0, (neg & (S == pos_score[:, None])).sum(1), -1)
    ls = np.where(live, S, NEG_INF)
    return {"greater": greater, "equal": equal, "n_pos": n_pos, "pos_idx": pos_idx, "pos_score": pos_score,
            "top1": np.where(live.any(1), ls.argmax(1), -1), "top1_score": ls.max(1)}


def assert_same(got, want, rows=None):
    for f in FIELDS:
        g, w = got[f], np.asarray(want[f])
        if rows is not None:
            g, w = g[rows], w[rows]
        assert np.array_equal(g.astype(np.float64), w.astype(np.float64)), f


def assert_bitwise(a, b):
    for f in FIELDS:
        assert a[f].dtype == b[f].dtype and a[f].tobytes() == b[f].tobytes(), f


# ------------------------------------------------------------------------------ 1. exact, integer inputs
@functools.lru_cache(maxsize=None)
def keyed_integer_case(E, N, M):
    """Integers in [-4, 4]; ten candidate rows duplicated, five of the copies under another key (a negative that
    ties a positive bit for bit) and five under the same key (two equal positives: the lower index is the best);
    every ninth query carries a key no candidate has."""
    rng = np.random.default_rng(E + N)
    q = rng.integers(-4, 5, (N, E)).astype(np.float32)
    c = rng.integers(-4, 5, (M, E)).astype(np.float32)
    qi, ci = rng.integers(0, 7, N), rng.integers(0, 7, M)
    idx = rng.permutation(M)[:20]
    src, dst = idx[:10], idx[10:]
    c[dst] = c[src]
    ci[dst[:5]] = (ci[src[:5]] + 1 + rng.integers(0, 6, 5)) % 7  # another key
    ci[dst[5:]] = ci[src[5:]]
    # the first ten queries look for the duplicated rows: q = the row itself, so it scores highest
    q[:10] = c[src]
    qi[:10] = ci[src]
    qk, ck = KEYS[qi], KEYS[ci]
    qk[8::9] = ABSENT
    S = q.astype(np.int64) @ c.astype(np.int64).T
    for a in (q, c, qk, ck, S):
        a.setflags(write=False)
    return q, c, qk, ck, S


@pytest.mark.parametrize("E", [64, 200])
@pytest.mark.parametrize("N,M", [(257, 300), (65, 35), (130, 1030)])
def test_integer_group_ranks_are_exact_and_block_independent(E, N, M):
    q, c, qk, ck, S = keyed_integer_case(E, N, M)
    want = reference_group(S, qk, ck)
    # what the case is there for, from the reference alone
    assert (want["n_pos"] == 0).sum() >= N // 9 and (want["n_pos"] > 1).sum() >= N // 2
    assert (want["equal"][:5] > 0).all()  # the copy under another key ties the best positive
    assert (want["n_pos"][5:8] >= 2).all() and (want["pos_idx"][5:8] >= 0).all()
    assert len({int(k) & 0xFFFFFFFF for k in KEYS}) < len(KEYS)  # keys that agree in their low words
    got = host(EV.group_ranks(cuda(q), cuda(c), cuda(qk), cuda(ck), block=128))
    assert_same(got, want)
    assert got["pos_score"][want["n_pos"] == 0].tolist() == [NEG_INF] * int((want["n_pos"] == 0).sum())
    whole = host(EV.group_ranks(cuda(q), cuda(c), cuda(qk), cuda(ck), block=2048))  # M = 1030: a workgroup per strip
    assert_bitwise(got, whole)
    # keys as a list of ints and as int32 where they fit
    if M == 35:
        small = (np.arange(M) % 3).astype(np.int32)
        a = host(EV.group_ranks(cuda(q), cuda(c), [int(v) for v in np.arange(N) % 4], cuda(small), block=128))
        assert_same(a, reference_group(S, np.arange(N) % 4, small))


@pytest.mark.parametrize("E", [64, 200])
@pytest.mark.parametrize("M", [300, 35, 1030])
def test_integer_group_ranks_same_set_with_exclude(E, M):
    """query is candidates, exclude = arange: a row never retrieves itself and is not its own positive."""
    _, c, _, ck, _ = keyed_integer_case(E, {300: 257, 35: 65, 1030: 130}[M], M)
    S = c.astype(np.int64) @ c.astype(np.int64).T
    ex = np.arange(M, dtype=np.int64)
    want = reference_group(S, ck, ck, ex)
    assert (want["top1"] != ex).all() and (want["pos_idx"] != ex).all()
    plain = reference_group(S, ck, ck)
    assert (plain["top1"] == ex).mean() > 0.6 and (plain["n_pos"] == want["n_pos"] + 1).all()
    cd, kd = cuda(c), cuda(ck)
    got = host(EV.group_ranks(cd, cd, kd, kd, exclude=cuda(ex), block=128))
    assert_same(got, want)
    assert_bitwise(got, host(EV.group_ranks(cd, cd, kd, kd, exclude=cuda(ex), block=2048)))
    # values outside [0, M) exclude nothing
    nothing = np.where(ex % 2 == 0, -1 - ex, M + ex)
    assert_same(host(EV.group_ranks(cd, cd, kd, kd, exclude=cuda(nothing), block=128)), plain)


# ------------------------------------------------------------------------------ 2. the diagonal ranks
@pytest.mark.parametrize("kind", ["integer", "float"])
@pytest.mark.parametrize("block", [128, 2048])
def test_distinct_keys_reduce_to_the_diagonal_ranks(kind, block):
    """All keys distinct, paired data: greater, equal, top1 and top1_score are target_ranks(q, c)'s bit for bit,
    pos_score is target_score, pos_idx = i and n_pos = 1.  The integer case has duplicated candidates, so the tie
    contract (a duplicate of the positive counts in `equal`) is pinned too."""
    if kind == "integer":
        q, c, _ = GE.integer_case(64, 257, 257, seed=5, paired=True)
    else:
        q, c, _ = GE.unit_case(64, 257, 257, seed=64)
    keys = cuda(np.arange(257, dtype=np.int64) * 2 ** 33 - 2 ** 40)
    want = GE.host(EV.target_ranks(cuda(q), cuda(c), block=block))
    if kind == "integer":
        assert (want["equal"] > 0).sum() >= 10
    got = host(EV.group_ranks(cuda(q), cuda(c), keys, keys, block=block))
    for f in ("greater", "equal", "top1", "top1_score"):
        assert got[f].dtype == want[f].dtype and got[f].tobytes() == want[f].tobytes(), f
    assert got["pos_score"].tobytes() == want["target_score"].tobytes()
    assert np.array_equal(got["pos_idx"], np.arange(257)) and (got["n_pos"] == 1).all()


# ------------------------------------------------------------------------------ 3. against target_ranks, floats
def keyed_unit_case(E, N, M):
    """The recipe of the fp64 test: unit vectors, seven keys, every even query planted on one of its positives."""
    rng = np.random.default_rng(E)
    q = rng.standard_normal((N, E))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    c = rng.standard_normal((M, E))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    qk = rng.integers(0, 7, N)
    ck = rng.integers(0, 7, M)
    for i in range(0, N, 2):
        mine = np.nonzero(ck == qk[i])[0]
        if len(mine):
            c[rng.choice(mine)] += 0.6 * q[i]
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    return q.astype(np.float32), c.astype(np.float32), qk.astype(np.int64), ck.astype(np.int64)


@pytest.mark.parametrize("block", [128, 2048])
def test_float_group_ranks_agree_with_target_ranks_on_the_best_positive(block):
    """No tolerance: at the same block the score bits are the same, and no positive scores above the best one."""
    q, c, qk, ck = keyed_unit_case(64, 257, 300)
    qk = qk.copy()
    qk[::11] = ABSENT
    res = EV.group_ranks(cuda(q), cuda(c), cuda(qk), cuda(ck), block=block)
    got = host(res)
    has = got["n_pos"] > 0
    assert has.sum() > 200 and (~has).sum() >= 20
    target = np.where(has, got["pos_idx"], 0).astype(np.int64)
    ranks = GE.host(EV.target_ranks(cuda(q), cuda(c), cuda(target), block=block))
    assert np.array_equal(got["greater"][has], ranks["greater"][has])
    assert got["pos_score"][has].tobytes() == ranks["target_score"][has].tobytes()
    assert got["top1"].tobytes() == ranks["top1"].tobytes()
    assert got["top1_score"].tobytes() == ranks["top1_score"].tobytes()
    assert (got["greater"][~has] == -1).all() and (got["equal"][~has] == -1).all()
    assert (got["pos_idx"][~has] == -1).all() and (got["pos_score"][~has] == NEG_INF).all()


# ------------------------------------------------------------------------------ 4. within the fp32 bound of fp64
@pytest.mark.parametrize("E,N,M", [(64, 257, 300), (512, 257, 96), (768, 65, 35)])
def test_float_group_ranks_within_the_fp32_dot_product_bound(E, N, M):
    """tau = 2 E 2^-24 as in test_float_ranks_within_the_fp32_dot_product_bound: every fp32 score is within tau / 2
    of its fp64 value, and so is the best positive (a maximum is 1-Lipschitz in the sup norm).  A negative more
    than tau above the fp64 best positive is counted, one more than tau below it is not; a row whose best
    positive is at least tau from every negative is determined."""
    q, c, qk, ck = keyed_unit_case(E, N, M)
    S = q.astype(np.float64) @ c.astype(np.float64).T
    want = reference_group(S, qk, ck)
    tau = 2.0 * E * 2.0 ** -24
    neg = qk[:, None] != ck[None, :]
    best = want["pos_score"][:, None]
    lo = (neg & (S > best + tau)).sum(1)
    hi = (neg & (S > best - tau)).sum(1)
    determined = np.where(neg, np.abs(S - best), np.inf).min(1) >= tau
    print(f"\n[E={E} N={N} M={M}] determined rows {100 * determined.mean():.1f} %, rows without a positive "
          f"{(want['n_pos'] == 0).sum()}")
    assert (want["n_pos"] > 0).all()
    assert determined.mean() >= 0.9  # from the fp64 reference alone
    got = host(EV.group_ranks(cuda(q), cuda(c), cuda(qk), cuda(ck), block=128))
    assert np.array_equal(got["n_pos"], want["n_pos"])
    assert np.all(lo <= got["greater"]) and np.all(got["greater"] <= hi)
    assert np.array_equal(got["greater"][determined], want["greater"][determined])
    assert np.abs(got["pos_score"] - want["pos_score"]).max() <= tau
    assert np.abs(got["top1_score"] - want["top1_score"]).max() <= tau
    # the best positive itself: its fp64 score is within tau of the fp64 best
    n = np.arange(N)
    assert (ck[got["pos_idx"]] == qk).all() and (want["pos_score"] - S[n, got["pos_idx"]]).max() <= tau


# ------------------------------------------------------------------------------ 5. direct C-ABI calls
ROWS = 37  # three strips of 16 rows: two full ones and one of five


@functools.lru_cache(maxsize=None)
def handmade(cols, seed, positives=True):
    """S [ROWS, cols] of small integers (many ties), candidate keys from three values, query keys from those and
    one more (rows without a positive); positives=False: no query key occurs among the candidates."""
    rng = np.random.default_rng(seed)
    S = rng.integers(-3, 4, (ROWS, cols)).astype(np.float32)
    ck = KEYS[rng.integers(2, 5, cols)]  # 3, 3 + 2^32, 7
    qk = KEYS[rng.integers(2, 6, ROWS)] if positives else KEYS[rng.integers(5, 7, ROWS)]
    for a in (S, ck, qk):
        a.setflags(write=False)
    return S, qk, ck


SENTINEL = dict(greater=777, equal=778, n_pos=779, pos_idx=780, pos_score=123.0, top1=781, top1_score=124.0)


def run_blocks(S, qk, ck, blocks, layout, exclude=None, row0=0, rows=None):
    """clipmi_group_pick over the column blocks [(col0, cols), ...] of S [N, M] in the given order, then
    clipmi_group_count over the same blocks, first = 1 on the first of each pass; every output sits in a guard
    band and starts from SENTINEL.  -> the seven outputs on the host, after the guard checks."""
    N, M = S.shape
    rows = N - row0 if rows is None else rows
    out, checks = {}, []
    for f in FIELDS:
        out[f], chk = guarded1d(N, DTYPES[f])
        out[f].fill_(SENTINEL[f])
        checks.append(chk)
    qd, cd = cuda(np.asarray(qk, np.int64)), cuda(np.asarray(ck, np.int64))
    ex = None if exclude is None else cuda(np.asarray(exclude, np.int64))
    s = T.K.stream()
    views = [TK.block_on_device(S[row0:row0 + rows, col0:col0 + cols], layout) for col0, cols in blocks]
    for n, ((col0, cols), (view, lds)) in enumerate(zip(blocks, views)):
        T.call("clipmi_group_pick", s, T.P_(view), lds, N, M, row0, rows, col0, cols, T.P_(qd), T.P_(cd), T.P_(ex),
               1 if n == 0 else 0, T.P_(out["pos_score"]), T.P_(out["pos_idx"]), T.P_(out["n_pos"]))
    for n, ((col0, cols), (view, lds)) in enumerate(zip(blocks, views)):
        T.call("clipmi_group_count", s, T.P_(view), lds, N, M, row0, rows, col0, cols, T.P_(qd), T.P_(cd), T.P_(ex),
               T.P_(out["pos_score"]), T.P_(out["n_pos"]), 1 if n == 0 else 0, T.P_(out["greater"]),
               T.P_(out["equal"]), T.P_(out["top1"]), T.P_(out["top1_score"]))
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    return {f: out[f].cpu().numpy() for f in FIELDS}


@pytest.mark.parametrize("layout", ["vec", "scalar"])
@pytest.mark.parametrize("cols", [1, 3, 64, 65, 1023, 1025])
def test_handmade_single_block(cols, layout):
    S, qk, ck = handmade(cols, seed=cols)
    want = reference_group(S, qk, ck)
    assert (want["n_pos"] == 0).any()
    if cols >= 64:
        assert (want["n_pos"] > 1).any() and (want["equal"] > 0).any()
    got = run_blocks(S, qk, ck, [(0, cols)], layout)
    assert_same(got, want)
    assert_bitwise(got, run_blocks(S, qk, ck, [(0, cols)], layout))  # a replay
    # even rows exclude their best positive (-1, where there is none, excludes nothing), odd rows their top1
    ex = np.where(np.arange(ROWS) % 2 == 0, want["pos_idx"], want["top1"])
    wex = reference_group(S, qk, ck, ex)
    if cols >= 64:
        assert (wex["pos_idx"] != want["pos_idx"]).any() and (wex["top1"] != want["top1"]).any()
    assert_same(run_blocks(S, qk, ck, [(0, cols)], layout, exclude=ex), wex)


@pytest.mark.parametrize("layout", ["vec", "scalar"])
@pytest.mark.parametrize("M,split", [(2000, 1100), (700, 300), (130, 1)])
def test_handmade_two_block_merge_in_both_orders(M, split, layout):
    """first = 1 then 0, in both block orders: bitwise equal and equal to the reference.  M = 2000: a wide block (a
    workgroup per strip) and a narrow one; (130, 1): a one-column block."""
    S, qk, ck = handmade(M, seed=M + 1)
    want = reference_group(S, qk, ck)
    a, b = (0, split), (split, M - split)
    fwd = run_blocks(S, qk, ck, [a, b], layout)
    assert_same(fwd, want)
    assert_bitwise(fwd, run_blocks(S, qk, ck, [b, a], layout))
    ex = (np.arange(ROWS) * 53) % M
    assert_same(run_blocks(S, qk, ck, [b, a], layout, exclude=ex), reference_group(S, qk, ck, ex))


@pytest.mark.parametrize("M", [300, 1500])
def test_handmade_positives_in_the_second_block_only(M):
    """The first block holds no positive of any row (pos_idx -1 is merged into), the second all of them."""
    S, qk, _ = handmade(M, seed=M + 2)
    half = M // 2 + 1
    ck = np.where(np.arange(M) < half, KEYS[0], handmade(M, seed=M + 2)[2])
    want = reference_group(S, qk, ck)
    assert (want["pos_idx"][want["n_pos"] > 0] >= half).all() and (want["top1"] < half).any()
    for blocks in ([(0, half), (half, M - half)], [(half, M - half), (0, half)]):
        assert_same(run_blocks(S, qk, ck, blocks, "vec"), want)


@pytest.mark.parametrize("layout", ["vec", "scalar"])
@pytest.mark.parametrize("cols", [65, 1025])
def test_handmade_block_without_any_positive(cols, layout):
    S, qk, ck = handmade(cols, seed=cols + 3, positives=False)
    want = reference_group(S, qk, ck)
    assert (want["n_pos"] == 0).all()
    got = run_blocks(S, qk, ck, [(0, cols)], layout)
    assert_same(got, want)
    assert (got["greater"] == -1).all() and (got["equal"] == -1).all() and (got["pos_idx"] == -1).all()
    assert (got["pos_score"] == NEG_INF).all() and np.array_equal(got["top1"], S.argmax(1))
    half = cols // 2
    assert_bitwise(got, run_blocks(S, qk, ck, [(0, half), (half, cols - half)], layout))


@pytest.mark.parametrize("M", [300, 1500])
def test_handmade_row_sub_range_leaves_its_neighbours(M):
    S, qk, ck = handmade(M, seed=M + 4)
    row0, rows = 5, 21  # a strip of 16 and one of 5
    half = M // 2 + 1
    got = run_blocks(S, qk, ck, [(0, half), (half, M - half)], "vec", row0=row0, rows=rows)
    outside = np.r_[0:row0, row0 + rows:ROWS]
    for f in FIELDS:
        assert (got[f][outside] == SENTINEL[f]).all(), f
    assert_same(got, reference_group(S, qk, ck), rows=np.arange(row0, row0 + rows))


# ------------------------------------------------------------------------------ 6. topk_hits
def reference_hits(indices, qk, ck):
    idx = np.asarray(indices).astype(np.int64)
    M = len(ck)
    ok = (idx >= 0) & (idx < M)
    rel = ok & (np.asarray(ck)[np.where(ok, idx, 0)] == np.asarray(qk)[:, None])
    return np.cumsum(rel, axis=1)


@pytest.mark.parametrize("N,M", [(257, 300), (65, 35), (130, 1030)])
def test_topk_hits_match_numpy_and_agree_with_the_ranks(N, M):
    q, c, qk, ck, S = keyed_integer_case(64, N, M)
    qd, cd, qkd, ckd = cuda(q), cuda(c), cuda(qk), cuda(ck)
    ranks = host(EV.group_ranks(qd, cd, qkd, ckd, block=128))
    has = ranks["n_pos"] > 0
    for k in (1, 10, 35, 256):
        top = EV.topk(qd, cd, k, block=128)
        idx = top.indices.cpu().numpy()
        assert np.array_equal(idx.astype(np.int64), TK.reference_topk(S, k)[1])
        if k > M:
            assert (idx[:, M:] == -1).all()  # padded slots
        hits = EV.topk_relevance(top, qkd, ckd)
        assert hits.is_cuda and hits.dtype == torch.int32 and hits.shape == (N, k)
        h = hits.cpu().numpy()
        assert np.array_equal(h, reference_hits(idx, qk, ck))
        assert np.array_equal(h, EV.topk_relevance(top.indices, qk.tolist(), ck.tolist()).cpu().numpy())
        if k >= M:
            assert np.array_equal(h[:, -1], ranks["n_pos"])  # every candidate is listed
        assert (h[~has] == 0).all()
        assert (h[has & (ranks["greater"] + ranks["equal"] < k), k - 1] > 0).all()
        assert (h[has & (ranks["greater"] >= k), k - 1] == 0).all()
    assert (has & (ranks["greater"] >= 10)).any() and (has & (ranks["greater"] + ranks["equal"] < 10)).any()


@pytest.mark.parametrize("k", [1, 63, 64, 65, 256])
def test_topk_hits_never_read_outside_the_candidate_keys(k):
    """Straight to the C ABI: -1, indices >= M and negative ones are no hits; hits inside a guard band."""
    N, M = 9, 50
    rng = np.random.default_rng(k)
    idx = rng.integers(0, M, (N, k)).astype(np.int32)
    idx[rng.random((N, k)) < 0.2] = -1
    idx[rng.random((N, k)) < 0.1] = M
    idx[rng.random((N, k)) < 0.1] = 2 ** 31 - 1
    idx[rng.random((N, k)) < 0.05] = -2 ** 31
    qk, ck = KEYS[rng.integers(0, 4, N)], KEYS[rng.integers(0, 4, M)]
    out, chk = guarded1d(N * k, torch.int32)
    idx_d, qk_d, ck_d = cuda(idx), cuda(qk), cuda(ck)  # held until the synchronisation
    T.call("clipmi_topk_hits", T.K.stream(), T.P_(idx_d), N, k, M, T.P_(qk_d), T.P_(ck_d), T.P_(out))
    torch.cuda.synchronize()
    chk()
    want = reference_hits(idx, qk, ck)
    assert want[:, -1].max() > 0
    assert np.array_equal(out.cpu().numpy().reshape(N, k), want)


# ------------------------------------------------------------------------------ 7. bounded memory
def test_scratch_is_one_block():
    N = M = 4096
    g = torch.Generator(device="cuda").manual_seed(3)
    q = torch.nn.functional.normalize(torch.randn(N, 64, device="cuda", generator=g), dim=1)
    c = torch.nn.functional.normalize(torch.randn(M, 64, device="cuda", generator=g), dim=1)
    qk = torch.randint(0, 35, (N,), device="cuda", generator=g)
    ck = torch.randint(0, 35, (M,), device="cuda", generator=g)
    EV.group_ranks(q[:300], c[:300], qk[:300], ck[:300], block=256)  # library load, kernel modules
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = EV.group_ranks(q, c, qk, ck, block=256)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"\npeak rise {rise / 2**20:.2f} MiB (the score matrix is {N * M * 4 / 2**20:.0f} MiB)")
    assert rise < 8 * 2**20
    got = host(res)
    assert (got["n_pos"] > 0).all() and got["greater"].min() >= 0 and got["greater"].max() < M
    assert (got["top1_score"] >= got["pos_score"]).all()
    own = ck.cpu().numpy()[got["top1"]] == qk.cpu().numpy()
    assert np.array_equal(got["greater"] == 0, (got["top1_score"] == got["pos_score"]) | own)


# ------------------------------------------------------------------------------ 8. the model path
def test_evaluate_retrieval_with_keys_on_the_tiny_model(tmp_path, monkeypatch):
    m = CLIPWithAdapters("tiny", use_shared_adapters=False, device="cuda", precision="fp32", pooling="eos")
    b_np = dict(synth.synthetic_batch(m.config, 21, seed=7))
    rep = np.arange(21) % 6  # six captions over 21 images
    b_np["input_ids"], b_np["attention_mask"] = b_np["input_ids"][rep], b_np["attention_mask"][rep]
    b_np["emotion"] = (np.arange(21) % 3).astype(np.int64)
    loader = [{k: torch.from_numpy(v[i:j]) for k, v in b_np.items()} for i, j in ((0, 8), (8, 16), (16, 21))]
    plain_keys = {"n", "i2t", "t2i"} | {f"{d}_{s}" for d in ("i2t", "t2i")
                                        for s in ("R@1", "R@5", "median_rank", "mean_rank")}
    scalars = plain_keys - {"i2t", "t2i"}

    # keys=None: today's result, through today's functions
    txt, img = [], []
    with torch.no_grad():
        for b in loader:
            o = m(input_ids=b["input_ids"].cuda(), attention_mask=b["attention_mask"].cuda(),
                  pixel_values=b["pixel_values"].cuda(), return_loss=False)
            txt.append(EV.l2_normalize(o["text_features"]))
            img.append(EV.l2_normalize(o["image_features"]))
    txt, img = torch.cat(txt), torch.cat(img)
    m.train()
    plain = EV.evaluate_retrieval(m, loader, ks=(1, 5), block=16)
    assert m.training and set(plain) == plain_keys
    for name, (a, b) in (("i2t", (img, txt)), ("t2i", (txt, img))):
        want = GE.host(EV.target_ranks(a, b, block=16))
        GE.assert_bitwise(GE.host(plain[name]), want)
        rank = want["greater"].astype(np.int64) + 1
        assert plain[f"{name}_R@1"] == float(np.mean(rank <= 1)) and plain[f"{name}_R@5"] == float(np.mean(rank <= 5))
        assert plain[f"{name}_median_rank"] == float(np.median(rank))
        assert plain[f"{name}_mean_rank"] == float(np.mean(rank))

    # keys="caption" with top-5, and the GEMM calls it costs
    calls = []
    real = T._gemm_f32

    def counting(*a, **kw):
        calls.append(a[:3])
        return real(*a, **kw)

    monkeypatch.setattr(T, "_gemm_f32", counting)
    out = EV.evaluate_retrieval(m, loader, ks=(1, 5, 10), block=16, topk=5, keys="caption")
    monkeypatch.setattr(T, "_gemm_f32", real)
    assert m.training
    blocks = 2 * 2  # ceil(21 / 16) row blocks x column blocks
    assert 0 < len(calls) <= 2 * (2 * blocks)  # two directions, at most two walks each
    grouped = {f"{d}_{s}" for d in ("i2t", "t2i")
               for s in ("gR@1", "gR@5", "gR@10", "g_median_rank", "g_mean_rank", "group", "P@1", "P@5", "mAP@5",
                         "topk", "R@10")}
    assert set(out) == plain_keys | grouped
    assert {k: out[k] for k in scalars} == {k: plain[k] for k in scalars}
    keys = LS.caption_keys(torch.from_numpy(b_np["input_ids"]).cuda())
    assert len(set(keys.tolist())) == 6
    for name, (a, b) in (("i2t", (img, txt)), ("t2i", (txt, img))):
        GE.assert_bitwise(GE.host(out[name]), GE.host(plain[name]))
        want = host(EV.group_ranks(a, b, keys, keys, block=16))
        assert isinstance(out[f"{name}_group"], EV.GroupRankResult)
        assert_bitwise(host(out[f"{name}_group"]), want)
        assert (want["n_pos"] >= 3).all()
        rank = want["greater"].astype(np.int64) + 1
        for k in (1, 5, 10):
            assert out[f"{name}_gR@{k}"] == float(np.mean(rank <= k))
            assert out[f"{name}_gR@{k}"] >= out[f"{name}_R@{k}"]
        assert out[f"{name}_g_median_rank"] == float(np.median(rank))
        assert out[f"{name}_g_mean_rank"] == float(np.mean(rank))
        top = EV.topk(a, b, 5, block=16)
        assert torch.equal(out[f"{name}_topk"].indices, top.indices)
        assert torch.equal(out[f"{name}_topk"].scores, top.scores)
        hits = EV.topk_relevance(top, keys, keys)
        assert np.array_equal(hits.cpu().numpy(), reference_hits(top.indices.cpu().numpy(), keys.cpu().numpy(),
                                                                 keys.cpu().numpy()))
        assert {k: out[f"{name}_P@{k}"] for k in (1, 5)} == EV.precision_at_k(hits, (1, 5))
        assert out[f"{name}_mAP@5"] == EV.average_precision_at_k(hits, out[f"{name}_group"].n_pos)
        assert 0.0 <= out[f"{name}_mAP@5"] <= 1.0 and out[f"{name}_P@1"] == out[f"{name}_gR@1"]
    assert "i2t_P@10" not in out  # 10 > topk

    # a batch field and a callable give what their keys give
    by_field = EV.evaluate_retrieval(m, loader, ks=(1,), block=16, keys="emotion")
    assert set(by_field) == {"n", "i2t", "t2i", "i2t_group", "t2i_group"} | {
        f"{d}_{s}" for d in ("i2t", "t2i")
        for s in ("R@1", "median_rank", "mean_rank", "gR@1", "g_median_rank", "g_mean_rank")}
    emo = torch.from_numpy(b_np["emotion"]).cuda()
    assert_bitwise(host(by_field["i2t_group"]), host(EV.group_ranks(img, txt, emo, emo, block=16)))
    by_call = EV.evaluate_retrieval(m, loader, ks=(1,), block=16, keys=lambda b: [int(v) * 2 ** 35 for v in b["emotion"]])
    assert_bitwise(host(by_call["t2i_group"]), host(by_field["t2i_group"]))
    with pytest.raises(ValueError):
        EV.evaluate_retrieval(m, loader, keys=lambda b: b["emotion"].float())

    # the trainer method: the same numbers at its default block (one block here)
    m.eval()
    tr = CLIPAdapterTrainer(m, loader, val_dataloader=loader, output_dir=str(tmp_path), positives="caption")
    assert set(tr.evaluate_retrieval(ks=(1, 5))) == plain_keys
    got = tr.evaluate_retrieval(ks=(1, 5, 10), topk=5, keys=tr.positives)
    want = EV.evaluate_retrieval(m, loader, ks=(1, 5, 10), topk=5, keys="caption")
    assert not m.training and set(got) == set(want) == set(out)
    tensors = {k for k, v in want.items() if not isinstance(v, (int, float))}
    assert {k: got[k] for k in set(got) - tensors} == {k: want[k] for k in set(want) - tensors}
    assert_bitwise(host(got["i2t_group"]), host(want["i2t_group"]))
    assert_bitwise(host(got["t2i_group"]), host(want["t2i_group"]))
