"""On-device top-K retrieval (csrc/topk.hip through clipmi.evaluation.topk and the C ABI) on the GPU.

The reference is numpy on the host: a stable sort of (-score, index), so equal scores keep the lower candidate
index first.  Exact on integer-valued inputs (every dot product is exact in fp32 in any order) and on hand-made
score blocks fed straight to clipmi_topk_merge; within the fp32 dot-product bound against fp64 on unit vectors;
consistent with the rank kernels on the same inputs; in bounded memory; and through evaluate_retrieval on the tiny
model."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_eval as GE  # noqa: E402  (integer_case, unit_case: the rank tests' inputs)
from clipmi import CLIPAdapterTrainer, CLIPWithAdapters, synth  # noqa: E402
from clipmi import evaluation as EV  # noqa: E402
from clipmi import towers as T  # noqa: E402
from kernel_checks import guarded  # noqa: E402

NEG_INF = -np.inf


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(res):
    return res.scores.cpu().numpy(), res.indices.cpu().numpy()


def canonical(S):
    """The scores as the kernel orders and reports them: a NaN as -inf, -0.0 as +0.0."""
    S = np.asarray(S)
    if S.dtype.kind != "f":
        return S
    return np.where(np.isnan(S), NEG_INF, S) + 0.0


def reference_topk(S, k, exclude=None):
    """(scores float64 [N, k], indices int64 [N, k]) from a full score matrix S [N, M] of an exact dtype: a stable
    sort of (-score, index) per row, candidate exclude[i] removed when it lies in [0, M), padded with -inf / -1."""
    S = canonical(S)
    N, M = S.shape
    order = np.argsort(-S, axis=1, kind="stable")
    scores = np.full((N, k), NEG_INF, np.float64)
    indices = np.full((N, k), -1, np.int64)
    for i in range(N):
        o = order[i]
        if exclude is not None and 0 <= int(exclude[i]) < M:
            o = o[o != int(exclude[i])]
        o = o[:k]
        indices[i, :len(o)] = o
        scores[i, :len(o)] = S[i, o]
    return scores, indices


def assert_equals_reference(got, want):
    (gs, gi), (ws, wi) = got, want
    assert gs.dtype == np.float32 and gi.dtype == np.int32
    assert np.array_equal(gi.astype(np.int64), wi), "indices"
    assert np.array_equal(gs.astype(np.float64), ws), "scores"


def assert_bitwise(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------ 1. exact, integer inputs
@functools.lru_cache(maxsize=None)
def integer_scores(E, N, M):
    q, c, target = GE.integer_case(E, N, M, seed=E + N)
    S = q.astype(np.int64) @ c.astype(np.int64).T
    S.setflags(write=False)
    return q, c, target, S


@pytest.mark.parametrize("E", [64, 200])
@pytest.mark.parametrize("N,M", [(257, 300), (65, 35), (130, 1030)])
def test_integer_topk_is_exact_and_block_independent(E, N, M):
    q, c, _, S = integer_scores(E, N, M)
    qd, cd = cuda(q), cuda(c)
    ks = [1, 10, 64, 256] + ([35] if M == 35 else [])  # M = 35: k = M, and k > M pads; 256 > a block of 128
    for k in ks:
        want = reference_topk(S, k)
        if k > M:
            assert (want[1][:, M:] == -1).all() and (want[1][:, :M] >= 0).all()
        got = host(EV.topk(qd, cd, k, block=128))
        assert_equals_reference(got, want)
        assert_bitwise(got, host(EV.topk(qd, cd, k, block=2048)))  # one block; M = 1030: one workgroup per row


def test_integer_case_ties_across_the_kth_boundary():
    """The case that exercises the index tie-break, asserted from the reference alone."""
    _, _, _, S = integer_scores(64, 257, 300)
    top = -np.sort(-S, axis=1, kind="stable")
    across = (top[:, 9] == top[:, 10]).mean()
    inside = (top[:, :9] == top[:, 1:10]).any(1).mean()
    print(f"\nrows tying across the 10th / 11th boundary {100 * across:.1f} %, inside the top 10 {100 * inside:.1f} %")
    assert across >= 0.05


# ------------------------------------------------------------------------------ 2. direct C-ABI calls
SPECIAL = np.array([-0.0, 0.0, np.inf, 1.5, -np.inf, np.nan, 0.0, -2.0, -0.0, 1.5], np.float32)


def handmade_rows(cols, seed):
    """[7, cols] fp32: strictly ascending (every element passes the threshold), strictly descending (none does
    after the first k), constant, +-0 / +-inf / one NaN, small integers (many ties), normal, ascending pairs."""
    rng = np.random.default_rng(seed)
    j = np.arange(cols, dtype=np.float32)
    special = np.resize(SPECIAL, cols).copy()
    special[np.nonzero(np.isnan(special))[0][1:]] = 0.25  # one NaN
    rows = [j - 7, -j * 0.5, np.full(cols, 3.25, np.float32), special,
            rng.integers(-3, 4, cols).astype(np.float32), rng.standard_normal(cols).astype(np.float32),
            np.floor(j / 2)]
    return np.stack(rows).astype(np.float32)


def block_on_device(block, layout):
    """The block as a device view: "vec" 16-byte aligned with lds % 4 == 0, "scalar" lds = cols + 1 and one
    element off the boundary."""
    rows, cols = block.shape
    if layout == "vec":
        lds, off = (cols + 3) // 4 * 4, 0
    else:
        lds, off = cols + 1, 1
    flat = torch.full((off + rows * lds,), float("nan"), dtype=torch.float32, device="cuda")
    view = torch.as_strided(flat, (rows, cols), (lds, 1), off)
    view.copy_(cuda(block))
    assert (view.data_ptr() % 16 == 0 and lds % 4 == 0) == (layout == "vec")
    return view, lds


def merge_blocks(S, k, blocks, layout, out=None, row0=0, rows=None, exclude=None):
    """clipmi_topk_merge over the column blocks [(col0, cols), ...] of S [N, M] in the given order, first = 1 on
    the first.  -> (scores, indices, check): guarded [N, k] device outputs and their guard check."""
    N, M = S.shape
    rows = N - row0 if rows is None else rows
    if out is None:
        (sc, chk_s), (ix, chk_i) = guarded(N, k, torch.float32), guarded(N, k, torch.int32)
    else:
        sc, ix, chk_s, chk_i = out
    ex = None if exclude is None else cuda(np.asarray(exclude, np.int64))
    for n, (col0, cols) in enumerate(blocks):
        view, lds = block_on_device(S[row0:row0 + rows, col0:col0 + cols], layout)
        T.call("clipmi_topk_merge", T.K.stream(), T.P_(view), lds, N, M, row0, rows, col0, cols, k, 1 if n == 0 else 0,
               T.P_(ex), T.P_(sc), T.P_(ix))
    torch.cuda.synchronize()

    def check():
        chk_s()
        chk_i()
    return sc, ix, check, (chk_s, chk_i)


def np_out(sc, ix):
    return sc.cpu().numpy(), ix.cpu().numpy()


@pytest.mark.parametrize("layout", ["vec", "scalar"])
@pytest.mark.parametrize("cols", [1, 3, 64, 65, 1023, 1025])
def test_handmade_rows_single_block(cols, layout):
    S = handmade_rows(cols, seed=cols)
    for k in (1, 10, 64, 256):
        want = reference_topk(S.astype(np.float64), k)
        if cols >= k:
            assert want[1][2].tolist() == list(range(k))  # the constant row: indices 0 .. k - 1
        sc, ix, check, _ = merge_blocks(S, k, [(0, cols)], layout)
        check()
        got = np_out(sc, ix)
        assert_equals_reference(got, want)
        sc2, ix2, check2, _ = merge_blocks(S, k, [(0, cols)], layout)  # a replay
        check2()
        assert_bitwise(got, np_out(sc2, ix2))


def test_special_values_order():
    """-0.0 == +0.0 (index order), +inf first, -inf and the NaN last with the NaN reported as -inf."""
    S = SPECIAL[None, :].copy()
    sc, ix, check, _ = merge_blocks(S, 10, [(0, 10)], "scalar")
    check()
    gs, gi = np_out(sc, ix)
    assert gi[0].tolist() == [2, 3, 9, 0, 1, 6, 8, 7, 4, 5]
    assert gs[0].tolist() == [np.inf, 1.5, 1.5, 0.0, 0.0, 0.0, 0.0, -2.0, -np.inf, -np.inf]
    assert not np.signbit(gs[0][3:7]).any()


@pytest.mark.parametrize("layout", ["vec", "scalar"])
@pytest.mark.parametrize("M,split", [(2000, 1100), (700, 300), (5000, 3500)])
def test_two_block_merge_in_both_orders(M, split, layout):
    """first = 1 then 0, in both block orders: bitwise equal, and equal to the reference.  M = 2000: a wide block
    (one workgroup per row) and a narrow one; M = 5000: the ascending row flushes every wave many times."""
    S = handmade_rows(M, seed=M)
    a, b = (0, split), (split, M - split)
    for k in (10, 256):
        want = reference_topk(S.astype(np.float64), k)
        sc, ix, check, _ = merge_blocks(S, k, [a, b], layout)
        check()
        fwd = np_out(sc, ix)
        assert_equals_reference(fwd, want)
        sc, ix, check, _ = merge_blocks(S, k, [b, a], layout)
        check()
        assert_bitwise(fwd, np_out(sc, ix))


@pytest.mark.parametrize("M", [300, 1500])
def test_row_sub_range_leaves_its_neighbours(M):
    rng = np.random.default_rng(M)
    S = rng.integers(-5, 6, (9, M)).astype(np.float32)
    k, row0, rows = 10, 2, 5
    (sc, chk_s), (ix, chk_i) = guarded(9, k, torch.float32), guarded(9, k, torch.int32)
    sc.fill_(123.0)
    ix.fill_(777)
    half = M // 2 + 1
    merge_blocks(S, k, [(0, half), (half, M - half)], "vec", out=(sc, ix, chk_s, chk_i), row0=row0, rows=rows)
    chk_s()
    chk_i()
    gs, gi = np_out(sc, ix)
    outside = np.r_[0:row0, row0 + rows:9]
    assert (gs[outside] == 123.0).all() and (gi[outside] == 777).all()
    want = reference_topk(S.astype(np.float64), k)
    assert_equals_reference((gs[row0:row0 + rows], gi[row0:row0 + rows]),
                            (want[0][row0:row0 + rows], want[1][row0:row0 + rows]))


@pytest.mark.parametrize("M,split", [(300, 128), (2000, 1100)])
def test_exclude_removes_exactly_that_candidate(M, split):
    rng = np.random.default_rng(M + 1)
    S = rng.integers(-5, 6, (8, M)).astype(np.float32)
    k = 10
    plain = reference_topk(S.astype(np.float64), k)
    # the best, the k-th, one past the list, a candidate of the second block, and four values that exclude nothing
    exclude = np.array([plain[1][0, 0], plain[1][1, k - 1], reference_topk(S.astype(np.float64), k + 1)[1][2, k],
                        M - 1, M, -1, 2 ** 40, -2 ** 40], np.int64)
    want = reference_topk(S.astype(np.float64), k, exclude)
    assert not np.array_equal(want[1][:2], plain[1][:2]) and np.array_equal(want[1][4:], plain[1][4:])
    blocks = [(0, split), (split, M - split)]
    sc, ix, check, _ = merge_blocks(S, k, blocks, "vec", exclude=exclude)
    check()
    assert_equals_reference(np_out(sc, ix), want)
    sc, ix, check, _ = merge_blocks(S, k, blocks[::-1], "scalar", exclude=exclude)
    check()
    assert_equals_reference(np_out(sc, ix), want)


# ------------------------------------------------------------------------------ 3. float inputs against fp64
def float_case(E, N, M):
    rng = np.random.default_rng(E)
    q = rng.standard_normal((N, E))
    c = rng.standard_normal((M, E))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    return q.astype(np.float32), c.astype(np.float32)


@pytest.mark.parametrize("E,N,M,k", [(64, 257, 300, 10), (512, 257, 96, 16), (768, 65, 35, 8), (64, 130, 1030, 256)])
def test_float_topk_within_the_fp32_dot_product_bound(E, N, M, k):
    """tau = 2 E 2^-24 as in test_float_ranks_within_the_fp32_dot_product_bound.  Order statistics are 1-Lipschitz
    in the sup norm, so every position's score is within tau of the fp64 one; a position whose fp64 score is at
    least 2 tau from both neighbours is determined and its index must agree."""
    q, c = float_case(E, N, M)
    S = q.astype(np.float64) @ c.astype(np.float64).T
    tau = 2.0 * E * 2.0 ** -24
    order = np.argsort(-S, axis=1, kind="stable")
    sorted64 = np.take_along_axis(S, order, 1)
    kk = min(k, M)
    gap = np.full((N, M + 1), np.inf)
    gap[:, 1:M] = sorted64[:, :-1] - sorted64[:, 1:]  # gap[p]: between positions p - 1 and p
    determined = (gap[:, :kk] >= 2 * tau) & (gap[:, 1:kk + 1] >= 2 * tau)
    print(f"\n[E={E} N={N} M={M} k={k}] determined positions {100 * determined.mean():.1f} %")
    assert determined.mean() >= 0.9  # from the fp64 reference alone
    gs, gi = host(EV.topk(cuda(q), cuda(c), k, block=128))
    assert np.abs(gs[:, :kk].astype(np.float64) - sorted64[:, :kk]).max() <= tau
    assert np.array_equal(gi[:, :kk][determined], order[:, :kk][determined])
    assert (gi[:, kk:] == -1).all() and (gs[:, kk:] == NEG_INF).all()
    for row in gi[:, :kk]:
        assert len(set(row.tolist())) == kk and row.min() >= 0 and row.max() < M


# ------------------------------------------------------------------------------ 4. consistency with the ranks
def _rank_consistency(q, c, target, k, block):
    qd, cd, td = cuda(q), cuda(c), cuda(target)
    ranks = GE.host(EV.target_ranks(qd, cd, td, block=block))
    gs, gi = host(EV.topk(qd, cd, k, block=block))
    assert np.array_equal(gi[:, 0], ranks["top1"])
    assert gs[:, 0].tobytes() == ranks["top1_score"].tobytes()
    listed = (gi == target[:, None]).any(1)
    assert (ranks["greater"][listed] < k).all()
    assert listed[ranks["greater"] + ranks["equal"] < k].all()
    assert listed.any() and not listed.all()
    # exclude = target: never listed, the others keep their order
    es, ei = host(EV.topk(qd, cd, k, exclude=td, block=block))
    assert not (ei == target[:, None]).any()
    ws, wi = host(EV.topk(qd, cd, k + 1, block=block))
    for i in range(len(target)):
        keep = wi[i] != target[i]
        assert np.array_equal(ei[i], wi[i][keep][:k]) and es[i].tobytes() == ws[i][keep][:k].tobytes()


def test_topk_agrees_with_the_ranks_on_the_integer_case():
    q, c, target, _ = integer_scores(64, 257, 300)
    _rank_consistency(q, c, target, 10, 128)


def test_topk_agrees_with_the_ranks_on_a_float_case():
    q, c, target = GE.unit_case(64, 257, 300, seed=64)
    _rank_consistency(q, c, target, 10, 128)


# ------------------------------------------------------------------------------ 5. bounded memory
def test_scratch_is_one_block_plus_the_outputs():
    N = M = 4096
    k, block = 10, 256
    g = torch.Generator(device="cuda").manual_seed(3)
    q = torch.nn.functional.normalize(torch.randn(N, 64, device="cuda", generator=g), dim=1)
    c = torch.nn.functional.normalize(torch.randn(M, 64, device="cuda", generator=g), dim=1)
    EV.topk(q[:300], c[:300], k, block=block)  # library load, kernel modules
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = EV.topk(q, c, k, block=block)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    bound = block * block * 4 + N * k * 8 + (N + M) * 64 * 4  # one block, the outputs, the inputs
    print(f"\npeak rise {rise / 2**20:.2f} MiB, bound {bound / 2**20:.2f} MiB (the score matrix is "
          f"{N * M * 4 / 2**20:.0f} MiB)")
    assert rise <= bound < N * M * 4 // 16
    gs, gi = host(res)
    assert gi.min() >= 0 and gi.max() < M and (np.diff(gs, axis=1) <= 0).all()
    top1 = (q @ c.T).argmax(1).cpu().numpy()  # 64 MiB, after the measurement
    assert (gi[:, 0] == top1).mean() > 0.999


def test_topk_rejects_empty_and_wrong_arguments_on_the_gpu():
    q, c = torch.zeros(5, 8, device="cuda"), torch.zeros(7, 8, device="cuda")
    with pytest.raises(ValueError, match="empty"):
        EV.topk(q[:0], c, 3)
    with pytest.raises(ValueError, match="empty"):
        EV.topk(q, c[:0], 3)
    with pytest.raises(ValueError, match="block"):
        EV.topk(q, c, 3, block=0)
    with pytest.raises(ValueError, match="GPU tensors"):
        EV.topk(q, c.cpu(), 3)
    with pytest.raises(ValueError, match="exclude"):
        EV.topk(q, c, 3, exclude=torch.zeros(7, dtype=torch.int64, device="cuda"))
    gs, gi = host(EV.topk(q, c, 3))  # all scores equal: indices 0, 1, 2
    assert (gi == np.arange(3)).all() and (gs == 0).all()


# ------------------------------------------------------------------------------ 6. the model path
def test_evaluate_retrieval_returns_the_topk_lists(tmp_path):
    m = CLIPWithAdapters("tiny", use_shared_adapters=False, device="cuda", precision="fp32", pooling="eos")
    b_np = synth.synthetic_batch(m.config, 21, seed=7)
    loader = [{k: torch.from_numpy(v[i:j]) for k, v in b_np.items()} for i, j in ((0, 8), (8, 16), (16, 21))]
    plain = EV.evaluate_retrieval(m, loader, ks=(1, 5), block=16)
    keys = {"n", "i2t", "t2i"} | {f"{d}_{s}" for d in ("i2t", "t2i") for s in ("R@1", "R@5", "median_rank", "mean_rank")}
    assert set(plain) == keys  # the default result is what it was
    out = EV.evaluate_retrieval(m, loader, ks=(1, 5), block=16, topk=5)
    assert set(out) == keys | {"i2t_topk", "t2i_topk"}
    assert {k: v for k, v in out.items() if k in keys - {"i2t", "t2i"}} == \
        {k: v for k, v in plain.items() if k in keys - {"i2t", "t2i"}}
    for name in ("i2t", "t2i"):
        top = out[f"{name}_topk"]
        assert isinstance(top, EV.TopK) and top.scores.is_cuda and top.indices.is_cuda
        assert top.scores.shape == (21, 5) and top.scores.dtype == torch.float32
        assert top.indices.shape == (21, 5) and top.indices.dtype == torch.int32
        assert torch.equal(top.indices[:, 0], out[name].top1)
        assert torch.equal(top.scores[:, 0], out[name].top1_score)
        assert (top.scores[:, :-1] >= top.scores[:, 1:]).all()
    with pytest.raises(ValueError):
        EV.evaluate_retrieval(m, loader, topk=257)
    tr = CLIPAdapterTrainer(m, loader, val_dataloader=loader, output_dir=str(tmp_path))
    assert set(tr.evaluate_retrieval(ks=(1, 5))) == keys
    got = tr.evaluate_retrieval(ks=(1, 5), topk=5)
    for name in ("i2t_topk", "t2i_topk"):
        # the trainer walks the default block: one block here, the same candidates in the same order
        assert torch.equal(got[name].indices[:, 0], got[name[:3]].top1)
        assert got[name].indices.shape == (21, 5)
