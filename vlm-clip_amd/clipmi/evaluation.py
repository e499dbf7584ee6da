"""On-device evaluation: retrieval ranks for the contrastive model, classification metrics for the heads.

Three families, all device-resident until one final transfer:

* **Retrieval** (``target_ranks``, ``recall_at_k``, ``rank_summary``, ``evaluate_retrieval``): recall@K and
  median / mean rank of ``CLIPWithAdapters`` over a whole validation set.  The reference has no such metric
  (``trainer.evaluate()`` is a mean of per-batch losses, which depends on the batch size); the naive form needs
  the [N, M] score matrix (40 GB of fp32 at N = 100k).  Here the scores are walked in ``block x block`` tiles of
  the exact-f32 GEMM (``towers._gemm_f32``, the cosines the contrastive head trains on) and reduced by
  csrc/eval.hip, so scratch is one tile.  ``topk`` keeps each query's k best candidates over the same tiles
  (csrc/topk.hip): which candidates were retrieved, or with ``exclude`` the hardest negatives; ``group_ranks``
  ranks the best of the candidates that share the query's key (csrc/eval_keys.hip).  All of them are consumers
  of the one walk, ``_block_walk``, alone or (``evaluate_retrieval`` with keys) together.
* **Classification** (``ClassificationMeter``, ``classification_report``, ``accuracy``, ``evaluate_model``,
  ``evaluate_enhanced_model``): drop-ins for the reference's ``evaluation.evaluate_model`` (evaluation.py:17-68)
  and ``utils.evaluate_enhanced_model`` (utils.py:24-68) without their four ``.cpu()`` round trips per batch and
  without sklearn: argmax, confidence and the confusion matrix accumulate on the device
  (``clipmi_classify_accumulate``), the report is formatted on the host from the confusion matrix in sklearn's
  layout.
* **Multi-label classification** (``average_precision``, ``MultiLabelMeter``, ``evaluate_multilabel``): EMOTIC's
  metric, mean average precision over the categories, exactly sklearn's ``average_precision_score`` from integer
  counts taken on the device (csrc/eval_multilabel.hip), and the thresholded per-class tp / fp / fn / tn with the
  scores derived from them, for ``heads.MultiLabelCLIPAdapter``.

One documented difference from the reference, shared by both ``evaluate_*`` functions: the confusion matrix
always covers all C classes (utils.py:61 does the same with ``labels=range(C)``; evaluation.py:54 lets sklearn
trim classes that occur neither as label nor as prediction, and its own ``classification_report`` call then
raises on the name count).  Results are identical whenever every class occurs among the labels or predictions.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Any, Optional

import numpy as np
import torch

from . import _lib
from . import towers as T

c_vp, c_int, c_i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
_lib.declare("clipmi_rank_pick", [c_vp, c_vp, c_i64, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp])
_lib.declare("clipmi_rank_count", [c_vp, c_vp, c_i64, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_int,
                                   c_vp, c_vp, c_vp, c_vp])
_lib.declare("clipmi_classify_accumulate", [c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp])
_lib.declare("clipmi_topk_merge", [c_vp, c_vp, c_i64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_vp,
                                   c_vp, c_vp])
_lib.declare("clipmi_group_pick", [c_vp, c_vp, c_i64, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp,
                                   c_int, c_vp, c_vp, c_vp])
_lib.declare("clipmi_group_count", [c_vp, c_vp, c_i64, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp,
                                    c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp])
_lib.declare("clipmi_topk_hits", [c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp])
_lib.declare("clipmi_ap_count", [c_vp, c_vp, c_vp, c_int, c_int, c_i64, c_vp, c_vp, c_vp, c_vp])
_lib.declare("clipmi_multilabel_accumulate", [c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp])

P_, call = T.P_, T.call

EMOTIONS = ["angry", "disgust", "fear", "happy", "neutral", "sad", "surprise"]  # constants.EMOTIONS order


# ------------------------------------------------------------------------------ retrieval
@dataclass
class RankResult:
    """Per-query outputs of ``target_ranks`` (device tensors, length N).  With s = the scores of query i and
    t = its target: ``target_score`` = s[t]; ``greater`` / ``equal`` = #{j != t: s[j] > / == s[t]};
    ``top1`` / ``top1_score`` = argmax / max of s (lowest index on ties).  ``bad`` (int32 [1]) is non-zero when
    a target was out of range; that row holds -1 everywhere."""
    greater: Any
    equal: Any
    top1: Any = None
    top1_score: Any = None
    target_score: Any = None
    bad: Any = None

    def check(self):
        """Raise IndexError if a target was out of range (one host synchronisation)."""
        if self.bad is not None and int(torch.as_tensor(self.bad).reshape(-1)[0].item()):
            raise IndexError("target_ranks: a target index is out of range [0, number of candidates)")
        return self


def eval_block():
    """Rows and columns per score block (CLIPMI_EVAL_BLOCK, default 8192: a 256 MiB fp32 scratch)."""
    return max(1, int(os.environ.get("CLIPMI_EVAL_BLOCK") or "8192"))


def l2_normalize(x, out=None):
    """Rows of x [B, E] (fp32, GPU) scaled to unit length by clipmi_l2norm_fwd, the contrastive head's kernel."""
    x = x.to(torch.float32).contiguous()
    if out is None:
        out = torch.empty_like(x)
    nrm = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    call("clipmi_l2norm_fwd", T.K.stream(), P_(x), P_(out), P_(nrm), x.shape[0], x.shape[1])
    return out


def _score_operands(who, query, candidates):
    """The argument checks shared by the block walks: -> (query, candidates) as contiguous fp32."""
    if query.dim() != 2 or candidates.dim() != 2 or query.shape[1] != candidates.shape[1]:
        raise ValueError(f"{who}: query [N, E] and candidates [M, E], got {tuple(query.shape)} and "
                         f"{tuple(candidates.shape)}")
    if not (query.is_cuda and candidates.is_cuda):
        raise ValueError(f"{who} needs GPU tensors (no CPU fallback)")
    if query.shape[0] <= 0 or candidates.shape[0] <= 0 or query.shape[1] <= 0:
        raise ValueError(f"{who}: empty input")
    return query.detach().to(torch.float32).contiguous(), candidates.detach().to(torch.float32).contiguous()


def _block_size(who, block):
    blk = eval_block() if block is None else int(block)
    if blk <= 0:
        raise ValueError(f"{who}: block must be positive")
    return blk


def _exclude_rows(who, exclude, n, dev):
    """``exclude`` as the kernels read it: int64 [n], contiguous, on the features' device (None stays None)."""
    if exclude is None:
        return None
    ex = torch.as_tensor(exclude)
    if ex.shape != (n,):
        raise ValueError(f"{who}: exclude must have shape ({n},), got {tuple(ex.shape)}")
    return ex.detach().to(device=dev, dtype=torch.int64).contiguous()


def target_ranks(query, candidates, target=None, *, block=None) -> RankResult:
    """Rank statistics of each query's target among all candidates, scores = query @ candidates.T.

    query [N, E], candidates [M, E]: fp32 GPU tensors, used as given (no normalisation, so integer-valued
    inputs give exact scores).  target: int64 [N] candidate index per query, or None for paired data
    (t_i = i, needs N == M).  block: rows and columns per GEMM block (default ``eval_block()``).

    Memory: one block x block fp32 scratch plus five length-N outputs; no [N, M] buffer.  Each row range
    walks its column blocks twice with the identical GEMM call: first to read the target scores out of the
    GEMM output (blocks that cannot hold a target are skipped: with paired data only those on the
    diagonal), then to count against them.  The bits of a score depend on the block shape (split-K is chosen
    from it), so the target score is never taken from anywhere else: ties with a duplicate of the target are
    exact.  No host synchronisation; ``RankResult.check()`` reports an out-of-range target."""
    q, c = _score_operands("target_ranks", query, candidates)
    N, M, dev = q.shape[0], c.shape[0], q.device
    if target is None:
        if N != M:
            raise ValueError(f"target_ranks: paired data (target=None) needs N == M, got {N} and {M}")
        tgt = None
    else:
        tgt = torch.as_tensor(target).detach().to(device=dev, dtype=torch.int64).contiguous()
        if tgt.shape != (N,):
            raise ValueError(f"target_ranks: target must have shape ({N},), got {tuple(tgt.shape)}")
    walk = _RankWalk(N, M, dev, tgt)
    _block_walk(q, c, _block_size("target_ranks", block), [walk])
    return walk.res


TOPK_MAX = 256  # CLIPMI_TOPK_MAX of include/clipmi.h


@dataclass
class TopK:
    """Per-query outputs of ``topk`` (device tensors): ``scores`` fp32 [N, k] and ``indices`` int32 [N, k], each
    row sorted best first (higher score first, lower candidate index on equal scores) and padded with -inf / -1
    where fewer than k candidates exist."""
    scores: Any
    indices: Any


def topk(query, candidates, k, *, exclude=None, block=None) -> TopK:
    """The k best candidates of every query, scores = query @ candidates.T, without the [N, M] score matrix.

    query [N, E], candidates [M, E] and block are as for ``target_ranks``: the same exact-f32 GEMM call per block,
    so a score here has the bits the rank kernels compare (``indices[:, 0]`` is ``RankResult.top1``, and a
    target with ``greater + equal < k`` is in the list).  1 <= k <= 256.  exclude: int64 [N], a candidate index
    per query that never enters its list (the positive, for hard-negative mining); values outside [0, M)
    exclude nothing.  The order is total (ties go to the lower index; -0.0 == +0.0; scores are expected to be
    finite, a NaN is ordered and reported as -inf), so the result does not depend on ``block`` beyond the bits of
    the GEMM output.

    One pass over the blocks, each merged into the running lists by clipmi_topk_merge; memory is one
    block x block fp32 scratch plus the two [N, k] outputs; no host synchronisation."""
    k = int(k)
    if not 1 <= k <= TOPK_MAX:
        raise ValueError(f"topk: k must be in [1, {TOPK_MAX}], got {k}")
    ex = _exclude_rows("topk", exclude, query.shape[0], query.device) if query.dim() == 2 else None
    q, c = _score_operands("topk", query, candidates)
    walk = _TopKWalk(q.shape[0], c.shape[0], q.device, k, ex)
    _block_walk(q, c, _block_size("topk", block), [walk])
    return walk.res


_topk = topk  # evaluate_retrieval's `topk` keyword shadows the function


# ------------------------------------------------------------------------------ group-aware retrieval
@dataclass
class GroupRankResult:
    """Per-query outputs of ``group_ranks`` (device tensors, length N).  The positives of query i are the
    candidates that carry its key (but the excluded one).  ``n_pos`` = how many; ``pos_idx`` / ``pos_score`` = the
    best of them (highest score, lowest index on equal scores; -1 / -inf when there is none); ``greater`` /
    ``equal`` = #{negatives j: s[j] > / == pos_score} (-1 when there is no positive); ``top1`` / ``top1_score`` =
    argmax / max of s over the non-excluded candidates (lowest index on ties)."""
    greater: Any
    equal: Any
    n_pos: Any
    pos_idx: Any = None
    pos_score: Any = None
    top1: Any = None
    top1_score: Any = None


def _host_keys(who, name, keys, n):
    """Keys as ``losses.as_pair_keys`` takes them (an int32 / int64 tensor or a sequence of ints, of length n),
    checked on the host before anything runs: -> an int64 tensor, wherever it lives."""
    if isinstance(keys, torch.Tensor):
        if keys.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{who}: {name} must be an int32 or int64 tensor, got {keys.dtype}")
        k = keys.detach()
    else:
        vals = list(keys)
        if not all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in vals):
            raise ValueError(f"{who}: {name} must be an int32 / int64 tensor or a sequence of ints")
        k = torch.tensor([int(v) for v in vals], dtype=torch.int64)
    if k.dim() != 1 or k.shape[0] != n:
        raise ValueError(f"{who}: {name} must have length {n} (one key per row), got shape {tuple(k.shape)}")
    return k


def _device_keys(k, dev):
    return k.to(device=dev, dtype=torch.int64, non_blocking=True).contiguous()


class _RankWalk:
    """The diagonal / target ranks (clipmi_rank_pick, clipmi_rank_count) as a consumer of ``_block_walk``."""

    def __init__(self, N, M, dev, tgt=None):
        self.N, self.M, self.tgt = N, M, tgt
        self.res = RankResult(greater=torch.empty(N, dtype=torch.int32, device=dev),
                              equal=torch.empty(N, dtype=torch.int32, device=dev),
                              top1=torch.empty(N, dtype=torch.int32, device=dev),
                              top1_score=torch.empty(N, dtype=torch.float32, device=dev),
                              target_score=torch.empty(N, dtype=torch.float32, device=dev),
                              bad=torch.zeros(1, dtype=torch.int32, device=dev))

    def wants(self, r0, rows, c0, cols):
        return self.tgt is not None or not (c0 >= r0 + rows or c0 + cols <= r0)  # paired: the diagonal blocks

    def first_pass(self, s, sbuf, r0, rows, c0, cols, first):
        call("clipmi_rank_pick", s, P_(sbuf), cols, self.N, self.M, r0, rows, c0, cols, P_(self.tgt),
             P_(self.res.target_score), P_(self.res.bad))

    def second_pass(self, s, sbuf, r0, rows, c0, cols, first):
        r = self.res
        call("clipmi_rank_count", s, P_(sbuf), cols, self.N, self.M, r0, rows, c0, cols, P_(self.tgt),
             P_(r.target_score), first, P_(r.greater), P_(r.equal), P_(r.top1), P_(r.top1_score))


class _GroupWalk:
    """The keyed ranks (clipmi_group_pick, clipmi_group_count) as a consumer of ``_block_walk``."""

    def __init__(self, N, M, dev, qk, ck, ex=None):
        self.N, self.M, self.qk, self.ck, self.ex = N, M, qk, ck, ex
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.res = GroupRankResult(greater=torch.empty(N, **i32), equal=torch.empty(N, **i32),
                                   n_pos=torch.empty(N, **i32), pos_idx=torch.empty(N, **i32),
                                   pos_score=torch.empty(N, **f32), top1=torch.empty(N, **i32),
                                   top1_score=torch.empty(N, **f32))

    def wants(self, r0, rows, c0, cols):
        return True

    def first_pass(self, s, sbuf, r0, rows, c0, cols, first):
        r = self.res
        call("clipmi_group_pick", s, P_(sbuf), cols, self.N, self.M, r0, rows, c0, cols, P_(self.qk), P_(self.ck),
             P_(self.ex), first, P_(r.pos_score), P_(r.pos_idx), P_(r.n_pos))

    def second_pass(self, s, sbuf, r0, rows, c0, cols, first):
        r = self.res
        call("clipmi_group_count", s, P_(sbuf), cols, self.N, self.M, r0, rows, c0, cols, P_(self.qk), P_(self.ck),
             P_(self.ex), P_(r.pos_score), P_(r.n_pos), first, P_(r.greater), P_(r.equal), P_(r.top1),
             P_(r.top1_score))


class _TopKWalk:
    """The top-k lists (clipmi_topk_merge) as a consumer of ``_block_walk``: the second pass alone."""

    def __init__(self, N, M, dev, k, ex=None):
        self.N, self.M, self.k, self.ex = N, M, k, ex
        self.res = TopK(scores=torch.empty(N, k, dtype=torch.float32, device=dev),
                        indices=torch.empty(N, k, dtype=torch.int32, device=dev))

    first_pass = None

    def second_pass(self, s, sbuf, r0, rows, c0, cols, first):
        call("clipmi_topk_merge", s, P_(sbuf), cols, self.N, self.M, r0, rows, c0, cols, self.k, first, P_(self.ex),
             P_(self.res.scores), P_(self.res.indices))


def _block_walk(q, c, blk, consumers):
    """The block walk every retrieval entry point rides: each ``blk x blk`` score block of q @ c.T is computed once
    per pass by the exact-f32 GEMM (this function holds the file's one call of it and its one scratch, of one
    block) and handed to every consumer.  Per row range, pass 1 (the picks) visits the column blocks some consumer
    wants (paired ranks: those that overlap the row range; a walk without picks, ``topk``'s, has no pass 1), pass 2
    (the counts and the top-k merge) all of them; a block that is still in the scratch from pass 1 (a single column
    block) is not computed again.  So the walk costs at most 2 x (row blocks x column blocks) GEMMs however many
    consumers ride on it, and every consumer sees the score bits it sees alone."""
    (N, E), M = q.shape, c.shape[0]
    sbuf = torch.empty(min(blk, N) * min(blk, M), dtype=torch.float32, device=q.device)
    s = T.K.stream()

    def scores(r0, rows, c0, cols):
        T._gemm_f32(rows, cols, E, q[r0:], E, True, c[c0:], E, True, sbuf, cols)

    cblocks = [(c0, min(blk, M - c0)) for c0 in range(0, M, blk)]
    pickers = [u for u in consumers if u.first_pass is not None]
    for r0 in range(0, N, blk):
        rows = min(blk, N - r0)
        held = None  # the column block the scratch holds
        for n, (c0, cols) in enumerate(cblocks):
            users = [u for u in pickers if u.wants(r0, rows, c0, cols)]
            if not users:
                continue
            scores(r0, rows, c0, cols)
            held = c0
            for u in users:
                u.first_pass(s, sbuf, r0, rows, c0, cols, 1 if n == 0 else 0)
        for n, (c0, cols) in enumerate(cblocks):
            if held != c0 or len(cblocks) > 1:
                scores(r0, rows, c0, cols)
            for u in consumers:
                u.second_pass(s, sbuf, r0, rows, c0, cols, 1 if n == 0 else 0)


def group_ranks(query, candidates, query_keys, candidate_keys, *, exclude=None, block=None) -> GroupRankResult:
    """Rank statistics of each query's best positive among all candidates, scores = query @ candidates.T, where
    the positives of query i are the candidates j with ``candidate_keys[j] == query_keys[i]``: the evaluation
    counterpart of the multi-positive loss (``pair_keys`` / ``positives=``).

    query [N, E], candidates [M, E] and block are as for ``target_ranks``.  query_keys / candidate_keys: what
    ``losses.as_pair_keys`` takes (an int32 / int64 tensor or a sequence of ints), of length N / M, compared as
    64-bit values.  exclude: int64 [N], a candidate per query that is neither positive nor negative nor top1 (pass
    ``arange(N)`` when queries and candidates are one set); values outside [0, M) exclude nothing.

    Two walks per row range with the identical GEMM call per block, as ``target_ranks``: the first keeps the
    best positive and counts the positives, the second counts the negatives against it, so a negative that is a
    bit-equal duplicate of the best positive lands in ``equal``, never in ``greater``.  With all keys distinct and
    paired data the result is ``target_ranks(query, candidates)``'s, bit for bit.  Memory is one block x block
    scratch plus seven length-N outputs; no host synchronisation."""
    N = query.shape[0] if query.dim() == 2 else -1
    M = candidates.shape[0] if candidates.dim() == 2 else -1
    qk = ck = ex = None
    if N >= 0 and M >= 0:
        qk = _host_keys("group_ranks", "query_keys", query_keys, N)
        ck = _host_keys("group_ranks", "candidate_keys", candidate_keys, M)
        ex = _exclude_rows("group_ranks", exclude, N, query.device)
    q, c = _score_operands("group_ranks", query, candidates)
    dev = q.device
    blk = _block_size("group_ranks", block)
    walk = _GroupWalk(N, M, dev, _device_keys(qk, dev), _device_keys(ck, dev), ex)
    _block_walk(q, c, blk, [walk])
    return walk.res


def topk_relevance(top, query_keys, candidate_keys):
    """hits int32 [N, k] (device): ``hits[i, r]`` = how many of query i's r + 1 best candidates carry its key.

    top: the ``TopK`` of ``topk`` (or its ``indices``, int32 [N, k] on the GPU; -1 = an empty slot, no hit);
    the keys are as for ``group_ranks``, of length N and of the number of candidates the lists index.
    ``precision_at_k`` and ``average_precision_at_k`` read the result; no host synchronisation."""
    idx = top.indices if isinstance(top, TopK) else top
    if not isinstance(idx, torch.Tensor) or idx.dim() != 2 or idx.dtype != torch.int32:
        raise ValueError("topk_relevance: top must be a TopK or an int32 [N, k] tensor of candidate indices")
    N, k = idx.shape
    if N <= 0 or not 1 <= k <= TOPK_MAX:
        raise ValueError(f"topk_relevance: top must be [N >= 1, 1 <= k <= {TOPK_MAX}], got {tuple(idx.shape)}")
    qk = _host_keys("topk_relevance", "query_keys", query_keys, N)
    if not isinstance(candidate_keys, torch.Tensor):
        candidate_keys = list(candidate_keys)
    elif candidate_keys.dim() != 1:
        raise ValueError("topk_relevance: candidate_keys must be one-dimensional")
    M = len(candidate_keys)
    ck = _host_keys("topk_relevance", "candidate_keys", candidate_keys, M)
    if M <= 0:
        raise ValueError("topk_relevance: no candidate keys")
    if not idx.is_cuda:
        raise ValueError("topk_relevance needs GPU tensors (no CPU fallback)")
    dev = idx.device
    idx = idx.detach().contiguous()
    qk, ck = _device_keys(qk, dev), _device_keys(ck, dev)
    hits = torch.empty(N, k, dtype=torch.int32, device=dev)
    call("clipmi_topk_hits", T.K.stream(), P_(idx), N, k, ck.shape[0], P_(qk), P_(ck), P_(hits))
    return hits


def _hits2d(who, hits):
    h = torch.as_tensor(hits)
    if h.dim() != 2 or h.shape[1] < 1 or h.dtype.is_floating_point:
        raise ValueError(f"{who}: hits must be an integer [N, k] tensor, got {tuple(h.shape)} {h.dtype}")
    return h


def precision_at_k(hits, ks=(1, 5, 10)):
    """{k: mean over the queries of hits[:, k - 1] / k}: the share of the k best candidates that are positives
    (``hits`` from ``topk_relevance``; every k must be within the lists' length).  float64 on the device of
    ``hits``; one transfer for the result."""
    h = _hits2d("precision_at_k", hits)
    ks = [int(k) for k in ks]
    for k in ks:
        if not 1 <= k <= h.shape[1]:
            raise ValueError(f"precision_at_k: k must be in [1, {h.shape[1]}], got {k}")
    if not ks:
        return {}
    cols = torch.tensor([k - 1 for k in ks], device=h.device)
    mean = h.index_select(1, cols).to(torch.float64).mean(0) / torch.tensor(ks, device=h.device, dtype=torch.float64)
    return {k: float(v) for k, v in zip(ks, mean.cpu().tolist())}


def average_precision_at_k(hits, n_pos):
    """Mean over the queries with ``n_pos > 0`` of AP@k_i = (1 / min(n_pos_i, k)) * sum_r rel_ir * hits_ir / (r + 1),
    rel = the differences of ``hits`` along a list (1 where position r holds a positive), k = the lists' length,
    ``n_pos`` = the number of positives that exist (``GroupRankResult.n_pos``).  float64 on the device of ``hits``;
    nan when no query has a positive."""
    h = _hits2d("average_precision_at_k", hits)
    n = torch.as_tensor(n_pos).to(h.device)
    if n.shape != (h.shape[0],) or n.dtype.is_floating_point:
        raise ValueError(f"average_precision_at_k: n_pos must be an integer tensor of shape ({h.shape[0]},), got "
                         f"{tuple(n.shape)} {n.dtype}")
    k = h.shape[1]
    h64 = h.to(torch.float64)
    rel = torch.diff(h64, dim=1, prepend=torch.zeros(h.shape[0], 1, dtype=torch.float64, device=h.device))
    pos = torch.arange(1, k + 1, dtype=torch.float64, device=h.device)
    has = n > 0
    ap = (rel * h64 / pos).sum(1) / n.clamp(1, k).to(torch.float64)
    cnt = has.sum()
    return float((torch.where(has, ap, torch.zeros_like(ap)).sum() / cnt).item())


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _ranks(result, ties):
    """1-based ranks (int64 numpy) under a tie policy; a device-resident result is checked and copied here.  A
    result with ``n_pos`` (``GroupRankResult``) gives the ranks of its rows with a positive only."""
    if ties not in ("optimistic", "pessimistic"):
        raise ValueError(f"ties must be 'optimistic' or 'pessimistic', got {ties!r}")
    if isinstance(result, RankResult):
        result.check()
    rank = _host(result.greater).astype(np.int64) + 1
    if ties == "pessimistic":
        rank = rank + _host(result.equal).astype(np.int64)
    n_pos = getattr(result, "n_pos", None)
    if n_pos is not None:
        rank = rank[_host(n_pos) > 0]
    return rank


def recall_at_k(result, ks=(1, 5, 10), ties="optimistic"):
    """{k: fraction of queries whose target ranks within the top k}.

    ``optimistic`` rank = greater + 1 (the target wins every tie); ``pessimistic`` rank = greater + equal + 1.
    Optimistic is the default because this project's data repeats captions (35 captions over thousands of
    images, dataset.py:13-63): the candidates then hold exact duplicates of the positive, every duplicate
    scores bit-equal to it, and retrieving any of them is a correct retrieval.  Counting them against the
    positive would cap R@1 near 35 / N whatever the model does.  Ties between distinct candidates are
    measure-zero in fp32 cosines, so the two policies differ by the duplicates alone."""
    rank = _ranks(result, ties)
    return {int(k): float(np.mean(rank <= int(k))) for k in ks}


def rank_summary(result, ties="optimistic"):
    """{"median_rank", "mean_rank"}: 1-based, under the same tie policies as ``recall_at_k``."""
    rank = _ranks(result, ties)
    return {"median_rank": float(np.median(rank)), "mean_rank": float(np.mean(rank))}


class _Rows:
    """A growing [n, ...] device buffer: preallocated when the total is known, doubled on demand otherwise."""

    def __init__(self, tail, dtype, device, capacity):
        self.buf = torch.empty((max(int(capacity), 1),) + tuple(tail), dtype=dtype, device=device)
        self.n = 0

    def take(self, b):
        """-> the next b rows (a contiguous view to write into)."""
        need = self.n + b
        if need > self.buf.shape[0]:
            grown = torch.empty((max(2 * self.buf.shape[0], need),) + tuple(self.buf.shape[1:]),
                                dtype=self.buf.dtype, device=self.buf.device)
            grown[:self.n].copy_(self.buf[:self.n])
            self.buf = grown
        view = self.buf[self.n:need]
        self.n = need
        return view

    def rows(self):
        return self.buf[:self.n]


def _dataset_len(loader):
    try:
        return len(loader.dataset)
    except (AttributeError, TypeError):
        return 0


def evaluate_retrieval(model, dataloader, ks=(1, 5, 10), block=None, topk=0, keys=None):
    """Image->text and text->image retrieval of a ``CLIPWithAdapters`` over a whole dataloader.

    Eval mode under no_grad; per batch ``model(..., return_loss=False)``, features L2-normalised by
    clipmi_l2norm_fwd into device buffers (sized from ``len(dataloader.dataset)`` when there is one); nothing
    inside the loop synchronises with the host.  Pair i is (image i, caption i).  Returns ``n``,
    ``i2t_R@k`` / ``t2i_R@k`` for k in ks, ``{i2t,t2i}_median_rank``, ``{i2t,t2i}_mean_rank`` (optimistic
    ties, see ``recall_at_k``) and the two ``RankResult``s under ``i2t`` / ``t2i``.  With topk > 0 the result
    also carries the ``topk`` best captions of every image and images of every caption as ``TopK`` objects under
    ``i2t_topk`` / ``t2i_topk``; with the default it has exactly the keys above.  The model's train / eval mode is
    restored.

    keys: what the trainer's ``positives`` takes (``losses.batch_keys``: "caption", a batch field name such as
    "emotion", or a callable on the batch), resolved per batch into 64-bit pair keys kept on the device next to the
    features; captions are hashed on the device.  Every pair that shares pair i's key is then a correct retrieval
    for it, as in the multi-positive loss, and the result gains, for both directions, ``{i2t,t2i}_gR@k``,
    ``_g_median_rank`` / ``_g_mean_rank`` (the rank of the best positive among the negatives, optimistic ties)
    and the ``GroupRankResult``s under ``i2t_group`` / ``t2i_group``; with topk > 0 also ``_P@k`` for every k in ks
    with k <= topk and ``_mAP@{topk}`` (``precision_at_k``, ``average_precision_at_k``).  The diagonal metrics
    above are unchanged.  With keys, a direction's diagonal ranks, keyed ranks and top-k lists ride on one shared
    walk: every score block is computed at most twice, not five times.  With keys=None nothing changes."""
    from .losses import batch_keys
    topk = int(topk)
    if topk < 0 or topk > TOPK_MAX:
        raise ValueError(f"evaluate_retrieval: topk must be in [0, {TOPK_MAX}], got {topk}")
    was_training = model.training
    device = model.clip.arena.device
    total = _dataset_len(dataloader)
    txt = img = kbuf = None
    model.eval()
    try:
        with torch.no_grad():
            for batch in dataloader:
                batch = {k: v.to(device, non_blocking=True) if isinstance(v, torch.Tensor) else v
                         for k, v in batch.items()}
                out = model(input_ids=batch.get("input_ids"), attention_mask=batch.get("attention_mask"),
                            pixel_values=batch.get("pixel_values"), return_loss=False)
                tf, imf = out["text_features"], out["image_features"]
                if tf is None or imf is None:
                    raise ValueError("evaluate_retrieval: every batch needs input_ids and pixel_values")
                if txt is None:
                    txt = _Rows((tf.shape[1],), torch.float32, device, total)
                    img = _Rows((imf.shape[1],), torch.float32, device, total)
                l2_normalize(tf, out=txt.take(tf.shape[0]))
                l2_normalize(imf, out=img.take(imf.shape[0]))
                if keys is not None:
                    bk = _host_keys("evaluate_retrieval", "the batch's keys", batch_keys(batch, keys, device),
                                    tf.shape[0])
                    if kbuf is None:
                        kbuf = _Rows((), torch.int64, device, total)
                    kbuf.take(tf.shape[0]).copy_(bk, non_blocking=True)
            if txt is None:
                raise ValueError("evaluate_retrieval: the dataloader is empty")
            group, hits = {}, {}
            if keys is None:
                i2t = target_ranks(img.rows(), txt.rows(), None, block=block)
                t2i = target_ranks(txt.rows(), img.rows(), None, block=block)
                if topk:
                    i2t_top = _topk(img.rows(), txt.rows(), topk, block=block)
                    t2i_top = _topk(txt.rows(), img.rows(), topk, block=block)
            else:
                i2t, group["i2t"], i2t_top = _keyed_walk(img.rows(), txt.rows(), kbuf.rows(), topk, block)
                t2i, group["t2i"], t2i_top = _keyed_walk(txt.rows(), img.rows(), kbuf.rows(), topk, block)
                if topk:
                    hits["i2t"] = topk_relevance(i2t_top, kbuf.rows(), kbuf.rows())
                    hits["t2i"] = topk_relevance(t2i_top, kbuf.rows(), kbuf.rows())
    finally:
        model.train(was_training)
    res = {"n": txt.n}
    for name, r in (("i2t", i2t), ("t2i", t2i)):
        on_host = RankResult(greater=_host(r.check().greater), equal=None)  # optimistic ties read `greater` alone
        for k, v in recall_at_k(on_host, ks).items():
            res[f"{name}_R@{k}"] = v
        for k, v in rank_summary(on_host).items():
            res[f"{name}_{k}"] = v
    for name, g in group.items():
        on_host = GroupRankResult(greater=_host(g.greater), equal=None, n_pos=_host(g.n_pos))
        for k, v in recall_at_k(on_host, ks).items():
            res[f"{name}_gR@{k}"] = v
        for k, v in rank_summary(on_host).items():
            res[f"{name}_g_{k}"] = v
    for name, h in hits.items():
        for k, v in precision_at_k(h, [k for k in ks if int(k) <= topk]).items():
            res[f"{name}_P@{k}"] = v
        res[f"{name}_mAP@{topk}"] = average_precision_at_k(h, group[name].n_pos)
    res["i2t"], res["t2i"] = i2t, t2i
    if topk:
        res["i2t_topk"], res["t2i_topk"] = i2t_top, t2i_top
    for name, g in group.items():
        res[f"{name}_group"] = g
    return res


def _keyed_walk(q, c, keys, topk, block):
    """The diagonal ranks, the keyed ranks and (topk > 0) the top-k lists of paired features over one shared
    walk: -> (RankResult, GroupRankResult, TopK or None), each bit for bit what its own function returns."""
    q, c = _score_operands("evaluate_retrieval", q, c)
    (N, _), M, dev = q.shape, c.shape[0], q.device
    users = [_RankWalk(N, M, dev), _GroupWalk(N, M, dev, keys, keys)]
    if topk:
        users.append(_TopKWalk(N, M, dev, topk))
    _block_walk(q, c, _block_size("evaluate_retrieval", block), users)
    return users[0].res, users[1].res, users[2].res if topk else None


# ------------------------------------------------------------------------------ classification
@dataclass
class ClassificationResult:
    """Host copies (numpy) of a ``ClassificationMeter``: confusion int64 [C, C] (rows = true class), preds
    int64 [n], confidences float32 [n], labels int64 [n], probs float32 [n, C]."""
    confusion: np.ndarray
    preds: np.ndarray
    confidences: np.ndarray
    labels: np.ndarray
    probs: np.ndarray


class ClassificationMeter:
    """Device-resident tallies of a classification run: per batch ``update(probs, labels)`` takes the row
    argmax (lowest index on ties) and its probability, exactly ``torch.max(probs, 1)``, and adds the batch into
    the [C, C] confusion matrix, all in clipmi_classify_accumulate without a host synchronisation;
    ``result()`` makes one transfer."""

    def __init__(self, num_classes, capacity=0):
        if int(num_classes) <= 0:
            raise ValueError("ClassificationMeter: num_classes must be positive")
        self.C = int(num_classes)
        self._capacity = int(capacity)
        self.confusion = None

    def _alloc(self, device):
        C, cap = self.C, self._capacity
        self.confusion = torch.zeros(C, C, dtype=torch.int64, device=device)
        self.bad = torch.zeros(1, dtype=torch.int32, device=device)
        self.pred = _Rows((), torch.int32, device, cap)
        self.conf = _Rows((), torch.float32, device, cap)
        self.label = _Rows((), torch.int64, device, cap)
        self.probs = _Rows((C,), torch.float32, device, cap)

    @property
    def n(self):
        return 0 if self.confusion is None else self.pred.n

    def update(self, probs, labels):
        if probs.dim() != 2 or probs.shape[1] != self.C:
            raise ValueError(f"ClassificationMeter: probs must be [B, {self.C}], got {tuple(probs.shape)}")
        if not probs.is_cuda:
            raise ValueError("ClassificationMeter needs GPU probabilities (no CPU fallback)")
        B = probs.shape[0]
        labels = torch.as_tensor(labels)
        if labels.shape != (B,):
            raise ValueError(f"ClassificationMeter: labels must have shape ({B},), got {tuple(labels.shape)}")
        if B == 0:
            return
        if self.confusion is None:
            self._alloc(probs.device)
        p, lab = self.probs.take(B), self.label.take(B)
        p.copy_(probs.detach())
        lab.copy_(labels.detach(), non_blocking=True)
        call("clipmi_classify_accumulate", T.K.stream(), P_(p), P_(lab), B, self.C, P_(self.pred.take(B)),
             P_(self.conf.take(B)), P_(self.confusion), P_(self.bad))

    def result(self) -> ClassificationResult:
        """One device-to-host transfer of everything; IndexError if a label was outside [0, C)."""
        C = self.C
        if self.confusion is None:
            return ClassificationResult(np.zeros((C, C), np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32),
                                        np.zeros(0, np.int64), np.zeros((0, C), np.float32))
        n = self.pred.n
        parts = [self.confusion, self.label.rows(), self.bad, self.pred.rows(), self.conf.rows(), self.probs.rows()]
        blob = torch.cat([t.reshape(-1).view(torch.uint8) for t in parts]).cpu().numpy()
        out, off = [], 0
        for t, dtype in zip(parts, (np.int64, np.int64, np.int32, np.int32, np.float32, np.float32)):
            out.append(np.frombuffer(blob, dtype=dtype, count=t.numel(), offset=off).copy())
            off += t.numel() * t.element_size()
        conf_matrix, lab, bad, pred, conf, probs = out
        if int(bad[0]):
            raise IndexError(f"ClassificationMeter: a label is out of range [0, {C})")
        return ClassificationResult(conf_matrix.reshape(C, C), pred.astype(np.int64), conf, lab, probs.reshape(n, C))


def accuracy(confusion):
    """Fraction of samples on the diagonal (sklearn accuracy_score of the same labels and predictions)."""
    cm = np.asarray(confusion, dtype=np.int64)
    total = int(cm.sum())
    return float(np.trace(cm)) / total if total else 0.0


def _div(num, den):
    """num / den with zero_division=0."""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.divide(num, den, out=np.zeros_like(num), where=den != 0)


def classification_report(confusion, target_names, digits=4):
    """sklearn.metrics.classification_report(labels, preds, target_names=..., digits=..., zero_division=0) as a
    string, computed from the confusion matrix (rows = true class) over all C classes: per class precision,
    recall, f1-score and support, then accuracy, macro avg and weighted avg."""
    cm = np.asarray(confusion, dtype=np.int64)
    C = cm.shape[0]
    if cm.shape != (C, C) or len(target_names) != C:
        raise ValueError(f"classification_report: a [C, C] confusion matrix and C names, got {cm.shape} and "
                         f"{len(target_names)}")
    tp = np.diag(cm).astype(np.float64)
    support = cm.sum(1)
    pred_sum = cm.sum(0)
    p, r = _div(tp, pred_sum), _div(tp, support)
    f1 = _div(2 * tp, support + pred_sum)
    total = int(support.sum())
    headers = ["precision", "recall", "f1-score", "support"]
    width = max(max(len(str(n)) for n in target_names), len("weighted avg"), digits)
    report = ("{:>{width}s} " + " {:>9}" * len(headers)).format("", *headers, width=width) + "\n\n"
    row_fmt = "{:>{width}s} " + " {:>9.{digits}f}" * 3 + " {:>9}\n"
    for row in zip(target_names, p, r, f1, support):
        report += row_fmt.format(str(row[0]), *row[1:], width=width, digits=digits)
    report += "\n"
    report += ("{:>{width}s} " + " {:>9.{digits}}" * 2 + " {:>9.{digits}f}" + " {:>9}\n").format(
        "accuracy", "", "", accuracy(cm), total, width=width, digits=digits)
    report += row_fmt.format("macro avg", p.mean(), r.mean(), f1.mean(), total, width=width, digits=digits)
    w = _div(support, total)
    report += row_fmt.format("weighted avg", (p * w).sum(), (r * w).sum(), (f1 * w).sum(), total, width=width,
                             digits=digits)
    return report


def _cuda():
    return torch.device("cuda", torch.cuda.current_device())


def _eval_mode(*mods):
    for m in mods:
        if m is not None and hasattr(m, "eval"):
            m.eval()


def _finish(meter, target_names):
    r = meter.result()
    return (accuracy(r.confusion), r.confusion, classification_report(r.confusion, target_names, digits=4),
            list(r.preds), list(r.labels), list(r.confidences), r.probs)


def evaluate_model(model, test_loader, use_all_descriptions=False):
    """evaluation.evaluate_model (evaluation.py:17-68) for ``heads.CLIPAdapter`` /
    ``heads.ZeroShotEmotionRecognition``: the same 8-tuple (accuracy, conf_matrix, class_report, all_preds,
    all_labels, all_image_paths, all_confidences, all_similarity_scores) over ``predict`` or
    ``predict_with_all_descriptions``.  The loader yields (pixel_values, labels, img_paths).  The report's class
    names are the model's description keys (constants.EMOTIONS order, see heads.py), else constants.EMOTIONS."""
    _eval_mode(getattr(model, "model", None), getattr(model, "visual_adapter", None),
               getattr(model, "text_adapter", None))
    descs = getattr(model, "emotion_descriptions", None)
    target_names = list(descs.keys()) if descs else EMOTIONS
    meter, paths = None, []
    with torch.no_grad():
        for pixel_values, labels, img_paths in test_loader:
            pixel_values = pixel_values.to(_cuda(), non_blocking=True)
            if use_all_descriptions and hasattr(model, "predict_with_all_descriptions"):
                probs = model.predict_with_all_descriptions(pixel_values)
            else:
                probs = model.predict(pixel_values)
            if meter is None:
                meter = ClassificationMeter(probs.shape[1], _dataset_len(test_loader))
            meter.update(probs, labels)
            if img_paths is not None:
                paths.extend(img_paths)
    if meter is None:
        raise ValueError("evaluate_model: the loader is empty")
    acc, cm, report, preds, labs, confs, probs = _finish(meter, target_names)
    return acc, cm, report, preds, labs, paths, confs, probs


def evaluate_enhanced_model(model, test_loader, emotions=EMOTIONS):
    """utils.evaluate_enhanced_model (utils.py:24-68) for ``heads.EnhancedCLIPAdapter``: the same 9-tuple
    (accuracy, conf_matrix, class_report, all_preds, all_labels, all_image_paths, all_confidences,
    all_similarity_scores, all_contexts_text) over ``predict_probs``.  The loader yields (pixel_values, labels,
    img_paths, context_features, contexts_text)."""
    model.eval()
    C = len(emotions)
    meter = ClassificationMeter(C, _dataset_len(test_loader))
    paths, contexts = [], []
    with torch.no_grad():
        for pixel_values, labels, img_paths, context_features, contexts_text in test_loader:
            dev = _cuda()
            pixel_values = pixel_values.to(dev, non_blocking=True)
            if isinstance(context_features, list):
                context_features = torch.stack(context_features)
            if context_features is not None:
                context_features = context_features.to(dev, non_blocking=True)
            meter.update(model.predict_probs(pixel_values, context_features), labels)
            if img_paths is not None:
                paths.extend(img_paths)
            if contexts_text is not None:
                contexts.extend(contexts_text)
    if meter.n == 0:  # utils.py:58-62 on an empty loader
        return 0.0, np.zeros((C, C)), "No data to report.", [], [], paths, [], np.array([]), contexts
    acc, cm, report, preds, labs, confs, probs = _finish(meter, list(emotions))
    return acc, cm, report, preds, labs, paths, confs, probs, contexts


# ------------------------------------------------------------------------------ multi-label classification
def _binary_u8(targets):
    """Targets as the kernels read them: uint8 with 1 / 0 where the value is exactly 1 / 0 and 2 (which sets
    ``bad``) anywhere else, so a soft label or a NaN is reported instead of truncated."""
    t = targets.detach()
    two = torch.full((), 2, dtype=torch.uint8, device=t.device)
    return torch.where(t == 1, torch.ones_like(two), torch.where(t == 0, torch.zeros_like(two), two))


def _ap_counts(scores_cm, targets_cm):
    """clipmi_ap_count on class-major device tensors (fp32 / uint8 [C, N], contiguous): -> (ge_all, ge_pos int32
    [C, N], n_pos int32 [C], bad int32 [1]), all on the device; no host synchronisation."""
    C, N = scores_cm.shape
    dev = scores_cm.device
    ge_all = torch.empty(C, N, dtype=torch.int32, device=dev)
    ge_pos = torch.empty_like(ge_all)
    n_pos = torch.empty(C, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    call("clipmi_ap_count", T.K.stream(), P_(scores_cm), P_(targets_cm), N, C, N, P_(ge_all), P_(ge_pos), P_(n_pos),
         P_(bad))
    return ge_all, ge_pos, n_pos, bad


def ap_from_counts(ge_all, ge_pos, n_pos):
    """AP per class from clipmi_ap_count's integers (host, class-major [C, N]): (1 / n_pos) * the sum over the
    positives, in index order and in float64, of ge_pos / ge_all; nan where a class has no positive."""
    ge_all = np.asarray(ge_all, np.int64)
    ge_pos = np.asarray(ge_pos, np.float64)
    n_pos = np.asarray(n_pos, np.int64)
    C = n_pos.shape[0]
    ratio = np.divide(ge_pos, ge_all, out=np.zeros(ge_pos.shape, np.float64), where=ge_all > 0)
    total = np.cumsum(ratio, axis=1)[:, -1] if ratio.shape[1] else np.zeros(C)  # cumsum: strictly in index order
    return np.divide(total, n_pos, out=np.full(C, np.nan), where=n_pos > 0)


def _nanmean(x):
    x = np.asarray(x, np.float64)
    keep = ~np.isnan(x)
    return float(x[keep].mean()) if keep.any() else float("nan")


def _to_host(parts, dtypes):
    """One device-to-host transfer of several tensors -> numpy copies, flat."""
    blob = torch.cat([t.reshape(-1).view(torch.uint8) for t in parts]).cpu().numpy()
    out, off = [], 0
    for t, dtype in zip(parts, dtypes):
        out.append(np.frombuffer(blob, dtype=dtype, count=t.numel(), offset=off).copy())
        off += t.numel() * t.element_size()
    return out


def _multilabel_operands(who, scores, targets):
    if scores.dim() != 2 or tuple(targets.shape) != tuple(scores.shape):
        raise ValueError(f"{who}: scores and targets must both be [N, C], got {tuple(scores.shape)} and "
                         f"{tuple(targets.shape)}")
    if not scores.is_cuda:
        raise ValueError(f"{who} needs GPU tensors (no CPU fallback)")
    if scores.shape[0] <= 0 or scores.shape[1] <= 0:
        raise ValueError(f"{who}: empty input")


def average_precision(scores, targets):
    """-> (ap float64 [C], n_pos int64 [C]) (numpy): per class ``sklearn.metrics.average_precision_score(targets[:,
    c], scores[:, c])`` of device tensors scores [N, C] (any float dtype, read as fp32; +-inf allowed) and targets
    [N, C] (0 / 1 in any dtype), ties included: one threshold per distinct score.  mAP = ``np.nanmean(ap)``.

    The O(N^2 C) comparisons run in clipmi_ap_count and yield integers (for each positive, how many samples and how
    many positives score at least as high), so the result does not depend on any summation order on the device;
    the host adds ``ge_pos / ge_all`` in float64 in index order.  One transfer.  Difference from sklearn: a class
    without positives gets ``nan`` and drops out of the mean, where sklearn returns 0.0 with a warning (its
    newer versions) and so pulls the mean down by a class that measures nothing.  A NaN score or a target other
    than 0 / 1 raises ValueError."""
    targets = torch.as_tensor(targets)
    _multilabel_operands("average_precision", scores, targets)
    dev = scores.device
    s = scores.detach().to(torch.float32).t().contiguous()
    t8 = _binary_u8(targets.to(dev)).t().contiguous()
    ge_all, ge_pos, n_pos, bad = _ap_counts(s, t8)
    C, N = s.shape
    ga, gp, npos, b = _to_host([ge_all, ge_pos, n_pos, bad], (np.int32,) * 4)
    if int(b[0]):
        raise ValueError("average_precision: a score is NaN or a target is not 0 / 1")
    return ap_from_counts(ga.reshape(C, N), gp.reshape(C, N), npos), npos.astype(np.int64)


@dataclass
class MultiLabelResult:
    """Host copies (numpy) of a ``MultiLabelMeter``.  counts int64 [C, 4] = (tp, fp, fn, tn) per class at the
    meter's thresholds; ap float64 [C] (nan for a class without positives) and mAP = nanmean(ap), threshold-free;
    precision / recall / f1 float64 [C] and support int64 [C] (= tp + fn), micro_f1, macro_f1, subset_accuracy
    (rows predicted exactly) and hamming_loss (wrong cells / all cells), all from the integer counts with
    zero_division=0; probs float32 [n, C], targets uint8 [n, C]."""
    n: int
    counts: np.ndarray
    exact_rows: int
    ap: np.ndarray
    mAP: float
    precision: np.ndarray
    recall: np.ndarray
    f1: np.ndarray
    support: np.ndarray
    micro_f1: float
    macro_f1: float
    subset_accuracy: float
    hamming_loss: float
    probs: Optional[np.ndarray] = None
    targets: Optional[np.ndarray] = None

    @classmethod
    def from_counts(cls, counts, exact_rows, n, ap, probs=None, targets=None):
        """The derived numbers from the integers: what sklearn's precision_recall_fscore_support (per class,
        average="micro" / "macro", zero_division=0), accuracy_score and hamming_loss give on the same
        thresholded predictions."""
        counts = np.asarray(counts, np.int64).reshape(-1, 4)
        C, n = counts.shape[0], int(n)
        tp, fp, fn = counts[:, 0], counts[:, 1], counts[:, 2]
        f1 = _div(2 * tp, 2 * tp + fp + fn)
        ap = np.asarray(ap, np.float64)
        return cls(n=n, counts=counts, exact_rows=int(exact_rows), ap=ap, mAP=_nanmean(ap),
                   precision=_div(tp, tp + fp), recall=_div(tp, tp + fn), f1=f1, support=tp + fn,
                   micro_f1=float(_div(2 * tp.sum(), 2 * tp.sum() + fp.sum() + fn.sum())),
                   macro_f1=float(f1.mean()) if C else 0.0,
                   subset_accuracy=float(_div(int(exact_rows), n)),
                   hamming_loss=float(_div(fp.sum() + fn.sum(), n * C)), probs=probs, targets=targets)


class MultiLabelMeter:
    """Device-resident tallies of a multi-label run, the sibling of ``ClassificationMeter``: per batch
    ``update(probs, targets)`` keeps the rows and adds pred = probs >= threshold into per-class (tp, fp, fn, tn)
    and the exact-row count (clipmi_multilabel_accumulate) without a host synchronisation; ``result()`` runs
    clipmi_ap_count over the kept rows and makes one transfer.  threshold: a float, or one per class."""

    def __init__(self, num_classes, capacity=0, threshold=0.5):
        if int(num_classes) <= 0:
            raise ValueError("MultiLabelMeter: num_classes must be positive")
        self.C = int(num_classes)
        self._capacity = int(capacity)
        thr = np.asarray(threshold, np.float32)
        if thr.shape not in ((), (self.C,)) or np.isnan(thr).any():
            raise ValueError(f"MultiLabelMeter: threshold must be a number or {self.C} numbers")
        self.threshold = np.broadcast_to(thr, (self.C,)).copy()
        self.counts = None

    def _alloc(self, device):
        C, cap = self.C, self._capacity
        self.counts = torch.zeros(C, 4, dtype=torch.int64, device=device)
        self.exact = torch.zeros(1, dtype=torch.int64, device=device)
        self.bad = torch.zeros(1, dtype=torch.int32, device=device)
        self.thr = torch.from_numpy(self.threshold).to(device)
        self.probs = _Rows((C,), torch.float32, device, cap)
        self.targets = _Rows((C,), torch.uint8, device, cap)

    @property
    def n(self):
        return 0 if self.counts is None else self.probs.n

    def update(self, probs, targets):
        if probs.dim() != 2 or probs.shape[1] != self.C:
            raise ValueError(f"MultiLabelMeter: probs must be [B, {self.C}], got {tuple(probs.shape)}")
        if not probs.is_cuda:
            raise ValueError("MultiLabelMeter needs GPU probabilities (no CPU fallback)")
        B = probs.shape[0]
        targets = torch.as_tensor(targets)
        if tuple(targets.shape) != (B, self.C):
            raise ValueError(f"MultiLabelMeter: targets must have shape ({B}, {self.C}), got {tuple(targets.shape)}")
        if B == 0:
            return
        if self.counts is None:
            self._alloc(probs.device)
        p, t = self.probs.take(B), self.targets.take(B)
        p.copy_(probs.detach())
        t.copy_(_binary_u8(targets.to(probs.device, non_blocking=True)))
        call("clipmi_multilabel_accumulate", T.K.stream(), P_(p), P_(t), B, self.C, P_(self.thr), P_(self.counts),
             P_(self.exact), P_(self.bad))

    def result(self) -> MultiLabelResult:
        """One device-to-host transfer of everything; ValueError if a target was not 0 / 1 or a probability NaN."""
        C = self.C
        if self.counts is None:
            return MultiLabelResult.from_counts(np.zeros((C, 4), np.int64), 0, 0, np.full(C, np.nan),
                                                np.zeros((0, C), np.float32), np.zeros((0, C), np.uint8))
        n = self.probs.n
        ge_all, ge_pos, n_pos, ap_bad = _ap_counts(self.probs.rows().t().contiguous(),
                                                   self.targets.rows().t().contiguous())
        parts = [self.counts, self.exact, self.bad, ap_bad, n_pos, ge_all, ge_pos, self.probs.rows(),
                 self.targets.rows()]
        counts, exact, bad, ap_bad, n_pos, ge_all, ge_pos, probs, targets = _to_host(
            parts, (np.int64, np.int64, np.int32, np.int32, np.int32, np.int32, np.int32, np.float32, np.uint8))
        if int(bad[0]) or int(ap_bad[0]):
            raise ValueError("MultiLabelMeter: a target is not 0 / 1 or a probability is NaN")
        ap = ap_from_counts(ge_all.reshape(C, n), ge_pos.reshape(C, n), n_pos)
        return MultiLabelResult.from_counts(counts, exact[0], n, ap, probs.reshape(n, C), targets.reshape(n, C))


def evaluate_multilabel(model, loader, threshold=0.5, use_all_descriptions=False) -> MultiLabelResult:
    """``heads.MultiLabelCLIPAdapter`` over the reference's EMOTIC batches ``(context image, body crop, categorical
    [B, C], continuous)``: sigmoid probabilities from ``predict`` (or ``predict_with_all_descriptions``) into a
    ``MultiLabelMeter``; the body crop is passed on when the model was built with body=True, the continuous values
    are ignored.  Replaces the host loop of ``sklearn.metrics.average_precision_score`` per category."""
    _eval_mode(getattr(model, "model", None), getattr(model, "visual_adapter", None),
               getattr(model, "text_adapter", None), getattr(model, "body_adapter", None))
    meter = None
    with torch.no_grad():
        for context, body, categorical, _continuous in loader:
            dev = _cuda()
            context = context.to(dev, non_blocking=True)
            args = (context, body.to(dev, non_blocking=True)) if getattr(model, "body", False) else (context,)
            if use_all_descriptions and hasattr(model, "predict_with_all_descriptions"):
                probs = model.predict_with_all_descriptions(*args)
            else:
                probs = model.predict(*args)
            if meter is None:
                meter = MultiLabelMeter(probs.shape[1], _dataset_len(loader), threshold)
            meter.update(probs, categorical)
    if meter is None:
        raise ValueError("evaluate_multilabel: the loader is empty")
    return meter.result()
