"""float64 numpy references for the multi-label head and its metrics (csrc/multilabel.hip,
csrc/eval_multilabel.hip).  Nothing here uses the library, torch or sklearn; the tests compare them with those."""
import numpy as np


def sigmoid(z):
    z = np.asarray(z, np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bce_elements(z, y, pos_weight=None):
    """l[b, c] = (1 - y) z + (1 + (pw - 1) y) (log1p(exp(-|z|)) + max(-z, 0)): torch's BCEWithLogitsLoss terms."""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    pw = np.ones(z.shape[1]) if pos_weight is None else np.asarray(pos_weight, np.float64)
    return (1.0 - y) * z + (1.0 + (pw - 1.0) * y) * (np.log1p(np.exp(-np.abs(z))) + np.maximum(-z, 0.0))


def bce(z, y, pos_weight=None):
    """-> (loss_rows [B] = mean_c l, dscore [B, C] = d loss_rows / d z, l [B, C])."""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    C = z.shape[1]
    pw = np.ones(C) if pos_weight is None else np.asarray(pos_weight, np.float64)
    l = bce_elements(z, y, pw)
    p, q = sigmoid(z), sigmoid(-z)
    return l.mean(1), ((1.0 - y) * p - pw * y * q) / C, l


def ap_counts(scores, targets):
    """The O(N^2) definition on [N, C] arrays: for each positive (i, c), ge_all = #{j: s[j, c] >= s[i, c]} and
    ge_pos = the same over the positives j; 0 at the non-positives.  -> (ge_all, ge_pos int64 [N, C], n_pos [C])."""
    s, t = np.asarray(scores), np.asarray(targets) == 1
    N, C = s.shape
    ge_all, ge_pos = np.zeros((N, C), np.int64), np.zeros((N, C), np.int64)
    for c in range(C):
        pos = np.flatnonzero(t[:, c])
        if pos.size:
            ge = s[:, c][None, :] >= s[pos, c][:, None]  # [n_pos, N]
            ge_all[pos, c] = ge.sum(1)
            ge_pos[pos, c] = ge[:, pos].sum(1)
    return ge_all, ge_pos, t.sum(0).astype(np.int64)


def ap_from_counts(ge_all, ge_pos, n_pos):
    """The count identity: AP_c = (1 / n_pos) sum over the positives of ge_pos / ge_all; nan without positives."""
    C = ge_all.shape[1]
    ap = np.full(C, np.nan)
    for c in range(C):
        if n_pos[c]:
            m = ge_all[:, c] > 0
            ap[c] = float(np.sum(ge_pos[m, c].astype(np.float64) / ge_all[m, c])) / n_pos[c]
    return ap


def ap_sorted(scores, targets):
    """AP per class by the independent route (no counts): sort descending, one threshold per distinct score,
    AP = sum over the thresholds of (recall_k - recall_{k-1}) * precision_k; nan without positives."""
    s, t = np.asarray(scores, np.float64), (np.asarray(targets) == 1).astype(np.float64)
    N, C = s.shape
    ap = np.full(C, np.nan)
    for c in range(C):
        total = t[:, c].sum()
        if total == 0:
            continue
        order = np.argsort(-s[:, c], kind="stable")
        ss, tt = s[order, c], t[order, c]
        last = np.r_[np.flatnonzero(ss[1:] != ss[:-1]), N - 1]  # the last sample of each run of equal scores
        tp = np.cumsum(tt)[last]
        precision = tp / (last + 1.0)
        recall = tp / total
        ap[c] = float(np.sum(np.diff(np.r_[0.0, recall]) * precision))
    return ap


def thresholded_counts(probs, targets, thr=0.5):
    """-> (counts int64 [C, 4] = tp, fp, fn, tn of pred = probs >= thr, exact_rows)."""
    p, t = np.asarray(probs), np.asarray(targets) == 1
    pred = p >= np.broadcast_to(np.asarray(thr, np.float32), (p.shape[1],))[None, :]
    counts = np.stack([(pred & t).sum(0), (pred & ~t).sum(0), (~pred & t).sum(0), (~pred & ~t).sum(0)], 1)
    return counts.astype(np.int64), int((pred == t).all(1).sum())


def tie_heavy(N, C, levels, seed, inf=True):
    """Scores from {k / 4: k < levels} (float32) and about 10 % positives (uint8); with C >= 3 class 0 is all
    positive, class 1 has none and class 2 has all scores equal; a few +-inf when N allows."""
    rng = np.random.default_rng(seed)
    s = (rng.integers(0, levels, (N, C)) / 4.0).astype(np.float32)
    t = (rng.random((N, C)) < 0.1).astype(np.uint8)
    if inf and N >= 8:
        s[rng.integers(0, N, 3), rng.integers(0, C, 3)] = np.inf
        s[rng.integers(0, N, 3), rng.integers(0, C, 3)] = -np.inf
    if C >= 3:
        t[:, 0] = 1
        t[:, 1] = 0
        s[:, 2] = 0.75
    return s, t
