"""The yardstick of the RerankingEvaluator tests: what sentence-transformers 2.2.2 computes per query from the scores of its
candidate documents, restated in numpy the way upstream does it -- a sort and a walk over the first k for the reciprocal rank,
the average precision as sklearn's average_precision_score takes it (fp64, a sum over the distinct scores), NDCG@k from
the sorted list -- and the cases the host and the GPU test share. The one thing stated here rather than inherited is the
order of equal scores: upstream's torch.argsort(-scores) is not stable, so the sort here is numpy's stable one: among equal
scores the earlier document comes first.

Nothing here is shared with the code under test, which never sorts: it counts.
"""
import numpy as np

KINDS = ("gauss", "ties", "flat", "zeros", "pos_last", "pos_first")
SINGLE_SIZES = ((1, 1), (1, 62), (1, 63), (2, 63), (63, 1), (1, 256), (3, 1022), (1, 4999), (4999, 1), (700, 700))   # (P, N)
KS = (1, 10, 100000)
RR, AP, NDCG = range(3)


# ------------------------------------------------------------------ one group
def group_expected(s, P, k):
    """[rr, ap, ndcg] of one group in fp64: scores s, the first P documents its positives."""
    s = np.asarray(s, dtype=np.float64)
    n = len(s)
    relevant = np.arange(n) < P
    order = np.argsort(-s, kind="stable")
    rr = 0.0
    for rank, index in enumerate(order[:k]):            # upstream's walk
        if relevant[index]:
            rr = 1.0 / (rank + 1)
            break
    # sklearn: thresholds at the distinct scores from the top, sum of (recall - previous recall) * precision
    y = relevant[order].astype(np.float64)
    last_of_run = np.r_[np.flatnonzero(np.diff(s[order])), n - 1]
    tps = np.cumsum(y)[last_of_run]
    precision = tps / (1.0 + last_of_run)
    recall = tps / tps[-1]
    ap = float(np.sum(np.diff(np.r_[0.0, recall]) * precision))
    top = order[:k]
    dcg = float(np.sum(relevant[top] / np.log2(2.0 + np.arange(len(top)))))
    ideal = float(np.sum(1.0 / np.log2(2.0 + np.arange(min(P, k)))))
    return [rr, ap, dcg / ideal]


def expected(scores, offsets, num_pos, k):
    """float64 [nq, 3] = {rr, ap, ndcg} per group of the flat score array."""
    return np.array([group_expected(scores[offsets[g]:offsets[g + 1]], int(num_pos[g]), k) for g in range(len(num_pos))],
                    dtype=np.float64).reshape(len(num_pos), 3)


def upstream_rr(s, P, k):
    """The MRR term of upstream's compute_metrices_individual, its argsort made stable."""
    is_relevant = [True] * P + [False] * (len(s) - P)
    pred_scores_argsort = np.argsort(-np.asarray(s), kind="stable")
    for rank, index in enumerate(pred_scores_argsort[0:k]):
        if is_relevant[index]:
            return 1 / (rank + 1)
    return 0


def ap_bound(P):
    """|ap - yardstick| allowed: a sum of P terms of size <= 1, each a correctly rounded quotient."""
    return P * 2.0 ** -52


def ndcg_bound(k):
    """|ndcg - yardstick| allowed: sums of at most k terms of size <= 1, each a quotient over a log2 within a few ulp."""
    return 4 * k * 2.0 ** -52


def mean_bound(num_pos, k, column):
    """... of a mean over the queries: the per-query bounds added up, and nq * 2^-52 for the sum itself."""
    nq = len(num_pos)
    per_query = {RR: 0.0, AP: float(sum(ap_bound(int(p)) for p in num_pos)), NDCG: nq * ndcg_bound(k)}[column]
    return per_query + nq * 2.0 ** -52


# ------------------------------------------------------------------ cases
def group_scores(kind, P, N, rng):
    """fp32 scores of one group, the P positives first."""
    n = P + N
    if kind == "gauss":
        return ((rng.permutation(n) - n // 2) / 8192.0).astype(np.float32)      # distinct multiples of 2^-13, exact in fp32
    if kind == "ties":
        return rng.choice(np.array([-0.5, 0.0, 0.25, 1.0], dtype=np.float32), size=n)
    if kind == "flat":
        return np.full(n, 0.375, dtype=np.float32)
    if kind == "zeros":
        return np.where(rng.rand(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    if kind == "pos_last":
        s = rng.rand(n).astype(np.float32)
        s[:P] -= np.float32(2.0)
        return s
    if kind == "pos_first":
        s = rng.rand(n).astype(np.float32)
        s[:P] += np.float32(2.0)
        return s
    raise KeyError(kind)


def ragged_sizes(seed=5, groups=300):
    """300 groups of 2 .. 70 documents, 1 <= P < size."""
    rng = np.random.RandomState(seed)
    sizes = rng.randint(2, 71, size=groups)
    sizes[:4] = (2, 70, 64, 65)
    pos = np.array([rng.randint(1, n) for n in sizes])
    return [(int(p), int(n - p)) for p, n in zip(pos, sizes)]


SIZE_SETS = {f"{P}+{N}": [(P, N)] for P, N in SINGLE_SIZES}
SIZE_SETS["ragged"] = ragged_sizes()


def case_seed(kind, name):
    return 1000 * KINDS.index(kind) + list(SIZE_SETS).index(name)


def case(kind, groups, seed):
    """(scores float32 [nd], offsets int64 [nq + 1], num_pos int32 [nq]) for groups = [(P, N), ...]; the same arguments
    give the same case."""
    rng = np.random.RandomState(seed)
    scores = np.concatenate([group_scores(kind, P, N, rng) for P, N in groups]).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum([P + N for P, N in groups])]).astype(np.int64)
    return scores, offsets, np.array([P for P, _ in groups], dtype=np.int32)
