"""The yardstick of the BinaryClassificationEvaluator tests: what sentence-transformers 2.2.2 computes from the scores and
the 0 / 1 labels of sentence pairs, restated in plain Python / numpy the way upstream does it -- `sorted` on (score, label)
rows and a loop over them for the best accuracy and the best F1, and the average precision as sklearn's
average_precision_score takes it (fp64, a sum over the distinct scores) -- and the cases the host and the GPU test share.

Nothing here is shared with the code under test, which never sorts and never loops: it counts.
"""
import numpy as np

SIZES = (1, 2, 3, 63, 64, 65, 257, 1000, 4099, 20011)
KINDS = ("gauss", "ties", "zeros", "all0", "all1", "multi")
# out of qst_binary_eval, per score row
ACC, ACC_THR, F1, PREC, REC, F1_THR, AP, POS = range(8)


# ------------------------------------------------------------------ upstream's three routines
def sorted_rows(scores, labels, high_score_more_similar):
    """Python's sort is stable, also with reverse=True: equal scores (-0.0 == 0.0 among them) stay in input order."""
    return sorted(zip(scores, labels), key=lambda x: x[0], reverse=bool(high_score_more_similar))


def best_acc(scores, labels, high_score_more_similar):
    """(max_acc, best_threshold): the walk of find_best_acc_and_threshold."""
    assert len(scores) == len(labels)
    rows = sorted_rows(scores, labels, high_score_more_similar)
    max_acc, best_threshold = 0, -1
    positive_so_far, remaining_negatives = 0, sum(np.asarray(labels) == 0)
    for i in range(len(rows) - 1):
        score, label = rows[i]
        if label == 1:
            positive_so_far += 1
        else:
            remaining_negatives -= 1
        acc = (positive_so_far + remaining_negatives) / len(labels)
        if acc > max_acc:
            max_acc = acc
            best_threshold = (rows[i][0] + rows[i + 1][0]) / 2
    return max_acc, best_threshold


def best_f1(scores, labels, high_score_more_similar):
    """(best_f1, best_precision, best_recall, threshold): the walk of find_best_f1_and_threshold."""
    assert len(scores) == len(labels)
    scores, labels = np.asarray(scores), np.asarray(labels)
    rows = sorted_rows(scores, labels, high_score_more_similar)
    best = best_precision = best_recall = 0
    threshold = 0
    nextract = ncorrect = 0
    total_num_duplicates = sum(labels)
    for i in range(len(rows) - 1):
        score, label = rows[i]
        nextract += 1
        if label == 1:
            ncorrect += 1
        if ncorrect > 0:
            precision = ncorrect / nextract
            recall = ncorrect / total_num_duplicates
            f1 = 2 * precision * recall / (precision + recall)
            if f1 > best:
                best, best_precision, best_recall = f1, precision, recall
                threshold = (rows[i][0] + rows[i + 1][0]) / 2
    return best, best_precision, best_recall, threshold


def average_precision(scores, labels, high_score_more_similar):
    """sklearn.metrics.average_precision_score(labels, scores if high else -scores) in fp64: over the distinct scores from
    the most similar down, sum of (recall - previous recall) * precision. No positive: 0.0 (sklearn warns and returns it)."""
    s = np.asarray(scores, dtype=np.float64) * (1.0 if high_score_more_similar else -1.0)
    y = np.asarray(labels, dtype=np.float64)
    order = np.argsort(s, kind="mergesort")[::-1]
    s, y = s[order], y[order]
    last_of_run = np.r_[np.flatnonzero(np.diff(s)), len(s) - 1]
    tps = np.cumsum(y)[last_of_run]
    if tps[-1] == 0:
        return 0.0
    precision = tps / (1.0 + last_of_run)
    recall = tps / tps[-1]
    return float(np.sum(np.diff(np.r_[0.0, recall]) * precision))


def expected(scores, labels, high_score_more_similar):
    """The eight numbers of a score row in the order qst_binary_eval writes them, as Python floats."""
    acc, acc_thr = best_acc(scores, labels, high_score_more_similar)
    f1, precision, recall, f1_thr = best_f1(scores, labels, high_score_more_similar)
    ap = average_precision(scores, labels, high_score_more_similar)
    return [float(acc), float(acc_thr), float(f1), float(precision), float(recall), float(f1_thr), ap,
            float(np.sum(labels))]


def ap_bound(n):
    """|ap - yardstick| allowed: the sum has at most n terms, each at most 1, each rounded to 2^-53 and added with as much."""
    return n * 2.0 ** -52


# ------------------------------------------------------------------ cases
# Twelve rows in sorted order whose best accuracy is reached behind rows 0, 2, 4 and 6 and whose best F1 (2 / 3 as a
# fraction) behind rows 6 and 9; with every row repeated k times the ties stay, behind rows k - 1, 3k - 1, ... .
MULTI_BASE = (1, 0, 1, 0, 1, 0, 1, 0, 0, 1, 0, 0)


def multi_max(n, seed, high_score_more_similar):
    rng = np.random.RandomState(seed)
    k = max(n // len(MULTI_BASE), 1)
    in_order = np.r_[np.repeat(MULTI_BASE, k), np.zeros(max(n - k * len(MULTI_BASE), 0), dtype=np.int64)][:n]
    similarity = (np.linspace(1.0, -1.0, n) if n > 1 else np.ones(1)).astype(np.float32)   # distinct, most similar first
    where = rng.permutation(n)                                                            # the input is not sorted
    scores, labels = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.int64)
    scores[where] = similarity if high_score_more_similar else -similarity
    labels[where] = in_order
    return scores, labels


def case(kind, n, seed, high_score_more_similar=True):
    """(scores float32 [n], labels int64 [n]) of one kind; the same arguments give the same case."""
    rng = np.random.RandomState(seed)
    if kind == "multi":
        return multi_max(n, seed, high_score_more_similar)
    if kind == "ties":      # multiples of 0.25 in [-1, 1]: most cuts fall inside a run of equal scores
        scores = (rng.randint(-4, 5, size=n) * 0.25).astype(np.float32)
    else:
        scores = rng.randn(n).astype(np.float32)
    if kind == "zeros" and n >= 2:          # -0.0 beside +0.0, and a few more of either sign further on
        at = rng.choice(n - 1, size=max(n // 16, 1), replace=False)
        scores[at] = 0.0
        scores[at + 1] = -0.0
        assert np.signbit(scores).any() and (scores == 0).sum() >= 2
    if kind == "all0":
        labels = np.zeros(n, dtype=np.int64)
    elif kind == "all1":
        labels = np.ones(n, dtype=np.int64)
    else:
        labels = (rng.rand(n) < rng.uniform(0.1, 0.9)).astype(np.int64)
    return scores, labels


def case_seed(kind, n):
    return 1000 * KINDS.index(kind) + n
