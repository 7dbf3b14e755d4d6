"""The yardstick of the streaming top-k (tests/test_gpu_topk_stream.py, tests/test_paraphrase_mining_host.py): an fp64
numpy reference that ranks by a FULL stable sort, the three score functions in fp64, and the inputs the tests share.
numpy only, so the host tests import it without the library. Imported like quadruplet_eval_helpers, not a conftest.

The order everywhere: score descending with NaN above +inf, then global id ascending. A candidate takes part unless its
id is the row's own (exclude_self) or its score is above max_score; a result row is padded with -inf / -1.
"""
import numpy as np


def topk_ref(scores, k, col_base=0, row_base=0, exclude_self=False, max_score=np.inf):
    """(values [rows, k] in the dtype of `scores`, ids int64 [rows, k]) of scores [rows, n]: column j is id col_base + j,
    row r is query row_base + r."""
    s = np.asarray(scores)
    rows, n = s.shape
    vals = np.full((rows, k), -np.inf, dtype=s.dtype)
    ids = np.full((rows, k), -1, dtype=np.int64)
    col = col_base + np.arange(n, dtype=np.int64)
    for r in range(rows):
        v = s[r].astype(np.float64)
        nan = np.isnan(v)
        keep = ~(v > max_score)
        if exclude_self:
            keep &= col != row_base + r
        order = np.lexsort((col, np.where(nan, 0.0, -v), ~nan))         # NaN first, then -score, then id
        order = order[keep[order]][:k]
        vals[r, :len(order)] = s[r][order]
        ids[r, :len(order)] = col[order]
    return vals, ids


def scores_ref(q, c, mode):
    """fp64 [nq, nc]: 'dot', 'cos' (rows normalised with eps 1e-12) or 'euclid' (1 / (1 + ||q - c||_2))."""
    q, c = np.asarray(q, dtype=np.float64), np.asarray(c, dtype=np.float64)
    if mode == "dot":
        return q @ c.T
    if mode == "cos":
        qn = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)
        cn = c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-12)
        return qn @ cn.T
    assert mode == "euclid"
    out = np.empty((len(q), len(c)))
    for r in range(len(q)):
        out[r] = 1.0 / (1.0 + np.sqrt(((q[r][None, :] - c) ** 2).sum(1)))
    return out


def hand_scores(rows, n, seed):
    """Small integers in [-3, 3] as fp32: at n >= 8 every value is tied many times over, at and around any cut."""
    return np.random.RandomState(seed).randint(-3, 4, size=(rows, n)).astype(np.float32)


def ternary(n, dim, seed):
    """Rows with entries in {-1, 0, 1}: every dot product is an integer of magnitude <= dim, exact in split-bf16 x3."""
    return np.random.RandomState(seed).randint(-1, 2, size=(n, dim)).astype(np.float32)


def slices(n, parts, seed=0):
    """[0, n) cut into min(parts, n) consecutive slices of unequal width (where n allows), as (start, stop) pairs."""
    parts = min(parts, n)
    cuts = np.sort(np.random.RandomState(seed + 31 * n + parts).choice(np.arange(1, n), size=parts - 1, replace=False)) \
        if parts > 1 else np.zeros(0, dtype=np.int64)
    edges = [0, *[int(x) for x in cuts], n]
    return list(zip(edges[:-1], edges[1:]))


def ranking_disagreements(got_scores, got_ids, full, want_ids, tol):
    """How a result may differ from the fp64 ranking `want_ids` of the fp64 matrix `full`: every returned score within
    tol(score) of the fp64 score of the id returned WITH it, and where the id at a position differs from the fp64
    ranking's, the two fp64 scores closer than twice that tolerance. Returns the number of such positions; asserts the
    rest. Padding must match exactly."""
    n_bad = 0
    for r in range(len(got_ids)):
        for p in range(got_ids.shape[1]):
            a, b = int(got_ids[r, p]), int(want_ids[r, p])
            assert (a < 0) == (b < 0), (r, p, a, b)
            if a < 0:
                assert got_scores[r, p] == -np.inf
                continue
            t = tol(full[r, a])
            assert abs(float(got_scores[r, p]) - full[r, a]) <= t, (r, p, a, float(got_scores[r, p]), full[r, a], t)
            if a != b:
                assert abs(full[r, a] - full[r, b]) < 2 * t, (r, p, a, b, full[r, a], full[r, b])
                n_bad += 1
    return n_bad
