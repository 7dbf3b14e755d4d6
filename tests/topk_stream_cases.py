"""The yardstick of every top-k (tests/test_gpu_topk_stream.py, tests/test_gpu_topk_oneshot.py,
tests/test_paraphrase_mining_host.py; judged itself by tests/test_topk_cases_host.py): an fp64 numpy reference that ranks
by a FULL stable sort, the required order as a key on fp32 bit patterns, the three score functions in fp64, and the inputs
the tests share. numpy only, so the host tests import it without the library. Imported like quadruplet_eval_helpers, not a
conftest.

The order everywhere: score descending with NaN (of either sign) above +inf and -0.0 = +0.0, then id ascending -- also
among the entries tied at the k-th place. A candidate takes part unless its
id is the row's own (exclude_self) or its score is above max_score; a result row is padded with -inf / -1.
"""
import numpy as np


def topk_ref(scores, k, col_base=0, row_base=0, exclude_self=False, max_score=np.inf, ids=None):
    """(values [rows, k] in the dtype of `scores`, ids int64 [rows, k]) of scores [rows, n]: column j is id col_base + j,
    row r is query row_base + r. ids (int64 [rows, n], the caller ids of an index_map) replaces the column numbers: ties
    then go to the smaller ID, not the smaller column."""
    s = np.asarray(scores)
    rows, n = s.shape
    vals = np.full((rows, k), -np.inf, dtype=s.dtype)
    out_ids = np.full((rows, k), -1, dtype=np.int64)
    cols = col_base + np.arange(n, dtype=np.int64)
    for r in range(rows):
        col = cols if ids is None else np.asarray(ids[r], dtype=np.int64)
        with np.errstate(invalid="ignore"):             # widening a signalling NaN raises the flag; it stays a NaN
            v = s[r].astype(np.float64)
        nan = np.isnan(v)
        keep = ~(v > max_score)
        if exclude_self:
            keep &= col != row_base + r
        order = np.lexsort((col, np.where(nan, 0.0, -v), ~nan))         # NaN first, then -score, then id
        order = order[keep[order]][:k]
        vals[r, :len(order)] = s[r][order]
        out_ids[r, :len(order)] = col[order]
    return vals, out_ids


def order_key(bits):
    """The total order every top-k kernel must rank by, on fp32 BIT PATTERNS (any integer array, taken as uint32): a
    uint32 key, larger = ranks first. Every NaN, of either sign and any payload, is the one top key above +inf; -0.0 and
    +0.0 share one key; the rest is numeric. Written on the bits alone, so it judges topk_ref (which ranks by value)
    rather than restating it."""
    u = np.asarray(bits).astype(np.uint32)
    u = np.where(u == np.uint32(0x80000000), np.uint32(0), u)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where((u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(0xFFFFFFFF), key).astype(np.uint32)


def f32_from_bits(bits):
    """fp32 array with exactly these bit patterns (a NaN keeps its sign and payload: no arithmetic touches it)."""
    return np.asarray(bits).astype(np.uint32).view(np.float32)


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


def exact_scores(q, c, dim):
    """The fp32 dot matrix of integer-valued rows, after checking that the split-bf16 x3 products hold every entry exactly."""
    full = scores_ref(q, c, "dot")
    assert np.array_equal(full, np.rint(full)) and np.abs(full).max() <= dim     # integers the x3 products hold exactly
    return full.astype(np.float32)


# Real-valued cases (nq, nc, k, chunk) and their seeds, shared by the streaming and the one-shot tests (both score through
# the same score_block). Seeds: with an fp32 matmul (cos, dot) or fp32 differences (euclid) standing in for the device, each
# of these cases stays inside its cap of ranking disagreements with the fp64 order (checked on the CPU when the seeds were
# chosen: the two small-k cases had none against a cap of 2; the k = 1024 case, which ranks all 515 rows, had 2 to 10
# against a cap of 665, and 74 for euclid at dim 384).
REAL_CASES = [(33, 1000, 10, 256), (4, 3000, 100, 1024), (130, 515, 1024, 200)]
REAL_SEED = {(33, 1000, 10, 256): 101, (4, 3000, 100, 1024): 102, (130, 515, 1024, 200): 103}


def real_tol(mode, want_scores):
    """tol(score) of a real-valued case for ranking_disagreements; want_scores = the fp64 top-k values of the case."""
    if mode == "euclid":
        return lambda s: 2e-6 * abs(s) + 1e-7                                       # fp32 FMA chain + sqrt + rcp
    atol = 2e-5 * float(np.abs(want_scores[np.isfinite(want_scores)]).max())        # split-bf16 x3 products
    return lambda s: atol


def real_cap(nq, k):
    """How many positions of a real-valued case may disagree with the fp64 ranking (within twice the tolerance)."""
    return max(2, nq * k // 200)


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
