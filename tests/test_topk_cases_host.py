"""Host: the yardstick of the top-k tests judged before any kernel is involved (no GPU, no library). topk_ref ranks by VALUE
with a full stable sort; order_key states the required order on fp32 BIT PATTERNS (every NaN above +inf, the two zeros
tied, the rest numeric). The two are written independently in tests/topk_stream_cases.py and must agree, also on the ids
of an index_map and on the NaN cases the one-shot kernel used to get wrong."""
import numpy as np
import pytest

import topk_stream_cases as T

QNAN, QNAN_NEG, SNAN, ALL_ONES = 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF
PINF, NINF, PZERO, NZERO = 0x7F800000, 0xFF800000, 0x00000000, 0x80000000
SALT = [QNAN, QNAN_NEG, SNAN, ALL_ONES, PINF, NINF, PZERO, NZERO,
        0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000]      # + denormals and the smallest normals


def salted_bits(rows, n, seed):
    """Random bit patterns, a third of the columns replaced by the salt, another third by copies of other columns of the row
    (exact ties, among them ties of NaNs with different payloads and of the two zeros)."""
    rng = np.random.RandomState(seed)
    bits = rng.randint(0, 2 ** 32, size=(rows, n), dtype=np.uint64).astype(np.uint32)
    for r in range(rows):
        where = rng.permutation(n)
        salt, ties = where[:n // 3], where[n // 3:2 * (n // 3)]
        bits[r, salt] = rng.choice(np.array(SALT, dtype=np.uint32), size=len(salt))
        bits[r, ties] = bits[r, rng.randint(0, n, size=len(ties))]
    return bits


def by_key(bits, ids, k):
    """ids [rows, k] of the k first by (order_key descending, id ascending): the full sort on the integer keys."""
    key = T.order_key(bits).astype(np.int64)
    out = np.empty((len(bits), k), dtype=np.int64)
    for r in range(len(bits)):
        order = np.lexsort((ids[r], -key[r]))
        out[r] = ids[r][order[:k]]
    return out


def test_order_key_on_the_special_values():
    key = lambda b: int(T.order_key(np.array([b]))[0])
    assert key(QNAN) == key(QNAN_NEG) == key(SNAN) == key(ALL_ONES) == key(0xFF800001) == 0xFFFFFFFF
    assert key(PINF) < 0xFFFFFFFF and key(0x7F7FFFFF) < key(PINF)                        # every NaN above +inf above FLT_MAX
    assert key(PZERO) == key(NZERO)
    assert key(0x80000001) < key(PZERO) < key(0x00000001)                                # the denormals around the zeros
    assert key(NINF) < key(0xFF7FFFFF) and key(NINF) > 0                                 # -inf is the smallest real key
    # numeric order wherever neither is a NaN: a dense sample of finite values and both infinities
    rng = np.random.RandomState(0)
    bits = rng.randint(0, 2 ** 32, size=20000, dtype=np.uint64).astype(np.uint32)
    with np.errstate(invalid="ignore"):
        v = T.f32_from_bits(bits).astype(np.float64)
    keep = ~np.isnan(v)
    bits, v = bits[keep], v[keep]
    order = np.argsort(v, kind="stable")
    k = T.order_key(bits)[order].astype(np.int64)
    assert (np.diff(k) >= 0).all() and ((np.diff(k) == 0) == (np.diff(v[order]) == 0)).all()


@pytest.mark.parametrize("n,k", [(1, 1), (7, 3), (40, 40), (257, 33), (1000, 100), (1000, 1000)])
def test_sorting_by_order_key_then_id_equals_topk_ref(n, k):
    bits = salted_bits(6, n, seed=n + k)
    s = T.f32_from_bits(bits)
    cols = np.broadcast_to(np.arange(n, dtype=np.int64), bits.shape)
    want_s, want_i = T.topk_ref(s, k)
    np.testing.assert_array_equal(want_i, by_key(bits, cols, k))
    for r in range(len(bits)):                              # the values are those of the chosen columns, bit for bit
        np.testing.assert_array_equal(want_s[r].view(np.uint32), bits[r][want_i[r]])
    # ... and with caller ids: a permutation per row plus a base; ties go to the smaller id, whatever the column
    rng = np.random.RandomState(n * k)
    ids = np.stack([rng.permutation(n) for _ in range(len(bits))]).astype(np.int64) + 1000
    want_s, want_i = T.topk_ref(s, k, ids=ids)
    np.testing.assert_array_equal(want_i, by_key(bits, ids, k))
    for r in range(len(bits)):
        col_of = {int(i): c for c, i in enumerate(ids[r])}
        np.testing.assert_array_equal(want_s[r].view(np.uint32), bits[r][[col_of[int(i)] for i in want_i[r]]])


def test_topk_ref_ids_decide_ties_not_columns():
    s = np.array([[5, 7, 5, 5, 7, 5]], dtype=np.float32)
    ids = np.array([[60, 50, 40, 30, 20, 10]], dtype=np.int64)
    vals, got = T.topk_ref(s, 4, ids=ids)
    np.testing.assert_array_equal(got, [[20, 50, 10, 30]])
    np.testing.assert_array_equal(vals, [[7, 7, 5, 5]])
    np.testing.assert_array_equal(T.topk_ref(s, 4)[1], [[1, 4, 0, 2]])                  # without ids: the columns
    vals, got = T.topk_ref(s, 6, ids=ids, max_score=6.0)                                # the cap and the padded tail stay
    np.testing.assert_array_equal(got, [[10, 30, 40, 60, -1, -1]])
    np.testing.assert_array_equal(vals, [[5, 5, 5, 5, -np.inf, -np.inf]])


@pytest.mark.parametrize("nan_bits", [QNAN, QNAN_NEG, SNAN, ALL_ONES])
def test_the_three_element_nan_case(nan_bits):
    """k = n = 3, scores [NaN, 0.896, -1.283]: a sort that compares floats returns [0.896, -inf, -1.283] / [1, -1, 2]."""
    s = np.array([0.896, 0.896, -1.283], dtype=np.float32)
    bits = s.view(np.uint32).copy()
    bits[0] = nan_bits
    s = T.f32_from_bits(bits)[None, :]
    vals, ids = T.topk_ref(s, 3)
    np.testing.assert_array_equal(ids, [[0, 1, 2]])
    assert vals.view(np.uint32)[0, 0] == nan_bits and vals[0, 1] == np.float32(0.896) and vals[0, 2] == np.float32(-1.283)
    np.testing.assert_array_equal(by_key(bits[None, :], np.arange(3, dtype=np.int64)[None, :], 3), ids)


def test_zeros_tie_and_go_by_id():
    bits = np.array([[NZERO, PZERO, NZERO, 0x80000001, PZERO, 0x00000001]], dtype=np.uint32)
    vals, ids = T.topk_ref(T.f32_from_bits(bits), 6)
    np.testing.assert_array_equal(ids, [[5, 0, 1, 2, 4, 3]])
    np.testing.assert_array_equal(by_key(bits, np.arange(6, dtype=np.int64)[None, :], 6), ids)
