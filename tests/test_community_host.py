"""CPU: community detection off the device -- the fp64 contract of tests/community_cases.py on hand-worked cases, the pure
numpy round planner of util.community_detection (an emulated run gives the same communities for every round budget; taken
rows are skipped only where they belong to their own community), the C-ABI's size and argument checks, and the
ValueErrors of the Python function, all of which come before any device use."""
import os
import sys

import numpy as np
import pytest

import quadruplet_sentence_transformer_amd  # noqa: F401
import community_cases as CC
from quadruplet_sentence_transformer_amd import _lib, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unit(*angles_deg):
    """Rows on the unit circle: the cosine of two rows is the cosine of the difference of their angles."""
    a = np.deg2rad(np.asarray(angles_deg, dtype=np.float64))
    return np.stack([np.cos(a), np.sin(a)], axis=1)


# ------------------------------------------------------------------ the oracle on hand-worked cases
def test_larger_community_wins_and_the_overlapping_smaller_one_is_dropped_whole():
    # within 25 deg: row 2 (20 deg) sees rows 0 .. 4; row 5 (60 deg) sees 41, 60, 70 -> the two overlap in row 4 (41 deg)
    e = unit(0, 11, 20, 28, 41, 60, 70)
    thr = np.cos(np.deg2rad(25.0))
    np.testing.assert_array_equal(CC.counts_ref(e, thr), [3, 4, 5, 4, 4, 3, 2])
    got = CC.community_ref(e, thr, 3)
    assert got == [[2, 3, 1, 0, 4]]                       # row 4 belongs to the first: {4, 5, 6} is dropped, not trimmed
    out, ncand, rejected = CC.community_ref(e, thr, 3, want_trace=True)
    assert (ncand, rejected) == (6, 5)                    # the candidates with 4 and 3 members all touch a taken row


def test_equal_size_the_lower_row_wins():
    # rows 1 and 2 both see three rows, each other among them
    e = unit(0, 10, 21, 31)
    thr = np.cos(np.deg2rad(15.0))
    np.testing.assert_array_equal(CC.counts_ref(e, thr), [2, 3, 3, 2])
    assert CC.community_ref(e, thr, 3) == [[1, 0, 2]]
    assert CC.community_ref(e[::-1], thr, 3) == [[1, 0, 2]]           # mirrored: again the lower row


def test_min_size_exactly_met_and_missed_by_one():
    e = unit(0, 1, 2, 90, 91)
    thr = 0.99
    assert CC.community_ref(e, thr, 3) == [[0, 1, 2]]
    assert CC.community_ref(e, thr, 2) == [[0, 1, 2], [3, 4]]
    assert CC.community_ref(e, thr, 4) == []


def test_min_size_one_returns_singletons_and_too_large_returns_nothing():
    e = unit(0, 1, 90, 180)
    assert CC.community_ref(e, 0.99, 1) == [[0, 1], [2], [3]]
    assert CC.community_ref(e, 0.99, 5) == []


def test_zero_and_nan_rows_belong_to_nothing():
    e = np.array([[1, 0], [0, 0], [1, 0.01], [np.nan, 1], [0.99, 0]], dtype=np.float64)
    np.testing.assert_array_equal(CC.counts_ref(e, 0.5), [3, 0, 3, 0, 3])
    assert CC.community_ref(e, 0.5, 1) == [[0, 4, 2]]
    # at threshold <= 0 a zero row scores 0 with everything finite, itself included, and is a member; a NaN row never is
    np.testing.assert_array_equal(CC.counts_ref(e, 0.0), [4, 4, 4, 0, 4])


def test_central_point_first_then_score_then_row():
    e = unit(10, 0.5, 20, 12, 7)                          # row 0 is the centre of everything within 10.5 deg
    thr = np.cos(np.deg2rad(10.5))
    assert CC.community_ref(e, thr, 5) == [[0, 3, 4, 1, 2]]           # 2, 3, 9.5 and 10 deg away
    # exact ties (+-1 rows: every other row has cosine 1/2 with row 1): ascending row, the centre still first
    e = np.array([[1, 1, 1, -1], [1, 1, 1, 1], [1, 1, -1, 1], [1, -1, 1, 1]], dtype=np.float64)
    assert CC.community_ref(e, 0.4, 3) == [[1, 0, 2, 3]]


def test_planted_cases_reject_and_accept():
    for name, (dim, sizes, maxflip, noise, k, min_size) in CC.PLANTED.items():
        if dim > 96:
            continue                                       # the large case's reference runs once, in the GPU test
        e, thr, ms = CC.planted_case(name)
        assert CC.margin(e, thr) >= 1e-3
        out, ncand, rejected = CC.community_ref(e, thr, ms, want_trace=True)
        assert rejected >= 1 and len(out) >= 2 and ncand == rejected + len(out)
        flat = [j for c in out for j in c]
        assert len(flat) == len(set(flat))


# ------------------------------------------------------------------ the round planner
def test_order_is_size_descending_then_row_ascending():
    counts = np.array([3, 7, 1, 7, 3, 9])
    np.testing.assert_array_equal(util.community_order(counts, 3), [5, 1, 3, 0, 4])
    np.testing.assert_array_equal(util.community_order(counts, 10), [])


def test_planner_budget_and_progress():
    counts = np.array([5, 4, 4, 3, 2])
    order = util.community_order(counts, 1)
    none = np.zeros(5, dtype=bool)
    all_self = np.ones(5, dtype=bool)
    picked, nxt = util.plan_community_round(order, counts, all_self, none, 0, 9)
    assert picked.tolist() == [0, 1] and nxt == 2
    picked, nxt = util.plan_community_round(order, counts, all_self, none, 2, 1)      # budget below one candidate: one anyway
    assert picked.tolist() == [2] and nxt == 3
    picked, nxt = util.plan_community_round(order, counts, all_self, none, 0, 1 << 40)
    assert picked.tolist() == [0, 1, 2, 3, 4] and nxt == 5
    picked, nxt = util.plan_community_round(order, counts, all_self, none, 5, 9)
    assert len(picked) == 0 and nxt == 5


def test_planner_skips_taken_rows_only_when_they_are_their_own_members():
    counts = np.array([5, 4, 4, 3, 2])
    order = util.community_order(counts, 1)
    taken = np.array([False, True, True, False, True])
    self_member = np.array([True, True, False, True, True])
    picked, nxt = util.plan_community_round(order, counts, self_member, taken, 0, 1 << 40)
    assert picked.tolist() == [0, 2, 3] and nxt == 5       # row 2 is taken but not its own member: still looked at
    # skipped candidates cost nothing: 5 + (4 skipped) + 4 fits a budget of 9
    picked, nxt = util.plan_community_round(order, counts, self_member, taken, 0, 9)
    assert picked.tolist() == [0, 2] and nxt == 3
    # nothing live left: the run ends
    picked, nxt = util.plan_community_round(order, counts, np.ones(5, bool), np.ones(5, bool), 0, 9)
    assert len(picked) == 0 and nxt == 5


@pytest.mark.parametrize("name", ["d96_k12", "d96_k6"])
def test_emulated_run_is_the_same_for_every_round_budget(name):
    e, thr, ms = CC.planted_case(name)
    want = [sorted(c) for c in CC.community_ref(e, thr, ms)]
    counts = CC.counts_ref(e, thr)
    budgets = {"one": 1, "three": int(3 * counts.max()), "everything": 1 << 40}
    rounds = {}
    for label, budget in budgets.items():
        got, rounds[label] = CC.emulate(e, thr, ms, budget, util.plan_community_round, util.community_order)
        assert got == want, label
    assert rounds["everything"] == 1 and rounds["one"] >= rounds["three"] >= 1 and rounds["one"] > 1


def test_emulated_run_with_rows_that_are_not_their_own_members():
    # at threshold 0 the zero row scores 0 with every finite row, itself included: a candidate that is its own member.
    # The NaN row never is. Both must leave the result equal to the oracle's at every budget.
    e = np.array([[1, 0], [0, 0], [1, 0.01], [np.nan, 1], [-1, 0], [-1, 0.01]], dtype=np.float64)
    for thr, ms in ((0.0, 1), (0.5, 1), (0.5, 2)):
        want = [sorted(c) for c in CC.community_ref(e, thr, ms)]
        for budget in (1, 4, 1 << 40):
            got, _ = CC.emulate(e, thr, ms, budget, util.plan_community_round, util.community_order)
            assert got == want, (thr, ms, budget)


def test_order_community_puts_the_centre_first():
    assert util.order_community(7, [2, 5, 7, 9], [0.9, 0.9, 1.0, 0.95]) == [7, 9, 2, 5]
    assert util.order_community(7, [2, 5, 9], [0.9, 0.95, 0.9]) == [5, 2, 9]           # the centre is not a member
    assert util.order_community(5, [2, 5, 7], [1.0, 1.0, 1.0]) == [5, 2, 7]            # duplicates: centre, then by row
    assert all(type(m) is int for m in util.order_community(1, np.array([1, 0]), np.array([1.0, 0.8])))


# ------------------------------------------------------------------ the library
def test_library_binds_the_entry_points_and_sizes_the_workspace_linearly():
    lib = _lib.load()
    assert lib.qst_version() >= 111
    for name in ("qst_community_workspace_bytes", "qst_community_count", "qst_community_members", "qst_community_claim",
                 "qst_community_rescore"):
        assert hasattr(lib, name) and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    ws = lib.qst_community_workspace_bytes
    assert ws(0, 4, 32) == 0 and ws(4, 0, 32) == 0 and ws(4, 4, 0) == 0
    for n, c, d in ((16384, 16384, 384), (100000, 16384, 384), (5000, 100, 32), (1 << 20, 7, 96)):
        assert 0 < ws(2 * n, c, d) <= 2 * ws(n, c, d)
    # independent of n^2: ten times the rows is about ten times the bytes, and the panel does not grow at all
    a, b = ws(10 ** 5, 16384, 384), ws(10 ** 6, 16384, 384)
    assert b < 10 * a and b - a == 9 * 10 ** 5 * 384 * 4
    assert ws(10 ** 6, 16384, 384) < 2 * 10 ** 9           # 1.5 GB of rows + a 128 MB panel, against 4 TB of scores
    assert ws(3, 100, 32) == ws(3, 3, 32)                   # a chunk past n is n


def test_library_checks_arguments_before_any_launch():
    lib = _lib.load()
    big = 1 << 40
    p = 4096                                                # a non-null pointer that is never followed
    count = lambda *a: lib.qst_community_count(*a)          # noqa: E731
    assert count(None, 8, 32, 0.5, 8, p, p, p, big, None) == -1
    assert count(p, 8, 32, 0.5, 8, None, p, p, big, None) == -1
    assert count(p, 8, 32, 0.5, 8, p, p, None, big, None) == -1
    assert count(p, 0, 32, 0.5, 8, p, p, p, big, None) == -1
    assert count(p, 8, 0, 0.5, 8, p, p, p, big, None) == -1
    assert count(p, 8, 32, 0.5, 0, p, p, p, big, None) == -1
    assert count(p, 8, 32, float("nan"), 8, p, p, p, big, None) == -1
    assert count(p, 8, 40, 0.5, 8, p, p, p, big, None) == -2                           # dim % 32
    assert count(p, 8, 32, 0.5, 8, p, p, p, lib.qst_community_workspace_bytes(8, 8, 32) - 1, None) == -3
    assert count(p, 1 << 30, 1 << 20, 0.5, 1 << 30, p, p, p, 1 << 62, None) == -2      # one chunk's operand past 2^31 bytes
    mem = lambda *a: lib.qst_community_members(*a)          # noqa: E731
    assert mem(None, 8, 32, 0.5, 8, 0, p, p, p, p, p, p, big, None) == -1
    for hole in range(6, 11):                               # begin, capacity, out_index, out_score, written
        args = [p, 8, 32, 0.5, 8, 0, p, p, p, p, p, p, big, None]
        args[hole] = None
        assert mem(*args) == -1, hole
    assert mem(p, 8, 40, 0.5, 8, 0, p, p, p, p, p, p, big, None) == -2
    assert mem(p, 8, 32, 0.5, 8, 0, p, p, p, p, p, p, 16, None) == -3
    assert mem(p, 5000, 32, 0.5, 8, 100, p, p, p, p, p, p, big, None) == -1            # row0 not a multiple of 2048
    assert mem(p, 5000, 32, 0.5, 8, 6144, p, p, p, p, p, p, big, None) == -1           # ... or past the rows
    assert mem(p, 5000, 32, 0.5, 8, -2048, p, p, p, p, p, p, big, None) == -1
    assert lib.qst_community_claim(p, p, 3, p, 8, None, p, None) == -1
    assert lib.qst_community_claim(p, p, -1, p, 8, p, p, None) == -1
    assert lib.qst_community_claim(None, p, 3, p, 8, p, p, None) == -1
    assert lib.qst_community_claim(p, p, 3, p, 0, p, p, None) == -1
    assert lib.qst_community_claim(None, None, 0, None, 8, p, None, None) == 0         # no candidates: nothing to do
    assert lib.qst_community_rescore(None, 8, 32, p, p, 4, p, None) == -1
    assert lib.qst_community_rescore(p, 8, 32, p, None, 4, p, None) == -1
    assert lib.qst_community_rescore(p, 8, 32, p, p, -1, p, None) == -1
    assert lib.qst_community_rescore(p, 8, 32, None, None, 0, None, None) == 0


# ------------------------------------------------------------------ the Python function, before any device use
def test_python_function_refuses_bad_arguments_before_any_device_use():
    e = np.ones((4, 8), dtype=np.float32)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="min_community_size"):
            util.community_detection(e, min_community_size=bad)
    for bad in (0, -1, 10.0, None):
        with pytest.raises(ValueError, match="init_max_size"):
            util.community_detection(e, init_max_size=bad)
    with pytest.raises(ValueError, match="threshold"):
        util.community_detection(e, threshold=float("nan"))
    for bad in (0, -7):
        with pytest.raises(ValueError, match="corpus_chunk_size"):
            util.community_detection(e, corpus_chunk_size=bad)
    with pytest.raises(TypeError):
        util.community_detection(e, 0.75, 10, 1000, 64)     # corpus_chunk_size is keyword-only
    assert util.community_detection(e, min_community_size=5) == []       # min_community_size > n: nothing, and no device
    assert "init_max_size" in util.community_detection.__doc__ and "Deliberate differences" in util.community_detection.__doc__


def test_dropin_namespace_exports_community_detection():
    drop = os.path.join(ROOT, "dropin")
    stale = lambda: [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]  # noqa: E731
    sys.path.insert(0, drop)
    try:
        for m in stale():
            del sys.modules[m]
        from sentence_transformers.util import community_detection
        assert community_detection is util.community_detection
    finally:
        sys.path.remove(drop)
        for m in stale():
            del sys.modules[m]
