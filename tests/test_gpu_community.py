"""GPU: community detection -- qst_community_count (|N(i)| per row from the chunked score panels), qst_community_members
(the members of wanted rows, compacted in column order out of the SAME panels), qst_community_claim (the greedy pass),
qst_community_rescore (fp64 cosines for the order inside a community) and util.community_detection on top. The yardstick
is the fp64 contract of tests/community_cases.py on rows of +-1, whose cosines are exact multiples of 1 / dim: every test
that compares memberships first asserts that no cosine is nearer to the threshold than 1e-3 (a condition on the inputs),
and then the comparison is exact. The sizes are what the tests need, not the workload's."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import community_cases as CC  # noqa: E402
from kernel_helpers import lib, stream  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import _lib, util  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = -77


def dev(e):
    return torch.from_numpy(np.ascontiguousarray(e, dtype=np.float32)).cuda()


def workspace(lib, n, chunk, dim):
    return torch.empty(lib.qst_community_workspace_bytes(n, chunk, dim), dtype=torch.uint8, device="cuda")


def count(lib, e, thr, chunk):
    """(counts int32 [n], self_member bool [n]) of qst_community_count."""
    n, dim = e.shape
    ed, ws = dev(e), workspace(lib, n, chunk, dim)
    counts = torch.full((n,), GUARD, dtype=torch.int32, device="cuda")
    own = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    rc = lib.qst_community_count(ed.data_ptr(), n, dim, thr, chunk, counts.data_ptr(), own.data_ptr(), ws.data_ptr(),
                                 ws.numel(), stream())
    assert rc == 0
    return counts.cpu().numpy(), own.cpu().numpy()


def members(lib, e, thr, chunk, row0, wanted, capacity):
    """qst_community_members for the row block at row0. wanted: block rows to extract; capacity: {block row: capacity}.
    Every wanted row gets a slot of `capacity` entries with one guard word before and after it. Returns (per wanted row
    (indices, scores) of its slot, written int32 [rows], the whole index / score buffers, the slot starts)."""
    n, dim = e.shape
    rows = min(2048, n - row0)
    begin = np.full(rows, -1, dtype=np.int64)
    cap = np.zeros(rows, dtype=np.int32)
    at = 0
    for r in wanted:
        begin[r] = at + 1
        cap[r] = capacity[r]
        at += capacity[r] + 2
    ed, ws = dev(e), workspace(lib, n, chunk, dim)
    oi = torch.full((max(at, 1),), GUARD, dtype=torch.int32, device="cuda")
    os_ = torch.full((max(at, 1),), float(GUARD), dtype=torch.float32, device="cuda")
    wr = torch.full((rows,), GUARD, dtype=torch.int32, device="cuda")
    bd, cd = torch.from_numpy(begin).cuda(), torch.from_numpy(cap).cuda()
    rc = lib.qst_community_members(ed.data_ptr(), n, dim, thr, chunk, row0, bd.data_ptr(), cd.data_ptr(), oi.data_ptr(),
                                   os_.data_ptr(), wr.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    assert rc == 0
    oi, os_ = oi.cpu().numpy(), os_.cpu().numpy()
    slots = {r: (oi[begin[r]:begin[r] + cap[r]], os_[begin[r]:begin[r] + cap[r]]) for r in wanted}
    return slots, wr.cpu().numpy(), oi, os_, begin


@functools.lru_cache(maxsize=None)
def planted_n(n, dim):
    """n rows of +-1 at width dim with three clusters (where n allows) and the rest noise; the threshold that takes rows
    differing in at most dim / 8 places. Returns (emb, threshold, fp64 counts); built once per size."""
    sizes = [s for s in (n // 3, n // 4, n // 8) if s > 0]
    e = CC.planted(sizes, dim, max(1, dim // 8), n - sum(sizes), seed=100 + n + dim)
    thr = CC.threshold_for(dim // 8, dim)
    assert len(e) == n and CC.margin(e, thr) >= 1e-3
    return e, thr, CC.counts_ref(e, thr)


@functools.lru_cache(maxsize=None)
def planted_ref(name):
    e, thr, ms = CC.planted_case(name)
    assert CC.margin(e, thr) >= 1e-3
    out, ncand, rejected = CC.community_ref(e, thr, ms, want_trace=True)
    assert rejected >= 1 and len(out) >= 2                 # rejection and more than one acceptance are exercised
    return e, thr, ms, out


# ------------------------------------------------------------------ 1. qst_community_count
@pytest.mark.parametrize("dim", [32, 96, 384])
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 257, 1030])
def test_count_equals_the_oracle_for_every_chunk(lib, n, dim):
    e, thr, want = planted_n(n, dim)
    if n >= 63:
        assert want.max() >= 10 and want.min() <= 2        # clusters and loners both present
    for chunk in (n, 64, 100, 7):
        got, own = count(lib, e, thr, chunk)
        np.testing.assert_array_equal(got, want, err_msg=f"chunk {chunk}")
        assert (own == 1).all()                             # a row of +-1 scores 1 with itself to fp32-class error


def test_count_two_row_blocks_the_second_with_four_rows(lib):
    e, thr, want = planted_n(2049 + 3, 32)
    got, own = count(lib, e, thr, 100)
    np.testing.assert_array_equal(got, want)
    assert (own == 1).all()


@pytest.mark.parametrize("n", [3, 65, 257])
def test_count_at_and_below_zero_does_not_see_the_padding(lib, n):
    # 31 entries of +-1 and a zero: every dot product is odd, so no cosine is 0 and the only scores of exactly 0 are the
    # padded columns' and padded rows'
    e = np.pad(CC.planted([n // 2], 31, 4, n - n // 2, seed=n), ((0, 0), (0, 1)))
    assert CC.margin(e, 0.0) >= 1e-3
    want0 = CC.counts_ref(e, 0.0)
    assert (want0 < n).any() and want0.sum() == (CC.cosine_ref(e) > 0).sum()
    for chunk in (n, 64, 7, 2):
        got, _ = count(lib, e, -1.0, chunk)
        np.testing.assert_array_equal(got, np.full(n, n), err_msg=f"chunk {chunk}")
        got, _ = count(lib, e, 0.0, chunk)
        np.testing.assert_array_equal(got, want0, err_msg=f"chunk {chunk}")


def test_count_is_identical_for_every_chunk_even_on_the_lattice(lib):
    # a threshold that IS a cosine of these rows: whether such a score passes is rounding's business, but the same bits
    # come out however the columns are cut, so every chunking gives the same counts
    e, _, _ = planted_n(257, 96)
    thr = 1.0 - 2 * 12 / 96
    assert CC.margin(e, thr) < 1e-9
    base, _ = count(lib, e, thr, 257)
    for chunk in (256, 128, 100, 64, 7, 1):
        got, _ = count(lib, e, thr, chunk)
        np.testing.assert_array_equal(got, base, err_msg=f"chunk {chunk}")


def test_count_zero_and_nan_rows(lib):
    e = np.zeros((6, 32), dtype=np.float32)
    e[0, 0] = e[2, 0] = e[4, 0] = 1.0
    e[2, 1] = 0.01
    e[4, 0] = 0.99
    e[3, 5] = np.nan
    want = CC.counts_ref(e, 0.5)
    np.testing.assert_array_equal(want, [3, 0, 3, 0, 3, 0])
    got, own = count(lib, e, 0.5, 4)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(own, [1, 0, 1, 0, 1, 0])  # a zero row and a NaN row are not their own members
    got, own = count(lib, e, 0.0, 4)
    np.testing.assert_array_equal(got, CC.counts_ref(e, 0.0))
    np.testing.assert_array_equal(own, [1, 1, 1, 0, 1, 1])  # at threshold 0 the zero rows are (score 0)


# ------------------------------------------------------------------ 2. qst_community_members
@pytest.mark.parametrize("chunk", [157, 64, 100, 7])
def test_members_are_the_oracles_in_column_order_with_the_scores_of_cos_sim(lib, chunk):
    e, thr, ms, _ = planted_ref("d96_k12")
    n = len(e)
    want = CC.members_ref(e, thr)
    full = util.cos_sim(dev(e), dev(e)).cpu().numpy()
    counts, _ = count(lib, e, thr, chunk)
    wanted = [r for r in range(n) if r % 3 != 1]            # every third row is not asked for
    slots, written, oi, os_, begin = members(lib, e, thr, chunk, 0, wanted, {r: int(counts[r]) for r in wanted})
    for r in wanted:
        idx, sc = slots[r]
        np.testing.assert_array_equal(idx, want[r])          # ascending, the oracle's set
        assert written[r] == counts[r] == len(want[r])
        np.testing.assert_array_equal(sc.view(np.uint32), full[r, idx].view(np.uint32))      # bit for bit
        assert oi[begin[r] - 1] == GUARD and oi[begin[r] + counts[r]] == GUARD
        assert os_[begin[r] - 1] == GUARD and os_[begin[r] + counts[r]] == GUARD
    # rows not asked for wrote nothing: the buffers hold the slots and guard words and nothing else
    assert (oi == GUARD).sum() == 2 * len(wanted) and (written[[r for r in range(n) if r % 3 == 1]] == 0).all()


def test_members_capacity_below_the_count_stops_the_stores_and_reports_the_count(lib):
    e, thr, ms, _ = planted_ref("d96_k12")
    want = CC.members_ref(e, thr)
    wanted = [r for r in range(len(e)) if len(want[r]) >= 5][:20]
    assert len(wanted) == 20
    cap = {r: len(want[r]) - 3 for r in wanted}
    cap[wanted[0]] = 0
    slots, written, oi, _, begin = members(lib, e, thr, 64, 0, wanted, cap)
    for r in wanted:
        np.testing.assert_array_equal(slots[r][0], want[r][:cap[r]])
        assert written[r] == len(want[r])
        assert oi[begin[r] - 1] == GUARD and oi[begin[r] + cap[r]] == GUARD


def test_members_of_the_second_row_block(lib):
    e, thr, want_counts = planted_n(2049 + 3, 32)
    want = CC.members_ref(e, thr)
    slots, written, _, _, _ = members(lib, e, thr, 700, 2048, [0, 1, 3], {r: int(want_counts[2048 + r]) for r in (0, 1, 3)})
    for r in (0, 1, 3):
        np.testing.assert_array_equal(slots[r][0], want[2048 + r])
    np.testing.assert_array_equal(written, [want_counts[2048], want_counts[2049], 0, want_counts[2051]])


def test_members_refuses_a_row_block_that_does_not_start_on_2048(lib):
    e, thr, _ = planted_n(65, 32)
    ed, ws = dev(e), workspace(lib, 65, 65, 32)
    b = torch.full((65,), -1, dtype=torch.int64, device="cuda")
    i32 = torch.zeros(65, dtype=torch.int32, device="cuda")
    f32 = torch.zeros(65, dtype=torch.float32, device="cuda")
    for row0 in (1, 64, 2048, -2048):
        assert lib.qst_community_members(ed.data_ptr(), 65, 32, thr, 65, row0, b.data_ptr(), i32.data_ptr(), i32.data_ptr(),
                                         f32.data_ptr(), i32.data_ptr(), ws.data_ptr(), ws.numel(), stream()) == -1


def test_members_pass_agrees_with_the_count_pass_on_inexact_scores(lib):
    n, dim, thr = 300, 96, 0.1
    e = np.random.RandomState(5).randn(n, dim).astype(np.float32)
    full = util.cos_sim(dev(e), dev(e)).cpu().numpy()
    for chunk in (300, 64, 7):
        counts, own = count(lib, e, thr, chunk)
        assert 3 * n < counts.sum() < n * n // 2            # the threshold cuts through the bulk of the scores
        slots, written, _, _, _ = members(lib, e, thr, chunk, 0, list(range(n)), {r: int(counts[r]) for r in range(n)})
        np.testing.assert_array_equal(written, counts)
        for r in range(n):
            np.testing.assert_array_equal(slots[r][0], np.flatnonzero(full[r] >= np.float32(thr)))
            np.testing.assert_array_equal(slots[r][1].view(np.uint32), full[r, slots[r][0]].view(np.uint32))
        np.testing.assert_array_equal(own, np.diag(full) >= np.float32(thr))


# ------------------------------------------------------------------ 3. qst_community_claim
def claim(lib, lists, n, taken=None, order=None):
    """The candidates' member lists, laid out in list order with a gap between them, claimed in `order`."""
    order = list(range(len(lists))) if order is None else order
    begin, flat = [], []
    for m in lists:
        flat.append(GUARD)
        begin.append(len(flat))
        flat.extend(m)
    flat.append(GUARD)
    mem = torch.tensor(flat, dtype=torch.int32, device="cuda")
    b = torch.tensor([begin[c] for c in order], dtype=torch.int64, device="cuda")
    ln = torch.tensor([len(lists[c]) for c in order], dtype=torch.int32, device="cuda")
    taken = torch.zeros(n, dtype=torch.uint8, device="cuda") if taken is None else taken
    acc = torch.full((max(len(order), 1),), 9, dtype=torch.uint8, device="cuda")
    assert lib.qst_community_claim(b.data_ptr(), ln.data_ptr(), len(order), mem.data_ptr(), n, taken.data_ptr(),
                                   acc.data_ptr(), stream()) == 0
    return acc.cpu().numpy()[:len(order)].tolist(), taken


def test_claim_hand_built_lists_and_the_order_decides(lib):
    lists = [[0, 1, 2, 3], [3, 4], [5, 6], [6, 7, 8], [9]]
    acc, taken = claim(lib, lists, 12)
    assert acc == [1, 0, 1, 0, 1]
    np.testing.assert_array_equal(taken.cpu().numpy(), [1, 1, 1, 1, 0, 1, 1, 0, 0, 1, 0, 0])    # a rejected one marks nothing
    acc, taken = claim(lib, lists, 12, order=[4, 3, 2, 1, 0])
    assert acc == [1, 1, 0, 1, 0]                           # the same lists the other way round: the others win
    np.testing.assert_array_equal(taken.cpu().numpy(), [0, 0, 0, 1, 1, 0, 1, 1, 1, 1, 0, 0])


def test_claim_one_taken_member_in_the_last_place_past_one_trip_of_the_loop(lib):
    n = 3000
    first = [2999]
    big = list(range(1000, 1700)) + [2999]                  # 701 members: the clash is in the loop's third trip
    clean = list(range(0, 700))
    acc, taken = claim(lib, [first, big, clean], n)
    assert acc == [1, 0, 1]
    t = taken.cpu().numpy()
    assert t[:700].all() and not t[700:2999].any() and t[2999] == 1
    acc, _ = claim(lib, [big, first], n)
    assert acc == [1, 0]


def test_claim_taken_carries_over_and_no_candidates_is_a_no_op(lib):
    acc, taken = claim(lib, [[1, 2], [7]], 10)
    assert acc == [1, 1]
    acc, taken = claim(lib, [[2, 3], [4, 5], [5, 7]], 10, taken=taken)
    assert acc == [0, 1, 0]
    before = taken.clone()
    acc, taken = claim(lib, [], 10, taken=taken)
    assert acc == [] and torch.equal(before, taken)
    # no members, or a member that is no row: rejected, nothing marked
    acc, taken = claim(lib, [[], [10], [-1], [8]], 10, taken=taken)
    assert acc == [0, 0, 0, 1]


# ------------------------------------------------------------------ 4. qst_community_rescore
def test_rescore_is_the_fp64_cosine_and_ties_where_the_rows_tie(lib):
    e = np.random.RandomState(11).randn(50, 96).astype(np.float32)
    e[7] = 0.0
    a = np.random.RandomState(12).randint(0, 50, size=333).astype(np.int32)
    b = np.random.RandomState(13).randint(0, 50, size=333).astype(np.int32)
    a[:3], b[:3] = [5, 7, 7], [5, 7, 9]
    out = torch.full((334,), float(GUARD), dtype=torch.float64, device="cuda")
    ed, ad, bd = dev(e), torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    assert lib.qst_community_rescore(ed.data_ptr(), 50, 96, ad.data_ptr(), bd.data_ptr(), 333, out.data_ptr(), stream()) == 0
    out = out.cpu().numpy()
    np.testing.assert_allclose(out[:333], CC.cosine_ref(e)[a, b], rtol=0, atol=1e-13)
    assert out[333] == GUARD and out[1] == 0.0
    # +-1 rows: equal cosines are equal numbers, whatever the sign patterns
    p, thr, ms, _ = planted_ref("d96_k12")
    n = len(p)
    pa = np.repeat(np.arange(0, 20, dtype=np.int32), n)
    pb = np.tile(np.arange(n, dtype=np.int32), 20)
    pb[-1] = n                                              # not a row
    o2 = torch.empty(20 * n, dtype=torch.float64, device="cuda")
    pd, ad, bd = dev(p), torch.from_numpy(pa).cuda(), torch.from_numpy(pb).cuda()
    assert lib.qst_community_rescore(pd.data_ptr(), n, 96, ad.data_ptr(), bd.data_ptr(), 20 * n, o2.data_ptr(), stream()) == 0
    o2 = o2.cpu().numpy()
    assert np.isnan(o2[-1])
    np.testing.assert_allclose(o2[:-1], CC.cosine_ref(p)[pa[:-1], pb[:-1]], rtol=0, atol=1e-15)
    dots = (p.astype(np.int64) @ p.astype(np.int64).T)[pa[:-1], pb[:-1]]
    for d in np.unique(dots):
        assert len(np.unique(o2[:-1][dots == d])) == 1, d


# ------------------------------------------------------------------ 5. util.community_detection
@pytest.mark.parametrize("name", sorted(CC.PLANTED))
def test_community_detection_equals_the_oracle_list_for_list(name):
    e, thr, ms, want = planted_ref(name)
    got = util.community_detection(dev(e), threshold=thr, min_community_size=ms)
    assert got == want
    assert all(type(m) is int for c in got for m in c)


def test_community_detection_does_not_depend_on_chunk_budget_or_input_kind(monkeypatch):
    e, thr, ms, want = planted_ref("d96_k6")
    n = len(e)
    for chunk in (n, 64, 7):
        assert util.community_detection(dev(e), thr, ms, corpus_chunk_size=chunk) == want, chunk
    for kind in (torch.from_numpy(e), e, [torch.from_numpy(r) for r in e], e.astype(np.float64)):
        assert util.community_detection(kind, thr, ms, init_max_size=3) == want
    rounds = []
    plan = util.plan_community_round

    def counting_plan(*a):
        rounds.append(1)
        return plan(*a)
    monkeypatch.setattr(util, "plan_community_round", counting_plan)
    assert util.community_detection(dev(e), thr, ms) == want
    one_round = len(rounds)
    monkeypatch.setattr(util, "COMMUNITY_ROUND_MEMBERS", 1)  # one candidate a round
    assert util.community_detection(dev(e), thr, ms, corpus_chunk_size=64) == want
    assert one_round == 1 and len(rounds) - one_round >= len(want) > 1


def test_community_detection_pads_a_width_that_is_no_multiple_of_32():
    dim, k = 40, 5
    e = CC.planted([30, 20, 9], dim, k, 25, seed=3)
    thr = CC.threshold_for(k, dim)
    assert CC.margin(e, thr) >= 1e-3
    want, ncand, rejected = CC.community_ref(e, thr, 8, want_trace=True)
    assert len(want) >= 2 and rejected >= 1
    assert util.community_detection(dev(e), thr, 8) == want
    assert util.community_detection(dev(e), thr, len(e) + 1) == []


def test_community_detection_duplicates_tie_at_one_and_follow_by_row():
    rng = np.random.RandomState(2)
    e = rng.randn(16, 64).astype(np.float32)
    for r in (5, 6, 9, 11):
        e[r] = e[2]
    e[13] = e[3]
    got = util.community_detection(dev(e), threshold=0.9, min_community_size=2)
    assert got == [[2, 5, 6, 9, 11], [3, 13]]
    got = util.community_detection(dev(e), threshold=0.9, min_community_size=1)
    assert got[:2] == [[2, 5, 6, 9, 11], [3, 13]] and sorted(c[0] for c in got[2:]) == [0, 1, 4, 7, 8, 10, 12, 14, 15]
    assert all(len(c) == 1 for c in got[2:]) and [c[0] for c in got[2:]] == sorted(c[0] for c in got[2:])


def test_community_detection_zero_and_nan_rows_belong_to_nothing():
    e = np.zeros((6, 32), dtype=np.float32)
    e[0, 0] = e[2, 0] = 1.0
    e[2, 1] = 0.01
    e[4, 0] = 0.99
    e[3, 5] = np.nan
    assert util.community_detection(dev(e), 0.5, 1) == CC.community_ref(e, 0.5, 1) == [[0, 4, 2]]


def test_dropin_namespace_resolves_community_detection():
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
