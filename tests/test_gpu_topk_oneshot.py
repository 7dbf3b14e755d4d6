"""GPU: the one-shot retrieval entry points of csrc/retrieval.hip -- qst_topk_rows, qst_topk_scores, qst_topk_scores_capped,
qst_score_matrix, qst_normalize_rows -- held to the standard of the streaming path (tests/test_gpu_topk_stream.py): the
yardstick is the full stable sort of tests/topk_stream_cases.py, and wherever the scores are exact the result must equal it
bit for bit, IDS INCLUDED: every tie at the cut goes to the smaller id, a NaN of either sign ranks first and displaces
nothing, the two zeros tie. Beside that: padding that is poisoned, workspaces of exactly the size asked for between guard
bands and prefilled with either byte, outputs untouched by a refused call.

NaNs are built from int32 bit patterns and copied to the device as integers, so their sign and payload survive."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import topk_stream_cases as T  # noqa: E402
from kernel_helpers import lib, real_case, stream, topk_stream_call  # noqa: E402,F401

INF = float("inf")
QNAN, QNAN_NEG, SNAN, ALL_ONES = 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF
NAN_BITS = [QNAN, QNAN_NEG, SNAN, ALL_ONES]
MODES = {"dot": 0, "cos": 1, "euclid": 2}
BAND, GUARD = 4096, 0xA5


def dev_bits(a):
    """A numpy fp32 (or uint32) array on the device with its bits untouched: it travels as int32."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def guarded(nbytes, fill):
    """Exactly nbytes bytes of `fill` between two guard bands: (the whole uint8 tensor, the view of the middle)."""
    whole = torch.full((BAND + nbytes + BAND,), GUARD, dtype=torch.uint8, device="cuda")
    mid = whole[BAND:BAND + nbytes]
    mid.fill_(fill)
    return whole, mid


def guards_intact(whole):
    return bool((whole[:BAND] == GUARD).all()) and bool((whole[-BAND:] == GUARD).all())


def same(got, want):
    np.testing.assert_array_equal(got[0], want[0])       # exact; a NaN equals a NaN in the same place
    np.testing.assert_array_equal(got[1], want[1])


def rows_call(lib, s, k, ids=None, pad=0):
    """qst_topk_rows on s (numpy fp32 [rows, n]) with ld = n + pad. The pad columns of the scores hold NaN, those of the
    index_map (ids: int64 [rows, n] or None) 2**62: neither may be read."""
    rows, n = s.shape
    ld = n + pad
    sb = np.full((rows, ld), QNAN, dtype=np.uint32)
    sb[:, :n] = s.view(np.uint32)
    sd = dev_bits(sb)
    im = None
    if ids is not None:
        ib = np.full((rows, ld), 2 ** 62, dtype=np.int64)
        ib[:, :n] = ids
        im = torch.from_numpy(ib).cuda()
    out_s = torch.full((rows, k), 123.0, dtype=torch.float32, device="cuda")
    out_i = torch.full((rows, k), -7, dtype=torch.int64, device="cuda")
    rc = lib.qst_topk_rows(sd.data_ptr(), ld, None if im is None else im.data_ptr(), rows, n, k, out_s.data_ptr(),
                           out_i.data_ptr(), stream())
    assert rc == 0
    return out_s.cpu().numpy(), out_i.cpu().numpy()


def permuted_ids(rows, n, seed):
    rng = np.random.RandomState(seed)
    return np.stack([rng.permutation(n) for _ in range(rows)]).astype(np.int64) + 1000


# ------------------------------------------------------------------ 1. qst_topk_rows
@pytest.mark.parametrize("n,k", [(n, k) for n in (1, 7, 255, 256, 257, 1000, 5000) for k in (1, 3, 10, 100, 1000, 1024)
                                 if k <= n])
def test_rows_equals_the_full_sort_on_integer_scores(lib, n, k):
    s = T.hand_scores(33, n, seed=n + k)                 # every value tied many times at and around every cut
    same(rows_call(lib, s, k), T.topk_ref(s, k))


@pytest.mark.parametrize("n,k", [(1, 1), (7, 3), (257, 100), (1000, 10), (1000, 1000)])
def test_rows_poisoned_padding_is_not_read(lib, n, k):
    s = T.hand_scores(5, n, seed=3 * n + k)
    same(rows_call(lib, s, k, pad=5), T.topk_ref(s, k))
    ids = permuted_ids(5, n, seed=n)
    same(rows_call(lib, s, k, ids=ids, pad=5), T.topk_ref(s, k, ids=ids))


@pytest.mark.parametrize("n,k", [(7, 3), (257, 33), (1000, 100), (5000, 1024)])
def test_rows_ties_at_the_cut_go_to_the_smallest_ids_of_the_index_map(lib, n, k):
    s = T.hand_scores(9, n, seed=n - k)
    ids = permuted_ids(9, n, seed=k)
    want = T.topk_ref(s, k, ids=ids)
    same(rows_call(lib, s, k, ids=ids), want)
    for r in range(9):                                   # said directly: of the value at the cut, the smallest ids
        cut = want[0][r, -1]
        tied = np.sort(ids[r][s[r] == cut])
        got = rows_call(lib, s[r:r + 1], k, ids=ids[r:r + 1])
        np.testing.assert_array_equal(got[1][0][got[0][0] == cut], tied[:int((want[0][r] == cut).sum())])
    # ids far from zero, and negative ones: ranked by their distance from the smallest
    for base in (2 ** 40, -3000, -2 ** 62):
        far = ids + base
        same(rows_call(lib, s, k, ids=far), T.topk_ref(s, k, ids=far))


@pytest.mark.parametrize("k", [10, 1024])
def test_rows_all_values_equal(lib, k):
    s = np.full((3, 2000), 0.5, dtype=np.float32)
    want = T.topk_ref(s, k)
    np.testing.assert_array_equal(want[1][0], np.arange(k))
    same(rows_call(lib, s, k), want)


def test_rows_more_than_k_copies_of_the_kth_value(lib):
    s = np.full((2, 40), 1.0, dtype=np.float32)
    s[:, [3, 33]] = 9.0
    s[:, 10:31] = 7.0                                    # 21 copies of the value at the cut
    want = T.topk_ref(s, 5)
    np.testing.assert_array_equal(want[1][0], [3, 33, 10, 11, 12])
    same(rows_call(lib, s, 5), want)
    # 1500 copies spread over every wave and many trips of the row loop, 100 places for them
    s = T.hand_scores(4, 3000, seed=8)
    s[:, ::2] = 3.0                                      # the largest value of hand_scores
    s[:, [5, 1001, 2999]] = 9.0
    want = T.topk_ref(s, 103)
    assert (want[0][:, 3:] == 3.0).all() and (s == 3.0).sum(1).min() >= 1500
    same(rows_call(lib, s, 103), want)


def nan_checks(got, want, n_nan):
    same(got, want)
    vals, ids = got
    for r in range(len(ids)):
        assert np.isnan(vals[r][:n_nan]).all() and not np.isnan(vals[r][n_nan:]).any()     # the NaNs first ...
        assert (np.diff(ids[r][:n_nan]) > 0).all()                                         # ... by ascending id
        rest = vals[r][n_nan:]
        assert (rest[:-1] >= rest[1:]).all()                                               # the rest descending
        assert (ids[r] >= 0).all() and len(set(ids[r].tolist())) == len(ids[r])            # nothing lost, nothing twice


@pytest.mark.parametrize("nan_bits", NAN_BITS)
def test_rows_the_three_element_nan_case(lib, nan_bits):
    bits = np.array([[0.0, 0.896, -1.283]], dtype=np.float32).view(np.uint32).copy()
    bits[0, 0] = nan_bits
    s = T.f32_from_bits(bits)
    want = T.topk_ref(s, 3)
    np.testing.assert_array_equal(want[1], [[0, 1, 2]])
    nan_checks(rows_call(lib, s, 3), want, 1)
    nan_checks(rows_call(lib, s, 2), T.topk_ref(s, 2), 1)
    assert rows_call(lib, s, 1)[1][0, 0] == 0


def test_rows_nans_among_few_and_among_33(lib):
    bits = np.array([[1.5, 0, -2.0, 0, 0]], dtype=np.float32).view(np.uint32).copy()
    bits[0, [1, 3, 4]] = [QNAN_NEG, QNAN, ALL_ONES]                                  # k = 5 of n = 5, three NaNs
    s = T.f32_from_bits(bits)
    nan_checks(rows_call(lib, s, 5), T.topk_ref(s, 5), 3)
    for cols in ([17], [4, 30]):                                                      # k = n = 33: kp = 64, 31 empty slots
        for nan_bits in (QNAN, QNAN_NEG):
            bits = np.random.RandomState(len(cols)).randn(6, 33).astype(np.float32).view(np.uint32).copy()
            bits[:, cols] = nan_bits
            s = T.f32_from_bits(bits)
            nan_checks(rows_call(lib, s, 33), T.topk_ref(s, 33), len(cols))


@pytest.mark.parametrize("cols", [[3, 300, 620, 900], [64, 65, 70, 100]])
def test_rows_nans_of_every_bit_pattern_far_apart_and_inside_one_wave(lib, cols):
    rng = np.random.RandomState(sum(cols))
    bits = rng.randn(5, 1000).astype(np.float32).view(np.uint32).copy()
    bits[:, ::9] = bits[:, 4:5]                                                       # exact ties as well
    for r in range(5):
        bits[r, cols] = np.roll(np.array(NAN_BITS, dtype=np.uint32), r)
    s = T.f32_from_bits(bits)
    nan_checks(rows_call(lib, s, 100), T.topk_ref(s, 100), 4)
    ids = permuted_ids(5, 1000, seed=1)
    got, want = rows_call(lib, s, 100, ids=ids), T.topk_ref(s, 100, ids=ids)
    nan_checks(got, want, 4)
    nan_checks(rows_call(lib, s, 3), T.topk_ref(s, 3), 3)                             # fewer places than NaNs


def test_rows_the_two_zeros_tie_and_go_by_id(lib):
    bits = np.zeros((3, 600), dtype=np.uint32)
    bits[:, 1::2] = 0x80000000                                                        # +0.0, -0.0, +0.0, ...
    bits[1, ::3] = 0x80000000
    bits[:, [7, 400]] = np.float32(1.0).view(np.uint32)
    bits[:, [8, 500]] = np.float32(-1.0).view(np.uint32)
    bits[2, [100, 101]] = [0x00000001, 0x80000001]                                    # the denormals next to them do not tie
    s = T.f32_from_bits(bits)
    for k in (1, 2, 50, 300, 598, 600):
        want = T.topk_ref(s, k)
        got = rows_call(lib, s, k)
        same(got, want)                                                               # 0.0 == -0.0: the ids decide
    np.testing.assert_array_equal(rows_call(lib, s, 6)[1][0], [7, 400, 0, 1, 2, 3])


def test_rows_infinities_are_ordinary_entries(lib):
    s = T.hand_scores(4, 300, seed=2)
    s[:, [9, 200]] = np.inf
    s[:, [0, 150, 299]] = -np.inf
    s[3, 77] = np.nan
    for k in (1, 2, 3, 10, 298, 300):
        same(rows_call(lib, s, k), T.topk_ref(s, k))
    vals, ids = rows_call(lib, s, 300)
    np.testing.assert_array_equal(ids[0][-3:], [0, 150, 299])                         # -inf keeps its id: it is no empty slot
    assert (vals[:, -3:] == -INF).all() and (ids >= 0).all()


@pytest.mark.parametrize("n", [1024, 1025])
def test_rows_k_1024(lib, n):
    rng = np.random.RandomState(n)
    s = rng.randn(3, n).astype(np.float32)
    s[:, ::5] = s[:, 2:3]
    s[1] = np.round(s[1])
    same(rows_call(lib, s, 1024), T.topk_ref(s, 1024))


# ------------------------------------------------------------------ 2. qst_topk_scores / qst_topk_scores_capped
def scores_call(lib, qd, cd, k, mode, cap=None, ws_fill=None, short=0, prefill=None):
    """qst_topk_scores (cap None) or qst_topk_scores_capped on device rows. ws_fill: the workspace is exactly the size asked
    for, between guard bands, prefilled with that byte. Returns rc, scores, ids, whether the guards survived."""
    nq, dim = qd.shape
    nc = cd.shape[0]
    need = lib.qst_topk_workspace_bytes(nq, nc, dim)
    whole, ws = guarded(need, 0 if ws_fill is None else ws_fill)
    out_s = torch.full((nq, k), 123.0, dtype=torch.float32, device="cuda")
    out_i = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    if cap is None:
        rc = lib.qst_topk_scores(qd.data_ptr(), cd.data_ptr(), nq, nc, dim, k, mode, out_s.data_ptr(), out_i.data_ptr(),
                                 ws.data_ptr(), need - short, stream())
    else:
        rc = lib.qst_topk_scores_capped(qd.data_ptr(), cd.data_ptr(), nq, nc, dim, k, mode, cap, out_s.data_ptr(),
                                        out_i.data_ptr(), ws.data_ptr(), need - short, stream())
    torch.cuda.synchronize()
    return rc, out_s.cpu().numpy(), out_i.cpu().numpy(), guards_intact(whole)


def untouched(s, i):
    return bool((s == 123.0).all()) and bool((i == -7).all())


@pytest.mark.parametrize("dim", [32, 64])
@pytest.mark.parametrize("nq,nc", [(nq, nc) for nq in (1, 5, 130) for nc in (1, 7, 300, 2500)] + [(2050, 40)])
def test_scores_dot_on_ternary_rows_is_exact(lib, nq, nc, dim):
    q, c = T.ternary(nq, dim, seed=nq + nc), T.ternary(nc, dim, seed=7 * nq + nc + dim)
    full = T.exact_scores(q, c, dim)
    qd, cd = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    for k in sorted({min(k, nc) for k in (1, 10, 100)}):
        want = T.topk_ref(full, k)
        rc, s, i, ok = scores_call(lib, qd, cd, k, 0)
        assert rc == 0 and ok
        same((s, i), want)
        rs, ri = topk_stream_call(lib, qd, cd, k, 0, nc)                              # the streaming path in one chunk
        same((s, i), (rs.cpu().numpy(), ri.cpu().numpy()))


@pytest.mark.parametrize("dim", [32, 64])
def test_scores_capped(lib, dim):
    nq, nc, k = 5, 300, 100
    q, c = T.ternary(nq, dim, seed=4), T.ternary(nc, dim, seed=5 + dim)
    full = T.exact_scores(q, c, dim)
    qd, cd = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    vals, counts = np.unique(full[0], return_counts=True)
    tied = float(vals[np.argmax(counts)])                                             # the most frequent score of row 0
    assert counts.max() >= 10
    rc, s0, i0, _ = scores_call(lib, qd, cd, k, 0)
    assert rc == 0
    for cap in (INF, 3.0, 0.0, -(dim + 1.0), tied):
        want = T.topk_ref(full, k, max_score=cap)
        rc, s, i, ok = scores_call(lib, qd, cd, k, 0, cap=cap)
        assert rc == 0 and ok
        same((s, i), want)
        assert not (s > cap).any()
        if cap == INF:
            assert np.array_equal(s.view(np.uint32), s0.view(np.uint32)) and np.array_equal(i, i0)
        if cap == -(dim + 1.0):
            assert (s == -INF).all() and (i == -1).all()                              # nothing qualifies
    few = T.topk_ref(full, k, max_score=-4.0)
    assert ((few[1] == -1).sum(1) > 0).all() and ((few[1] >= 0).sum(1) > 0).all()     # a padded tail behind real entries
    rc, s, i, _ = scores_call(lib, qd, cd, k, 0, cap=-4.0)
    assert rc == 0
    same((s, i), few)
    rc, s, i, ok = scores_call(lib, qd, cd, k, 0, cap=float("nan"))                   # refused before any launch
    assert rc == -1 and ok and untouched(s, i)


@pytest.mark.parametrize("nc", [1, 7, 301])
def test_scores_all_negative_pad_columns_are_no_candidates(lib, nc):
    """The score block is pad4(nc) wide and its pad columns hold 0.0, above every real score here."""
    dim = 32
    q = np.ones((3, dim), dtype=np.float32)
    c = -np.abs(T.ternary(nc, dim, seed=nc))
    c[:, 0] = -1.0                                                                    # every score <= -1
    full = T.exact_scores(q, c, dim)
    assert full.max() < 0 and nc % 4 != 0
    for mode in (0, 1):
        rc, s, i, ok = scores_call(lib, torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda(), nc, mode)
        assert rc == 0 and ok and (i < nc).all() and (i >= 0).all() and (s < 0).all()
        if mode == 0:
            same((s, i), T.topk_ref(full, nc))
        else:
            assert all(sorted(r.tolist()) == list(range(nc)) for r in i)


def test_scores_cosine_with_a_zero_row_and_a_nan_row(lib):
    nq, nc, dim = 5, 50, 64
    g = torch.Generator().manual_seed(13)
    q, c = torch.randn(nq, dim, generator=g).numpy(), torch.randn(nc, dim, generator=g).numpy()
    c[10] = 0.0
    cb = c.view(np.uint32).copy()
    cb[20, 3] = QNAN_NEG                                                              # the NaN a host division leaves
    ref = c.copy()
    ref[20] = 0.0
    full = T.scores_ref(q, ref, "cos")
    rc, s, i, ok = scores_call(lib, torch.from_numpy(q).cuda(), dev_bits(cb).view(torch.float32), nc, 1)
    assert rc == 0 and ok
    for r in range(nq):
        assert i[r, 0] == 20 and np.isnan(s[r, 0]) and not np.isnan(s[r, 1:]).any()  # the NaN row first, for every query
        assert sorted(i[r].tolist()) == list(range(nc))                               # nothing lost
        assert (s[r, 1:-1] >= s[r, 2:]).all()
        at = int(np.where(i[r] == 10)[0][0])
        assert s[r, at] == 0.0                                                        # the zero row: exactly 0.0
        np.testing.assert_allclose(s[r, 1:], full[r][i[r, 1:]], rtol=0, atol=2e-5)
    rc, s3, i3, _ = scores_call(lib, torch.from_numpy(q).cuda(), dev_bits(cb).view(torch.float32), 3, 1)
    assert rc == 0 and np.array_equal(i3, i[:, :3])


@pytest.mark.parametrize("nq,nc,dim,k", [(5, 7, 32, 7), (130, 300, 64, 100)])
def test_scores_workspace_is_what_it_asks_for_and_stale_bytes_do_not_show(lib, nq, nc, dim, k):
    q, c = T.ternary(nq, dim, seed=1), T.ternary(nc, dim, seed=2)
    qd, cd = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    want = T.topk_ref(T.exact_scores(q, c, dim), k)
    for mode in (0, 1, 2):
        for cap in (None, 1.0):
            rc, s0, i0, ok0 = scores_call(lib, qd, cd, k, mode, cap=cap, ws_fill=0x00)
            rc1, s1, i1, ok1 = scores_call(lib, qd, cd, k, mode, cap=cap, ws_fill=0xFF)
            assert rc == 0 and rc1 == 0 and ok0 and ok1
            assert np.array_equal(s0.view(np.uint32), s1.view(np.uint32)) and np.array_equal(i0, i1)
            if mode == 0 and cap is None:
                same((s0, i0), want)
            rc, s, i, ok = scores_call(lib, qd, cd, k, mode, cap=cap, ws_fill=0xFF, short=1)
            assert rc == -3 and ok and untouched(s, i)


@pytest.mark.parametrize("mode", ["cos", "dot", "euclid"])
@pytest.mark.parametrize("dim", [64, 384])
@pytest.mark.parametrize("nq,nc,k,chunk", T.REAL_CASES)
def test_scores_match_the_fp64_ranking(lib, nq, nc, k, chunk, dim, mode):
    """The cases, seeds, tolerances and cap of test_stream_matches_the_fp64_ranking: both paths score through score_block."""
    q, c, full, want_s, want_i = real_case(nq, nc, k, chunk, dim, mode)
    k1 = min(k, nc)
    rc, s, i, ok = scores_call(lib, q.cuda(), c.cuda(), k1, MODES[mode])
    assert rc == 0 and ok
    n_bad = T.ranking_disagreements(s, i, full, want_i[:, :k1], T.real_tol(mode, want_s))
    assert n_bad <= T.real_cap(nq, k1)                   # k <= nc here: the cap of the positions that exist, never more


# ------------------------------------------------------------------ 3. qst_score_matrix
def matrix_call(lib, qd, cd, mode, ws_fill=0x00, short=0, ld=None, dim=None):
    """out [nq, ld] prefilled with NaN (0xFF bytes) between guard bands, the workspace as in scores_call."""
    nq, d = qd.shape
    nc = cd.shape[0]
    dim = d if dim is None else dim
    ld = (nc + 3) // 4 * 4 if ld is None else ld
    need = lib.qst_score_workspace_bytes(nq, nc, d)
    wwhole, ws = guarded(need, ws_fill)
    owhole, ob = guarded(nq * ld * 4, 0xFF)
    rc = lib.qst_score_matrix(qd.data_ptr(), cd.data_ptr(), nq, nc, dim, mode, ob.data_ptr(), ld, ws.data_ptr(), need - short,
                              stream())
    torch.cuda.synchronize()
    out = ob.cpu().numpy().view(np.float32).reshape(nq, ld)
    return rc, out, guards_intact(wwhole) and guards_intact(owhole)


@pytest.mark.parametrize("dim", [32, 64])
@pytest.mark.parametrize("nq", [1, 3, 2049])
@pytest.mark.parametrize("nc", [1, 5, 130])
def test_score_matrix_exact_values(lib, nq, nc, dim):
    q, c = T.ternary(nq, dim, seed=nq + dim), T.ternary(nc, dim, seed=nc)
    q[:, 0], c[:, 1] = 1.0, 1.0                                                       # no zero row by accident
    c[0] = q[nq - 1]                                                                  # an equal pair: (nq - 1, 0)
    if nc > 1:
        c[nc - 1] = 0.0                                                               # a zero corpus row
    if nq > 1:
        q[0] = 0.0                                                                    # a zero query row
    qd, cd = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    rc, out, ok = matrix_call(lib, qd, cd, 0)
    assert rc == 0 and ok
    np.testing.assert_array_equal(out[:, :nc], T.exact_scores(q, c, dim))             # dot: the integer matrix
    rc, out, ok = matrix_call(lib, qd, cd, 1)
    assert rc == 0 and ok
    np.testing.assert_allclose(out[:, :nc], T.scores_ref(q, c, "cos"), rtol=0, atol=2e-5)
    if nc > 1:
        assert (out[:, nc - 1].view(np.uint32) << 1 == 0).all()                       # cosine with a zero row: exactly 0.0
    if nq > 1:
        assert (out[0, :nc] == 0.0).all()
    rc, out, ok = matrix_call(lib, qd, cd, 2)
    assert rc == 0 and ok
    want = T.scores_ref(q, c, "euclid")
    np.testing.assert_allclose(out[:, :nc], want, rtol=2e-6, atol=1e-7)
    equal = (q[:, None, :] == c[None, :, :]).all(-1) if nq * nc * dim < 4e7 else None
    assert out[nq - 1, 0] == 1.0                                                      # euclid of equal rows: exactly 1.0
    if equal is not None:
        assert (out[:, :nc][equal] == 1.0).all()


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("nq,nc,dim", [(3, 5, 32), (130, 7, 64), (2049, 130, 32)])
def test_score_matrix_layout_workspace_and_refusals(lib, nq, nc, dim, mode):
    q, c = T.ternary(nq, dim, seed=11), T.ternary(nc, dim, seed=12)
    qd, cd = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    ld = (nc + 3) // 4 * 4
    rc, out0, ok0 = matrix_call(lib, qd, cd, mode, ws_fill=0x00)
    rc1, out1, ok1 = matrix_call(lib, qd, cd, mode, ws_fill=0xFF)
    assert rc == 0 and rc1 == 0 and ok0 and ok1                                       # nothing past row nq, nothing outside ws
    assert np.array_equal(out0.view(np.uint32), out1.view(np.uint32))                 # stale workspace bytes do not show
    assert not np.isnan(out0).any()                                                   # every element of out was written
    assert ld == nc or (out0[:, nc:].view(np.uint32) == 0).all()                      # the pad columns: exactly 0.0
    rc, out, ok = matrix_call(lib, qd, cd, mode, ws_fill=0xFF, short=1)
    assert rc == -3 and ok and np.isnan(out).all()
    for bad_ld in (nc if ld != nc else ld + 4, ld + 4, ld - 4):
        rc, out, ok = matrix_call(lib, qd, cd, mode, ld=max(bad_ld, 1))
        assert rc == -2 and ok and np.isnan(out).all()
    rc, out, ok = matrix_call(lib, qd, cd, mode, dim=dim - 8)                         # dim % 32 != 0
    assert rc == -2 and ok and np.isnan(out).all()
    rc, out, ok = matrix_call(lib, qd, cd, 3)
    assert rc == -1 and ok and np.isnan(out).all()


# ------------------------------------------------------------------ 4. qst_normalize_rows
def normalize_call(lib, x, in_place=False):
    """x numpy fp32 [n, dim]; the output (or, in place, x itself) sits between guard bands. Returns rc, out, guards intact."""
    n, dim = x.shape
    whole, ob = guarded(n * dim * 4, 0xFF)
    xd = torch.from_numpy(x).cuda()
    if in_place:
        ob.copy_(xd.view(-1).view(torch.uint8))
        rc = lib.qst_normalize_rows(ob.data_ptr(), n, dim, ob.data_ptr(), stream())
    else:
        rc = lib.qst_normalize_rows(xd.data_ptr(), n, dim, ob.data_ptr(), stream())
    torch.cuda.synchronize()
    return rc, ob.cpu().numpy().view(np.float32).reshape(n, dim), guards_intact(whole)


def normalize_ref(x):
    x64 = x.astype(np.float64)
    return x64 / np.maximum(np.linalg.norm(x64, axis=1, keepdims=True), 1e-12)


@pytest.mark.parametrize("dim", [1, 3, 63, 64, 65, 384, 1000])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1000])
def test_normalize_rows_matches_fp64(lib, n, dim):
    x = np.random.RandomState(n + dim).randn(n, dim).astype(np.float32) * 1.7
    if n >= 3:
        u = x[1:3].astype(np.float64)
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        x[0] = 0.0                                                                    # a zero row gives zeros
        x[1] = (u[0] * 1e-20).astype(np.float32)                                      # norm 1e-20: the clamp branch
        x[2] = (u[1] * 1e15).astype(np.float32)                                       # norm 1e15
    rc, out, ok = normalize_call(lib, x)
    assert rc == 0 and ok                                                             # rows past n untouched
    np.testing.assert_allclose(out, normalize_ref(x), rtol=1e-6, atol=1e-7)
    if n >= 3:
        assert (out[0] == 0.0).all()
        np.testing.assert_allclose(out[1], x[1].astype(np.float64) * 1e12, rtol=1e-6, atol=0)
        assert abs(float(np.linalg.norm(out[2].astype(np.float64))) - 1.0) < 1e-6
    rc, out2, ok = normalize_call(lib, x, in_place=True)
    assert rc == 0 and ok and np.array_equal(out.view(np.uint32), out2.view(np.uint32))


def test_normalize_rows_bad_arguments(lib):
    x = torch.ones(4, 8, device="cuda")
    o = torch.full((4, 8), 5.0, device="cuda")
    f = lambda *a: lib.qst_normalize_rows(*a, stream())
    assert f(None, 4, 8, o.data_ptr()) == -1
    assert f(x.data_ptr(), 4, 8, None) == -1
    assert f(x.data_ptr(), 0, 8, o.data_ptr()) == -1
    assert f(x.data_ptr(), -1, 8, o.data_ptr()) == -1
    assert f(x.data_ptr(), 4, 0, o.data_ptr()) == -1
    torch.cuda.synchronize()
    assert (o == 5.0).all()
