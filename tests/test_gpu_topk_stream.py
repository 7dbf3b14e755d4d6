"""GPU: the streaming top-k -- qst_topk_merge_rows (merge one chunk of scores into a running top-k, ties decided by id,
self-exclusion, cap, fewer than k candidates), qst_topk_stream (prepare + score + merge over a corpus of any size) and what
stands on them: util.topk_stream, semantic_search, paraphrase_mining(_embeddings) and ParaphraseMiningEvaluator. The
yardstick is the full stable sort of tests/topk_stream_cases.py; wherever the scores are exact (small integers), the
result must equal it bit for bit and must not change with the way the columns are cut into chunks."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import topk_stream_cases as T  # noqa: E402
from kernel_helpers import lib, new_topk_state, real_case, real_rows, stream, topk_stream_call  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import _lib, util  # noqa: E402
from quadruplet_sentence_transformer_amd.evaluation import ParaphraseMiningEvaluator, paraphrase_metrics  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import SentenceTransformer  # noqa: E402

INF = float("inf")
new_state = new_topk_state


def merge(lib, s, k, cuts, col_base=0, row_base=0, exclude_self=0, max_score=INF, state=None):
    """s [rows, n] (numpy fp32) merged slice by slice, each slice a strided view of ONE device matrix (ld = n)."""
    rows, n = s.shape
    sd = torch.from_numpy(s).cuda()
    rs, ri = new_state(rows, k) if state is None else state
    for a, b in cuts:
        rc = lib.qst_topk_merge_rows(sd.data_ptr() + 4 * a, n, rows, b - a, col_base + a, row_base, exclude_self, max_score,
                                     k, rs.data_ptr(), ri.data_ptr(), stream())
        assert rc == 0
    return rs.cpu().numpy(), ri.cpu().numpy()


def same(got, want):
    np.testing.assert_array_equal(got[0], want[0])       # exact; a NaN equals a NaN in the same place
    np.testing.assert_array_equal(got[1], want[1])


# ------------------------------------------------------------------ 1. qst_topk_merge_rows
@pytest.mark.parametrize("k", [1, 3, 10, 100, 1000, 1024])
@pytest.mark.parametrize("n", [1, 7, 255, 256, 257, 1000, 5000])
def test_merge_rows_equals_the_full_sort_for_every_slicing(lib, n, k):
    for rows in (1, 5):
        s = T.hand_scores(rows, n, seed=n + k + rows)
        want = T.topk_ref(s, k, col_base=1000)
        for parts in (1, 2, 7):
            same(merge(lib, s, k, T.slices(n, parts), col_base=1000), want)


def test_merge_rows_more_than_k_copies_of_the_kth_value_across_two_slices(lib):
    k, n = 5, 40
    s = np.full((2, n), 1.0, dtype=np.float32)
    s[:, [3, 33]] = 9.0
    s[:, 10:31] = 7.0                                   # 21 copies of the value at the cut, on both sides of column 20
    want = T.topk_ref(s, k)
    np.testing.assert_array_equal(want[1][0], [3, 33, 10, 11, 12])
    same(merge(lib, s, k, [(0, 20), (20, 40)]), want)
    same(merge(lib, s, k, [(20, 40), (0, 20)]), want)   # the smaller ids win even when they arrive later
    same(merge(lib, s, k, [(0, 40)]), want)


@pytest.mark.parametrize("k", [10, 1024])
def test_merge_rows_all_values_equal(lib, k):
    s = np.full((3, 300), 0.5, dtype=np.float32)
    want = T.topk_ref(s, k, col_base=7)
    np.testing.assert_array_equal(want[1][0][:min(k, 300)], 7 + np.arange(min(k, 300)))
    for parts in (1, 2, 7):
        same(merge(lib, s, k, T.slices(300, parts), col_base=7), want)


def test_merge_rows_nan_ranks_above_inf(lib):
    s = T.hand_scores(2, 100, seed=3)
    s[0, 40], s[0, 70], s[1, 99], s[1, 0] = np.nan, np.inf, np.nan, -np.inf
    want = T.topk_ref(s, 4)
    assert np.isnan(want[0][0, 0]) and want[1][0, 0] == 40 and want[0][0, 1] == np.inf and want[1][0, 1] == 70
    for parts in (1, 2, 7):
        same(merge(lib, s, 4, T.slices(100, parts)), want)
    same(merge(lib, s, 100, T.slices(100, 2)), T.topk_ref(s, 100))      # -inf is a real entry and keeps its id
    assert T.topk_ref(s, 100)[1][1, -1] == 0


def test_merge_rows_exclude_self_drops_the_row_maximum(lib):
    rows, n, k, row_base, col_base = 5, 60, 6, 100, 98
    s = T.hand_scores(rows, n, seed=9)
    for r in range(rows):
        s[r, row_base + r - col_base] = 50.0             # the row's own column holds its maximum
    want = T.topk_ref(s, k, col_base=col_base, row_base=row_base, exclude_self=True)
    assert (want[0] < 50.0).all()
    for parts in (1, 2, 7):
        same(merge(lib, s, k, T.slices(n, parts), col_base=col_base, row_base=row_base, exclude_self=1), want)
    kept = merge(lib, s, k, T.slices(n, 2), col_base=col_base, row_base=row_base, exclude_self=0)
    same(kept, T.topk_ref(s, k, col_base=col_base, row_base=row_base))
    assert (kept[0][:, 0] == 50.0).all()


def test_merge_rows_cap_at_a_tied_value(lib):
    s = T.hand_scores(5, 500, seed=21)                   # values -3 .. 3, each about 70 times a row
    want = T.topk_ref(s, 100, max_score=2.0)
    assert want[0].max() == 2.0 and (want[0][:, 0] == 2.0).all()        # entries AT the cap take part, those above do not
    for parts in (1, 2, 7):
        same(merge(lib, s, 100, T.slices(500, parts), max_score=2.0), want)


def test_merge_rows_fewer_than_k_candidates_leave_a_padded_tail(lib):
    s = np.array([[3, 1, 3, 0, 3, -2, 3]], dtype=np.float32)
    want = T.topk_ref(s, 10, max_score=2.0)
    np.testing.assert_array_equal(want[1][0], [1, 3, 5] + [-1] * 7)
    assert (want[0][0, 3:] == -INF).all()
    for parts in (1, 2, 7):
        same(merge(lib, s, 10, T.slices(7, parts), max_score=2.0), want)
    # one column that is the row's own: nothing survives
    got = merge(lib, np.ones((1, 1), dtype=np.float32), 3, [(0, 1)], col_base=4, row_base=4, exclude_self=1)
    assert (got[0] == -INF).all() and (got[1] == -1).all()


def test_merge_rows_bad_arguments(lib):
    s = torch.zeros(2, 8, device="cuda")
    rs, ri = new_state(2, 4)
    before = (rs.clone(), ri.clone())
    f = lambda *a: lib.qst_topk_merge_rows(*a, stream())
    sp, op, ip = s.data_ptr(), rs.data_ptr(), ri.data_ptr()
    assert f(None, 8, 2, 8, 0, 0, 0, INF, 4, op, ip) == -1
    assert f(sp, 8, 2, 8, 0, 0, 0, INF, 4, None, ip) == -1
    assert f(sp, 8, 2, 8, 0, 0, 0, INF, 4, op, None) == -1
    assert f(sp, 4, 2, 8, 0, 0, 0, INF, 4, op, ip) == -1            # ld < n
    assert f(sp, 8, 0, 8, 0, 0, 0, INF, 4, op, ip) == -1
    assert f(sp, 8, 2, 0, 0, 0, 0, INF, 4, op, ip) == -1
    assert f(sp, 8, 2, 8, 0, 0, 0, INF, 0, op, ip) == -1
    assert f(sp, 8, 2, 8, -1, 0, 0, INF, 4, op, ip) == -1           # ids are not negative
    assert f(sp, 8, 2, 8, 0, -1, 0, INF, 4, op, ip) == -1
    assert f(sp, 8, 2, 8, 0, 0, 0, float("nan"), 4, op, ip) == -1
    assert f(sp, 8, 2, 8, 0, 0, 0, INF, 1025, op, ip) == -2         # k > 1024
    torch.cuda.synchronize()
    assert torch.equal(rs, before[0]) and torch.equal(ri, before[1])


# ------------------------------------------------------------------ 2. qst_topk_stream, exact
stream_call = topk_stream_call          # q, c: device fp32 [nq, dim], [nc, dim]
exact_scores = T.exact_scores


@pytest.mark.parametrize("dim", [32, 64])
@pytest.mark.parametrize("nq,nc", [(nq, nc) for nq in (1, 5, 130) for nc in (1, 7, 300, 2500)] + [(2050, 40)])
def test_stream_dot_on_ternary_rows_is_exact_for_every_chunk(lib, nq, nc, dim):
    q, c = T.ternary(nq, dim, seed=nq + nc), T.ternary(nc, dim, seed=7 * nq + nc + dim)
    full = exact_scores(q, c, dim)
    qd, cd = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    for k in (1, 10, 100):
        want = T.topk_ref(full, k)
        for chunk in sorted({1, 64, 257, nc}):
            rs, ri = stream_call(lib, qd, cd, k, 0, chunk)
            same((rs.cpu().numpy(), ri.cpu().numpy()), want)


@pytest.mark.parametrize("dim", [32, 64])
def test_stream_exclude_self_bases_and_a_second_corpus_piece(lib, dim):
    n, k = 300, 10
    e = T.ternary(n, dim, seed=5)
    e[17] = e[3]                                          # an exact duplicate: a tie with the self entry's score
    full = exact_scores(e, e, dim)
    ed = torch.from_numpy(e).cuda()
    # queries = corpus, both numbered from 1000: the diagonal (every row's maximum, dim or close) is dropped
    want = T.topk_ref(full, k, col_base=1000, row_base=1000, exclude_self=True)
    assert not (want[1] == 1000 + np.arange(n)[:, None]).any()
    for chunk in (1, 64, 257, n):
        rs, ri = stream_call(lib, ed, ed, k, 0, chunk, query_base=1000, corpus_base=1000, exclude_self=1)
        same((rs.cpu().numpy(), ri.cpu().numpy()), want)
    # the queries are rows 5 .. 104 of the corpus: query r is corpus row r + 5
    want = T.topk_ref(full[5:105], k, row_base=5, exclude_self=True)
    for chunk in (64, n):
        rs, ri = stream_call(lib, ed[5:105], ed, k, 0, chunk, query_base=5, exclude_self=1)
        same((rs.cpu().numpy(), ri.cpu().numpy()), want)
    # the corpus in two pieces, two calls: the state carries over, also through a cap
    for cap in (INF, 3.0):
        want = T.topk_ref(full, k, exclude_self=True, max_score=cap)
        for chunk in (64, 257):
            st = stream_call(lib, ed, ed[:170], k, 0, chunk, exclude_self=1, max_score=cap)
            rs, ri = stream_call(lib, ed, ed[170:], k, 0, chunk, corpus_base=170, exclude_self=1, max_score=cap, state=st)
            same((rs.cpu().numpy(), ri.cpu().numpy()), want)


def test_stream_bad_arguments(lib):
    q, c = torch.zeros(4, 32, device="cuda"), torch.zeros(9, 32, device="cuda")
    rs, ri = new_state(4, 3)
    need = lib.qst_topk_stream_workspace_bytes(4, 9, 32)
    assert need >= (4 + 12) * 32 * 4 + 4 * 12 * 4 and lib.qst_topk_stream_workspace_bytes(0, 9, 32) == 0
    # bounded by the chunk, not by the corpus
    assert lib.qst_topk_stream_workspace_bytes(100, 1000, 384) < lib.qst_topk_workspace_bytes(100, 100000, 384) // 50
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    qp, cp, op, ip, wp = q.data_ptr(), c.data_ptr(), rs.data_ptr(), ri.data_ptr(), ws.data_ptr()

    def f(qp=qp, cp=cp, nq=4, nc=9, dim=32, k=3, mode=0, chunk=9, qb=0, cb=0, ex=0, cap=INF, op=op, ip=ip, wp=wp, wb=need):
        return lib.qst_topk_stream(qp, cp, nq, nc, dim, k, mode, chunk, qb, cb, ex, cap, op, ip, wp, wb, stream())

    for bad in (dict(qp=None), dict(cp=None), dict(op=None), dict(ip=None), dict(wp=None), dict(nq=0), dict(nc=0),
                dict(dim=0), dict(k=0), dict(chunk=0), dict(mode=3), dict(qb=-1), dict(cb=-1), dict(cap=float("nan"))):
        assert f(**bad) == -1, bad
    assert f(k=1025) == -2 and f(dim=48) == -2
    assert f(wb=need - 1) == -3
    torch.cuda.synchronize()
    assert (ri == -1).all()
    assert f() == 0 and f(chunk=1000) == 0                # a chunk beyond the corpus is the corpus


# ------------------------------------------------------------------ 3. qst_topk_stream, real-valued
# The cases, their seeds (and how they were chosen), the tolerances and the cap: topk_stream_cases, shared with the one-shot
# tests; the rows themselves: kernel_helpers.real_rows.
REAL_CASES, REAL_SEED = T.REAL_CASES, T.REAL_SEED


@pytest.mark.parametrize("mode", ["cos", "dot", "euclid"])
@pytest.mark.parametrize("dim", [64, 384])
@pytest.mark.parametrize("nq,nc,k,chunk", REAL_CASES)
def test_stream_matches_the_fp64_ranking(lib, nq, nc, k, chunk, dim, mode):
    q, c, full, want_s, want_i = real_case(nq, nc, k, chunk, dim, mode)
    rs, ri = stream_call(lib, q.cuda(), c.cuda(), k, {"dot": 0, "cos": 1, "euclid": 2}[mode], chunk)
    n_bad = T.ranking_disagreements(rs.cpu().numpy(), ri.cpu().numpy(), full, want_i, T.real_tol(mode, want_s))
    assert n_bad <= T.real_cap(nq, k)


# ------------------------------------------------------------------ 4. the Python surface
def hits_arrays(hits, k):
    s = np.full((len(hits), k), -INF)
    i = np.full((len(hits), k), -1, dtype=np.int64)
    for r, row in enumerate(hits):
        assert len(row) <= k and all(set(h) == {"corpus_id", "score"} for h in row)
        assert all(type(h["corpus_id"]) is int and type(h["score"]) is float for h in row)
        s[r, :len(row)] = [h["score"] for h in row]
        i[r, :len(row)] = [h["corpus_id"] for h in row]
    return s, i


@pytest.mark.parametrize("fn,mode", [(util.cos_sim, "cos"), (util.dot_score, "dot"), (util.euclidean_score, "euclid")])
def test_semantic_search_with_the_built_in_score_functions(fn, mode):
    q, c = real_rows(40, 300, 64, seed=11)
    full = T.scores_ref(q.numpy(), c.numpy(), mode)
    want_s, want_i = T.topk_ref(full, 10)
    tol = (lambda s: 2e-6 * abs(s) + 1e-7) if mode == "euclid" else (lambda s: 2e-5 * float(np.abs(want_s).max()))
    for kw, qq, cc in ((dict(), q.cuda(), c.cuda()), (dict(query_chunk_size=3, corpus_chunk_size=64), q.cuda(), c.cuda()),
                       (dict(corpus_chunk_size=64), q.numpy(), c.numpy()), (dict(), list(q), c)):
        hits = util.semantic_search(qq, cc, score_function=fn, **kw)
        assert len(hits) == 40 and all(len(h) == 10 for h in hits)
        got_s, got_i = hits_arrays(hits, 10)
        assert T.ranking_disagreements(got_s, got_i, full, want_i, tol) <= 2
    one = util.semantic_search(q[0].cuda(), c.cuda(), top_k=3, score_function=fn)        # a 1-D query
    assert len(one) == 1 and [h["corpus_id"] for h in one[0]] == [int(x) for x in want_i[0, :3]]
    short = util.semantic_search(q[:2], c[:4], top_k=10, score_function=fn)              # top_k > nc: shorter lists
    assert [len(h) for h in short] == [4, 4]
    assert [h["corpus_id"] for h in short[1]] == [int(x) for x in T.topk_ref(full[1:2, :4], 4)[1][0]]


def test_semantic_search_with_a_callable_goes_through_merge_rows():
    q, c = T.ternary(40, 64, seed=1), T.ternary(300, 64, seed=2)
    full = exact_scores(q, c, 64)
    calls = []

    def fn(a, b):
        calls.append((tuple(a.shape), tuple(b.shape)))
        return a @ b.T                                     # integers: exact however the matrix is blocked

    want = T.topk_ref(full, 10)
    for kw in (dict(), dict(query_chunk_size=3), dict(corpus_chunk_size=64), dict(query_chunk_size=7, corpus_chunk_size=50)):
        calls.clear()
        hits = util.semantic_search(torch.from_numpy(q), c, score_function=fn, **kw)
        got_s, got_i = hits_arrays(hits, 10)
        np.testing.assert_array_equal(got_i, want[1])
        np.testing.assert_array_equal(got_s, want[0].astype(np.float64))
        nqc = -(-40 // kw.get("query_chunk_size", 100))
        ncc = -(-300 // kw.get("corpus_chunk_size", 500000))
        assert len(calls) == nqc * ncc and max(s[0][0] for s in calls) <= kw.get("query_chunk_size", 100)
    with pytest.raises(ValueError):
        util.semantic_search(q, c, score_function=lambda a, b: (a @ b.T)[:, :-1])
    with pytest.raises(ValueError):
        util.semantic_search(q, c, top_k=2000)


def test_topk_stream_wrapper_state_and_defaults():
    q, c = T.ternary(9, 40, seed=3), T.ternary(130, 40, seed=4)       # dim 40: zero-padded to 64
    full = exact_scores(q, c, 40)
    qd, cd = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    want = T.topk_ref(full, 200, col_base=50)
    st = util.topk_stream(qd, cd[:60], 200, mode="dot", chunk=32, corpus_base=50)
    rs, ri = util.topk_stream(qd, cd[60:], 200, mode="dot", chunk=32, corpus_base=110, state=st)
    assert rs.data_ptr() == st[0].data_ptr() and ri.data_ptr() == st[1].data_ptr()
    same((rs.cpu().numpy(), ri.cpu().numpy()), want)
    assert (ri[:, 130:] == -1).all()
    rs, ri = util.topk_stream(qd, cd, 5, mode="dot", max_score=4.0)
    same((rs.cpu().numpy(), ri.cpu().numpy()), T.topk_ref(full, 5, max_score=4.0))
    with pytest.raises(ValueError):
        util.topk_stream(qd, cd, 5, state=(rs[:, :4], ri[:, :4]))


def planted(seed=0):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(170, 64, generator=g)
    dup = base[:30] + 1e-3 * torch.randn(30, 64, generator=g)
    return torch.cat([base, dup], 0)


def is_sorted_pair_list(pairs):
    keys = [(-s, i, j) for s, i, j in pairs]
    return keys == sorted(keys) and all(i < j for _, i, j in pairs) and len({(i, j) for _, i, j in pairs}) == len(pairs)


def test_paraphrase_mining_embeddings_finds_the_planted_pairs():
    e = planted()
    pairs = util.paraphrase_mining_embeddings(e.cuda(), top_k=5)
    assert is_sorted_pair_list(pairs)
    assert all(type(s) is float and type(i) is int and type(j) is int for s, i, j in pairs)
    found = {(i, j) for _, i, j in pairs}
    assert all((t, 170 + t) in found for t in range(30))
    assert {(i, j) for _, i, j in pairs[:30]} == {(t, 170 + t) for t in range(30)}       # cosine ~ 1 - 5e-7: the best 30
    cut = util.paraphrase_mining_embeddings(e.cuda(), top_k=5, max_pairs=25)
    assert 13 <= len(cut) <= 25 and cut == pairs[:len(cut)]          # 25 candidates = both directions of 12.5 pairs or more
    host = util.paraphrase_mining_embeddings(e.numpy(), top_k=5, query_chunk_size=64, corpus_chunk_size=50)
    assert is_sorted_pair_list(host) and {(i, j) for _, i, j in host[:30]} == {(t, 170 + t) for t in range(30)}


@pytest.mark.parametrize("fn", [util.dot_score, lambda a, b: a @ b.T])
def test_paraphrase_mining_embeddings_does_not_depend_on_the_chunking(fn):
    e = T.ternary(200, 64, seed=8)
    e[170:] = e[:30]                                       # exact duplicates: score = |row|^2, tied with other pairs
    full = exact_scores(e, e, 64)
    ws, wi = T.topk_ref(full, 6, exclude_self=True)
    want = util.merge_mined_pairs(ws, np.repeat(np.arange(200), 6).reshape(200, 6), wi, 500000)
    got = [util.paraphrase_mining_embeddings(torch.from_numpy(e), top_k=6, query_chunk_size=qc, corpus_chunk_size=cc,
                                             score_function=fn) for qc, cc in ((5000, 200), (5000, 50), (33, 50))]
    assert got[0] == want and got[1] == want and got[2] == want
    assert is_sorted_pair_list(want) and len(want) >= 600


WORDS = ("a man rides red horse two dogs play in park woman eats green apple near old bridge small cat sleeps "
         "quick brown fox jumps over lazy river stone tower bright morning").split()


def sentence(seed, n):
    return " ".join(np.random.RandomState(seed).choice(WORDS, size=n))


def test_paraphrase_mining_and_the_evaluator_end_to_end(tmp_path):
    model = SentenceTransformer("tiny-bert", device="cuda")
    smap = {f"s{i}": sentence(i, 6 + i % 5) for i in range(40)}
    for t in range(8):                                     # eight paraphrases: one word appended
        smap[f"p{t}"] = smap[f"s{t}"] + " " + WORDS[t]
    dups = [(f"s{t}", f"p{t}") for t in range(8)] + [("s0", "s1"), ("s1", "nowhere")]
    sentences = list(smap.values())
    pairs = util.paraphrase_mining(model, sentences, batch_size=16, top_k=4)
    emb = model.encode(sentences, batch_size=16, convert_to_tensor=True)
    assert pairs == util.paraphrase_mining_embeddings(emb, top_k=4) and is_sorted_pair_list(pairs)
    full = T.scores_ref(emb.cpu().numpy(), emb.cpu().numpy(), "cos")
    assert all(abs(s - full[i, j]) <= 2e-5 for s, i, j in pairs)
    ev = ParaphraseMiningEvaluator(smap, duplicates_list=dups, top_k=4, batch_size=16, name="t")
    assert ev.total_num_duplicates == 9
    closed = ParaphraseMiningEvaluator(smap, duplicates_list=dups, add_transitive_closure=True, top_k=4, batch_size=16)
    assert closed.total_num_duplicates == 6 + 6            # {s0, p0, s1, p1}: 6 pairs, and six components of two
    mined = ev.mine(model)
    assert mined == pairs
    want = paraphrase_metrics(mined, ev.ids, ev.duplicates)
    ap = ev(model, output_path=str(tmp_path), epoch=2, steps=5)
    assert ap == want["average_precision"] and 0.0 < ap <= 1.0
    rows = open(os.path.join(str(tmp_path), ev.csv_file)).read().strip().splitlines()
    assert ev.csv_file == "paraphrase_mining_evaluation_t_results.csv" and len(rows) == 2
    assert rows[0].split(",") == ["epoch", "steps", "precision", "recall", "f1", "threshold", "average_precision"]
    got = rows[1].split(",")
    assert got[:2] == ["2", "5"]
    assert [float(x) for x in got[2:]] == [want[k] for k in ("precision", "recall", "f1", "threshold", "average_precision")]
    assert ev(model) == ap and len(os.listdir(str(tmp_path))) == 1                       # no output_path: nothing written
