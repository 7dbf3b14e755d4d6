"""GPU: retrieval scoring + top-k kernels (libqst qst_topk_rows / qst_topk_scores) against the fp64 oracle, and the
InformationRetrievalEvaluator end to end (encode -> score -> top-k across corpus chunks -> metrics) against the same
metrics computed by the oracle from the model's own embeddings. The last section holds the Python
surface to the order the kernels promise (tests/test_gpu_topk_oneshot.py checks the entry points themselves): duplicate
documents rank by corpus position for every chunking, a host-style NaN of a foreign score function ranks first and no empty
slot is looked up as a document, duplicated mining candidates come back in id order."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import topk_stream_cases as T  # noqa: E402
from quadruplet_sentence_transformer_amd import _lib, evaluation, util  # noqa: E402
from quadruplet_sentence_transformer_amd.evaluation import InformationRetrievalEvaluator  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import SentenceTransformer  # noqa: E402
from oracle import ir_oracle  # noqa: E402


@pytest.mark.parametrize("rows,n,k", [(1, 1, 1), (3, 10, 1), (5, 100, 100), (4, 1000, 10), (2, 50000, 100),
                                      (3, 5000, 1024), (7, 257, 33)])
def test_topk_rows_matches_a_full_sort(rows, n, k):
    g = torch.Generator().manual_seed(rows * 1000 + n + k)
    s = torch.randn(rows, n, generator=g)
    if n >= 100:
        s[:, ::7] = s[:, 3:4]                         # many exact ties
        s[0, 5] = float("inf")
        s[-1, 11] = -float("inf")
    sd = s.cuda()
    vals, idx = util.topk_rows(sd, k)
    order = np.lexsort((np.broadcast_to(np.arange(n), (rows, n)), -s.numpy().astype(np.float64)), axis=1)[:, :k]
    want = np.take_along_axis(s.numpy(), order, axis=1)
    np.testing.assert_array_equal(vals.cpu().numpy(), want)                       # bit-exact values, sorted
    got_idx = idx.cpu().numpy()
    np.testing.assert_array_equal(np.take_along_axis(s.numpy(), got_idx, axis=1), want)   # indices point at them
    for r in range(rows):
        assert len(set(got_idx[r].tolist())) == k                                 # no element taken twice
        strictly = want[r] > want[r][-1]                                          # above the cut: the choice is forced
        np.testing.assert_array_equal(got_idx[r][strictly], order[r][strictly])
    np.testing.assert_array_equal(got_idx, order)             # ... and AT the cut it is the smaller index: the full sort
    # index_map translates columns into caller ids
    imap = torch.arange(n, dtype=torch.int64).flip(0).repeat(rows, 1).cuda() + 1000
    vals2, idx2 = util.topk_rows(sd, k, index_map=imap)
    np.testing.assert_array_equal(vals2.cpu().numpy(), want)
    np.testing.assert_array_equal(np.take_along_axis(s.numpy(), (n - 1) - (idx2.cpu().numpy() - 1000), axis=1), want)
    # the ids are the columns reversed: among equal scores the smaller ID is the LARGER column, also at the cut
    np.testing.assert_array_equal(idx2.cpu().numpy(), T.topk_ref(s.numpy(), k, ids=imap.cpu().numpy())[1])


def test_topk_rows_bad_arguments():
    lib = _lib.load()
    s = torch.zeros(2, 8, device="cuda")
    o, i = torch.empty(2, 9, device="cuda"), torch.empty(2, 9, dtype=torch.int64, device="cuda")
    st = _lib.current_stream_ptr()
    assert lib.qst_topk_rows(s.data_ptr(), 8, None, 2, 8, 9, o.data_ptr(), i.data_ptr(), st) == -2      # k > n
    assert lib.qst_topk_rows(s.data_ptr(), 4, None, 2, 8, 2, o.data_ptr(), i.data_ptr(), st) == -1      # ld < n
    assert lib.qst_topk_rows(None, 8, None, 2, 8, 2, o.data_ptr(), i.data_ptr(), st) == -1


@pytest.mark.parametrize("nq,nc,dim,k,cosine", [(5, 37, 64, 10, True), (33, 1001, 384, 100, True), (7, 300, 128, 5, False),
                                                (2100, 2500, 64, 3, True), (1, 64, 768, 64, False)])
def test_topk_scores_matches_fp64_ranking(nq, nc, dim, k, cosine):
    g = torch.Generator().manual_seed(nq + nc + dim)
    q = torch.randn(nq, dim, generator=g)
    c = torch.randn(nc, dim, generator=g) * (0.5 + torch.rand(nc, 1, generator=g))     # varied norms
    vals, idx = util.topk_scores(q.cuda(), c.cuda(), k, cosine=cosine)
    want_s, want_i = ir_oracle.rank(q.numpy(), c.numpy(), k, cosine)
    scale = 1.0 if cosine else float(np.abs(want_s).max())
    np.testing.assert_allclose(vals.cpu().numpy(), want_s, rtol=0, atol=2e-5 * scale)     # split-bf16 x3 products
    got_i = idx.cpu().numpy()
    # the same documents, except where two candidates are closer than the arithmetic can tell apart
    gap_ok = 0
    for r in range(nq):
        if np.array_equal(got_i[r], want_i[r]):
            continue
        full = ir_oracle.rank(q.numpy()[r:r + 1], c.numpy(), nc, cosine)[0][0]
        pos = {int(d): p for p, d in enumerate(ir_oracle.rank(q.numpy()[r:r + 1], c.numpy(), nc, cosine)[1][0])}
        for a, b in zip(got_i[r], want_i[r]):
            if a != b:
                assert abs(full[pos[int(a)]] - full[pos[int(b)]]) < 4e-5 * scale
                gap_ok += 1
    assert gap_ok <= max(2, nq * k // 200)


@pytest.mark.parametrize("nq,nc,dim,k", [(5, 37, 64, 10), (33, 1001, 384, 100), (130, 300, 96, 7), (1, 64, 768, 64)])
def test_topk_scores_euclid_matches_fp64_ranking(nq, nc, dim, k):
    """mode 'euclid' = the reference's euclidean_score (models/evaluators.py:392-405). Near-duplicates of the queries are
    planted in the corpus: their distances (1e-3 .. 1e-1 at norm ~ sqrt(dim)) are what a |q|^2+|c|^2-2qc formulation
    would lose; the direct-difference kernel must rank them as float64 does."""
    g = torch.Generator().manual_seed(nq * 7 + nc + dim)
    q = torch.randn(nq, dim, generator=g)
    c = torch.randn(nc, dim, generator=g) * (0.5 + torch.rand(nc, 1, generator=g))
    ndup = min(nq, nc // 3, 8)
    for t in range(ndup):
        c[3 * t] = q[t] + 10.0 ** (-3 + 2 * t / max(1, ndup - 1)) * torch.randn(dim, generator=g) / dim ** 0.5
    vals, idx = util.topk_scores(q.cuda(), c.cuda(), k, mode="euclid")
    want_s, want_i = ir_oracle.rank(q.numpy(), c.numpy(), k, "euclid")
    np.testing.assert_allclose(vals.cpu().numpy(), want_s, rtol=2e-6, atol=1e-7)      # fp32 FMA chain + sqrt + rcp
    got_i = idx.cpu().numpy()
    full = ir_oracle.scores(q.numpy(), c.numpy(), "euclid")
    for r in range(nq):
        for a, b in zip(got_i[r], want_i[r]):
            assert a == b or abs(full[r, a] - full[r, b]) < 1e-6, (r, a, b)
    for t in range(ndup):
        assert got_i[t, 0] == 3 * t                                                    # the planted near-duplicate wins


@pytest.mark.parametrize("nq,nc,dim", [(3, 5, 32), (17, 130, 384), (2, 9, 100)])
def test_score_functions_match_fp64(nq, nc, dim):
    """util.cos_sim / dot_score / euclidean_score as functions (qst_score_matrix); dim 100 exercises the zero padding."""
    g = torch.Generator().manual_seed(nq + nc + dim)
    q = torch.randn(nq, dim, generator=g) * 1.3
    c = torch.randn(nc, dim, generator=g) * 0.7 + 0.1
    for fn, mode, tol in ((util.cos_sim, "cos", 2e-5), (util.dot_score, "dot", None), (util.euclidean_score, "euclid", 1e-6)):
        want = ir_oracle.scores(q.numpy(), c.numpy(), mode)
        got = fn(q.cuda(), c.cuda())
        assert got.is_cuda and tuple(got.shape) == (nq, nc)
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=tol if tol else 2e-5 * float(np.abs(want).max()))
        host = fn(q, c)                                     # host tensors in -> host tensor out, same arithmetic
        assert not host.is_cuda and torch.equal(host, got.cpu())
    one = util.cos_sim(q[0], c[1])                          # 1-D inputs are rows, as in sentence_transformers.util
    assert tuple(one.shape) == (1, 1)


class _HashTexts:
    """Deterministic pseudo-sentences over a small vocabulary (the synthetic tokenizer hashes words to ids)."""
    words = ("a man rides red horse two dogs play in park woman eats green apple near old bridge small cat sleeps "
             "quick brown fox jumps over lazy river stone tower bright morning").split()

    @classmethod
    def make(cls, seed, n):
        rng = np.random.RandomState(seed)
        return " ".join(rng.choice(cls.words, size=n))


@pytest.mark.parametrize("preset,chunk", [("tiny-bert", 50000), ("tiny-bert", 17), ("tiny-mpnet", 40)])
def test_ir_evaluator_end_to_end(tmp_path, preset, chunk):
    model = SentenceTransformer(preset, device="cuda")
    corpus = {f"d{i}": _HashTexts.make(i, 5 + i % 9) for i in range(90)}
    queries, relevant = {}, {}
    rng = np.random.RandomState(7)
    for qn in range(23):
        base = rng.randint(0, 90)
        queries[f"q{qn}"] = corpus[f"d{base}"] + " " + _HashTexts.make(1000 + qn, 2)     # a perturbed corpus sentence
        relevant[f"q{qn}"] = {f"d{base}", f"d{(base + 1) % 90}"}
    queries["unused"] = "no relevant documents"                                          # dropped by the constructor
    ks = dict(mrr_at_k=[10], ndcg_at_k=[10], accuracy_at_k=[1, 3, 5, 10], precision_recall_at_k=[1, 3, 5, 10], map_at_k=[30])
    ev = InformationRetrievalEvaluator(queries, corpus, relevant, corpus_chunk_size=chunk, name="t", batch_size=16, **ks)
    got = ev.compute_metrices(model)
    # oracle: the same embeddings (fp32 from encode), ranked and scored on the CPU in float64
    q_emb = model.encode(ev.queries, batch_size=16, convert_to_numpy=True)
    c_emb = model.encode(ev.corpus, batch_size=16, convert_to_numpy=True)
    for name, cosine in (("cos_sim", True), ("dot_score", False)):
        _, order = ir_oracle.rank(q_emb, c_emb, 30, cosine)
        ranked = [[ev.corpus_ids[j] for j in row] for row in order]
        want = ir_oracle.metrics(ranked, [relevant[q] for q in ev.queries_ids], ks["mrr_at_k"], ks["ndcg_at_k"],
                                 ks["accuracy_at_k"], ks["precision_recall_at_k"], ks["map_at_k"])
        for metric in want:
            for k in want[metric]:
                assert got[name][metric][k] == pytest.approx(want[metric][k], abs=1e-9), (name, metric, k)
    score = ev(model, output_path=str(tmp_path), epoch=1, steps=2)
    assert score == pytest.approx(max(got[n]["map@k"][30] for n in ("cos_sim", "dot_score")), abs=1e-12)
    rows = open(os.path.join(str(tmp_path), ev.csv_file)).read().strip().splitlines()
    assert len(rows) == 2 and rows[0].split(",") == ev.csv_headers and rows[1].startswith("1,2,")


def _reference_euclidean_score(a, b):
    """models/evaluators.py:392-405 restated (the reference module cannot be imported offline): a foreign callable."""
    a = a if isinstance(a, torch.Tensor) else torch.tensor(a)
    b = b if isinstance(b, torch.Tensor) else torch.tensor(b)
    a = a.unsqueeze(0) if a.dim() == 1 else a
    b = b.unsqueeze(0) if b.dim() == 1 else b
    return 1 / (1 + torch.cdist(a, b, p=2))


def test_score_function_resolution_is_by_behaviour():
    from quadruplet_sentence_transformer_amd.evaluation import resolve_score_function
    assert resolve_score_function("euclid_score", _reference_euclidean_score, "cuda") == ("native", 2)
    assert resolve_score_function("whatever", lambda a, b: a @ b.T, "cuda") == ("native", 0)
    custom = lambda a, b: -torch.cdist(a, b, p=1)                                  # Manhattan: none of the native modes
    assert resolve_score_function("cos_sim", custom, "cuda") == ("callable", custom)    # the NAME does not decide
    cpu_only = lambda a, b: torch.tensor(np.asarray(a.cpu()) @ np.asarray(b.cpu()).T)   # returns a host tensor
    assert resolve_score_function("np_dot", cpu_only, "cuda") == ("native", 0)
    broken = lambda a, b: (_ for _ in ()).throw(RuntimeError("no probe"))
    assert resolve_score_function("x", broken, "cuda") == ("callable", broken)


@pytest.mark.parametrize("chunk", [50000, 17])
def test_ir_evaluator_with_the_reference_score_functions(tmp_path, chunk):
    """Exactly the dictionary training/main.py:57 / ir_evauation_script.py:71 build, through the constructor call of
    models/evaluators.py:572-588, on one and on several corpus chunks; plus a custom callable under a stock name."""
    model = SentenceTransformer("tiny-bert", device="cuda")
    corpus = {f"d{i}": _HashTexts.make(i, 5 + i % 9) for i in range(90)}
    queries, relevant = {}, {}
    rng = np.random.RandomState(5)
    for qn in range(19):
        base = rng.randint(0, 90)
        queries[f"q{qn}"] = corpus[f"d{base}"] + " " + _HashTexts.make(2000 + qn, 2)
        relevant[f"q{qn}"] = {f"d{base}", f"d{(base + 3) % 90}"}
    manhattan = lambda a, b: -torch.cdist(a, b, p=1)
    score_functions = {"cos_sim": util.cos_sim, "dot_score": util.dot_score, "euclid_score": _reference_euclidean_score,
                       "manhattan": manhattan}
    ks = dict(mrr_at_k=[10], ndcg_at_k=[10], accuracy_at_k=[1, 3, 5, 10], precision_recall_at_k=[1, 3, 5, 10], map_at_k=[100])
    ev = InformationRetrievalEvaluator(queries=queries, corpus=corpus, relevant_docs=relevant, corpus_chunk_size=chunk,
                                       show_progress_bar=False, batch_size=32, name="exp", write_csv=True,
                                       score_functions=score_functions, main_score_function=None, **ks)
    got = ev.compute_metrices(model)
    assert ev._resolved["euclid_score"] == ("native", 2) and ev._resolved["manhattan"][0] == "callable"
    q_emb = model.encode(ev.queries, batch_size=32, convert_to_numpy=True)
    c_emb = model.encode(ev.corpus, batch_size=32, convert_to_numpy=True)
    man = -np.abs(q_emb.astype(np.float64)[:, None, :] - c_emb.astype(np.float64)[None, :, :]).sum(-1)
    for name, mode in (("cos_sim", "cos"), ("dot_score", "dot"), ("euclid_score", "euclid"), ("manhattan", None)):
        s = man if mode is None else ir_oracle.scores(q_emb, c_emb, mode)
        order = np.lexsort((np.broadcast_to(np.arange(s.shape[1]), s.shape), -s), axis=1)[:, :90]
        ranked = [[ev.corpus_ids[j] for j in row] for row in order]
        want = ir_oracle.metrics(ranked, [relevant[q] for q in ev.queries_ids], ks["mrr_at_k"], ks["ndcg_at_k"],
                                 ks["accuracy_at_k"], ks["precision_recall_at_k"], ks["map_at_k"])
        for metric in want:
            for k in want[metric]:
                assert got[name][metric][k] == pytest.approx(want[metric][k], abs=1e-9), (name, metric, k)
    score = ev(model, output_path=str(tmp_path), epoch=0, steps=5)
    assert score == pytest.approx(max(got[n]["map@k"][100] for n in score_functions), abs=1e-12)
    rows = open(os.path.join(str(tmp_path), ev.csv_file)).read().strip().splitlines()
    assert rows[0].split(",") == ev.csv_headers and "euclid_score-MAP@100" in rows[0]


def test_hard_negative_mining_matches_brute_force():
    """for every reference the k most similar candidates among those with cosine <= threshold
    (the reference's NEG_EXAMPLE_SIM_TRESHOLD filter + hard_contrastive_sampling), all references in one pass."""
    g = torch.Generator().manual_seed(11)
    R_, C_, D, k, thr = 37, 500, 128, 6, 0.05
    q = torch.randn(R_, D, generator=g)
    c = torch.randn(C_, D, generator=g)
    c[:40] = q[:1] + 0.3 * torch.randn(40, D, generator=g)          # near-duplicates of reference 0: must be filtered
    idx, sc = util.mine_hard_negatives(q.cuda(), c.cuda(), k, threshold=thr)
    qn = (q / q.norm(dim=1, keepdim=True)).double()
    cn = (c / c.norm(dim=1, keepdim=True)).double()
    s = (qn @ cn.T).numpy()
    for r in range(R_):
        ok = np.where(s[r] <= thr)[0]
        want = ok[np.argsort(-s[r][ok], kind="stable")][:k]
        got = idx[r].cpu().numpy()
        np.testing.assert_allclose(sc[r].cpu().numpy()[:len(want)], s[r][want], rtol=0, atol=2e-5)
        assert float(sc[r].max()) <= thr + 1e-6
        assert set(got[:len(want)].tolist()) == set(want.tolist()) or np.allclose(s[r][got[:len(want)]], s[r][want], atol=4e-5)
    assert not (set(idx[0].cpu().tolist()) & set(range(40)))       # the paraphrase-like candidates never come back
    # fewer qualifying candidates than k -> padded with (-1, -inf)
    idx2, sc2 = util.mine_hard_negatives(q[:2].cuda(), c[:3].cuda(), 5, threshold=-0.99)
    assert (idx2 == -1).all() and torch.isinf(sc2).all()
    # sentences + embedder
    model = SentenceTransformer("tiny-bert", device="cuda")
    refs = [_HashTexts.make(i, 7) for i in range(5)]
    cands = [_HashTexts.make(100 + i, 6) for i in range(30)]
    i3, s3 = util.mine_hard_negatives(refs, cands, 4, threshold=0.9, embedder=model)
    e_r, e_c = model.encode(refs, convert_to_tensor=True), model.encode(cands, convert_to_tensor=True)
    i4, s4 = util.mine_hard_negatives(e_r, e_c, 4, threshold=0.9)
    assert torch.equal(i3, i4) and torch.allclose(s3, s4)
    with pytest.raises(ValueError):
        util.mine_hard_negatives(refs, cands, 4)


# ------------------------------------------------------------------ exact ties and NaNs through the Python surface
class _NoNegativeIndex(list):
    """corpus_ids that refuses what list[-1] would silently answer with the LAST document."""

    def __getitem__(self, i):
        assert i >= 0, f"corpus_ids[{i}]: an empty top-k slot was looked up as a document"
        return list.__getitem__(self, i)


def _fp64_dot(a, b):
    """A foreign callable: a @ b.T accumulated in fp64 and rounded once, so that the score of a duplicated document has the
    same bits wherever its column lies and however the corpus is chunked (an fp32 matmul may pick another kernel per shape)."""
    return (a.double() @ b.double().T).float()


def _duplicate_corpus(model, max_k=10):
    """90 documents and 23 queries on `model`, with duplicate documents planted from the fp64 ranking of the model's own
    embeddings: for some queries the document at the LAST place of the top max_k gets a copy at least 40 positions away
    (another chunk at chunk sizes 17 and 40), before or after it in turn, so that the two tie exactly across the cut; for
    others (in turn) the document at the third place, so that both copies are inside. A copy repeats the text and, so that it is
    bit-identical whatever batch it was encoded in, the embedding row. Of a pair only the copy with the LARGER position is
    relevant: the wrong choice at the cut changes every metric. Returns queries, corpus, relevant, corpus embeddings
    (device), query embeddings (numpy), the pairs."""
    corpus = {f"d{i}": _HashTexts.make(i, 5 + i % 9) for i in range(90)}
    rng = np.random.RandomState(7)
    queries, bases = {}, []
    for qn in range(23):
        base = rng.randint(0, 90)
        queries[f"q{qn}"] = corpus[f"d{base}"] + " " + _HashTexts.make(1000 + qn, 2)
        bases.append(base)
    q_emb = model.encode(list(queries.values()), batch_size=16, convert_to_numpy=True)
    c = model.encode(list(corpus.values()), batch_size=16, convert_to_numpy=True).copy()
    used, pairs, relevant = set(), [], {f"q{qn}": {f"d{bases[qn]}"} for qn in range(23)}
    for t, qn in enumerate(range(0, 23, 2)):
        s = ir_oracle.scores(q_emb[qn:qn + 1], c, "dot")[0]
        order = np.lexsort((np.arange(90), -s))
        j1 = int(order[max_k - 1] if t % 2 == 0 else order[2])
        far = [j for j in range(90) if abs(j - j1) >= 40 and j not in used and j not in bases
               and j not in order[:max_k + 2].tolist()]
        far = [j for j in far if (j < j1) == (t % 4 < 2)] or far
        if j1 in used or not far:
            continue
        j2 = far[len(far) // 2]
        c[j2] = c[j1]
        corpus[f"d{j2}"] = corpus[f"d{j1}"]
        used |= {j1, j2}
        pairs.append((qn, j1, j2))
        relevant[f"q{qn}"].add(f"d{max(j1, j2)}")
    return queries, corpus, relevant, torch.from_numpy(c).cuda(), q_emb, pairs


def _hits_per_function(monkeypatch, ev, model, c_dev):
    """compute_metrices with the hit lists it hands to ir_metrics recorded: ({name: metrics}, {name: hit lists})."""
    seen, real = [], evaluation.ir_metrics
    monkeypatch.setattr(evaluation, "ir_metrics", lambda results, *a, **kw: (seen.append(results), real(results, *a, **kw))[1])
    got = ev.compute_metrices(model, corpus_embeddings=c_dev)
    monkeypatch.setattr(evaluation, "ir_metrics", real)
    assert len(seen) == len(ev.score_function_names)
    return got, dict(zip(ev.score_function_names, seen))


def _hit_arrays(ev, hits, k):
    pos = {cid: j for j, cid in enumerate(ev.corpus_ids)}
    s = np.full((len(hits), k), -np.inf, dtype=np.float64)
    i = np.full((len(hits), k), -1, dtype=np.int64)
    for r, row in enumerate(hits):
        s[r, :len(row)] = [h["score"] for h in row]
        i[r, :len(row)] = [pos[h["corpus_id"]] for h in row]
    return s, i


def test_ir_evaluator_duplicate_documents_rank_by_corpus_position_for_every_chunking(monkeypatch):
    model = SentenceTransformer("tiny-bert", device="cuda")
    queries, corpus, relevant, c_dev, q_emb, pairs = _duplicate_corpus(model)
    c64 = c_dev.cpu().numpy()
    ks = dict(mrr_at_k=[10], ndcg_at_k=[10], accuracy_at_k=[1, 3, 5, 10], precision_recall_at_k=[1, 3, 5, 10], map_at_k=[10])
    fns = {"cos_sim": util.cos_sim, "dot_score": util.dot_score, "foreign": _fp64_dot}
    mode = {"cos_sim": "cos", "dot_score": "dot", "foreign": "dot"}
    # the yardstick first: exact ties across the cut and inside the list do occur (fp64 scores of identical rows are equal)
    full = {nm: ir_oracle.scores(q_emb, c64, mode[nm]) for nm in fns}
    want = {nm: T.topk_ref(full[nm], 11) for nm in fns}
    across = sum(1 for r in range(23) if want["dot_score"][0][r, 9] == want["dot_score"][0][r, 10])
    inside = sum(1 for r in range(23) if (np.diff(want["dot_score"][0][r, :10]) == 0).any())
    assert len(pairs) >= 6 and across >= 3 and inside >= 2, (pairs, across, inside)
    runs = {}
    for chunk in (17, 40, len(corpus)):
        ev = InformationRetrievalEvaluator(queries, corpus, relevant, corpus_chunk_size=chunk, batch_size=16, score_functions=fns,
                                           **ks)
        ev._resolved = {"cos_sim": ("native", 1), "dot_score": ("native", 0), "foreign": ("callable", _fp64_dot)}
        ev.corpus_ids = _NoNegativeIndex(ev.corpus_ids)
        runs[chunk] = _hits_per_function(monkeypatch, ev, model, c_dev)
    got, hits = runs[len(corpus)]
    for chunk in (17, 40):
        assert runs[chunk][1] == hits, chunk                  # the same hit lists, ids and score bits, for every chunking
        assert runs[chunk][0] == got, chunk                   # ... and so every metric
    for nm in fns:
        assert all(len(h) == 10 for h in hits[nm])
        gs, gi = _hit_arrays(ev, hits[nm], 10)
        wi = want[nm][1][:, :10]
        scale = float(np.abs(full[nm]).max())
        n_bad = T.ranking_disagreements(gs, gi, full[nm], wi, lambda s: 2e-5 * scale)
        assert n_bad <= 2
        for r, p in zip(*np.where(gi != wi)):                 # two ids may trade places only where fp32 cannot tell them apart
            assert full[nm][r, gi[r, p]] != full[nm][r, wi[r, p]], (nm, r, p)      # ... never where they tie exactly
        ranked = [[h["corpus_id"] for h in row] for row in hits[nm]]
        mw = ir_oracle.metrics(ranked, [relevant[q] for q in ev.queries_ids], ks["mrr_at_k"], ks["ndcg_at_k"],
                               ks["accuracy_at_k"], ks["precision_recall_at_k"], ks["map_at_k"])
        for metric in mw:
            for k in mw[metric]:
                assert got[nm][metric][k] == pytest.approx(mw[metric][k], abs=1e-9), (nm, metric, k)
    for qn, j1, j2 in pairs:                                  # said directly for the planted pairs, on the exact callable
        ids = [int(x) for x in _hit_arrays(ev, hits["foreign"], 10)[1][qn]]
        if max(j1, j2) in ids:
            assert ids.index(min(j1, j2)) + 1 == ids.index(max(j1, j2)), (qn, j1, j2, ids)


def test_ir_evaluator_host_style_nans_of_a_foreign_callable(monkeypatch):
    """A NaN with the sign bit set (0xFFC00000: what inf - inf and 0 / 0 give on the host) in a few cells of a foreign score
    matrix: those documents rank first, by corpus position, nothing else is displaced and no id -1 is looked up."""
    model = SentenceTransformer("tiny-bert", device="cuda")
    queries, corpus, relevant, c_dev, q_emb, pairs = _duplicate_corpus(model)
    _, j1, j2 = pairs[0]
    lone = next(j for j in range(90) if all(j not in p[1:] for p in pairs))
    poison = [(c_dev[j1].clone(), [0, 1, 2]), (c_dev[lone].clone(), [1, 5])]          # a duplicated document and a single one

    def nan_fn(a, b):
        out = _fp64_dot(a, b)
        bits = out.view(torch.int32)
        for row, qrows in poison:
            for col in (b == row).all(1).nonzero().flatten().tolist():
                bits[qrows, col] = -4194304                                           # 0xFFC00000
        return out

    q_dev = torch.from_numpy(q_emb).cuda()
    whole = nan_fn(q_dev, c_dev).cpu().numpy()
    assert whole.view(np.uint32)[1, lone] == 0xFFC00000 and np.isnan(whole[0, [j1, j2]]).all()
    want_s, want_i = T.topk_ref(whole, 10)
    np.testing.assert_array_equal(want_i[1, :3], sorted([j1, j2, lone]))
    ks = dict(mrr_at_k=[10], ndcg_at_k=[10], accuracy_at_k=[1, 10], precision_recall_at_k=[1, 10], map_at_k=[10])
    for chunk in (17, 40, 90):
        ev = InformationRetrievalEvaluator(queries, corpus, relevant, corpus_chunk_size=chunk, batch_size=16,
                                           score_functions={"foreign": nan_fn}, **ks)
        ev._resolved = {"foreign": ("callable", nan_fn)}
        ev.corpus_ids = _NoNegativeIndex(ev.corpus_ids)
        _, hits = _hits_per_function(monkeypatch, ev, model, c_dev)
        gs, gi = _hit_arrays(ev, hits["foreign"], 10)
        np.testing.assert_array_equal(gi, want_i)                                     # every id the yardstick's, in its order
        np.testing.assert_array_equal(gs, want_s.astype(np.float64))
        assert (gi >= 0).all()


def test_hard_negative_mining_duplicated_candidates_come_back_in_id_order():
    g = torch.Generator().manual_seed(17)
    R_, C_, D, k = 12, 700, 128, 6
    q = torch.randn(R_, D, generator=g)
    qn, c = q.numpy(), torch.randn(C_, D, generator=g).numpy()
    # a threshold no score comes near: the widest gap between two fp64 scores in (0, 0.1), so that fp32 scores (within 2e-5)
    # qualify exactly when the fp64 ones do. Copying a candidate row adds no new score value to any reference's row.
    v = np.sort(ir_oracle.scores(qn, c, "cos").ravel())
    v = v[(v > 0.0) & (v < 0.1)]
    at = int(np.argmax(np.diff(v)))
    thr = float(0.5 * (v[at] + v[at + 1]))
    assert v[at + 1] - v[at] > 1e-4
    used, across, inside = set(), [], []
    for r in range(R_):                                   # from the fp64 ranking: a copy of the row's last (or second) choice
        s = ir_oracle.scores(qn[r:r + 1], c, "cos")[0]
        order = [int(j) for j in np.lexsort((np.arange(C_), -s)) if s[j] <= thr]
        j1 = order[k - 1] if r % 2 == 0 else order[1]
        far = [j for j in range(C_) if abs(j - j1) > 256 and j not in used and j not in order[:k + 2]]
        far = [j for j in far if (j < j1) == (r % 4 < 2)] or far
        if j1 in used:
            continue
        j2 = far[len(far) // 3]                           # more than 256 columns away: another trip of the row loop
        c[j2] = c[j1]
        used |= {j1, j2}
        (across if r % 2 == 0 else inside).append((r, min(j1, j2), max(j1, j2)))
    full = ir_oracle.scores(qn, c, "cos")
    want_s, want_i = T.topk_ref(full, k + 1, max_score=thr)
    across = [(r, a, b) for r, a, b in across if want_i[r, k - 1] == a and want_i[r, k] == b]     # still tied across the cut
    inside = [(r, a, b) for r, a, b in inside if a in want_i[r, :k] and b in want_i[r, :k]]
    assert len(across) >= 3 and len(inside) >= 3
    idx, sc = util.mine_hard_negatives(q.cuda(), torch.from_numpy(c).cuda(), k, threshold=thr)
    gi, gs = idx.cpu().numpy(), sc.cpu().numpy()
    assert T.ranking_disagreements(gs, gi, full, want_i[:, :k], lambda s: 2e-5) <= 2
    for r, a, b in across:
        assert gi[r, k - 1] == a and b not in gi[r]       # of the two tied at the last place, the smaller id
    for r, a, b in inside:
        pa = gi[r].tolist().index(a)
        assert gi[r, pa + 1] == b and gs[r, pa].tobytes() == gs[r, pa + 1].tobytes()
    # fewer qualifying candidates than k: the duplicates in id order, then the documented tail (-1, -inf)
    small = c[:8].copy()
    s = ir_oracle.scores(qn[:1], small, "cos")[0]
    by = np.argsort(s)
    small[by[7]] = small[by[1]]                           # the second-lowest candidate copied over the highest
    s = ir_oracle.scores(qn[:1], small, "cos")[0]
    u = np.unique(s)
    assert len(u) == 7 and u[2] - u[1] > 1e-3 and s[by[1]] == s[by[7]] == u[1]
    thr2 = float(0.5 * (u[1] + u[2]))                     # three qualify: the lowest and the two copies
    idx2, sc2 = util.mine_hard_negatives(q[:1].cuda(), torch.from_numpy(small).cuda(), 6, threshold=thr2)
    np.testing.assert_array_equal(idx2.cpu().numpy()[0], [min(by[1], by[7]), max(by[1], by[7]), by[0], -1, -1, -1])
    assert (sc2[0, 3:] == -float("inf")).all() and sc2[0, 0] == sc2[0, 1] and (sc2[0, :3] <= thr2).all()
