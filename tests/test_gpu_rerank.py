"""GPU: qst_rerank_scores and qst_rerank_metrics (csrc/rerank.hip) against the yardstick in rerank_helpers -- a stable sort
and a walk per group, the average precision as sklearn takes it -- and evaluation.RerankingEvaluator on top of them: its
one encode, its scoring paths, its CSV file and a fit() that selects by it.

The reciprocal rank is compared for equality of the doubles; the average precision within P * 2^-52 and NDCG@k within
4 k * 2^-52 of the yardstick's fp64 values (rerank_helpers.ap_bound, ndcg_bound); a score within (D + 8) * 2^-24 of its
scale from fp64 numpy."""
import csv
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import rerank_helpers as RH  # noqa: E402
from kernel_helpers import lib, ptr, stream  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import evaluation, st_losses as S, util  # noqa: E402
from quadruplet_sentence_transformer_amd.evaluation import RerankingEvaluator  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample, SentenceTransformer  # noqa: E402

MODES = {"cos": util.SCORE_COS, "dot": util.SCORE_DOT, "euclid": util.SCORE_EUCLID}


def metrics_call(lib, scores, offsets, num_pos, k, ws=None, nd=None):
    """lib.qst_rerank_metrics on device tensors: (per_query [nq, 3], out [5]) as numpy doubles."""
    nq, nd = num_pos.numel(), scores.numel() if nd is None else nd
    nbytes = lib.qst_rerank_workspace_bytes(nq, nd)
    assert nbytes == 16 * nd + (4 * nq + 15) // 16 * 16
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    per_query = torch.full((nq, 3), -7.0, dtype=torch.float64, device="cuda")
    out = torch.full((5,), -7.0, dtype=torch.float64, device="cuda")
    rc = lib.qst_rerank_metrics(ptr(scores), ptr(offsets), ptr(num_pos), nq, nd, k, ptr(per_query), ptr(out), ptr(ws), nbytes,
                                stream())
    assert rc == 0
    return per_query.cpu().numpy(), out.cpu().numpy()


def on_device(case):
    return tuple(torch.from_numpy(x).cuda() for x in case)


_ALONE = {}


def alone(lib, kind, name):
    """One case -- a kind over a size set -- with the yardstick and the kernel's output for every k: computed once, left
    unchanged."""
    if (kind, name) not in _ALONE:
        case = RH.case(kind, RH.SIZE_SETS[name], RH.case_seed(kind, name))
        dev = on_device(case)
        _ALONE[(kind, name)] = (case, {k: (RH.expected(*case, k), *metrics_call(lib, *dev, k)) for k in RH.KS})
    return _ALONE[(kind, name)]


def check(what, num_pos, k, want, per_query, out):
    nq = len(num_pos)
    d_ap, d_ndcg = np.abs(per_query[:, RH.AP] - want[:, RH.AP]), np.abs(per_query[:, RH.NDCG] - want[:, RH.NDCG])
    print(f"  {what} k={k}: nq {nq}; worst |d ap| / bound {(d_ap / [RH.ap_bound(int(p)) for p in num_pos]).max():.3f}, "
          f"worst |d ndcg| / bound {(d_ndcg / RH.ndcg_bound(k)).max():.3f}; means {out[:3].tolist()} want "
          f"{want.mean(axis=0).tolist()}; counts {out[3:].tolist()}")
    assert np.array_equal(per_query[:, RH.RR], want[:, RH.RR]), what
    assert (d_ap <= [RH.ap_bound(int(p)) for p in num_pos]).all(), what
    assert (d_ndcg <= RH.ndcg_bound(k)).all(), what
    for c in (RH.RR, RH.AP, RH.NDCG):
        assert abs(out[c] - want[:, c].mean()) <= RH.mean_bound(num_pos, k, c), (what, c)
    assert out[3] == 0 and out[4] == 0


# ------------------------------------------------------------------ 1. the metrics against the yardstick
@pytest.mark.parametrize("name", list(RH.SIZE_SETS))
@pytest.mark.parametrize("kind", RH.KINDS)
def test_metrics_equal_the_yardstick(lib, kind, name):
    (scores, offsets, num_pos), by_k = alone(lib, kind, name)
    for k in RH.KS:
        check(f"{kind} {name}", num_pos, k, *by_k[k])
    P, N = RH.SIZE_SETS[name][0]
    if name != "ragged" and kind == "flat":         # the tie rule: the first document, a positive, is ranked first
        rr, ap, ndcg = by_k[10][1][0]
        assert rr == 1.0 and ndcg == 1.0 and abs(ap - P / (P + N)) <= RH.ap_bound(P)
    if name != "ragged" and kind == "pos_last":
        assert by_k[10][1][0, RH.RR] == (0.0 if N >= 10 else 1.0 / (N + 1))


@pytest.mark.parametrize("kind", RH.KINDS)
def test_single_groups_in_one_call_keep_their_bits(lib, kind):
    names = [n for n in RH.SIZE_SETS if n != "ragged"]
    cases = [alone(lib, kind, n)[0] for n in names]
    scores = np.concatenate([c[0] for c in cases])
    num_pos = np.concatenate([c[2] for c in cases])
    offsets = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])]).astype(np.int64)
    assert len(num_pos) == 10
    dev = on_device((scores, offsets, num_pos))
    for k in RH.KS:
        per_query, out = metrics_call(lib, *dev, k)
        check(f"{kind} ten groups", num_pos, k, RH.expected(scores, offsets, num_pos, k), per_query, out)
        for g, n in enumerate(names):
            assert per_query[g].tobytes() == alone(lib, kind, n)[1][k][1][0].tobytes(), (n, k)


# ------------------------------------------------------------------ 2. the scores
def embeddings(D, seed):
    """(queries [nq, D], docs [nd, D], offsets, group of every document) over the ragged mix, fp32 on the host: every
    document at a distance of 1.25 .. 4.25 from its query; group 3's query and document 1 are zero rows."""
    rng = np.random.RandomState(seed)
    sizes = np.array([P + N for P, N in RH.SIZE_SETS["ragged"]])
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    gid = np.repeat(np.arange(len(sizes)), sizes)
    q = rng.randn(len(sizes), D).astype(np.float32)
    delta = rng.randn(len(gid), D)
    delta *= ((1.25 + 3.0 * rng.rand(len(gid))) / np.linalg.norm(delta, axis=1))[:, None]
    d = (q[gid] + delta).astype(np.float32)
    return q, d, offsets, gid


@pytest.mark.parametrize("D", [1, 33, 384, 1000])
@pytest.mark.parametrize("mode", list(MODES))
def test_scores_equal_fp64_numpy(lib, mode, D):
    q, d, offsets, gid = embeddings(D, 100 + D)
    if mode == "cos":
        q[3] = 0.0
        d[1] = 0.0
    q64, d64 = q.astype(np.float64)[gid], d.astype(np.float64)
    eps = (D + 8) * 2.0 ** -24
    if mode == "cos":
        want = (q64 * d64).sum(1) / (np.maximum(np.linalg.norm(q64, axis=1), 1e-12) * np.maximum(np.linalg.norm(d64, axis=1), 1e-12))
        bound = np.full(len(gid), eps)
    elif mode == "dot":
        want = (q64 * d64).sum(1)
        bound = eps * (np.abs(q64) * np.abs(d64)).sum(1)
    else:
        dist = np.linalg.norm(q64 - d64, axis=1)
        assert (dist >= 1.0).all()
        want = 1.0 / (1.0 + dist)
        bound = np.full(len(gid), eps)
    dq, dd, doff = on_device((q, d, offsets))
    got = torch.full((len(gid),), float("nan"), dtype=torch.float32, device="cuda")
    rc = lib.qst_rerank_scores(ptr(dq), ptr(dd), ptr(doff), len(q), len(gid), D, MODES[mode], ptr(got), stream())
    assert rc == 0
    got = got.cpu().numpy()
    err = np.abs(got.astype(np.float64) - want)
    print(f"  {mode} D={D}: nd {len(gid)}; worst error / bound {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert np.isfinite(got).all() and (err <= bound).all()
    if mode == "cos":
        assert got[1] == 0.0 and (got[offsets[3]:offsets[4]] == 0.0).all()
    # the wrapper: host offsets are checked and moved, a device tensor goes through; the same launch, the same bits
    assert util.rerank_scores(dq, dd, offsets, mode).cpu().numpy().tobytes() == got.tobytes()
    assert util.rerank_scores(dq, dd, doff, MODES[mode]).cpu().numpy().tobytes() == got.tobytes()
    # rows that do not start on 16 bytes take the element-wise walk: the same scores within the same bound
    if D % 4 == 0:
        shifted = torch.empty(dd.numel() + 1, dtype=torch.float32, device="cuda")[1:].view_as(dd).copy_(dd)
        assert shifted.data_ptr() % 16 == 4
        walked = torch.empty(len(gid), dtype=torch.float32, device="cuda")
        rc = lib.qst_rerank_scores(ptr(dq), ptr(shifted), ptr(doff), len(q), len(gid), D, MODES[mode], ptr(walked), stream())
        assert rc == 0
        assert (np.abs(walked.cpu().numpy().astype(np.float64) - want) <= bound).all()


# ------------------------------------------------------------------ 3. determinism
def test_same_inputs_give_the_same_bits(lib):
    (scores, offsets, num_pos), by_k = alone(lib, "ties", "ragged")
    dev = on_device((scores, offsets, num_pos))
    want_pq, want_out = by_k[10][1:]
    pq, out = metrics_call(lib, *dev, 10)
    assert pq.tobytes() == want_pq.tobytes() and out.tobytes() == want_out.tobytes()
    # what the workspace held before does not matter
    ws = torch.full((lib.qst_rerank_workspace_bytes(len(num_pos), len(scores)),), 0xFF, dtype=torch.uint8, device="cuda")
    pq, out = metrics_call(lib, *dev, 10, ws=ws)
    assert pq.tobytes() == want_pq.tobytes() and out.tobytes() == want_out.tobytes()
    # nor which stream runs it
    q, d, off, gid = embeddings(33, 7)
    dq, dd, doff = on_device((q, d, off))
    first = util.rerank_scores(dq, dd, doff, "cos")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert stream() == side.cuda_stream
        pq, out = metrics_call(lib, *dev, 10)
        second = util.rerank_scores(dq, dd, doff, "cos")
        pq2, out2 = util.rerank_metrics(dev[0], dev[1], dev[2], 10)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert pq.tobytes() == want_pq.tobytes() and out.tobytes() == want_out.tobytes()
    assert pq2.cpu().numpy().tobytes() == want_pq.tobytes() and out2.cpu().numpy().tobytes() == want_out.tobytes()
    assert second.cpu().numpy().tobytes() == first.cpu().numpy().tobytes()


# ------------------------------------------------------------------ 4. groups the kernel cannot use, scores without a rank
def test_invalid_groups_are_counted_and_left_out(lib):
    groups = [(2, 5), (1, 70), (3, 4), (64, 64), (2, 6), (1, 3)]
    scores, offsets, num_pos = RH.case("ties", groups, 77)
    nd = len(scores)
    want = RH.expected(scores, offsets, num_pos, 10)
    bad_pos, bad_off = num_pos.copy(), offsets.copy()
    bad_pos[2] = 0                                      # no positive
    bad_pos[4] = 8                                      # nothing but positives
    bad_off[6] = nd + 5                                 # the last group runs past the scores, which stay nd long
    dev = on_device((scores, bad_off, bad_pos))
    per_query, out = metrics_call(lib, *dev, 10, nd=nd)
    valid = [0, 1, 3]
    print(f"  per_query {per_query.tolist()} out {out.tolist()}")
    assert out[4] == 3 and out[3] == 0
    assert (per_query[[2, 4, 5]] == 0.0).all()
    assert np.array_equal(per_query[valid, RH.RR], want[valid, RH.RR])
    assert (np.abs(per_query[valid, RH.AP] - want[valid, RH.AP]) <= [RH.ap_bound(int(num_pos[g])) for g in valid]).all()
    assert (np.abs(per_query[valid, RH.NDCG] - want[valid, RH.NDCG]) <= RH.ndcg_bound(10)).all()
    for c in (RH.RR, RH.AP, RH.NDCG):
        assert abs(out[c] - want[valid, c].mean()) <= RH.mean_bound(num_pos[valid], 10, c)
    # a group with a negative start, and one that is empty
    for g, lo, hi in ((0, -1, 7), (2, 78, 78)):
        off = offsets.copy()
        off[g], off[g + 1] = lo, hi
        pq, o = metrics_call(lib, *on_device((scores, off, num_pos)), 10)
        assert o[4] >= 1 and (pq[g] == 0.0).all()
    # the wrapper hands device tensors through: the count is the caller's to read
    pq, o = util.rerank_metrics(dev[0], dev[1][:6].contiguous(), dev[2][:5].contiguous(), 10)
    assert pq.shape == (5, 3) and o.cpu().numpy()[4] == 2


def test_non_finite_scores_are_counted(lib):
    groups = [(2, 5), (1, 70), (3, 4)]
    scores, offsets, num_pos = RH.case("gauss", groups, 78)
    scores[4] = np.nan                                  # a negative of group 0
    scores[offsets[1] + 40] = np.inf                    # a negative of group 1
    per_query, out = metrics_call(lib, *on_device((scores, offsets, num_pos)), 10)
    assert out[3] == 2 and out[4] == 0
    scores[offsets[2]] = -np.inf                        # the first positive of group 2
    per_query, out = metrics_call(lib, *on_device((scores, offsets, num_pos)), 10)
    assert out[3] == 3 and out[4] == 0


# ------------------------------------------------------------------ 5. the evaluator
WORDS = ("a man rides red horse two dogs play in park woman eats green apple near old bridge small cat sleeps under tall "
         "tree while rain falls on quiet town boats cross wide river").split()


def sent(i, n):
    rng = np.random.RandomState(i)
    return " ".join(rng.choice(WORDS, size=n))


def rerank_samples(n=12):
    """n samples with 1 - 3 positives and 2 - 9 negatives out of a pool of 40 sentences: texts repeat across the samples (a
    query is another sample's document), never inside one."""
    rng = np.random.RandomState(21)
    pool = [sent(i, 4 + i % 7) for i in range(40)]
    assert len(set(pool)) == 40
    samples = []
    for i in range(n):
        P, N = 1 + i % 3, 2 + (5 * i) % 8
        pick = rng.choice(40, size=1 + P + N, replace=False)
        samples.append({"query": pool[pick[0]], "positive": [pool[j] for j in pick[1:1 + P]],
                        "negative": [pool[j] for j in pick[1 + P:]]})
    return samples


@pytest.fixture(scope="module")
def model():
    m = SentenceTransformer("tiny-bert", device="cuda")
    m.eval()
    return m


def read_csv(path):
    with open(path) as f:
        return list(csv.reader(f))


def flat_embeddings(model, ev):
    """(queries, docs) of the evaluator's samples from encode() -- one call over the distinct texts, as the evaluator makes
    it -- laid out as the evaluator lays them out, on the device."""
    queries = [s["query"] for s in ev.samples]
    docs = [t for s in ev.samples for t in list(s["positive"]) + list(s["negative"])]
    texts = list(dict.fromkeys(queries + docs))
    emb = model.encode(texts, batch_size=ev.batch_size, convert_to_tensor=True).to(torch.float32)
    at = {t: i for i, t in enumerate(texts)}
    return emb[[at[t] for t in queries]], emb[[at[t] for t in docs]]


def assert_metrics(got, table, want, num_pos, k):
    assert list(got) == ["map", "mrr", "ndcg"] and all(type(v) is float for v in got.values())
    assert np.array_equal(table[:, RH.RR], want[:, RH.RR])
    assert (np.abs(table[:, RH.AP] - want[:, RH.AP]) <= [RH.ap_bound(int(p)) for p in num_pos]).all()
    assert (np.abs(table[:, RH.NDCG] - want[:, RH.NDCG]) <= RH.ndcg_bound(k)).all()
    for name, c in (("mrr", RH.RR), ("map", RH.AP), ("ndcg", RH.NDCG)):
        assert abs(got[name] - want[:, c].mean()) <= RH.mean_bound(num_pos, k, c), name


def test_evaluator_equals_the_yardstick_on_fp64_scores(model, tmp_path):
    samples = rerank_samples()
    assert len(samples) == 12 and {len(s["positive"]) for s in samples} == {1, 2, 3}
    assert all(2 <= len(s["negative"]) <= 9 for s in samples)
    ev = RerankingEvaluator(samples, mrr_at_k=3, name="dev", batch_size=16)
    offsets, num_pos = ev._groups()
    texts = {s["query"] for s in samples} | {t for s in samples for t in s["positive"] + s["negative"]}
    assert len(texts) < len(samples) + offsets[-1]          # texts repeat across the samples
    q, d = flat_embeddings(model, ev)
    D = q.shape[1]
    q64, d64 = q.cpu().numpy().astype(np.float64), d.cpu().numpy().astype(np.float64)
    gid = np.repeat(np.arange(len(samples)), np.diff(offsets))
    scores64 = (q64[gid] * d64).sum(1) / (np.linalg.norm(q64[gid], axis=1) * np.linalg.norm(d64, axis=1))
    # the precondition of comparing ranks: no two scores of a group within the fp32 kernel's error of each other
    gap = min(np.diff(np.sort(scores64[offsets[g]:offsets[g + 1]])).min() for g in range(len(samples)))
    print(f"  D {D}; smallest gap between two scores of a group {gap:.3e}; score bound {(D + 8) * 2.0 ** -24:.3e}")
    assert gap > 2 * (D + 8) * 2.0 ** -24
    want = RH.expected(scores64, offsets, num_pos, 3)
    calls, scored = [], []
    orig, raw = model.encode, util.rerank_scores
    model.encode = lambda *args, **kwargs: (calls.append(len(args[0])), orig(*args, **kwargs))[1]
    util.rerank_scores = lambda *a: (scored.append(a[3]), raw(*a))[1]
    try:
        got = ev.compute_metrices(model)
        table = ev.per_query_metrics(model)
        first = ev(model, output_path=str(tmp_path), epoch=0, steps=10)
        second = ev(model, output_path=str(tmp_path), epoch=1, steps=-1)
    finally:
        del model.encode
        util.rerank_scores = raw
    assert calls == [len(texts)] * 4                        # one encode per evaluation, over the distinct texts
    assert scored == [util.SCORE_COS] * 4
    print(f"  {got}")
    assert table.shape == (12, 3) and table.dtype == np.float64
    assert_metrics(got, table, want, num_pos, 3)
    assert first == second == got["map"]
    assert os.listdir(tmp_path) == ["RerankingEvaluator_dev_results.csv"]
    rows = read_csv(tmp_path / ev.csv_file)
    assert rows[0] == ["epoch", "steps", "MAP", "MRR@3"] and len(rows) == 3
    assert rows[1][:2] == ["0", "10"] and rows[2][:2] == ["1", "-1"]
    assert [float(v) for v in rows[1][2:]] == [got["map"], got["mrr"]] == [float(v) for v in rows[2][2:]]


def foreign_euclidean_score(a, b):
    """The third score function of the scripts this build serves, as a foreign torch callable: 1 / (1 + |a_i - b_j|)."""
    return 1.0 / (1.0 + torch.cdist(a, b, p=2))


def test_evaluator_scoring_paths(model, monkeypatch):
    samples = rerank_samples()
    offsets, num_pos = RerankingEvaluator(samples)._groups()
    q, d = flat_embeddings(model, RerankingEvaluator(samples))
    native, raw = [], util.rerank_scores
    monkeypatch.setattr(util, "rerank_scores", lambda *a: (native.append(a[3]), raw(*a))[1])
    # this package's dot_score by its tag, a foreign euclidean score by what it computes: both on the native path
    for fn, mode in ((util.dot_score, util.SCORE_DOT), (foreign_euclidean_score, util.SCORE_EUCLID)):
        ev = RerankingEvaluator(samples, mrr_at_k=5, similarity_fct=fn)
        assert evaluation.resolve_score_function("f", fn, q.device) == ("native", mode)
        got, table = ev.compute_metrices(model), ev.per_query_metrics(model)
        assert native == [mode, mode]
        native.clear()
        own = raw(q, d, offsets, mode).cpu().numpy()
        assert_metrics(got, table, RH.expected(own, offsets, num_pos, 5), num_pos, 5)
    # any other callable is called once per group on (query [D], documents [n, D]), as upstream calls it
    seen = []

    def custom(qe, de):
        seen.append((tuple(qe.shape), tuple(de.shape)))
        return -((qe - de) ** 2).sum(-1)

    ev = RerankingEvaluator(samples, mrr_at_k=5, similarity_fct=custom)
    got = ev.compute_metrices(model)
    D = q.shape[1]
    assert native == [] and seen[-12:] == [((D,), (int(n), D)) for n in np.diff(offsets)]
    table = ev.per_query_metrics(model)
    own = torch.cat([-((q[g] - d[offsets[g]:offsets[g + 1]]) ** 2).sum(-1) for g in range(12)]).cpu().numpy()
    assert_metrics(got, table, RH.expected(own, offsets, num_pos, 5), num_pos, 5)
    # a 2-D result gives its first row
    two_d = RerankingEvaluator(samples, mrr_at_k=5, similarity_fct=lambda qe, de: custom(qe, de).unsqueeze(0))
    assert two_d.compute_metrices(model) == got
    # a score without a rank is refused
    nan = RerankingEvaluator(samples, similarity_fct=lambda qe, de: torch.full((de.shape[0],), float("nan"), device=de.device))
    with pytest.raises(ValueError, match="NaN or infinite"):
        nan.compute_metrices(model)
    with pytest.raises(ValueError, match="NaN or infinite"):
        nan(model)


# ------------------------------------------------------------------ 6. fit() selects by it
def test_evaluator_selects_inside_fit(tmp_path):
    m = SentenceTransformer("tiny-bert", device="cuda")
    samples = rerank_samples()
    pairs = [InputExample(texts=[sent(100 + i, 6), sent(100 + i, 6) + " " + WORDS[i]]) for i in range(16)]
    evaluator = RerankingEvaluator(samples, mrr_at_k=5, name="dev")
    seen = []
    out = str(tmp_path / "out")
    m.fit([(DataLoader(pairs, batch_size=8, shuffle=False), S.MultipleNegativesRankingLoss(m))], evaluator=evaluator, epochs=2,
          warmup_steps=0, scheduler="constantlr", optimizer_params={"lr": 1e-4}, evaluation_steps=1, output_path=out,
          show_progress_bar=False, callback=lambda score, epoch, steps: seen.append((score, epoch, steps)))
    # two steps an epoch: an evaluation after each, and one at the end of the epoch
    want_steps = [(0, 1), (0, 2), (0, -1), (1, 1), (1, 2), (1, -1)]
    assert [s[1:] for s in seen] == want_steps
    assert all(type(s[0]) is float and 0.0 < s[0] <= 1.0 for s in seen)
    rows = read_csv(os.path.join(out, "eval", "RerankingEvaluator_dev_results.csv"))
    assert rows[0] == ["epoch", "steps", "MAP", "MRR@5"] and [tuple(int(v) for v in r[:2]) for r in rows[1:]] == want_steps
    assert [float(r[2]) for r in rows[1:]] == [s[0] for s in seen]
    assert m.best_score == max(s[0] for s in seen)
    # save_best_model wrote the encoder at the best evaluation
    assert os.path.isfile(os.path.join(out, "modules.json")) and os.path.isfile(os.path.join(out, "model.safetensors"))
    assert torch.isfinite(m._enc.params).all()
