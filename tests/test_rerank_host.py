"""CPU: RerankingEvaluator's host side -- the yardstick of the GPU test (rerank_helpers) against sklearn and against
upstream's walk, the counting form the kernel uses against that yardstick, the library's new symbols and their refusals
(which precede any launch), the wrappers' checks of host offsets / num_pos, the constructor surface and the drop-in
export. No kernel runs."""
import inspect
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import quadruplet_sentence_transformer_amd  # noqa: F401
import rerank_helpers as RH
from quadruplet_sentence_transformer_amd import _lib, evaluation, util
from quadruplet_sentence_transformer_amd.evaluation import RerankingEvaluator, SentenceEvaluator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = -1, -2
EMPTY = inspect.Parameter.empty
HOST_SETS = ("1+1", "1+62", "1+63", "2+63", "63+1", "1+256", "3+1022", "700+700", "ragged")


def all_groups():
    """(kind, P, scores of one group) over every kind and the smaller size sets."""
    for kind in RH.KINDS:
        for name in HOST_SETS:
            scores, offsets, num_pos = RH.case(kind, RH.SIZE_SETS[name], RH.case_seed(kind, name))
            for g, P in enumerate(num_pos):
                yield kind, int(P), scores[offsets[g]:offsets[g + 1]]


# ------------------------------------------------------------------ the yardstick
def test_yardstick_ap_equals_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    worst = 0.0
    for kind, P, s in all_groups():
        got = RH.group_expected(s, P, 10)[RH.AP]
        ref = metrics.average_precision_score([True] * P + [False] * (len(s) - P), s.astype(np.float64))
        worst = max(worst, abs(got - ref) / RH.ap_bound(P))
        assert abs(got - ref) <= RH.ap_bound(P), (kind, P, len(s))
    print(f"  largest |ap - sklearn| / bound = {worst:.3f}")


def test_yardstick_rr_equals_upstreams_walk():
    for kind, P, s in all_groups():
        for k in RH.KS:
            assert RH.group_expected(s, P, k)[RH.RR] == RH.upstream_rr(s, P, k), (kind, P, len(s), k)


def test_yardstick_is_the_counting_form():
    """What the kernel counts per positive p -- rank(p), ge_all(p), ge_pos(p) -- gives the yardstick's three numbers."""
    for kind, P, s in all_groups():
        if len(s) > 300:
            continue
        s64, n = s.astype(np.float64), len(s)
        ranks = [1 + sum(1 for d in range(n) if s64[d] > s64[p] or (s64[d] == s64[p] and d < p)) for p in range(P)]
        ap = sum(Fraction(int((s64[:P] >= s64[p]).sum()), int((s64 >= s64[p]).sum())) for p in range(P)) / P
        for k in (1, 10):
            want = RH.group_expected(s, P, k)
            assert want[RH.RR] == (1.0 / min(ranks) if min(ranks) <= k else 0.0), (kind, P, n, k)
            assert abs(want[RH.AP] - float(ap)) <= RH.ap_bound(P)
            dcg = sum(1.0 / np.log2(1.0 + r) for r in ranks if r <= k)
            ideal = sum(1.0 / np.log2(1.0 + i) for i in range(1, min(P, k) + 1))
            assert abs(want[RH.NDCG] - dcg / ideal) <= RH.ndcg_bound(k)


def test_cases_are_what_they_say():
    for name, groups in RH.SIZE_SETS.items():
        assert all(P >= 1 and N >= 1 for P, N in groups)
    assert len(RH.SIZE_SETS["ragged"]) == 300 and {P + N for P, N in RH.SIZE_SETS["ragged"]} <= set(range(2, 71))
    s, off, pos = RH.case("gauss", RH.SIZE_SETS["1+4999"], 1)
    assert len(np.unique(s)) == 5000
    s, off, pos = RH.case("zeros", RH.SIZE_SETS["700+700"], 2)
    assert (s == 0).all() and np.signbit(s).any() and not np.signbit(s).all()
    # every score equal: the first document, a positive, ranks first only by the tie rule; ap = P / n whatever the rule
    for P, N in ((1, 62), (3, 1022), (700, 700)):
        s, off, pos = RH.case("flat", [(P, N)], 3)
        assert RH.expected(s, off, pos, 10).tolist() == [[1.0, P / (P + N), 1.0]]
    # every positive below every negative: nothing within k once there are k negatives
    s, off, pos = RH.case("pos_last", [(2, 63)], 4)
    assert RH.expected(s, off, pos, 10)[0, RH.RR] == 0.0 and RH.expected(s, off, pos, 100)[0, RH.RR] == 1.0 / 64
    s, off, pos = RH.case("pos_first", [(2, 63)], 4)
    assert RH.expected(s, off, pos, 10).tolist() == [[1.0, 1.0, 1.0]]


# ------------------------------------------------------------------ the library
def test_library_binds_the_entry_points_and_checks_arguments_first():
    lib = _lib.load()
    assert lib.qst_version() >= 113
    for name, arity in (("qst_rerank_scores", 9), ("qst_rerank_workspace_bytes", 2), ("qst_rerank_metrics", 11)):
        assert hasattr(lib, name) and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert len(_lib.SIGNATURES[name][1]) == arity
    ws = lib.qst_rerank_workspace_bytes
    # a 16-byte record per document and an info word per query, the words rounded up to 16 bytes
    assert ws(1, 2) == 32 + 16 and ws(5, 100) == 1600 + 32 and ws(10000, 10000000) == 160000000 + 40000
    assert ws(0, 5) == 0 and ws(1, 1) == 0 and ws(-1, 5) == 0 and ws(1 << 31, 5) == 0 and ws(5, 1 << 31) == 0
    assert ws((1 << 31) - 1, (1 << 31) - 1) == 16 * ((1 << 31) - 1) + 4 * (1 << 31)
    # refusals come before anything touches a device: fake non-NULL pointers
    P = 64
    scores = dict(queries=P, docs=P, offsets=P, nq=3, nd=10, dim=8, mode=1, scores=P)
    run = lambda **k: lib.qst_rerank_scores(*[k.get(n, v) for n, v in scores.items()], None)  # noqa: E731
    for bad in (dict(queries=None), dict(docs=None), dict(offsets=None), dict(scores=None), dict(nq=0), dict(nq=-1), dict(nd=1),
                dict(nd=0), dict(dim=0), dict(dim=-4), dict(mode=3), dict(mode=-1)):
        assert run(**bad) == BAD_ARG, bad
    for bad in (dict(nd=1 << 31), dict(nq=1 << 31), dict(nd=1 << 40)):
        assert run(**bad) == UNSUPPORTED, bad
    big = 1 << 62
    metrics = dict(scores=P, offsets=P, num_pos=P, nq=3, nd=10, k=10, per_query=P, out=P, ws=P, nbytes=ws(3, 10))
    run = lambda **k: lib.qst_rerank_metrics(*[k.get(n, v) for n, v in metrics.items()], None)  # noqa: E731
    for bad in (dict(scores=None), dict(offsets=None), dict(num_pos=None), dict(per_query=None), dict(out=None), dict(ws=None),
                dict(nq=0), dict(nd=1), dict(k=0), dict(k=-3), dict(ws=P + 8), dict(nbytes=ws(3, 10) - 1), dict(nbytes=0)):
        assert run(**bad) == BAD_ARG, bad
    for bad in (dict(nd=1 << 31, nbytes=big), dict(nq=1 << 31, nbytes=big)):
        assert run(**bad) == UNSUPPORTED, bad


# ------------------------------------------------------------------ the wrappers
def test_wrappers_name_the_first_bad_group():
    s = torch.zeros(10)
    good_off, good_pos = [0, 3, 5, 10], [1, 1, 2]
    for off, pos, text in (([1, 3, 5, 10], good_pos, r"group 0 starts at offsets\[0\] = 1"),
                           ([0, 5, 3, 10], good_pos, r"group 1: offsets descend, 5 -> 3"),
                           ([0, 3, 5, 9], good_pos, r"group 2 ends at offsets\[nq\] = 9, but there are 10 documents"),
                           ([0, 3, 5, 11], good_pos, r"group 2 ends at offsets\[nq\] = 11"),
                           (good_off, [1, 0, 2], r"group 1: 0 positives of 2 documents"),
                           (good_off, [1, 2, 2], r"group 1: 2 positives of 2 documents"),
                           (good_off, [3, 1, 2], r"group 0: 3 positives of 3 documents"),
                           (good_off, [1, 1, -1], r"group 2: -1 positives"),
                           ([0, 3, 3, 10], good_pos, r"group 1: 1 positives of 0 documents"),
                           (good_off, [1, 1], r"num_pos must be 3 integers"),
                           (good_off, [1.0, 1.0, 2.0], r"num_pos must be 3 integers"),
                           ([0], [], r"offsets must be nq \+ 1 integers"),
                           ([0.0, 10.0], [1], r"offsets must be nq \+ 1 integers")):
        for o, p in ((off, pos), (np.asarray(off), np.asarray(pos)), (torch.as_tensor(off), torch.as_tensor(pos))):
            with pytest.raises(ValueError, match=text):
                util.rerank_metrics(s, o, p)
    for off, text in (([1, 3, 10], r"group 0 starts"), ([0, 7, 3, 10], r"group 1: offsets descend"), ([0, 3, 9], r"group 1 ends")):
        with pytest.raises(ValueError, match=text):
            util.rerank_scores(torch.zeros(len(off) - 1, 4), torch.zeros(10, 4), off)
    with pytest.raises(ValueError, match="3 queries but offsets describe 2 groups"):
        util.rerank_scores(torch.zeros(3, 4), torch.zeros(10, 4), [0, 3, 10])
    with pytest.raises(ValueError):
        util.rerank_scores(torch.zeros(2, 4), torch.zeros(10, 5), [0, 3, 10])
    with pytest.raises(ValueError):
        util.rerank_metrics(s, good_off, good_pos, k=0)
    # well-formed groups on host tensors: there is no CPU path
    with pytest.raises(_lib.QstError, match="HIP device"):
        util.rerank_metrics(s, good_off, good_pos)
    with pytest.raises(_lib.QstError, match="HIP device"):
        util.rerank_scores(torch.zeros(3, 4), torch.zeros(10, 4), good_off)


# ------------------------------------------------------------------ the surface
SAMPLES = [{"query": "q0", "positive": ["a", "b"], "negative": ["c"]},
           {"query": "q1", "positive": [], "negative": ["c", "d"]},
           {"query": "q2", "positive": ["a"], "negative": []},
           {"query": "q3", "positive": ["d"], "negative": ["a", "q0", "e"]}]


def test_constructor_surface():
    sig = {k: p.default for k, p in inspect.signature(RerankingEvaluator.__init__).parameters.items() if k != "self"}
    assert sig == {"samples": EMPTY, "mrr_at_k": 10, "name": "", "write_csv": True, "similarity_fct": evaluation.cos_sim,
                   "batch_size": 64, "show_progress_bar": False, "use_batched_encoding": True}
    assert list(sig) == ["samples", "mrr_at_k", "name", "write_csv", "similarity_fct", "batch_size", "show_progress_bar",
                         "use_batched_encoding"]
    assert evaluation.cos_sim._qst_mode == util.cos_sim._qst_mode == util.SCORE_COS
    assert evaluation.resolve_score_function("cos_sim", evaluation.cos_sim) == ("native", util.SCORE_COS)
    assert issubclass(RerankingEvaluator, SentenceEvaluator)
    ev = RerankingEvaluator(SAMPLES, mrr_at_k=5, name="dev", batch_size=8, use_batched_encoding=False)
    assert (ev.mrr_at_k, ev.name, ev.batch_size, ev.write_csv, ev.show_progress_bar) == (5, "dev", 8, True, False)
    assert ev.similarity_fct is evaluation.cos_sim
    # samples without a positive or without a negative are dropped
    assert ev.samples == [SAMPLES[0], SAMPLES[3]]
    assert ev.csv_file == "RerankingEvaluator_dev_results.csv" and ev.csv_headers == ["epoch", "steps", "MAP", "MRR@5"]
    plain = RerankingEvaluator(SAMPLES)
    assert plain.csv_file == "RerankingEvaluator_results.csv" and plain.csv_headers == ["epoch", "steps", "MAP", "MRR@10"]
    # a dict gives its values
    assert RerankingEvaluator({"x": SAMPLES[3], "y": SAMPLES[1], "z": SAMPLES[0]}).samples == [SAMPLES[3], SAMPLES[0]]
    offsets, num_pos = ev._groups()
    assert offsets.tolist() == [0, 3, 7] and offsets.dtype == np.int64 and num_pos.tolist() == [2, 1] and num_pos.dtype == np.int32
    assert "use_batched_encoding" in RerankingEvaluator.__doc__
    for fn in ("compute_metrices", "per_query_metrics"):
        assert list(inspect.signature(getattr(RerankingEvaluator, fn)).parameters) == ["self", "model"]


def test_no_usable_sample_is_refused_before_anything_is_encoded():
    ev = RerankingEvaluator(SAMPLES[1:3])
    assert ev.samples == []
    with pytest.raises(ValueError, match="no sample has both"):
        ev(None)
    with pytest.raises(ValueError, match="no sample has both"):
        ev.compute_metrices(None)


class FixedMetrics(RerankingEvaluator):
    def compute_metrices(self, model):
        return {"map": 0.625, "mrr": 0.75, "ndcg": 0.875}


def test_call_returns_map_and_appends_rows(tmp_path):
    import csv
    ev = FixedMetrics(SAMPLES, mrr_at_k=3, name="dev")
    assert ev(None, output_path=str(tmp_path), epoch=0, steps=5) == 0.625
    assert ev(None, output_path=str(tmp_path), epoch=1, steps=-1) == 0.625
    assert os.listdir(tmp_path) == ["RerankingEvaluator_dev_results.csv"]
    with open(tmp_path / ev.csv_file) as f:
        table = list(csv.reader(f))
    assert table == [["epoch", "steps", "MAP", "MRR@3"], ["0", "5", "0.625", "0.75"], ["1", "-1", "0.625", "0.75"]]
    # nothing is written without an output path, or with write_csv=False
    ev(None)
    FixedMetrics(SAMPLES, write_csv=False)(None, output_path=str(tmp_path))
    assert len(os.listdir(tmp_path)) == 1


def test_dropin_import_resolves():
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]
        from sentence_transformers.evaluation import RerankingEvaluator as E
        assert E is RerankingEvaluator
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]
    assert "RerankingEvaluator" in evaluation.__doc__
