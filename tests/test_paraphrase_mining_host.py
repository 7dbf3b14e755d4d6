"""Host (no GPU): the numpy half of paraphrase mining (util.merge_mined_pairs), the metric arithmetic of
ParaphraseMiningEvaluator (evaluation.paraphrase_metrics) on values worked by hand, the transitive closure, the
constructor's checks, the fp64 yardstick of the streaming top-k itself, and the drop-in exports."""
import os
import sys

import numpy as np
import pytest

import quadruplet_sentence_transformer_amd  # noqa: F401
import topk_stream_cases as T
from quadruplet_sentence_transformer_amd import util
from quadruplet_sentence_transformer_amd.evaluation import (ParaphraseMiningEvaluator, duplicate_closure,
                                                            paraphrase_metrics)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ merge_mined_pairs
def test_both_directions_of_a_pair_merge_and_keep_the_larger_score():
    # row 0 found 1 (0.9) and 2 (0.5); row 1 found 0 (0.95: the other direction, a little larger) and 2 (0.7); row 2 found 1
    scores = [[0.9, 0.5], [0.95, 0.7], [0.7, -np.inf]]
    cols = [[1, 2], [0, 2], [1, -1]]
    rows = [[0, 0], [1, 1], [2, 2]]
    assert util.merge_mined_pairs(scores, rows, cols, 100) == [[0.95, 0, 1], [0.7, 1, 2], [0.5, 0, 2]]


def test_max_pairs_cuts_the_candidates_before_the_merge():
    scores = [[0.9, 0.5], [0.95, 0.7], [0.7, -np.inf]]
    cols = [[1, 2], [0, 2], [1, -1]]
    rows = [[0, 0], [1, 1], [2, 2]]
    # the best three CANDIDATES are 0.95 (1->0), 0.9 (0->1), 0.7 (1->2): two pairs, not three
    assert util.merge_mined_pairs(scores, rows, cols, 3) == [[0.95, 0, 1], [0.7, 1, 2]]
    assert util.merge_mined_pairs(scores, rows, cols, 2) == [[0.95, 0, 1]]
    assert util.merge_mined_pairs(scores, rows, cols, 1) == [[0.95, 0, 1]]
    with pytest.raises(ValueError):
        util.merge_mined_pairs(scores, rows, cols, 0)


def test_tied_scores_are_ordered_by_the_smaller_then_the_larger_index():
    s = np.ones(6)
    i = np.array([5, 2, 2, 0, 3, 4])
    j = np.array([1, 9, 4, 7, 0, 2])
    assert util.merge_mined_pairs(s, i, j, 100) == [[1.0, 0, 3], [1.0, 0, 7], [1.0, 1, 5], [1.0, 2, 4], [1.0, 2, 9]]
    # the cut falls inside the tie: the same order decides
    assert util.merge_mined_pairs(s, i, j, 2) == [[1.0, 0, 3], [1.0, 0, 7]]


def test_empty_slots_self_pairs_and_an_empty_input_are_dropped():
    assert util.merge_mined_pairs([0.5, 0.4, -np.inf], [0, 1, 2], [0, 3, -1], 10) == [[0.4, 1, 3]]
    assert util.merge_mined_pairs([], [], [], 10) == []
    with pytest.raises(ValueError):
        util.merge_mined_pairs([1.0], [0, 1], [1], 10)
    out = util.merge_mined_pairs(np.float32([0.25]), [3], [1], 10)
    assert out == [[0.25, 1, 3]] and type(out[0][0]) is float and type(out[0][1]) is int


def test_mined_pairs_from_the_reference_top_k():
    """The whole host path on the yardstick's own top-k: 6 ternary rows, exact integer dot products."""
    e = T.ternary(6, 32, seed=2)
    full = T.scores_ref(e, e, "dot")
    ws, wi = T.topk_ref(full, 2, exclude_self=True)
    pairs = util.merge_mined_pairs(ws, np.arange(6)[:, None].repeat(2, 1), wi, 100)
    assert all(s == full[i, j] and i < j for s, i, j in pairs)
    assert [(-s, i, j) for s, i, j in pairs] == sorted((-s, i, j) for s, i, j in pairs)
    for r in range(6):                                        # every row's best other row is in the list
        best = int(wi[r, 0])
        assert (min(r, best), max(r, best)) in {(i, j) for _, i, j in pairs}


# ------------------------------------------------------------------ the yardstick itself
def test_topk_ref_order_exclusion_cap_and_padding():
    s = np.array([[1.0, 3.0, 3.0, np.nan, np.inf, -np.inf, 3.0]], dtype=np.float32)
    v, i = T.topk_ref(s, 9, col_base=10)
    np.testing.assert_array_equal(i[0], [13, 14, 11, 12, 16, 10, 15, -1, -1])
    assert np.isnan(v[0, 0]) and v[0, 1] == np.inf and v[0, 6] == -np.inf and (v[0, 7:] == -np.inf).all()
    v, i = T.topk_ref(s, 3, col_base=10, row_base=11, exclude_self=True, max_score=3.0)
    np.testing.assert_array_equal(i[0], [13, 12, 16])         # NaN is not above the cap; +inf is; id 11 is the row's own
    assert T.slices(1, 7) == [(0, 1)] and T.slices(7, 7) == [(t, t + 1) for t in range(7)]
    for n, parts in ((255, 2), (1000, 7), (5000, 7)):
        cuts = T.slices(n, parts)
        assert cuts[0][0] == 0 and cuts[-1][1] == n and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
        assert len({b - a for a, b in cuts}) > 1              # unequal widths


# ------------------------------------------------------------------ paraphrase_metrics
IDS = ["a", "b", "c", "d", "e", "f", "g", "h"]


def fs(*pairs):
    return {frozenset(p) for p in pairs}


def test_metrics_worked_by_hand():
    """Six mined pairs, four gold pairs, the 1st, 2nd and 5th mined pair are gold (one gold pair is never found):

        n   correct  precision  recall  f1 = 2 * correct / (n + 4)
        1      1       1          1/4     2/5
        2      2       1          2/4     4/6      <- best (first of two equal)
        3      2       2/3        2/4     4/7
        4      2       2/4        2/4     4/8
        5      3       3/5        3/4     6/9  = 4/6
        6      3       3/6        3/4     6/10
    average precision = (1 + 1 + 3/5) / 4 = 0.65; threshold = (0.8 + 0.7) / 2."""
    pairs = [[0.9, 0, 1], [0.8, 2, 3], [0.7, 0, 2], [0.6, 1, 3], [0.5, 4, 5], [0.4, 0, 5]]
    gold = fs(("a", "b"), ("d", "c"), ("e", "f"), ("g", "h"))
    m = paraphrase_metrics(pairs, IDS, gold)
    assert m["average_precision"] == pytest.approx(0.65, abs=1e-15)
    assert m["f1"] == pytest.approx(2 / 3, abs=1e-15)
    assert m["precision"] == 1.0 and m["recall"] == 0.5
    assert m["threshold"] == pytest.approx(0.75, abs=1e-15)
    assert set(m) == {"precision", "recall", "f1", "threshold", "average_precision"}


def test_metrics_threshold_of_the_last_pair_is_its_own_score():
    pairs = [[0.9, 0, 2], [0.8, 0, 1], [0.3, 2, 3]]
    m = paraphrase_metrics(pairs, IDS, fs(("a", "b"), ("c", "d")))
    # correct: 0, 1, 2 -> f1 0, 2/4, 4/5: the best cut is the whole list
    assert m["f1"] == pytest.approx(0.8, abs=1e-15) and m["precision"] == pytest.approx(2 / 3, abs=1e-15) and m["recall"] == 1.0
    assert m["threshold"] == 0.3
    assert m["average_precision"] == pytest.approx((1 / 2 + 2 / 3) / 2, abs=1e-15)


def test_metrics_of_an_empty_list_or_without_gold_pairs_are_zero():
    zero = {"precision": 0.0, "recall": 0.0, "f1": 0.0, "threshold": 0.0, "average_precision": 0.0}
    assert paraphrase_metrics([], IDS, fs(("a", "b"))) == zero
    assert paraphrase_metrics([[0.9, 0, 1]], IDS, set()) == zero
    assert paraphrase_metrics([[0.9, 0, 2]], IDS, fs(("a", "b"))) == zero          # nothing found


# ------------------------------------------------------------------ the evaluator's constructor
SMAP = {k: f"sentence {k}" for k in IDS}


def test_transitive_closure_on_two_components():
    gold = duplicate_closure([("a", "b"), ("b", "c"), ("c", "d"), ("e", "f")])
    assert gold == fs(("a", "b"), ("a", "c"), ("a", "d"), ("b", "c"), ("b", "d"), ("c", "d"), ("e", "f"))
    ev = ParaphraseMiningEvaluator(SMAP, duplicates_list=[("a", "b"), ("b", "c"), ("c", "d"), ("e", "f")],
                                   add_transitive_closure=True)
    assert ev.duplicates == gold and ev.total_num_duplicates == 7
    plain = ParaphraseMiningEvaluator(SMAP, duplicates_list=[("a", "b"), ("b", "c"), ("c", "d"), ("e", "f")])
    assert plain.total_num_duplicates == 4


def test_constructor_reads_both_duplicate_forms_and_drops_what_it_cannot_use():
    ev = ParaphraseMiningEvaluator(SMAP, duplicates_list=[("a", "b"), ("b", "a"), ("a", "a"), ("a", "zz")],
                                   duplicates_dict={"c": {"d": True, "e": False}, "d": {"c": True}}, name="dev")
    assert ev.duplicates == fs(("a", "b"), ("c", "d")) and ev.total_num_duplicates == 2
    assert ev.ids == IDS and ev.sentences == [SMAP[k] for k in IDS]
    assert ev.csv_file == "paraphrase_mining_evaluation_dev_results.csv"
    assert ev.csv_headers == ["epoch", "steps", "precision", "recall", "f1", "threshold", "average_precision"]
    assert ParaphraseMiningEvaluator(SMAP, duplicates_list=[]).csv_file == "paraphrase_mining_evaluation_results.csv"
    assert (ev.query_chunk_size, ev.corpus_chunk_size, ev.max_pairs, ev.top_k, ev.batch_size) == (5000, 100000, 500000, 100, 16)


@pytest.mark.parametrize("kw", [dict(), dict(duplicates_list=[("a", "b")], top_k=0), dict(duplicates_list=[("a", "b")], top_k=1025),
                                dict(duplicates_list=[("a", "b")], max_pairs=0), dict(duplicates_list=[("a", "b")], corpus_chunk_size=0),
                                dict(duplicates_list=[("a", "b")], query_chunk_size=0), dict(duplicates_list=[("a", "b")], batch_size=0)])
def test_constructor_validation(kw):
    with pytest.raises(ValueError):
        ParaphraseMiningEvaluator(SMAP, **kw)


def test_constructor_refuses_an_empty_sentence_map():
    with pytest.raises(ValueError):
        ParaphraseMiningEvaluator({}, duplicates_list=[("a", "b")])


# ------------------------------------------------------------------ exports
def test_dropin_namespaces_export_the_new_names():
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        for m in [k for k in sys.modules if k.startswith("sentence_transformers")]:
            del sys.modules[m]
        import sentence_transformers.evaluation as E
        import sentence_transformers.util as U
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
    assert U.semantic_search is util.semantic_search and U.paraphrase_mining is util.paraphrase_mining
    assert U.paraphrase_mining_embeddings is util.paraphrase_mining_embeddings and U.topk_stream is util.topk_stream
    assert E.ParaphraseMiningEvaluator is ParaphraseMiningEvaluator
    import inspect
    sig = inspect.signature(util.semantic_search)
    assert list(sig.parameters) == ["query_embeddings", "corpus_embeddings", "query_chunk_size", "corpus_chunk_size", "top_k",
                                    "score_function"]
    assert [sig.parameters[p].default for p in list(sig.parameters)[2:]] == [100, 500000, 10, util.cos_sim]
    sig = inspect.signature(util.paraphrase_mining_embeddings)
    assert [sig.parameters[p].default for p in list(sig.parameters)[1:]] == [5000, 100000, 500000, 100, util.cos_sim]
    sig = inspect.signature(util.paraphrase_mining)
    assert list(sig.parameters)[:4] == ["model", "sentences", "show_progress_bar", "batch_size"]
    assert sig.parameters["show_progress_bar"].default is False and sig.parameters["batch_size"].default == 32
