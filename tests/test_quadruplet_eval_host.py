"""CPU: the host side of QuadrupletEvaluator, QuadrupletLossEvaluator and get_sequential_evaluator -- constructor surface,
sampling and re-sampling, the gamma formula, the CSV files -- with the device step (quadruplet_counts) replaced by fixed
counts, and the yardstick of the GPU test (quadruplet_eval_helpers.ref) against three TripletEvaluators. No kernel runs."""
import csv
import inspect
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

import quadruplet_sentence_transformer_amd  # noqa: F401
import quadruplet_eval_helpers as Q
import tuple_loss_helpers as H
from quadruplet_sentence_transformer_amd import _lib, evaluation, st_losses as S
from quadruplet_sentence_transformer_amd.evaluation import (QuadrupletEvaluator, QuadrupletLossEvaluator, SimilarityFunction,
                                                            TripletEvaluator, get_sequential_evaluator)
from quadruplet_sentence_transformer_amd.losses import GammaQuadrupletLoss
from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = inspect.Parameter.empty


def defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if k != "self"}


class FixedCounts(QuadrupletEvaluator):
    """The evaluator with its device step replaced: counts[3 * metric + comparison] of N rows."""

    def __init__(self, counts, N, **kw):
        super().__init__(["a"] * N, ["p"] * N, ["q"] * N, ["n"] * N, **kw)
        self.fixed = (np.asarray(counts), N)

    def quadruplet_counts(self, model):
        return self.fixed


#            cosine: pos_part, pos_neg, part_neg | manhattan | euclidean      (of 20 rows)
COUNTS = [10, 16, 4, 12, 14, 6, 8, 18, 5]


def read_csv(path):
    with open(path) as f:
        return list(csv.reader(f))


# ------------------------------------------------------------------ constructors
def test_constructor_surface_follows_the_reference():
    assert defaults(QuadrupletEvaluator.__init__) == {
        "anchors": EMPTY, "positives": EMPTY, "partially_positives": EMPTY, "negatives": EMPTY, "gamma": 0.6,
        "main_distance_function": None, "name": "", "batch_size": 16, "show_progress_bar": False, "write_csv": True,
        "all_examples": None}
    assert defaults(QuadrupletLossEvaluator.__init__) == {
        "quadruplet_dataset": EMPTY, "quadruplet_loss": EMPTY, "batch_size": 32, "additional_model_kwargs": None,
        "additional_loss_kwargs": None, "use_amp": False}
    d = defaults(get_sequential_evaluator)
    assert list(d) == ["dataset", "loss", "evaluation_queries_path", "no_transform_dataset", "corpus_chunk_size", "mrr_at_k",
                       "ndcg_at_k", "accuracy_at_k", "precision_recall_at_k", "map_at_k", "show_progress_bar", "batch_size",
                       "write_csv", "score_functions", "main_score_function", "main_distance_function", "name",
                       "additional_model_kwargs", "additional_loss_kwargs", "use_amp"]
    assert (d["corpus_chunk_size"], d["mrr_at_k"], d["ndcg_at_k"], d["accuracy_at_k"], d["precision_recall_at_k"],
            d["map_at_k"], d["batch_size"], d["write_csv"], d["use_amp"]) == \
           (50000, [10], [10], [1, 3, 5, 10], [1, 3, 5, 10], [100], 32, True, False)
    assert QuadrupletEvaluator.N_EPOCHS_RESET_EXAMPLES == 5
    ev = QuadrupletEvaluator(["a"], ["p"], ["q"], ["n"], gamma=0.25, name="dev", batch_size=4)
    assert (ev.anchors, ev.positives, ev.partially_positives, ev.negatives) == (["a"], ["p"], ["q"], ["n"])
    assert ev._gamma == 0.25 and ev.name == "dev" and ev.batch_size == 4 and ev.main_distance_function is None
    assert ev.write_csv is True and ev.show_progress_bar is False and ev._all_examples is None and ev._epoch_counter == 0
    assert ev.csv_file == "quadruplet_evaluation_dev_results.csv"
    assert QuadrupletEvaluator(["a"], ["p"], ["q"], ["n"]).csv_file == "quadruplet_evaluation_results.csv"
    assert ev.csv_headers == ["epoch", "steps", "pos_part_accuracy", "pos_neg_accuracy", "part_neg_accuracy",
                              "global_accuracy"]
    le = QuadrupletLossEvaluator([1], "loss", batch_size=8, use_amp=True)
    assert (le._quadruplet_dataset, le._quadruplet_loss, le._batch_size, le._use_amp) == ([1], "loss", 8, True)


@pytest.mark.parametrize("short", [1, 2, 3])
def test_constructor_asserts_equal_lengths(short):
    cols = [["x", "y"]] * 4
    cols[short] = ["x"]
    with pytest.raises(AssertionError):
        QuadrupletEvaluator(*cols)


# ------------------------------------------------------------------ sampling
def rows_of_three_kinds():
    return [InputExample(texts=["a0", "p0", "q0", "n0"]),
            (InputExample(texts=["a1", "p1", "q1", "n1"]), 0),
            {"reference": "a2", "positive": "p2", "part_positive": "q2", "negative": "n2"},
            ({"reference": "a3", "positive": ["p3"], "part_positive": ["q3"], "negative": ["n3"]}, 1),
            {"reference": "a4", "positive": ["p4x", "p4y", "p4z"], "part_positive": "q4", "negative": ["n4x", "n4y"]}]


def test_from_input_examples_takes_examples_tuples_and_dicts():
    rows = rows_of_three_kinds()
    ev = QuadrupletEvaluator.from_input_examples(rows, gamma=0.5, name="x", batch_size=8)
    assert ev.anchors == ["a0", "a1", "a2", "a3", "a4"]
    assert ev.positives[:4] == ["p0", "p1", "p2", "p3"] and ev.positives[4] in ("p4x", "p4y", "p4z")
    assert ev.partially_positives == ["q0", "q1", "q2", "q3", "q4"]
    assert ev.negatives[:4] == ["n0", "n1", "n2", "n3"] and ev.negatives[4] in ("n4x", "n4y")
    assert ev._all_examples is rows and ev._gamma == 0.5 and ev.name == "x" and ev.batch_size == 8
    # one entry is drawn where a value is a list: over many draws every entry turns up
    random.seed(0)
    seen = {QuadrupletEvaluator.from_input_examples(rows).positives[4] for _ in range(60)}
    assert seen == {"p4x", "p4y", "p4z"}
    with pytest.raises(ValueError):
        QuadrupletEvaluator.from_input_examples([InputExample(texts=["a", "p", "n"])])


def test_examples_are_drawn_again_on_every_fifth_call_only():
    rows = [{"reference": f"a{i}", "positive": [f"p{i}_{k}" for k in range(50)], "part_positive": [f"q{i}_{k}" for k in range(50)],
             "negative": [f"n{i}_{k}" for k in range(50)]} for i in range(4)]
    random.seed(11)
    ev = QuadrupletEvaluator.from_input_examples(rows)
    ev.quadruplet_counts = lambda model: (np.zeros(9, dtype=np.int64), 4)
    first = (list(ev.positives), list(ev.partially_positives), list(ev.negatives))
    for call in range(1, 11):
        if call % 5 == 0:
            # what a draw at this state of `random` gives, taken without disturbing the state
            state = random.getstate()
            expect = evaluation.sample_quadruplets(rows)
            random.setstate(state)
        before = (list(ev.positives), list(ev.partially_positives), list(ev.negatives))
        ev(None)
        now = (list(ev.positives), list(ev.partially_positives), list(ev.negatives))
        assert ev._epoch_counter == call
        if call % 5 == 0:
            assert now == tuple(expect[1:]) and now != before       # 12 draws of 50: the same lists again is ~1e-20
            assert ev.anchors == ["a0", "a1", "a2", "a3"]
        else:
            assert now == before
        if call < 5:
            assert now == first
    # without all_examples nothing is ever drawn
    fixed = FixedCounts(COUNTS, 20)
    for _ in range(6):
        fixed(None)
    assert fixed.positives == ["p"] * 20 and fixed._epoch_counter == 6


# ------------------------------------------------------------------ the score
@pytest.mark.parametrize("gamma", [0.6, 0.0, 1.0, 0.25])
@pytest.mark.parametrize("fn,pick", [(None, None), (SimilarityFunction.COSINE, 0), (SimilarityFunction.MANHATTAN, 1),
                                     (SimilarityFunction.EUCLIDEAN, 2)], ids=["max", "cosine", "manhattan", "euclidean"])
def test_score_is_the_gamma_formula_over_the_chosen_accuracies(gamma, fn, pick):
    acc = np.asarray(COUNTS, dtype=np.float64).reshape(3, 3) / 20           # [metric, comparison]
    chosen = [acc[:, j].max() if pick is None else acc[pick, j] for j in range(3)]
    pos_part, pos_neg, part_neg = chosen
    got = FixedCounts(COUNTS, 20, gamma=gamma, main_distance_function=fn)(None)
    assert isinstance(got, float)
    assert got == pytest.approx(((1 - gamma) * pos_part + gamma * part_neg + pos_neg) / 2, abs=1e-15)
    if pick is None:
        assert chosen == [12 / 20, 18 / 20, 6 / 20]
    # DOT_PRODUCT names none of the three: the largest, as TripletEvaluator does
    assert FixedCounts(COUNTS, 20, gamma=gamma, main_distance_function=SimilarityFunction.DOT_PRODUCT)(None) == \
        FixedCounts(COUNTS, 20, gamma=gamma)(None)


def test_csv_files_headers_and_append(tmp_path):
    ev = FixedCounts(COUNTS, 20, name="dev")
    s0 = ev(None, output_path=str(tmp_path), epoch=0, steps=50)
    names = ["quadruplet_evaluation_dev_results.csv", "triplet_evaluation_part_neg_results.csv",
             "triplet_evaluation_pos_neg_results.csv", "triplet_evaluation_pos_part_results.csv"]
    assert sorted(os.listdir(tmp_path)) == names
    ev.fixed = (np.asarray(COUNTS[::-1]), 20)
    s1 = ev(None, output_path=str(tmp_path), epoch=1, steps=-1)
    quad = read_csv(tmp_path / names[0])
    assert quad[0] == ["epoch", "steps", "pos_part_accuracy", "pos_neg_accuracy", "part_neg_accuracy", "global_accuracy"]
    assert len(quad) == 3
    assert quad[1] == ["0", "50", str(12 / 20), str(18 / 20), str(6 / 20), str(s0)]
    assert quad[2][:2] == ["1", "-1"] and float(quad[2][5]) == s1
    for j, t in enumerate(("pos_part", "pos_neg", "part_neg")):
        table = read_csv(tmp_path / f"triplet_evaluation_{t}_results.csv")
        assert table[0] == TripletEvaluator(["a"], ["p"], ["n"]).csv_headers
        assert table[0] == ["epoch", "steps", "accuracy_cosinus", "accuracy_manhattan", "accuracy_euclidean"]
        assert len(table) == 3
        assert table[1] == ["0", "50"] + [str(COUNTS[3 * m + j] / 20) for m in range(3)]
        assert table[2] == ["1", "-1"] + [str(COUNTS[::-1][3 * m + j] / 20) for m in range(3)]
    # the file names are TripletEvaluator's for the names pos_part, pos_neg, part_neg
    assert TripletEvaluator(["a"], ["p"], ["n"], name="pos_part").csv_file == "triplet_evaluation_pos_part_results.csv"
    # nothing is written without an output path, or with write_csv=False
    ev(None)
    FixedCounts(COUNTS, 20, write_csv=False)(None, output_path=str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == names and len(read_csv(tmp_path / names[0])) == 3


# ------------------------------------------------------------------ the GPU test's yardstick
class StubModel:
    """encode() returns fixed arrays by sentence list."""

    def __init__(self, table):
        self.table = table
        self.calls = 0

    def encode(self, sentences, **kwargs):
        self.calls += 1
        return self.table[sentences[0]]


@pytest.mark.parametrize("B,D", [(64, 384), (7, 33), (200, 64)])
def test_yardstick_equals_three_triplet_evaluators(B, D):
    a, p, q, n = [t.numpy() for t in Q.case(B, D, B * 1000 + D)]
    dist, holds = Q.ref(a, p, q, n)
    assert dist.shape == (B, 9) and holds.shape == (B, 9) and dist.dtype == np.float64
    model = StubModel({"a": a, "p": p, "q": q, "n": n})
    lists = {k: [k] * B for k in "apqn"}
    acc = Q.accuracies(holds)
    for j, (pos, neg) in enumerate((("p", "q"), ("p", "n"), ("q", "n"))):
        for m, fn in enumerate((SimilarityFunction.COSINE, SimilarityFunction.MANHATTAN, SimilarityFunction.EUCLIDEAN)):
            got = TripletEvaluator(lists["a"], lists[pos], lists[neg], main_distance_function=fn)(model)
            assert got == acc[j][m]
        assert TripletEvaluator(lists["a"], lists[pos], lists[neg])(model) == max(acc[j])
    assert model.calls == 36
    # the gaps are those of the nine comparisons, and a tie is a close row whose bit is clear
    g = Q.gaps(dist)
    assert np.array_equal(g[:, 1], np.abs(dist[:, 0] - dist[:, 2])) and np.array_equal(g[:, 8], np.abs(dist[:, 7] - dist[:, 8]))
    assert not Q.close_rows(dist, D).any()
    q2 = q.copy()
    q2[0] = p[0]
    dist2, holds2 = Q.ref(a, p, q2, n)
    close = Q.close_rows(dist2, D)
    assert close[0] and not close[1:].any() and not holds2[0, [0, 3, 6]].any()
    # one tolerance away on the Manhattan distance only is close; six away is not
    tol = H.value_tol(H.L1_PLAIN, D)
    d3 = dist.copy()
    d3[1, 3:6] = [10.0, 10.0 + tol, 20.0]
    assert Q.close_rows(d3, D)[1]
    d3[1, 3:6] = [10.0, 10.0 + 6 * tol, 20.0]
    assert not Q.close_rows(d3, D)[1]


def test_case_gives_unit_rows_in_every_order():
    xs = Q.case(500, 64, 3)
    assert all(t.dtype == torch.float32 and t.shape == (500, 64) for t in xs)
    a, p, q, n = [t.double() for t in xs]
    assert all(float((t.norm(dim=1) - 1.0).abs().max()) < 1e-6 for t in (a, p, q, n))
    # the three noise levels of a row are distinct: no two of its distances are equal, and all six orders turn up
    d = np.stack([(a - x).norm(dim=1).numpy() for x in (p, q, n)], axis=1)
    assert (np.diff(np.sort(d, axis=1), axis=1) > 0).all()
    assert len({tuple(np.argsort(r)) for r in d}) == 6
    # the same seed gives the same case
    assert all(torch.equal(x, y) for x, y in zip(xs, Q.case(500, 64, 3)))


# ------------------------------------------------------------------ get_sequential_evaluator, exports, refusals
def test_get_sequential_evaluator_host_side(tmp_path, capsys):
    rows = rows_of_three_kinds()
    loss = GammaQuadrupletLoss(gamma=0.3)
    seq = get_sequential_evaluator(rows, loss, batch_size=8, name="dev", main_distance_function=SimilarityFunction.COSINE,
                                   use_amp=True, additional_loss_kwargs=["w"])
    assert isinstance(seq, evaluation.SequentialEvaluator)
    qe, le = seq.evaluators
    assert type(qe) is QuadrupletEvaluator and type(le) is QuadrupletLossEvaluator
    assert qe._gamma == 0.3 and qe.name == "dev" and qe.batch_size == 8 and qe._all_examples is rows
    assert qe.main_distance_function == SimilarityFunction.COSINE and qe.anchors == ["a0", "a1", "a2", "a3", "a4"]
    assert le._quadruplet_dataset is rows and le._quadruplet_loss is loss and le._batch_size == 8 and le._use_amp is True
    assert le._additional_loss_kwargs == ["w"] and le._additional_model_kwargs is None
    # a dataset to build the retrieval set from, and no readable file: refused, naming what is missing
    with pytest.raises(NotImplementedError, match="create_ir_evaluation_set"):
        get_sequential_evaluator(rows, loss, no_transform_dataset=rows)
    with pytest.raises(NotImplementedError, match="create_ir_evaluation_set"):
        get_sequential_evaluator(rows, loss, evaluation_queries_path=str(tmp_path / "missing.json"), no_transform_dataset=rows)
    assert "missing.json file could not be opened due to error" in capsys.readouterr().out
    # an unreadable file alone: the message, and the chain without the retrieval evaluator
    seq = get_sequential_evaluator(rows, loss, evaluation_queries_path=str(tmp_path / "missing.json"))
    assert len(seq.evaluators) == 2 and "could not be opened" in capsys.readouterr().out
    # a readable file: the retrieval evaluator first, every query with its own relevant documents as a set
    path = tmp_path / "queries.json"
    path.write_text(json.dumps({"queries": {"q0": "x", "q1": "y"}, "corpus": {"c0": "x", "c1": "y", "c2": "z"},
                                "relevant": {"q0": ["c0", "c2"], "q1": ["c1"]}}))
    seq = get_sequential_evaluator(rows, loss, evaluation_queries_path=str(path), no_transform_dataset=rows, name="dev",
                                   corpus_chunk_size=7, map_at_k=[3], main_score_function="cos_sim")
    ir = seq.evaluators[0]
    assert [type(e) for e in seq.evaluators] == [evaluation.InformationRetrievalEvaluator, QuadrupletEvaluator,
                                                 QuadrupletLossEvaluator]
    assert ir.relevant_docs == {"q0": {"c0", "c2"}, "q1": {"c1"}} and ir.queries == ["x", "y"] and ir.corpus == ["x", "y", "z"]
    assert ir.corpus_chunk_size == 7 and ir.map_at_k == [3] and ir.main_score_function == "cos_sim" and ir.name == "dev"
    assert ir.score_function_names == ["cos_sim", "dot_score"]


def test_dropin_exports_and_the_shadow_package_stays_losses_only():
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]
        from sentence_transformers import evaluation as E
        assert E.QuadrupletEvaluator is QuadrupletEvaluator and E.QuadrupletLossEvaluator is QuadrupletLossEvaluator
        assert E.get_sequential_evaluator is get_sequential_evaluator
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]
    assert not os.path.exists(os.path.join(ROOT, "dropin", "models", "evaluators.py"))


def test_library_binds_the_entry_point_and_cpu_tensors_are_refused():
    lib = _lib.load()
    assert lib.qst_version() >= 104
    assert hasattr(lib, "qst_quadruplet_eval") and len(_lib.SIGNATURES["qst_quadruplet_eval"][1]) == 10
    assert lib.qst_quadruplet_eval.argtypes == _lib.SIGNATURES["qst_quadruplet_eval"][1]
    # argument checks come before anything touches a device
    assert lib.qst_quadruplet_eval(None, None, None, None, 4, 8, None, None, None, None) == -1
    x = torch.randn(4, 8)
    with pytest.raises(_lib.QstError):
        S.quadruplet_eval(x, x, x, x)
    with pytest.raises(ValueError):
        S.quadruplet_eval(x, x, x[:, :4], x)
    assert list(inspect.signature(S.quadruplet_eval).parameters) == ["a", "p", "q", "n", "want_dist"]
    assert inspect.signature(S.quadruplet_eval).parameters["want_dist"].default is False
