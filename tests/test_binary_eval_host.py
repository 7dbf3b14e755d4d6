"""CPU: BinaryClassificationEvaluator's host side -- the yardstick of the GPU test (binary_eval_helpers) against sklearn,
the numpy restatement behind the two static methods against that yardstick, the constructor surface, the CSV layout, the
drop-in export and the library's new symbols. No kernel runs."""
import ctypes
import inspect
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import quadruplet_sentence_transformer_amd  # noqa: F401
import binary_eval_helpers as BH
from quadruplet_sentence_transformer_amd import _lib, evaluation, st_losses as S
from quadruplet_sentence_transformer_amd.evaluation import BinaryClassificationEvaluator, SentenceEvaluator
from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SIZES = (1, 2, 3, 12, 63, 64, 65, 257, 1000)
EMPTY = inspect.Parameter.empty


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    """The static methods take the numpy path: this file checks the restatement, wherever it runs."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def all_cases(sizes):
    for kind in BH.KINDS:
        for n in sizes:
            for high in (True, False):
                yield kind, n, high, BH.case(kind, n, BH.case_seed(kind, n), high)


# ------------------------------------------------------------------ the yardstick
def test_yardstick_ap_equals_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    import warnings
    worst = 0.0
    for kind, n, high, (scores, labels) in all_cases(HOST_SIZES):
        got = BH.average_precision(scores, labels, high)
        if labels.sum() == 0:
            assert got == 0.0
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = metrics.average_precision_score(labels, scores.astype(np.float64) * (1 if high else -1))
        worst = max(worst, abs(got - ref))
        assert abs(got - ref) < 1e-12, (kind, n, high)
    print(f"  largest |ap - sklearn| = {worst:.2e}")


def test_yardstick_ap_is_the_counting_sum():
    """(1 / T) * sum over the positives of TP_ge / N_ge, pairs of equal score included in both counts."""
    for kind, n, high, (scores, labels) in all_cases((3, 65, 257)):
        if labels.sum() == 0:
            continue
        s = scores.astype(np.float64) * (1 if high else -1)
        total = Fraction(0)
        for i in np.flatnonzero(labels):
            ge = s >= s[i]
            total += Fraction(int(labels[ge].sum()), int(ge.sum()))
        assert abs(BH.average_precision(scores, labels, high) - float(total / int(labels.sum()))) <= BH.ap_bound(n)


def test_multi_case_reaches_both_maxima_at_several_cuts():
    for n in (12, 65, 257, 1000):
        for high in (True, False):
            scores, labels = BH.case("multi", n, BH.case_seed("multi", n), high)
            rows = BH.sorted_rows(scores, labels, high)
            y = np.array([r[1] for r in rows])
            hits, T = np.cumsum(y)[:-1], int(y.sum())
            count = 2 * hits - np.arange(1, n)
            f1 = [Fraction(2 * int(c), e + T) for e, c in enumerate(hits, start=1)]
            assert (count == count.max()).sum() >= 4 and f1.count(max(f1)) >= 2
            # the walk keeps the first of them
            k = n // 12
            assert BH.best_acc(scores, labels, high)[1] == (rows[k - 1][0] + rows[k][0]) / 2
            assert BH.best_f1(scores, labels, high)[3] == (rows[7 * k - 1][0] + rows[7 * k][0]) / 2


def test_zero_case_holds_both_zeros_and_sorts_them_as_equal():
    scores, labels = BH.case("zeros", 64, BH.case_seed("zeros", 64))
    assert np.signbit(scores[scores == 0]).any() and not np.signbit(scores[scores == 0]).all()
    rows = BH.sorted_rows(scores, labels, True)
    zeros = [i for i, r in enumerate(rows) if r[0] == 0]
    assert zeros == list(range(zeros[0], zeros[0] + len(zeros)))
    # inside the run: input order
    assert [np.signbit(rows[i][0]) for i in zeros] == [bool(np.signbit(v)) for v in scores if v == 0]


# ------------------------------------------------------------------ the numpy restatement behind the static methods
def test_static_methods_equal_the_yardstick_exactly():
    for kind, n, high, (scores, labels) in all_cases(HOST_SIZES):
        want = BH.expected(scores, labels, high)
        acc = BinaryClassificationEvaluator.find_best_acc_and_threshold(scores, labels, high)
        f1 = BinaryClassificationEvaluator.find_best_f1_and_threshold(scores, labels, high)
        assert all(type(v) is float for v in acc + f1)
        assert list(acc) == want[BH.ACC:BH.ACC_THR + 1], (kind, n, high)
        assert list(f1) == want[BH.F1:BH.F1_THR + 1], (kind, n, high)


def test_static_methods_take_lists_tensors_and_doubles():
    scores, labels = BH.case("ties", 65, 5)
    want_acc, want_f1 = BH.best_acc(scores, labels, True), BH.best_f1(scores, labels, True)
    for s, y in ((scores.tolist(), labels.tolist()), (torch.from_numpy(scores), torch.from_numpy(labels)),
                 (scores.astype(np.float64), labels.astype(bool))):
        assert BinaryClassificationEvaluator.find_best_acc_and_threshold(s, y, True) == want_acc
        assert BinaryClassificationEvaluator.find_best_f1_and_threshold(s, y, True) == want_f1
    # double scores keep their thresholds in double, as upstream's (a + b) / 2 on them does
    d = np.array([0.1, 0.2, 0.7, 0.3], dtype=np.float64)
    y = np.array([0, 0, 1, 1])
    assert BinaryClassificationEvaluator.find_best_acc_and_threshold(d, y, True) == BH.best_acc(d, y, True) == (1.0, 0.25)
    assert BinaryClassificationEvaluator.find_best_acc_and_threshold([], [], True) == (0.0, -1.0)
    assert BinaryClassificationEvaluator.find_best_f1_and_threshold([], [], True) == (0.0, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        BinaryClassificationEvaluator.find_best_acc_and_threshold([0.5, float("nan")], [0, 1], True)
    with pytest.raises(ValueError):
        BinaryClassificationEvaluator.find_best_f1_and_threshold([0.5, 0.25], [0, 2], True)
    with pytest.raises(ValueError):
        BinaryClassificationEvaluator.find_best_f1_and_threshold([0.5, 0.25], [0], True)


# ------------------------------------------------------------------ the surface
def test_constructor_surface():
    sig = {k: p.default for k, p in inspect.signature(BinaryClassificationEvaluator.__init__).parameters.items() if k != "self"}
    assert sig == {"sentences1": EMPTY, "sentences2": EMPTY, "labels": EMPTY, "name": "", "batch_size": 32,
                   "show_progress_bar": False, "write_csv": True}
    assert issubclass(BinaryClassificationEvaluator, SentenceEvaluator)
    ev = BinaryClassificationEvaluator(["a", "b"], ["c", "d"], [1, 0], name="dev", batch_size=8)
    assert (ev.sentences1, ev.sentences2, ev.labels, ev.name, ev.batch_size) == (["a", "b"], ["c", "d"], [1, 0], "dev", 8)
    assert ev.write_csv is True and ev.show_progress_bar is False
    assert ev.csv_file == "binary_classification_evaluation_dev_results.csv"
    assert BinaryClassificationEvaluator(["a"], ["b"], [1]).csv_file == "binary_classification_evaluation_results.csv"
    for bad in ((["a", "b"], ["c"], [1, 0]), (["a", "b"], ["c", "d"], [1]), (["a", "b"], ["c", "d"], [1, 2]),
                (["a", "b"], ["c", "d"], [0.5, 1])):
        with pytest.raises(AssertionError):
            BinaryClassificationEvaluator(*bad)
    assert hasattr(BinaryClassificationEvaluator, "compute_metrices")
    for fn in ("find_best_acc_and_threshold", "find_best_f1_and_threshold"):
        assert isinstance(inspect.getattr_static(BinaryClassificationEvaluator, fn), staticmethod)
        assert list(inspect.signature(getattr(BinaryClassificationEvaluator, fn)).parameters) == \
            ["scores", "labels", "high_score_more_similar"]


def test_from_input_examples():
    examples = [InputExample(texts=["a", "b"], label=1), InputExample(texts=["c", "d"], label=0)]
    ev = BinaryClassificationEvaluator.from_input_examples(examples, name="x", batch_size=4, write_csv=False)
    assert (ev.sentences1, ev.sentences2, ev.labels) == (["a", "c"], ["b", "d"], [1, 0])
    assert ev.name == "x" and ev.batch_size == 4 and ev.write_csv is False


def test_csv_headers_in_order():
    ev = BinaryClassificationEvaluator(["a"], ["b"], [1])
    want = ["epoch", "steps"]
    for score in ("cossim", "manhattan", "euclidean", "dot"):
        want += [f"{score}_accuracy", f"{score}_accuracy_threshold", f"{score}_f1", f"{score}_precision", f"{score}_recall",
                 f"{score}_f1_threshold", f"{score}_ap"]
    assert ev.csv_headers == want and len(want) == 30


class FixedMetrics(BinaryClassificationEvaluator):
    def compute_metrices(self, model):
        return {s: {m: 0.01 * (10 * i + j) for j, m in enumerate(self._METRICS)} for i, s in enumerate(self._SCORES)}


def test_call_returns_the_largest_ap_and_appends_rows(tmp_path):
    import csv
    ev = FixedMetrics(["a"], ["b"], [1], name="dev")
    assert ev(None, output_path=str(tmp_path), epoch=0, steps=5) == 0.36
    assert ev(None, output_path=str(tmp_path), epoch=1, steps=-1) == 0.36
    assert os.listdir(tmp_path) == ["binary_classification_evaluation_dev_results.csv"]
    with open(tmp_path / ev.csv_file) as f:
        table = list(csv.reader(f))
    assert table[0] == ev.csv_headers and len(table) == 3
    assert table[1][:2] == ["0", "5"] and table[2][:2] == ["1", "-1"]
    assert [float(v) for v in table[1][2:]] == [0.01 * (10 * i + j) for i in range(4) for j in range(7)]
    # nothing is written without an output path, or with write_csv=False
    ev(None)
    FixedMetrics(["a"], ["b"], [1], write_csv=False)(None, output_path=str(tmp_path))
    assert len(os.listdir(tmp_path)) == 1


def test_too_many_pairs_are_refused_before_anything_is_encoded():
    n = S.BINARY_EVAL_MAX_PAIRS + 1
    ev = BinaryClassificationEvaluator(["a"] * n, ["b"] * n, np.zeros(n, dtype=np.int64))
    with pytest.raises(_lib.QstError, match=r"1048576 \(2\^20\)"):
        ev.compute_metrices(None)


def test_dropin_import_resolves():
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]
        from sentence_transformers.evaluation import BinaryClassificationEvaluator as E
        assert E is BinaryClassificationEvaluator
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]
    assert "BinaryClassificationEvaluator" in evaluation.__doc__


# ------------------------------------------------------------------ the library
def test_library_binds_the_entry_points_and_checks_arguments_first():
    lib = _lib.load()
    assert lib.qst_version() >= 109
    for name in ("qst_binary_eval", "qst_binary_eval_workspace_bytes"):
        assert hasattr(lib, name) and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["qst_binary_eval"][1]) == 9
    ws = lib.qst_binary_eval_workspace_bytes
    # a 64-bit order word and a 16-byte record per pair and set, the words rounded up to 16 bytes
    assert ws(1, 1) == 16 + 16 and ws(3, 1) == 32 + 48 and ws(1000, 4) == 24 * 4000 and ws(1 << 20, 8) == 24 * 8 << 20
    assert ws(0, 1) == 0 and ws(5, 0) == 0 and ws((1 << 20) + 1, 1) == 0 and ws(5, 9) == 0
    # refusals come before anything touches a device
    flags = (ctypes.c_int32 * 8)(1, 0, 0, 1, 1, 1, 1, 1)
    assert lib.qst_binary_eval(None, None, 4, 1, flags, None, None, 0, None) == -1
    assert lib.qst_binary_eval(16, 16, 4, 1, None, 16, 16, 1 << 20, None) == -1
    assert lib.qst_binary_eval(16, 16, 0, 1, flags, 16, 16, 1 << 20, None) == -1
    assert lib.qst_binary_eval(16, 16, 4, 0, flags, 16, 16, 1 << 20, None) == -1
    assert lib.qst_binary_eval(16, 16, 4, 1, flags, 16, 24, 1 << 20, None) == -1          # workspace not 16-byte aligned
    assert lib.qst_binary_eval(16, 16, 4, 1, flags, 16, 16, ws(4, 1) - 1, None) == -1     # ... or short
    assert lib.qst_binary_eval(16, 16, (1 << 20) + 1, 1, flags, 16, 16, 1 << 40, None) == -2
    assert lib.qst_binary_eval(16, 16, 4, 9, flags, 16, 16, 1 << 40, None) == -2
    x = torch.zeros(1, 4)
    with pytest.raises(ValueError):
        S.binary_eval_raw(x, torch.zeros(3, dtype=torch.int64), [True])
    with pytest.raises(ValueError):
        S.binary_eval_raw(x, torch.zeros(4, dtype=torch.int64), [True, False])
