"""GPU: qst_binary_eval (csrc/binary_eval.hip) against the sort-and-loop yardstick in binary_eval_helpers, exactly, and
evaluation.BinaryClassificationEvaluator on top of it: its scores, its one encode, its CSV file and a fit() that selects by it.

Every number but the average precision is compared for equality of the doubles; the average precision within n * 2^-52 of the
yardstick's fp64 value (binary_eval_helpers.ap_bound: at most n terms, each at most 1)."""
import csv
import ctypes
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import binary_eval_helpers as BH  # noqa: E402
from kernel_helpers import lib, ptr, stream  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import st_losses as S  # noqa: E402
from quadruplet_sentence_transformer_amd.evaluation import BinaryClassificationEvaluator  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample, SentenceTransformer  # noqa: E402

BAD_ARG, UNSUPPORTED = -1, -2
MIXED_FLAGS = (1, 0, 0, 1)
EXACT = (BH.ACC, BH.ACC_THR, BH.F1, BH.PREC, BH.REC, BH.F1_THR, BH.POS)


def call(lib, scores, labels, flags, ws=None, out=None):
    """lib.qst_binary_eval on device tensors scores [nsets, n] and labels [n]: the [nsets, 8] doubles."""
    nsets, n = scores.shape
    nbytes = lib.qst_binary_eval_workspace_bytes(n, nsets)
    assert nbytes == ((8 * n * nsets + 15) // 16) * 16 + 16 * n * nsets
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    if out is None:
        out = torch.empty(nsets, 8, dtype=torch.float64, device="cuda")
    rc = lib.qst_binary_eval(ptr(scores), ptr(labels), n, nsets, (ctypes.c_int32 * nsets)(*flags), ptr(out), ptr(ws), nbytes,
                             stream())
    assert rc == 0
    return out


_CASES = {}


def shared_case(lib, kind, n):
    """Four score rows over the labels of one case -- the case's own scores for either meaning of a high score, Gaussian
    distances and tie-heavy similarities -- with the yardstick on each and the kernel's output of ONE call, computed once and
    left unchanged."""
    if (kind, n) not in _CASES:
        seed = BH.case_seed(kind, n)
        s_high, labels = BH.case(kind, n, seed, True)
        s_low, labels_low = BH.case(kind, n, seed, False)
        assert np.array_equal(labels, labels_low)
        rows = np.stack([s_high, s_low, BH.case("gauss", n, seed + 7)[0], BH.case("ties", n, seed + 9)[0]])
        want = np.array([BH.expected(r, labels, bool(f)) for r, f in zip(rows, MIXED_FLAGS)], dtype=np.float64)
        scores, y = torch.from_numpy(rows).cuda(), torch.from_numpy(labels).cuda()
        got = call(lib, scores, y, MIXED_FLAGS).cpu().numpy()
        _CASES[(kind, n)] = (scores, y, want, got)
    return _CASES[(kind, n)]


def check(got, want, n, what):
    for s in range(len(want)):
        print(f"  {what} set {s}: got {got[s].tolist()}\n  {' ' * len(what)}    want {want[s].tolist()}; "
              f"|d ap| = {abs(got[s, BH.AP] - want[s, BH.AP]):.2e} (bound {BH.ap_bound(n):.2e})")
    for k in EXACT:
        assert np.array_equal(got[:, k], want[:, k]), (what, k)
    assert (np.abs(got[:, BH.AP] - want[:, BH.AP]) <= BH.ap_bound(n)).all(), what


# ------------------------------------------------------------------ 1. the kernel against the yardstick
@pytest.mark.parametrize("n", BH.SIZES)
@pytest.mark.parametrize("kind", BH.KINDS)
def test_kernel_equals_the_yardstick(lib, kind, n):
    scores, y, want, got = shared_case(lib, kind, n)
    check(got, want, n, f"{kind} n={n} four sets")
    # each meaning of a high score alone: one set, the same bits as in the call of four
    for s in (0, 1):
        alone = call(lib, scores[s:s + 1].contiguous(), y, MIXED_FLAGS[s:s + 1]).cpu().numpy()
        check(alone, want[s:s + 1], n, f"{kind} n={n} flag {MIXED_FLAGS[s]} alone")
        assert alone.tobytes() == got[s:s + 1].tobytes()
    # upstream's start values where nothing beats them
    if n == 1:
        assert got[:, :6].tolist() == [[0.0, -1.0, 0.0, 0.0, 0.0, 0.0]] * 4
    if kind == "all0":
        # the best cut is the first: its one pair is taken as positive, wrongly
        assert (got[:, BH.F1:BH.POS + 1] == 0).all() and (got[:, BH.ACC] == (n - 1) / n).all()
    if kind == "all1":
        assert (got[:, BH.AP] == 1.0).all() and (got[:, BH.POS] == n).all()


# ------------------------------------------------------------------ 2. determinism
def test_same_inputs_give_the_same_bits(lib):
    n = 4099
    scores, y, want, got = shared_case(lib, "ties", n)
    again = call(lib, scores, y, MIXED_FLAGS)
    assert again.cpu().numpy().tobytes() == got.tobytes()
    # what the workspace held before does not matter
    nbytes = lib.qst_binary_eval_workspace_bytes(n, 4)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")          # NaN in every reading
    assert call(lib, scores, y, MIXED_FLAGS, ws=ws).cpu().numpy().tobytes() == got.tobytes()
    # set 0 does not depend on what sets 1 to 3 hold
    other = scores.clone()
    other[1:] = torch.from_numpy(np.stack([BH.case("gauss", n, 100 + k)[0] for k in range(3)])).cuda()
    mixed = call(lib, other, y, (1, 1, 0, 0)).cpu().numpy()
    assert mixed[0].tobytes() == got[0].tobytes() and mixed[1:].tobytes() != got[1:].tobytes()
    # eight sets, the most: every odd one a copy of set 0 under the same flag
    eight = torch.cat([scores[:1], scores[2:3]] * 4).contiguous()
    out8 = call(lib, eight, y, (1, 0) * 4).cpu().numpy()
    assert all(out8[k].tobytes() == got[0].tobytes() for k in (0, 2, 4, 6))
    assert all(out8[k].tobytes() == got[2].tobytes() for k in (1, 3, 5, 7))


# ------------------------------------------------------------------ 3. refusals
def test_bad_arguments_are_refused_and_nothing_is_written(lib):
    n, nsets = 65, 2
    scores = torch.randn(nsets, n, device="cuda")
    y = torch.zeros(n, dtype=torch.int64, device="cuda")
    out = torch.full((nsets, 8), -7.0, dtype=torch.float64, device="cuda")
    nbytes = lib.qst_binary_eval_workspace_bytes(n, nsets)
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    flags = (ctypes.c_int32 * 8)(1, 0, 1, 0, 1, 0, 1, 0)
    names = ("scores", "labels", "n", "nsets", "flags", "out", "ws", "nbytes")
    good = dict(scores=ptr(scores), labels=ptr(y), n=n, nsets=nsets, flags=flags, out=ptr(out), ws=ptr(ws), nbytes=nbytes)
    run = lambda **k: lib.qst_binary_eval(*[k.get(nm, good[nm]) for nm in names], stream())  # noqa: E731
    for bad in (dict(scores=None), dict(labels=None), dict(flags=None), dict(out=None), dict(ws=None), dict(n=0), dict(n=-4),
                dict(nsets=0), dict(ws=ptr(ws) + 8), dict(nbytes=nbytes - 1), dict(nbytes=0)):
        assert run(**bad) == BAD_ARG, bad
    for bad in (dict(n=(1 << 20) + 1, nbytes=1 << 40), dict(nsets=9, nbytes=1 << 40)):
        assert run(**bad) == UNSUPPORTED, bad
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    assert run() == 0
    torch.cuda.synchronize()
    assert (out[:, BH.POS] == 0).all() and (out[:, BH.ACC] == (n - 1) / n).all()
    # the Python entry point
    with pytest.raises(ValueError):
        S.binary_eval_raw(scores, y[:3], [True, False])
    with pytest.raises(ValueError):
        S.binary_eval_raw(scores, y, [True])
    got = S.binary_eval_raw(scores, y, [True, False])
    assert got.dtype == torch.float64 and got.shape == (2, 8) and got.is_cuda and torch.equal(got, out)


# ------------------------------------------------------------------ 4. the static methods go through the kernel
def test_static_methods_on_the_device_equal_the_yardstick(lib, monkeypatch):
    calls = []
    raw = S.binary_eval_raw
    monkeypatch.setattr(S, "binary_eval_raw", lambda *a: (calls.append(a[0].shape), raw(*a))[1])
    for kind in BH.KINDS:
        for high in (True, False):
            scores, labels = BH.case(kind, 257, BH.case_seed(kind, 257), high)
            want = BH.expected(scores, labels, high)
            acc = BinaryClassificationEvaluator.find_best_acc_and_threshold(scores, labels, high)
            f1 = BinaryClassificationEvaluator.find_best_f1_and_threshold(torch.from_numpy(scores), labels.tolist(), high)
            assert all(type(v) is float for v in acc + f1)
            assert list(acc) == want[BH.ACC:BH.ACC_THR + 1] and list(f1) == want[BH.F1:BH.F1_THR + 1]
    assert calls == [(1, 257)] * 24
    # doubles (a list of Python floats) keep upstream's arithmetic in double: the host's restatement, not the kernel
    ties, labels = BH.case("ties", 257, 3)
    assert BinaryClassificationEvaluator.find_best_acc_and_threshold(ties.tolist(), labels, True) == BH.best_acc(ties, labels, True)
    assert len(calls) == 24
    with pytest.raises(ValueError):
        BinaryClassificationEvaluator.find_best_acc_and_threshold(np.array([0.5, np.inf], dtype=np.float32), [0, 1], True)


# ------------------------------------------------------------------ 5. the evaluator
WORDS = ("a man rides red horse two dogs play in park woman eats green apple near old bridge small cat sleeps under tall "
         "tree while rain falls on quiet town boats cross wide river").split()


def sent(i, n):
    rng = np.random.RandomState(i)
    return " ".join(rng.choice(WORDS, size=n))


def labelled_pairs(n):
    """n pairs over n // 2 + 8 sentences: every sentence turns up in several pairs; a pair that shares most of its words is
    labelled 1 three times out of four, any other one time out of four."""
    rng = np.random.RandomState(11)
    pool = [sent(i, 5 + i % 6) for i in range(n // 2)] + [sent(i, 5 + i % 6) + " today" for i in range(8)]
    first = [pool[i % len(pool)] for i in range(n)]
    second = [(pool[i % 8] + " today") if i % 2 else pool[(7 * i + 3) % len(pool)] for i in range(n)]
    labels = [int(rng.rand() < (0.75 if i % 2 else 0.25)) for i in range(n)]
    return first, second, labels


@pytest.fixture(scope="module")
def model():
    return SentenceTransformer("tiny-bert", device="cuda")


def read_csv(path):
    with open(path) as f:
        return list(csv.reader(f))


def test_evaluator_equals_the_yardstick_on_its_own_scores(model, tmp_path):
    s1, s2, labels = labelled_pairs(200)
    distinct = len(set(s1 + s2))
    assert distinct < 200 and 0 < sum(labels) < 200
    model.eval()
    ev = BinaryClassificationEvaluator(s1, s2, labels, name="dev", batch_size=16)
    scores = ev.pair_scores(model)
    assert list(scores) == ["cossim", "manhattan", "euclidean", "dot"]
    assert all(v.dtype == np.float32 and v.shape == (200,) for v in scores.values())
    assert (scores["manhattan"] >= 0).all() and (scores["euclidean"] >= 0).all()         # distances, not negated
    calls = []
    orig = model.encode
    model.encode = lambda *args, **kwargs: (calls.append(len(args[0])), orig(*args, **kwargs))[1]
    try:
        got = ev.compute_metrices(model)
        first = ev(model, output_path=str(tmp_path), epoch=0, steps=10)
        second = ev(model, output_path=str(tmp_path), epoch=1, steps=-1)
    finally:
        del model.encode
    assert calls == [distinct] * 3                          # one encode per evaluation, over the distinct sentences
    y = np.asarray(labels)
    assert list(got) == ["cossim", "manhattan", "euclidean", "dot"]
    names = ("accuracy", "accuracy_threshold", "f1", "precision", "recall", "f1_threshold", "ap")
    for key, high in zip(got, (True, False, False, True)):
        want = BH.expected(scores[key], y, high)
        assert list(got[key]) == list(names) and all(type(v) is float for v in got[key].values())
        print(f"  {key}: {got[key]}")
        for k, nm in enumerate(names):
            if nm == "ap":
                assert abs(got[key][nm] - want[k]) <= BH.ap_bound(200)
            else:
                assert got[key][nm] == want[k], (key, nm)
        assert 0.0 < got[key]["accuracy"] <= 1.0 and 0.0 < got[key]["f1"] <= 1.0
    assert first == second == max(got[k]["ap"] for k in got)
    assert os.listdir(tmp_path) == ["binary_classification_evaluation_dev_results.csv"]
    table = read_csv(tmp_path / ev.csv_file)
    assert table[0] == ev.csv_headers and len(table) == 3 and table[1][:2] == ["0", "10"] and table[2][:2] == ["1", "-1"]
    assert [float(v) for v in table[1][2:]] == [got[k][nm] for k in got for nm in names] == [float(v) for v in table[2][2:]]
    # an infinite score is refused
    inf = BinaryClassificationEvaluator(s1[:4], s2[:4], [0, 1, 1, 0])
    inf._device_scores = lambda m: torch.tensor([[0.5, float("inf"), 0.1, 0.2]] * 4, device="cuda")
    with pytest.raises(ValueError, match="NaN or infinite"):
        inf.compute_metrices(model)


def test_evaluator_selects_inside_fit(tmp_path):
    m = SentenceTransformer("tiny-bert", device="cuda")
    s1, s2, labels = labelled_pairs(32)
    examples = [InputExample(texts=[a, b], label=y) for a, b, y in zip(s1, s2, labels)]
    evaluator = BinaryClassificationEvaluator.from_input_examples(examples, batch_size=16)
    seen = []
    m.fit([(DataLoader(examples, batch_size=16, shuffle=False), S.OnlineContrastiveLoss(m))], evaluator=evaluator, epochs=1,
          warmup_steps=0, scheduler="constantlr", optimizer_params={"lr": 1e-4}, evaluation_steps=1, output_path=str(tmp_path),
          save_best_model=False, show_progress_bar=False, callback=lambda score, epoch, steps: seen.append((score, epoch, steps)))
    # two steps: an evaluation after each, and one at the end of the epoch
    table = read_csv(tmp_path / "eval" / "binary_classification_evaluation_results.csv")
    assert table[0] == evaluator.csv_headers and [r[:2] for r in table[1:]] == [["0", "1"], ["0", "2"], ["0", "-1"]]
    assert [s[1:] for s in seen] == [(0, 1), (0, 2), (0, -1)]
    assert all(type(s[0]) is float and 0.0 < s[0] <= 1.0 for s in seen)
    assert m.best_score == max(s[0] for s in seen)
    assert torch.isfinite(m._enc.params).all()
