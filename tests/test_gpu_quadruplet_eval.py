"""GPU: qst_quadruplet_eval (csrc/tuple_loss.hip) against the fp64 yardstick in quadruplet_eval_helpers, and the evaluators
on top of it (evaluation.QuadrupletEvaluator, QuadrupletLossEvaluator, get_sequential_evaluator) against what the project
already has: three TripletEvaluators composed by hand, and a hand loop over the loss model.
"""
import csv
import json
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import quadruplet_eval_helpers as Q  # noqa: E402
import tuple_loss_helpers as H  # noqa: E402
from kernel_helpers import lib, ptr, stream  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import st_losses as S  # noqa: E402
from quadruplet_sentence_transformer_amd.evaluation import (InformationRetrievalEvaluator, QuadrupletEvaluator,  # noqa: E402
                                                            QuadrupletLossEvaluator, SequentialEvaluator,
                                                            SimilarityFunction, TripletEvaluator,
                                                            get_sequential_evaluator)
from quadruplet_sentence_transformer_amd.losses import GammaQuadrupletLoss  # noqa: E402
from quadruplet_sentence_transformer_amd.quadruplet_model import QuadrupletSentenceTransformerLossModel  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import (InputExample, SentenceTransformer,  # noqa: E402
                                                                      batch_to_device)

BAD_ARG = -1
SHAPES = H.SHAPES + Q.LONG_SHAPES
METRIC_LABEL = ("cosine", "manhattan", "euclidean")


def dev(xs):
    return [t.cuda().contiguous() for t in xs]


def bits_of(flags):
    """int32 [B] -> bool numpy [B, 9]"""
    f = flags.cpu().numpy().astype(np.int64)
    return ((f[:, None] >> np.arange(9)[None, :]) & 1).astype(bool)


def compare_on(dist):
    """The nine strict comparisons made on a float32 numpy [B, 9] of distances, as the kernel defines its flags."""
    return np.stack([dist[:, 3 * m + lo] < dist[:, 3 * m + hi] for m in range(3) for lo, hi in Q.PAIRS], axis=1)


_CASES = {}


def shared_case(B, D):
    """The inputs of a shape, its yardstick and the kernel's output on it, computed once and left unchanged."""
    if (B, D) not in _CASES:
        xs = Q.case(B, D, B * 1000 + D)
        dist_ref, holds_ref = Q.ref(*xs)
        got = S.quadruplet_eval_raw(*dev(xs), want_dist=True)
        _CASES[(B, D)] = (xs, dist_ref, holds_ref, got)
    return _CASES[(B, D)]


def check_against_ref(dist, flags, dist_ref, holds_ref, B, D):
    got = dist.cpu().double().numpy()
    for m, metric in enumerate(Q.METRICS):
        tol = H.value_tol(metric, D)
        err = np.abs(got[:, 3 * m:3 * m + 3] - dist_ref[:, 3 * m:3 * m + 3]).max()
        print(f"  {METRIC_LABEL[m]}: max |d| = {err:.3e} (tol {tol:.1e})")
        torch.testing.assert_close(torch.from_numpy(got[:, 3 * m:3 * m + 3]), torch.from_numpy(dist_ref[:, 3 * m:3 * m + 3]),
                                   rtol=tol, atol=tol)
    close = Q.close_rows(dist_ref, D)
    bits = bits_of(flags)
    print(f"  close rows: {int(close.sum())} of {B}; flags that differ from the yardstick: {int((bits != holds_ref).sum())} "
          f"({int((bits != holds_ref)[~close].sum())} outside the close rows); accuracies {np.round(holds_ref.mean(0), 3)}")
    # conditions on the test data: if one trips, change the data and not the cap
    assert close.sum() <= 0.002 * B and (B > 64 or close.sum() == 0)
    assert np.array_equal(bits[~close], holds_ref[~close])


# ------------------------------------------------------------------ 1. the kernel against the yardstick
@pytest.mark.parametrize("B,D", SHAPES)
def test_kernel_matches_yardstick(lib, B, D):
    xs, dist_ref, holds_ref, (dist, flags, counts) = shared_case(B, D)
    assert dist.shape == (B, 9) and flags.shape == (B,) and counts.shape == (9,)
    assert flags.dtype == torch.int32 and counts.dtype == torch.int32
    check_against_ref(dist, flags, dist_ref, holds_ref, B, D)
    if B >= 64:     # both outcomes occur in every column
        assert ((holds_ref.mean(0) > 0.1) & (holds_ref.mean(0) < 0.9)).all()


# ------------------------------------------------------------------ 2. internal consistency, exact
@pytest.mark.parametrize("B,D", SHAPES)
def test_flags_counts_and_distances_agree_exactly(lib, B, D):
    xs, _, _, (dist, flags, counts) = shared_case(B, D)
    bits = bits_of(flags)
    assert np.array_equal(bits, compare_on(dist.cpu().numpy()))
    assert (flags.cpu().numpy() >> 9 == 0).all()
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), bits.sum(0))
    d = dev(xs)
    none, flags0, counts0 = S.quadruplet_eval_raw(*d, want_dist=False)
    assert none is None and torch.equal(flags0, flags) and torch.equal(counts0, counts)
    dist2, flags2, counts2 = S.quadruplet_eval_raw(*d, want_dist=True)
    assert torch.equal(dist2, dist) and torch.equal(flags2, flags) and torch.equal(counts2, counts)


# ------------------------------------------------------------------ 3. ties
@pytest.mark.parametrize("D", [33, 384, 2052])
def test_equal_columns_give_equal_distances_and_a_clear_bit(lib, D):
    B = 12
    a, p, q, n = Q.case(B, D, 77 + D)
    _, base, _ = S.quadruplet_eval_raw(*dev((a, p, q, n)))
    q2, n2 = q.clone(), n.clone()
    q2[:4] = p[:4].clone()          # rows 0-3: q == p
    n2[4:8] = q[4:8].clone()        # rows 4-7: n == q
    dist, flags, counts = S.quadruplet_eval_raw(*dev((a, p, q2, n2)), want_dist=True)
    bits, base_bits, dist = bits_of(flags), bits_of(base), dist.cpu().numpy()
    for m in range(3):
        pos_part, pos_neg, part_neg = 3 * m, 3 * m + 1, 3 * m + 2
        # q == p: d(a, p) and d(a, q) are the same bits, pos_part is clear; pos_neg has not moved, and part_neg now asks what
        # pos_neg asks
        assert np.array_equal(dist[:4, 3 * m], dist[:4, 3 * m + 1])
        assert not bits[:4, pos_part].any()
        assert np.array_equal(bits[:4, pos_neg], base_bits[:4, pos_neg])
        assert np.array_equal(bits[:4, part_neg], bits[:4, pos_neg])
        # n == q: part_neg is clear; pos_part has not moved, and pos_neg now asks what pos_part asks
        assert np.array_equal(dist[4:8, 3 * m + 1], dist[4:8, 3 * m + 2])
        assert not bits[4:8, part_neg].any()
        assert np.array_equal(bits[4:8, pos_part], base_bits[4:8, pos_part])
        assert np.array_equal(bits[4:8, pos_neg], bits[4:8, pos_part])
    assert np.array_equal(bits[8:], base_bits[8:])
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), bits.sum(0))


# ------------------------------------------------------------------ 4. paths
def test_unaligned_rows_take_the_scalar_path(lib):
    """D = 384 rows that start at an odd float of a larger buffer: not 16-byte aligned, so no 16-byte loads."""
    B, D = 64, 384
    xs, dist_ref, holds_ref, _ = shared_case(B, D)
    views = []
    for t in xs:
        buf = torch.zeros(B * D + 3, device="cuda")
        v = buf[1:1 + B * D].view(B, D)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        views.append(v)
    dist, flags, counts = S.quadruplet_eval_raw(*views, want_dist=True)
    check_against_ref(dist, flags, dist_ref, holds_ref, B, D)
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), bits_of(flags).sum(0))
    # one unaligned input among aligned ones is enough to leave the vector path
    d = dev(xs)
    dist1, flags1, _ = S.quadruplet_eval_raw(d[0], d[1], views[2], d[3], want_dist=True)
    check_against_ref(dist1, flags1, dist_ref, holds_ref, B, D)


@pytest.mark.parametrize("D", [1, 3, 4, 64, 260, 5120])
def test_single_row(lib, D):
    xs = Q.case(1, D, 5 + D) if D > 1 else [torch.tensor([[v]]) for v in (1.0, 0.5, -0.25, 3.0)]
    dist_ref, holds_ref = Q.ref(*xs)
    dist, flags, counts = S.quadruplet_eval(*dev(xs), want_dist=True)
    got = dist.cpu().double().numpy()
    for m, metric in enumerate(Q.METRICS):
        tol = H.value_tol(metric, D)
        torch.testing.assert_close(torch.from_numpy(got[:, 3 * m:3 * m + 3]), torch.from_numpy(dist_ref[:, 3 * m:3 * m + 3]),
                                   rtol=tol, atol=tol)
    bits = bits_of(flags)
    assert np.array_equal(bits, compare_on(dist.cpu().numpy()))
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), bits[0].astype(np.int64))
    if D > 1:
        assert not Q.close_rows(dist_ref, D).any() and np.array_equal(bits, holds_ref)
    else:
        # |1 - 0.5| < |1 + 0.25| < |1 - 3|: every Manhattan and Euclidean comparison holds
        assert bits[0, 3:].all()


# ------------------------------------------------------------------ 5. bad arguments
def test_bad_arguments_are_refused_and_nothing_is_written(lib):
    B, D = 4, 8
    x = torch.randn(B, D, device="cuda")
    dist = torch.full((B, 9), 7.0, device="cuda")
    flags = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    counts = torch.full((9,), -5, dtype=torch.int32, device="cuda")
    names = ("a", "p", "q", "n", "B", "D", "dist", "flags", "counts")
    good = dict(a=ptr(x), p=ptr(x), q=ptr(x), n=ptr(x), B=B, D=D, dist=ptr(dist), flags=ptr(flags), counts=ptr(counts))
    call = lambda **k: lib.qst_quadruplet_eval(*[k.get(nm, good[nm]) for nm in names], stream())  # noqa: E731
    for bad in (dict(B=0), dict(B=-3), dict(D=0), dict(D=-1), dict(a=None), dict(p=None), dict(q=None), dict(n=None),
                dict(flags=None), dict(counts=None), dict(flags=None, dist=None)):
        assert call(**bad) == BAD_ARG, bad
    torch.cuda.synchronize()
    assert (dist == 7.0).all() and (flags == -5).all() and (counts == -5).all()
    assert call() == 0 and call(dist=None) == 0
    torch.cuda.synchronize()
    # four equal inputs: every distance equal, no strict comparison holds
    assert (flags == 0).all() and (counts == 0).all()
    # the Python entry point checks shape and device as pair_metric does
    with pytest.raises(ValueError):
        S.quadruplet_eval(x, x, x[:2], x)
    with pytest.raises(ValueError):
        S.quadruplet_eval(x[:0], x[:0], x[:0], x[:0])
    with pytest.raises(S._lib.QstError):
        S.quadruplet_eval(x, x, x.cpu(), x)


# ------------------------------------------------------------------ 6. QuadrupletEvaluator end to end
WORDS = ("a man rides red horse two dogs play in park woman eats green apple near old bridge small cat sleeps under tall "
         "tree while rain falls on quiet town boats cross wide river").split()


def sent(i, n):
    rng = np.random.RandomState(i)
    return " ".join(rng.choice(WORDS, size=n))


def quadruplet_texts(n):
    """anchor, the anchor plus one word, half of the anchor's words, an unrelated sentence"""
    anchors = [sent(i, 8 + i % 5) for i in range(n)]
    positives = [s + " " + WORDS[(7 * i) % len(WORDS)] for i, s in enumerate(anchors)]
    partials = [" ".join(s.split()[:len(s.split()) // 2]) for s in anchors]
    negatives = [sent(5000 + i, 6 + i % 7) for i in range(n)]
    return anchors, positives, partials, negatives


def quadruplet_examples(n):
    return [InputExample(texts=list(t)) for t in zip(*quadruplet_texts(n))]


@pytest.fixture(scope="module")
def model():
    return SentenceTransformer("tiny-bert", device="cuda")


def read_csv(path):
    with open(path) as f:
        return list(csv.reader(f))


@pytest.mark.parametrize("fn", [None, SimilarityFunction.COSINE, SimilarityFunction.EUCLIDEAN, SimilarityFunction.MANHATTAN],
                         ids=lambda f: "max" if f is None else f.name.lower())
def test_quadruplet_evaluator_equals_three_triplet_evaluators(model, tmp_path, fn):
    a, p, q, n = quadruplet_texts(64)
    model.eval()
    # the composition the evaluator replaces: three TripletEvaluators (nine encodes) and the gamma formula
    kw = dict(main_distance_function=fn, batch_size=16, write_csv=False)
    ref = [TripletEvaluator(a, p, q, name="pos_part", **kw)(model), TripletEvaluator(a, p, n, name="pos_neg", **kw)(model),
           TripletEvaluator(a, q, n, name="part_neg", **kw)(model)]
    # rows on which the device's fp32 distances may order two values the other way than the host's fp64 ones
    emb = [np.asarray(model.encode(xs, batch_size=16), dtype=np.float64) for xs in (a, p, q, n)]
    n_close = int(Q.close_rows(Q.ref(*emb)[0], emb[0].shape[1]).sum())
    print(f"  n_close = {n_close} of 64")
    assert n_close <= 6, "change the sentences, not the bound"
    for gamma in (0.6, 0.0):
        out = tmp_path / f"g{gamma}"
        out.mkdir()
        ev = QuadrupletEvaluator(a, p, q, n, gamma=gamma, main_distance_function=fn, batch_size=16)
        calls = []
        orig = model.encode
        model.encode = lambda *args, **kwargs: (calls.append(len(args[0])), orig(*args, **kwargs))[1]
        try:
            score = ev(model, output_path=str(out), epoch=1, steps=20)
        finally:
            del model.encode
        assert calls == [64, 64, 64, 64]
        row = read_csv(out / "quadruplet_evaluation_results.csv")[1]
        assert row[:2] == ["1", "20"]
        got = [float(v) for v in row[2:5]]
        print(f"  gamma {gamma}: accuracies {got} (composition {ref}), score {score:.6f}")
        for g, r in zip(got, ref):
            assert abs(g - r) <= n_close / 64 + 1e-12
        assert score == float(row[5]) == ((1 - gamma) * got[0] + gamma * got[2] + got[1]) / 2
        assert abs(score - ((1 - gamma) * ref[0] + gamma * ref[2] + ref[1]) / 2) <= n_close / 64 + 1e-12


def test_quadruplet_evaluator_files(model, tmp_path):
    a, p, q, n = quadruplet_texts(64)
    model.eval()
    ev = QuadrupletEvaluator(a, p, q, n, name="dev", batch_size=16)
    counts, N = ev.quadruplet_counts(model)
    assert N == 64 and counts.shape == (9,) and (counts >= 0).all() and (counts <= 64).all()
    ev(model, output_path=str(tmp_path), epoch=0, steps=-1)
    names = ["quadruplet_evaluation_dev_results.csv", "triplet_evaluation_part_neg_results.csv",
             "triplet_evaluation_pos_neg_results.csv", "triplet_evaluation_pos_part_results.csv"]
    assert sorted(os.listdir(tmp_path)) == names
    ev(model, output_path=str(tmp_path), epoch=1, steps=7)
    quad = read_csv(tmp_path / names[0])
    assert quad[0] == ["epoch", "steps", "pos_part_accuracy", "pos_neg_accuracy", "part_neg_accuracy", "global_accuracy"]
    assert len(quad) == 3 and quad[1][:2] == ["0", "-1"] and quad[2][:2] == ["1", "7"]
    for j, t in enumerate(("pos_part", "pos_neg", "part_neg")):
        table = read_csv(tmp_path / f"triplet_evaluation_{t}_results.csv")
        assert table[0] == ["epoch", "steps", "accuracy_cosinus", "accuracy_manhattan", "accuracy_euclidean"]
        assert len(table) == 3 and table[2][:2] == ["1", "7"]
        assert [float(v) for v in table[1][2:]] == [counts[3 * m + j] / 64 for m in range(3)]
        assert float(quad[1][2 + j]) == max(float(v) for v in table[1][2:])
    # write_csv=False and output_path=None write nothing
    QuadrupletEvaluator(a, p, q, n, write_csv=False)(model, output_path=str(tmp_path))
    ev(model)
    assert sorted(os.listdir(tmp_path)) == names and len(read_csv(tmp_path / names[0])) == 3


# ------------------------------------------------------------------ 7. QuadrupletLossEvaluator
def hand_loop(model, loss, examples, batch_size):
    lm = QuadrupletSentenceTransformerLossModel(model, loss)
    avg = torch.zeros((), device="cuda")
    with torch.no_grad():
        for i, (features, labels) in enumerate(DataLoader(examples, batch_size=batch_size, shuffle=False,
                                                          collate_fn=model.smart_batching_collate)):
            value = lm([batch_to_device(f, model.device) for f in features], labels.to(model.device))
            avg += (value - avg) / (i + 1)
    return avg


def test_quadruplet_loss_evaluator(model, tmp_path):
    examples = quadruplet_examples(40)                      # 16 + 16 + 8: a partial last batch
    loss = GammaQuadrupletLoss(gamma=0.6, margin_pos_neg=1.0, margin_pos_part=0.5, margin_part_neg=0.5)
    model.eval()
    ref = hand_loop(model, loss, examples, 16)
    ev = QuadrupletLossEvaluator(examples, loss, batch_size=16)
    got = ev(model, output_path=str(tmp_path), epoch=0, steps=10)
    assert torch.is_tensor(got) and got.dim() == 0 and got.is_cuda
    assert not model.training and ref.item() > 0
    print(f"  average loss {got.item():.7f} (hand loop {ref.item():.7f})")
    torch.testing.assert_close(got, ref, rtol=1e-6, atol=0)
    got2 = ev(model, output_path=str(tmp_path), epoch=1, steps=-1)
    with open(tmp_path / "_quadruplet_loss_eval.json") as f:
        log = json.load(f)
    assert log == {"epoch": [0, 1], "steps": [10, -1], "average_loss": [got.item(), got2.item()]}
    assert os.listdir(tmp_path) == ["_quadruplet_loss_eval.json"]
    # no output path: nothing written, the loss returned
    before = set(os.listdir(os.getcwd()))
    torch.testing.assert_close(ev(model), ref, rtol=1e-6, atol=0)
    assert set(os.listdir(os.getcwd())) == before and os.listdir(tmp_path) == ["_quadruplet_loss_eval.json"]
    # quadruplet dicts (a list with one entry is drawn from), and (example, label) rows
    keys = ("reference", "positive", "part_positive", "negative")
    dicts = [dict(zip(keys, [ex.texts[0], [ex.texts[1]], ex.texts[2], [ex.texts[3]]])) for ex in examples]
    torch.testing.assert_close(QuadrupletLossEvaluator(dicts, loss, batch_size=16)(model), ref, rtol=1e-6, atol=0)
    torch.testing.assert_close(QuadrupletLossEvaluator([(ex, 0) for ex in examples], loss, batch_size=16)(model), ref,
                               rtol=1e-6, atol=0)
    # the model's mode is left alone
    model.train()
    ev(model)
    assert model.training
    model.eval()


# ------------------------------------------------------------------ 8. get_sequential_evaluator
def test_get_sequential_evaluator(model, tmp_path):
    examples = quadruplet_examples(32)
    loss = GammaQuadrupletLoss(gamma=0.3)
    model.eval()
    seq = get_sequential_evaluator(examples, loss, batch_size=16)
    assert isinstance(seq, SequentialEvaluator)
    assert [type(e) for e in seq.evaluators] == [QuadrupletEvaluator, QuadrupletLossEvaluator]
    assert seq.evaluators[0]._gamma == 0.3 and seq.evaluators[0].batch_size == 16
    score = seq(model, output_path=str(tmp_path), epoch=0, steps=1)
    torch.testing.assert_close(score, QuadrupletLossEvaluator(examples, loss, batch_size=16)(model), rtol=1e-6, atol=0)
    assert {"quadruplet_evaluation_results.csv", "_quadruplet_loss_eval.json"} <= set(os.listdir(tmp_path))
    # with a queries file: the retrieval evaluator comes first, each query with its own relevant set
    a, p, q, n = quadruplet_texts(8)
    queries = {"queries": {"q0": a[0], "q1": a[1]}, "corpus": {f"c{i}": t for i, t in enumerate(p + n)},
               "relevant": {"q0": ["c0", "c8"], "q1": ["c1"]}}
    path = tmp_path / "queries.json"
    path.write_text(json.dumps(queries))
    seq3 = get_sequential_evaluator(examples, loss, evaluation_queries_path=str(path), batch_size=16, map_at_k=[5],
                                    accuracy_at_k=[1, 3], precision_recall_at_k=[1, 3], mrr_at_k=[5], ndcg_at_k=[5])
    assert [type(e) for e in seq3.evaluators] == [InformationRetrievalEvaluator, QuadrupletEvaluator, QuadrupletLossEvaluator]
    assert seq3.evaluators[0].relevant_docs == {"q0": {"c0", "c8"}, "q1": {"c1"}}
    out3 = tmp_path / "three"
    out3.mkdir()
    torch.testing.assert_close(seq3(model, output_path=str(out3)), score, rtol=1e-6, atol=0)
    assert "Information-Retrieval_evaluation_results.csv" in os.listdir(out3)


# ------------------------------------------------------------------ 9. inside fit
def test_sequential_evaluator_inside_fit(tmp_path):
    m = SentenceTransformer("tiny-bert", device="cuda")
    examples = quadruplet_examples(64)
    loss = GammaQuadrupletLoss(gamma=0.6, margin_pos_neg=1.0, margin_pos_part=0.5, margin_part_neg=0.5)
    lm = QuadrupletSentenceTransformerLossModel(m, loss)
    evaluator = get_sequential_evaluator(examples[:32], loss, batch_size=16)
    scores = []
    m.fit([(DataLoader(examples, batch_size=16, shuffle=False), lm)], evaluator=evaluator, epochs=1, warmup_steps=0,
          scheduler="constantlr", optimizer_params={"lr": 1e-4}, evaluation_steps=2, output_path=str(tmp_path),
          save_best_model=False, show_progress_bar=False, callback=lambda score, epoch, steps: scores.append((score, epoch, steps)))
    # four steps: evaluations after steps 2 and 4, and at the end of the epoch
    table = read_csv(tmp_path / "eval" / "quadruplet_evaluation_results.csv")
    assert len(table) == 4 and [r[:2] for r in table[1:]] == [["0", "2"], ["0", "4"], ["0", "-1"]]
    assert all(0.0 <= float(v) <= 1.0 for r in table[1:] for v in r[2:])
    with open(tmp_path / "eval" / "_quadruplet_loss_eval.json") as f:
        log = json.load(f)
    assert log["epoch"] == [0, 0, 0] and log["steps"] == [2, 4, -1] and len(log["average_loss"]) == 3
    assert [s[1:] for s in scores] == [(0, 2), (0, 4), (0, -1)]
    assert all(torch.is_tensor(s[0]) and torch.isfinite(s[0]) for s in scores)
    assert [s[0].item() for s in scores] == log["average_loss"]
    assert torch.isfinite(m._enc.params).all()
