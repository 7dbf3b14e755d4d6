"""GPU: the row-wise pair and triplet losses (csrc/tuple_loss.hip: qst_pair_metric, qst_pair_loss, qst_triplet_loss), the
loss classes on top of them (st_losses.py) and EmbeddingSimilarityEvaluator, against the yardstick in tuple_loss_helpers:
sentence-transformers 2.2.2's formulas in torch ops, fp64 on the CPU with autograd."""
import csv
import os

import numpy as np
import pytest
import torch
from torch import nn
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import tuple_loss_helpers as H  # noqa: E402
from tuple_loss_helpers import (RED, check_grads, check_value, dev, f64, margin_between, pair_labels,  # noqa: E402
                                upstream)
from kernel_helpers import lib, ptr, stream  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import st_losses as S  # noqa: E402
from quadruplet_sentence_transformer_amd.evaluation import EmbeddingSimilarityEvaluator, SimilarityFunction  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample, SentenceTransformer  # noqa: E402

BAD_ARG = -1
# Past one trip of the one-workgroup second stages (row_sum_kernel, online_select_kernel: 1024 rows a trip): a third,
# partial trip on the scalar path (D % 4 != 0) and on the vector path. Local: H.SHAPES is shared with the host tests.
LONG_SHAPES = [(2500, 33), (2500, 64)]


# ------------------------------------------------------------------ 1. kernel parity
@pytest.mark.parametrize("B,D", H.SHAPES)
@pytest.mark.parametrize("metric", sorted(H.METRIC_NAMES), ids=lambda m: H.METRIC_NAMES[m])
def test_pair_metric_matches_yardstick(lib, B, D, metric):
    u, v = H.rows(B, D, 2, B * 1000 + D)
    xs = f64((u, v))
    ref = H.metric_ref(*xs, metric)
    w = upstream(B, 0)
    (ref * w.double()).sum().backward()
    out, grads = S.pair_metric_raw(dev(u), dev(v), metric, grad_out=dev(w), want_grads=True)
    if metric == H.DOT:
        # no tolerance of the project's covers a raw dot product (it can cancel to 0 while its terms are O(1)), so the
        # bound is the a-priori one of the summation: every product passes through at most D/64 + 10 fp32 additions (a
        # lane's chain, the wave tree) and one multiplication, each within 2^-24 relative: |err| <= n * 2^-24 * sum |u v|
        bound = (D / 64 + 11) * 2.0 ** -24 * (u.double() * v.double()).abs().sum(1)
        err = (out.cpu().double() - ref.detach()).abs()
        print(f"  dot: max |d| = {err.max().item():.3e}, bound {bound.min().item():.3e}")
        assert (err <= bound).all()
    else:
        check_value(out, ref, metric, B, D, 0)
    check_grads(grads, xs)


@pytest.mark.parametrize("B,D", H.SHAPES + LONG_SHAPES)
@pytest.mark.parametrize("kind,metric", [(H.MSE, H.COS_SIM)] + [(H.CONTRASTIVE, m) for m in H.DISTANCES],
                         ids=lambda x: None)
def test_pair_loss_matches_yardstick(lib, B, D, kind, metric):
    u, v = H.rows(B, D, 2, B * 1000 + D + 1)
    y = pair_labels(B, kind, B + D)
    margin = margin_between(H.metric_ref(u.double(), v.double(), metric), metric, D) if kind == H.CONTRASTIVE else 0.0
    for red_name, red in RED:
        xs = f64((u, v))
        ref = H.mse_ref(*xs, y, red_name) if kind == H.MSE else H.contrastive_ref(*xs, y, metric, margin, red_name)
        w = upstream(B, red)
        (ref * w.double()).sum().backward()
        out, grads = S.pair_loss_raw(dev(u), dev(v), dev(y), kind, metric, margin, red, grad_out=dev(w), want_grads=True)
        check_value(out, ref, metric, B, D, red)
        check_grads(grads, xs)


# (1025, 64) is not among them: with this test's seed a cosine row lies within five tolerances of the hinge there
@pytest.mark.parametrize("B,D", H.SHAPES + LONG_SHAPES)
@pytest.mark.parametrize("metric", H.DISTANCES, ids=lambda m: H.METRIC_NAMES[m])
def test_triplet_loss_matches_yardstick(lib, B, D, metric):
    a, p, n = H.rows(B, D, 3, B * 1000 + D + 2)
    dap, dan = H.metric_ref(a.double(), p.double(), metric), H.metric_ref(a.double(), n.double(), metric)
    margin = margin_between(dan - dap, metric, D)
    for red_name, red in RED:
        xs = f64((a, p, n))
        ref = H.triplet_ref(*xs, metric, margin, red_name)
        w = upstream(B, red)
        (ref * w.double()).sum().backward()
        out, grads = S.triplet_loss_raw(dev(a), dev(p), dev(n), metric, margin, red, grad_out=dev(w), want_grads=True)
        check_value(out, ref, metric, B, D, red)
        check_grads(grads, xs)


# ------------------------------------------------------------------ 2. OnlineContrastiveLoss: the selection
# online_case seeds for which the conditions on the test data below hold for all three metrics (searched on the CPU; 1 where
# nothing is listed). Past 1024 rows: the first row of a second trip of online_select_kernel's loops, and a third, partial trip
ONLINE_SEED = {(128, 1024): 2, (1025, 64): 5, (2500, 64): 1, (2500, 33): 3}


@pytest.mark.parametrize("B,D", H.ONLINE_SHAPES + [(16, 5120), (7, 33), (1025, 64), (2500, 64), (2500, 33)])
@pytest.mark.parametrize("metric", H.DISTANCES, ids=lambda m: H.METRIC_NAMES[m])
def test_online_contrastive_selects_what_the_yardstick_selects(lib, B, D, metric):
    u, v, y = H.online_case(B, D, ONLINE_SEED.get((B, D), 1))
    xs = f64((u, v))
    d = H.metric_ref(*xs, metric).detach()
    pos_sel, neg_sel, t_pos, t_neg = H.online_selection(d, y)
    # conditions on the test data (an error in the data if violated, not a skip): both selections are proper, non-empty
    # subsets, and no distance is closer to its threshold than five times the error the project accepts on a distance
    assert 0 < int(pos_sel.sum()) < int((y == 1).sum()) and 0 < int(neg_sel.sum()) < int((y == 0).sum())
    gap = min((d[y == 1] - t_pos).abs().min().item(), (d[y == 0] - t_neg).abs().min().item())
    assert gap >= 5 * H.value_tol(metric, D), gap
    margin = 1.05 * float(d.max()) + 0.1         # every selected negative is inside the margin: its gradient is not zero
    for red in (0, 1, 2):                        # always a sum: `reduction` changes nothing
        for x in xs:
            x.grad = None
        ref = H.online_ref(*xs, y, metric, margin)
        (ref * 1.7).backward()
        out, grads = S.pair_loss_raw(dev(u), dev(v), dev(y), H.ONLINE, metric, margin, red, grad_out=dev(torch.tensor([1.7])),
                                     want_grads=True)
        assert out.shape == (1,)
        selected = int((grads[0].abs().sum(1) != 0).sum())
        print(f"  selected rows: {selected} of {B} (yardstick {int(pos_sel.sum())} + {int(neg_sel.sum())})")
        assert selected == int(pos_sel.sum()) + int(neg_sel.sum())
        assert torch.equal((grads[0].abs().sum(1) != 0).cpu(), pos_sel | neg_sel)
        check_value(out, ref, metric, int(pos_sel.sum() + neg_sel.sum()), D, 1)
        check_grads(grads, xs)


def online_raw(u, v, y, metric=H.COS_DIST, margin=0.5):
    out, grads = S.pair_loss_raw(dev(u), dev(v), dev(y), H.ONLINE, metric, margin, 1, want_grads=True)
    return out.cpu().double()[0], [g.cpu().double() for g in grads]


@pytest.mark.parametrize("labels", ["all0", "all1", "one_positive", "B1_pos", "B1_neg", "half", "late_positives"])
def test_online_contrastive_edge_cases(lib, labels):
    # late_positives: 2049 rows (the third trip of online_select_kernel's loops is a single row) whose positives all sit at
    # rows >= 1024 (odd rows, so that last row is a negative): their count, maximum and sum come from the second trip alone
    B = 1 if labels.startswith("B1") else (2049 if labels == "late_positives" else 12)
    u, v, _ = H.online_case(B, 64, 7)
    y = {"all0": torch.zeros(B), "all1": torch.ones(B), "one_positive": (torch.arange(B) == 3).float(),
         "B1_pos": torch.ones(1), "B1_neg": torch.zeros(1), "half": torch.full((B,), 0.5),
         "late_positives": ((torch.arange(B) >= 1024) & (torch.arange(B) % 2 == 1)).float()}[labels]
    if labels == "half":
        y[:8] = torch.tensor([1.0, 0, 0, 1, 1, 0, 0, 1])      # eight rows take part, four are ignored
    xs = f64((u, v))
    ref = H.online_ref(*xs, y, H.COS_DIST, 0.5)
    ref.backward()
    out, grads = online_raw(u, v, y)
    if B == 1:
        # a single row: its own class's threshold is its own value (d > d is false), the other class's is the mean of an
        # empty set (NaN) -- nothing is selected, the loss is exactly 0 and so is every gradient
        assert ref.item() == 0.0 and out.item() == 0.0
        assert all((g == 0).all() for g in grads)
        return
    # one class only (all0 / all1): the other class's threshold is that class's own mean, so the rows on the hard side of
    # their mean are selected; one_positive: t_neg = mean(negs), t_pos = min(negs)
    d = H.metric_ref(u.double(), v.double(), H.COS_DIST)
    part = (y == 0) | (y == 1)
    pos_sel, neg_sel, t_pos, t_neg = H.online_selection(d, y)
    gaps = [(d[y == c] - t).abs().min().item() for c, t in ((1, t_pos), (0, t_neg)) if (y == c).any() and not torch.isnan(t)]
    assert min(gaps) >= 5 * H.value_tol(H.COS_DIST, 64), gaps
    assert int(pos_sel.sum()) + int(neg_sel.sum()) > 0
    if labels == "late_positives":
        assert not (y[:1024] == 1).any() and y[2048] == 0 and 0 < int(pos_sel.sum()) < int((y == 1).sum())
    torch.testing.assert_close(out, ref.detach(), rtol=1e-5, atol=1e-5)
    assert torch.equal(grads[0].abs().sum(1) != 0, pos_sel | (neg_sel & (d < 0.5)))
    assert (grads[0][~part] == 0).all() and (grads[1][~part] == 0).all()
    check_grads([g.float() for g in grads], xs)


# ------------------------------------------------------------------ 3. degenerate rows
@pytest.mark.parametrize("D", [64, 384, 2052])
@pytest.mark.parametrize("metric", sorted(H.METRIC_NAMES), ids=lambda m: H.METRIC_NAMES[m])
def test_zero_and_identical_rows(lib, D, metric):
    B = 6
    u, v = H.rows(B, D, 2, D)
    u[0] = 0; v[0] = 0            # both zero: cosine 0, L2 = 1e-6 * sqrt(D)
    u[1] = 0                      # one zero
    v[2] = u[2]; v[3] = u[3]      # identical rows
    xs = f64((u, v))
    ref = H.metric_ref(*xs, metric)
    ref.sum().backward()
    out, grads = S.pair_metric_raw(dev(u), dev(v), metric, want_grads=True)
    if metric in (H.COS_SIM, H.COS_DIST):
        assert out[0].item() == (0.0 if metric == H.COS_SIM else 1.0) and out[1].item() == out[0].item()
    if metric == H.L2:
        torch.testing.assert_close(out[0].item(), 1e-6 * D ** 0.5, rtol=1e-5, atol=0)
    tol = H.value_tol(metric, D)
    torch.testing.assert_close(out.cpu().double(), ref.detach(), rtol=tol, atol=tol)
    # torch's cosine gradients at a zero row are O(1 / eps): not compared there, only required to be finite
    zero = torch.tensor([True, True, False, False, False, False]) if metric in (H.COS_SIM, H.COS_DIST) else None
    check_grads(grads, xs, skip_rows=zero)
    if metric == H.L2_PLAIN:
        assert (grads[0][2:4] == 0).all() and (grads[1][2:4] == 0).all()


def test_losses_on_identical_rows(lib):
    a, p, n = H.rows(8, 384, 3, 5)
    p[:4] = a[:4]
    y = (torch.arange(8) % 2).float()
    for metric in H.DISTANCES:
        xs = f64((a, p, n))
        ref = H.triplet_ref(*xs, metric, 0.3, "mean")
        ref.backward()
        out, grads = S.triplet_loss_raw(dev(a), dev(p), dev(n), metric, 0.3, 2, want_grads=True)
        check_value(out, ref, metric, 8, 384, 2)
        check_grads(grads, xs)
        xs = f64((a, p))
        ref = H.contrastive_ref(*xs, y, metric, 0.5, "mean")
        ref.backward()
        out, grads = S.pair_loss_raw(dev(a), dev(p), dev(y), H.CONTRASTIVE, metric, 0.5, 2, want_grads=True)
        check_value(out, ref, metric, 8, 384, 2)
        check_grads(grads, xs)


# ------------------------------------------------------------------ 4. arguments, forward only, determinism
def test_bad_arguments_are_refused(lib):
    x = torch.randn(4, 8, device="cuda")
    y = torch.zeros(4, device="cuda")
    o = torch.zeros(4, device="cuda")
    s = torch.zeros(6, device="cuda")
    g = torch.full((4, 8), 7.0, device="cuda")
    X, Y, O, Sc, G, st = x.data_ptr(), y.data_ptr(), o.data_ptr(), s.data_ptr(), g.data_ptr(), stream()
    pm = lambda **k: lib.qst_pair_metric(*[k.get(n, d) for n, d in  # noqa: E731
                                           (("u", X), ("v", X), ("B", 4), ("D", 8), ("metric", 0), ("out", O), ("go", None),
                                            ("gu", None), ("gv", None), ("st", st))])
    pl = lambda **k: lib.qst_pair_loss(*[k.get(n, d) for n, d in  # noqa: E731
                                         (("u", X), ("v", X), ("y", Y), ("B", 4), ("D", 8), ("kind", 1), ("metric", 1),
                                          ("margin", 0.5), ("red", 2), ("out", O), ("go", None), ("gu", None), ("gv", None),
                                          ("sc", Sc), ("st", st))])
    tl = lambda **k: lib.qst_triplet_loss(*[k.get(n, d) for n, d in  # noqa: E731
                                            (("a", X), ("p", X), ("n", X), ("B", 4), ("D", 8), ("metric", 2), ("margin", 1.0),
                                             ("red", 2), ("out", O), ("go", None), ("ga", None), ("gp", None), ("gn", None),
                                             ("sc", Sc), ("st", st))])
    assert pm() == 0 and pl() == 0 and tl() == 0
    for fn in (pm, pl, tl):
        assert fn(B=0) == BAD_ARG and fn(B=-3) == BAD_ARG and fn(D=0) == BAD_ARG
        assert fn(out=None) == BAD_ARG
        assert fn(metric=7) == BAD_ARG and fn(metric=-1) == BAD_ARG
    assert pm(u=None) == BAD_ARG and pm(v=None) == BAD_ARG
    assert pl(u=None) == BAD_ARG and pl(v=None) == BAD_ARG and pl(y=None) == BAD_ARG
    assert tl(a=None) == BAD_ARG and tl(p=None) == BAD_ARG and tl(n=None) == BAD_ARG
    for fn in (pl, tl):
        assert fn(red=3) == BAD_ARG and fn(red=-1) == BAD_ARG
        assert fn(margin=-0.1) == BAD_ARG and fn(margin=float("nan")) == BAD_ARG
        assert fn(sc=None) == BAD_ARG and fn(sc=None, red=0) == 0
        assert fn(metric=H.COS_SIM) == BAD_ARG and fn(metric=H.DOT) == BAD_ARG and fn(metric=H.L2_PLAIN) == BAD_ARG
    assert pl(kind=3) == BAD_ARG and pl(kind=-1) == BAD_ARG
    assert pl(kind=H.MSE, metric=H.L2) == BAD_ARG and pl(kind=H.MSE, metric=H.COS_SIM) == 0
    assert pl(kind=H.ONLINE, sc=None, red=0) == BAD_ARG
    # some gradient pointers but not all: refused, and the buffer that was given is not written
    assert pm(gu=G) == BAD_ARG and pl(gv=G) == BAD_ARG and tl(ga=G, gp=G) == BAD_ARG
    torch.cuda.synchronize()
    assert (g == 7.0).all()


def test_forward_only_equals_the_value_of_a_gradient_call_and_writes_nothing_else(lib):
    B, D = 9, 96
    a, p, n = [dev(t) for t in H.rows(B, D, 3, 11)]
    y = dev((torch.arange(B) % 2).float())
    # [guard | out | guard]: a forward-only call writes its B (or 1) outputs and nothing around them
    for red, n_out in ((0, B), (2, 1)):
        for call in ("metric", "mse", "contrastive", "online", "triplet"):
            buf = torch.full((3, B), 7.0, device="cuda")
            o = buf[1]
            sc = torch.zeros(B + 2, device="cuda")
            if call == "metric":
                rc = lib.qst_pair_metric(ptr(a), ptr(p), B, D, H.L2, ptr(o), None, None, None, stream())
                full = S.pair_metric_raw(a, p, H.L2, want_grads=True)[0]
                n_o = B
            elif call == "triplet":
                rc = lib.qst_triplet_loss(ptr(a), ptr(p), ptr(n), B, D, H.L2, 1.0, red, ptr(o), None, None, None, None, ptr(sc),
                                          stream())
                full = S.triplet_loss_raw(a, p, n, H.L2, 1.0, red, want_grads=True)[0]
                n_o = n_out
            else:
                kind = {"mse": H.MSE, "contrastive": H.CONTRASTIVE, "online": H.ONLINE}[call]
                metric = H.COS_SIM if kind == H.MSE else H.COS_DIST
                rc = lib.qst_pair_loss(ptr(a), ptr(p), ptr(y), B, D, kind, metric, 0.5, red, ptr(o), None, None, None, ptr(sc),
                                       stream())
                full = S.pair_loss_raw(a, p, y, kind, metric, 0.5, red, want_grads=True)[0]
                n_o = 1 if kind == H.ONLINE else n_out
            assert rc == 0
            assert torch.equal(o[:n_o], full) and (buf[0] == 7.0).all() and (buf[2] == 7.0).all() and (o[n_o:] == 7.0).all()


def test_two_identical_calls_are_bit_identical(lib):
    for B, D in ((64, 384), (2000, 768), (5, 5120), (7, 33)):
        a, p, n = [dev(t) for t in H.rows(B, D, 3, 3)]
        y = dev((torch.arange(B) % 2).float())
        w = dev(torch.tensor([1.3]))
        calls = [lambda: S.pair_metric_raw(a, p, H.COS_SIM, grad_out=dev(upstream(B, 0)), want_grads=True),
                 lambda: S.pair_loss_raw(a, p, y, H.MSE, H.COS_SIM, 0.0, 2, grad_out=w, want_grads=True),
                 lambda: S.pair_loss_raw(a, p, y, H.CONTRASTIVE, H.L2, 0.5, 1, grad_out=w, want_grads=True),
                 lambda: S.pair_loss_raw(a, p, y, H.ONLINE, H.COS_DIST, 0.5, 1, grad_out=w, want_grads=True),
                 lambda: S.triplet_loss_raw(a, p, n, H.L1, 5.0, 2, grad_out=w, want_grads=True)]
        for call in calls:
            o1, g1 = call()
            o2, g2 = call()
            assert torch.equal(o1, o2) and all(torch.equal(x, z) for x, z in zip(g1, g2))


# ------------------------------------------------------------------ 5. the classes
WORDS = "a man rides red horse two dogs play in park woman eats green apple near old bridge small cat sleeps".split()


def sent(i, n):
    rng = np.random.RandomState(i)
    return " ".join(rng.choice(WORDS, size=n))


def pair_examples(n, graded):
    # every other pair shares most of its words; the 0 / 1 labels do not follow that, so that both classes hold near and far
    # pairs and OnlineContrastiveLoss has something to select
    rng = np.random.RandomState(3)
    return [InputExample(texts=[sent(i, 5 + i % 6), sent((i if i % 2 else 500 + i), 4 + i % 5) + " today"],
                         label=(float(rng.rand()) if graded else (i // 2) % 2)) for i in range(n)]


def triplet_examples(n):
    return [InputExample(texts=[sent(i, 9), sent(i, 9) + " now", sent(1000 + i, 5 + i % 7)]) for i in range(n)]


class TorchOpLoss(nn.Module):
    """The same objective with the loss written in torch ops on the embeddings (the yardstick functions, fp32 on the GPU):
    what a user had to write before the kernels existed. Shares the encoder pass rule with the class under test."""

    def __init__(self, model, fn):
        super().__init__()
        self.model, self.fn = model, fn

    def forward(self, feats, labels):
        from quadruplet_sentence_transformer_amd.sentence_transformer import encode_columns_fused
        return self.fn(*encode_columns_fused(self.model, list(feats)), labels.view(-1))


CLASS_CASES = {
    "cosine": (lambda m, **k: S.CosineSimilarityLoss(m, **k), lambda u, v, y: H.mse_ref(u, v, y), True, H.COS_SIM),
    "contrastive": (lambda m, **k: S.ContrastiveLoss(m, **k), lambda u, v, y: H.contrastive_ref(u, v, y, H.COS_DIST, 0.5),
                    False, H.COS_DIST),
    "online": (lambda m, **k: S.OnlineContrastiveLoss(m, **k), lambda u, v, y: H.online_ref(u, v, y, H.COS_DIST, 0.5), False,
               H.COS_DIST),
    "triplet": (lambda m, **k: S.TripletLoss(m, **k), lambda a, p, n, y: H.triplet_ref(a, p, n, H.L2, 5.0), None, H.L2),
}

# Relative L2 difference of the gradient arena, per parameter tensor, between a class and the torch-op path on the same
# model (the bf16 backward re-rounds activations that depend on grad_emb, so no bound can be derived in advance): measured
# on an MI355X over the four classes and asserted at x 1.25 (README "Parity").
#   every tensor:             cosine 1.605e-2, contrastive 1.425e-2, online 1.598e-2, triplet 4.037e-3
#   all but the key biases:   cosine 6.753e-5, contrastive 6.061e-5, online 8.661e-5, triplet 1.884e-5
# The maxima over every tensor sit at attention.self.key.bias. Its exact gradient is zero (a softmax does not move when
# every score of a row shifts by q . b_k), so what the arena holds there is the backward's rounding residue, |g| = 1e-8 ...
# 4e-7 next to 1e-2 for the weights: the figure compares two residues. Both maxima are asserted; two runs of the torch-op
# path itself differ by 3e-7 at most.
GRAD_REL_MEASURED = 1.605e-2
GRAD_REL_MEASURED_NO_KEY_BIAS = 8.661e-5
GRAD_REL_SANITY = 1.65e-2           # the bf16 path's bound against the oracle: at or above it is a bug, not rounding
# the custom loss_fct / transformation path (qst_pair_metric + torch): whole arena, and per tensor but the key biases
CUSTOM_REL_ARENA_MEASURED = 7.387e-6
CUSTOM_REL_MEASURED_NO_KEY_BIAS = 3.945e-4


def grad_rel(gh, gt):
    """(max over every tensor, max over all but the key biases, whole arena, name of the worst tensor)."""
    rel = {k: ((gh[k] - gt[k]).norm() / gt[k].norm()).item() for k in gt if gt[k].norm().item() > 0}
    worst = max(rel, key=rel.get)
    arena = (torch.cat([(gh[k] - gt[k]).reshape(-1) for k in gt]).norm() / torch.cat([gt[k].reshape(-1) for k in gt]).norm()).item()
    return rel[worst], max(v for k, v in rel.items() if "key.bias" not in k), arena, worst


@pytest.fixture(scope="module")
def model():
    return SentenceTransformer("tiny-bert", device="cuda")


def one_backward(model, lm, feats, labels):
    enc = model._enc
    enc.ensure_train_state()
    enc.grads.zero_()
    loss = lm([dict(f) for f in feats], labels)
    loss.backward()
    g = {k: v.clone() for k, v in enc.grad_views().items()}
    enc.grads.zero_()
    return loss.detach(), g


def class_batch(model, name):
    graded = CLASS_CASES[name][2]
    batch = triplet_examples(16) if graded is None else pair_examples(16, graded)
    feats, labels = model.smart_batching_collate(batch)
    return [{k: v.cuda() for k, v in f.items()} for f in feats], labels.cuda()


@pytest.mark.parametrize("name", sorted(CLASS_CASES))
def test_class_fused_pass_equals_one_pass_per_column(model, name):
    make = CLASS_CASES[name][0]
    feats, labels = class_batch(model, name)
    model.train()
    lk, gk = one_backward(model, make(model, fused=False), feats, labels)
    l1, g1 = one_backward(model, make(model, fused=True), feats, labels)
    flat = lambda g: torch.cat([t.reshape(-1) for t in g.values()])  # noqa: E731
    assert abs(lk.item() - l1.item()) < 2e-4
    assert (flat(gk) - flat(g1)).norm().item() <= 2e-2 * flat(g1).norm().item()


@pytest.mark.parametrize("name", sorted(CLASS_CASES))
def test_class_equals_torch_ops_on_the_same_model(model, name):
    make, fn, _, metric = CLASS_CASES[name]
    feats, labels = class_batch(model, name)
    model.train()
    lt, gt = one_backward(model, TorchOpLoss(model, fn), feats, labels)
    lh, gh = one_backward(model, make(model), feats, labels)
    assert lt.item() != 0.0
    tol = H.value_tol(metric, model.get_sentence_embedding_dimension())
    print(f"  {name}: loss hip {lh.item():.7f} torch ops {lt.item():.7f}")
    torch.testing.assert_close(lh, lt, rtol=tol, atol=tol * (16 if name == "online" else 1))
    every, no_kb, arena, worst = grad_rel(gh, gt)
    print(f"  {name}: gradient arena, relative L2 difference per tensor: max {every:.3e} at {worst}; without the key biases "
          f"{no_kb:.3e}; whole arena {arena:.3e}")
    assert every < GRAD_REL_SANITY
    assert every <= 1.25 * GRAD_REL_MEASURED and no_kb <= 1.25 * GRAD_REL_MEASURED_NO_KEY_BIAS


def test_custom_loss_fct_and_score_transformation_equal_torch(model):
    feats, labels = class_batch(model, "cosine")
    model.train()
    lm = S.CosineSimilarityLoss(model, loss_fct=nn.L1Loss(), cos_score_transformation=nn.Sigmoid())
    ref = TorchOpLoss(model, lambda u, v, y: nn.functional.l1_loss(torch.sigmoid(nn.functional.cosine_similarity(u, v)), y))
    lt, gt = one_backward(model, ref, feats, labels)
    lh, gh = one_backward(model, lm, feats, labels)
    torch.testing.assert_close(lh, lt, rtol=1e-5, atol=1e-5)
    every, no_kb, arena, worst = grad_rel(gh, gt)
    print(f"  custom loss_fct: gradient arena relative L2 difference: whole arena {arena:.3e}; per tensor without the key biases "
          f"{no_kb:.3e}; max {every:.3e} at {worst}")
    assert arena <= 1.25 * CUSTOM_REL_ARENA_MEASURED and no_kb <= 1.25 * CUSTOM_REL_MEASURED_NO_KEY_BIAS
    # and on the embeddings themselves, at the kernels' gradient tolerance
    g = torch.Generator().manual_seed(4)
    u, v = [nn.functional.normalize(torch.randn(16, 64, generator=g), dim=1).cuda().requires_grad_(True) for _ in range(2)]
    y = torch.rand(16, generator=g).cuda()
    nn.functional.l1_loss(torch.sigmoid(nn.functional.cosine_similarity(u, v)), y).backward()
    ref_g = [u.grad.clone(), v.grad.clone()]
    u.grad = v.grad = None
    nn.functional.l1_loss(torch.sigmoid(S.pair_metric(u, v, S.METRIC_COS_SIM)), y).backward()
    for got, ref in zip((u.grad, v.grad), ref_g):
        torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-6)
    # MSELoss with another reduction stays on the fused kernel
    lsum = S.CosineSimilarityLoss(model, loss_fct=nn.MSELoss(reduction="sum"))([dict(f) for f in feats], labels)
    lmean = S.CosineSimilarityLoss(model)([dict(f) for f in feats], labels)
    torch.testing.assert_close(lsum, lmean * 16, rtol=1e-5, atol=1e-6)
    model._enc.grads.zero_()


def test_a_callable_distance_metric_runs_in_torch(model):
    """A metric that is not a member of the metric classes is called on the embeddings as given."""
    feats, labels = class_batch(model, "triplet")
    model.train()
    seen = []

    def sq_l2(x, y):
        seen.append(x.shape)
        return (x - y).pow(2).sum(1)

    with torch.no_grad():
        got = S.TripletLoss(model, distance_metric=sq_l2, triplet_margin=0.1)([dict(f) for f in feats], labels)
        a, p, n = [model(dict(f))["sentence_embedding"] for f in feats]
        ref = torch.relu(sq_l2(a, p) - sq_l2(a, n) + 0.1).mean()
        member = S.TripletLoss(model, distance_metric=S.TripletDistanceMetric.EUCLIDEAN, triplet_margin=0.1)(
            [dict(f) for f in feats], labels)
        direct = torch.relu(S.TripletDistanceMetric.EUCLIDEAN(a, p) - S.TripletDistanceMetric.EUCLIDEAN(a, n) + 0.1).mean()
    assert len(seen) == 4
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=2e-4)
    torch.testing.assert_close(member, direct, rtol=1e-4, atol=2e-4)


class RecordLoss(nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner, self.seen = inner, []

    def forward(self, feats, labels):
        loss = self.inner(feats, labels)
        self.seen.append(loss.detach())
        return loss


@pytest.mark.parametrize("use_amp", [False, True])
@pytest.mark.parametrize("name", ["cosine", "triplet"])
def test_fit_lowers_the_training_loss(name, use_amp):
    m = SentenceTransformer("tiny-bert", device="cuda")          # a fresh model: amp schedule counters persist per model
    if name == "cosine":
        # graded pairs whose score says whether the two sentences are the same
        data = [InputExample(texts=[sent(i, 8), sent(i, 8) + " today" if i % 2 else sent(2000 + i, 8)], label=float(i % 2))
                for i in range(64)]
        lm = RecordLoss(S.CosineSimilarityLoss(m))
    else:
        data = triplet_examples(64)
        lm = RecordLoss(S.TripletLoss(m, distance_metric=S.TripletDistanceMetric.COSINE, triplet_margin=0.5))
    dl = DataLoader(data, batch_size=16, shuffle=False)
    m.fit([(dl, lm)], epochs=5, warmup_steps=0, scheduler="constantlr", optimizer_params={"lr": 1e-3}, dropout=0,
          use_amp=use_amp, show_progress_bar=False)
    seen = torch.stack(lm.seen).cpu()
    assert len(seen) == 20
    print(f"  fit {name} amp={use_amp}: first 5 {seen[:5].mean().item():.5f} last 5 {seen[-5:].mean().item():.5f}")
    assert torch.isfinite(seen).all() and seen[-5:].mean() < seen[:5].mean()
    assert torch.isfinite(m._enc.params).all()


# ------------------------------------------------------------------ 6. the evaluator
def test_embedding_similarity_evaluator(model, tmp_path):
    s1 = [sent(i, 4 + i % 7) for i in range(50)]
    s2 = [sent(i if i % 3 else 700 + i, 5 + i % 5) + " now" for i in range(50)]
    gold = np.random.RandomState(0).rand(50).tolist()
    ev = EmbeddingSimilarityEvaluator(s1, s2, gold, batch_size=16, name="dev")
    model.eval()
    got = ev.pair_scores(model)
    e1 = np.asarray(model.encode(s1, batch_size=16), dtype=np.float64)
    e2 = np.asarray(model.encode(s2, batch_size=16), dtype=np.float64)
    ref = {"cosine": (e1 * e2).sum(1) / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)),
           "euclidean": -np.linalg.norm(e1 - e2, axis=1), "manhattan": -np.abs(e1 - e2).sum(1), "dot": (e1 * e2).sum(1)}
    main = ev(model, output_path=str(tmp_path), epoch=2, steps=30)
    with open(tmp_path / "similarity_evaluation_dev_results.csv") as f:
        table = list(csv.reader(f))
    assert table[0] == ["epoch", "steps", "cosine_pearson", "cosine_spearman", "euclidean_pearson", "euclidean_spearman",
                        "manhattan_pearson", "manhattan_spearman", "dot_pearson", "dot_spearman"]
    assert len(table) == 2 and table[1][:2] == ["2", "30"]
    row = [float(x) for x in table[1][2:]]
    spearmans = []
    for i, key in enumerate(("cosine", "euclidean", "manhattan", "dot")):
        np.testing.assert_allclose(got[key], ref[key], rtol=0, atol=1e-5)
        srt = np.sort(ref[key])
        assert np.diff(srt).min() > 1e-5, "two yardstick scores closer than the fp32 floor: change the test sentences"
        assert np.array_equal(H.rank_avg(got[key]), H.rank_avg(ref[key]))
        p, s = H.pearson_np(gold, ref[key]), H.spearman_np(gold, ref[key])
        print(f"  {key}: pearson {row[2 * i]:.7f} ({p:.7f}) spearman {row[2 * i + 1]:.7f} ({s:.7f})")
        assert abs(row[2 * i] - p) <= 1e-5 and abs(row[2 * i + 1] - s) <= 1e-5
        spearmans.append(s)
    assert abs(main - max(spearmans)) <= 1e-5
    for fn, idx in ((SimilarityFunction.COSINE, 0), (SimilarityFunction.EUCLIDEAN, 1), (SimilarityFunction.MANHATTAN, 2),
                    (SimilarityFunction.DOT_PRODUCT, 3)):
        one = EmbeddingSimilarityEvaluator(s1, s2, gold, main_similarity=fn, write_csv=False)(model, output_path=str(tmp_path))
        assert abs(one - spearmans[idx]) <= 1e-5
    assert sorted(os.listdir(tmp_path)) == ["similarity_evaluation_dev_results.csv"]
    ex = [InputExample(texts=[a, b], label=g) for a, b, g in zip(s1, s2, gold)]
    ev2 = EmbeddingSimilarityEvaluator.from_input_examples(ex, name="dev", batch_size=16)
    assert ev2.sentences1 == s1 and ev2.sentences2 == s2 and ev2.scores == gold and ev2.csv_file == ev.csv_file
    assert abs(ev2(model) - main) <= 1e-6
    # a second call appends a row under the same header
    ev(model, output_path=str(tmp_path), epoch=3, steps=-1)
    with open(tmp_path / "similarity_evaluation_dev_results.csv") as f:
        assert len(list(csv.reader(f))) == 3


def test_spearman_second_opinion():
    stats = pytest.importorskip("scipy.stats")
    from quadruplet_sentence_transformer_amd.evaluation import pearson, spearman
    r = np.random.RandomState(1)
    x, y = r.randint(0, 6, 40).astype(float), r.randn(40)
    assert abs(spearman(x, y) - stats.spearmanr(x, y)[0]) < 1e-12 and abs(H.spearman_np(x, y) - stats.spearmanr(x, y)[0]) < 1e-12
    assert abs(pearson(x, y) - stats.pearsonr(x, y)[0]) < 1e-12
