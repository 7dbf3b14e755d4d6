"""CPU: the host side of the batch-mining triplet losses -- the yardstick itself (its two formulations against each other,
the seed search), SentenceLabelDataset, constructor surface, drop-in namespaces, the refusal of CPU tensors and bad
arguments, and the argument checks of qst_batch_triplet_loss (made before any launch, so they hold without a device). No
kernel runs here."""
import ctypes as C
import inspect
import math
import os
import random
import sys

import numpy as np
import pytest
import torch
from torch import nn
from torch.utils.data import DataLoader, IterableDataset

import quadruplet_sentence_transformer_amd  # noqa: F401
import batch_triplet_helpers as T
from quadruplet_sentence_transformer_amd import _lib, data, st_losses as S
from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = (S.BatchHardTripletLoss, S.BatchHardSoftMarginTripletLoss, S.BatchSemiHardTripletLoss, S.BatchAllTripletLoss)
DF = S.BatchHardTripletLossDistanceFunction


# ------------------------------------------------------------------ the yardstick
def both_formulations(x, labels, kind, metric):
    m = T.MARGIN[metric]
    a = x.double().clone().requires_grad_(True)
    b = x.double().clone().requires_grad_(True)
    la, ca = T.loss_tensor(a, labels, kind, metric, m)
    lb, cb, _ = T.loss_loops(b, labels, kind, metric, m)
    assert tuple(ca) == tuple(cb)
    if math.isnan(la.item()) or math.isnan(lb.item()):
        assert math.isnan(la.item()) and math.isnan(lb.item())
        return
    assert abs(la.item() - lb.item()) <= 1e-12 * max(1.0, abs(la.item()))
    la.backward()
    if lb.requires_grad:
        lb.backward()
    ga = a.grad
    gb = b.grad if b.grad is not None else torch.zeros_like(b)
    assert (ga - gb).abs().max().item() <= 1e-12 * max(1.0, ga.abs().max().item())


@pytest.mark.parametrize("metric", T.METRICS, ids=[T.METRIC_NAMES[m] for m in T.METRICS])
@pytest.mark.parametrize("kind", T.KINDS, ids=[T.KIND_NAMES[k] for k in T.KINDS])
def test_seed_search_succeeds_and_the_two_formulations_agree(kind, metric):
    """Every shape finds a tie-free seed whose reference is not vacuous (reference() asserts both), and on it the tensor
    formulation and the loops give the same loss, counts and gradient in fp64."""
    for (B, D) in T.shapes_of(kind):
        x, labels, loss, grad, counts, k = T.reference(B, D, kind, metric)
        assert T.fragility(x, labels, kind, metric) >= T.MIN_FRAGILITY and 0 <= k < T.SEED_TRIES
        assert x.dtype == torch.float32 and labels.dtype == torch.int64 and torch.isfinite(grad).all()
        both_formulations(x, labels, kind, metric)


@pytest.mark.parametrize("metric", T.METRICS, ids=[T.METRIC_NAMES[m] for m in T.METRICS])
@pytest.mark.parametrize("kind", T.KINDS, ids=[T.KIND_NAMES[k] for k in T.KINDS])
def test_edge_batches_in_both_formulations(kind, metric):
    m = T.MARGIN[metric]
    for name, (x, labels) in T.edge_cases().items():
        both_formulations(x, labels, kind, metric)
        loss, counts = T.loss_tensor(x.double(), labels, kind, metric, m)
        if name == "all_distinct":
            if kind == T.ALL:
                assert loss.item() == 0.0 and counts == (0, 0)
            if kind == T.SEMI:
                assert math.isnan(loss.item()) and counts == (0, 0)
        if name == "all_equal":
            if kind == T.ALL:
                assert loss.item() == 0.0 and counts == (0, 0)
            if kind == T.HARD:                          # hp = rowmax, hn = d_ii + rowmax
                assert abs(loss.item() - m) < 1e-6
            if kind == T.SEMI:                          # the diagonal rule: every pair pays d_ij + m (euclid: d_ii = 0)
                d = T.dist_ref(x.double(), metric)
                off = ~torch.eye(8, dtype=torch.bool)
                assert abs(loss.item() - (d[off] + m).mean().item()) < 1e-6 and counts == (56, 56)
        if name == "duplicate_rows" and metric == T.EUCLID:
            d = T.dist_ref(x.double(), metric)
            j = int((x == x[0]).all(1).nonzero()[1])
            assert d[0, j].item() == 0.0
            _, grad, _ = T.reference_of(x, labels, kind, metric)
            assert torch.isfinite(loss) and torch.isfinite(grad).all()


def test_recipe_draws_clustered_rows_with_lengths_of_their_own():
    x, labels = T.case(33, 768, T.seed_of(33, 768, 0))
    assert labels.unique().numel() == 8 and torch.bincount(labels).min().item() >= 4
    n = x.norm(dim=1)
    assert n.min().item() >= 0.5 - 1e-6 and n.max().item() <= 2.0 + 1e-6 and n.std().item() > 0.1


# ------------------------------------------------------------------ SentenceLabelDataset
def labelled(counts):
    return [InputExample(texts=[f"text {lab} {i}"], label=lab) for lab, n in counts.items() for i in range(n)]


@pytest.mark.parametrize("spl", [2, 3])
def test_sentence_label_dataset_yields_runs_of_one_label(spl):
    np.random.seed(3)
    random.seed(3)
    ex = labelled({0: 6, 1: 6, 2: 1, 3: 12, 4: spl - 1, 5: 6})
    ds = data.SentenceLabelDataset(ex, samples_per_label=spl)
    assert isinstance(ds, IterableDataset)
    kept = 6 + 6 + 12 + 6                                 # labels 2 and 4 are too rare
    assert len(ds) == kept
    out = list(ds)
    assert len(out) == kept and all(e.label in (0, 1, 3, 5) for e in out)
    for r in range(0, kept, spl):
        assert len({e.label for e in out[r:r + spl]}) == 1
    # within the first lap over the labels nothing repeats (each label gives one run per lap)
    first_lap = out[:4 * spl]
    assert len({e.texts[0] for e in first_lap}) == len(first_lap) and len({e.label for e in first_lap}) == 4


def test_sentence_label_dataset_is_deterministic_under_a_seed_and_feeds_a_dataloader():
    ex = labelled({7: 4, 8: 4, 9: 4, 10: 3})

    def run():
        np.random.seed(11)
        random.seed(11)
        ds = data.SentenceLabelDataset(list(ex), samples_per_label=2)
        return [e.texts[0] for e in ds], ds

    a, ds = run()
    b, _ = run()
    assert a == b and len(a) == 16                      # 15 kept examples go out as 8 whole runs
    assert len(ds) == 15
    np.random.seed(12)
    assert [e.texts[0] for e in ds] != a                # another seed, another order
    dl = DataLoader(ds, batch_size=4)
    dl.collate_fn = lambda batch: [e.label for e in batch]      # what fit() sets
    assert len(dl) == 4
    for labels in dl:
        assert len(labels) == 4 and labels[0] == labels[1] and labels[2] == labels[3]
    with_repl = data.SentenceLabelDataset(labelled({0: 2, 1: 2}), samples_per_label=2, with_replacement=True)
    assert len(list(with_repl)) == 4
    assert len(data.SentenceLabelDataset(labelled({0: 1, 1: 1}))) == 0 and list(data.SentenceLabelDataset(labelled({0: 1}))) == []


# ------------------------------------------------------------------ the classes
def defaults(cls):
    return {k: p.default for k, p in inspect.signature(cls.__init__).parameters.items() if k not in ("self", "model")}


def test_constructor_defaults_follow_sentence_transformers():
    for cls in CLASSES:
        want = {"distance_metric": DF.eucledian_distance, "margin": 5, "fused": True}
        if cls is S.BatchHardSoftMarginTripletLoss:
            del want["margin"]
        assert defaults(cls) == want
        assert list(inspect.signature(cls.forward).parameters)[:3] == ["self", "sentence_features", "labels"]
        assert issubclass(cls, S._TupleLoss) and cls.reduction == "mean"
    for cls, helper in zip(CLASSES, ("batch_hard_triplet_loss", "batch_hard_triplet_soft_margin_loss",
                                     "batch_semi_hard_triplet_loss", "batch_all_triplet_loss")):
        assert list(inspect.signature(getattr(cls, helper)).parameters) == ["self", "labels", "embeddings"]
    assert DF.eucledian_distance._qst_metric == S.METRIC_L2_PLAIN == T.EUCLID
    assert DF.cosine_distance._qst_metric == S.METRIC_COS_DIST == T.COS
    assert (S.BT_HARD, S.BT_HARD_SOFT, S.BT_SEMIHARD, S.BT_ALL) == (T.HARD, T.SOFT, T.SEMI, T.ALL) == (0, 1, 2, 3)


def test_distance_functions_are_callable_on_their_own():
    x, _ = T.case(5, 10, 5010)
    x = x.double()
    for metric, fn in ((T.EUCLID, DF.eucledian_distance), (T.COS, DF.cosine_distance)):
        assert torch.allclose(fn(x), T.dist_ref(x, metric), rtol=0, atol=1e-12)
    assert torch.allclose(DF.eucledian_distance(x, squared=True), T.dist_ref(x, T.EUCLID) ** 2, rtol=0, atol=1e-12)


def test_an_untagged_callable_mines_in_torch_like_the_yardstick():
    """The torch route of the classes (any other distance_metric) is the reference's formula: on the CPU, in fp64."""
    x, labels = T.case(8, 32, 8032)
    x = x.double()
    for cls, kind in zip(CLASSES, T.KINDS):
        for metric, fn in ((T.EUCLID, DF.eucledian_distance), (T.COS, DF.cosine_distance)):
            kw = {} if kind == T.SOFT else {"margin": T.MARGIN[metric]}
            lm = cls(nn.Identity(), distance_metric=lambda e, fn=fn: fn(e), **kw)
            got = lm._loss(labels, x)
            want, _ = T.loss_tensor(x, labels, kind, metric, T.MARGIN[metric])
            assert abs(got.item() - want.item()) < 1e-12


def test_cpu_tensors_and_bad_arguments_are_refused():
    x, labels = T.case(8, 32, 8032)
    for kind in T.KINDS:
        with pytest.raises(_lib.QstError):
            S.batch_triplet_loss(x, labels, kind, T.EUCLID, 0.1)
    with pytest.raises(ValueError):
        S.batch_triplet_loss(x, labels, S.BT_HARD, T.EUCLID, -0.1)
    with pytest.raises(ValueError):
        S.batch_triplet_loss(x, labels, S.BT_HARD, T.EUCLID, float("nan"))
    with pytest.raises(ValueError):
        S.batch_triplet_loss(x, labels[:7], S.BT_HARD, T.EUCLID, 0.1)
    with pytest.raises(ValueError):
        S.batch_triplet_loss(x[0], labels, S.BT_HARD, T.EUCLID, 0.1)
    with pytest.raises(ValueError):
        S.batch_triplet_loss(x, labels.float(), S.BT_HARD, T.EUCLID, 0.1)
    with pytest.raises(ValueError):
        S.batch_triplet_loss(x, labels, 4, T.EUCLID, 0.1)
    with pytest.raises(ValueError):
        S.batch_triplet_loss(x, labels, S.BT_HARD, S.METRIC_L2, 0.1)
    ids = {"input_ids": torch.zeros(2, 3, dtype=torch.long)}
    for cls in CLASSES:
        with pytest.raises(ValueError):
            cls(nn.Identity())([ids, ids], torch.zeros(2, dtype=torch.long))       # two text columns


def test_dropin_namespaces_export_the_new_names():
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    stale = lambda: [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]  # noqa: E731
    for m in stale():
        del sys.modules[m]
    try:
        from sentence_transformers import datasets, losses
        for name in ("BatchHardTripletLoss", "BatchHardSoftMarginTripletLoss", "BatchSemiHardTripletLoss",
                     "BatchAllTripletLoss", "BatchHardTripletLossDistanceFunction"):
            assert getattr(losses, name) is getattr(S, name)
        assert datasets.SentenceLabelDataset is data.SentenceLabelDataset
        assert datasets.NoDuplicatesDataLoader is data.NoDuplicatesDataLoader and losses.TripletLoss is S.TripletLoss
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
        for m in stale():
            del sys.modules[m]


# ------------------------------------------------------------------ the library, without a device
def test_library_version_and_new_symbols():
    lib = _lib.load()
    assert lib.qst_version() >= 106
    for name, nargs in (("qst_batch_triplet_workspace_bytes", 2), ("qst_batch_triplet_loss", 14)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.SIGNATURES["qst_batch_triplet_workspace_bytes"][0] is C.c_size_t
    sizes = [lib.qst_batch_triplet_workspace_bytes(B, 64) for B in range(1, 300)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    assert lib.qst_batch_triplet_workspace_bytes(130, 64) >= 130 * 132 * 4          # at least d [B, ldB]
    assert lib.qst_batch_triplet_workspace_bytes(0, 8) == 0 and lib.qst_batch_triplet_workspace_bytes(8, 0) == 0


def test_bad_arguments_are_refused_without_a_device():
    """Every QST_ERR_BAD_ARG of qst_batch_triplet_loss comes back before anything is launched: host memory stands in for
    the device pointers, and must be left as it was."""
    lib = _lib.load()
    B, D = 6, 8
    nbytes = lib.qst_batch_triplet_workspace_bytes(B, D)
    assert nbytes > 0
    x, g = (C.c_float * (B * D))(), (C.c_float * (B * D))()
    labels = (C.c_int64 * B)()
    out = (C.c_float * 1)(7.0)
    counts = (C.c_int64 * 2)(-5, -5)
    raw = (C.c_char * (nbytes + 32))()
    base = (C.addressof(raw) + 15) & ~15                    # a 16-byte aligned workspace inside the buffer
    for i in range(len(g)):
        g[i] = -3.0

    def call(x=x, labels=labels, B=B, D=D, kind=S.BT_HARD, metric=T.EUCLID, margin=0.1, out=out, ws=base, nb=nbytes):
        p = lambda v: None if v is None else C.cast(v, C.c_void_p)  # noqa: E731
        return lib.qst_batch_triplet_loss(p(x), p(labels), B, D, kind, metric, margin, p(out), p(counts), None, p(g),
                                          ws, nb, None)

    bad = [dict(B=0), dict(B=-1), dict(D=0), dict(x=None), dict(labels=None), dict(out=None), dict(ws=None),
           dict(nb=nbytes - 1), dict(nb=0), dict(ws=base + 4), dict(ws=base + 8), dict(kind=4), dict(kind=-1),
           dict(metric=S.METRIC_L2), dict(metric=S.METRIC_COS_SIM), dict(metric=7), dict(margin=-0.5),
           dict(margin=float("inf")), dict(margin=float("nan"))]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert out[0] == 7.0 and list(counts) == [-5, -5] and all(v == -3.0 for v in g)
    assert all(b == b"\x00" for b in raw)
