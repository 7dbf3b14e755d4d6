"""CPU: the host side of the pair / triplet losses and of EmbeddingSimilarityEvaluator -- constructor surface, drop-in
namespaces, the refusal of CPU tensors, the rank correlation, and the library's exports. No kernel runs here."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch
from torch import nn

import quadruplet_sentence_transformer_amd  # noqa: F401
import tuple_loss_helpers as H
from quadruplet_sentence_transformer_amd import _lib, evaluation, st_losses as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def defaults(cls):
    return {k: p.default for k, p in inspect.signature(cls.__init__).parameters.items() if k not in ("self", "model")}


def test_constructor_defaults_follow_sentence_transformers():
    d = defaults(S.CosineSimilarityLoss)
    assert list(d) == ["loss_fct", "cos_score_transformation", "fused"]
    assert type(d["loss_fct"]) is nn.MSELoss and d["loss_fct"].reduction == "mean"
    assert type(d["cos_score_transformation"]) is nn.Identity and d["fused"] is True
    assert defaults(S.ContrastiveLoss) == {"distance_metric": S.SiameseDistanceMetric.COSINE_DISTANCE, "margin": 0.5,
                                           "size_average": True, "fused": True}
    assert defaults(S.OnlineContrastiveLoss) == {"distance_metric": S.SiameseDistanceMetric.COSINE_DISTANCE, "margin": 0.5,
                                                 "fused": True}
    assert defaults(S.TripletLoss) == {"distance_metric": S.TripletDistanceMetric.EUCLIDEAN, "triplet_margin": 5,
                                       "fused": True}
    for cls in (S.CosineSimilarityLoss, S.ContrastiveLoss, S.OnlineContrastiveLoss, S.TripletLoss):
        assert list(inspect.signature(cls.forward).parameters)[:3] == ["self", "sentence_features", "labels"]
    d = defaults(evaluation.EmbeddingSimilarityEvaluator)
    assert d == {"sentences1": inspect.Parameter.empty, "sentences2": inspect.Parameter.empty,
                 "scores": inspect.Parameter.empty, "batch_size": 16, "main_similarity": None, "name": "",
                 "show_progress_bar": False, "write_csv": True}


def test_metric_members_map_to_the_kernel_codes():
    members = lambda cls: {k: getattr(cls, k)._qst_metric for k in vars(cls) if not k.startswith("_")}  # noqa: E731
    assert members(S.SiameseDistanceMetric) == {"EUCLIDEAN": H.L2, "MANHATTAN": H.L1, "COSINE_DISTANCE": H.COS_DIST}
    assert members(S.TripletDistanceMetric) == {"COSINE": H.COS_DIST, "EUCLIDEAN": H.L2, "MANHATTAN": H.L1}
    # the Python codes are the header's
    src = open(os.path.join(ROOT, "include", "qst.h")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"(QST_(?:METRIC|PAIR)_[A-Z0-9_]+) = (\d+)", src))
    assert enum == {"QST_METRIC_COS_SIM": S.METRIC_COS_SIM, "QST_METRIC_COS_DIST": S.METRIC_COS_DIST,
                    "QST_METRIC_L2": S.METRIC_L2, "QST_METRIC_L1": S.METRIC_L1, "QST_METRIC_DOT": S.METRIC_DOT,
                    "QST_METRIC_L2_PLAIN": S.METRIC_L2_PLAIN, "QST_METRIC_L1_PLAIN": S.METRIC_L1_PLAIN,
                    "QST_PAIR_MSE": S.PAIR_MSE, "QST_PAIR_CONTRASTIVE": S.PAIR_CONTRASTIVE,
                    "QST_PAIR_ONLINE_CONTRASTIVE": S.PAIR_ONLINE_CONTRASTIVE}
    assert (H.COS_SIM, H.COS_DIST, H.L2, H.L1, H.DOT, H.L2_PLAIN, H.L1_PLAIN) == tuple(range(7))
    lm = S.ContrastiveLoss(nn.Identity(), distance_metric=S.SiameseDistanceMetric.MANHATTAN, size_average=False)
    assert lm.get_config_dict() == {"distance_metric": "SiameseDistanceMetric.MANHATTAN", "margin": 0.5, "size_average": False}
    assert lm.reduction == "sum" and S.ContrastiveLoss(nn.Identity()).reduction == "mean"
    assert S.OnlineContrastiveLoss(nn.Identity()).reduction == "sum" and S.TripletLoss(nn.Identity()).reduction == "mean"
    assert S.CosineSimilarityLoss(nn.Identity(), loss_fct=nn.MSELoss(reduction="sum")).reduction == "sum"


def test_dropin_losses_and_evaluator_resolve_to_this_build():
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]
        from sentence_transformers import losses
        from sentence_transformers.evaluation import EmbeddingSimilarityEvaluator
        from sentence_transformers.losses import (ContrastiveLoss, CosineSimilarityLoss, OnlineContrastiveLoss,
                                                  SiameseDistanceMetric, TripletDistanceMetric, TripletLoss)
        assert losses.CosineSimilarityLoss is CosineSimilarityLoss is S.CosineSimilarityLoss
        assert ContrastiveLoss is S.ContrastiveLoss and OnlineContrastiveLoss is S.OnlineContrastiveLoss
        assert TripletLoss is S.TripletLoss and SiameseDistanceMetric is S.SiameseDistanceMetric
        assert TripletDistanceMetric is S.TripletDistanceMetric
        assert EmbeddingSimilarityEvaluator is evaluation.EmbeddingSimilarityEvaluator
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
        for m in [k for k in sys.modules if k == "sentence_transformers" or k.startswith("sentence_transformers.")]:
            del sys.modules[m]


def test_cpu_tensors_are_refused():
    u, v, w = torch.randn(3, 4, 8).unbind(0)
    y = torch.zeros(4)
    with pytest.raises(_lib.QstError):
        S.pair_metric(u, v, S.METRIC_COS_SIM)
    with pytest.raises(_lib.QstError):
        S.pair_loss(u, v, y, S.PAIR_MSE, S.METRIC_COS_SIM)
    with pytest.raises(_lib.QstError):
        S.pair_loss(u, v, y, S.PAIR_ONLINE_CONTRASTIVE, S.METRIC_COS_DIST)
    with pytest.raises(_lib.QstError):
        S.triplet_loss(u, v, w)
    with pytest.raises(_lib.QstError):
        S.SiameseDistanceMetric.EUCLIDEAN(u, v)
    with pytest.raises(ValueError):
        S.triplet_loss(u, v, w[:2])
    with pytest.raises(ValueError):
        S.triplet_loss(u, v, w, margin=-1.0)


def test_spearman_with_ties_by_hand():
    # x = 10 20 20 30 has ranks 1 2.5 2.5 4; y = 1 3 2 3 has ranks 1 3.5 2 3.5. Centred: (-1.5 0 0 1.5) and (-1.5 1 -0.5 1):
    # covariance sum 2.25 + 0 + 0 + 1.5 = 3.75, squared sums 4.5 and 4.5 -> rho = 3.75 / 4.5 = 5 / 6
    x, y = [10, 20, 20, 30], [1, 3, 2, 3]
    np.testing.assert_array_equal(evaluation.average_ranks(x), [1, 2.5, 2.5, 4])
    np.testing.assert_array_equal(evaluation.average_ranks(y), [1, 3.5, 2, 3.5])
    assert abs(evaluation.spearman(x, y) - 5.0 / 6.0) < 1e-15
    assert abs(H.spearman_np(x, y) - 5.0 / 6.0) < 1e-15
    assert abs(evaluation.pearson([1, 2, 3, 4], [2, 4, 6, 9]) - 11.5 / np.sqrt(5 * 26.75)) < 1e-15
    r = np.random.RandomState(0)
    a, b = r.randint(0, 5, 200), r.randn(200)
    np.testing.assert_array_equal(evaluation.average_ranks(a), H.rank_avg(a))
    assert abs(evaluation.spearman(a, b) - H.spearman_np(a, b)) < 1e-14


def test_library_version_and_new_symbols():
    lib = _lib.load()
    assert lib.qst_version() >= 103
    for name in ("qst_pair_metric", "qst_pair_loss", "qst_triplet_loss"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["qst_pair_metric"][1]) == 10
    assert len(_lib.SIGNATURES["qst_pair_loss"][1]) == 15 and len(_lib.SIGNATURES["qst_triplet_loss"][1]) == 15
