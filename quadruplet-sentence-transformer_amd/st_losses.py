"""sentence-transformers 2.2.2's row-wise pair and triplet objectives on the HIP path: `CosineSimilarityLoss`,
`ContrastiveLoss`, `OnlineContrastiveLoss`, `TripletLoss`, `SiameseDistanceMetric`, `TripletDistanceMetric` -- same
constructors and `forward(sentence_features, labels)` as `sentence_transformers.losses`, so
`model.fit(train_objectives=[(dataloader, losses.TripletLoss(model))])` is used the same way -- with the arithmetic on
the embeddings (the metric, the loss and their autograd) as fused HIP kernels: qst_pair_metric, qst_pair_loss and
qst_triplet_loss (csrc/tuple_loss.hip) through the C-ABI. Inputs must live on a HIP device: there is no CPU path.

What the classes add to sentence-transformers' signatures is `fused` (default True): the text columns of a batch run as
ONE [k*B, L] encoder pass instead of k (sentence_transformer.encode_columns_fused, the quadruplet model's rule);
`fused=False` keeps one pass per column.

A distance metric given as a member of the two metric classes maps to the kernel's metric. Any other callable
`f(rep_a, rep_b) -> [B]` is called on the embeddings as given, and the rest of the loss runs in torch on its result.

Data parallel and use_amp need nothing here (fit() shards the batch and scales the loss). Under `split_batch`
`OnlineContrastiveLoss` selects its hard pairs among the rows of each rank, as sentence-transformers under
DistributedDataParallel does too.

`MultipleNegativesRankingLoss` and `MultipleNegativesSymmetricRankingLoss` (in-batch negatives) are not row-wise: every
anchor is scored against every candidate of the batch, by qst_mnrl_loss (csrc/mnrl.hip) -- score matrix, softmax, loss and
both gradients in fp32. `similarity_fct` is recognised by identity: `util.cos_sim` and `util.dot_score` of this package
(the objects the drop-in `sentence_transformers.util` re-exports) run in the kernels; any other callable is called as
`similarity_fct(a, c) -> [B, N]` and the cross entropy runs in torch. Under `split_batch` the negatives of a rank are the
rows of its own shard, as with sentence-transformers under DistributedDataParallel: embeddings are not gathered across
ranks. `data.NoDuplicatesDataLoader` is the loader these losses are meant to be fed by.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional

import torch
from torch import nn

from . import _lib, util
from .sentence_transformer import encode_columns_fused

# include/qst.h
METRIC_COS_SIM, METRIC_COS_DIST, METRIC_L2, METRIC_L1, METRIC_DOT, METRIC_L2_PLAIN, METRIC_L1_PLAIN = range(7)
PAIR_MSE, PAIR_CONTRASTIVE, PAIR_ONLINE_CONTRASTIVE = range(3)
_RED_CODE = {"none": 0, "sum": 1, "mean": 2}
SCORE_DOT, SCORE_COS = 0, 1                       # QST_SCORE_*: what qst_mnrl_loss takes as `sim`
_SIM_CODE = {"dot": SCORE_DOT, "cos": SCORE_COS, SCORE_DOT: SCORE_DOT, SCORE_COS: SCORE_COS}


# ------------------------------------------------------------------ direct calls (contiguous fp32 HIP tensors [B, D])
def _grad_slabs(k: int, like: torch.Tensor, want: bool):
    return list(torch.empty(k, *like.shape, dtype=torch.float32, device=like.device).unbind(0)) if want else [None] * k


def pair_metric_raw(u, v, metric: int, grad_out: Optional[torch.Tensor] = None, want_grads: bool = False):
    """qst_pair_metric: the metric per row [B] and, with want_grads, grad_out[b] * d(metric[b]) / d(u[b]), d(v[b])."""
    lib = _lib.load()
    B, D = u.shape
    out = torch.empty(B, dtype=torch.float32, device=u.device)
    grads = _grad_slabs(2, u, want_grads)
    with torch.cuda.device(u.device):
        _lib.check(lib.qst_pair_metric(u.data_ptr(), v.data_ptr(), B, D, int(metric), out.data_ptr(), _lib.ptr(grad_out),
                                       _lib.ptr(grads[0]), _lib.ptr(grads[1]), _lib.current_stream_ptr()), "qst_pair_metric")
    return out, grads


def pair_loss_raw(u, v, labels, kind: int, metric: int, margin: float, reduction: int,
                  grad_out: Optional[torch.Tensor] = None, want_grads: bool = False):
    """qst_pair_loss: loss [B] (reduction none of the MSE / contrastive kinds) or [1], and the two gradients."""
    lib = _lib.load()
    B, D = u.shape
    per_row = reduction == 0 and kind != PAIR_ONLINE_CONTRASTIVE
    out = torch.empty(B if per_row else 1, dtype=torch.float32, device=u.device)
    scratch = torch.empty(B + 2, dtype=torch.float32, device=u.device)
    grads = _grad_slabs(2, u, want_grads)
    with torch.cuda.device(u.device):
        _lib.check(lib.qst_pair_loss(u.data_ptr(), v.data_ptr(), labels.data_ptr(), B, D, int(kind), int(metric), float(margin),
                                     int(reduction), out.data_ptr(), _lib.ptr(grad_out), _lib.ptr(grads[0]), _lib.ptr(grads[1]),
                                     scratch.data_ptr(), _lib.current_stream_ptr()), "qst_pair_loss")
    return out, grads


def triplet_loss_raw(a, p, n, metric: int, margin: float, reduction: int,
                     grad_out: Optional[torch.Tensor] = None, want_grads: bool = False):
    """qst_triplet_loss: relu(d(a, p) - d(a, n) + margin) per row or reduced, and the three gradients."""
    lib = _lib.load()
    B, D = a.shape
    out = torch.empty(B if reduction == 0 else 1, dtype=torch.float32, device=a.device)
    scratch = torch.empty(B, dtype=torch.float32, device=a.device)
    grads = _grad_slabs(3, a, want_grads)
    with torch.cuda.device(a.device):
        _lib.check(lib.qst_triplet_loss(a.data_ptr(), p.data_ptr(), n.data_ptr(), B, D, int(metric), float(margin),
                                        int(reduction), out.data_ptr(), _lib.ptr(grad_out), *[_lib.ptr(g) for g in grads],
                                        scratch.data_ptr(), _lib.current_stream_ptr()), "qst_triplet_loss")
    return out, grads


def mnrl_loss_raw(a, c, sim, scale: float, symmetric: bool, grad_out: Optional[torch.Tensor] = None,
                  want_grads: bool = False):
    """qst_mnrl_loss on contiguous fp32 HIP tensors a [B, D], c [N, D] (sim "cos" / "dot" or SCORE_*): the loss [1] and,
    with want_grads, [grad_a, grad_c] times grad_out (a device scalar; None = 1)."""
    lib = _lib.load()
    (B, D), N = a.shape, c.shape[0]
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    grads = [torch.empty_like(a), torch.empty_like(c)] if want_grads else [None, None]
    nbytes = int(lib.qst_mnrl_workspace_bytes(B, N, D))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(lib.qst_mnrl_loss(a.data_ptr(), c.data_ptr(), B, N, D, _SIM_CODE[sim], float(scale), int(bool(symmetric)),
                                     out.data_ptr(), _lib.ptr(grad_out), _lib.ptr(grads[0]), _lib.ptr(grads[1]),
                                     ws.data_ptr(), nbytes, _lib.current_stream_ptr()), "qst_mnrl_loss")
    return out, grads


# ------------------------------------------------------------------ autograd (save the inputs, recompute in backward)
def _f32(xs):
    return [x.detach().to(torch.float32).contiguous() for x in xs]


def _upstream(grad_output):
    return grad_output.detach().to(torch.float32).contiguous().reshape(-1)


class _PairMetricFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, v, metric):
        xs = _f32((u, v))
        out, _ = pair_metric_raw(xs[0], xs[1], metric)
        ctx.save_for_backward(*xs)
        ctx.metric, ctx.in_dtypes = metric, (u.dtype, v.dtype)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        u, v = ctx.saved_tensors
        _, grads = pair_metric_raw(u, v, ctx.metric, _upstream(grad_output), True)
        return grads[0].to(ctx.in_dtypes[0]), grads[1].to(ctx.in_dtypes[1]), None


class _PairLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, v, labels, kind, metric, margin, red_code):
        xs = _f32((u, v))
        y = labels.detach().to(torch.float32).contiguous().reshape(-1)
        out, _ = pair_loss_raw(xs[0], xs[1], y, kind, metric, margin, red_code)
        ctx.save_for_backward(xs[0], xs[1], y)
        ctx.hp, ctx.in_dtypes = (kind, metric, margin, red_code), (u.dtype, v.dtype)
        return out if red_code == 0 and kind != PAIR_ONLINE_CONTRASTIVE else out.reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        u, v, y = ctx.saved_tensors
        _, grads = pair_loss_raw(u, v, y, *ctx.hp, grad_out=_upstream(grad_output), want_grads=True)
        return grads[0].to(ctx.in_dtypes[0]), grads[1].to(ctx.in_dtypes[1]), None, None, None, None, None


class _TripletLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, p, n, metric, margin, red_code):
        xs = _f32((a, p, n))
        out, _ = triplet_loss_raw(*xs, metric, margin, red_code)
        ctx.save_for_backward(*xs)
        ctx.hp, ctx.in_dtypes = (metric, margin, red_code), (a.dtype, p.dtype, n.dtype)
        return out if red_code == 0 else out.reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        _, grads = triplet_loss_raw(*ctx.saved_tensors, *ctx.hp, grad_out=_upstream(grad_output), want_grads=True)
        return (*[g.to(dt) for g, dt in zip(grads, ctx.in_dtypes)], None, None, None)


class _MnrlFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, c, sim, scale, symmetric):
        xs = _f32((a, c))
        out, _ = mnrl_loss_raw(xs[0], xs[1], sim, scale, symmetric)
        ctx.save_for_backward(*xs)
        ctx.hp, ctx.in_dtypes = (sim, scale, symmetric), (a.dtype, c.dtype)
        return out.reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        _, grads = mnrl_loss_raw(*ctx.saved_tensors, *ctx.hp, grad_out=_upstream(grad_output), want_grads=True)
        return grads[0].to(ctx.in_dtypes[0]), grads[1].to(ctx.in_dtypes[1]), None, None, None


def _require_rows(what: str, *xs) -> None:
    if any(x.dim() != 2 for x in xs) or any(x.shape != xs[0].shape for x in xs):
        raise ValueError(f"{what}: the embeddings must all have the same shape (B, D)")
    if not all(x.is_cuda for x in xs):
        raise _lib.QstError(f"{what} runs on the HIP device only (inputs are CPU tensors; no CPU path)")


def _require_labels(what: str, labels, B: int) -> None:
    if labels.numel() != B:
        raise ValueError(f"{what}: {B} rows but {labels.numel()} labels")
    if not labels.is_cuda:
        raise _lib.QstError(f"{what} runs on the HIP device only (labels are a CPU tensor; no CPU path)")


def pair_metric(u: torch.Tensor, v: torch.Tensor, metric: int) -> torch.Tensor:
    """The row-wise metric [B] of two [B, D] HIP tensors (METRIC_* above), differentiable."""
    _require_rows("pair_metric", u, v)
    return _PairMetricFn.apply(u, v, int(metric))


def pair_loss(u, v, labels, kind: int, metric: int, margin: float = 0.5, reduction: str = "mean") -> torch.Tensor:
    """qst_pair_loss with autograd: PAIR_MSE (metric METRIC_COS_SIM), PAIR_CONTRASTIVE or PAIR_ONLINE_CONTRASTIVE
    (always a sum)."""
    if margin < 0:
        raise ValueError(f"margin must not be negative, {margin} given")
    _require_rows("pair_loss", u, v)
    _require_labels("pair_loss", labels, u.shape[0])
    return _PairLossFn.apply(u, v, labels, int(kind), int(metric), float(margin), _RED_CODE[reduction])


def triplet_loss(anchor, pos, neg, metric: int = METRIC_L2, margin: float = 5.0, reduction: str = "mean") -> torch.Tensor:
    if margin < 0:
        raise ValueError(f"margin must not be negative, {margin} given")
    _require_rows("triplet_loss", anchor, pos, neg)
    return _TripletLossFn.apply(anchor, pos, neg, int(metric), float(margin), _RED_CODE[reduction])


def multiple_negatives_ranking_loss(a: torch.Tensor, c: torch.Tensor, scale: float = 20.0, sim: str = "cos",
                                    symmetric: bool = False) -> torch.Tensor:
    """F.cross_entropy(scale * sim(a, c), arange(B)) of anchors a [B, D] and candidates c [N, D], N >= B (candidate i is
    the positive of anchor i, the rows from B on are further negatives); `symmetric` adds the cross entropy of the
    transposed B x B block and halves the sum. One qst_mnrl_loss call, differentiable in a and c."""
    if sim not in ("cos", "dot"):
        raise ValueError(f"sim is 'cos' or 'dot', {sim!r} given")
    if not (scale > 0 and scale < float("inf")):
        raise ValueError(f"scale must be positive and finite, {scale} given")
    if a.dim() != 2 or c.dim() != 2 or a.shape[1] != c.shape[1] or a.shape[1] < 1:
        raise ValueError("multiple_negatives_ranking_loss: anchors (B, D) and candidates (N, D) must share D >= 1")
    if a.shape[0] < 1 or c.shape[0] < a.shape[0]:
        raise ValueError(f"multiple_negatives_ranking_loss: {a.shape[0]} anchors need at least as many candidates, "
                         f"{c.shape[0]} given")
    if not (a.is_cuda and c.is_cuda):
        raise _lib.QstError("multiple_negatives_ranking_loss runs on the HIP device only (inputs are CPU tensors; no CPU path)")
    return _MnrlFn.apply(a, c, sim, float(scale), bool(symmetric))


def quadruplet_eval_raw(a, p, q, n, want_dist: bool = False):
    """qst_quadruplet_eval on contiguous fp32 HIP tensors [B, D] (contiguous in their own storage: a view at an offset
    is taken as it is): (dist fp32 [B, 9] or None, flags int32 [B], counts int32 [9])."""
    lib = _lib.load()
    B, D = a.shape
    dist = torch.empty(B, 9, dtype=torch.float32, device=a.device) if want_dist else None
    flags = torch.empty(B, dtype=torch.int32, device=a.device)
    counts = torch.empty(9, dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(lib.qst_quadruplet_eval(a.data_ptr(), p.data_ptr(), q.data_ptr(), n.data_ptr(), B, D, _lib.ptr(dist),
                                           flags.data_ptr(), counts.data_ptr(), _lib.current_stream_ptr()),
                   "qst_quadruplet_eval")
    return dist, flags, counts


def quadruplet_eval(a, p, q, n, want_dist: bool = False):
    """What QuadrupletEvaluator scores with, in one launch over four [B, D] HIP tensors (anchor, positive, partially
    positive, negative): index k = 3 * metric + j, metric 0 cosine distance, 1 Manhattan, 2 Euclidean.
      dist   fp32 [B, 9] (None without want_dist): j = the pair (a, p), (a, q), (a, n)
      flags  int32 [B]: bit k = comparison j holds, j = 0 d(a, p) < d(a, q), 1 d(a, p) < d(a, n), 2 d(a, q) < d(a, n)
      counts int32 [9]: rows with bit k set
    Every comparison is strict and made on the fp32 distances `dist` holds. No autograd."""
    _require_rows("quadruplet_eval", a, p, q, n)
    if a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("quadruplet_eval: the embeddings must have at least one row and one column")
    return quadruplet_eval_raw(*_f32((a, p, q, n)), want_dist=want_dist)


# ------------------------------------------------------------------ the metric classes
def _tagged(metric: int, doc: str):
    def fn(x, y):
        return pair_metric(x, y, metric)
    fn._qst_metric = metric
    fn.__doc__ = doc
    return staticmethod(fn)


class SiameseDistanceMetric:
    """The metric for the contrastive losses. As in sentence-transformers the members are plain callables
    `f(x, y) -> [B]`; these carry the kernel's metric code, and called directly they run qst_pair_metric."""
    EUCLIDEAN = _tagged(METRIC_L2, "F.pairwise_distance(x, y, p=2)")
    MANHATTAN = _tagged(METRIC_L1, "F.pairwise_distance(x, y, p=1)")
    COSINE_DISTANCE = _tagged(METRIC_COS_DIST, "1 - F.cosine_similarity(x, y)")


class TripletDistanceMetric:
    """The metric for the triplet loss (see SiameseDistanceMetric)."""
    COSINE = _tagged(METRIC_COS_DIST, "1 - F.cosine_similarity(x, y)")
    EUCLIDEAN = _tagged(METRIC_L2, "F.pairwise_distance(x, y, p=2)")
    MANHATTAN = _tagged(METRIC_L1, "F.pairwise_distance(x, y, p=1)")


def _metric_name(cls, fn) -> str:
    for name in vars(cls):
        if not name.startswith("_") and getattr(cls, name) is fn:
            return f"{cls.__name__}.{name}"
    return getattr(fn, "__name__", "Unknown")


# ------------------------------------------------------------------ the loss classes
class _TupleLoss(nn.Module):
    def __init__(self, model, fused: bool = True):
        super().__init__()
        self.model = model
        self.fused = fused

    def _embed(self, sentence_features: Iterable[Dict[str, torch.Tensor]], k: int) -> List[torch.Tensor]:
        cols = list(sentence_features)
        if len(cols) != k:
            raise ValueError(f"{type(self).__name__} takes {k} text columns per example, {len(cols)} given")
        if self.fused:
            return encode_columns_fused(self.model, cols)
        return [self.model(c)["sentence_embedding"] for c in cols]


class CosineSimilarityLoss(_TupleLoss):
    """loss_fct(cos_score_transformation(cos_sim(u, v)), labels.view(-1)). With `nn.MSELoss` (any of its reductions) and
    `nn.Identity` -- the defaults -- value and gradients are one qst_pair_loss call; with anything else the cosine
    similarity is qst_pair_metric (with its autograd) and the two callables run in torch on its [B] output."""

    def __init__(self, model, loss_fct=nn.MSELoss(), cos_score_transformation=nn.Identity(), fused: bool = True):
        super().__init__(model, fused)
        self.loss_fct = loss_fct
        self.cos_score_transformation = cos_score_transformation

    @property
    def reduction(self) -> str:
        red = getattr(self.loss_fct, "reduction", "mean")
        return red if isinstance(red, str) else "mean"

    def forward(self, sentence_features: Iterable[Dict[str, torch.Tensor]], labels: torch.Tensor) -> torch.Tensor:
        u, v = self._embed(sentence_features, 2)
        if type(self.loss_fct) is nn.MSELoss and type(self.cos_score_transformation) is nn.Identity \
                and self.loss_fct.reduction in _RED_CODE:
            return pair_loss(u, v, labels.view(-1), PAIR_MSE, METRIC_COS_SIM, 0.0, self.loss_fct.reduction)
        output = self.cos_score_transformation(pair_metric(u, v, METRIC_COS_SIM))
        return self.loss_fct(output, labels.view(-1).to(output.dtype))


class ContrastiveLoss(_TupleLoss):
    """0.5 * (label * d^2 + (1 - label) * relu(margin - d)^2), label 1 = similar pair; mean over the batch, or the sum
    with size_average=False."""

    def __init__(self, model, distance_metric=SiameseDistanceMetric.COSINE_DISTANCE, margin: float = 0.5,
                 size_average: bool = True, fused: bool = True):
        super().__init__(model, fused)
        self.distance_metric = distance_metric
        self.margin = margin
        self.size_average = size_average

    @property
    def reduction(self) -> str:
        return "mean" if self.size_average else "sum"

    def get_config_dict(self):
        return {"distance_metric": _metric_name(SiameseDistanceMetric, self.distance_metric), "margin": self.margin,
                "size_average": self.size_average}

    def forward(self, sentence_features: Iterable[Dict[str, torch.Tensor]], labels: torch.Tensor) -> torch.Tensor:
        u, v = self._embed(sentence_features, 2)
        code = getattr(self.distance_metric, "_qst_metric", None)
        if code is not None:
            return pair_loss(u, v, labels.view(-1), PAIR_CONTRASTIVE, code, self.margin, self.reduction)
        d = self.distance_metric(u, v)
        y = labels.view(-1).float()
        losses = 0.5 * (y * d.pow(2) + (1 - y) * torch.relu(self.margin - d).pow(2))
        return losses.mean() if self.size_average else losses.sum()


class OnlineContrastiveLoss(_TupleLoss):
    """ContrastiveLoss over the hard pairs of the batch only: positives farther apart than the closest negative, negatives
    closer than the farthest positive (the class mean stands in when the other class has a single member). Always a sum,
    without the factor 0.5. Labels are 0 / 1; rows with another label take no part."""
    reduction = "sum"

    def __init__(self, model, distance_metric=SiameseDistanceMetric.COSINE_DISTANCE, margin: float = 0.5,
                 fused: bool = True):
        super().__init__(model, fused)
        self.distance_metric = distance_metric
        self.margin = margin

    def forward(self, sentence_features: Iterable[Dict[str, torch.Tensor]], labels: torch.Tensor,
                size_average: bool = False) -> torch.Tensor:
        u, v = self._embed(sentence_features, 2)
        code = getattr(self.distance_metric, "_qst_metric", None)
        if code is not None:
            return pair_loss(u, v, labels.view(-1), PAIR_ONLINE_CONTRASTIVE, code, self.margin, "sum")
        d = self.distance_metric(u, v)
        y = labels.view(-1)
        negs, poss = d[y == 0], d[y == 1]
        negative_pairs = negs[negs < (poss.max() if len(poss) > 1 else negs.mean())]
        positive_pairs = poss[poss > (negs.min() if len(negs) > 1 else poss.mean())]
        return positive_pairs.pow(2).sum() + torch.relu(self.margin - negative_pairs).pow(2).sum()


class TripletLoss(_TupleLoss):
    """mean over the batch of relu(d(anchor, positive) - d(anchor, negative) + triplet_margin)."""
    reduction = "mean"

    def __init__(self, model, distance_metric=TripletDistanceMetric.EUCLIDEAN, triplet_margin: float = 5,
                 fused: bool = True):
        super().__init__(model, fused)
        self.distance_metric = distance_metric
        self.triplet_margin = triplet_margin

    def get_config_dict(self):
        return {"distance_metric": _metric_name(TripletDistanceMetric, self.distance_metric),
                "triplet_margin": self.triplet_margin}

    def forward(self, sentence_features: Iterable[Dict[str, torch.Tensor]], labels: torch.Tensor = None) -> torch.Tensor:
        a, p, n = self._embed(sentence_features, 3)
        code = getattr(self.distance_metric, "_qst_metric", None)
        if code is not None:
            return triplet_loss(a, p, n, code, self.triplet_margin, "mean")
        return torch.relu(self.distance_metric(a, p) - self.distance_metric(a, n) + self.triplet_margin).mean()


class MultipleNegativesRankingLoss(_TupleLoss):
    """F.cross_entropy(scale * similarity_fct(anchors, candidates), arange(B)): each example is (anchor, positive[, hard
    negatives ...]); the candidates of anchor i are the positives of the whole batch followed by all its hard negatives,
    and candidate i is the right answer. Takes 2 or more text columns. With `util.cos_sim` (the default) or
    `util.dot_score` the whole loss and its gradients are one qst_mnrl_loss call; any other callable is called as
    `similarity_fct(a, c) -> [B, N]` and the cross entropy runs in torch. `labels` is not looked at, as in
    sentence-transformers -- but fit() skips a step whose labels tensor is empty, so the examples keep InputExample's
    default label. Feed it from `NoDuplicatesDataLoader`: a text that appears twice in a batch is its own false negative."""
    reduction = "mean"
    _symmetric = False

    def __init__(self, model, scale: float = 20.0, similarity_fct=util.cos_sim, fused: bool = True):
        super().__init__(model, fused)
        self.scale = scale
        self.similarity_fct = similarity_fct

    def get_config_dict(self):
        return {"scale": self.scale, "similarity_fct": self.similarity_fct.__name__}

    def _kernel_sim(self) -> Optional[str]:
        if self.similarity_fct is util.cos_sim:
            return "cos"
        if self.similarity_fct is util.dot_score:
            return "dot"
        return None

    def forward(self, sentence_features: Iterable[Dict[str, torch.Tensor]], labels: torch.Tensor = None) -> torch.Tensor:
        cols = list(sentence_features)
        if len(cols) < 2:
            raise ValueError(f"{type(self).__name__} takes 2 or more text columns per example, {len(cols)} given")
        reps = self._embed(cols, len(cols))
        a = reps[0]
        c = reps[1] if len(reps) == 2 else torch.cat(reps[1:], 0)
        sim = self._kernel_sim()
        if sim is not None:
            return multiple_negatives_ranking_loss(a, c, self.scale, sim, self._symmetric)
        scores = self.similarity_fct(a, c) * self.scale
        target = torch.arange(scores.shape[0], device=scores.device)
        loss = torch.nn.functional.cross_entropy(scores, target)
        if self._symmetric:
            loss = (loss + torch.nn.functional.cross_entropy(scores[:, :scores.shape[0]].t(), target)) / 2
        return loss


class MultipleNegativesSymmetricRankingLoss(MultipleNegativesRankingLoss):
    """MultipleNegativesRankingLoss plus the same question asked the other way round -- given positive i, find anchor i among
    the anchors of the batch (the transposed B x B block of the scores) -- and the two halved."""
    _symmetric = True
