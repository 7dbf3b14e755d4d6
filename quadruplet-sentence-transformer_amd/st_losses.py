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

`CachedMultipleNegativesRankingLoss` and `CachedMultipleNegativesSymmetricRankingLoss` (GradCache; sentence-transformers
2.3) are the same two objectives at batches whose activations would not fit: the batch is embedded in mini-batches without
autograd, loss and embedding gradients come from one qst_mnrl_stream_loss call (csrc/mnrl_stream.hip: strips of anchors, no
B x N score matrix), and backward() replays the mini-batches with autograd under the same dropout masks. Single process only.

`GISTEmbedLoss` and `CachedGISTEmbedLoss` (sentence-transformers 2.3 / 3.x) are in-batch negatives filtered by a frozen
`guide` model: anchors against positives, anchors and hard negatives, positives against positives, and whatever the guide
scores above the anchor's own positive leaves the softmax. Both score matrices, the mask, the loss and the gradients of
every column are one qst_gist_loss call (csrc/gist.hip, strips as in mnrl_stream.hip); the cached form follows the three
GradCache steps with the guide embedded per mini-batch and not replayed.

`BatchHardTripletLoss`, `BatchHardSoftMarginTripletLoss`, `BatchSemiHardTripletLoss` and `BatchAllTripletLoss` take ONE text
column and an integer class label per example, and mine their triplets among the B x B distances of the batch at every
step: distance matrix, mining, loss and the gradient through the selections are qst_batch_triplet_loss
(csrc/batch_triplet.hip), fp32, without atomics. `distance_metric` is one of the two members of
`BatchHardTripletLossDistanceFunction` (recognised by their tag: they run in the kernels); any other callable is called as
`f(embeddings) -> [B, B]` and the mining runs in torch on its result -- `eucledian_distance` with `squared=True` goes that
way. `data.SentenceLabelDataset` is the loader they are meant to be fed by. Under `split_batch` rank r mines among rows
r::world of the batch only, so `samples_per_label` must be at least 2 * world for a rank to see a positive.

`MSELoss` and `MarginMSELoss` distil from a teacher (csrc/distill.hip). `MSELoss` takes ONE text column and the teacher's
embedding of each example as its label ([B, D]: SentenceTransformer.smart_batching_collate stacks vector labels, and
`data.ParallelSentencesDataset` produces them); value and gradient are one qst_embed_mse call. `MarginMSELoss` takes
(query, positive, negative) and the teacher's score margin per example; with `util.pairwise_dot_score` (the default) or
`util.pairwise_cos_sim` -- recognised by identity, like the similarity functions above -- the two similarities, their
difference, the squared error and all three gradients are one qst_margin_mse_loss call; any other callable
`f(a, b) -> [B]` is called on the embeddings and the rest runs in torch.

`DistillKLDivLoss` (sentence-transformers 3.4) and `MarginMSELoss` with four or more text columns (3.x) distil from the
teacher's scores over a LIST per query -- (query, positive, negatives ...), K candidates, labels [B, K] scores or [B, K - 1]
margins. The K similarities, the softmaxes and the divergence (or the K - 1 squared errors) and the gradients of all 1 + K
columns are one qst_listwise_distill_loss call (csrc/listwise.hip) on the one buffer the fused encoder pass returns, for the
same two similarity functions and up to 64 candidates; anything else is sentence-transformers' composition in torch ops.

`SoftmaxLoss` is the one objective here with parameters of its own: an `nn.Linear` classifier on [u, v, |u - v|, u * v] whose
weights live in a `loss_params.LossParameters`, a flat buffer the fused optimiser step takes next to the arena. Logits, cross
entropy and all four gradients are csrc/softmax_head.hip (qst_softmax_head_fwd, qst_softmax_ce, qst_softmax_head_bwd).

`CoSENTLoss` and `AnglELoss` (sentence-transformers 2.3 / 2.5) rank graded pairs: two text columns and a float label, the
loss a logsumexp over every pair of examples whose labels differ. Scores, loss and gradients are one qst_cosent_loss call
(csrc/cosent.hip) that keeps B scores instead of the B x B differences; `similarity_fct` is recognised by identity
(`util.pairwise_cos_sim`, `util.pairwise_angle_sim`), any other callable `f(u, v) -> [B]` goes through torch ops.

`MatryoshkaLoss` (sentence-transformers 2.4) wraps one of the objectives above and scores ONE encoder pass at nested prefixes
of the embedding, each cut, normalised again, weighted and summed. Over the two in-batch-negatives losses all widths are one
qst_mnrl_nested_loss call forward and one backward (csrc/mnrl_nested.hip), whatever their number up to 8; over any other
base loss, or with `fused_dims=False`, the base loss's own forward runs once per width on torch slices of the one pass.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional

import torch
from torch import nn

from . import _lib, util
from .loss_params import LossParameters
from .sentence_transformer import encode_columns_fused

# include/qst.h
METRIC_COS_SIM, METRIC_COS_DIST, METRIC_L2, METRIC_L1, METRIC_DOT, METRIC_L2_PLAIN, METRIC_L1_PLAIN = range(7)
PAIR_MSE, PAIR_CONTRASTIVE, PAIR_ONLINE_CONTRASTIVE = range(3)
_RED_CODE = {"none": 0, "sum": 1, "mean": 2}
SCORE_DOT, SCORE_COS = 0, 1                       # QST_SCORE_*: what qst_mnrl_loss takes as `sim`
_SIM_CODE = {"dot": SCORE_DOT, "cos": SCORE_COS, SCORE_DOT: SCORE_DOT, SCORE_COS: SCORE_COS}
BT_HARD, BT_HARD_SOFT, BT_SEMIHARD, BT_ALL = range(4)      # QST_BT_*: what qst_batch_triplet_loss takes as `kind`
PAIRSIM_COS, PAIRSIM_ANGLE = 0, 1                 # QST_PAIRSIM_*: what qst_cosent_loss takes as `sim`
_PAIRSIM_CODE = {"cos": PAIRSIM_COS, "angle": PAIRSIM_ANGLE, PAIRSIM_COS: PAIRSIM_COS, PAIRSIM_ANGLE: PAIRSIM_ANGLE}
GIST_ABSOLUTE, GIST_RELATIVE = 0, 1               # QST_GIST_*: what qst_gist_loss takes as `margin_strategy`
_GIST_CODE = {"absolute": GIST_ABSOLUTE, "relative": GIST_RELATIVE, GIST_ABSOLUTE: GIST_ABSOLUTE, GIST_RELATIVE: GIST_RELATIVE}


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


def mnrl_stream_loss_raw(a, c, sim, scale: float, symmetric: bool, strip_rows: int = 0,
                         grad_out: Optional[torch.Tensor] = None, want_grads: bool = False):
    """qst_mnrl_stream_loss on contiguous fp32 HIP tensors a [B, D], c [N, D]: mnrl_loss_raw without a B x N score matrix --
    the anchors are walked in strips of `strip_rows` rows (0 = the library's choice, else a positive multiple of 64)."""
    lib = _lib.load()
    (B, D), N = a.shape, c.shape[0]
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    grads = [torch.empty_like(a), torch.empty_like(c)] if want_grads else [None, None]
    nbytes = int(lib.qst_mnrl_stream_workspace_bytes(B, N, D, int(strip_rows)))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(lib.qst_mnrl_stream_loss(a.data_ptr(), c.data_ptr(), B, N, D, _SIM_CODE[sim], float(scale),
                                            int(bool(symmetric)), int(strip_rows), out.data_ptr(), _lib.ptr(grad_out),
                                            _lib.ptr(grads[0]), _lib.ptr(grads[1]), ws.data_ptr(), nbytes,
                                            _lib.current_stream_ptr()), "qst_mnrl_stream_loss")
    return out, grads


def gist_loss_raw(x, g, K: int, temperature: float, margin_strategy, margin: float, strip_rows: int = 0,
                  grad_out: Optional[torch.Tensor] = None, want_grads: bool = False):
    """qst_gist_loss on contiguous fp32 HIP tensors x [K * B, D] (the student's K text columns stacked: anchors, positives,
    hard negatives) and g [K * B, Dg] (the guide's embeddings of the same texts): the loss [1] and, with want_grads, grad_x
    times grad_out (a device scalar; None = 1), else None. margin_strategy "absolute" / "relative" or GIST_*."""
    lib = _lib.load()
    (rows, D), Dg = x.shape, g.shape[1]
    B = rows // K
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    grad = torch.empty_like(x) if want_grads else None
    nbytes = int(lib.qst_gist_workspace_bytes(B, K, D, Dg, int(strip_rows)))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.qst_gist_loss(x.data_ptr(), g.data_ptr(), B, K, D, Dg, float(temperature), _GIST_CODE[margin_strategy],
                                     float(margin), int(strip_rows), out.data_ptr(), _lib.ptr(grad_out), _lib.ptr(grad),
                                     ws.data_ptr(), nbytes, _lib.current_stream_ptr()), "qst_gist_loss")
    return out, grad


NESTED_MAX_DIMS = 8                                # the K qst_mnrl_nested_loss takes


def mnrl_nested_loss_raw(a, c, dims, weights, scale: float, symmetric: bool, grad_out: Optional[torch.Tensor] = None,
                         want_grads: bool = False):
    """qst_mnrl_nested_loss on contiguous fp32 HIP tensors a [B, D], c [N, D]: the cosine MNRL of the first dims[k] columns,
    weighted by weights[k] and summed -- (loss [1], terms [K] in the order of `dims`, [grad_a, grad_c] full width or
    [None, None]). One call whatever K (1 .. 8) is."""
    lib = _lib.load()
    if not (a.is_cuda and c.is_cuda):
        raise _lib.QstError("mnrl_nested_loss_raw runs on the HIP device only (inputs are CPU tensors; no CPU path)")
    (B, D), N = a.shape, c.shape[0]
    K = len(dims)
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    terms = torch.empty(max(K, 1), dtype=torch.float32, device=a.device)
    grads = [torch.empty_like(a), torch.empty_like(c)] if want_grads else [None, None]
    nbytes = int(lib.qst_mnrl_nested_workspace_bytes(B, N, D, K))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=a.device)
    hd = (_lib.C.c_int32 * max(K, 1))(*[int(d) for d in dims])
    hw = (_lib.C.c_float * max(K, 1))(*[float(w) for w in weights])
    with torch.cuda.device(a.device):
        _lib.check(lib.qst_mnrl_nested_loss(a.data_ptr(), c.data_ptr(), B, N, D, hd, hw, K, float(scale),
                                            int(bool(symmetric)), out.data_ptr(), terms.data_ptr(), _lib.ptr(grad_out),
                                            _lib.ptr(grads[0]), _lib.ptr(grads[1]), ws.data_ptr(), nbytes,
                                            _lib.current_stream_ptr()), "qst_mnrl_nested_loss")
    return out, terms[:K], grads


def batch_triplet_loss_raw(x, labels, kind: int, metric: int, margin: float, grad_out: Optional[torch.Tensor] = None,
                           want_grads: bool = False):
    """qst_batch_triplet_loss on a contiguous fp32 HIP tensor x [B, D] and contiguous int64 HIP labels [B] (kind BT_*,
    metric METRIC_L2_PLAIN or METRIC_COS_DIST): the loss [1], the gradient [B, D] times grad_out (a device scalar; None = 1)
    or None, and the counts int64 [2] = {terms the denominator is drawn from, terms > 0}."""
    lib = _lib.load()
    B, D = x.shape
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    counts = torch.empty(2, dtype=torch.int64, device=x.device)
    grad = torch.empty_like(x) if want_grads else None
    nbytes = int(lib.qst_batch_triplet_workspace_bytes(B, D))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.qst_batch_triplet_loss(x.data_ptr(), labels.data_ptr(), B, D, int(kind), int(metric), float(margin),
                                              out.data_ptr(), counts.data_ptr(), _lib.ptr(grad_out), _lib.ptr(grad),
                                              ws.data_ptr(), nbytes, _lib.current_stream_ptr()), "qst_batch_triplet_loss")
    return out, grad, counts


def cosent_loss_raw(u, v, labels, sim, scale: float, grad_out: Optional[torch.Tensor] = None, want_grads: bool = False):
    """qst_cosent_loss on contiguous fp32 HIP tensors u, v [B, D] and labels [B] (sim "cos" / "angle" or PAIRSIM_*): the
    loss [1], the unscaled pairwise scores [B] and, with want_grads, [grad_u, grad_v] times grad_out (a device scalar;
    None = 1), else [None, None]."""
    lib = _lib.load()
    if not (u.is_cuda and v.is_cuda and labels.is_cuda):
        raise _lib.QstError("cosent_loss_raw runs on the HIP device only (inputs are CPU tensors; no CPU path)")
    B, D = u.shape
    out = torch.empty(1, dtype=torch.float32, device=u.device)
    scores = torch.empty(B, dtype=torch.float32, device=u.device)
    grads = _grad_slabs(2, u, want_grads)
    nbytes = int(lib.qst_cosent_workspace_bytes(B, D))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=u.device)
    with torch.cuda.device(u.device):
        _lib.check(lib.qst_cosent_loss(u.data_ptr(), v.data_ptr(), labels.data_ptr(), B, D, _PAIRSIM_CODE[sim], float(scale),
                                       out.data_ptr(), scores.data_ptr(), _lib.ptr(grad_out), _lib.ptr(grads[0]),
                                       _lib.ptr(grads[1]), ws.data_ptr(), nbytes, _lib.current_stream_ptr()), "qst_cosent_loss")
    return out, scores, grads


def embed_mse_raw(x, t, grad_out: Optional[torch.Tensor] = None, want_grads: bool = False):
    """qst_embed_mse on contiguous fp32 HIP tensors [B, D]: mean((x - t)^2) [1] and, with want_grads, the gradient in x
    times grad_out (a device scalar; None = 1), else None."""
    lib = _lib.load()
    B, D = x.shape
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    scratch = torch.empty(B, dtype=torch.float32, device=x.device)
    grad = torch.empty_like(x) if want_grads else None
    with torch.cuda.device(x.device):
        _lib.check(lib.qst_embed_mse(x.data_ptr(), t.data_ptr(), B, D, out.data_ptr(), _lib.ptr(grad_out), _lib.ptr(grad),
                                     scratch.data_ptr(), _lib.current_stream_ptr()), "qst_embed_mse")
    return out, grad


def margin_mse_raw(q, p, n, labels, sim: int, reduction: int, grad_out: Optional[torch.Tensor] = None,
                   want_grads: bool = False, want_margin: bool = False):
    """qst_margin_mse_loss: (sim(q, p) - sim(q, n) - labels)^2 per row or reduced (sim METRIC_DOT or METRIC_COS_SIM), the
    three gradients, and with want_margin the margins [B] as a third result."""
    lib = _lib.load()
    B, D = q.shape
    out = torch.empty(B if reduction == 0 else 1, dtype=torch.float32, device=q.device)
    scratch = torch.empty(B, dtype=torch.float32, device=q.device)
    margin = torch.empty(B, dtype=torch.float32, device=q.device) if want_margin else None
    grads = _grad_slabs(3, q, want_grads)
    with torch.cuda.device(q.device):
        _lib.check(lib.qst_margin_mse_loss(q.data_ptr(), p.data_ptr(), n.data_ptr(), labels.data_ptr(), B, D, int(sim),
                                           int(reduction), out.data_ptr(), _lib.ptr(margin), _lib.ptr(grad_out),
                                           *[_lib.ptr(g) for g in grads], scratch.data_ptr(), _lib.current_stream_ptr()),
                   "qst_margin_mse_loss")
    return (out, grads, margin) if want_margin else (out, grads)


LISTWISE_KL, LISTWISE_MARGIN_MSE = 0, 1           # QST_LISTWISE_*: what qst_listwise_distill_loss takes as `kind`
_LISTWISE_CODE = {"kl": LISTWISE_KL, "margin_mse": LISTWISE_MARGIN_MSE, LISTWISE_KL: LISTWISE_KL,
                  LISTWISE_MARGIN_MSE: LISTWISE_MARGIN_MSE}
LISTWISE_MAX_K = 64                               # the candidates per query the kernel takes: lane j holds score j


def listwise_distill_raw(q, docs, labels, kind, sim: int, temperature: float, reduction: int,
                         grad_out: Optional[torch.Tensor] = None, want_grads: bool = False, want_scores: bool = False):
    """qst_listwise_distill_loss on contiguous fp32 HIP tensors q [B, D], docs [K, B, D] (candidate 0 the positive) and
    labels [B, K] (kind "kl" / LISTWISE_KL: the teacher's scores) or [B, K - 1] ("margin_mse": its margins): the loss per
    row [B] or reduced [1], [grad_q, grad_docs] or [None, None], and with want_scores the similarities [B, K] as a third
    result. sim METRIC_DOT or METRIC_COS_SIM."""
    lib = _lib.load()
    if not (q.is_cuda and docs.is_cuda and labels.is_cuda):
        raise _lib.QstError("listwise_distill_raw runs on the HIP device only (inputs are CPU tensors; no CPU path)")
    (B, D), K = q.shape, docs.shape[0]
    out = torch.empty(B if reduction == 0 else 1, dtype=torch.float32, device=q.device)
    scratch = torch.empty(B, dtype=torch.float32, device=q.device)
    scores = torch.empty(B, K, dtype=torch.float32, device=q.device) if want_scores else None
    grads = [torch.empty_like(q), torch.empty_like(docs)] if want_grads else [None, None]
    with torch.cuda.device(q.device):
        _lib.check(lib.qst_listwise_distill_loss(q.data_ptr(), docs.data_ptr(), labels.data_ptr(), B, K, D,
                                                 _LISTWISE_CODE[kind], int(sim), float(temperature), int(reduction),
                                                 out.data_ptr(), _lib.ptr(scores), _lib.ptr(grad_out), _lib.ptr(grads[0]),
                                                 _lib.ptr(grads[1]), scratch.data_ptr(), _lib.current_stream_ptr()),
                   "qst_listwise_distill_loss")
    return (out, grads, scores) if want_scores else (out, grads)


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


class _MnrlStreamFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, c, sim, scale, symmetric, strip_rows):
        xs = _f32((a, c))
        out, _ = mnrl_stream_loss_raw(xs[0], xs[1], sim, scale, symmetric, strip_rows)
        ctx.save_for_backward(*xs)
        ctx.hp, ctx.in_dtypes = (sim, scale, symmetric, strip_rows), (a.dtype, c.dtype)
        return out.reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        _, grads = mnrl_stream_loss_raw(*ctx.saved_tensors, *ctx.hp, grad_out=_upstream(grad_output), want_grads=True)
        return grads[0].to(ctx.in_dtypes[0]), grads[1].to(ctx.in_dtypes[1]), None, None, None, None


class _GistFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, g, K, temperature, margin_strategy, margin, strip_rows):
        xs = _f32((x, g))
        out, _ = gist_loss_raw(xs[0], xs[1], K, temperature, margin_strategy, margin, strip_rows)
        ctx.save_for_backward(*xs)
        ctx.hp, ctx.in_dtype = (K, temperature, margin_strategy, margin, strip_rows), x.dtype
        return out.reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        _, grad = gist_loss_raw(*ctx.saved_tensors, *ctx.hp, grad_out=_upstream(grad_output), want_grads=True)
        return grad.to(ctx.in_dtype), None, None, None, None, None, None


class _MnrlNestedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, c, dims, weights, scale, symmetric):
        xs = _f32((a, c))
        out, _, _ = mnrl_nested_loss_raw(xs[0], xs[1], dims, weights, scale, symmetric)
        ctx.save_for_backward(*xs)
        ctx.hp, ctx.in_dtypes = (dims, weights, scale, symmetric), (a.dtype, c.dtype)
        return out.reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        _, _, grads = mnrl_nested_loss_raw(*ctx.saved_tensors, *ctx.hp, grad_out=_upstream(grad_output), want_grads=True)
        return grads[0].to(ctx.in_dtypes[0]), grads[1].to(ctx.in_dtypes[1]), None, None, None, None


class _BatchTripletFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, labels, kind, metric, margin):
        (x32,) = _f32((x,))
        y = labels.detach().to(torch.int64).contiguous().reshape(-1)
        out, _, _ = batch_triplet_loss_raw(x32, y, kind, metric, margin)
        ctx.save_for_backward(x32, y)
        ctx.hp, ctx.in_dtype = (kind, metric, margin), x.dtype
        return out.reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        x32, y = ctx.saved_tensors
        _, grad, _ = batch_triplet_loss_raw(x32, y, *ctx.hp, grad_out=_upstream(grad_output), want_grads=True)
        return grad.to(ctx.in_dtype), None, None, None, None


class _CosentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, v, labels, sim, scale):
        xs = _f32((u, v))
        y = labels.detach().to(torch.float32).contiguous().reshape(-1)
        out, _, _ = cosent_loss_raw(xs[0], xs[1], y, sim, scale)
        ctx.save_for_backward(xs[0], xs[1], y)
        ctx.hp, ctx.in_dtypes = (sim, scale), (u.dtype, v.dtype)
        return out.reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        _, _, grads = cosent_loss_raw(*ctx.saved_tensors, *ctx.hp, grad_out=_upstream(grad_output), want_grads=True)
        return grads[0].to(ctx.in_dtypes[0]), grads[1].to(ctx.in_dtypes[1]), None, None, None


class _EmbedMseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t):
        xs = _f32((x, t))
        out, _ = embed_mse_raw(*xs)
        ctx.save_for_backward(*xs)
        ctx.in_dtype = x.dtype
        return out.reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        _, grad = embed_mse_raw(*ctx.saved_tensors, grad_out=_upstream(grad_output), want_grads=True)
        return grad.to(ctx.in_dtype), None


class _MarginMseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, p, n, labels, sim, red_code):
        xs = _f32((q, p, n))
        y = labels.detach().to(torch.float32).contiguous().reshape(-1)
        out, _ = margin_mse_raw(*xs, y, sim, red_code)
        ctx.save_for_backward(*xs, y)
        ctx.hp, ctx.in_dtypes = (sim, red_code), (q.dtype, p.dtype, n.dtype)
        return out if red_code == 0 else out.reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        _, grads = margin_mse_raw(*ctx.saved_tensors, *ctx.hp, grad_out=_upstream(grad_output), want_grads=True)
        return (*[g.to(dt) for g, dt in zip(grads, ctx.in_dtypes)], None, None, None)


class _ListwiseDistillFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, docs, labels, kind, sim, temperature, red_code):
        xs = _f32((q, docs))
        y = labels.detach().to(torch.float32).contiguous()
        out, _ = listwise_distill_raw(*xs, y, kind, sim, temperature, red_code)
        ctx.save_for_backward(*xs, y)
        ctx.hp, ctx.in_dtypes = (kind, sim, temperature, red_code), (q.dtype, docs.dtype)
        return out if red_code == 0 else out.reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        _, grads = listwise_distill_raw(*ctx.saved_tensors, *ctx.hp, grad_out=_upstream(grad_output), want_grads=True)
        return (*[g.to(dt) for g, dt in zip(grads, ctx.in_dtypes)], None, None, None, None, None)


def _device_of(model) -> torch.device:
    """Where a model's tensors live: its `device`, else that of its first parameter, else the CPU (a stand-in without any)."""
    dev = getattr(model, "device", None)
    if isinstance(dev, (str, torch.device)):
        return torch.device(dev)
    first = next(iter(model.parameters()), None) if isinstance(model, nn.Module) else None
    return first.device if first is not None else torch.device("cpu")


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


def _check_mnrl_args(name: str, a: torch.Tensor, c: torch.Tensor, scale: float, sim: str) -> None:
    if sim not in ("cos", "dot"):
        raise ValueError(f"sim is 'cos' or 'dot', {sim!r} given")
    if not (scale > 0 and scale < float("inf")):
        raise ValueError(f"scale must be positive and finite, {scale} given")
    if a.dim() != 2 or c.dim() != 2 or a.shape[1] != c.shape[1] or a.shape[1] < 1:
        raise ValueError(f"{name}: anchors (B, D) and candidates (N, D) must share D >= 1")
    if a.shape[0] < 1 or c.shape[0] < a.shape[0]:
        raise ValueError(f"{name}: {a.shape[0]} anchors need at least as many candidates, {c.shape[0]} given")
    if not (a.is_cuda and c.is_cuda):
        raise _lib.QstError(f"{name} runs on the HIP device only (inputs are CPU tensors; no CPU path)")


def multiple_negatives_ranking_loss_stream(a: torch.Tensor, c: torch.Tensor, scale: float = 20.0, sim: str = "cos",
                                           symmetric: bool = False, strip_rows: int = 0) -> torch.Tensor:
    """multiple_negatives_ranking_loss for batches whose B x N score matrix should not exist: one qst_mnrl_stream_loss call,
    which scores `strip_rows` anchors at a time (0 = the library's choice, else a positive multiple of 64) on the fp32 matrix
    cores. Differentiable in a and c; memory linear in B + N."""
    if strip_rows < 0 or strip_rows % 64 != 0:
        raise ValueError(f"strip_rows is 0 or a positive multiple of 64, {strip_rows} given")
    _check_mnrl_args("multiple_negatives_ranking_loss_stream", a, c, scale, sim)
    return _MnrlStreamFn.apply(a, c, sim, float(scale), bool(symmetric), int(strip_rows))


def _check_gist_hp(temperature: float, margin_strategy: str, margin: float) -> None:
    if not (temperature > 0 and temperature < float("inf")):
        raise ValueError(f"temperature must be positive and finite, {temperature} given")
    if margin_strategy not in ("absolute", "relative"):
        raise ValueError(f"margin_strategy is 'absolute' or 'relative', {margin_strategy!r} given")
    if not (margin > float("-inf") and margin < float("inf")):
        raise ValueError(f"margin must be finite, {margin} given")


def gist_embed_loss(reps, guide_reps, temperature: float = 0.01, margin_strategy: str = "absolute", margin: float = 0.0,
                    strip_rows: int = 0) -> torch.Tensor:
    """GISTEmbedLoss on embeddings: `reps` the student's K >= 2 text columns [B, D] (anchors, positives, hard negatives ...),
    `guide_reps` the guide's embeddings of the same texts [B, Dg]. Every anchor is scored against all positives, anchors and
    hard negatives and every positive against all positives (cosine / temperature); a candidate the guide finds more similar
    than the anchor's own positive -- guide score > thr_i - margin ("absolute") or thr_i * (1 - margin) ("relative") --
    leaves the softmax, the positive itself never does. One qst_gist_loss call, differentiable in `reps`; the guide gets no
    gradient. strip_rows as in multiple_negatives_ranking_loss_stream."""
    reps, guide_reps = list(reps), list(guide_reps)
    if len(reps) < 2 or len(guide_reps) != len(reps):
        raise ValueError(f"gist_embed_loss takes 2 or more text columns and as many guide columns, {len(reps)} and "
                         f"{len(guide_reps)} given")
    _check_gist_hp(temperature, margin_strategy, margin)
    if strip_rows < 0 or strip_rows % 64 != 0:
        raise ValueError(f"strip_rows is 0 or a positive multiple of 64, {strip_rows} given")
    for what, xs in (("student", reps), ("guide", guide_reps)):
        if any(x.dim() != 2 or x.shape != xs[0].shape for x in xs) or xs[0].shape[0] < 1 or xs[0].shape[1] < 1:
            raise ValueError(f"gist_embed_loss: the {what} columns must all have the same shape (B, D), B and D at least 1")
    if guide_reps[0].shape[0] != reps[0].shape[0]:
        raise ValueError(f"gist_embed_loss: {reps[0].shape[0]} student rows but {guide_reps[0].shape[0]} guide rows")
    if not all(x.is_cuda for x in reps + guide_reps):
        raise _lib.QstError("gist_embed_loss runs on the HIP device only (inputs are CPU tensors; no CPU path)")
    return _GistFn.apply(torch.cat(reps, 0), torch.cat([r.detach() for r in guide_reps], 0), len(reps), float(temperature),
                         margin_strategy, float(margin), int(strip_rows))


def matryoshka_mnrl_loss(a: torch.Tensor, c: torch.Tensor, dims, weights=None, scale: float = 20.0,
                         symmetric: bool = False) -> torch.Tensor:
    """sum_k weights[k] * MNRL(F.normalize(a[:, :dims[k]]), F.normalize(c[:, :dims[k]])) of anchors a [B, D] and candidates
    c [N, D], N >= B: 1 .. 8 distinct widths in any order, each at most D. One qst_mnrl_nested_loss call, differentiable in
    a and c (the gradients are full width, zero from the largest width on)."""
    dims = tuple(int(d) for d in dims)
    weights = tuple(float(w) for w in (weights if weights is not None else [1.0] * len(dims)))
    if a.dim() != 2 or c.dim() != 2 or a.shape[1] != c.shape[1] or a.shape[1] < 1:
        raise ValueError("matryoshka_mnrl_loss: anchors (B, D) and candidates (N, D) must share D >= 1")
    if a.shape[0] < 1 or c.shape[0] < a.shape[0]:
        raise ValueError(f"matryoshka_mnrl_loss: {a.shape[0]} anchors need at least as many candidates, {c.shape[0]} given")
    if not 1 <= len(dims) <= NESTED_MAX_DIMS or len(set(dims)) != len(dims) or len(weights) != len(dims):
        raise ValueError(f"matryoshka_mnrl_loss: 1 to {NESTED_MAX_DIMS} distinct widths and as many weights, "
                         f"{list(dims)} and {list(weights)} given")
    if min(dims) < 1 or max(dims) > a.shape[1]:
        raise ValueError(f"matryoshka_mnrl_loss: the widths {list(dims)} must lie in 1 .. {a.shape[1]}, the embedding width")
    if not (scale > 0 and scale < float("inf")):
        raise ValueError(f"scale must be positive and finite, {scale} given")
    if not (a.is_cuda and c.is_cuda):
        raise _lib.QstError("matryoshka_mnrl_loss runs on the HIP device only (inputs are CPU tensors; no CPU path)")
    return _MnrlNestedFn.apply(a, c, dims, weights, float(scale), bool(symmetric))


def batch_triplet_loss(x: torch.Tensor, labels: torch.Tensor, kind: int = BT_HARD, metric: int = METRIC_L2_PLAIN,
                       margin: float = 5.0) -> torch.Tensor:
    """One of the four batch-mining triplet losses (kind BT_HARD, BT_HARD_SOFT, BT_SEMIHARD, BT_ALL) of embeddings x [B, D]
    with one integer class label per row, under METRIC_L2_PLAIN (eucledian_distance) or METRIC_COS_DIST (cosine_distance).
    One qst_batch_triplet_loss call, differentiable in x. BT_HARD_SOFT takes no margin. BT_SEMIHARD is NaN for a batch in
    which no label occurs twice, as in sentence-transformers."""
    if kind not in (BT_HARD, BT_HARD_SOFT, BT_SEMIHARD, BT_ALL):
        raise ValueError(f"kind is one of BT_HARD, BT_HARD_SOFT, BT_SEMIHARD, BT_ALL (0 .. 3), {kind!r} given")
    if metric not in (METRIC_L2_PLAIN, METRIC_COS_DIST):
        raise ValueError(f"metric is METRIC_L2_PLAIN or METRIC_COS_DIST, {metric!r} given")
    if not (margin >= 0 and margin < float("inf")):
        raise ValueError(f"margin must be finite and not negative, {margin} given")
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("batch_triplet_loss: the embeddings must have the shape (B, D), B >= 1, D >= 1")
    if labels.dtype.is_floating_point or labels.dtype == torch.bool or labels.is_complex():
        raise ValueError(f"batch_triplet_loss: the labels are integer class ids, {labels.dtype} given")
    if labels.numel() != x.shape[0]:
        raise ValueError(f"batch_triplet_loss: {x.shape[0]} rows but {labels.numel()} labels")
    _require_rows("batch_triplet_loss", x)
    _require_labels("batch_triplet_loss", labels, x.shape[0])
    return _BatchTripletFn.apply(x, labels, int(kind), int(metric), float(margin))


def cosent_loss(u: torch.Tensor, v: torch.Tensor, labels: torch.Tensor, scale: float = 20.0, sim: str = "cos") -> torch.Tensor:
    """log(1 + sum over the pairs (i, j) with labels[i] < labels[j] of exp(scale * (s_i - s_j))) of two [B, D] HIP tensors and
    the grades [B], s the pairwise cosine (sim "cos") or util.pairwise_angle_sim (sim "angle", D even). One qst_cosent_loss
    call, differentiable in u and v; O(B) memory whatever B is."""
    if sim not in ("cos", "angle"):
        raise ValueError(f"sim is 'cos' or 'angle', {sim!r} given")
    if not (scale > 0 and scale < float("inf")):
        raise ValueError(f"scale must be positive and finite, {scale} given")
    if u.dim() != 2 or u.shape != v.shape or u.shape[0] < 1 or u.shape[1] < 1:
        raise ValueError(f"cosent_loss: two (B, D) tensors of one shape, {tuple(u.shape)} and {tuple(v.shape)} given")
    if sim == "angle" and u.shape[1] % 2:
        raise ValueError(f"cosent_loss: the angle similarity splits each row into two halves: the width {u.shape[1]} is odd")
    if labels.numel() != u.shape[0]:
        raise ValueError(f"cosent_loss: {u.shape[0]} rows but {labels.numel()} labels")
    _require_rows("cosent_loss", u, v)
    _require_labels("cosent_loss", labels, u.shape[0])
    return _CosentFn.apply(u, v, labels, sim, float(scale))


def cosent_loss_torch(scores: torch.Tensor, labels: torch.Tensor, scale: float = 20.0) -> torch.Tensor:
    """The same loss from the pairwise scores [B] as sentence-transformers composes it in torch ops: the B x B differences,
    the label mask pushed down by 1e12, logsumexp with a zero in front. What CoSENTLoss runs on a foreign similarity_fct."""
    s = scores * scale
    s = s[:, None] - s[None, :]
    mask = (labels[:, None] < labels[None, :]).to(s.dtype)
    s = s - (1 - mask) * 1e12
    return torch.logsumexp(torch.cat((torch.zeros(1, dtype=s.dtype, device=s.device), s.view(-1)), dim=0), dim=0)


def embed_mse(x: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """torch.nn.MSELoss()(x, t) of two [B, D] HIP tensors: the mean over all B * D elements of (x - t)^2. One qst_embed_mse
    call, differentiable in x; the target carries no gradient."""
    if x.dim() != 2 or x.shape != t.shape or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"embed_mse: embeddings {tuple(x.shape)} and targets {tuple(t.shape)} must share one shape (B, D)")
    _require_rows("embed_mse", x, t)
    return _EmbedMseFn.apply(x, t)


def margin_mse(q, p, n, labels, sim: int = METRIC_DOT, reduction: str = "mean") -> torch.Tensor:
    """(sim(q, p) - sim(q, n) - labels)^2 of three [B, D] HIP tensors and the teacher's margins [B], sim METRIC_DOT or
    METRIC_COS_SIM. One qst_margin_mse_loss call, differentiable in q, p and n."""
    if sim not in (METRIC_DOT, METRIC_COS_SIM):
        raise ValueError(f"sim is METRIC_DOT or METRIC_COS_SIM, {sim!r} given")
    if q.dim() == 2 and labels.numel() != q.shape[0]:
        raise ValueError(f"margin_mse: {q.shape[0]} rows but {labels.numel()} labels")
    _require_rows("margin_mse", q, p, n)
    _require_labels("margin_mse", labels, q.shape[0])
    return _MarginMseFn.apply(q, p, n, labels, int(sim), _RED_CODE[reduction])


def _listwise_label_shape(kind: int, B: int, K: int) -> tuple:
    return (B, K) if kind == LISTWISE_KL else (B, K - 1)


def listwise_distill(q, docs, labels, kind="kl", sim: int = METRIC_DOT, temperature: float = 1.0,
                     reduction: str = "mean") -> torch.Tensor:
    """Distillation over a list of candidates per query: q [B, D], docs [K, B, D] (candidate 0 the positive, 1 <= K <= 64),
    sim METRIC_DOT or METRIC_COS_SIM. kind "kl": temperature^2 * KL(softmax(labels / temperature) ||
    softmax(sim(q, docs) / temperature)) per row, labels [B, K] the teacher's scores, "mean" over the batch (batchmean).
    kind "margin_mse": sum over the negatives of (sim(q, docs_0) - sim(q, docs_j) - labels_{j-1})^2, labels [B, K - 1] the
    teacher's margins, "mean" over all B (K - 1) of them. One qst_listwise_distill_loss call, differentiable in q and docs."""
    if kind not in _LISTWISE_CODE:
        raise ValueError(f"kind is 'kl' or 'margin_mse', {kind!r} given")
    kind = _LISTWISE_CODE[kind]
    if sim not in (METRIC_DOT, METRIC_COS_SIM):
        raise ValueError(f"sim is METRIC_DOT or METRIC_COS_SIM, {sim!r} given")
    if reduction not in _RED_CODE:
        raise ValueError(f"reduction is 'none', 'sum' or 'mean', {reduction!r} given")
    if q.dim() != 2 or docs.dim() != 3 or docs.shape[1:] != q.shape or q.shape[0] < 1 or q.shape[1] < 1:
        raise ValueError(f"listwise_distill: queries (B, D) and candidates (K, B, D), {tuple(q.shape)} and "
                         f"{tuple(docs.shape)} given")
    (B, _), K = q.shape, docs.shape[0]
    k_min = 2 if kind == LISTWISE_MARGIN_MSE else 1
    if not k_min <= K <= LISTWISE_MAX_K:
        raise ValueError(f"listwise_distill: {K} candidates per query; the kernel takes {k_min} to {LISTWISE_MAX_K}")
    want = _listwise_label_shape(kind, B, K)
    if tuple(labels.shape) != want:
        raise ValueError(f"listwise_distill: the labels of {tuple(docs.shape)} candidates have the shape {want}; "
                         f"{tuple(labels.shape)} given")
    if kind == LISTWISE_KL and not (0.0 < float(temperature) < float("inf")):
        raise ValueError(f"temperature must be finite and positive, {temperature!r} given")
    if not (q.is_cuda and docs.is_cuda):
        raise _lib.QstError("listwise_distill runs on the HIP device only (inputs are CPU tensors; no CPU path)")
    if not labels.is_cuda:
        raise _lib.QstError("listwise_distill runs on the HIP device only (labels are a CPU tensor; no CPU path)")
    return _ListwiseDistillFn.apply(q, docs, labels, kind, int(sim), float(temperature), _RED_CODE[reduction])


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


# ------------------------------------------------------------------ GradCache over the in-batch-negatives losses
def mini_batch_bounds(batch_size: int, mini_batch_size: int) -> List[tuple]:
    """[(lo, hi)] of the mini-batches of a batch, in order; the last one may be ragged, and a mini_batch_size of at least
    the batch gives one."""
    if mini_batch_size < 1:
        raise ValueError(f"mini_batch_size must be at least 1, {mini_batch_size} given")
    return [(lo, min(batch_size, lo + mini_batch_size)) for lo in range(0, batch_size, mini_batch_size)]


def slice_features(cols: List[Dict[str, torch.Tensor]], lo: int, hi: int) -> List[Dict[str, torch.Tensor]]:
    """Rows lo .. hi-1 of every text column of an already-collated batch (views; whatever is not a tensor passes through)."""
    return [{k: (v[lo:hi] if isinstance(v, torch.Tensor) else v) for k, v in col.items()} for col in cols]


def _sentence_transformer_of(model):
    """The SentenceTransformer behind `model`: the model itself, or what a wrapper holds as `.model`."""
    while not hasattr(model, "_enc") and hasattr(model, "model"):
        model = model.model
    if not hasattr(model, "_enc"):
        raise TypeError(f"{type(model).__name__} is not a SentenceTransformer of this package and wraps none as .model")
    return model


class _GradCacheFn(torch.autograd.Function):
    """The loss value of step 2; its backward is step 3, the replay of the mini-batches with the cached gradients."""

    @staticmethod
    def forward(ctx, hook, loss, replay):
        ctx.replay = replay
        return loss.reshape(()).clone()

    @staticmethod
    def backward(ctx, grad_output):
        ctx.replay(grad_output)
        ctx.replay = None
        return None, None, None


class CachedMultipleNegativesRankingLoss(MultipleNegativesRankingLoss):
    """MultipleNegativesRankingLoss at a batch size the activations of one pass would not fit (GradCache, Gao et al. 2021):
      1. the batch is embedded in mini-batches of `mini_batch_size` examples without autograd;
      2. loss and its gradient with respect to all embeddings come from ONE qst_mnrl_stream_loss call
         (csrc/mnrl_stream.hip: no B x N score matrix either);
      3. backward() runs every mini-batch again with autograd and pushes its slice of that gradient through the encoder.
    Memory is that of one mini-batch whatever the batch; the price is one more forward. The second pass sees the masks of
    the first: dropout masks here are a function of (seed, step, tensor, element), so the replay puts the encoder's step
    counter back (HipEncoder.set_dropout_step) instead of saving and restoring generator states, and afterwards the counter
    stands where step 1 left it. Both passes run at fit()'s `precision`. A foreign `similarity_fct` is scored by torch ops on
    the full matrix, as in MultipleNegativesRankingLoss. Without autograd (torch.no_grad(), eval()) forward is steps 1 and 2
    without gradients. Not supported yet: a data-parallel fit() (refused there), and MatryoshkaLoss around it."""
    _replays_mini_batches = True        # what fit() refuses in a data-parallel world

    def __init__(self, model, scale: float = 20.0, similarity_fct=util.cos_sim, mini_batch_size: int = 32,
                 show_progress_bar: bool = False, fused: bool = True):
        super().__init__(model, scale, similarity_fct, fused)
        if mini_batch_size < 1:
            raise ValueError(f"mini_batch_size must be at least 1, {mini_batch_size} given")
        self.mini_batch_size = int(mini_batch_size)
        self.show_progress_bar = show_progress_bar

    def _scores_in_torch(self, a, c):
        scores = self.similarity_fct(a, c) * self.scale
        target = torch.arange(scores.shape[0], device=scores.device)
        loss = torch.nn.functional.cross_entropy(scores, target)
        if self._symmetric:
            loss = (loss + torch.nn.functional.cross_entropy(scores[:, :scores.shape[0]].t(), target)) / 2
        return loss

    def _loss_and_cache(self, a, c, want_grads: bool):
        """Step 2: the loss [1] and, with want_grads, d loss / d a and d loss / d c."""
        sim = self._kernel_sim()
        if sim is not None:
            return mnrl_stream_loss_raw(a, c, sim, self.scale, self._symmetric, want_grads=want_grads)
        if not want_grads:
            return self._scores_in_torch(a, c).reshape(1), [None, None]
        with torch.enable_grad():
            a, c = a.requires_grad_(True), c.requires_grad_(True)
            loss = self._scores_in_torch(a, c)
            grads = torch.autograd.grad(loss, [a, c])
        return loss.detach().reshape(1), [g.to(torch.float32) for g in grads]

    def _mini_batches(self, bounds):
        if not self.show_progress_bar:
            return bounds
        from tqdm.autonotebook import tqdm
        return tqdm(bounds, desc="Mini-batches", leave=False)

    def forward(self, sentence_features: Iterable[Dict[str, torch.Tensor]], labels: torch.Tensor = None) -> torch.Tensor:
        cols = list(sentence_features)
        k = len(cols)
        if k < 2:
            raise ValueError(f"{type(self).__name__} takes 2 or more text columns per example, {k} given")
        st = _sentence_transformer_of(self.model)
        enc = st._enc
        B = cols[0]["input_ids"].shape[0]
        bounds = mini_batch_bounds(B, self.mini_batch_size)
        want_grads = torch.is_grad_enabled() and st.training

        # 1. every mini-batch without autograd, at the precision (and with the masks) its replay will have
        steps, parts = [], []
        with torch.no_grad(), st.no_grad_passes_at_training_precision():
            for lo, hi in self._mini_batches(bounds):
                steps.append(enc.dropout_step)
                parts.append([r.to(torch.float32) for r in self._embed(slice_features(cols, lo, hi), k)])
        end = enc.dropout_step
        reps = [torch.cat([p[j] for p in parts], 0) if len(parts) > 1 else parts[0][j] for j in range(k)]
        a = reps[0].contiguous()
        c = (reps[1] if k == 2 else torch.cat(reps[1:], 0)).contiguous()
        del parts, reps

        # 2. the loss and the gradient cache
        loss, (grad_a, grad_c) = self._loss_and_cache(a, c, want_grads)
        if not want_grads:
            return loss.reshape(())

        # 3. backward(): one mini-batch's activation arena at a time
        def replay(grad_output):
            g = _upstream(grad_output)                  # a device scalar: under use_amp it carries the loss scale
            with torch.enable_grad():
                for (lo, hi), step in zip(self._mini_batches(bounds), steps):
                    enc.set_dropout_step(step)
                    again = self._embed(slice_features(cols, lo, hi), k)
                    cached = [grad_a[lo:hi]] + [grad_c[(j - 1) * B + lo:(j - 1) * B + hi] for j in range(1, k)]
                    torch.autograd.backward(again, [(d * g).to(r.dtype) for d, r in zip(cached, again)])
            enc.set_dropout_step(end)

        hook = torch.zeros((), device=a.device, requires_grad=True)
        return _GradCacheFn.apply(hook, loss, replay)


class CachedMultipleNegativesSymmetricRankingLoss(CachedMultipleNegativesRankingLoss):
    """MultipleNegativesSymmetricRankingLoss by the three steps of CachedMultipleNegativesRankingLoss."""
    _symmetric = True


# ------------------------------------------------------------------ guided in-batch negatives
def _synthetic_ids_agree(a, b) -> bool:
    """Two models without vocabulary files hash a text to the same ids when their stand-in tokenizers agree."""
    ta, tb = a._synthetic_tokenizer, b._synthetic_tokenizer
    return (a.cfg.vocab_size, ta.cls_id, ta.sep_id, ta.pad_id) == (b.cfg.vocab_size, tb.cls_id, tb.sep_id, tb.pad_id)


def _must_retokenize(st, guide) -> bool:
    """sentence-transformers' rule: the guide reads the model's token ids unless its vocabulary or max_seq_length differs;
    then the ids are decoded and tokenised again by the guide. Ids of a stand-in tokenizer (a model without vocabulary files)
    cannot be decoded, and a guide with one cannot tokenise real text the same way: such a pair raises instead of scoring
    garbage."""
    if st.tokenizer is None and guide.tokenizer is None:
        if _synthetic_ids_agree(st, guide) and st.max_seq_length == guide.max_seq_length:
            return False
        raise ValueError("GISTEmbedLoss: model and guide have no vocabulary files and their stand-in tokenizers or "
                         "max_seq_length differ; the model's token ids cannot be decoded for the guide")
    if st.tokenizer is None or guide.tokenizer is None:
        raise ValueError("GISTEmbedLoss: one of model and guide has a real vocabulary and the other a stand-in tokenizer; "
                         "the model's token ids cannot be turned into the guide's")
    return st.tokenizer.get_vocab() != guide.tokenizer.get_vocab() or st.max_seq_length != guide.max_seq_length


class GISTEmbedLoss(_TupleLoss):
    """sentence-transformers' GISTEmbedLoss (Solatorio 2024): MultipleNegativesRankingLoss whose in-batch negatives a frozen
    `guide` model filters. Each example is (anchor, positive[, hard negatives ...]); anchor i is scored against every positive,
    every anchor and every hard negative of the batch, and positive i against every positive (cosine / temperature). A
    candidate the guide finds more similar to the anchor than the anchor's own positive is a probable false negative and
    leaves the softmax: guide score > thr_i - margin (`margin_strategy="absolute"`) or > thr_i * (1 - margin) ("relative"),
    thr_i the guide's score of (anchor i, positive i); margin 0 is the paper's rule. A text that appears twice in a batch is
    removed that way too. Student scores, guide scores, mask, loss and the gradients of all columns are ONE qst_gist_loss call
    (csrc/gist.hip).

    `guide` is a SentenceTransformer of this package, of any width. It is embedded under torch.no_grad() in eval mode and is
    not a submodule of the loss: train() does not reach it, and fit() neither steps nor checkpoints it. If its vocabulary or
    max_seq_length differs from the model's, the model's input_ids are decoded and tokenised again for it. `labels` is not
    looked at (see MultipleNegativesRankingLoss for fit() and empty labels)."""
    reduction = "mean"

    def __init__(self, model, guide, temperature: float = 0.01, margin_strategy: str = "absolute", margin: float = 0.0,
                 fused: bool = True):
        super().__init__(model, fused)
        _check_gist_hp(temperature, margin_strategy, margin)
        from .sentence_transformer import SentenceTransformer
        if not isinstance(guide, SentenceTransformer):
            raise TypeError(f"guide must be a SentenceTransformer of this package, {type(guide).__name__} given")
        object.__setattr__(self, "guide", guide.eval())     # not registered: a frozen model, outside train() and parameters()
        self.temperature = temperature
        self.margin_strategy = margin_strategy
        self.margin = margin
        self.must_retokenize = _must_retokenize(_sentence_transformer_of(model), guide)

    def get_config_dict(self):
        return {"guide": getattr(self.guide, "_model_card_name", None) or type(self.guide).__name__,
                "temperature": self.temperature, "margin_strategy": self.margin_strategy, "margin": self.margin}

    def _guide_columns(self, cols):
        if not self.must_retokenize:
            return [dict(c) for c in cols]
        tok = _sentence_transformer_of(self.model).tokenizer
        dev = self.guide.device
        return [{k: v.to(dev) for k, v in self.guide.tokenize(tok.batch_decode(c["input_ids"], skip_special_tokens=True)).items()}
                for c in cols]

    def _embed_guide(self, cols) -> torch.Tensor:
        """The guide's embeddings of every column, stacked [K * B, Dg] fp32: no autograd, eval mode (no dropout)."""
        guide = self.guide
        with torch.no_grad():
            guide.eval()
            reps = encode_columns_fused(guide, self._guide_columns(cols))
        return torch.cat([r.to(torch.float32) for r in reps], 0)

    def forward(self, sentence_features: Iterable[Dict[str, torch.Tensor]], labels: torch.Tensor = None) -> torch.Tensor:
        cols = list(sentence_features)
        if len(cols) < 2:
            raise ValueError(f"{type(self).__name__} takes 2 or more text columns per example, {len(cols)} given")
        guide_reps = self._embed_guide(cols)
        reps = self._embed(cols, len(cols))
        return gist_embed_loss(reps, guide_reps.chunk(len(cols), 0), self.temperature, self.margin_strategy, self.margin)


class CachedGISTEmbedLoss(GISTEmbedLoss):
    """GISTEmbedLoss by the three steps of CachedMultipleNegativesRankingLoss (GradCache): (1) every mini-batch of
    `mini_batch_size` examples is embedded without autograd, by the model and by the guide; (2) the loss and its gradient with
    respect to all student embeddings come from ONE qst_gist_loss call, which holds no B x B tensor; (3) backward() replays the
    model's mini-batches with autograd under the masks of the first pass. The guide is not replayed. Single process only."""
    _replays_mini_batches = True        # what fit() refuses in a data-parallel world

    def __init__(self, model, guide, temperature: float = 0.01, mini_batch_size: int = 32, show_progress_bar: bool = False,
                 margin_strategy: str = "absolute", margin: float = 0.0):
        super().__init__(model, guide, temperature, margin_strategy, margin)
        if mini_batch_size < 1:
            raise ValueError(f"mini_batch_size must be at least 1, {mini_batch_size} given")
        self.mini_batch_size = int(mini_batch_size)
        self.show_progress_bar = show_progress_bar

    _mini_batches = CachedMultipleNegativesRankingLoss._mini_batches

    def forward(self, sentence_features: Iterable[Dict[str, torch.Tensor]], labels: torch.Tensor = None) -> torch.Tensor:
        cols = list(sentence_features)
        k = len(cols)
        if k < 2:
            raise ValueError(f"{type(self).__name__} takes 2 or more text columns per example, {k} given")
        st = _sentence_transformer_of(self.model)
        enc = st._enc
        B = cols[0]["input_ids"].shape[0]
        bounds = mini_batch_bounds(B, self.mini_batch_size)
        want_grads = torch.is_grad_enabled() and st.training

        # 1. every mini-batch without autograd: the guide's embeddings, and the student's at the precision (and with the
        #    masks) its replay will have
        steps, parts, guide_parts = [], [], []
        with torch.no_grad(), st.no_grad_passes_at_training_precision():
            for lo, hi in self._mini_batches(bounds):
                mini = slice_features(cols, lo, hi)
                guide_parts.append(self._embed_guide(mini).view(k, hi - lo, -1))
                steps.append(enc.dropout_step)
                parts.append(torch.stack([r.to(torch.float32) for r in self._embed(mini, k)], 0))
        end = enc.dropout_step
        x = torch.cat(parts, 1).reshape(k * B, -1)      # [k, B, D] stacked in column order
        g = torch.cat(guide_parts, 1).reshape(k * B, -1)
        del parts, guide_parts

        # 2. the loss and the gradient cache
        loss, grad_x = gist_loss_raw(x, g, k, self.temperature, self.margin_strategy, self.margin, want_grads=want_grads)
        if not want_grads:
            return loss.reshape(())

        # 3. backward(): one mini-batch's activation arena at a time, the student only
        def replay(grad_output):
            scale = _upstream(grad_output)              # a device scalar: under use_amp it carries the loss scale
            with torch.enable_grad():
                for (lo, hi), step in zip(self._mini_batches(bounds), steps):
                    enc.set_dropout_step(step)
                    again = self._embed(slice_features(cols, lo, hi), k)
                    cached = [grad_x[j * B + lo:j * B + hi] for j in range(k)]
                    torch.autograd.backward(again, [(d * scale).to(r.dtype) for d, r in zip(cached, again)])
            enc.set_dropout_step(end)

        hook = torch.zeros((), device=x.device, requires_grad=True)
        return _GradCacheFn.apply(hook, loss, replay)


# ------------------------------------------------------------------ the batch-mining triplet losses
class BatchHardTripletLossDistanceFunction:
    """The distance of every pair of rows of the batch, `f(embeddings) -> [B, B]`. The members carry the kernel's metric
    code: given to one of the four losses below as they are, they run inside qst_batch_triplet_loss; called directly they
    are sentence-transformers' torch formulas, on any device and differentiable."""

    @staticmethod
    def cosine_distance(embeddings):
        """1 - cos_sim(embeddings, embeddings)"""
        e = torch.nn.functional.normalize(embeddings, p=2, dim=1, eps=1e-12)
        return 1 - e @ e.t()

    @staticmethod
    def eucledian_distance(embeddings, squared=False):
        """||a - b||_2 (squared: its square) from the Gram matrix, clamped at 0; an exactly-zero distance has gradient 0."""
        dot_product = embeddings @ embeddings.t()
        square_norm = torch.diag(dot_product)
        distances = (square_norm.unsqueeze(0) - 2.0 * dot_product + square_norm.unsqueeze(1)).clamp_min(0)
        if not squared:
            mask = distances.eq(0).to(distances.dtype)
            distances = (1.0 - mask) * torch.sqrt(distances + mask * 1e-16)
        return distances


BatchHardTripletLossDistanceFunction.cosine_distance._qst_metric = METRIC_COS_DIST
BatchHardTripletLossDistanceFunction.eucledian_distance._qst_metric = METRIC_L2_PLAIN


def _masked_minimum(data, mask, dim=1):
    axis_maximums = data.max(dim, keepdim=True)[0]
    return ((data - axis_maximums) * mask).min(dim, keepdim=True)[0] + axis_maximums


def _masked_maximum(data, mask, dim=1):
    axis_minimums = data.min(dim, keepdim=True)[0]
    return ((data - axis_minimums) * mask).max(dim, keepdim=True)[0] + axis_minimums


def batch_triplet_mining_torch(d: torch.Tensor, labels: torch.Tensor, kind: int, margin: float) -> torch.Tensor:
    """The mining of the four losses in sentence-transformers' tensor formulation, on a distance matrix d [B, B] that is
    already there: what a `distance_metric` the kernels do not know is followed by."""
    labels = labels.view(-1)
    B = labels.numel()
    same = labels.unsqueeze(0) == labels.unsqueeze(1)
    eye = torch.eye(B, dtype=torch.bool, device=d.device)
    pos, neg = (same & ~eye).to(d.dtype), (~same).to(d.dtype)
    if kind in (BT_HARD, BT_HARD_SOFT):
        hardest_positive = (pos * d).max(1, keepdim=True)[0]
        hardest_negative = (d + d.max(1, keepdim=True)[0] * (1.0 - neg)).min(1, keepdim=True)[0]
        if kind == BT_HARD_SOFT:
            return torch.log1p(torch.exp(hardest_positive - hardest_negative)).mean()
        return torch.relu(hardest_positive - hardest_negative + margin).mean()
    if kind == BT_ALL:
        t = d.unsqueeze(2) - d.unsqueeze(1) + margin
        t = torch.relu((pos.unsqueeze(2) * neg.unsqueeze(1)) * t)
        return t.sum() / ((t > 1e-16).sum().to(d.dtype) + 1e-16)
    if kind != BT_SEMIHARD:
        raise ValueError(f"kind is one of BT_HARD, BT_HARD_SOFT, BT_SEMIHARD, BT_ALL (0 .. 3), {kind!r} given")
    tile = d.repeat(B, 1)                                           # row j * B + i holds d[i, :]
    mask = (~same).repeat(B, 1) & (tile > d.t().reshape(-1, 1))     # ... and asks for the negatives farther than d[i, j]
    mask_final = (mask.sum(1, keepdim=True) > 0).reshape(B, B).t()
    negatives_outside = _masked_minimum(tile, mask.to(d.dtype)).reshape(B, B).t()
    negatives_inside = _masked_maximum(d, neg).repeat(1, B)
    semi_hard_negatives = torch.where(mask_final, negatives_outside, negatives_inside)
    loss_mat = d - semi_hard_negatives + margin
    return torch.relu(loss_mat * pos).sum() / pos.sum()


class _BatchTripletLoss(_TupleLoss):
    reduction = "mean"
    _kind = BT_HARD

    def __init__(self, model, distance_metric=BatchHardTripletLossDistanceFunction.eucledian_distance, margin: float = 5,
                 fused: bool = True):
        super().__init__(model, fused)
        self.distance_metric = distance_metric
        self.triplet_margin = margin

    def forward(self, sentence_features: Iterable[Dict[str, torch.Tensor]], labels: torch.Tensor) -> torch.Tensor:
        (rep,) = self._embed(sentence_features, 1)
        return self._loss(labels, rep)

    def _loss(self, labels: torch.Tensor, embeddings: torch.Tensor) -> torch.Tensor:
        code = getattr(self.distance_metric, "_qst_metric", None)
        if code is not None:
            return batch_triplet_loss(embeddings, labels, self._kind, code, self.triplet_margin)
        return batch_triplet_mining_torch(self.distance_metric(embeddings), labels, self._kind, self.triplet_margin)


class BatchHardTripletLoss(_BatchTripletLoss):
    """mean over the anchors of relu(hardest positive - hardest negative + margin): per anchor the farthest row of its own
    label and the closest row of another, mined among the rows of the batch (one text column, integer class labels)."""
    _kind = BT_HARD

    def batch_hard_triplet_loss(self, labels: torch.Tensor, embeddings: torch.Tensor) -> torch.Tensor:
        return self._loss(labels, embeddings)


class BatchHardSoftMarginTripletLoss(_BatchTripletLoss):
    """BatchHardTripletLoss with the soft margin log1p(exp(hardest positive - hardest negative)) in place of the hinge."""
    _kind = BT_HARD_SOFT

    def __init__(self, model, distance_metric=BatchHardTripletLossDistanceFunction.eucledian_distance, fused: bool = True):
        super().__init__(model, distance_metric, 0.0, fused)

    def batch_hard_triplet_soft_margin_loss(self, labels: torch.Tensor, embeddings: torch.Tensor) -> torch.Tensor:
        return self._loss(labels, embeddings)


class BatchSemiHardTripletLoss(_BatchTripletLoss):
    """Per pair (anchor, positive) the closest negative that is farther away than the positive; if there is none, the
    farthest negative. Mean over the pairs of relu(d(a, p) - d(a, n) + margin). A batch in which no label occurs twice has
    no pair and gives NaN, as in sentence-transformers: feed it from SentenceLabelDataset."""
    _kind = BT_SEMIHARD

    def batch_semi_hard_triplet_loss(self, labels: torch.Tensor, embeddings: torch.Tensor) -> torch.Tensor:
        return self._loss(labels, embeddings)


class BatchAllTripletLoss(_BatchTripletLoss):
    """relu(d(a, p) - d(a, n) + margin) over every valid triplet of the batch, averaged over those that are positive."""
    _kind = BT_ALL

    def batch_all_triplet_loss(self, labels: torch.Tensor, embeddings: torch.Tensor) -> torch.Tensor:
        return self._loss(labels, embeddings)


# ------------------------------------------------------------------ distillation from a teacher
class MSELoss(_TupleLoss):
    """nn.MSELoss() between the student's embedding of the one text column and `labels`, the teacher's embedding of each
    example [B, D]: one qst_embed_mse call. The teacher and the student must have the same embedding width; where they
    differ, the model carries a models.Dense behind its pooling (a trained projection, or the teacher's PCA), as
    sentence-transformers users do."""
    reduction = "mean"

    def __init__(self, model):
        super().__init__(model, True)

    def forward(self, sentence_features: Iterable[Dict[str, torch.Tensor]], labels: torch.Tensor) -> torch.Tensor:
        cols = list(sentence_features)
        rep = self.model(cols[0])["sentence_embedding"]
        if labels.dim() != 2 or labels.shape != rep.shape:
            raise ValueError(f"MSELoss: the labels are the teacher's embeddings, shape {tuple(rep.shape)} like the student's; "
                             f"{tuple(labels.shape)} given")
        return embed_mse(rep, labels)


def _list_operands(reps: List[torch.Tensor]):
    """(query [B, D], candidates [K, B, D]) of the embedded text columns, as qst_listwise_distill_loss takes them. The columns
    of one fused pass are the row blocks of one [(1 + K) * B, D] buffer (encode_columns_fused splits it), and the candidates
    are then a view of its rows from B on; columns embedded one by one are stacked."""
    q, cands = reps[0], reps[1:]
    B, D = q.shape
    whole = getattr(q, "_base", None)
    if (whole is not None and whole.dim() == 2 and tuple(whole.shape) == (len(reps) * B, D) and whole.is_contiguous()
            and all(r._base is whole and tuple(r.shape) == (B, D) and r.is_contiguous()
                    and r.storage_offset() == whole.storage_offset() + k * B * D for k, r in enumerate(reps))):
        return q, whole[B:].view(len(cands), B, D)
    return q, torch.stack(cands, 0)


def _require_list_labels(what: str, labels: torch.Tensor, want: tuple, n_cols: int) -> None:
    if tuple(labels.shape) != want:
        raise ValueError(f"{what}: with {n_cols} text columns the labels have the shape {want}; "
                         f"{tuple(labels.shape)} given")


class MarginMSELoss(_TupleLoss):
    """mean over the batch of (similarity_fct(query, positive) - similarity_fct(query, negative) - label)^2, the label
    being the teacher's (usually a cross-encoder's) margin score(query, positive) - score(query, negative). With
    `util.pairwise_dot_score` or `util.pairwise_cos_sim` one qst_margin_mse_loss call; any other callable
    `f(a, b) -> [B]` is called on the embeddings as given and the squared error runs in torch.
    With four or more text columns (query, positive, negatives ...; sentence-transformers 3.x) the labels are [B, K - 1],
    the teacher's margin against each negative, and the loss is nn.MSELoss() over all of them: one
    qst_listwise_distill_loss call (csrc/listwise.hip) for the two similarities above and up to 64 candidates, the stacked
    `similarity_fct` differences in torch otherwise."""
    reduction = "mean"

    def __init__(self, model, similarity_fct=util.pairwise_dot_score, fused: bool = True):
        super().__init__(model, fused)
        self.similarity_fct = similarity_fct

    def _kernel_sim(self) -> Optional[int]:
        if self.similarity_fct is util.pairwise_dot_score:
            return METRIC_DOT
        if self.similarity_fct is util.pairwise_cos_sim:
            return METRIC_COS_SIM
        return None

    def forward(self, sentence_features: Iterable[Dict[str, torch.Tensor]], labels: torch.Tensor) -> torch.Tensor:
        cols = list(sentence_features)
        if len(cols) > 3:
            return self._forward_list(cols, labels)
        q, p, n = self._embed(cols, 3)
        sim = self._kernel_sim()
        if sim is not None:
            return margin_mse(q, p, n, labels.view(-1), sim, "mean")
        margin = self.similarity_fct(q, p) - self.similarity_fct(q, n)
        return torch.nn.functional.mse_loss(margin, labels.view(-1).to(margin.dtype))

    def _forward_list(self, cols: List[Dict[str, torch.Tensor]], labels: torch.Tensor) -> torch.Tensor:
        reps = self._embed(cols, len(cols))
        K = len(reps) - 1
        _require_list_labels(type(self).__name__, labels, (reps[0].shape[0], K - 1), len(cols))
        sim = self._kernel_sim()
        if sim is not None and K <= LISTWISE_MAX_K:
            return listwise_distill(*_list_operands(reps), labels, LISTWISE_MARGIN_MSE, sim, 1.0, "mean")
        pos = self.similarity_fct(reps[0], reps[1])
        margins = torch.stack([pos - self.similarity_fct(reps[0], n) for n in reps[2:]], dim=1)
        return torch.nn.functional.mse_loss(margins, labels.to(margins.dtype))


class DistillKLDivLoss(_TupleLoss):
    """sentence-transformers' DistillKLDivLoss (3.4): temperature^2 * KLDivLoss(batchmean) between the teacher's softmax over
    the K candidates of a query and the student's, both at `temperature`. Two or more text columns (query, positive,
    negatives ...) and labels [B, K], the teacher's (usually a cross-encoder's) score of every candidate. With
    `util.pairwise_dot_score` (the default) or `util.pairwise_cos_sim`, recognised by identity, and up to 64 candidates the K
    similarities, both softmaxes, the divergence and every gradient are one qst_listwise_distill_loss call
    (csrc/listwise.hip); any other callable `f(a, b) -> [B]` is called once per candidate on the embeddings as given and
    sentence-transformers' composition runs in torch on the stacked result."""
    reduction = "mean"

    def __init__(self, model, similarity_fct=util.pairwise_dot_score, temperature: float = 1.0, fused: bool = True):
        super().__init__(model, fused)
        self.similarity_fct = similarity_fct
        self.temperature = temperature

    def get_config_dict(self):
        return {"similarity_fct": self.similarity_fct.__name__, "temperature": self.temperature}

    def _kernel_sim(self) -> Optional[int]:
        if self.similarity_fct is util.pairwise_dot_score:
            return METRIC_DOT
        if self.similarity_fct is util.pairwise_cos_sim:
            return METRIC_COS_SIM
        return None

    def forward(self, sentence_features: Iterable[Dict[str, torch.Tensor]], labels: torch.Tensor) -> torch.Tensor:
        cols = list(sentence_features)
        if len(cols) < 2:
            raise ValueError(f"{type(self).__name__} takes 2 or more text columns per example, {len(cols)} given")
        reps = self._embed(cols, len(cols))
        K = len(reps) - 1
        _require_list_labels(type(self).__name__, labels, (reps[0].shape[0], K), len(cols))
        sim = self._kernel_sim()
        if sim is not None and K <= LISTWISE_MAX_K:
            return listwise_distill(*_list_operands(reps), labels, LISTWISE_KL, sim, self.temperature, "mean")
        T = self.temperature
        scores = torch.stack([self.similarity_fct(reps[0], d) for d in reps[1:]], dim=1) / T
        student = torch.log_softmax(scores, dim=1)
        teacher = torch.softmax(labels.to(scores.dtype) / T, dim=1)
        return nn.KLDivLoss(reduction="batchmean")(student, teacher) * (T ** 2)


# ------------------------------------------------------------------ pairwise ranking of graded pairs
class CoSENTLoss(_TupleLoss):
    """sentence-transformers' CoSENTLoss: log(1 + sum exp(scale * (s_i - s_j))) over the pairs of the batch in which example
    i has the smaller label, s = similarity_fct(u, v) -- every pair the model ranks against its labels costs, so the loss
    optimises the order EmbeddingSimilarityEvaluator's Spearman correlation scores. Two text columns and a graded label.
    With `util.pairwise_cos_sim` (the default) or `util.pairwise_angle_sim`, recognised by identity, scores, loss and both
    gradients are one qst_cosent_loss call (csrc/cosent.hip) in O(B) memory; any other callable is called as
    `similarity_fct(u, v) -> [B]` and sentence-transformers' B x B composition runs in torch on its result."""
    reduction = "mean"

    def __init__(self, model, scale: float = 20.0, similarity_fct=util.pairwise_cos_sim, fused: bool = True):
        super().__init__(model, fused)
        self.scale = scale
        self.similarity_fct = similarity_fct

    def get_config_dict(self):
        return {"scale": self.scale, "similarity_fct": self.similarity_fct.__name__}

    def _kernel_sim(self) -> Optional[str]:
        if self.similarity_fct is util.pairwise_cos_sim:
            return "cos"
        if self.similarity_fct is util.pairwise_angle_sim:
            return "angle"
        return None

    def forward(self, sentence_features: Iterable[Dict[str, torch.Tensor]], labels: torch.Tensor) -> torch.Tensor:
        u, v = self._embed(sentence_features, 2)
        y = labels.view(-1).to(torch.float32)
        sim = self._kernel_sim()
        if sim == "angle" and u.shape[1] % 2:
            raise ValueError(f"{type(self).__name__}: the angle similarity splits each embedding into two halves: the "
                             f"width {u.shape[1]} is odd")
        if sim is not None:
            return cosent_loss(u, v, y, self.scale, sim)
        return cosent_loss_torch(self.similarity_fct(u, v), y, self.scale)


class AnglELoss(CoSENTLoss):
    """sentence-transformers' AnglELoss: CoSENTLoss on `util.pairwise_angle_sim`, the angle difference of the embeddings read
    as complex numbers, which does not flatten out near +-1 as the cosine does. The embedding width must be even."""

    def __init__(self, model, scale: float = 20.0, fused: bool = True):
        super().__init__(model, scale, util.pairwise_angle_sim, fused)


# ------------------------------------------------------------------ SoftmaxLoss: a classifier the loss owns and trains
SOFTMAX_REP, SOFTMAX_DIFF, SOFTMAX_MULT = 1, 2, 4          # QST_SOFTMAX_*: the parts of the classifier's input
_HEAD_MAX_C, _HEAD_MAX_D = 8, 2048


def softmax_head_supported(D: int, C: int, parts: int) -> bool:
    """Whether qst_softmax_head_fwd / _bwd take this shape (include/qst.h)."""
    return 1 <= C <= _HEAD_MAX_C and D % 4 == 0 and 4 <= D <= _HEAD_MAX_D and 1 <= parts <= 7


def softmax_head_fwd_raw(u, v, w, b, parts: int) -> torch.Tensor:
    """qst_softmax_head_fwd on contiguous fp32 HIP tensors u, v [B, D], w [C, K], b [C]: the logits [B, C]."""
    lib = _lib.load()
    (B, D), C = u.shape, w.shape[0]
    logits = torch.empty(B, C, dtype=torch.float32, device=u.device)
    with torch.cuda.device(u.device):
        _lib.check(lib.qst_softmax_head_fwd(u.data_ptr(), v.data_ptr(), w.data_ptr(), b.data_ptr(), B, D, C, int(parts),
                                            logits.data_ptr(), _lib.current_stream_ptr()), "qst_softmax_head_fwd")
    return logits


def softmax_head_bwd_raw(u, v, w, dlogits, parts: int):
    """qst_softmax_head_bwd: (grad_u, grad_v [B, D], grad_w [C, K], grad_b [C]) from dlogits [B, C]."""
    lib = _lib.load()
    (B, D), C = u.shape, w.shape[0]
    gu, gv = _grad_slabs(2, u, True)
    gw = torch.empty_like(w)
    gb = torch.empty(C, dtype=torch.float32, device=u.device)
    nbytes = int(lib.qst_softmax_head_bwd_workspace_bytes(B, D, C, int(parts)))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=u.device)
    with torch.cuda.device(u.device):
        _lib.check(lib.qst_softmax_head_bwd(u.data_ptr(), v.data_ptr(), w.data_ptr(), dlogits.data_ptr(), B, D, C, int(parts),
                                            gu.data_ptr(), gv.data_ptr(), gw.data_ptr(), gb.data_ptr(), ws.data_ptr(), nbytes,
                                            _lib.current_stream_ptr()), "qst_softmax_head_bwd")
    return gu, gv, gw, gb


def softmax_ce_raw(logits, labels, reduction: int = 2, ignore_index: int = -100, grad_out: Optional[torch.Tensor] = None,
                   want_grads: bool = False, want_counts: bool = False):
    """qst_softmax_ce on contiguous fp32 logits [B, C] and int64 labels [B] (HIP): (loss [B] or [1], dlogits [B, C] or None,
    counts int64 [2] = {rows with a label in range, rows whose argmax is the label} or None)."""
    lib = _lib.load()
    B, C = logits.shape
    out = torch.empty(B if reduction == 0 else 1, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits) if want_grads else None
    counts = torch.empty(2, dtype=torch.int64, device=logits.device) if want_counts else None
    scratch = torch.empty(B + 2, dtype=torch.float32, device=logits.device)
    with torch.cuda.device(logits.device):
        _lib.check(lib.qst_softmax_ce(logits.data_ptr(), labels.data_ptr(), B, C, int(ignore_index), int(reduction),
                                      out.data_ptr(), _lib.ptr(grad_out), _lib.ptr(dlogits), _lib.ptr(counts),
                                      scratch.data_ptr(), _lib.current_stream_ptr()), "qst_softmax_ce")
    return out, dlogits, counts


BINARY_EVAL_MAX_PAIRS, BINARY_EVAL_MAX_SETS = 1 << 20, 8       # qst_binary_eval's limits (include/qst.h)


def binary_eval_raw(scores, labels, high_flags) -> torch.Tensor:
    """qst_binary_eval on contiguous fp32 HIP scores [nsets, n], contiguous int64 HIP labels [n] in {0, 1} and one flag per
    set (true: a higher score is more similar): float64 [nsets, 8] on the device, per set {accuracy, accuracy_threshold, f1,
    precision, recall, f1_threshold, ap, number of positives}. No host synchronisation."""
    lib = _lib.load()
    nsets, n = scores.shape
    high_flags = list(high_flags)
    if nsets < 1 or n < 1 or len(high_flags) != nsets or labels.numel() != n:
        raise ValueError(f"binary_eval: scores {tuple(scores.shape)} need at least one row and one pair, {nsets} flags and "
                         f"{n} labels; {len(high_flags)} flags and {labels.numel()} labels given")
    flags = (_lib.C.c_int32 * nsets)(*[int(bool(f)) for f in high_flags])
    if n > BINARY_EVAL_MAX_PAIRS or nsets > BINARY_EVAL_MAX_SETS:
        raise _lib.QstError(f"binary_eval: {n} pairs in {nsets} score rows; the kernel takes up to {BINARY_EVAL_MAX_PAIRS} "
                            f"(2^20) pairs and {BINARY_EVAL_MAX_SETS} rows")
    out = torch.empty(nsets, 8, dtype=torch.float64, device=scores.device)
    nbytes = int(lib.qst_binary_eval_workspace_bytes(n, nsets))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=scores.device)
    with torch.cuda.device(scores.device):
        _lib.check(lib.qst_binary_eval(scores.data_ptr(), labels.data_ptr(), n, nsets, flags, out.data_ptr(), ws.data_ptr(),
                                       nbytes, _lib.current_stream_ptr()), "qst_binary_eval")
    return out


class _SoftmaxHeadFn(torch.autograd.Function):
    """logits = classifier([u, v, |u - v|, u * v]): qst_softmax_head_fwd, and qst_softmax_head_bwd from autograd's dlogits."""

    @staticmethod
    def forward(ctx, u, v, w, b, parts):
        xs = _f32((u, v, w, b))
        logits = softmax_head_fwd_raw(*xs, parts)
        ctx.save_for_backward(*xs[:3])
        ctx.parts, ctx.in_dtypes = parts, (u.dtype, v.dtype, w.dtype, b.dtype)
        return logits

    @staticmethod
    def backward(ctx, grad_logits):
        u, v, w = ctx.saved_tensors
        grads = softmax_head_bwd_raw(u, v, w, grad_logits.detach().to(torch.float32).contiguous(), ctx.parts)
        return (*[g.to(dt) for g, dt in zip(grads, ctx.in_dtypes)], None)


class _SoftmaxLossFn(torch.autograd.Function):
    """nn.CrossEntropyLoss()(classifier([u, v, |u - v|, u * v]), labels): forward = qst_softmax_head_fwd + qst_softmax_ce,
    backward = qst_softmax_ce (dlogits, times the upstream scalar on the device) + qst_softmax_head_bwd."""

    @staticmethod
    def forward(ctx, u, v, w, b, labels, parts, ignore_index):
        xs = _f32((u, v, w, b))
        y = labels.detach().to(torch.int64).contiguous().reshape(-1)
        logits = softmax_head_fwd_raw(*xs, parts)
        out, _, _ = softmax_ce_raw(logits, y, _RED_CODE["mean"], ignore_index)
        ctx.save_for_backward(*xs[:3], logits, y)
        ctx.hp, ctx.in_dtypes = (parts, ignore_index), (u.dtype, v.dtype, w.dtype, b.dtype)
        return out.reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        u, v, w, logits, y = ctx.saved_tensors
        parts, ignore_index = ctx.hp
        _, dlogits, _ = softmax_ce_raw(logits, y, _RED_CODE["mean"], ignore_index, grad_out=_upstream(grad_output),
                                       want_grads=True)
        grads = softmax_head_bwd_raw(u, v, w, dlogits, parts)
        return (*[g.to(dt) for g, dt in zip(grads, ctx.in_dtypes)], None, None, None)


def label_counts(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """int64 [2] on the device: {rows whose label is in [0, C), rows among them whose largest logit is the label's} of logits
    [B, C] and integer labels [B] (HIP tensors). One forward-only qst_softmax_ce call; among equal logits the lowest index
    is the prediction, as torch.argmax returns it."""
    if logits.dim() != 2 or labels.numel() != logits.shape[0]:
        raise ValueError(f"label_counts: logits {tuple(logits.shape)} need one label per row, {labels.numel()} given")
    _require_rows("label_counts", logits)
    _require_labels("label_counts", labels, logits.shape[0])
    (z,) = _f32((logits,))
    y = labels.detach().to(torch.int64).contiguous().reshape(-1)
    return softmax_ce_raw(z, y, _RED_CODE["mean"], want_counts=True)[2]


class SoftmaxLoss(_TupleLoss):
    """sentence-transformers 2.2.2's SoftmaxLoss, the NLI objective: loss_fct(classifier(cat(parts)), labels) with the parts
    u, v (concatenation_sent_rep), |u - v| (concatenation_sent_difference), u * v (concatenation_sent_multiplication) of the two
    sentence embeddings, in that order. `classifier` is an nn.Linear built as sentence-transformers builds it (the same
    torch.manual_seed gives the same initial weights) whose parameters live in a loss_params.LossParameters: fit() finds it
    through owned_parameters() and clips and steps it together with the encoder. Its state_dict keys are classifier.weight
    and classifier.bias; save() and the checkpoints of fit() hold the encoder only, as in sentence-transformers.

    With a default-configured nn.CrossEntropyLoss (mean, no class weights, no label smoothing; any ignore_index) the logits,
    the cross entropy and the gradients for u, v, weight and bias are qst_softmax_head_fwd / qst_softmax_ce /
    qst_softmax_head_bwd (csrc/softmax_head.hip), fp32. Any other loss_fct is called in torch on the kernels' logits. A shape
    the kernels do not take (more than 8 labels, an embedding width that is no multiple of 4 or above 2048) runs as torch
    ops on the same parameter views. forward(sentence_features, labels=None) returns (reps, logits), as 2.2.2 does."""
    reduction = "mean"

    def __init__(self, model, sentence_embedding_dimension: int, num_labels: int, concatenation_sent_rep: bool = True,
                 concatenation_sent_difference: bool = True, concatenation_sent_multiplication: bool = False,
                 loss_fct=nn.CrossEntropyLoss(), fused: bool = True):
        super().__init__(model, fused)
        self.num_labels = num_labels
        self.concatenation_sent_rep = concatenation_sent_rep
        self.concatenation_sent_difference = concatenation_sent_difference
        self.concatenation_sent_multiplication = concatenation_sent_multiplication
        num_vectors_concatenated = 0
        if concatenation_sent_rep:
            num_vectors_concatenated += 2
        if concatenation_sent_difference:
            num_vectors_concatenated += 1
        if concatenation_sent_multiplication:
            num_vectors_concatenated += 1
        if num_vectors_concatenated == 0:
            raise ValueError("SoftmaxLoss: at least one of the three concatenation flags must be set")
        self.classifier = nn.Linear(num_vectors_concatenated * sentence_embedding_dimension, num_labels)
        self.loss_fct = loss_fct
        self.sentence_embedding_dimension = sentence_embedding_dimension
        self._parts = (SOFTMAX_REP if concatenation_sent_rep else 0) | (SOFTMAX_DIFF if concatenation_sent_difference else 0) \
            | (SOFTMAX_MULT if concatenation_sent_multiplication else 0)
        self._owned = LossParameters(self.classifier, device=_device_of(model))

    def owned_parameters(self) -> "LossParameters":
        return self._owned

    def _default_ce(self) -> bool:
        f = self.loss_fct
        return type(f) is nn.CrossEntropyLoss and f.weight is None and f.reduction == "mean" \
            and getattr(f, "label_smoothing", 0.0) == 0.0

    def _features(self, u, v):
        parts = []
        if self.concatenation_sent_rep:
            parts += [u, v]
        if self.concatenation_sent_difference:
            parts.append(torch.abs(u - v))
        if self.concatenation_sent_multiplication:
            parts.append(u * v)
        return torch.cat(parts, 1)

    def forward(self, sentence_features: Iterable[Dict[str, torch.Tensor]], labels: torch.Tensor = None):
        self._owned.ensure()
        u, v = self._embed(sentence_features, 2)
        w, b = self.classifier.weight, self.classifier.bias
        kernels = u.is_cuda and w.device == u.device and softmax_head_supported(u.shape[1], self.num_labels, self._parts)
        if labels is not None and kernels and self._default_ce():
            _require_labels("SoftmaxLoss", labels, u.shape[0])
            return _SoftmaxLossFn.apply(u, v, w, b, labels.view(-1), self._parts, int(self.loss_fct.ignore_index))
        if kernels:
            output = _SoftmaxHeadFn.apply(u, v, w, b, self._parts)
        else:
            output = torch.nn.functional.linear(self._features(u, v), w, b)
        if labels is None:
            return [u, v], output
        return self.loss_fct(output, labels.view(-1))


# ------------------------------------------------------------------ Matryoshka: one encoder pass scored at nested widths
def _full_embedding_width(model) -> Optional[int]:
    """The untruncated width of the model's sentence embeddings (training is never truncated); None for a stand-in that
    cannot say."""
    get = getattr(model, "get_sentence_embedding_dimension", None)
    if get is None:
        return None
    cut = getattr(model, "truncate_sentence_embeddings", None)
    if cut is None:
        return int(get())
    with cut(None):
        return int(get())


class MatryoshkaLoss(nn.Module):
    """sentence-transformers' MatryoshkaLoss: sum_k matryoshka_weights[k] * loss on the embeddings cut to their first
    matryoshka_dims[k] columns and normalised again, from ONE encoder pass -- the trained model can then be cut to any of
    those widths (SentenceTransformer(truncate_dim=...), model.truncate_sentence_embeddings(d)).

    `loss` is any of this module's objectives that take their embeddings through `_TupleLoss._embed`. Over
    `MultipleNegativesRankingLoss` or its symmetric form with `util.cos_sim` or `util.dot_score` (the same scores once the
    prefix is normalised), up to 8 widths and `fused_dims=True`, all widths are ONE qst_mnrl_nested_loss call
    (csrc/mnrl_nested.hip) forward and one backward, whatever their number. Anything else -- another base loss, a foreign
    `similarity_fct`, more than 8 widths, `fused_dims=False` -- runs the base loss's own forward once per width on
    F.normalize(rep[:, :d], p=2, dim=1) in torch ops, and autograd sums the gradients. `labels` pass through unchanged.
    `n_dims_per_step` = n with 0 < n < K scores `random.sample` of n of the widths per forward, as sentence-transformers does.
    `SoftmaxLoss` (its classifier has a fixed input width) and `MSELoss` (the teacher's vectors have the full width) are
    refused."""

    def __init__(self, model, loss, matryoshka_dims, matryoshka_weights=None, n_dims_per_step: int = -1,
                 fused_dims: bool = True):
        super().__init__()
        if not isinstance(loss, _TupleLoss):
            raise TypeError(f"MatryoshkaLoss wraps a loss of this package that embeds through _TupleLoss._embed; "
                            f"{type(loss).__name__} does not derive from _TupleLoss")
        if isinstance(loss, SoftmaxLoss):
            raise ValueError("MatryoshkaLoss cannot wrap SoftmaxLoss: its classifier has a fixed input width")
        if isinstance(loss, MSELoss):
            raise ValueError("MatryoshkaLoss cannot wrap MSELoss: the teacher's vectors have the full width")
        if getattr(loss, "_replays_mini_batches", False):       # the cached in-batch-negatives losses, GIST's included
            raise ValueError(f"MatryoshkaLoss cannot wrap {type(loss).__name__} yet: the cached losses embed in mini-batches "
                             f"and replay them in backward(), and the per-width losses are not part of that replay")
        dims = [int(d) for d in matryoshka_dims]
        if not dims:
            raise ValueError("matryoshka_dims is empty")
        if len(set(dims)) != len(dims):
            raise ValueError(f"matryoshka_dims repeats a width: {dims}")
        if min(dims) < 1:
            raise ValueError(f"matryoshka_dims must be positive: {dims}")
        weights = [1.0] * len(dims) if matryoshka_weights is None else [float(w) for w in matryoshka_weights]
        if len(weights) != len(dims):
            raise ValueError(f"matryoshka_weights has {len(weights)} entries for {len(dims)} matryoshka_dims")
        full = _full_embedding_width(model)
        if full is not None and max(dims) > full:
            raise ValueError(f"matryoshka_dims {dims}: {max(dims)} is larger than the model's embedding dimension {full}")
        self.model = model
        self.loss = loss
        self.matryoshka_dims = dims
        self.matryoshka_weights = weights
        self.n_dims_per_step = n_dims_per_step
        self.fused_dims = fused_dims

    @property
    def reduction(self) -> str:
        red = getattr(self.loss, "reduction", "mean")
        return red if isinstance(red, str) else "mean"

    def get_config_dict(self):
        return {"loss": type(self.loss).__name__, "matryoshka_dims": self.matryoshka_dims,
                "matryoshka_weights": self.matryoshka_weights, "n_dims_per_step": self.n_dims_per_step}

    def _step_indices(self) -> List[int]:
        idx = range(len(self.matryoshka_dims))
        if 0 < self.n_dims_per_step < len(idx):
            import random
            return random.sample(idx, self.n_dims_per_step)
        return list(idx)

    def _one_call(self, K: int) -> bool:
        return self.fused_dims and K <= NESTED_MAX_DIMS and type(self.loss) in (
            MultipleNegativesRankingLoss, MultipleNegativesSymmetricRankingLoss) and self.loss._kernel_sim() is not None

    def forward(self, sentence_features: Iterable[Dict[str, torch.Tensor]], labels: torch.Tensor = None) -> torch.Tensor:
        base = self.loss
        idx = self._step_indices()
        dims = [self.matryoshka_dims[i] for i in idx]
        weights = [self.matryoshka_weights[i] for i in idx]
        cols = list(sentence_features)
        if self._one_call(len(dims)):
            if len(cols) < 2:
                raise ValueError(f"{type(base).__name__} takes 2 or more text columns per example, {len(cols)} given")
            reps = base._embed(cols, len(cols))
            c = reps[1] if len(reps) == 2 else torch.cat(reps[1:], 0)
            return matryoshka_mnrl_loss(reps[0], c, dims, weights, base.scale, base._symmetric)

        # the base loss's own forward per width, its _embed answering with the cut and renormalised embeddings of one pass
        embed, state = base._embed, {"reps": None, "d": None}
        shadowed = base.__dict__.get("_embed")

        def answer(features, k):
            if state["reps"] is None:
                state["reps"] = embed(features, k)
            if any(state["d"] > r.shape[1] for r in state["reps"]):
                raise ValueError(f"matryoshka width {state['d']} is larger than the embedding width "
                                 f"{state['reps'][0].shape[1]}")
            return [torch.nn.functional.normalize(r[:, :state["d"]], p=2, dim=1) for r in state["reps"]]

        base._embed = answer
        try:
            total = None
            for d, w in zip(dims, weights):
                state["d"] = d
                term = base(cols, labels) * w
                total = term if total is None else total + term
        finally:
            if shadowed is None:
                del base._embed
            else:
                base._embed = shadowed
        return total
