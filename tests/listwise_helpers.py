"""The yardstick and the a-priori bounds of the listwise distillation objectives (tests/test_gpu_listwise.py,
tests/test_listwise_host.py, tools/listwise_bench.py): sentence-transformers' DistillKLDivLoss and MarginMSELoss with several
negatives written in torch ops, in whatever dtype and on whatever device the inputs have -- fp64 on the CPU with autograd for
the kernel tests, fp32 on the GPU as the torch-op path the loss classes are compared with. Imported like distill_helpers,
not a conftest.

Layout everywhere: q [B, D], docs [K, B, D] with candidate 0 the positive, labels [B, K] (KL) or [B, K - 1] (margin).

The bounds (every one absolute, in fp64, from the fp64 yardstick's own quantities; U = 2^-24)
---------------------------------------------------------------------------------------------
Scores.  dS[b, j] = distill_helpers.sim_bound(q, docs[j], sim): the summation bound of an fp32 dot product for the dot
score, the project's tolerance of a cosine for the cosine.

KL kind.  The kernel forms s = sim / T (one rounding), so |s^ - s| <= a = dS / T + U |s|, and A = max_j a_j. log_softmax is
1-Lipschitz in the sup norm twice over (the entry itself and the logsumexp), hence |log_softmax(s^) - log_softmax(s)| <= 2 A:
twice the largest score error divided by T. What fp32 adds on the way, with R = max s - min s + 2 A the range of the
shifted scores x = s^ - max s^ (so |x| <= R) and Z = sum exp(x) in [1, K]:
    U R                 the subtraction of the maximum (the maximum itself is exact)
    (R + 4) U           exp: its argument is off by U |x| <= U R, which is a relative error of exp(x), and expf's own
                        rounding is within 2 ulp = 4 U; every term of Z is positive, so Z inherits the largest of these
    6 U                 the additions of the wave tree over 64 lanes (four DPP steps, two levels over the four totals)
    4 U log K           logf's own rounding, 2 ulp of log Z <= log K (the relative error of Z enters log Z absolutely: above)
    U (R + log K)       the final subtraction x - log Z
    2 U                 second-order terms
  = softmax_log_slack(R, K) = U (3 R + 5 log K + 12), and E = 2 A + softmax_log_slack(R, K) bounds log_softmax's error. The
teacher's side is the same with a = U |labels / T| (the division's rounding: the yardstick divides the same fp32 labels in
double). The probabilities exp(x) / Z carry the same ingredients and a division in place of the subtraction, so their
RELATIVE error is at most expm1(E + 2 U), plus 2^-120 absolute for a quotient that leaves the normal range (a teacher weight
that underflows to exactly 0 is such a one: its term is then exactly 0, and the yardstick's is below 2^-120 |log t - log p|).
With d = log t - log p, E_d = E_t + E_p + U |d| and dt the teacher weight's bound, a term t d is off by at most
    t E_d + |d| dt + dt E_d + U t |d|
(the last for the product's rounding); the row adds the 64 lanes' terms (6 U sum |t d|) and is multiplied by T * T (2 U).
g = d row / d sim_j = T (p - t) is off by T (dp + dt) + 2 U |g| (the subtraction and the product).

Margin kind.  As distill_helpers.margin_bounds per negative: m_j = S_0 - S_j within dS_0 + dS_j + U |m_j|, the residual
e_j = m_j - y_j one rounding more, its square 2 |e| de + de^2 + U (|e| + de)^2, the row's sum 6 U sum (|e| + de)^2.
g_j = -2 e_j (exact doubling) within 2 de_j; g_0 = sum_j 2 e_j within their sum and the tree's 6 U sum 2 (|e| + de).

Reductions.  'mean' divides g once more (U |c|); the row values go through the second stage in double (nothing to add) and
the result is rounded to fp32 once (distill_helpers.reduced_bound, with the divisor B or B (K - 1)).

Gradients.  With c = g [/ divisor] within dc and W = |grad_out| of the row (the last multiplication is one more rounding):
  dot     grad_docs_j = c_j q:              (dc_j + 2 U (|c_j| + dc_j)) |q_e| W
          grad_q = sum_j c_j docs_j:        (sum_j dc_j |d_je| + (K + 3) U sum_j (|c_j| + dc_j) |d_je|) W -- K additions in a
                                            lane's chain, each within U of the partial sum, the products, the last factor
  cosine  d sim / d d = kxy q + kyy d, d sim / d q = kxy d + kxx q with kxy = 1 / (|q| |d|), kyy = -cos / |d|^2,
          kxx = -cos / |q|^2. A norm is the square root of an all-positive sum: (D / 128 + 8) U = rn relative (half the
          sum's (D / 64 + 11) U, the root's rounding, second order). kxy is within rxy = 2 rn + 2 U relative, kyy within
          dS / |d|^2 + |cos| / |d|^2 (2 rn + 3 U) absolute, kxx likewise. Then cxy = c kxy, cyy = c kyy and
          cq = sum_j c_j kxx_j (a wave tree) follow by the product rule, and
          grad_docs_j = cxy_j q + cyy_j d_j:        (dcxy |q_e| + dcyy |d_e| + 3 U (|cxy q_e| + |cyy d_e|)) W
          grad_q = sum_j cxy_j d_j + cq q:          (sum_j dcxy_j |d_je| + dcq |q_e| + (K + 4) U (sum_j |cxy_j d_je| + |cq q_e|)) W
          with |cxy|, |cyy|, |cq| taken at their bounds. A row whose norm is at or below the clamp (a zero row) is the one
          exception the project already makes (test_margin_mse_cosine_with_zero_rows): torch's gradients there are O(1 / eps),
          the kernel passes none through the norm, and the gradients of that example must only be finite.
There is no free tolerance: every element of every output is compared against its own bound.
"""
import functools
import math

import torch
import torch.nn.functional as F

import distill_helpers as DH
import tuple_loss_helpers as H
from distill_helpers import U

KL, MARGIN = 0, 1                   # include/qst.h: QST_LISTWISE_*
KIND_NAMES = {KL: "kl", MARGIN: "margin_mse"}
SIMS = DH.SIMS
TINY = 2.0 ** -120
BAD_ARG, UNSUPPORTED = -1, -2

# (B, K, D): B = 1, a partial workgroup (3, 5), a full one (4), 17 workgroups (67); K = 1 (KL only), 2, 7, and the last two lane
# counts; D = 4 and 6 (one float4 / the element form), 384 and 768 (the usual widths), 2048 (the last width in registers),
# 2050 (streaming, by element) and 2052 (streaming, 16 bytes a lane)
CASES = [(1, 1, 4), (3, 2, 6), (4, 7, 384), (5, 63, 768), (67, 64, 384), (5, 7, 2048), (3, 2, 2050), (4, 7, 2052),
         (67, 2, 768), (1, 64, 6), (5, 1, 384), (3, 64, 2052)]
TEMPERATURES = (0.5, 1.0, 4.0)


# What qst_listwise_distill_loss refuses before any launch, as keyword overrides of a good call (B, K, D, kind, sim, T, red
# and the pointers q, docs, y, out, so, go, gq, gd, sc; the good call has kind KL, K = 3, red mean and every pointer set)
REFUSED_BAD_ARG = [dict(B=0), dict(B=-1), dict(D=0), dict(D=-1), dict(q=None), dict(docs=None), dict(y=None), dict(out=None),
                   dict(sc=None), dict(red=1, sc=None), dict(kind=2), dict(kind=-1), dict(sim=1), dict(sim=2), dict(sim=3),
                   dict(sim=5), dict(sim=-1), dict(sim=7), dict(red=3), dict(red=-1), dict(T=0.0), dict(T=-1.0),
                   dict(T=math.inf), dict(T=-math.inf), dict(T=math.nan), dict(kind=MARGIN, K=1), dict(gq=None), dict(gd=None)]
REFUSED_UNSUPPORTED = [dict(K=0), dict(K=-1), dict(K=65), dict(K=1 << 20), dict(kind=MARGIN, K=0), dict(kind=MARGIN, K=65)]


def kinds_of(K):
    return (KL, MARGIN) if K >= 2 else (KL,)


def sim_scale(sim, D):
    """The size of a similarity of list_rows' data: unit rows at D = 384 and any cosine are O(1), a raw dot product O(sqrt D)."""
    return 1.0 if (sim == H.COS_SIM or D == 384) else D ** 0.5


def list_rows(B, K, D, seed):
    """q [B, D] and docs [K, B, D] as tuple_loss_helpers.rows draws them: unit rows at D = 384, raw randn elsewhere."""
    x = H.rows(B, D, 1 + K, seed)
    return x[0], torch.stack(x[1:], 0)


# ------------------------------------------------------------------ the yardstick
def sims_ref(q, docs, sim):
    """[B, K]: sim(q, docs[j]) with distill_helpers.sim_ref (the cosine as F.cosine_similarity: qst_pair_metric's semantics)."""
    return torch.stack([DH.sim_ref(q, d, sim) for d in docs], 1)


def rows_ref(q, docs, y, kind, sim, T=1.0):
    s = sims_ref(q, docs, sim)
    y = y.to(s.dtype)
    if kind == KL:
        # nn.KLDivLoss's pointwise xlogy(t, t) - t * log_p: a term with t == 0 is exactly 0
        return F.kl_div(F.log_softmax(s / T, 1), F.softmax(y / T, 1), reduction="none").sum(1) * T ** 2
    return ((s[:, :1] - s[:, 1:] - y) ** 2).sum(1)


def divisor(kind, B, K, red):
    return 1 if red != 2 else (B if kind == KL else B * (K - 1))


def loss_ref(q, docs, y, kind, sim, T=1.0, red=2):
    """red 0 none, 1 sum, 2 mean: upstream's batchmean (KL) / nn.MSELoss() over [B, K - 1] (margin)."""
    rows = rows_ref(q, docs, y, kind, sim, T)
    return rows if red == 0 else rows.sum() / divisor(kind, q.shape[0], docs.shape[0], red)


def kl_upstream(q, docs, y, sim_fct, T):
    """DistillKLDivLoss.forward as sentence-transformers 3.4 writes it."""
    scores = torch.stack([sim_fct(q, d) for d in docs], dim=1) / T
    return torch.nn.KLDivLoss(reduction="batchmean")(F.log_softmax(scores, dim=1), F.softmax(y / T, dim=1)) * T ** 2


def margin_upstream(q, docs, y, sim_fct):
    """MarginMSELoss.forward with several negatives as sentence-transformers 3.x writes it."""
    pos = sim_fct(q, docs[0])
    return F.mse_loss(torch.stack([pos - sim_fct(q, d) for d in docs[1:]], dim=1), y)


# ------------------------------------------------------------------ labels
def kl_labels(B, K, seed, spread=3.0):
    """The teacher's scores: what a cross-encoder's logits look like, a few units apart."""
    g = torch.Generator().manual_seed(seed)
    return spread * torch.randn(B, K, generator=g)


def margin_list_labels(q, docs, sim, seed):
    """The teacher's margins [B, K - 1]: the yardstick's own margin plus a disagreement of 0.51 .. 1.51 times the scale of the
    similarity, sign alternating -- distill_helpers.margin_labels per negative. A residual that cancels to nearly nothing
    has a gradient whose relative error no fp32 evaluation bounds; this keeps every residual at half the scale or more."""
    K, B, D = docs.shape
    g = torch.Generator().manual_seed(seed)
    scale = sim_scale(sim, D)
    s = sims_ref(q.double(), docs.double(), sim)
    m = s[:, :1] - s[:, 1:]
    sign = 1.0 - 2.0 * ((torch.arange(B)[:, None] + torch.arange(K - 1)[None, :]) % 2).double()
    return (m - sign * scale * (0.51 + torch.rand(B, K - 1, generator=g, dtype=torch.float64))).float()


def residuals_hold(q, docs, y, sim):
    """The condition on the margin kind's data: every residual at or above half the similarity's scale."""
    s = sims_ref(q.double(), docs.double(), sim)
    e = s[:, :1] - s[:, 1:] - y.double()
    return bool((e.abs() >= 0.5 * sim_scale(sim, docs.shape[2])).all())


def labels_of(q, docs, kind, sim, seed):
    return kl_labels(q.shape[0], docs.shape[0], seed) if kind == KL else margin_list_labels(q, docs, sim, seed)


# ------------------------------------------------------------------ reference with gradients, computed once per case
def upstream(B, red):
    return H.upstream(B, red)


def reference_of(q, docs, y, kind, sim, T, red, w=None):
    """The fp64 yardstick with autograd: dict(loss, scores [B, K], grad_q, grad_docs), the gradients times w ([B] for
    red 0, [1] otherwise; None = ones)."""
    qd, dd = q.double().clone().requires_grad_(True), docs.double().clone().requires_grad_(True)
    loss = loss_ref(qd, dd, y, kind, sim, T, red)
    (loss * (1.0 if w is None else w.double())).sum().backward()
    return {"loss": loss.detach(), "scores": sims_ref(q.double(), docs.double(), sim), "grad_q": qd.grad, "grad_docs": dd.grad}


@functools.lru_cache(maxsize=None)
def case(B, K, D, kind, sim, T=1.0, red=2, with_w=True):
    """Inputs, labels, upstream gradient, reference and bounds of one case, drawn from a seed the shape fixes. Shared by the
    tests that need it and never written to."""
    q, docs = list_rows(B, K, D, 1000 * B + 10 * K + D)
    y = labels_of(q, docs, kind, sim, B + K + D)
    w = upstream(B, red) if with_w else None
    ref = reference_of(q, docs, y, kind, sim, T, red, w)
    return q, docs, y, w, ref, bounds_of(q, docs, y, kind, sim, T, red, w)


# ------------------------------------------------------------------ the bounds
def softmax_log_slack(R, K):
    return U * (3 * R + 5 * math.log(K) + 12)


def _log_softmax_bound(x, a, K):
    """E [B, 1] for scores x [B, K] known to within a [B, K]."""
    A = a.max(1, keepdim=True).values
    R = x.max(1, keepdim=True).values - x.min(1, keepdim=True).values + 2 * A
    return 2 * A + softmax_log_slack(R, K)


def score_bounds(q, docs, sim):
    return torch.stack([DH.sim_bound(q, d, sim) for d in docs], 1)


def row_bounds(q, docs, y, kind, sim, T=1.0):
    """(bound on the row value [B], g = d row / d sim [B, K] in fp64, bound on g [B, K])."""
    K = docs.shape[0]
    S = sims_ref(q.double(), docs.double(), sim)
    dS = score_bounds(q, docs, sim)
    yd = y.double()
    if kind == KL:
        s, l = S / T, yd / T
        E_p = _log_softmax_bound(s, dS / T + U * s.abs(), K)
        E_t = _log_softmax_bound(l, U * l.abs(), K)
        lp, lt = F.log_softmax(s, 1), F.log_softmax(l, 1)
        p, t = lp.exp(), lt.exp()
        dp = torch.expm1(E_p + 2 * U) * p + TINY
        dt = torch.expm1(E_t + 2 * U) * t + TINY
        d = lt - lp
        E_d = E_t + E_p + U * d.abs()
        term = t * E_d + d.abs() * dt + dt * E_d + U * t * d.abs()
        row = T ** 2 * (t * d).sum(1)
        drow = T ** 2 * (term.sum(1) + 6 * U * (t * d.abs()).sum(1))
        drow = drow + 2 * U * (row.abs() + drow)
        g = T * (p - t)
        return drow, g, (T * (dp + dt) + 2 * U * g.abs()) * (1 + 4 * U)
    m = S[:, :1] - S[:, 1:]
    e = m - yd
    dm = dS[:, :1] + dS[:, 1:] + U * m.abs()
    de = dm + U * (e.abs() + dm)
    sq = (e.abs() + de) ** 2
    drow = (2 * e.abs() * de + de ** 2 + U * sq).sum(1) + 6 * U * sq.sum(1)
    g = torch.cat([2 * e.sum(1, keepdim=True), -2 * e], 1)
    dg0 = (2 * de).sum(1, keepdim=True) + 6 * U * (2 * (e.abs() + de)).sum(1, keepdim=True)
    return drow, g, torch.cat([dg0, 2 * de], 1)


def reduced_bound(drow, ref, kind, K, red):
    """distill_helpers.reduced_bound with the divisor of the kind."""
    if red == 0:
        return drow
    total = drow.sum() / divisor(kind, drow.numel(), K, red)
    return total + U * (ref.detach().abs() + total)


def bounds_of(q, docs, y, kind, sim, T, red, w=None):
    """dict(loss, scores, grad_q, grad_docs) of absolute bounds shaped like the outputs, and `clamped` [B]: the examples
    with a row at or below the cosine's clamp, whose gradients are only required to be finite."""
    K, B, D = docs.shape
    qd, dd = q.double(), docs.double()
    drow, g, dg = row_bounds(q, docs, y, kind, sim, T)
    den = divisor(kind, B, K, red)
    c = g / den
    dc = dg / den + (U * c.abs() if den != 1 else 0.0)
    ca = c.abs() + dc                                   # |c| at its bound
    W = torch.ones(B, dtype=torch.float64) if w is None else w.double().abs().expand(B)
    aq, ad = qd.abs(), dd.abs()                         # [B, D], [K, B, D]
    cT, dcT, caT = c.t()[:, :, None], dc.t()[:, :, None], ca.t()[:, :, None]       # [K, B, 1]
    clamped = torch.zeros(B, dtype=torch.bool)
    if sim == H.DOT:
        b_docs = (dcT + 2 * U * caT) * aq[None]
        b_q = (dcT * ad).sum(0) + (K + 3) * U * (caT * ad).sum(0)
    else:
        nq, nd = qd.norm(dim=1), dd.norm(dim=2)         # [B], [K, B]
        clamped = (nq <= 1e-8) | (nd <= 1e-8).any(0)
        nq, nd = nq.clamp_min(1e-8), nd.clamp_min(1e-8)
        S = sims_ref(qd, dd, sim).t()                   # [K, B]
        dS = score_bounds(q, docs, sim).t()
        rn = (D / 128 + 8) * U
        kxy = 1 / (nq[None] * nd)
        kyy, kxx = S.abs() / nd ** 2, S.abs() / nq[None] ** 2
        dkyy = dS / nd ** 2 + kyy * (2 * rn + 3 * U)
        dkxx = dS / nq[None] ** 2 + kxx * (2 * rn + 3 * U)
        c2, dc2, ca2 = c.t(), dc.t(), ca.t()            # [K, B]
        cxy = ca2 * kxy
        dcxy = dc2 * kxy + cxy * (2 * rn + 3 * U)
        cxy = cxy + dcxy
        cyy = ca2 * kyy
        dcyy = dc2 * kyy + ca2 * dkyy + U * cyy
        cyy = cyy + dcyy
        cq = (ca2 * kxx).sum(0)
        dcq = (dc2 * kxx + ca2 * dkxx + U * ca2 * kxx).sum(0) + 6 * U * cq
        cq = cq + dcq
        b_docs = dcxy[:, :, None] * aq[None] + dcyy[:, :, None] * ad + 3 * U * (cxy[:, :, None] * aq[None] + cyy[:, :, None] * ad)
        b_q = ((dcxy[:, :, None] * ad).sum(0) + dcq[:, None] * aq
               + (K + 4) * U * ((cxy[:, :, None] * ad).sum(0) + cq[:, None] * aq))
    ref = loss_ref(qd, dd, y, kind, sim, T, red)
    return {"loss": reduced_bound(drow, ref, kind, K, red), "scores": score_bounds(q, docs, sim),
            "grad_q": b_q * W[:, None] * (1 + 4 * U), "grad_docs": b_docs * W[None, :, None] * (1 + 4 * U), "clamped": clamped}


def worst(got, ref, bound):
    """max over the elements of |got - ref| / bound (0 / 0 = 0): at most 1 where the bound holds."""
    err = (got.double() - ref).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / bound).max().item()
