"""The yardstick of the batch-mining triplet losses (tests/test_gpu_batch_triplet.py, tests/test_batch_triplet_host.py,
tools/batch_triplet_report.py): sentence-transformers 2.2.2's BatchHardTripletLoss, BatchHardSoftMarginTripletLoss,
BatchSemiHardTripletLoss and BatchAllTripletLoss written twice -- in upstream's tensor formulation (max / min over masked
matrices, the tiled semi-hard form with _masked_minimum / _masked_maximum) in whatever dtype the inputs have, fp64 on the
CPU with autograd for the kernel tests, and as plain loops over anchors and positives that also measure how far every
decision of the mining is from flipping -- and the recipe the test inputs are drawn by. Imported like mnrl_helpers, not a
conftest.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import tuple_loss_helpers as H
from mnrl_helpers import grad_error  # noqa: F401  (rtol 1e-4, atol 1e-6 * max(1, max |ref|))

EUCLID, COS = H.L2_PLAIN, H.COS_DIST                # include/qst.h: QST_METRIC_L2_PLAIN, QST_METRIC_COS_DIST
METRICS = (EUCLID, COS)
METRIC_NAMES = {EUCLID: "euclid", COS: "cos"}
HARD, SOFT, SEMI, ALL = range(4)                    # include/qst.h: QST_BT_*
KINDS = (HARD, SOFT, SEMI, ALL)
KIND_NAMES = {HARD: "hard", SOFT: "soft", SEMI: "semi", ALL: "all"}
# at upstream's default margin of 5 every hinge is active and clips nothing
MARGIN = {EUCLID: 0.1, COS: 0.1}
# (B, D): one and two 64-wide tile edges in B, an unaligned D, a D with a 16-byte tail, the widest pooled embedding;
# (130, 64) keeps the O(B^3) kinds to a few million comparisons, (257, 32) is for the O(B^2) kinds only
SHAPES = [(4, 8), (5, 10), (8, 384), (33, 768), (64, 384), (65, 384), (130, 64), (6, 2052), (16, 5120)]
HARD_ONLY_SHAPES = [(257, 32)]
MIN_FRAGILITY = 1e-5            # a condition on the inputs, not a tolerance: > 10 x the fp32 error of a distance <= 4
MIN_REF_LOSS = MIN_REF_GRAD = 1e-3
SEED_TRIES = 64


def shapes_of(kind):
    return SHAPES + (HARD_ONLY_SHAPES if kind in (HARD, SOFT) else [])


# ------------------------------------------------------------------ distances
def dist_ref(x, metric):
    """BatchHardTripletLossDistanceFunction: eucledian_distance (Gram form, clamped at 0; an exactly-zero distance is 0
    with gradient 0) or cosine_distance."""
    if metric == COS:
        e = F.normalize(x, p=2, dim=1, eps=1e-12)
        return 1 - e @ e.t()
    g = x @ x.t()
    sq = torch.diag(g)
    d2 = (sq.unsqueeze(0) - 2.0 * g + sq.unsqueeze(1)).clamp_min(0)
    zero = (d2 == 0).to(d2.dtype)
    return (1.0 - zero) * torch.sqrt(d2 + zero * 1e-16)


# ------------------------------------------------------------------ formulation 1: upstream's tensors
def _masked_minimum(data, mask, dim=1):
    axis_maximums = data.max(dim, keepdim=True)[0]
    return ((data - axis_maximums) * mask).min(dim, keepdim=True)[0] + axis_maximums


def _masked_maximum(data, mask, dim=1):
    axis_minimums = data.min(dim, keepdim=True)[0]
    return ((data - axis_minimums) * mask).max(dim, keepdim=True)[0] + axis_minimums


def mine_tensor(d, labels, kind, margin):
    """(loss, (terms the denominator is drawn from, terms > 0)) on a distance matrix d [B, B]."""
    B = labels.numel()
    labels = labels.view(-1)
    same = labels.unsqueeze(0) == labels.unsqueeze(1)
    eye = torch.eye(B, dtype=torch.bool)
    pos, neg = (same & ~eye).to(d.dtype), (~same).to(d.dtype)
    if kind in (HARD, SOFT):
        hp = (pos * d).max(1, keepdim=True)[0]
        hn = (d + d.max(1, keepdim=True)[0] * (1.0 - neg)).min(1, keepdim=True)[0]
        if kind == SOFT:
            return torch.log1p(torch.exp(hp - hn)).mean(), (B, B)
        tl = torch.relu(hp - hn + margin)
        return tl.mean(), (B, int((tl > 0).sum()))
    if kind == ALL:
        mask = pos.unsqueeze(2) * neg.unsqueeze(1)
        t = torch.relu(mask * (d.unsqueeze(2) - d.unsqueeze(1) + margin))
        n_active = int((t > 1e-16).sum())
        return t.sum() / (n_active + 1e-16), (int(mask.sum()), n_active)
    tile = d.repeat(B, 1)                                            # row j * B + i holds d[i, :]
    mask = (~same).repeat(B, 1) & (tile > d.t().reshape(-1, 1))      # the negatives of i farther away than d[i, j]
    mask_final = (mask.sum(1, keepdim=True) > 0).reshape(B, B).t()
    negatives_outside = _masked_minimum(tile, mask.to(d.dtype)).reshape(B, B).t()
    negatives_inside = _masked_maximum(d, neg).repeat(1, B)
    semi_hard_negatives = torch.where(mask_final, negatives_outside, negatives_inside)
    terms = torch.relu((d - semi_hard_negatives + margin) * pos)
    return terms.sum() / pos.sum(), (int(pos.sum()), int((terms > 0).sum()))


def loss_tensor(x, labels, kind, metric, margin):
    return mine_tensor(dist_ref(x, metric), labels, kind, margin)


# ------------------------------------------------------------------ formulation 2: loops over anchors and positives
def mine_loops(d, labels, kind, margin):
    """The same four losses from the definitions, anchor by anchor, on d as a float64 numpy array: (numerator, denominator,
    counts, W with W[i, j] = d(numerator) / d(d[i, j]), fragility = the smallest distance of any decision -- an arg-max, an
    arg-min, a membership, the sign of a hinge -- from flipping)."""
    d = np.asarray(d, dtype=np.float64)
    lab = np.asarray(labels)
    B = len(lab)
    W = np.zeros((B, B))
    num, frag = 0.0, np.inf
    c0 = c1 = 0

    def gap(values, largest):
        """best minus runner-up of a selection"""
        if len(values) < 2:
            return np.inf
        s = np.sort(values)
        return s[-1] - s[-2] if largest else s[1] - s[0]

    for i in range(B):
        P = [j for j in range(B) if j != i and lab[j] == lab[i]]
        N = [k for k in range(B) if lab[k] != lab[i]]
        if kind in (HARD, SOFT):
            c0 += 1
            hp, jp = 0.0, None
            if P and d[i, P].max() > 0:
                jp = P[int(np.argmax(d[i, P]))]
                hp = d[i, jp]
                frag = min(frag, gap(d[i, P], True))
            if N:
                kn = N[int(np.argmin(d[i, N]))]
                hn = d[i, kn]
                frag = min(frag, gap(d[i, N], False))
                parts = [(kn, -1.0)]
            else:                                       # every entry is d_ik + rowmax: the row minimum plus the row maximum
                kn, km = int(np.argmin(d[i])), int(np.argmax(d[i]))
                hn = d[i, kn] + d[i, km]
                parts = [(kn, -1.0), (km, -1.0)]
            if jp is not None:
                parts.append((jp, 1.0))
            arg = hp - hn
            if kind == HARD:
                frag = min(frag, abs(arg + margin))
                sig = 1.0 if arg + margin > 0 else 0.0
                num += max(arg + margin, 0.0)
                c1 += int(arg + margin > 0)
            else:
                sig = 1.0 / (1.0 + np.exp(-arg))
                num += np.log1p(np.exp(arg))
                c1 += 1
            for k, w in parts:
                W[i, k] += w * sig
        elif kind == ALL:
            for j in P:
                if not N:
                    break
                t = d[i, j] - d[i, N] + margin
                frag = min(frag, np.abs(t).min())
                act = t > 0
                num += t[act].sum()
                c0 += len(N)
                c1 += int((t > 1e-16).sum())
                W[i, j] += act.sum()
                W[i, np.asarray(N)[act]] -= 1.0
        else:
            for j in P:
                c0 += 1
                if N:
                    dn = d[i, N]
                    frag = min(frag, np.abs(dn - d[i, j]).min())
                    far = dn > d[i, j]
                    if far.any():
                        pool, kpool = dn[far], np.asarray(N)[far]
                        kn = int(kpool[np.argmin(pool)])
                        frag = min(frag, gap(pool, False))
                    else:
                        kn = N[int(np.argmax(dn))]
                        frag = min(frag, gap(dn, True))
                else:
                    kn = int(np.argmin(d[i]))           # no negative at all: the row minimum, i.e. the diagonal
                h = d[i, j] - d[i, kn] + margin
                frag = min(frag, abs(h))
                if h > 0:
                    num += h
                    c1 += 1
                    W[i, j] += 1.0
                    W[i, kn] -= 1.0
    if kind == ALL:
        den = c1 + 1e-16
    else:
        den = float(c0)
    return num, den, (c0, c1), W, float(frag)


def loss_loops(x, labels, kind, metric, margin):
    """(loss, counts, fragility) with the selections made by mine_loops on the detached distances; the loss is a
    differentiable function of x through the selected entries only."""
    d = dist_ref(x, metric)
    num, den, counts, W, frag = mine_loops(d.detach().numpy(), labels.numpy(), kind, margin)
    if kind == SOFT:
        # the soft margin is not linear in d: rebuild it from the selected entries
        sel = torch.from_numpy(np.sign(W))
        loss = torch.log1p(torch.exp((sel * d).sum(1))).sum() / den if den else torch.tensor(float("nan"))
    else:
        const = num - float((torch.from_numpy(W) * d.detach()).sum())       # the margins of the active hinges
        loss = ((torch.from_numpy(W) * d).sum() + const) / den if den else (d.sum() * 0 + float("nan"))
    return loss, counts, frag


# ------------------------------------------------------------------ the inputs
def case(B, D, seed):
    """Clustered rows with a label each: unit rows pulled towards the unit centroid of their class (0.3 of it), then every
    row gets a length of its own in [0.5, 2]. ncls = max(2, B // 4) classes, labels a shuffled arange(B) % ncls. x fp32,
    labels int64."""
    g = torch.Generator().manual_seed(seed)
    x = F.normalize(torch.randn(B, D, generator=g, dtype=torch.float64), dim=1)
    ncls = max(2, B // 4)
    labels = torch.randperm(B, generator=g) % ncls
    centroid = F.normalize(torch.randn(ncls, D, generator=g, dtype=torch.float64), dim=1)
    x = F.normalize(x + 0.3 * centroid[labels], dim=1)
    x = x * (0.5 + 1.5 * torch.rand(B, 1, generator=g, dtype=torch.float64))
    return x.float(), labels.to(torch.int64)


def reference_of(x, labels, kind, metric, margin=None):
    """(loss, grad_x, counts) of the fp64 CPU reference (the tensor formulation) with autograd on the fp32 input x."""
    margin = MARGIN[metric] if margin is None else margin
    x64 = x.double().clone().requires_grad_(True)
    loss, counts = loss_tensor(x64, labels, kind, metric, margin)
    if torch.isfinite(loss):
        loss.backward()
    grad = x64.grad if x64.grad is not None else torch.zeros_like(x64)
    return loss.detach(), grad, counts


def fragility(x, labels, kind, metric, margin=None):
    margin = MARGIN[metric] if margin is None else margin
    d = dist_ref(x.double(), metric)
    return mine_loops(d.numpy(), labels.numpy(), kind, margin)[4]


def seed_of(B, D, k):
    return 1000 * B + D + 7919 * k


@functools.lru_cache(maxsize=None)
def reference(B, D, kind, metric):
    """(x, labels, loss, grad, counts, k) of the first seed 1000 B + D + 7919 k, k < 64, whose every mining decision is at
    least MIN_FRAGILITY from flipping -- computed once and shared (nobody writes to them). The reference of a case with
    B >= 4 must itself show a loss and a gradient above 1e-3: a wrong kernel has nowhere to hide."""
    for k in range(SEED_TRIES):
        x, labels = case(B, D, seed_of(B, D, k))
        if fragility(x, labels, kind, metric) >= MIN_FRAGILITY:
            break
    else:
        raise AssertionError(f"no seed with fragility >= {MIN_FRAGILITY} for {(B, D)} {KIND_NAMES[kind]} {METRIC_NAMES[metric]}")
    loss, grad, counts = reference_of(x, labels, kind, metric)
    if B >= 4:
        assert loss.item() > MIN_REF_LOSS and grad.abs().max().item() > MIN_REF_GRAD, (B, D, kind, metric, loss.item(),
                                                                                      grad.abs().max().item())
    return x, labels, loss, grad, counts, k


# ------------------------------------------------------------------ edge batches at (8, 32)
def edge_cases():
    """name -> (x fp32 [8, 32], labels int64 [8])."""
    x, labels = case(8, 32, 8032)                       # two classes of four
    out = {}
    lone = labels.clone()
    lone[0] = 7                                         # a label that occurs once
    out["lone_label"] = (x, lone)
    out["all_equal"] = (x, torch.zeros(8, dtype=torch.int64))
    out["all_distinct"] = (x, torch.arange(8, dtype=torch.int64))
    dup = x.clone()
    j = int((labels == labels[0]).nonzero()[1])         # another row of row 0's class
    dup[j] = dup[0]
    out["duplicate_rows"] = (dup, labels)
    return out


# ------------------------------------------------------------------ past one chunk of the staged row
BIG = (1030, 16)
BIG_KINDS = (SEMI, ALL)         # the kinds that stage the row; hard / soft read it in place at any B ((257, 32) above)


def big_case(seed):
    """More rows than the mining kernels stage through LDS at a time (1024) and than one trip of their 256-thread loops:
    eight classes of two rows, one in the first chunk and one in the second (rows c and 1022 + c), and 1014 rows with a
    label of their own -- negatives in both chunks, and few enough decisions (16 pairs x 1028 negatives) for a tie-free
    seed to exist."""
    B, D = BIG
    x, _ = case(B, D, seed)
    labels = torch.arange(B, dtype=torch.int64) + 100
    for c in range(8):
        labels[c] = labels[1022 + c] = c
    return x, labels


@functools.lru_cache(maxsize=None)
def big_reference(kind, metric):
    """(x, labels, loss, grad, counts) of big_case from the loop formulation in fp64 (B^3 is out of reach of the tensor
    one; tests/test_batch_triplet_host.py holds the two against each other), first seed with fragility >= MIN_FRAGILITY."""
    m = MARGIN[metric]
    for k in range(SEED_TRIES):
        x, labels = big_case(seed_of(*BIG, k))
        x64 = x.double().clone().requires_grad_(True)
        loss, counts, frag = loss_loops(x64, labels, kind, metric, m)
        if frag >= MIN_FRAGILITY:
            break
    else:
        raise AssertionError(f"no seed with fragility >= {MIN_FRAGILITY} for the big case")
    loss.backward()
    assert loss.item() > MIN_REF_LOSS and x64.grad.abs().max().item() > MIN_REF_GRAD
    return x, labels, loss.detach(), x64.grad, counts


def value_tol(metric, D):
    return H.value_tol(metric, D)


def value_error(got, ref, metric, D):
    """|got - ref| as a fraction of the value tolerance (rtol = atol = value_tol(metric, D))."""
    tol = value_tol(metric, D)
    return abs(float(got) - float(ref)) / (tol + tol * abs(float(ref)))
