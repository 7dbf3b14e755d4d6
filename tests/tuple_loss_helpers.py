"""The yardstick of the pair and triplet losses (tests/test_gpu_tuple_losses.py, tests/test_tuple_losses_host.py):
sentence-transformers 2.2.2's formulas written with torch's own F.cosine_similarity / F.pairwise_distance, in whatever
dtype and on whatever device the inputs have -- fp64 on the CPU with autograd for the kernel tests, fp32 on the GPU as the
torch-op path the loss classes are compared with. Imported like kernel_helpers, not a conftest.
"""
import numpy as np
import torch
import torch.nn.functional as F

# include/qst.h
COS_SIM, COS_DIST, L2, L1, DOT, L2_PLAIN, L1_PLAIN = range(7)
METRIC_NAMES = {COS_SIM: "cos_sim", COS_DIST: "cos_dist", L2: "l2", L1: "l1", DOT: "dot", L2_PLAIN: "l2_plain",
                L1_PLAIN: "l1_plain"}
DISTANCES = (COS_DIST, L2, L1)
MSE, CONTRASTIVE, ONLINE = range(3)
SHAPES = [(1, 10), (5, 10), (8, 384), (64, 384), (32, 768), (7, 33), (3, 2052), (16, 5120)]
ONLINE_SHAPES = [(64, 384), (33, 768), (256, 384), (8, 64), (128, 1024)]


def metric_ref(u, v, metric):
    if metric == COS_SIM:
        return F.cosine_similarity(u, v)
    if metric == COS_DIST:
        return 1 - F.cosine_similarity(u, v)
    if metric == L2:
        return F.pairwise_distance(u, v, p=2)
    if metric == L1:
        return F.pairwise_distance(u, v, p=1)
    if metric == DOT:
        return (u * v).sum(1)
    if metric == L2_PLAIN:
        return (u - v).norm(p=2, dim=1)
    if metric == L1_PLAIN:
        return (u - v).norm(p=1, dim=1)
    raise ValueError(metric)


def reduce_ref(rows, reduction):
    return rows if reduction == "none" else (rows.sum() if reduction == "sum" else rows.mean())


def mse_ref(u, v, y, reduction="mean"):
    """CosineSimilarityLoss with nn.MSELoss and nn.Identity."""
    return reduce_ref((F.cosine_similarity(u, v) - y.to(u.dtype)) ** 2, reduction)


def contrastive_ref(u, v, y, metric, margin, reduction="mean"):
    d = metric_ref(u, v, metric)
    y = y.to(u.dtype)
    return reduce_ref(0.5 * (y * d.pow(2) + (1 - y) * F.relu(margin - d).pow(2)), reduction)


def online_selection(d, y):
    """(rows of the selected positives, rows of the selected negatives, t_pos, t_neg) of OnlineContrastiveLoss."""
    negs, poss = d[y == 0], d[y == 1]
    t_neg = poss.max() if len(poss) > 1 else negs.mean()
    t_pos = negs.min() if len(negs) > 1 else poss.mean()
    return (y == 1) & (d > t_pos), (y == 0) & (d < t_neg), t_pos, t_neg


def online_ref(u, v, y, metric, margin):
    d = metric_ref(u, v, metric)
    negs, poss = d[y == 0], d[y == 1]
    negative_pairs = negs[negs < (poss.max() if len(poss) > 1 else negs.mean())]
    positive_pairs = poss[poss > (negs.min() if len(negs) > 1 else poss.mean())]
    return positive_pairs.pow(2).sum() + F.relu(margin - negative_pairs).pow(2).sum()


def triplet_ref(a, p, n, metric, margin, reduction="mean"):
    return reduce_ref(F.relu(metric_ref(a, p, metric) - metric_ref(a, n, metric) + margin), reduction)


def value_tol(metric, D):
    """The project's tolerance for qst_quadruplet_loss (tests/test_gpu_kernels.py): L2 and the cosine metrics, L1."""
    return max(1e-4, 2e-6 * D) if metric in (L1, L1_PLAIN) else max(1e-5, 1.5e-8 * D)


def rows(B, D, k, seed):
    """k [B, D] fp32 inputs as the quadruplet kernel's test draws them: unit rows at D = 384, raw randn elsewhere."""
    g = torch.Generator().manual_seed(seed)
    x = [torch.randn(B, D, generator=g) for _ in range(k)]
    if D == 384:
        x = [t / t.norm(dim=1, keepdim=True) for t in x]
    return x


def online_case(B, D, seed):
    """Labels alternating 0 / 1, u unit rows, v = normalize(u + s * normalize(noise)), s uniform in [0.2, 1.0] for the
    positives and in [0.6, 1.5] for the negatives: both selected sets are proper non-empty subsets."""
    g = torch.Generator().manual_seed(seed)
    y = (torch.arange(B) % 2).to(torch.float32)
    u = F.normalize(torch.randn(B, D, generator=g, dtype=torch.float64), dim=1)
    noise = F.normalize(torch.randn(B, D, generator=g, dtype=torch.float64), dim=1)
    r = torch.rand(B, generator=g, dtype=torch.float64)
    s = torch.where(y == 1, 0.2 + 0.8 * r, 0.6 + 0.9 * r)
    v = F.normalize(u + s[:, None] * noise, dim=1)
    return u.to(torch.float32), v.to(torch.float32), y


def rank_avg(x):
    """Average ranks (ties share the mean rank), written out the slow way."""
    x = np.asarray(x, dtype=np.float64)
    return np.array([(x < xi).sum() + ((x == xi).sum() + 1) / 2.0 for xi in x])


def pearson_np(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    x, y = x - x.mean(), y - y.mean()
    return float((x * y).sum() / np.sqrt((x * x).sum() * (y * y).sum()))


def spearman_np(x, y):
    return pearson_np(rank_avg(x), rank_avg(y))


# ------------------------------------------------------------------ what the GPU tests of these kernels share
RED = (("none", 0), ("sum", 1), ("mean", 2))


def dev(t):
    return t.cuda().contiguous()


def f64(xs):
    return [t.double().clone().requires_grad_(True) for t in xs]


def upstream(B, red):
    """A non-trivial upstream gradient, as test_loss_matches_oracle uses."""
    return torch.linspace(0.5, 1.5, B) if red == 0 else torch.tensor([1.7])


def check_value(out, ref, metric, B, D, red):
    tol = value_tol(metric, D)
    got = out.cpu().double().view(ref.shape)
    print(f"  value: max |d| = {(got - ref.detach()).abs().max().item():.3e} (tol {tol:.1e})")
    torch.testing.assert_close(got, ref.detach(), rtol=tol, atol=tol * (B if red == 1 else 1))


def check_grads(grads, xs, skip_rows=None):
    for gi, xi in zip(grads, xs):
        got, ref = gi.cpu().double(), xi.grad
        assert torch.isfinite(got).all()
        if skip_rows is not None:
            got, ref = got[~skip_rows], ref[~skip_rows]
        torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-6)


def margin_between(vals, metric, D):
    """A margin inside the central half of `vals` (the yardstick's distances, or d(a, n) - d(a, p)), in the middle of the widest
    space between two neighbours there: a good part of the hinges open, the rest closed, and -- a condition on the test data
    -- no row closer to the hinge's kink than five times the error the project accepts on a distance, where fp32 and fp64
    could fall on different sides of it."""
    s = vals.detach().sort().values
    if len(s) == 1:
        m = 0.5 * float(s[0])
    else:
        lo, hi = (len(s) - 1) // 4, max((len(s) - 1) // 4 + 1, (3 * len(s)) // 4)
        k = lo + int((s[lo + 1:hi + 1] - s[lo:hi]).argmax())
        m = 0.5 * float(s[k] + s[k + 1])
    m = float(torch.tensor(max(0.0, m), dtype=torch.float32))   # as the C ABI's `float margin` holds it: the yardstick's too
    gap = (vals.detach() - m).abs().min().item()
    assert gap >= 5 * value_tol(metric, D), gap
    return m


def pair_labels(B, kind, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, generator=g) if kind == MSE else (torch.arange(B) % 2).float()
