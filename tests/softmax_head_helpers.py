"""The yardstick of losses.SoftmaxLoss's kernels (tests/test_gpu_softmax_head.py, tests/test_gpu_softmax_loss.py,
tests/test_softmax_loss_host.py): sentence-transformers 2.2.2's definition written as torch.cat -> F.linear ->
F.cross_entropy in whatever dtype and on whatever device the inputs have -- fp64 on the CPU with autograd for the kernel
tests -- the recipe the test inputs are drawn by, and the error measures. Imported like mnrl_helpers, not a conftest.

Error measures (tests/mnrl_helpers.py's): a value -- a logit, a loss -- is held within rtol = atol = max(1e-5, 1.5e-8 * K),
K = the width of the classifier's input; a gradient within rtol 1e-4 and atol 1e-6 * max(1, max |reference gradient|).
"""
import functools

import torch
import torch.nn.functional as F

from mnrl_helpers import grad_error  # noqa: F401  (the gradients' measure, shared)

REP, DIFF, MULT = 1, 2, 4                   # include/qst.h QST_SOFTMAX_*
ALL_PARTS = [1, 2, 3, 4, 5, 6, 7]
# the three flag combinations sentence-transformers users pick: the default (u, v, |u - v|), all four parts, (u, v) alone
ST_FLAGS = {"default": (True, True, False), "all": (True, True, True), "rep": (True, False, False)}
RED = {"none": 0, "sum": 1, "mean": 2}
BAD_ARG, UNSUPPORTED = -1, -2               # include/qst.h QST_ERR_*


def nvec(parts):
    return (2 if parts & REP else 0) + (1 if parts & DIFF else 0) + (1 if parts & MULT else 0)


def features(u, v, parts):
    """The classifier's input: the selected parts in sentence-transformers' order u, v, |u - v|, u * v."""
    out = []
    if parts & REP:
        out += [u, v]
    if parts & DIFF:
        out.append(torch.abs(u - v))
    if parts & MULT:
        out.append(u * v)
    return torch.cat(out, 1)


def logits_ref(u, v, w, b, parts):
    return F.linear(features(u, v, parts), w, b)


def loss_ref(u, v, w, b, labels, parts, reduction="mean", ignore_index=-100):
    return F.cross_entropy(logits_ref(u, v, w, b, parts), labels, reduction=reduction, ignore_index=ignore_index)


def case(B, D, C, parts, seed, tied_rows=()):
    """fp32 inputs: rows of u and v with entries of order 1 (a third of v's entries pulled onto u's, so that |u - v| has
    small and exact-zero entries next to large ones; `tied_rows` are copied whole: u == v), a classifier with logits of
    order 1, labels uniform in [0, C)."""
    g = torch.Generator().manual_seed(seed)
    K = nvec(parts) * D
    u = torch.randn(B, D, generator=g)
    v = torch.randn(B, D, generator=g)
    same = torch.rand(B, D, generator=g) < 1.0 / 3.0
    v = torch.where(same, u, v)
    for r in tied_rows:
        v[r] = u[r]
    w = torch.randn(C, K, generator=g) * (2.0 / K ** 0.5)
    b = torch.randn(C, generator=g) * 0.5
    labels = torch.randint(0, C, (B,), generator=g)
    return u, v, w, b, labels


def reference_of(u, v, w, b, labels, parts, reduction, ignore_index=-100, upstream=None):
    """fp64 CPU autograd on the fp32 inputs: (logits, loss, (grad_u, grad_v, grad_w, grad_b)). `upstream`: what the loss is
    multiplied by before the backward -- a [B] tensor under 'none' (the default there: ones), a scalar otherwise."""
    xs = [t.double().clone().requires_grad_(True) for t in (u, v, w, b)]
    logits = logits_ref(*xs, parts)
    loss = F.cross_entropy(logits, labels, reduction=reduction, ignore_index=ignore_index)
    if upstream is None:
        total = loss.sum()
    else:
        total = (loss * torch.as_tensor(upstream, dtype=torch.float64)).sum()
    total.backward()
    return logits.detach(), loss.detach(), tuple(x.grad if x.grad is not None else torch.zeros_like(x) for x in xs)


@functools.lru_cache(maxsize=None)
def reference(B, D, C, parts, reduction):
    """The inputs of a case and their reference, computed once and shared (nobody writes to them)."""
    inputs = case(B, D, C, parts, 7000 + 131 * B + 17 * D + 3 * C + parts)
    return inputs + reference_of(*inputs, parts, reduction)


def value_tol(K):
    return max(1e-5, 1.5e-8 * K)


def value_error(got, ref, K):
    """max |got - ref| as a fraction of the value tolerance (rtol = atol = value_tol(K)); a NaN on either side is infinite."""
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    ref = torch.as_tensor(ref).detach().double().cpu().reshape(-1)
    tol = value_tol(K)
    e = ((got - ref).abs() / (tol + tol * ref.abs())).max().item()
    return e if e == e else float("inf")
