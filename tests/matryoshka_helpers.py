"""The yardstick of MatryoshkaLoss over MultipleNegativesRankingLoss (tests/test_gpu_matryoshka.py,
tests/test_matryoshka_host.py, tools/matryoshka_report.py): sum_k w_k * mnrl_helpers.mnrl_ref on the first d_k columns
(cosine, scale 20) in fp64 on the CPU with autograd, on the inputs mnrl_helpers.case draws. Imported like mnrl_helpers,
not a conftest.
"""
import functools

import torch

import mnrl_helpers as M

SCALE = M.SCALE
MIN_REF_LOSS, MIN_REF_GRAD = M.MIN_REF_LOSS, M.MIN_REF_GRAD
# (B, N, D, dims): one and two 64-wide tile edges in each of B, N and D, widths off the 4- and the 16-element grid, K = 8,
# the largest width equal to D everywhere (a smaller one is an edge test of its own). A width of 1 has an identically
# zero gradient (the normalisation's Jacobian vanishes), so it appears in the N = 1 case only.
CASES = [(1, 1, 4, [4, 1]),
         (2, 4, 8, [8, 4, 2]),
         (5, 5, 10, [10, 7, 3, 2]),
         (7, 14, 33, [33, 32, 17, 4]),
         (8, 16, 384, [384, 256, 128, 64, 32]),
         (64, 128, 384, [384, 256, 128, 64]),
         (65, 195, 768, [768, 512, 256, 128, 64]),
         (33, 99, 768, [768, 100, 6]),
         (130, 260, 64, [64, 48, 16, 8]),
         (16, 32, 1024, [1024, 512, 256, 128, 64, 32, 16, 8]),
         (257, 257, 32, [32, 20, 12])]


def case_id(case):
    B, N, D, dims = case
    return f"{B}x{N}x{D}-" + "_".join(str(d) for d in dims)


def weights_of(dims):
    return [1.0 / (k + 1) for k in range(len(dims))]


def matryoshka_ref(a, c, dims, weights, symmetric, scale=SCALE):
    """(loss, [term_k]) in the dtype and on the device of a, c."""
    terms = [M.mnrl_ref(a[:, :d], c[:, :d], "cos", scale, symmetric) for d in dims]
    loss = terms[0] * weights[0]
    for t, w in zip(terms[1:], weights[1:]):
        loss = loss + t * w
    return loss, terms


def reference_of(a, c, dims, weights, symmetric, scale=SCALE):
    """(loss, terms [K], grad_a, grad_c, per-term max |d term_k / d a| [K]) of the fp64 CPU reference on fp32 inputs."""
    a64, c64 = a.double().clone().requires_grad_(True), c.double().clone().requires_grad_(True)
    loss, terms = matryoshka_ref(a64, c64, dims, weights, symmetric, scale)
    term_grad = [torch.autograd.grad(t, a64, retain_graph=True)[0].abs().max().item() for t in terms]
    loss.backward()
    return loss.detach(), torch.stack([t.detach() for t in terms]), a64.grad, c64.grad, term_grad


@functools.lru_cache(maxsize=None)
def _reference(B, N, D, dims, symmetric, trained):
    a, c = M.case(B, N, D, "cos", trained, 1000 * B + D)
    return (a, c) + reference_of(a, c, list(dims), weights_of(dims), symmetric)


def reference(B, N, D, dims, symmetric, trained):
    """The inputs of a case and their reference, computed once and shared (nobody writes to them):
    (a, c, loss, terms, grad_a, grad_c, term_grad)."""
    return _reference(B, N, D, tuple(dims), symmetric, trained)


def assert_not_saturated(N, terms, term_grad):
    """Every term on its own: a softmax that is not saturated, so that a wrong gradient cannot hide behind zeros."""
    if N > 1:
        for t, g in zip(terms.tolist(), term_grad):
            assert t >= MIN_REF_LOSS and g >= MIN_REF_GRAD, (t, g)
