"""The yardstick of MultipleNegativesRankingLoss and its symmetric form (tests/test_gpu_mnrl.py, tests/test_mnrl_host.py,
tools/mnrl_report.py): sentence-transformers 2.2.2's formula written with F.normalize, @ and F.cross_entropy in whatever
dtype and on whatever device the inputs have -- fp64 on the CPU with autograd for the kernel tests -- and the recipe the
test inputs are drawn by. Imported like tuple_loss_helpers, not a conftest.
"""
import functools

import torch
import torch.nn.functional as F

import tuple_loss_helpers as H

SCALE = 20.0
# the smallest shapes (B, N, D) that cross one and two 64-, 128- and 256-wide tile edges in each of B, N, D, an unaligned D,
# a D with a 16-byte tail, and the widest pooled embedding (5 x 1024)
SHAPES = [(1, 1, 1), (1, 3, 10), (2, 4, 8), (5, 5, 10), (7, 14, 33), (8, 16, 384), (64, 64, 384), (64, 128, 384),
          (65, 195, 384), (33, 99, 768), (130, 260, 64), (3, 3, 2052), (16, 32, 5120), (257, 257, 32)]
# what the reference must show before anything is compared with it (every case with N > 1): a softmax that is not
# saturated, so that a wrong gradient cannot hide behind zeros
MIN_REF_LOSS, MIN_REF_GRAD = 4e-3, 2.5e-3


def mnrl_ref(a, c, sim, scale, symmetric):
    """F.cross_entropy(scale * sim(a, c), arange(B)) [+ the same on the transposed B x B block, halved]."""
    if sim == "cos":
        s = F.normalize(a, p=2, dim=1, eps=1e-12) @ F.normalize(c, p=2, dim=1, eps=1e-12).t()
    else:
        s = a @ c.t()
    s = s * scale
    B = a.shape[0]
    target = torch.arange(B, device=a.device)
    loss = F.cross_entropy(s, target)
    if symmetric:
        loss = (loss + F.cross_entropy(s[:, :B].t(), target)) / 2
    return loss


def case(B, N, D, sim, trained, seed):
    """Unit rows drawn in fp64; `trained` pulls every positive towards its anchor (c[:B] = normalize(a + 3 c[:B])), as the
    embeddings of a model that has learnt something are; for cos every row then gets a length of its own in [0.5, 2] (the
    normalisation has to undo it). fp32 out."""
    g = torch.Generator().manual_seed(seed)
    a = F.normalize(torch.randn(B, D, generator=g, dtype=torch.float64), dim=1)
    c = F.normalize(torch.randn(N, D, generator=g, dtype=torch.float64), dim=1)
    if trained:
        c[:B] = F.normalize(a + 3.0 * c[:B], dim=1)
    if sim == "cos":
        a = a * (0.5 + 1.5 * torch.rand(B, 1, generator=g, dtype=torch.float64))
        c = c * (0.5 + 1.5 * torch.rand(N, 1, generator=g, dtype=torch.float64))
    return a.float(), c.float()


def reference_of(a, c, sim, symmetric, scale=SCALE):
    """(loss, grad_a, grad_c) of the fp64 CPU reference with autograd on the fp32 inputs a, c."""
    a64, c64 = a.double().clone().requires_grad_(True), c.double().clone().requires_grad_(True)
    loss = mnrl_ref(a64, c64, sim, scale, symmetric)
    loss.backward()
    return loss.detach(), a64.grad, c64.grad


@functools.lru_cache(maxsize=None)
def reference(B, N, D, sim, symmetric, trained):
    """The inputs of a case and their reference, computed once and shared (nobody writes to them)."""
    a, c = case(B, N, D, sim, trained, 1000 * B + D)
    return (a, c) + reference_of(a, c, sim, symmetric)


def value_tol(D):
    return H.value_tol(H.COS_SIM, D)


def value_error(got, ref, D):
    """|got - ref| as a fraction of the value tolerance (rtol = atol = value_tol(D))."""
    tol = value_tol(D)
    return abs(float(got) - float(ref)) / (tol + tol * abs(float(ref)))


def grad_error(got, ref):
    """max |got - ref| / (atol + rtol |ref|), rtol 1e-4, atol 1e-6 * max(1, max |ref|): at scale 20 gradient entries reach
    3 - 5, and an entry that cancels towards 0 carries the rounding of its O(1) terms."""
    ref = ref.double()
    atol = 1e-6 * max(1.0, ref.abs().max().item())
    return ((got.double() - ref).abs() / (atol + 1e-4 * ref.abs())).max().item()
