"""The yardstick of CoSENTLoss and AnglELoss (tests/test_gpu_cosent.py, tests/test_cosent_host.py, tools/cosent_bench.py):
sentence-transformers' two pairwise score functions and its loss restated in torch ops, in whatever dtype and on whatever
device the inputs have -- fp64 on the CPU with autograd for the kernel tests -- and the recipe the test inputs are drawn by.
Imported like mnrl_helpers, not a conftest.
"""
import functools

import torch
import torch.nn.functional as F

import mnrl_helpers as M
import tuple_loss_helpers as H

SCALE = 20.0
# (B, D): no pair; the smallest batches; even D with D % 4 != 0 (element form); odd D (cos only); D % 4 == 0 with the angle
# halves 16-byte misaligned; a row past the last full workgroup (twice); a j loop past 256; the first streamed width (cos) and
# the first streamed width whose angle halves are aligned; wide streamed rows; a second stage past one pass of 1024
SHAPES = [(1, 2), (2, 2), (2, 4), (5, 10), (7, 34), (7, 33), (8, 388), (64, 384), (65, 768), (257, 32), (3, 2052), (3, 2056),
          (16, 5120), (1030, 64)]
SIMS = ("cos", "angle")
LABEL_SETS = ("graded", "ties", "binary")
# what the reference must show before anything is compared with it (B >= 5): a loss that is not saturated at 0, gradients a
# wrong formula cannot hide behind, and angle scores whose sign fp32 and fp64 agree on
MIN_REF_LOSS, MIN_REF_GRAD, MIN_ANGLE_SCORE = 1.0, 0.3, 1e-3


def sims_of(D):
    return SIMS if D % 2 == 0 else ("cos",)


def cases():
    return [(B, D, sim) for B, D in SHAPES for sim in sims_of(D)]


# ------------------------------------------------------------------ the score functions
def cos_sim_ref(u, v):
    """util.pairwise_cos_sim as sentence-transformers defines it: the dot product of the F.normalize'd rows."""
    return torch.sum(F.normalize(u, p=2, dim=1, eps=1e-12) * F.normalize(v, p=2, dim=1, eps=1e-12), dim=1)


def angle_sim_ref(x, y):
    """util.pairwise_angle_sim, sentence-transformers' chunk form."""
    a, b = torch.chunk(x, 2, dim=1)
    c, d = torch.chunk(y, 2, dim=1)
    z = torch.sum(c ** 2 + d ** 2, dim=1, keepdim=True)
    re = (a * c + b * d) / z
    im = (b * c - a * d) / z
    dz = torch.sum(a ** 2 + b ** 2, dim=1, keepdim=True) ** 0.5
    dw = torch.sum(c ** 2 + d ** 2, dim=1, keepdim=True) ** 0.5
    re = re / (dz / dw)
    im = im / (dz / dw)
    return torch.abs(torch.sum(torch.cat((re, im), dim=1), dim=1))


def angle_sim_closed(x, y):
    """The same value in one pass with three sums: |x . [c - d, c + d]| / (|x| |y|)."""
    c, d = torch.chunk(y, 2, dim=1)
    t = torch.sum(x * torch.cat((c - d, c + d), dim=1), dim=1)
    return torch.abs(t) / (x.norm(dim=1) * y.norm(dim=1))


SIM_REF = {"cos": cos_sim_ref, "angle": angle_sim_ref}


# ------------------------------------------------------------------ the loss
def cosent_ref(scores, labels, scale=SCALE):
    """sentence-transformers' CoSENTLoss.forward from the pairwise scores on: the B x B differences, the pairs the labels do
    not order pushed down by 1e12, logsumexp with a zero in front."""
    s = scores * scale
    s = s[:, None] - s[None, :]
    mask = (labels[:, None] < labels[None, :]).to(s.dtype)
    s = s - (1 - mask) * 1e12
    return torch.logsumexp(torch.cat((torch.zeros(1, dtype=s.dtype, device=s.device), s.view(-1)), dim=0), dim=0)


def cosent_excluded(scores, labels, scale=SCALE):
    """log(1 + sum over the pairs with labels[i] < labels[j] of exp(scale * (s_i - s_j))): the same loss with the other pairs
    left out instead of pushed down."""
    s = scores * scale
    s = (s[:, None] - s[None, :])[labels[:, None] < labels[None, :]]
    return torch.logsumexp(torch.cat((torch.zeros(1, dtype=s.dtype, device=s.device), s)), dim=0)


def loss_ref(u, v, labels, sim, scale=SCALE):
    return cosent_ref(SIM_REF[sim](u, v), labels.to(u.dtype), scale)


# ------------------------------------------------------------------ the cases
def labels_of(kind, B, g):
    if kind == "graded":
        return torch.rand(B, generator=g)
    if kind == "ties":
        return torch.randint(0, 6, (B,), generator=g).float() / 5
    return (torch.arange(B) % 2).float()


def case(B, D, kind, seed=None):
    """u: unit rows drawn in fp64; v = normalize(u + (0.3 + 1.7 r) * normalize(noise)), r uniform per row: scores spread from
    close to far; every row of u and v then gets a length of its own in [0.5, 2] (both scores have to undo it). fp32 out,
    with fp32 labels of the kind asked for."""
    g = torch.Generator().manual_seed(1000 * B + D if seed is None else seed)
    u = F.normalize(torch.randn(B, D, generator=g, dtype=torch.float64), dim=1)
    noise = F.normalize(torch.randn(B, D, generator=g, dtype=torch.float64), dim=1)
    r = torch.rand(B, 1, generator=g, dtype=torch.float64)
    v = F.normalize(u + (0.3 + 1.7 * r) * noise, dim=1)
    u = u * (0.5 + 1.5 * torch.rand(B, 1, generator=g, dtype=torch.float64))
    v = v * (0.5 + 1.5 * torch.rand(B, 1, generator=g, dtype=torch.float64))
    return u.float(), v.float(), labels_of(kind, B, g)


def reference_of(u, v, labels, sim, scale=SCALE):
    """(loss, scores, grad_u, grad_v) of the fp64 CPU reference with autograd on the fp32 inputs."""
    u64, v64 = u.double().clone().requires_grad_(True), v.double().clone().requires_grad_(True)
    scores = SIM_REF[sim](u64, v64)
    loss = cosent_ref(scores, labels.double(), scale)
    loss.backward()
    return loss.detach(), scores.detach(), u64.grad, v64.grad


@functools.lru_cache(maxsize=None)
def reference(B, D, sim, kind):
    """The inputs of a case and their reference, computed once and shared (nobody writes to them)."""
    u, v, y = case(B, D, kind)
    return (u, v, y) + reference_of(u, v, y, sim)


def assert_conditions(B, sim, loss, scores, gu, gv):
    """What the data must show before a comparison means anything (see MIN_* above)."""
    if B < 5:
        return
    assert loss.item() >= MIN_REF_LOSS, loss.item()
    assert max(gu.abs().max().item(), gv.abs().max().item()) >= MIN_REF_GRAD
    if sim == "angle":
        assert scores.min().item() >= MIN_ANGLE_SCORE, scores.min().item()


# ------------------------------------------------------------------ the tolerances (the project's own)
def value_tol(D):
    return H.value_tol(H.COS_SIM, D)


value_error = M.value_error          # |got - ref| as a share of rtol = atol = value_tol(D)
grad_error = M.grad_error            # max |got - ref| / (1e-6 max(1, max |ref|) + 1e-4 |ref|)


def score_error(got, ref, D):
    """The worst score as a share of rtol = atol = value_tol(D)."""
    tol = value_tol(D)
    return ((got.double() - ref.double()).abs() / (tol + tol * ref.double().abs())).max().item()
