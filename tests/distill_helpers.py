"""The yardstick of the distillation objectives (tests/test_gpu_distill.py, tests/test_distill_host.py):
sentence-transformers 2.2.2's MSELoss and MarginMSELoss written in torch ops, in whatever dtype and on whatever device the
inputs have -- fp64 on the CPU with autograd for the kernel tests, fp32 on the GPU as the torch-op path the loss classes are
compared with. Imported like tuple_loss_helpers, not a conftest.
"""
import hashlib

import numpy as np
import torch
import torch.nn.functional as F

import tuple_loss_helpers as H

U = 2.0 ** -24          # unit roundoff of fp32


def embed_mse_ref(x, t):
    """nn.MSELoss() on [B, D]: the mean over every element."""
    return ((x - t) ** 2).mean()


def sim_ref(a, b, sim):
    """H.DOT or H.COS_SIM, the latter as F.cosine_similarity (each norm clamped at 1e-8): qst_pair_metric's semantics."""
    return H.metric_ref(a, b, sim)


def margin_ref(q, p, n, sim):
    return sim_ref(q, p, sim) - sim_ref(q, n, sim)


def margin_mse_ref(q, p, n, y, sim, reduction="mean"):
    return H.reduce_ref((margin_ref(q, p, n, sim) - y.to(q.dtype)) ** 2, reduction)


def dot_bound(u, v):
    """test_pair_metric_matches_yardstick's a-priori bound of an fp32 dot product summed a lane's chain and then the wave
    tree: every product passes through at most D/64 + 10 additions and one multiplication, each within 2^-24 relative --
    [B] absolute bounds, from the fp64 |u v| sums."""
    D = u.shape[1]
    return (D / 64 + 11) * U * (u.double() * v.double()).abs().sum(1)


def sim_bound(a, b, sim):
    """The per-similarity bound the project uses, [B]: H.value_tol for the cosine, the summation bound for the dot product."""
    if sim == H.DOT:
        return dot_bound(a, b)
    return torch.full((a.shape[0],), H.value_tol(H.COS_SIM, a.shape[1]), dtype=torch.float64)


def hash_vector(sentence, dim=8):
    """A vector that depends on nothing but the sentence: what the fake teachers of the host tests return."""
    h = hashlib.sha256(sentence.encode("utf8")).digest()
    return (np.frombuffer(h[:dim], dtype=np.uint8).astype(np.float32) - 128.0) / 64.0


class FakeTeacher:
    """Anything with encode(): counts its calls and the sentences it was given."""

    def __init__(self, dim=8):
        self.dim, self.calls, self.sentences, self.batch_sizes = dim, 0, [], []

    def encode(self, sentences, batch_size=32, show_progress_bar=False, convert_to_numpy=True, **kwargs):
        self.calls += 1
        self.sentences.extend(sentences)
        self.batch_sizes.append(batch_size)
        return np.stack([hash_vector(s, self.dim) for s in sentences]) if len(sentences) else np.zeros((0, self.dim), np.float32)


def cos_matrix(a, b):
    """The fp64 cosine of every pair of rows, numpy."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a / np.linalg.norm(a, axis=1, keepdims=True)) @ (b / np.linalg.norm(b, axis=1, keepdims=True)).T


# ------------------------------------------------------------------ what the GPU tests of these kernels share
SIMS = (H.DOT, H.COS_SIM)


def mse_rel_bound(D):
    """The a-priori relative bound of qst_embed_mse's value. Every term (x - t)^2 is non-negative, so the error of the sum
    is at most the largest relative error a term can pick up on its way into it:
      2   the difference is rounded once, and it enters squared
      1   the square (none if it is fused into the addition that follows)
      D/64 + 4   the additions of a lane's chain: a lane holds at most 4 * ceil(D / 256) <= D/64 + 4 elements
      6   the wave tree: four DPP steps and two levels over the four row totals
      1   the division by B * D and the rounding of the result to fp32
    each within 2^-24 relative, + 1 for their second-order terms and for the second stage, which adds the row sums in
    double (2^-53 each)."""
    return (D / 64 + 15) * U


def margin_labels(q, p, n, sim, seed):
    """The teacher's margins: the yardstick's own margin of the row plus a disagreement of 0.5 .. 1.5 times the scale of
    the similarity, sign alternating. A residual m - y that cancels to nearly nothing has a gradient 2 (m - y) dm/dx whose
    RELATIVE error is err(m) / |m - y| in any fp32 evaluation, without bound as the residual goes to 0; this keeps every
    residual at half the similarity's scale or more (asserted by the callers: a condition on the test data)."""
    B, D = q.shape
    g = torch.Generator().manual_seed(seed)
    scale = 1.0 if (sim == H.COS_SIM or D == 384) else D ** 0.5      # H.rows: unit rows at D = 384, raw randn elsewhere
    sign = 1.0 - 2.0 * (torch.arange(B) % 2).double()
    m = margin_ref(q.double(), p.double(), n.double(), sim)
    y = (m - sign * scale * (0.5 + torch.rand(B, generator=g, dtype=torch.float64))).float()
    assert ((m - y.double()).abs() >= 0.49 * scale).all()
    return y


def margin_bounds(q, p, n, y, sim):
    """(bound on m [B], bound on the row value (m - y)^2 [B]), a priori: each similarity within the bound the project holds
    it to (sim_bound), one rounding for their difference, one for the residual, one for the square."""
    m = margin_ref(q.double(), p.double(), n.double(), sim)
    e = m - y.double()
    dm = sim_bound(q, p, sim) + sim_bound(q, n, sim) + U * m.abs()
    de = dm + U * (e.abs() + dm)
    return dm, 2 * e.abs() * de + de ** 2 + U * (e.abs() + de) ** 2


def reduced_bound(drow, ref, red):
    """The row bounds through the second stage (double: nothing to add) and the one rounding of the result to fp32."""
    if red == 0:
        return drow
    total = drow.sum() / (drow.numel() if red == 2 else 1)
    return total + U * (ref.detach().abs() + total)
