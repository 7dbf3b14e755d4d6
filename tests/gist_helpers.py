"""The yardstick of GISTEmbedLoss (tests/test_gist_host.py, tests/test_gpu_gist.py, tests/test_gpu_gist_model.py,
tools/gist_bench.py): sentence-transformers' formula written literally -- sim matrices, boolean masks, -inf, torch.cat,
F.cross_entropy -- in whatever dtype and on whatever device the inputs have (fp64 on the CPU with autograd for the kernel
tests), and the recipe the test inputs are drawn by. Imported like mnrl_helpers, not a conftest.

The guide of a test must DECIDE its masks: an entry whose guide score sits within fp32 rounding of the row's threshold is
masked by one arithmetic and kept by another, and the comparison of two correct implementations fails. A plain random guide
does not do (the smallest |entry - threshold| of a batch shrinks like 1 / B^2), so the guide columns are clustered and bimodal
(guide_case), the seeds are fixed, and `conditions` asserts on the CPU what every case must show before anything is compared
with it.
"""
import functools

import torch
import torch.nn.functional as F

import mnrl_helpers as M

# (B, K, D, Dg): the smallest shapes that cross one and two 64- and 128-wide tile edges in B and in (K + 1) * B, an unaligned D
# and Dg, a D with a 16-byte tail, K = 4, and Dg != D both ways
SHAPES = [(1, 2, 1, 1), (2, 2, 8, 4), (5, 3, 10, 7), (7, 3, 33, 16), (8, 2, 384, 384), (64, 2, 384, 768), (65, 3, 384, 384),
          (33, 4, 768, 384), (130, 2, 64, 256), (257, 2, 32, 384), (3, 2, 2052, 2052), (16, 3, 5120, 8)]
# the larger tiles, (K + 1) * B > 4096 and accumulation over strips
BIG_SHAPES = [(1100, 2, 24, 256), (128, 3, 256, 256)]
# the guide seed: seed 0 meets `conditions` at margin 0 for every shape above. The margins of MARGINS pull the bound into the
# guide's in-cluster scores, and there the masks are decided (all four settings, gap 2.1e-3) by MARGIN_SHAPE with MARGIN_SEED,
# the first of 1,500 seeds to pass MIN_GAP twice over (searched once on the CPU; nothing is re-drawn at run time)
GUIDE_SEED = 0
MARGIN_SHAPE, MARGIN_SEED = (33, 4, 768, 384), 1407
MARGINS = [("absolute", 0.0), ("absolute", 0.1), ("relative", 0.0), ("relative", 0.1)]
MIN_GAP = 1e-3
TEMPERATURES = [0.05, 0.01]


def sim_matrix(u, v):
    return F.normalize(u, p=2, dim=1, eps=1e-12) @ F.normalize(v, p=2, dim=1, eps=1e-12).t()


def gist_blocks(cols):
    """The score blocks of K columns in upstream's order: ap, aa, pp, an_1 ..."""
    a, p = cols[0], cols[1]
    return [sim_matrix(a, p), sim_matrix(a, a), sim_matrix(p, p)] + [sim_matrix(a, n) for n in cols[2:]]


def gist_masks(guide_cols, margin_strategy="absolute", margin=0.0):
    """(masks, gaps) per block: what upstream removes, and |guide entry - bound_i| (the ap diagonal, kept by index, at inf)."""
    blocks = gist_blocks(guide_cols)
    thr = blocks[0].diagonal().view(-1, 1)
    bound = thr - margin if margin_strategy == "absolute" else thr * (1 - margin)
    eye = torch.eye(thr.shape[0], dtype=torch.bool, device=thr.device)
    masks, gaps = [], []
    for idx, gb in enumerate(blocks):
        mask = gb > bound
        gap = (gb - bound).abs()
        if idx == 0:
            mask = mask & ~eye
            gap = gap.masked_fill(eye, float("inf"))
        masks.append(mask)
        gaps.append(gap)
    return masks, gaps


def gist_ref(cols, guide_cols, temperature=0.01, margin_strategy="absolute", margin=0.0):
    """GISTEmbedLoss.forward of sentence-transformers on embeddings: cols / guide_cols are the K columns [B, D] / [B, Dg]."""
    masks, _ = gist_masks([g.detach() for g in guide_cols], margin_strategy, margin)
    scores = []
    for sim_mat, mask in zip(gist_blocks(cols), masks):
        sim_mat[mask] = -torch.inf
        scores.append(sim_mat)
    scores = torch.cat(scores, dim=1) / temperature
    return F.cross_entropy(scores, torch.arange(scores.shape[0], device=scores.device))


def student_case(B, K, D, seed):
    """K columns [B, D] fp32, drawn as mnrl_helpers.case draws anchors and candidates for cos: unit rows, then a length of its
    own in [0.5, 2] for every row. Untrained: at temperature 0.01 positives pulled towards their anchors would saturate the
    softmax and let a wrong gradient hide behind zeros."""
    a, c = M.case(B, (K - 1) * B, D, "cos", False, seed)
    return [a] + list(c.chunk(K - 1, 0))


def guide_case(B, K, Dg, seed):
    """K guide columns [B, Dg] fp32 whose masks are decided. Clusters of four examples share a centre (in-cluster anchor cosine
    about 0.9); positives alternate between far from their anchor (thr_i about 0.67: the row masks its cluster) and next to it
    (thr_i about 0.99: the row masks next to nothing), and the far ones share a second centre so that pp has masked entries
    too; hard negatives sit between."""
    g = torch.Generator().manual_seed(seed)

    def unit(n):
        return F.normalize(torch.randn(n, Dg, generator=g, dtype=torch.float64), dim=1)

    cl = torch.arange(B) // 4
    ncl = int(cl.max()) + 1
    c1, c2 = unit(ncl), unit(ncl)
    a = F.normalize(c1[cl] + 0.3 * unit(B), dim=1)
    far = (torch.arange(B) % 2 == 0).view(-1, 1)
    u = F.normalize(c2[cl] + 0.3 * unit(B), dim=1)
    p = torch.where(far, F.normalize(a + 1.1 * u, dim=1), F.normalize(a + 0.15 * unit(B), dim=1))
    cols = [a, p] + [F.normalize(a + 0.35 * unit(B), dim=1) for _ in range(K - 2)]
    return [(x * (0.5 + 1.5 * torch.rand(B, 1, generator=g, dtype=torch.float64))).float() for x in cols]


def case(B, K, D, Dg, seed=GUIDE_SEED):
    return student_case(B, K, D, 1000 * B + D), guide_case(B, K, Dg, seed)


def reference_of(cols, guide_cols, temperature, margin_strategy="absolute", margin=0.0):
    """(loss, [grad per column]) of the fp64 CPU reference with autograd on the fp32 inputs."""
    c64 = [c.double().clone().requires_grad_(True) for c in cols]
    loss = gist_ref(c64, [g.double() for g in guide_cols], temperature, margin_strategy, margin)
    loss.backward()
    return loss.detach(), [c.grad for c in c64]


def conditions(cols, guide_cols, temperature, margin_strategy="absolute", margin=0.0):
    """Asserts what a case must show (see the module docstring) and returns (min gap, masked share per block)."""
    B = cols[0].shape[0]
    m64, gaps = gist_masks([g.double() for g in guide_cols], margin_strategy, margin)
    m32, _ = gist_masks(guide_cols, margin_strategy, margin)
    min_gap = min(float(gp.min()) for gp in gaps)
    assert min_gap >= MIN_GAP, f"guide entry within {min_gap:.2e} of its bound"
    assert all(torch.equal(x, y) for x, y in zip(m64, m32)), "fp32 and fp64 masks differ"
    shares = [float(m.double().mean()) for m in m64]
    if B >= 8:
        off = ~torch.eye(B, dtype=torch.bool)
        for name, m, share in zip(block_names(len(cols)), m64, shares):
            assert bool(m[off].any()) and bool((~m)[off].any()), f"block {name}: masked and unmasked off-diagonal entries"
            assert share <= 0.6, f"block {name}: {share:.0%} masked"
    if B > 1:
        loss, grads = reference_of(cols, guide_cols, temperature, margin_strategy, margin)
        gmax = max(float(g.abs().max()) for g in grads)
        assert float(loss) >= M.MIN_REF_LOSS and gmax >= M.MIN_REF_GRAD, (float(loss), gmax)
    return min_gap, shares


def block_names(K):
    return ["ap", "aa", "pp"] + [f"an{k}" for k in range(1, K - 1)]


@functools.lru_cache(maxsize=None)
def reference(B, K, D, Dg, temperature, margin_strategy="absolute", margin=0.0, seed=GUIDE_SEED):
    """The inputs of a case and their reference, computed once and shared (nobody writes to them):
    (x [K * B, D], g [K * B, Dg], loss, grad_x [K * B, D])."""
    cols, guide_cols = case(B, K, D, Dg, seed)
    conditions(cols, guide_cols, temperature, margin_strategy, margin)
    loss, grads = reference_of(cols, guide_cols, temperature, margin_strategy, margin)
    return torch.cat(cols, 0), torch.cat(guide_cols, 0), loss, torch.cat(grads, 0)
