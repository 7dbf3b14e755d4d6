"""The yardstick of qst_quadruplet_eval and QuadrupletEvaluator (tests/test_gpu_quadruplet_eval.py,
tests/test_quadruplet_eval_host.py): the nine fp64 distances of a row written exactly as TripletEvaluator writes them, the
nine comparisons, and the rows on which fp32 and fp64 may rightly disagree. Imported like tuple_loss_helpers, not a conftest.

Index k = 3 * metric + j: metric 0 cosine, 1 Manhattan, 2 Euclidean (the column order of TripletEvaluator's CSV); in the
distances j is the pair (a, p), (a, q), (a, n), in the comparisons j is pos_part d(a, p) < d(a, q), pos_neg d(a, p) < d(a, n),
part_neg d(a, q) < d(a, n).
"""
import numpy as np
import torch
import torch.nn.functional as F

import tuple_loss_helpers as H

LEVELS = (0.3, 0.6, 0.9, 1.2, 1.5)
METRICS = (H.COS_DIST, H.L1_PLAIN, H.L2_PLAIN)      # the kernel's metric of each block of three, for value_tol
LONG_SHAPES = [(2500, 33), (2500, 64), (2500, 384)]  # past one and two trips of the counting stage (1024 rows a trip)
PAIRS = ((0, 1), (0, 2), (1, 2))                     # comparison j holds when distance PAIRS[j][0] < distance PAIRS[j][1]


def case(B, D, seed):
    """a = unit rows drawn in fp64; each of p, q, n = normalize(a + s * normalize(noise)) with the three s of a row a random
    choice of three distinct LEVELS, so that every order of the three distances occurs and no two are close; cast to fp32."""
    g = torch.Generator().manual_seed(seed)
    a = F.normalize(torch.randn(B, D, generator=g, dtype=torch.float64), dim=1)
    pick = torch.rand(B, len(LEVELS), generator=g).argsort(dim=1)[:, :3]
    s = torch.tensor(LEVELS, dtype=torch.float64)[pick]                       # [B, 3]
    out = [a]
    for i in range(3):
        noise = F.normalize(torch.randn(B, D, generator=g, dtype=torch.float64), dim=1)
        out.append(F.normalize(a + s[:, i:i + 1] * noise, dim=1))
    return [t.to(torch.float32) for t in out]


def ref(a, p, q, n):
    """(dist fp64 [B, 9], holds bool [B, 9]) of four [B, D] arrays or tensors."""
    a, p, q, n = [np.asarray(t.cpu() if torch.is_tensor(t) else t, dtype=np.float64) for t in (a, p, q, n)]

    def cosd(x, y):
        return 1.0 - (x * y).sum(1) / (np.linalg.norm(x, axis=1) * np.linalg.norm(y, axis=1) + 1e-30)

    cols = [cosd(a, x) for x in (p, q, n)]
    cols += [np.abs(a - x).sum(1) for x in (p, q, n)]
    cols += [np.linalg.norm(a - x, axis=1) for x in (p, q, n)]
    dist = np.stack(cols, axis=1)
    holds = np.stack([dist[:, 3 * m + lo] < dist[:, 3 * m + hi] for m in range(3) for lo, hi in PAIRS], axis=1)
    return dist, holds


def gaps(dist):
    """|difference| of the two fp64 distances each of the nine comparisons is made on, [B, 9]."""
    return np.stack([np.abs(dist[:, 3 * m + lo] - dist[:, 3 * m + hi]) for m in range(3) for lo, hi in PAIRS], axis=1)


def close_rows(dist, D):
    """bool [B]: rows where any of the nine gaps is below five times the error the project accepts on that distance
    (tuple_loss_helpers.value_tol; the L1 tolerance for Manhattan) -- there fp32 may fall on the other side."""
    tol = np.repeat([5 * H.value_tol(m, D) for m in METRICS], 3)
    return (gaps(dist) < tol[None, :]).any(axis=1)


def accuracies(holds):
    """[3 comparisons][3 metrics]: for comparison j the accuracies under cosine, Manhattan, Euclidean."""
    acc = np.asarray(holds, dtype=np.float64).mean(axis=0).reshape(3, 3)      # [metric, comparison]
    return [[float(acc[m, j]) for m in range(3)] for j in range(3)]
