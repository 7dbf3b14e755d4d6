"""The yardstick of community detection (tests/test_community_host.py, tests/test_gpu_community.py): the contract of
util.community_detection written out plainly in fp64, and inputs whose cosines are exact. numpy only, so the host tests
import it without the library. Imported like topk_stream_cases, not a conftest.

The contract (sentence-transformers 2.2.2 restated): S = the cosine matrix of the rows (norms clamped at 1e-12),
N(i) = {j : S[i, j] >= threshold} (a NaN passes nothing); row i is a candidate when |N(i)| >= min_size; candidates go by
(|N(i)| descending, i ascending); one is accepted when none of its members was accepted before, and then returned whole;
inside a community the candidate row first when it is a member, the rest by (score descending, row ascending).
"""
import numpy as np


def cosine_ref(emb):
    """fp64 [n, n]: dot products over the product of the clamped norms. For rows of +-1 the dot products are integers
    and the norms equal, so equal cosines are equal numbers."""
    e = np.asarray(emb, dtype=np.float64)
    nrm = np.maximum(np.sqrt((e * e).sum(1)), 1e-12)
    with np.errstate(invalid="ignore"):
        return (e @ e.T) / np.outer(nrm, nrm)


def counts_ref(emb, threshold):
    with np.errstate(invalid="ignore"):
        return (cosine_ref(emb) >= threshold).sum(1).astype(np.int64)


def members_ref(emb, threshold):
    """Per row the ascending list of its members."""
    with np.errstate(invalid="ignore"):
        ok = cosine_ref(emb) >= threshold
    return [np.flatnonzero(r) for r in ok]


def community_ref(emb, threshold, min_size, want_trace=False):
    """The accepted communities, list of lists of int. want_trace: also (candidates, rejected) counts."""
    s = cosine_ref(emb)
    n = len(s)
    cand = []
    for i in range(n):
        with np.errstate(invalid="ignore"):
            mem = [j for j in range(n) if s[i, j] >= threshold]
        if len(mem) >= min_size:
            cand.append((i, mem))
    cand.sort(key=lambda t: (-len(t[1]), t[0]))
    taken, out, rejected = set(), [], 0
    for i, mem in cand:
        if any(j in taken for j in mem):
            rejected += 1
            continue
        taken.update(mem)
        rest = sorted((j for j in mem if j != i), key=lambda j: (-s[i, j], j))
        out.append(([i] if i in mem else []) + rest)
    return (out, len(cand), rejected) if want_trace else out


def planted(sizes, dim, maxflip, noise, seed):
    """+-1 rows, fp32 [sum(sizes) + noise, dim]: one random centre per cluster, its members the centre with 1 .. maxflip
    signs flipped, plus `noise` random rows, then permuted. Every row has norm sqrt(dim): every cosine is an integer
    multiple of 1 / dim, and with threshold = 1 - (2k + 1) / dim none is nearer to the threshold than 1 / dim."""
    rng = np.random.RandomState(seed)
    rows = []
    for size in sizes:
        centre = rng.choice([-1.0, 1.0], size=dim)
        for _ in range(size):
            r = centre.copy()
            flip = rng.choice(dim, size=rng.randint(1, maxflip + 1), replace=False)
            r[flip] *= -1.0
            rows.append(r)
    for _ in range(noise):
        rows.append(rng.choice([-1.0, 1.0], size=dim))
    e = np.asarray(rows, dtype=np.float32)
    return e[rng.permutation(len(e))]


def threshold_for(k, dim):
    """Rows of +-1 differing in at most k places pass, k + 1 do not: halfway between the two cosines."""
    return 1.0 - (2 * k + 1) / dim


def margin(emb, threshold):
    """The distance of the nearest fp64 cosine to the threshold (NaN scores aside). Tests that compare memberships first
    assert margin >= 1e-3: a condition on the inputs, not a tolerance on the kernel."""
    d = np.abs(cosine_ref(emb) - threshold)
    return float(np.nanmin(d))


# the three planted cases the device result is compared on list for list: (dim, sizes, maxflip, noise, k, min size)
PLANTED = {
    "d96_k12": (96, [40, 25, 12, 9, 30], 12, 41, 12, 10),
    "d96_k6": (96, [40, 25, 12, 9, 30], 12, 41, 6, 3),
    "d384_k40": (384, [300, 200, 120, 64, 33, 10, 9], 40, 294, 40, 10),
}
SEED = 7


def planted_case(name):
    """(emb, threshold, min size) of a PLANTED case."""
    dim, sizes, maxflip, noise, k, min_size = PLANTED[name]
    return planted(sizes, dim, maxflip, noise, SEED), threshold_for(k, dim), min_size


def emulate(emb, threshold, min_size, budget, plan, order_fn):
    """util.community_detection with the device taken out: counts and members from the reference, the claim in numpy, the
    rounds from `plan` (util.plan_community_round) over `order_fn` (util.community_order). Returns the accepted
    communities as sorted member lists in acceptance order, and the number of rounds."""
    mem = members_ref(emb, threshold)
    counts = np.array([len(m) for m in mem], dtype=np.int64)
    self_member = np.array([i in set(m.tolist()) for i, m in enumerate(mem)], dtype=bool)
    order = order_fn(counts, min_size)
    taken = np.zeros(len(mem), dtype=bool)
    out, start, rounds = [], 0, 0
    while start < len(order):
        picked, start = plan(order, counts, self_member, taken, start, budget)
        if len(picked) == 0:
            break
        rounds += 1
        for i in picked:
            if not taken[mem[i]].any():
                taken[mem[i]] = True
                out.append(sorted(int(j) for j in mem[i]))
    return out, rounds
