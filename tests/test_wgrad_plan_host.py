"""CPU: the M-range plan of the grouped weight-gradient launch (qst_tn_group_ranges, csrc/gemm.hip), no device needed.

The launch cuts the reduction over M into `splits` ranges of whole 64-row stages and, with one range per XCD, may skew their
lengths by off(x) * skew stages (off = -4, -3, -2, -1, +1, +2, +3, +4) so that the XCDs flush at different times. The kernel
takes its ranges from the same function, so what holds here holds for the launch: the ranges tile [0, M) exactly.
"""
import ctypes as C

import pytest

import quadruplet_sentence_transformer_amd  # noqa: F401
from quadruplet_sentence_transformer_amd import _lib

OFF = [-4, -3, -2, -1, 1, 2, 3, 4]
MS = [96, 777, 2543, 2560, 32768, 196608]
SPLITS = [0, 8, 16]
SKEWS = [-1, 0, 1, 2, 9, 1000]


def plan(M, splits, skew, order=0, N=384, K=384):
    lib = _lib.load()
    grp = _lib.QstTnGroup()
    grp.nprob, grp.splits, grp.skew, grp.order = 1, splits, skew, order
    q = grp.prob[0]
    q.M, q.N, q.K, q.lda, q.ldb, q.ldc = M, N, K, N, K, K
    n = max(8, (splits + 7) // 8 * 8)
    begins = (C.c_int32 * (n + 1))()
    eff = lib.qst_tn_group_ranges(grp, begins)
    assert eff >= 0, eff
    return eff, list(begins), n


@pytest.mark.parametrize("skew", SKEWS)
@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("M", MS)
def test_ranges_tile_the_rows_exactly(M, splits, skew):
    eff, b, n = plan(M, splits, skew)
    assert len(b) == n + 1 and b[0] == 0 and b[-1] == M
    assert all(b[i] <= b[i + 1] for i in range(n))
    assert all(x % 64 == 0 for x in b[1:-1])
    lens = [b[i + 1] - b[i] for i in range(n)]
    assert sum(lens) == M
    if M >= 64 * n:
        assert min(lens) >= 64
    # equal ranges: what skew < 0 gives -- lengths within one stage of each other
    _, beq, _ = plan(M, splits, -1)
    leq = [beq[i + 1] - beq[i] for i in range(n)]
    stages_eq = [(x + 63) // 64 for x in leq]
    assert max(stages_eq) - min(stages_eq) <= 1
    if skew < 0 or n == 16:
        assert eff == 0 and b == beq
    # the clamp: the shortest range keeps a stage; where M is too small for that, no skew at all
    if skew > 0 and n == 8:
        assert eff == min(skew, max(0, (min(stages_eq) - 1) // 4))
    # the skewed lengths are the equal ones moved by off(x) * skew whole stages (the ragged rows stay in the last range), and
    # sum to the unskewed total
    if n == 8:
        assert [lens[x] - leq[x] for x in range(8)] == [64 * OFF[x] * eff for x in range(8)]
    assert sum(lens) == sum(leq)


def test_explicit_plans():
    """the cases the GPU tests rely on, spelled out"""
    assert plan(2560, 0, 1) == (1, [0, 64, 192, 384, 640, 1024, 1472, 1984, 2560], 8)     # 1, 2, 3, 4, 6, 7, 8, 9 stages
    assert plan(2560, 0, 9)[:2] == plan(2560, 0, 1)[:2]                                   # clamped to 1
    eff, b, _ = plan(2560 - 17, 0, 1)
    assert eff == 1 and b[-2:] == [1984, 2543]                                             # ragged last stage in the longest range
    eff, b, _ = plan(96, 0, 3)
    assert eff == 0 and sum(1 for i in range(8) if b[i + 1] > b[i]) == 2                  # two non-empty ranges, no skew
    eff, b, _ = plan(512, 0, 0, order=2)
    assert [b[i + 1] - b[i] for i in range(8)] == [64] * 8                                 # one stage per range
    assert plan(32768, 0, -1)[1] == [4096 * i for i in range(9)]
    assert plan(32768, 0, 2)[1][1] == 4096 - 8 * 64


def test_auto_skew_is_a_valid_plan():
    """skew = 0 asks for the library's choice: whatever it picks per shape class, it reports it and the plan is one of the
    explicit ones"""
    for M in MS:
        for N, K in [(384, 384), (768, 3072), (1152, 1152)]:
            eff, b, _ = plan(M, 0, 0, N=N, K=K)
            assert b == plan(M, 0, eff if eff > 0 else -1, N=N, K=K)[1]


def test_bad_arguments():
    lib = _lib.load()
    grp = _lib.QstTnGroup()
    begins = (C.c_int32 * 9)()
    assert lib.qst_tn_group_ranges(grp, begins) < 0               # nprob = 0
    assert lib.qst_tn_group_ranges(None, begins) < 0
    grp.nprob = 1
    grp.prob[0].M, grp.prob[0].N, grp.prob[0].K = 0, 384, 384
    assert lib.qst_tn_group_ranges(grp, begins) < 0
