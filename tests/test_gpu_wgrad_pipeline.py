"""The grouped weight-gradient kernel (csrc/gemm.hip, gemm_tn_group_kernel) at the edges of its operand pipeline.

The loader waves keep two stages of 64 reduction rows in flight into a three-slot LDS ring while the MFMA waves read the third
(a variant with two to four more stages on their way through the loaders' registers was measured and is kept as
tools/experiments/tn_reg_stages.patch: these cases cover its pipeline as well, at most six stages deep). A piece of work sees
the prologue, the steady state and the drain of that pipeline according to its number of stages, and the MFMA waves walk the
ring's slots with a running address. With splits = 0 the reduction is cut into 8 ranges, 32 workgroups each: M = 8 * 64 * S
gives every whole tile S stages, the leftover tiles are cut into one-stage pieces, and some workgroups get none.

Reference: fp32 A^T . B of the operands rounded to the kernel's operand type, on the CPU. Tolerances: those of
test_gemm_tn_wgrad (rtol 1e-3, atol 1e-3 * sqrt(M); the column sums alike); after two launches into the same C both errors
add up, so 2e-3 * sqrt(M).
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from quadruplet_sentence_transformer_amd import _lib  # noqa: E402
from kernel_helpers import OPDT, gemm_args, kf, lib, op, opr, stream  # noqa: E402,F401


@pytest.fixture(autouse=True)
def tiled(lib):
    """the tiled kernel of csrc/gemm.hip, whatever qst_gemm8_mode was left at"""
    lib.qst_gemm8_mode(0)
    yield
    lib.qst_gemm8_mode(-1)


@functools.lru_cache(maxsize=None)
def problem(op, M, N, K):
    """dY [M, N] and X [M, K] rounded to the operand type, their device copies, dY^T . X and the column sums of dY"""
    g = torch.Generator().manual_seed(M * 3 + N + K)
    A = opr(op, torch.randn(M, N, generator=g))
    B = opr(op, torch.randn(M, K, generator=g))
    return A.to(OPDT[op]).cuda(), B.to(OPDT[op]).cuda(), A.t() @ B, A.sum(0)


def launch(lib, op, Ad, Bd, C, cs, M, N, K):
    _lib.check(kf(lib, "qst_gemm_tn", op)(gemm_args(A=Ad, B=Bd, C=C, colsum=cs, M=M, N=N, K=K, lda=N, ldb=K, ldc=K, splits=0),
                                           stream()))


def check(lib, op, M, N, K, launches=1):
    Ad, Bd, ref, rcs = problem(op, M, N, K)
    C = torch.zeros(N, K, dtype=torch.float32, device="cuda")
    cs = torch.zeros(N, dtype=torch.float32, device="cuda")
    for _ in range(launches):
        launch(lib, op, Ad, Bd, C, cs, M, N, K)
    atol = launches * 1e-3 * math.sqrt(M)
    torch.testing.assert_close(C.cpu(), launches * ref, rtol=1e-3, atol=atol)
    torch.testing.assert_close(cs.cpu(), launches * rcs, rtol=1e-3, atol=atol)


@pytest.mark.parametrize("ragged", [0, 17], ids=["whole", "ragged"])
@pytest.mark.parametrize("S", range(1, 9))
def test_short_stage_counts(lib, op, S, ragged):
    """36 tiles on 32 workgroups per range: one whole tile of S stages each -- fewer than, as many as and more than the
    stages the pipeline holds -- then one-stage pieces of the four leftover tiles (S < 8: some workgroups get an empty
    piece). M - 17: the last stage of the last range is ragged, and that range is shorter than the others."""
    check(lib, op, 8 * 64 * S - ragged, 1152, 1152)


def test_fewer_tiles_than_workgroups(lib, op):
    """one tile, five stages per range, 32 workgroups: every workgroup that works runs a single-stage piece"""
    check(lib, op, 8 * 64 * 5, 192, 192)


@pytest.mark.parametrize("N,K", [(192, 192), (1152, 1152)])
def test_empty_ranges(lib, op, N, K):
    """M = 96: two ranges of 64 and 32 rows, six empty ones"""
    check(lib, op, 96, N, K)


def test_width_not_a_multiple_of_the_tile(lib, op):
    """lanes past the operand's width take the out-of-range offset (zero fill) in every one of the twelve loads of a stage"""
    check(lib, op, 777, 200, 136)


@pytest.mark.parametrize("M,N,K", [(8 * 64 * 1, 1152, 1152), (8 * 64 * 3 - 17, 1152, 1152), (8 * 64 * 5, 1152, 1152),
                                   (8 * 64 * 5, 192, 192), (777, 200, 136)])
def test_back_to_back_launches_accumulate(lib, op, M, N, K):
    """two launches into the same C with nothing in between: C doubles, and nothing a task left in flight or in the ring
    reaches the next task or the next launch"""
    check(lib, op, M, N, K, launches=2)


def test_grouped_minilm_layer(lib, op):
    """all four weight gradients of a MiniLM-shaped layer in one launch, M = 2560 - 17: 48 tiles of five stages (the last
    stage of the last range ragged) on 32 workgroups -- one whole tile each, then the 16 left over in pieces of 3 + 2 stages"""
    M, H, I = 2560 - 17, 384, 1536
    shapes = [(H, I), (I, H), (H, H), (3 * H, H)]
    grp = _lib.QstTnGroup()
    grp.nprob, grp.splits = 4, 0
    outs = []
    for i, (N, K) in enumerate(shapes):
        Ad, Bd, ref, rcs = problem(op, M, N, K)
        C = torch.ones(N, K, device="cuda")                    # accumulation semantics: C += A^T . B
        cs = torch.zeros(N, device="cuda")
        q = grp.prob[i]
        q.A, q.B, q.C, q.colsum = Ad.data_ptr(), Bd.data_ptr(), C.data_ptr(), cs.data_ptr()
        q.M, q.N, q.K, q.lda, q.ldb, q.ldc = M, N, K, N, K, K
        outs.append((C, cs, ref + 1.0, rcs))
    _lib.check(kf(lib, "qst_gemm_tn_group", op)(grp, stream()))
    torch.cuda.synchronize()
    for C, cs, ref, rcs in outs:
        torch.testing.assert_close(C.cpu(), ref, rtol=1e-3, atol=1e-3 * math.sqrt(M))
        torch.testing.assert_close(cs.cpu(), rcs, rtol=1e-3, atol=1e-3 * math.sqrt(M))
