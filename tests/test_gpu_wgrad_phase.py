"""The grouped weight-gradient kernel (csrc/gemm.hip, gemm_tn_group_kernel) under the two knobs that schedule its flushes:
QstTnGroup.skew (M-ranges of unequal length, one per XCD, so that the XCDs flush at different times) and QstTnGroup.order
(2: the workgroups with an odd leftover-piece index run that piece before their whole tile). Both move range boundaries and
task order only: every row must still be reduced exactly once into every tile.

Reference: fp32 A^T . B of the operands rounded to the kernel's operand type, on the CPU. Tolerances: those of
test_gpu_wgrad_pipeline (rtol 1e-3, atol 1e-3 * sqrt(M), the column sums alike; doubled for two launches into the same C).
The exact cases draw the operands from the integers -2 .. 2: every product and every partial sum is an integer below
4 * 2560 < 2^24, so fp32 sums are exact in any grouping and the result must EQUAL the reference -- a row counted twice or
dropped at a moved boundary changes an element by up to 4, far inside the tolerance above.
"""
import pytest

pytestmark = pytest.mark.gpu

import wgrad_helpers  # noqa: E402
from kernel_helpers import kf, lib, op  # noqa: E402,F401

LAYER = [(384, 1536), (1536, 384), (384, 384), (1152, 384)]         # dW2, dW1, dWo, dWqkv of a MiniLM layer: 48 tiles


@pytest.fixture(autouse=True)
def tiled(lib):
    """the tiled kernel of csrc/gemm.hip, whatever qst_gemm8_mode was left at"""
    lib.qst_gemm8_mode(0)
    yield
    lib.qst_gemm8_mode(-1)


def run(lib, op, M, shapes, skew, order, **kw):
    return wgrad_helpers.run(kf(lib, "qst_gemm_tn_group", op), op, M, shapes, skew, order, **kw)


def effective_skew(lib, grp):
    return wgrad_helpers.effective_skew(lib.qst_tn_group_ranges, grp)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("skew", [1, 9])
@pytest.mark.parametrize("ragged", [0, 17], ids=["whole", "ragged"])
def test_skewed_ranges_around_the_ring_depth(lib, op, ragged, skew, order):
    """M = 2560: five stages per equal range, so skew 1 gives ranges of 1, 2, 3, 4, 6, 7, 8, 9 stages -- shorter than, as long
    as and longer than the three stages the ring holds, in one launch; 36 tiles on 32 workgroups: a whole tile each, then
    pieces of the four leftover tiles. M - 17: the last stage of the longest range is ragged. skew 9 must be clamped to 1."""
    M = 2560 - ragged
    grp = run(lib, op, M, [(1152, 1152)], skew, order)
    eff, b = effective_skew(lib, grp)
    assert eff == 1 and b == [0, 64, 192, 384, 640, 1024, 1472, 1984, M]


def test_too_few_rows_to_skew(lib, op):
    """M = 96: two non-empty ranges of one stage, so the skew falls back to 0"""
    grp = run(lib, op, 96, [(1152, 1152)], 3, 1)
    eff, b = effective_skew(lib, grp)
    assert eff == 0 and sum(1 for i in range(8) if b[i + 1] > b[i]) == 2


def test_empty_pieces_come_first(lib, op):
    """M = 512, order 2: one stage per range, the leftover tiles are cut into two pieces of which the second -- the odd one,
    which now runs FIRST -- is empty"""
    run(lib, op, 512, [(1152, 1152)], -1, 2)
    run(lib, op, 512, LAYER, -1, 2)


@pytest.mark.parametrize("order", [1, 2])
def test_every_row_is_reduced_exactly_once(lib, op, order):
    """integer operands, exact sums: C and the column sums EQUAL the reference"""
    run(lib, op, 2560 - 17, [(1152, 1152)], 1, order, ints=True)
    run(lib, op, 2560 - 17, LAYER, 1, order, ints=True)


@pytest.mark.parametrize("launches", [1, 2])
@pytest.mark.parametrize("order", [1, 2])
def test_grouped_minilm_layer_skewed(lib, op, order, launches):
    """all four weight gradients of a MiniLM-shaped layer, M = 2560 - 17, 48 tiles on 32 workgroups (one whole tile each and the
    16 left over in two pieces), C preset to ones, skew 1; two launches back to back into the same C"""
    run(lib, op, 2560 - 17, LAYER, 1, order, launches=launches, preset=1.0)
