"""The grouped weight-gradient kernels (csrc/gemm.hip gemm_tn_group_kernel, csrc/gemm8.hip gemm_tn8_group_kernel) across the
classes of their work decomposition, kernel level and EXACT.

T tiles over the W workgroups of an M-range are a = T / W whole tiles per workgroup and b = T % W leftover tiles cut into
max(1, W / b) stage pieces; workgroups past b * pieces run no piece; the order decides who takes which piece, and when; a walk
over the group's tile counts finds the problem of a flat tile index; lanes past an operand's width are zero-filled. Which of
these a launch meets depends on the layer's width: test_gpu_wgrad_pipeline and test_gpu_wgrad_phase reach four classes (the
MiniLM layer and three single problems), every other width ran the grouped launch only inside whole encoders, at 1.65e-2
relative L2 per tensor -- where a row counted twice in one piece of one tile does not show. The case table and what each
entry is there for: tests/wgrad_helpers.py, kept honest by tests/test_wgrad_cases_host.py.

Reference: fp32 dY^T . X and column sums of dY, by torch on the CPU. Operands from the integers -2 .. 2: every product and
partial sum is an integer below 4 * 8192 < 2^24, fp32 sums are exact in any grouping, and C (preset to an integer, so that the
accumulation is checked too) and the column sums must EQUAL the reference: rtol = atol = 0. One case (H) runs Gaussian
operands at the bound of test_gpu_wgrad_pipeline, rtol 1e-3 and atol 1e-3 * sqrt(M): small integers leave most of the 16-bit
mantissa unused, and a fragment-layout error that mixes up elements of equal value would hide behind them.

Paths: qst_gemm_tn_group on the tiled kernel (qst_gemm8_mode 0) with order 1 and 2, and qst_gemm_tn8_group by name.
"""
import pytest

pytestmark = pytest.mark.gpu

import wgrad_helpers as W  # noqa: E402
from kernel_helpers import kf, lib, op  # noqa: E402,F401


@pytest.fixture(autouse=True)
def tiled(lib):
    """qst_gemm_tn_group runs the tiled kernel of csrc/gemm.hip, whatever qst_gemm8_mode was left at"""
    lib.qst_gemm8_mode(0)
    yield
    lib.qst_gemm8_mode(-1)


PATHS = [("tiled", 1), ("tiled", 2), ("eightphase", 0)]


@pytest.fixture(params=PATHS, ids=["tiled-order1", "tiled-order2", "eightphase"])
def path(request):
    return request.param


def run(lib, op, path, M, shapes, skew=1, **kw):
    """the exact run on one path: integer operands, C preset to 1 (the skew and the order are the tiled kernel's: the 8-phase
    one cuts equal ranges and runs its pieces last)"""
    kernel, order = path
    if kernel == "eightphase":
        entry = kf(lib, "qst_gemm_tn8_group", op)
    else:
        entry = kf(lib, "qst_gemm_tn_group", op)
    kw.setdefault("ints", True)
    kw.setdefault("preset", 1.0)
    return W.run(entry, op, M, shapes, skew, order, **kw)


# ------------------------------------------------------------------ A: layer mixes by width class
@pytest.mark.parametrize("H,I,M", W.CASES_A, ids=[f"H{H}" for H, _, _ in W.CASES_A])
def test_layer_of_every_width_class(lib, op, path, H, I, M):
    """the four gradients of a layer at every width class the library accepts. H <= 512: five stages per range, the last
    ragged, skew 1 on the tiled path -- ranges of 1, 2, 3, 4, 6, 7, 8 and 9 stages, fewer than the pieces of a leftover tile in
    some and more in others; H = 768, 1024: two stages per range. Classes (tiled): no whole tile (64, 128), a = 1 (256, 320),
    a >= 2 and then a piece (448: uncut leftovers and idle workgroups; 512, 1024), a = 6 and no leftover (768: the mpnet and
    bert-base layer); the tile walk crosses problems ragged in N or K everywhere but at 768. The 128 x 384 tile of the 8-phase
    kernel turns the same widths into other classes (256: 22 tiles, none whole, uncut, ten workgroups idle; 320: one leftover
    tile in 32 pieces)."""
    run(lib, op, path, M, W.layer(H, I))


# ------------------------------------------------------------------ B: two or more ranges per XCD
@pytest.mark.parametrize("splits,HI", W.CASES_B, ids=[f"splits{s}-H{HI[0]}" for s, HI in W.CASES_B])
def test_several_ranges_per_xcd(lib, op, path, splits, HI):
    """splits = 16 and 24: two and three ranges per XCD, 16 and 10 workgroups each. 16 workgroups make the MiniLM layer three
    whole tiles and no leftover, and the 448 layer five whole tiles and ten uncut leftovers. A skew is asked for and must
    not be applied: it is defined for one range per XCD only."""
    grp = run(lib, op, path, W.M_FIVE, W.layer(*HI), skew=1, splits=splits)
    eff, b = W.effective_skew(lib.qst_tn_group_ranges, grp)
    assert eff == 0, f"skew {eff} in effect with {splits} ranges"
    assert len(b) == splits + 1 and b[0] == 0 and b[-1] == W.M_FIVE and all(x <= y for x, y in zip(b, b[1:]))


# ------------------------------------------------------------------ C: leading dimensions and guard bands
def test_leading_dimensions_and_guard_bands(lib, op, path):
    """the (320, 1280) group -- ragged in N and in K -- at M = 777, each operand a view [:M, 40 : 40 + width] of a matrix
    [M + 64, width + 72] of ONES (lda = N + 72, ldb = K + 72), C [N + 1, K + 8] with ldc = K + 8 and a colsum of N + 8
    elements, both preset to 7. Products and sums equal the reference of the view; every guard element still holds 7. The
    dense zero-fill case (777, 200, 136) cannot tell a read past the width from a correct one where the neighbours are the
    next row's own data or the end of the allocation, nor a row stride taken from the width."""
    run(lib, op, path, 777, W.layer(320, 1280), padded=True, preset=7.0, cs_preset=7.0)


# ------------------------------------------------------------------ D: colsum == NULL, nprob
def test_colsum_null_on_some_problems(lib, op, path):
    """the (128, 512) group without colsum on problems 0 and 2: the other two still get their exact sums"""
    run(lib, op, path, W.M_FIVE, W.layer(128, 512), no_colsum=(0, 2))


@pytest.mark.parametrize("M,shapes", W.CASES_NPROB, ids=[f"nprob{len(s)}" for _, s in W.CASES_NPROB])
def test_problem_counts(lib, op, path, M, shapes):
    """nprob = 8 (the (64, 256) layer's gradients, then the (128, 512) layer's), 2 (a one-tile problem in front of a
    36-tile one) and 3 (ragged, whole, ragged): the tile walk over other counts than 1 and 4"""
    run(lib, op, path, M, shapes)


# ------------------------------------------------------------------ E: few rows
@pytest.mark.parametrize("HI", W.FEW_ROWS_LAYERS, ids=[f"H{H}" for H, _ in W.FEW_ROWS_LAYERS])
@pytest.mark.parametrize("M", W.FEW_ROWS)
def test_few_rows(lib, op, path, M, HI):
    """M = 1, 63 (one ragged stage: seven empty ranges, and fewer (tile, stage) pairs than workgroups on the small layer), 65
    (a stage and a row) and 520 (eight stages and a ragged ninth). skew 3 on the tiled path must fall back to equal ranges."""
    grp = run(lib, op, path, M, W.layer(*HI), skew=3)
    eff, b = W.effective_skew(lib.qst_tn_group_ranges, grp)
    assert eff == 0 and b[0] == 0 and b[-1] == M


# ------------------------------------------------------------------ F: the library's own skew and order
@pytest.mark.parametrize("shapes,skewed", W.CASES_AUTO, ids=["4tiles", "36tiles", "64tiles", "90tiles"])
def test_library_choice_of_skew_and_order(lib, op, shapes, skewed):
    """skew = 0, order = 0 at M = 8192 - 17, 16 stages per equal range: what the training step runs. 4 tiles keep equal ranges;
    36, 64 (no leftover) and 90 tiles (the 448 layer) get a skew -- its value is a tuning choice recorded in csrc/gemm.hip and
    not pinned here, but a retune that makes it 0 at these shapes leaves this case testing nothing the explicit ones do not."""
    grp = run(lib, op, ("tiled", 0), W.M_AUTO, shapes, skew=0)
    eff, b = W.effective_skew(lib.qst_tn_group_ranges, grp)
    assert b[0] == 0 and b[-1] == W.M_AUTO
    if skewed:
        assert eff > 0, (f"the library no longer skews the ranges of {shapes} at M = {W.M_AUTO}: this case has gone vacuous -- "
                         "move it to a shape the library's choice (tn_auto_skew, csrc/gemm.hip) still skews")
    else:
        assert eff == 0, f"the library now skews a {len(shapes)}-problem launch of 4 tiles by {eff}: update this case"


# ------------------------------------------------------------------ G: the 256 x 256 instantiation
@pytest.mark.parametrize("HI", [(256, 1024), (320, 1280)], ids=["256x256", "fallback"])
def test_eightphase_256_tile(lib, op, HI):
    """splits = -256 asks qst_gemm_tn8_group for its 256 x 256 tile, which it grants where 256 divides every N and K -- the
    (256, 1024) group -- and answers with the 128 x 384 form elsewhere: the (320, 1280) group"""
    run(lib, op, ("eightphase", 0), W.M_TWO, W.layer(*HI), splits=-256)


# ------------------------------------------------------------------ H: random operands once
@pytest.mark.parametrize("kernel", ["tiled", "eightphase"])
def test_gaussian_operands_on_the_widest_layer(lib, op, kernel):
    """the (1024, 4096) group with Gaussian operands rounded to the operand type: rtol 1e-3, atol 1e-3 * sqrt(M)"""
    run(lib, op, (kernel, 0), W.M_TWO, W.layer(1024, 4096), skew=0, ints=False)
