"""CPU, no library: the case table of tests/test_gpu_wgrad_shapes.py (tests/wgrad_helpers.py) still contains every class of
the grouped weight-gradient kernels' work decomposition it was drawn up to contain.

The tile sizes (192 x 192 for gemm_tn_group_kernel, 128 x 384 for the form of gemm_tn8_group_kernel in use) and the 32
workgroups per XCD mirror csrc/gemm.hip and csrc/gemm8.hip as of this change and serve only to LABEL the cases: what the GPU
tests assert -- equality with A^T . B -- does not depend on them. If a kernel's tile changes, the classes below name what its
tests should be re-derived for; an edit of the width list that silently drops a class fails here.
"""
from wgrad_helpers import (CASES_A, CASES_B, EIGHT_PHASE, M_FIVE, M_TWO, MINILM, TILED, decomposition, layer, ragged,
                           workgroups_per_range)


def tiled_cases():
    """(T, a, b, pieces, idle) of cases A (32 workgroups per range) and B (16 and 10) on the 192 x 192 tile"""
    out = [decomposition(layer(H, I), *TILED, 32) for H, I, _ in CASES_A]
    out += [decomposition(layer(*HI), *TILED, workgroups_per_range(splits)) for splits, HI in CASES_B]
    return out


def test_decomposition_arithmetic():
    assert decomposition([(192, 192)], 192, 192, 32) == (1, 0, 1, 32, 0)
    assert decomposition([(200, 136)], 192, 192, 32) == (2, 0, 2, 16, 0)
    assert decomposition([(1152, 1152)], 192, 192, 32) == (36, 1, 4, 8, 0)
    assert decomposition([(1536, 1536)], 192, 192, 32) == (64, 2, 0, 0, 0)
    assert [workgroups_per_range(s) for s in (0, 8, 16, 24, 3)] == [32, 32, 16, 10, 32]


def test_the_table_of_the_tiled_kernel():
    """T, a, b, pieces, idle workgroups and raggedness of a layer's four gradients by width, 192 x 192 tiles on 32 workgroups"""
    want = {(64, 256): (6, 0, 6, 5, 2, True), (128, 512): (9, 0, 9, 3, 5, True), (256, 1024): (36, 1, 4, 8, 0, True),
            (320, 1280): (42, 1, 10, 3, 2, True), (384, 1536): (48, 1, 16, 2, 0, False), (448, 1792): (90, 2, 26, 1, 6, True),
            (512, 2048): (99, 3, 3, 10, 2, True), (768, 3072): (192, 6, 0, 0, 0, False), (1024, 4096): (396, 12, 12, 2, 8, True)}
    widths = [(H, I) for H, I, _ in CASES_A]
    for HI, (T, a, b, pieces, idle, rag) in want.items():
        assert decomposition(layer(*HI), *TILED, 32) == (T, a, b, pieces, idle), HI
        assert any(ragged(layer(*HI), *TILED)) == rag, HI
        assert HI in widths or HI == MINILM, f"{HI} left the case table"
    assert MINILM not in widths                      # the older files' layer; case B runs it on 16 and 10 workgroups
    # two and more ranges per XCD
    assert decomposition(layer(*MINILM), *TILED, 16) == (48, 3, 0, 0, 0)
    assert decomposition(layer(448, 1792), *TILED, 16) == (90, 5, 10, 1, 6)
    assert {(s, HI) for s, HI in CASES_B} == {(s, HI) for s in (16, 24) for HI in (MINILM, (448, 1792))}


def test_rows_per_case():
    """five stages per equal range with a ragged last one up to H = 512, two for the wide layers"""
    for H, _, M in CASES_A:
        assert M == (M_FIVE if H <= 512 else M_TWO)
    assert (-(-M_FIVE // 64) // 8, M_FIVE % 64 != 0) == (5, True)
    assert (-(-M_TWO // 64) // 8, M_TWO % 64 != 0) == (2, True)


def test_every_class_of_the_tiled_kernel_is_in_the_table():
    cases = tiled_cases()

    def some(pred):
        return any(pred(*c) for c in cases)

    assert some(lambda T, a, b, pieces, idle: a == 0 and b > 0)
    assert some(lambda T, a, b, pieces, idle: a >= 2 and b == 0)
    assert some(lambda T, a, b, pieces, idle: a >= 2 and b > 0)
    assert some(lambda T, a, b, pieces, idle: pieces == 1 and idle > 0)
    assert some(lambda T, a, b, pieces, idle: pieces >= 2 and idle > 0)
    assert some(lambda T, a, b, pieces, idle: pieces >= 2 and idle == 0)
    groups = [layer(H, I) for H, I, _ in CASES_A] + [layer(*HI) for _, HI in CASES_B]
    assert any(ragged(g, *TILED)[0] for g in groups) and any(ragged(g, *TILED)[1] for g in groups)


def test_classes_of_the_eight_phase_tile():
    """the same widths on 128 x 384 tiles, 32 workgroups"""
    widths = [(H, I) for H, I, _ in CASES_A]
    assert (256, 1024) in widths and (320, 1280) in widths
    T, a, b, pieces, idle = decomposition(layer(256, 1024), *EIGHT_PHASE, 32)
    assert (T, a, pieces) == (22, 0, 1) and idle > 0
    T, a, b, pieces, idle = decomposition(layer(320, 1280), *EIGHT_PHASE, 32)
    assert (T, b, pieces) == (33, 1, 32)
    assert any(a >= 2 and b > 0 for _, a, b, _, _ in (decomposition(layer(H, I), *EIGHT_PHASE, 32) for H, I in widths))
