"""CPU: the host side of the paired weight-gradient launch (csrc/qst_api.hip: wgrad_shapes, wgrad_pair_rule), no device needed.

One grouped launch takes the four weight gradients of a layer, or the eight of two neighbouring layers. What is checked here:
the tile count of a pair is twice the layer's at every layer width the library accepts (the pair of a 48-tile MiniLM layer is
96 tiles = three whole tiles for each of the 32 workgroups of an M-range), the count is the sum over the four products, and
the library's own choice (qst_encoder_set_wgrad_pairs(0)) is the rule include/qst.h documents.
"""
from dataclasses import replace

import pytest

import quadruplet_sentence_transformer_amd  # noqa: F401
from quadruplet_sentence_transformer_amd import _lib
from quadruplet_sentence_transformer_amd.config import PRESETS

TT = 192                    # the output tile of gemm_tn_group_kernel (csrc/gemm.hip: TT)
PAIR_MIN_ROWS = 8192      # include/qst.h, qst_wgrad_pairs_rule
# every width qst_encoder_create accepts: H a multiple of 64 up to 1024 with heads of 32 or 64; I = 4 H, and the two odd
# feed-forward widths of the presets' families (I a multiple of 64)
WIDTHS = [(H, I, H // d) for H in range(64, 1025, 64) for d in (32, 64) for I in (4 * H, 2 * H + 64)]


def cfg_of(H, I, A, layers=6):
    return _lib.make_config(replace(PRESETS["all-MiniLM-L6-v2"], hidden_size=H, intermediate_size=I, num_heads=A, num_layers=layers))


def tiles_of(H, I):
    t = lambda n: (n + TT - 1) // TT     # noqa: E731
    return t(H) * t(I) + t(I) * t(H) + t(H) * t(H) + t(3 * H) * t(H)


@pytest.mark.parametrize("H,I,A", WIDTHS)
def test_a_pair_has_twice_the_tiles_of_a_layer(H, I, A):
    lib = _lib.load()
    for M in (320, 32768):
        one, two = lib.qst_wgrad_tiles(cfg_of(H, I, A), M, 1), lib.qst_wgrad_tiles(cfg_of(H, I, A), M, 2)
        assert one == tiles_of(H, I) and two == 2 * one, (H, I, M, one, two)


def test_the_minilm_pair_is_three_whole_tiles_per_workgroup():
    lib = _lib.load()
    c = cfg_of(384, 1536, 12)
    assert (lib.qst_wgrad_tiles(c, 32768, 1), lib.qst_wgrad_tiles(c, 32768, 2)) == (48, 96)
    assert 96 % 32 == 0 and 48 % 32 != 0
    assert lib.qst_wgrad_tiles(cfg_of(768, 3072, 12), 32768, 1) == 192


def test_arguments_are_checked():
    lib = _lib.load()
    c = cfg_of(384, 1536, 12)
    assert lib.qst_wgrad_tiles(c, 32768, 0) < 0 and lib.qst_wgrad_tiles(c, 32768, 3) < 0 and lib.qst_wgrad_tiles(c, 0, 1) < 0
    assert lib.qst_wgrad_tiles(None, 32768, 1) < 0 and lib.qst_wgrad_pairs_rule(None, 32768) < 0
    assert lib.qst_wgrad_pairs_rule(c, 0) < 0
    assert lib.qst_version() >= 115


@pytest.mark.parametrize("H,I,A", WIDTHS)
def test_the_librarys_choice_is_the_documented_rule(H, I, A):
    """Pairs where a layer alone gives each of the 32 workgroups of an M-range at least one and fewer than two whole tiles
    (32 <= tiles < 64), from 8,192 token rows, in a model of at least two layers."""
    lib = _lib.load()
    t = tiles_of(H, I)
    for M in (320, 4096, PAIR_MIN_ROWS - 32, PAIR_MIN_ROWS, 32768, 196608):
        for layers in (1, 2, 3, 6):
            want = int(layers >= 2 and M >= PAIR_MIN_ROWS and 32 <= t < 64)
            assert lib.qst_wgrad_pairs_rule(cfg_of(H, I, A, layers), M) == want, (H, I, M, layers)


def test_the_measured_points_of_the_rule():
    lib = _lib.load()
    minilm, base = cfg_of(384, 1536, 12), cfg_of(768, 3072, 12, 12)
    assert [lib.qst_wgrad_pairs_rule(minilm, M) for M in (4096, 8192, 16384, 32768)] == [0, 1, 1, 1]
    assert lib.qst_wgrad_pairs_rule(base, 32768) == 0
    assert lib.qst_wgrad_pairs_rule(cfg_of(384, 1536, 12, 1), 32768) == 0
