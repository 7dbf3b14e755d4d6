"""CPU, no library: the operands of tests/test_gpu_nt_shapes.py (tests/nt_helpers.py) are exact where the GPU tests compare at
rtol = atol = 0, and its case table still contains every class of shape it was drawn up to contain.

The tiles, wave tiles and K stages (nt_helpers.FORMS) mirror csrc/gemm.hip and csrc/gemm8.hip as of this change and serve only
to LABEL the cases: what the GPU tests assert -- equality with A.B^T and its epilogues -- does not depend on them. If a
kernel's tile changes, the classes below name what its tests should be re-derived for; an edit of the table that silently drops
a class, or turns a case into one a form falls back on, fails here.
"""
import torch

from nt_helpers import (CASES, COL_CLASSES, COL_CLASSES_N4, FORM, FORMS, PADDED_CASES, RAGGED, ROW_CLASSES, SENTINEL, TILE_COUNTS,
                        VIA_NT, accepts, cases_for, col_classes, expected, host_problem, k_classes, row_classes, scale_exp,
                        tile_count)

SHAPES = sorted({c[1:] for c in CASES})


def test_the_table_is_small_and_labelled_once():
    assert len({c[0] for c in CASES}) == len(CASES) == len(SHAPES)
    for _, M, N, K in CASES:
        assert 1 <= M <= 600 and 4 <= N <= 1200 and 64 <= K <= 512 and K % 64 == 0 and N % 4 == 0
    assert set(PADDED_CASES) <= set(SHAPES) and RAGGED in SHAPES


def test_every_reference_is_exact():
    """fp32 = fp64 = a summation in chunks of 32, whatever the grouping: every partial sum is a multiple of 2^-s below 2^24 2^-s"""
    for M, N, K in SHAPES:
        p = host_problem(M, N, K)
        A, B, s = p["A"], p["B"], scale_exp(K)
        for t in (A, B, p["bias"], p["resid"], p["aux"]):
            assert torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t.to(torch.float16).float(), t)
        assert torch.equal(A, A.round()) and float(A.abs().max()) <= 2
        assert torch.equal(B * 2.0 ** s, (B * 2.0 ** s).round()) and float(B.abs().max()) <= 2 * 2.0 ** -s
        acc64 = A.double() @ B.double().t()
        assert torch.equal(p["acc"].double(), acc64), (M, N, K)
        chunked = torch.zeros(M, N)
        for k0 in range(0, K, 32):
            chunked = chunked + A[:, k0:k0 + 32] @ B[:, k0:k0 + 32].t()
        assert torch.equal(chunked, p["acc"]), (M, N, K)
        assert float((A.abs().double() @ B.abs().double().t()).max()) * 2.0 ** s < 2.0 ** 24
        assert torch.equal(p["u"].double(), acc64 + p["bias"].double())
        assert torch.equal((p["u"] + p["resid"]).double(), acc64 + p["bias"].double() + p["resid"].double())
        assert torch.equal((p["acc"] * p["aux"]).double(), acc64 * p["aux"].double())
        assert float((p["u"].abs() < 3).float().mean()) >= 0.5, (M, N, K)
        for dt in (torch.bfloat16, torch.float16):
            for epi in (0, 1, 3, 4):
                for want in expected(p, epi, dt):
                    assert want is None or not bool((want == SENTINEL).any())
        assert not bool((p["gelu"] == SENTINEL).any()) and not bool((p["dgelu"] == SENTINEL).any())


def test_no_case_is_a_fallback():
    """every (form, case) pair test_gpu_nt_shapes.py parametrises runs on the form's own kernel"""
    for f in FORMS:
        got = cases_for(f)
        assert got, f.name
        for _, M, N, K in got:
            assert accepts(f, N, K) and K % f.stage == 0 and N % (4 if f.n4 else 8) == 0
        assert (len(got) == len(CASES)) == f.n4            # the 8-phase kernels leave out exactly the N % 8 == 4 entries
        assert {c for c in CASES if c not in got} == ({c for c in CASES if c[2] % 8 == 4} if not f.n4 else set())
    for M, N, K in PADDED_CASES:
        for f in FORMS:
            assert accepts(f, N, K, K + 72, K + 72, N + (76 if N % 8 == 4 else 72)) == (f.n4 or N % 8 == 0)
            if N % 8 == 4:
                assert accepts(f, N, K, K + 72, K + 72, N + 72) == f.n4 and (N + 72) % 8 == 4
    assert [accepts(FORM["tiles128"], 100, 64, ldc=ld) for ld in (100, 102, 104)] == [True, False, True]
    assert not accepts(FORM["eight128x384"], 104, 64, ldc=108) and not accepts(FORM["tiles128"], 104, 96)
    assert VIA_NT[0x20].tile == (128, 384) and VIA_NT[0x40].tile == (256, 256) and VIA_NT[0x80].tile == (128, 192)


def test_every_class_is_in_every_forms_cases():
    for f in FORMS:
        cases = cases_for(f)
        rows = set().union(*(row_classes(f, M) for _, M, _, _ in cases))
        cols = set().union(*(col_classes(f, N) for _, _, N, _ in cases))
        ks = set().union(*(k_classes(f, K) for _, _, _, K in cases))
        assert rows == ROW_CLASSES, (f.name, ROW_CLASSES - rows)
        assert cols >= COL_CLASSES, (f.name, COL_CLASSES - cols)
        assert (cols >= COL_CLASSES_N4) if f.n4 else not (cols & COL_CLASSES_N4), (f.name, COL_CLASSES_N4 - cols)
        assert ks == {"one_stage64", "even_stages", "odd_stages"} if f.stage == 64 else ks == {"one_stage64", "even_stages"}, f.name
        counts = {tile_count(f, M, N) for _, M, N, _ in cases}
        assert counts >= TILE_COUNTS, (f.name, TILE_COUNTS - counts)
        assert {c % 8 for c in counts} == set(range(8)), (f.name, sorted(counts))
        assert any(c > 8 and c % 8 == 7 for c in counts) or 7 in counts       # x < r taken by seven of the eight XCDs


def test_the_tall_form_cannot_run_an_odd_number_of_its_stages():
    """qst_gemm_nt takes K % 64 == 0 only, so the 32-deep stages of the tall wave tile always come in pairs: the class "an odd
    number of 32-deep stages" is empty by the library's own rule, not by an omission of the table"""
    f = FORM["tall256"]
    assert f.stage == 32 and all((K // f.stage) % 2 == 0 for _, _, _, K in cases_for(f))
    assert not accepts(f, 192, 96)


def test_the_labels_name_what_the_arithmetic_finds():
    t128, t256, tall, wide, e384, e256 = (FORM[n] for n in ("tiles128", "tiles256", "tall256", "wide128x384", "eight128x384",
                                                             "eight256x256"))
    assert row_classes(t128, 65) == {"above_wave"} and row_classes(tall, 129) == {"above_wave"} == row_classes(e256, 129)
    assert row_classes(t128, 129) == {"above_tile"} and row_classes(t128, 127) == {"below_tile"}
    assert row_classes(t256, 255) == {"below_tile"} and row_classes(t256, 257) == {"above_tile"}
    assert row_classes(t128, 200) == {"ragged_second"} and row_classes(t256, 300) == {"ragged_second"}
    assert "ragged_second" not in row_classes(t256, 200) and "ragged_second" not in row_classes(t128, 300)
    assert col_classes(t128, 96) == {"wave_boundary"} and col_classes(e256, 192) == {"wave_boundary"}
    assert col_classes(t128, 192) == {"whole_tiles"} and col_classes(wide, 384) == {"whole_tiles"}
    assert col_classes(t128, 200) == {"vec_past_wave", "vec_past_tile"} and "vec_past_tile" in col_classes(e384, 392)
    assert col_classes(e256, 264) == {"vec_past_wave", "vec_past_tile"}
    assert col_classes(t128, 196) == {"vec_past_wave4", "vec_past_tile4"} and "vec_past_tile4" in col_classes(wide, 388)
    assert col_classes(t128, 100) == {"vec_past_wave4"} and col_classes(t128, 36) == {"past_block4"}
    assert col_classes(t128, 216) == {"first_block"} == col_classes(e256, 216) and col_classes(t128, 116) == {"first_block4"}
    assert col_classes(t128, 4) == {"min4"} and col_classes(t128, 8) == {"min"}
    assert (tile_count(t128, 300, 520), tile_count(t256, 600, 520), tile_count(e384, 300, 776), tile_count(e256, 600, 520)) == (9, 9, 9, 9)
    assert (tile_count(t128, 600, 520), tile_count(e384, 600, 776), tile_count(e256, 600, 1160), tile_count(tall, 70, 1160)) == (15, 15, 15, 7)
    for label, M, N, K in CASES:
        kind = label.split("-")[0]
        assert kind in ("rows", "cols", "k", "count")
        if kind == "rows":
            assert any(row_classes(f, M) for f in FORMS), label
        if kind == "cols":
            assert any(col_classes(f, N) for f in FORMS), label
