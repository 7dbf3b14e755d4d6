"""The NT GEMM kernels (csrc/gemm.hip gemm_nt_kernel in its four instantiations, csrc/gemm8.hip gemm_nt8_kernel in its two) at
rtol = atol = 0, over every class of shape their tiles distinguish, with leading dimensions larger than the widths and
outputs inside guard bands.

tests/test_gpu_kernels.py compares Gaussian operands at rtol 8e-3 / atol 2e-2 on dense tensors of (mostly) whole tiles: a store
past [M, N] lands in the next row's own columns or behind the allocation, a row stride taken from the width is the width,
and a dropped 8-element fragment of a long reduction stays inside the tolerance. Here (tests/nt_helpers.py):

  * operands are small integers (times a power of two), so every product and partial sum is exact in fp32 and the result
    does not depend on the order of summation: bias, residual, the 16-bit rounding and the gelu' multiply are compared
    bit for bit, the GELU epilogue against fp64 of the exact pre-activation;
  * the case table holds, for every form, M = 1, the rows around an MFMA block, a wave tile and a workgroup tile, the column
    tails inside a wave's first block, on a wave boundary, one vector past a wave and past a tile (N % 8 == 4 on the tiled
    kernels), 1 to 8 K stages and tile counts in every residue of 8 (tests/test_nt_cases_host.py keeps the classes in);
  * the padded runs put every operand, residual and aux inside bands of ones, C and C2 inside 264 rows and 72 columns of a
    sentinel that must survive -- 264 rows because a store that loses its row guard reaches at most 255 rows past M.

A: exact, dense. B: exact, padded. C: dropout under a padded output. D: Gaussian operands once per form. E: refusals.
F: the fp8 forms' strides and bands. G: the selector bits of qst_gemm_nt.
"""
import pytest
import torch

import quadruplet_sentence_transformer_amd  # noqa: F401
from oracle import dropout_ref as D
from quadruplet_sentence_transformer_amd import _lib
from kernel_helpers import OPDT, drop_desc, drop_state, gemm_args, kf, lib, op, opr, quant_dev, row_major, stream  # noqa: F401
from nt_helpers import (BIAS_GUARD, C_GUARD_ROWS, ERR_BAD_ARG, ERR_UNSUPPORTED, F32_EPIS, FORM, FORMS, GUARD_COLS, GUARD_ROWS,
                        PADDED_CASES, RAGGED, SENTINEL, VIA_NT, accepts, assert_band, assert_untouched, call, case_id, cases_for,
                        host_problem, run)

pytestmark = pytest.mark.gpu


def entry_of(lib, op, form):
    """the entry point a form is called through, by name (tests/test_kernel_coverage_host.py reads this file)"""
    return kf(lib, "qst_gemm_nt", op) if form.call == "nt" else kf(lib, "qst_gemm_nt8", op)


# ------------------------------------------------------------------ A. exact, dense
@pytest.mark.parametrize("form,case", [pytest.param(f, c, id=case_id(f, c)) for f in FORMS for c in cases_for(f)])
def test_exact_dense(lib, op, form, case):
    """every epilogue the form's kernel has, bit for bit (QST_EPI_GELU: within nt_helpers.GELU_ULPS of fp64 on the exact u).

    Measured on gfx950 over all forms and cases, the largest error of the GELU epilogue in ulps of the operand type, beyond
    the erf approximation's absolute term GELU_ABS * max(1, |u|): bf16 0.499 (gelu') / 0.493 (gelu), f16 0.493 / 0.488; without
    that term over |reference| >= 2^-6: 0.499 / 0.495 and 0.498 / 0.488. The bound, the larger of 1 ulp and twice that, is 1 ulp
    (nt_helpers.GELU_ULPS), and never looser than rtol 8e-3 / atol 2e-2. On this epilogue the five kernels that have it agreed
    bit for bit at the three shapes compared, both outputs, both operand types (reported, not asserted)."""
    _, M, N, K = case
    run(entry_of(lib, op, form), op, form, M, N, K)


# ------------------------------------------------------------------ B. exact, padded
def padded_params():
    out = []
    for f in FORMS:
        for M, N, K in PADDED_CASES:
            # N % 8 == 4: a pad of 76 keeps ldc % 8 == 0; 72 gives ldc % 8 == 4, which the tiled kernels take (ldc % 4 == 0)
            for pad in ((GUARD_COLS + 4, GUARD_COLS) if N % 8 == 4 else (GUARD_COLS,)):
                if accepts(f, N, K, K + GUARD_COLS, K + GUARD_COLS, N + pad):
                    out.append(pytest.param(f, M, N, K, pad, id=f"{f.name}-{M}x{N}x{K}-ldc{N + pad}"))
    return out


@pytest.mark.parametrize("form,M,N,K,pad", padded_params())
def test_exact_padded(lib, op, form, M, N, K, pad):
    """lda = ldb = K + 72 around ones, resid / aux / C / C2 with ldc = ldr = N + pad, 264 guard rows: the exact results of A, and
    every guard element of C, C2 (QST_EPI_GELU's and QST_EPI_F32_RESID_BF16's too) and bias intact"""
    run(entry_of(lib, op, form), op, form, M, N, K, padded=True, pad=pad)


# ------------------------------------------------------------------ C. dropout under a padded output
SEED, STEP, SITE = 2 ** 40 + 5, 2, D.site_ffn_out(2)


@pytest.mark.parametrize("form", [f for f in FORMS if set(f.epis) & set(F32_EPIS)], ids=lambda f: f.name)
def test_dropout_mask_does_not_follow_the_leading_dimension(lib, op, form):
    """drop_where 1, p = 0.1, epilogues 1 and 4: the mask index is m * N + n, not m * ldc + n, so the padded run equals the dense
    one bit for bit on [:M, :N]. (Whether the mask is the right one: tests/test_gpu_dropout_epilogues.py.)"""
    M, N, K = RAGGED
    st = drop_state(lib, SEED, STEP)
    dd = drop_desc(st, SITE, 0.1)
    entry = entry_of(lib, op, form)
    plain = run(entry, op, form, M, N, K, epis=[e for e in form.epis if e in F32_EPIS])
    dense = run(entry, op, form, M, N, K, drop=dd)
    padded = run(entry, op, form, M, N, K, padded=True, drop=dd)
    assert sorted(dense) == sorted(padded) == [e for e in form.epis if e in F32_EPIS]
    resid = host_problem(M, N, K)["resid"]
    for epi, (C, C2) in dense.items():
        assert torch.equal(padded[epi][0], C), (form.name, epi)
        dropped = float(((C == resid) & (plain[epi][0] != resid)).float().mean())
        assert 0.05 < dropped < 0.15, (form.name, epi, dropped)      # a mask was applied at all
        if C2 is not None:
            assert torch.equal(padded[epi][1], C2) and torch.equal(C2, C.to(OPDT[op])), (form.name, epi)


# ------------------------------------------------------------------ D. Gaussian operands, once per form
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f.name)
def test_gaussian_operands(lib, op, form):
    """Small integers leave most of the mantissa unused, and a fragment-layout error that swaps elements of equal value hides
    behind them: the reference and tolerances of test_gemm_nt_epilogues on one shape ragged in M and N."""
    M, N, K = RAGGED
    dt = OPDT[op]
    g = torch.Generator().manual_seed(M + N + K)
    A = opr(op, torch.randn(M, K, generator=g))
    B = opr(op, torch.randn(N, K, generator=g) * 0.05)
    bias, resid = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    gp = opr(op, torch.rand(M, N, generator=g) * 1.2 - 0.1)
    ref = A @ B.t() + bias
    ur = ref.clone().requires_grad_(True)
    torch.nn.functional.gelu(ur).sum().backward()
    Ad, Bd, biasd, residd, gpd = A.to(dt).cuda(), B.to(dt).cuda(), bias.cuda(), resid.cuda(), gp.to(dt).cuda()
    entry = entry_of(lib, op, form)
    for epi in form.epis:
        C = torch.full((M, N), SENTINEL, dtype=torch.float32 if epi in F32_EPIS else dt, device="cuda")
        C2 = torch.full((M, N), SENTINEL, dtype=dt, device="cuda")
        a = gemm_args(A=Ad, B=Bd, C=C, C2=C2, aux=gpd, bias=None if epi == 3 else biasd, resid=residd, M=M, N=N, K=K, lda=K,
                      ldb=K, ldc=N, ldr=N)
        _lib.check(call(entry, form, a, epi))
        Ch, C2h = C.float().cpu(), C2.float().cpu()
        if epi == 0:
            torch.testing.assert_close(Ch, ref, rtol=8e-3, atol=2e-2)
        elif epi in F32_EPIS:
            torch.testing.assert_close(Ch, ref + resid, rtol=1e-4, atol=1e-3)
            if epi == 4:
                assert torch.equal(C2, C.to(dt))
        elif epi == 2:
            torch.testing.assert_close(Ch, ur.grad, rtol=8e-3, atol=2e-2)
            torch.testing.assert_close(C2h, torch.nn.functional.gelu(ref), rtol=8e-3, atol=2e-2)
        else:
            torch.testing.assert_close(Ch, (A @ B.t()) * gp, rtol=8e-3, atol=2e-2)


# ------------------------------------------------------------------ E. refusals
def test_shapes_the_kernels_do_not_take_are_refused(lib, op):
    """N % 4, ldc % 4, lda % 8, K % 64: QST_ERR_UNSUPPORTED from qst_gemm_nt and from qst_gemm_nt8 by name, nothing written.
    QST_EPI_GELU without C2 and QST_EPI_GELU_BWD without aux: QST_ERR_BAD_ARG from qst_gemm_nt8. (qst_gemm_nt does not look
    at C2 before it launches, so that call is not made here: its kernel would store through the null pointer.)"""
    dt = OPDT[op]
    M, N, K = 70, 104, 128
    A = torch.ones(M, K + 8, dtype=dt, device="cuda"); B = torch.ones(N, K + 8, dtype=dt, device="cuda")
    resid = torch.ones(M, N + 8, device="cuda"); aux = torch.ones(M, N + 8, dtype=dt, device="cuda")
    good = dict(M=M, N=N, K=K, lda=K + 8, ldb=K + 8, ldc=N + 8, ldr=N + 8)
    bad = [dict(good, N=N - 2), dict(good, ldc=N + 6), dict(good, lda=K + 4), dict(good, K=96)]
    nt, nt8 = kf(lib, "qst_gemm_nt", op), kf(lib, "qst_gemm_nt8", op)
    for epi in range(5):
        C = torch.full((M, N + 8), SENTINEL, dtype=torch.float32 if epi in F32_EPIS else dt, device="cuda")
        C2 = torch.full((M, N + 8), SENTINEL, dtype=dt, device="cuda")

        def args(dims, **kw):
            return gemm_args(**dict(dict(A=A, B=B, C=C, C2=C2, aux=aux, resid=resid, **dims), **kw))
        for dims in bad:
            for splits in (0, 1, 2, 3, 4, 0x20, 0x40, 0x80):
                assert nt(args(dims, splits=splits), epi, stream()) == ERR_UNSUPPORTED, (epi, dims, splits)
            for tile in (0, 1):
                assert nt8(args(dims), epi, tile, stream()) == ERR_UNSUPPORTED, (epi, dims, tile)
        for tile in (0, 1):
            if epi in (2, 4):
                assert nt8(args(good, C2=None), epi, tile, stream()) == ERR_BAD_ARG
            if epi == 3:
                assert nt8(args(good, aux=None), epi, tile, stream()) == ERR_BAD_ARG
        torch.cuda.synchronize()
        assert_untouched(C.cpu(), f"refused, epilogue {epi}, C")
        assert_untouched(C2.cpu(), f"refused, epilogue {epi}, C2")
        # the same arguments in a shape the kernels do take are launched: the refusals above are about the shape
        _lib.check(nt(args(good, splits=1), epi, stream()))
        _lib.check(nt8(args(good), epi, 0, stream()))
        assert_band(C.cpu(), M, N, f"taken, epilogue {epi}, C")


# ------------------------------------------------------------------ F. the fp8 forms: strides and bands
E4M3_ONE = 0x38
F8_COL, F8_COLS = 48, 80               # the padded fp8 operand is [rows + 64, K + 80] bytes, the view starts at byte 48


def deq(q, s, rows, K):
    e = row_major(s.cpu(), rows, K).to(torch.int32) - 127
    return torch.ldexp(q.cpu().view(torch.float8_e4m3fn).float().reshape(rows, K // 32, 32), e[..., None]).reshape(rows, K)


def f8_band(q, rows, K):
    big = torch.full((rows + GUARD_ROWS, K + F8_COLS), E4M3_ONE, dtype=torch.uint8, device="cuda")
    big[:rows, F8_COL:F8_COL + K] = q
    return big[:rows, F8_COL:F8_COL + K]


@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("how,sel", [("f8", 0x80), ("f8", 0x40), ("f8x8", 0), ("f8x8", 1)], ids=lambda v: v if isinstance(v, str) else f"{v:#x}")
def test_fp8_forms_under_padded_operands_and_outputs(lib, how, sel, K):
    """qst_gemm_nt_f8 tiled (splits 0x80) and forced to the 8-phase form (0x40), qst_gemm_nt8_f8 by name in both tiles, epilogues
    0 and 1, on the integer operands of the 16-bit tests, which MXFP8 holds exactly (checked first, on the device's own
    quantisation). One dense run and one with lda = ldb = K + 80 around e4m3 ones, resid with ldr = N + 72 and the output
    [M + 264, N + 72]: bit for bit the same on [:M, :N], every guard element intact. The MX scale arrays are laid out by row
    count ([ceil(K / 128)][rows][4], no leading dimension), so they cannot be views and are not padded."""
    M, N, _ = RAGGED
    p = host_problem(M, N, K)
    (Aq, As), (Bq, Bs) = quant_dev(lib, p["A"]), quant_dev(lib, p["B"])
    assert torch.equal(deq(Aq, As, M, K), p["A"]) and torch.equal(deq(Bq, Bs, N, K), p["B"])
    bias = torch.cat([p["bias"], torch.full((BIAS_GUARD,), SENTINEL)]).cuda()
    Ap, Bp = f8_band(Aq, M, K), f8_band(Bq, N, K)
    rbig = torch.ones(M + GUARD_ROWS, N + GUARD_COLS, device="cuda")
    rbig[:M, :N] = p["resid"].cuda()
    for epi in (0, 1):
        outs = []
        for A_, B_, r_, rows, ld in ((Aq, Bq, p["resid"].cuda(), M, N), (Ap, Bp, rbig[:M, :N], M + C_GUARD_ROWS, N + GUARD_COLS)):
            C = torch.full((rows, ld), SENTINEL, dtype=torch.float32 if epi else torch.bfloat16, device="cuda")
            a = gemm_args(A=A_, B=B_, aux=As, bscale=Bs, C=C, bias=bias, resid=r_ if epi else None, M=M, N=N, K=K,
                          lda=A_.stride(0), ldb=B_.stride(0), ldc=ld, ldr=r_.stride(0), splits=sel if how == "f8" else 0)
            if how == "f8":
                _lib.check(lib.qst_gemm_nt_f8(a, epi, stream()))
            else:
                _lib.check(lib.qst_gemm_nt8_f8(a, epi, sel, stream()))
            Ch = C.cpu()
            assert_band(Ch, M, N, f"{how}-{sel:#x} epilogue {epi}, ldc = {ld}, C")
            outs.append(Ch[:M, :N])
        assert not bool((outs[0] == SENTINEL).any())
        assert torch.equal(outs[0], outs[1]), (how, sel, epi)
    assert bool((bias.cpu()[N:] == SENTINEL).all())


# ------------------------------------------------------------------ G. the selector bits of qst_gemm_nt
@pytest.mark.parametrize("sel", [0x20, 0x40])
@pytest.mark.parametrize("M,N,K", [RAGGED, (300, 776, 64)])
def test_selector_bits_reach_the_eight_phase_kernels(lib, op, sel, M, N, K):
    """qst_gemm_nt with splits 0x20 / 0x40: exact, padded, and -- the same kernel on the same operands -- bit for bit what
    qst_gemm_nt8 gives by name with tile 0 / 1, the GELU outputs included"""
    via, direct = VIA_NT[sel], FORM["eight128x384" if sel == 0x20 else "eight256x256"]
    a = run(kf(lib, "qst_gemm_nt", op), op, via, M, N, K, padded=True)
    b = run(kf(lib, "qst_gemm_nt8", op), op, direct, M, N, K, padded=True)
    for epi in direct.epis:
        assert torch.equal(a[epi][0], b[epi][0]) and (b[epi][1] is None or torch.equal(a[epi][1], b[epi][1])), epi


def test_n_not_a_multiple_of_eight_falls_back_to_the_tiled_kernel(lib, op):
    """N % 8 == 4: qst_gemm_nt8_supported says no, qst_gemm_nt8 by name refuses and writes nothing, qst_gemm_nt with 0x20 / 0x40
    still gives the exact result (through its 128-row tiled kernel)"""
    M, N, K = 70, 196, 128
    dt = OPDT[op]
    A = torch.ones(M, K, dtype=dt, device="cuda"); B = torch.ones(N, K, dtype=dt, device="cuda")
    for epi in range(5):
        C = torch.full((M, N), SENTINEL, dtype=torch.float32 if epi in F32_EPIS else dt, device="cuda")
        C2 = torch.full((M, N), SENTINEL, dtype=dt, device="cuda")
        a = gemm_args(A=A, B=B, C=C, C2=C2, aux=C2, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, ldr=N)
        assert kf(lib, "qst_gemm_nt8_supported", op)(a, epi) == 0
        for tile in (0, 1):
            assert kf(lib, "qst_gemm_nt8", op)(a, epi, tile, stream()) == ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert_untouched(C.cpu(), "refused C"); assert_untouched(C2.cpu(), "refused C2")
    for sel in (0x20, 0x40):
        run(kf(lib, "qst_gemm_nt", op), op, FORM["tiles128"]._replace(name=f"nt-{sel:#x}-fallback", sel=sel), M, N, K, padded=True)


def test_the_selector_that_forbids_the_eight_phase_kernels(lib, op):
    """splits 0x80: one more selector of the 128-row tiled kernel -- exact, and bit for bit splits 1"""
    M, N, K = RAGGED
    a = run(kf(lib, "qst_gemm_nt", op), op, VIA_NT[0x80], M, N, K, padded=True)
    b = run(kf(lib, "qst_gemm_nt", op), op, FORM["tiles128"], M, N, K, padded=True)
    for epi in b:
        assert torch.equal(a[epi][0], b[epi][0]) and (b[epi][1] is None or torch.equal(a[epi][1], b[epi][1])), epi
