"""Dropout in the GEMM epilogues (QstGemmArgs.drop, drop_where 1 / 2 / 3), kernel by kernel.

Every epilogue recomputes the mask from the element's flat index m * N + n with its own arithmetic from lane and register to
(m, n). tests/test_gpu_dropout.py runs them with a mask on bf16 operands, at the form the dispatcher picks and with
ldc = N only. Here every form is called by name or forced through QstGemmArgs.splits, on both operand types and on the
fp8 kernels, with a seed whose high word is not zero and a padded output, and the set of dropped elements is compared
exactly: oracle/dropout_ref.py regenerates the masks, the values come from an fp64 reference on the operands as the
kernel holds them (opr(op, .) for the 16-bit kernels, the de-quantised MXFP8 operands for the fp8 ones).

Inputs are chosen so that "dropped" can be read off the output without ambiguity. A kept element looks dropped when
(acc + bias) * k is too small to change resid (part 1, 3) or when ds * k rounds to zero (part 2, where 2). The biases of
parts 1 and 3 and the residual-path gradient of part 2 therefore stay away from zero (random signs, magnitude above the
spread of the accumulator), and each case counts on the CPU, from the fp64 reference, the kept positions that could still
coincide: |(acc + bias) * k| <= half an fp32 ulp of |resid| + the value tolerance of the case (a kernel inside its
tolerance cannot land on resid either), respectively |ds * k| <= 1e-6 + the tolerance on ds. The count is asserted to be 0
in every case of this file (plain_case, f8_case, ln_case), so the kept-position checks below hold at ALL kept positions.
"""
import functools

import numpy as np
import pytest
import torch

import quadruplet_sentence_transformer_amd  # noqa: F401
from oracle import dropout_ref as D
from oracle import torch_ref as R
from quadruplet_sentence_transformer_amd import _lib
from kernel_helpers import OPDT, drop_desc, drop_state, gemm_args, kf, lib, ln_epi, op, opr, stage_major, stream  # noqa: F401

pytestmark = pytest.mark.gpu

SEED, STEP = 2 ** 40 + 5, 2              # the high seed word enters the key through rotl16(seed hi)
SITE_PLAIN, SITE_LN, SITE_F8 = D.site_ffn_out(2), D.site_attn_out(3), D.site_ffn_out(1)
U32 = 2.0 ** -24                         # unit roundoff of fp32
NAN = float("nan")


def mult(site, shape, p):
    return torch.from_numpy(D.multipliers(SEED, STEP, site, int(np.prod(shape)), p).reshape(shape))


def keep_scale(p):
    return 65536.0 / (65536 - D.thr16_of(p))


def away_from_zero(g, shape, lo):
    """random signs, magnitudes in [lo, lo + 1)"""
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float() * (lo + torch.rand(shape, generator=g))


def half_ulp32(x):
    a = x.abs()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double() * 0.5


def padded(t, ld, dtype=None):
    """t [M, N] as the first N columns of a NaN-filled [M, ld] device tensor"""
    out = torch.full((t.shape[0], ld), NAN, dtype=dtype or t.dtype)
    out[:, :t.shape[1]] = t
    return out.cuda()


def check_dropped_set_and_values(C, c, N):
    """C: the kernel's fp32 [M, ldc] output on the CPU. The dropped set exactly, the values, and the pad columns."""
    out = C[:, :N]
    dropped = c["mk"] == 0
    assert torch.equal(out.contiguous().view(torch.int32)[dropped], c["resid"].view(torch.int32)[dropped])   # bit for bit resid
    assert bool((out[~dropped] != c["resid"][~dropped]).all())         # and nowhere else (c["coincidences"] == 0)
    err = (out.double() - c["ref"]).abs()
    assert bool((err <= c["tol"]).all()), float((err - c["tol"]).max())
    assert bool(torch.isnan(C[:, N:]).all())


# ------------------------------------------------------------------ 1. plain GEMM with residual
@functools.lru_cache(maxsize=None)
def plain_case(op, M, N, K, p):
    g = torch.Generator().manual_seed(1000 * M + N + K)
    A = opr(op, torch.randn(M, K, generator=g)); B = opr(op, torch.randn(N, K, generator=g) * 0.05)
    bias = away_from_zero(g, (N,), 2.5)                              # the accumulator spreads by 0.05 sqrt(K) <= 0.57
    resid = torch.randn(M, N, generator=g)
    mk = mult(SITE_PLAIN, (M, N), p)
    v = (A.double() @ B.double().t() + bias.double()) * mk.double()
    ref = v + resid.double()
    # test_gemm_nt_epilogues' bound for the fp32 epilogue; the kept accumulator error is scaled by 65536 / (65536 - thr16)
    tol = 1e-4 * ref.abs() + 1e-3 * keep_scale(p)
    coincidences = int(((mk != 0) & (v.abs() <= half_ulp32(resid) + tol)).sum())
    assert coincidences == 0
    return dict(A=A, B=B, bias=bias, resid=resid, mk=mk, ref=ref, tol=tol, coincidences=coincidences)


PLAIN_SHAPES = [(300, 1152, 128, 1152, 0.1),      # ragged last row tile at 128 and 256 rows; N = 3 x 384 = 4.5 x 256 = 6 x 192
                (200, 192, 64, 192, 0.1),         # one partial tile
                (264, 200, 64, 256, 0.1),         # padded output: ldc = ldr = 256
                (200, 192, 64, 192, 0.5)]
PLAIN_FORMS = [("nt", 1), ("nt", 2), ("nt", 0x20), ("nt", 0x40), ("nt8", 0), ("nt8", 1)]


@pytest.mark.parametrize("M,N,K,ld,p", PLAIN_SHAPES)
@pytest.mark.parametrize("form", PLAIN_FORMS, ids=lambda f: f"{f[0]}-{f[1]:#x}")
def test_plain_epilogues_drop_exactly_the_oracles_set(lib, op, form, M, N, K, ld, p):
    """C = (A.B^T + bias) * mask + resid, drop_where 1, epi QST_EPI_F32_RESID (1) and QST_EPI_F32_RESID_BF16 (4): qst_gemm_nt
    with splits 1 / 2 (128- / 256-row tiled kernels) and 0x20 / 0x40 (the 8-phase tiles), qst_gemm_nt8 with tile 0 / 1."""
    c = plain_case(op, M, N, K, p)
    dt = OPDT[op]
    st = drop_state(lib, SEED, STEP)
    Ad, Bd, biasd, residd = c["A"].to(dt).cuda(), c["B"].to(dt).cuda(), c["bias"].cuda(), padded(c["resid"], ld)
    for epi in (1, 4):
        C = torch.full((M, ld), NAN, device="cuda")
        C2 = torch.full((M, ld), NAN, dtype=dt, device="cuda")
        a = gemm_args(A=Ad, B=Bd, C=C, C2=C2, bias=biasd, resid=residd, M=M, N=N, K=K, lda=K, ldb=K, ldc=ld, ldr=ld,
                      drop=drop_desc(st, SITE_PLAIN, p), drop_where=1, splits=form[1] if form[0] == "nt" else 0)
        if form[0] == "nt":
            _lib.check(kf(lib, "qst_gemm_nt", op)(a, epi, stream()))
        else:
            _lib.check(kf(lib, "qst_gemm_nt8", op)(a, epi, form[1], stream()))
        check_dropped_set_and_values(C.cpu(), c, N)
        if epi == 4:
            assert torch.equal(C2[:, :N], C[:, :N].to(dt)) and bool(torch.isnan(C2[:, N:]).all())
        else:
            assert bool(torch.isnan(C2).all())


# ------------------------------------------------------------------ 2. GEMM + LayerNorm
def ln_bwd_ref(dy, gamma, xhat, rstd):
    dx = dy * gamma
    return rstd[:, None] * (dx - dx.mean(1, keepdim=True) - xhat * (dx * xhat).mean(1, keepdim=True))


@functools.lru_cache(maxsize=4)
def ln_case(op, M, K, N, p):
    g = torch.Generator().manual_seed(1000 * M + N + K + 1)
    A = opr(op, torch.randn(M, K, generator=g)); B = opr(op, torch.randn(N, K, generator=g) * 0.03)
    bias = torch.randn(N, generator=g); resid = torch.randn(M, N, generator=g)
    gamma = 1 + 0.1 * torch.randn(N, generator=g); beta = 0.1 * torch.randn(N, generator=g)
    mk = mult(SITE_LN, (M, N), p)
    acc = A.double() @ B.double().t()
    # mode 0
    v = (acc + bias.double()) * mk.double() + resid.double()
    mean = v.mean(1, keepdim=True)
    rstd0 = 1.0 / torch.sqrt(((v - mean) ** 2).mean(1) + 1e-12)
    xhat0 = (v - mean) * rstd0[:, None]
    y = xhat0 * gamma.double() + beta.double()
    del v
    # mode 1: dy = A.B^T + resid1; the residual-path gradient stays away from zero so that no kept ds vanishes
    xhat = opr(op, torch.randn(M, N, generator=g)); rstd = torch.rand(M, generator=g) + 0.5
    resid1 = away_from_zero(g, (M, N), 3.0)                          # the accumulator spreads by 0.03 sqrt(K) <= 0.34
    dy = acc + resid1.double()
    xd, gd, rd, md = xhat.double(), gamma.double(), rstd.double(), mk.double()
    ds = ln_bwd_ref(dy, gd, xd, rd)
    ds3 = ln_bwd_ref(dy * md, gd, xd, rd)
    coincidences = int(((mk != 0) & ((ds * md).abs() <= 1e-6 + 2e-3 + 1e-3 * ds.abs())).sum())
    assert coincidences == 0
    # gamma / beta gradient rows: each is a sum over rows of fp32 terms whose own accumulation is K deep, gathered per block
    # of at most 256 rows (the blocks are added in fp64 here): first-order bound (K + 256 + 2) u sum_m |term|, |dy| bounded
    # by |A|.|B|^T + |resid1|
    bound = (A.abs().double() @ B.abs().double().t() + resid1.abs().double()) * keep_scale(p)
    ptol = (K + 258) * U32 * torch.stack([(bound * xd.abs()).sum(0), bound.sum(0)])
    return dict(A=A, B=B, bias=bias, resid=resid, gamma=gamma, beta=beta, mk=mk, y=y, xhat0=xhat0, rstd0=rstd0,
                xhat=xhat, rstd=rstd, resid1=resid1, ds=ds, ds3=ds3, ptol=ptol, coincidences=coincidences,
                part2=torch.stack([(dy * xd).sum(0), dy.sum(0)]), part3=torch.stack([(dy * md * xd).sum(0), (dy * md).sum(0)]))


def close(got, want, rtol, atol):
    err = (got.double() - want).abs()
    lim = atol + rtol * want.abs()
    assert bool((err <= lim).all()), float((err - lim).max())


def fused_layernorm_with_masks(lib, op, entry, M, K, N, p):
    c = ln_case(op, M, K, N, p)
    dt = OPDT[op]
    st = drop_state(lib, SEED, STEP)
    mk = c["mk"]
    if entry == "nt_ln":
        fn, br = kf(lib, "qst_gemm_nt_ln", op), lib.qst_gemm_nt_ln_block_rows_m(N, M)
    else:
        fn, br = kf(lib, "qst_gemm_nt8_ln", op), kf(lib, "qst_gemm_nt8_ln_block_rows", op)(M, N)
    Ad, Bd = c["A"].to(dt).cuda(), c["B"].to(dt).cuda()
    gd, bd = c["gamma"].cuda(), c["beta"].cuda()

    def args(**kw):
        return gemm_args(A=Ad, B=Bd, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, ldr=N, drop=drop_desc(st, SITE_LN, p), **kw)
    # mode 0, where 1: y = LayerNorm((A.B^T + bias) * mask + resid); xhat / rstd of the masked rows; C2 = the 16-bit rounding of C
    C = torch.full((M, N), NAN, device="cuda"); C2 = torch.full((M, N), NAN, dtype=dt, device="cuda")
    xh = torch.full((M, N), NAN, dtype=dt, device="cuda"); rs = torch.full((M,), NAN, device="cuda")
    _lib.check(fn(args(C=C, C2=C2, bias=c["bias"].cuda(), resid=c["resid"].cuda(), drop_where=1),
                  ln_epi(gamma=gd, beta=bd, eps=1e-12, xhat=xh, rstd=rs), 0, stream()))
    close(C.cpu(), c["y"], 1e-3, 2e-3)
    assert torch.equal(C2, C.to(dt))
    close(xh.float().cpu(), c["xhat0"], 2.0 ** -8, 2e-3)       # one 16-bit rounding (bf16: 2^-9 relative) on top of the fp32 error
    close(rs.cpu(), c["rstd0"], 1e-4, 0)
    # mode 1: where 2 masks the 16-bit copy only, where 3 the incoming gradient
    xhd, rsd, r1d = c["xhat"].to(dt).cuda(), c["rstd"].cuda(), c["resid1"].cuda()
    for where, want_c, want_c2, want_part in ((2, c["ds"], c["ds"] * mk.double(), c["part2"]), (3, c["ds3"], c["ds3"], c["part3"])):
        C.fill_(NAN); C2.fill_(NAN)
        part = torch.zeros((M + br - 1) // br, 2, N, device="cuda")
        _lib.check(fn(args(C=C, C2=C2, resid=r1d, drop_where=where), ln_epi(gamma=gd, xhat=xhd, rstd=rsd, partials=part), 1, stream()))
        Cc, C2c = C.cpu(), C2.cpu()
        if where == 2:
            assert torch.equal((C2c == 0), (mk == 0))             # zero at every dropped position and at no kept one
        close(Cc, want_c, 1e-3, 2e-3)
        close(C2c.float(), want_c2, 1e-2, 1e-2)
        # the mask multiplies the fp32 result (where 2) or came before it (where 3), then one rounding
        assert torch.equal(C2c, ((Cc * mk) if where == 2 else Cc).to(dt))
        perr = (part.cpu().double().sum(0) - want_part).abs()
        assert bool((perr <= c["ptol"]).all()), float((perr / c["ptol"]).max())
    assert kf(lib, "qst_gemm_nt8_ln_timeouts", op)() == 0


LN_CASES = [(e, 300, 128, N, 0.1) for N in (384, 512, 768, 1024) for e in ("nt_ln", "nt8_ln")] + \
           [("nt_ln", 300, 128, 384, 0.5), ("nt8_ln", 300, 128, 768, 0.5)]


@pytest.mark.parametrize("entry,M,K,N,p", LN_CASES)
def test_fused_layernorm_epilogues_with_masks(lib, op, entry, M, K, N, p):
    """qst_gemm_nt_ln (N = 384: gemm_nt_ln_kernel; above: forwards) and qst_gemm_nt8_ln by name (N = 384 there: the 128 x 384
    tile alone in its row panel; above: 256 x 256 tiles exchanging row statistics), all three mask sites, both partial rows."""
    fused_layernorm_with_masks(lib, op, entry, M, K, N, p)


def test_fused_layernorm_128x384_tile_with_masks_f16(lib):
    """M = 32,700 at N = 768 takes the 128 x 384 tile of qst_gemm_nt8_ln (two workgroups per row panel, ragged last panel) on
    the f16 twin; test_gpu_dropout.py has the bf16 case."""
    assert lib.qst_gemm_nt8_ln_block_rows_f16(32700, 768) == 128
    fused_layernorm_with_masks(lib, "f16", "nt8_ln", 32700, 64, 768, 0.1)
    ln_case.cache_clear()


# ------------------------------------------------------------------ 3. fp8 kernels (bf16 build only)
def mx_dev(x):
    """x as MXFP8 on the device (elements, stage-major scales: bit for bit what qst_quant_mx writes) and de-quantised"""
    q, s, deq = R.mx_quant(x)
    return q.cuda(), stage_major(s).cuda(), deq


@functools.lru_cache(maxsize=None)
def f8_case(M, N, K, p):
    g = torch.Generator().manual_seed(1000 * M + N + K + 2)
    A = torch.randn(M, K, generator=g) * (0.5 + torch.rand(M, 1, generator=g))
    B = torch.randn(N, K, generator=g) * 0.02
    bias = away_from_zero(g, (N,), 2.5)                              # the accumulator spreads by 1.5 * 0.02 sqrt(K) <= 0.48
    resid = torch.randn(M, N, generator=g)
    Aq, As, Ad = mx_dev(A); Bq, Bs, Bd = mx_dev(B)
    mk = mult(SITE_F8, (M, N), p)
    v = (Ad.double() @ Bd.double().t() + bias.double()) * mk.double()
    ref = v + resid.double()
    acc_scale = float((Ad.abs().double() @ Bd.abs().double().t()).max())
    # test_gemm_f8_matches_fp32_on_dequantised_operands' bound, times the keep scale
    tol = torch.full_like(ref, (2e-5 * acc_scale + 1e-5) * keep_scale(p))
    coincidences = int(((mk != 0) & (v.abs() <= half_ulp32(resid) + tol)).sum())
    assert coincidences == 0
    return dict(Aq=Aq, As=As, Bq=Bq, Bs=Bs, bias=bias, resid=resid, mk=mk, ref=ref, tol=tol, coincidences=coincidences)


@pytest.mark.parametrize("M,N,K,p", [(300, 1152, 128, 0.1), (200, 192, 256, 0.1), (200, 192, 256, 0.5)])
@pytest.mark.parametrize("form", [("f8", 0x80), ("f8", 0x40), ("f8x8", 0), ("f8x8", 1)], ids=lambda f: f"{f[0]}-{f[1]:#x}")
def test_fp8_epilogues_drop_exactly_the_oracles_set(lib, form, M, N, K, p):
    """qst_gemm_nt_f8 tiled (splits 0x80) and forced to the 8-phase form (0x40), qst_gemm_nt8_f8 with tile 0 / 1; epi 1."""
    c = f8_case(M, N, K, p)
    st = drop_state(lib, SEED, STEP)
    C = torch.full((M, N), NAN, device="cuda")
    a = gemm_args(A=c["Aq"], B=c["Bq"], aux=c["As"], bscale=c["Bs"], C=C, bias=c["bias"].cuda(), resid=c["resid"].cuda(), M=M, N=N,
                  K=K, lda=K, ldb=K, ldc=N, ldr=N, drop=drop_desc(st, SITE_F8, p), drop_where=1, splits=form[1] if form[0] == "f8" else 0)
    if form[0] == "f8":
        _lib.check(lib.qst_gemm_nt_f8(a, 1, stream()))
    else:
        _lib.check(lib.qst_gemm_nt8_f8(a, 1, form[1], stream()))
    check_dropped_set_and_values(C.cpu(), c, N)


@pytest.mark.parametrize("M,K,N,p", [(300, 128, 768, 0.1), (257, 128, 512, 0.1), (257, 128, 512, 0.5)])
def test_fp8_fused_layernorm_with_a_mask(lib, M, K, N, p):
    """qst_gemm_nt8_f8_ln: y = LayerNorm((A.B^T + bias) * mask + resid) on the de-quantised operands; its MXFP8 output is bit for
    bit mx_quant of its own bf16 output."""
    g = torch.Generator().manual_seed(1000 * M + N + K + 3)
    A = torch.randn(M, K, generator=g) * (0.5 + torch.rand(M, 1, generator=g))
    B = torch.randn(N, K, generator=g) * 0.05
    bias = torch.randn(N, generator=g) * 0.3; resid = torch.randn(M, N, generator=g)
    gamma = 1 + 0.2 * torch.randn(N, generator=g); beta = 0.3 * torch.randn(N, generator=g)
    Aq, As, Ad = mx_dev(A); Bq, Bs, Bd = mx_dev(B)
    mk = mult(SITE_F8, (M, N), p)
    v = (Ad.double() @ Bd.double().t() + bias.double()) * mk.double() + resid.double()
    mean = v.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((v - mean) ** 2).mean(1) + 1e-12)
    xhat = (v - mean) * rstd[:, None]
    st = drop_state(lib, SEED, STEP)
    y = torch.full((M, N), NAN, device="cuda"); yb = torch.full((M, N), NAN, dtype=torch.bfloat16, device="cuda")
    xh = torch.full((M, N), NAN, dtype=torch.bfloat16, device="cuda"); rs = torch.full((M,), NAN, device="cuda")
    yq = torch.zeros(M, N, dtype=torch.uint8, device="cuda"); ys = torch.zeros(N // 128 * M * 4, dtype=torch.uint8, device="cuda")
    _lib.check(lib.qst_gemm_nt8_f8_ln(gemm_args(A=Aq, B=Bq, aux=As, bscale=Bs, C=y, C2=yb, C3=yq, C4=ys, bias=bias.cuda(), resid=resid.cuda(),
                                                M=M, N=N, K=K, lda=K, ldb=K, ldc=N, ldr=N, drop=drop_desc(st, SITE_F8, p), drop_where=1),
                                      ln_epi(gamma=gamma.cuda(), beta=beta.cuda(), eps=1e-12, xhat=xh, rstd=rs), stream()))
    close(y.cpu(), xhat * gamma.double() + beta.double(), 1e-3, 2e-3)
    assert torch.equal(yb, y.to(torch.bfloat16))
    close(xh.float().cpu(), xhat, 2.0 ** -8, 2e-3)
    close(rs.cpu(), rstd, 1e-4, 0)
    qr, sr, _ = R.mx_quant(yb.float().cpu())
    assert torch.equal(yq.cpu(), qr) and torch.equal(ys.cpu(), stage_major(sr))
    assert lib.qst_gemm_nt8_ln_timeouts() == 0


# ------------------------------------------------------------------ 4. refusals
def test_mask_descriptions_a_kernel_cannot_honour_are_refused(lib, op):
    """drop_where 2 on the plain 8-phase GEMM, drop_where 1 on the LayerNorm backward, a mask on the bf16 epilogue: an error
    code, and nothing written."""
    dt = OPDT[op]
    M, N, K = 64, 512, 128
    st = drop_state(lib, SEED, STEP)
    Ad, Bd = torch.ones(M, K, dtype=dt, device="cuda"), torch.ones(N, K, dtype=dt, device="cuda")
    resid = torch.zeros(M, N, device="cuda")
    C = torch.full((M, N), NAN, device="cuda"); C2 = torch.full((M, N), NAN, dtype=dt, device="cuda")
    gamma = torch.ones(N, device="cuda"); rstd = torch.ones(M, device="cuda")

    def args(where):
        return gemm_args(A=Ad, B=Bd, C=C, C2=C2, resid=resid, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, ldr=N,
                         drop=drop_desc(st, SITE_PLAIN, 0.1), drop_where=where)
    e1 = ln_epi(gamma=gamma, xhat=Ad.new_zeros(M, N), rstd=rstd)
    # the same arguments with a mask the kernel does apply are taken: the refusals below are about the mask
    _lib.check(kf(lib, "qst_gemm_nt8", op)(args(1), 1, 1, stream()))
    _lib.check(kf(lib, "qst_gemm_nt8_ln", op)(args(2), e1, 1, stream()))
    torch.cuda.synchronize()
    assert not bool(torch.isnan(C).any())
    C.fill_(NAN); C2.fill_(NAN)
    assert kf(lib, "qst_gemm_nt8", op)(args(2), 1, 1, stream()) != 0
    assert kf(lib, "qst_gemm_nt8", op)(args(1), 0, 1, stream()) != 0
    assert kf(lib, "qst_gemm_nt8_ln", op)(args(1), e1, 1, stream()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(C).all()) and bool(torch.isnan(C2).all())


def test_mask_descriptions_the_fp8_kernels_cannot_honour_are_refused(lib):
    M, N, K = 64, 256, 128
    st = drop_state(lib, SEED, STEP)
    Aq, As, _ = mx_dev(torch.ones(M, K)); Bq, Bs, _ = mx_dev(torch.ones(N, K))
    C = torch.full((M, N), NAN, device="cuda")
    a = gemm_args(A=Aq, B=Bq, aux=As, bscale=Bs, C=C, resid=torch.zeros(M, N, device="cuda"), M=M, N=N, K=K, lda=K, ldb=K, ldc=N,
                  ldr=N, drop=drop_desc(st, SITE_F8, 0.1), drop_where=1)
    _lib.check(lib.qst_gemm_nt_f8(a, 1, stream()))                   # taken with drop_where 1: the refusals are about the mask
    _lib.check(lib.qst_gemm_nt8_f8(a, 1, 0, stream()))
    torch.cuda.synchronize()
    assert not bool(torch.isnan(C).any())
    C.fill_(NAN)
    a.drop_where = 2
    assert lib.qst_gemm_nt_f8(a, 1, stream()) != 0
    assert lib.qst_gemm_nt8_f8(a, 1, 0, stream()) != 0 and lib.qst_gemm_nt8_f8(a, 1, 1, stream()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(C).all())
