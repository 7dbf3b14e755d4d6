"""The fp32 building blocks of the parity precision (QST_PREC_BF16X3, forward and backward) against fp64: the split-bf16 NT
GEMM's epilogues, transpose, exact-erf GELU and its derivative, the embedding sum, the LayerNorm backward from pre-norm rows,
the attention forward / backward with a full position-bias table, and the hidden-state dropout. Copies and gathers are
compared bit for bit; arithmetic at fp32-class tolerances."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import _lib  # noqa: E402
from oracle import dropout_ref as D  # noqa: E402
from kernel_helpers import attn_ref, drop_desc, drop_state, gemm_args, lib, ptr, stream  # noqa: E402,F401
from test_gpu_row_kernels import embed_inputs, embed_sum_ref  # noqa: E402

BAD_ARG, UNSUPPORTED = -1, -2
SQRT1_2 = 1.0 / math.sqrt(2.0)


def gelu64(x):
    return x * 0.5 * torch.erfc(-x * SQRT1_2)


def gelu_grad64(x):
    return 0.5 * torch.erfc(-x * SQRT1_2) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


# ------------------------------------------------------------------ split-bf16 NT GEMM epilogues
@pytest.mark.parametrize("M,N,K", [(1, 4, 32), (100, 60, 64), (129, 388, 3072), (4097, 1152, 64), (4097, 388, 32),
                                   (100, 1152, 3072), (129, 4, 3072), (1, 1152, 64)])
@pytest.mark.parametrize("padded", [False, True], ids=["dense", "ld_gt_n"])
def test_gemm_nt_x3_epilogues_match_fp64(lib, M, N, K, padded):
    """qst_gemm_nt_x3 epilogues 0 (+bias), 1 (+bias +resid, ldr > N), 2 (gelu), 4 (u and gelu(u)) and 5 ((dY W) * gelu'(aux))
    against fp64; with ldc > N the padding columns keep their NaN.
    Tolerance: rtol 1e-5 and, per element, 6 standard deviations of the split-bf16 product error. Each product a b is formed
    as ah bh + ah bl + al bh with a = ah + al + O(2^-18 a): an error of about 2^-17 |a b| of random sign, so a K-term sum is
    off by sigma ~ 2^-17 sqrt(sum (a b)^2) (6e-6 sqrt(K) for unit-normal operands). The epilogue-3 test's atol 2e-5 sqrt(K)
    is ~3.5 sigma: enough for its 10^5 outputs, exceeded by a few of the 10^6 - 10^7 here (measured 4.4 sigma at
    4097 x 1152 x 64). The GELU epilogues scale it by the largest slope of gelu / value of gelu', 1.13."""
    g = torch.Generator().manual_seed(M * 7 + N + K)
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    bias = torch.randn(N, generator=g)
    ldc = N + 8 if padded else N
    ldr = N + 12 if padded else N
    resid = torch.randn(M, ldr, generator=g)
    aux = torch.randn(M, ldc, generator=g) * 2
    Ad, Bd, biasd, residd, auxd = A.cuda(), B.cuda(), bias.cuda(), resid.cuda(), aux.cuda()
    acc = A.double() @ B.double().t()
    u = acc + bias.double()
    sigma = 2.0 ** -17 * torch.sqrt((A.double() ** 2) @ (B.double() ** 2).t())

    def close(got, want, slope=1.0):
        bound = 1e-5 * want.abs() + slope * 6 * sigma
        err = (got - want).abs()
        assert bool((err <= bound).all()), f"off by {float((err / bound).max()):.2f} of the bound"

    def run(epi, **kw):
        Cd = torch.full((M, ldc), float("nan"), device="cuda")
        C2 = torch.full((M, ldc), float("nan"), device="cuda")
        _lib.check(lib.qst_gemm_nt_x3(gemm_args(A=Ad, B=Bd, C=Cd, C2=C2, M=M, N=N, K=K, lda=K, ldb=K, ldc=ldc, **kw), epi,
                                      stream()), f"epi {epi}")
        Cc, C2c = Cd.cpu(), C2.cpu()
        assert bool(torch.isnan(Cc[:, N:]).all()), f"epi {epi} wrote past N"
        return Cc[:, :N].double(), C2c

    c, _ = run(0, bias=biasd)
    close(c, u)
    c, _ = run(1, bias=biasd, resid=residd, ldr=ldr)
    close(c, u + resid[:, :N].double())
    c, _ = run(2, bias=biasd)
    close(c, gelu64(u), 1.13)
    c, c2 = run(4, bias=biasd)
    close(c, u)
    close(c2[:, :N].double(), gelu64(u), 1.13)
    assert bool(torch.isnan(c2[:, N:]).all())
    c, _ = run(5, aux=auxd)
    close(c, acc * gelu_grad64(aux[:, :N].double()), 1.13)


def test_gemm_nt_x3_refuses_what_it_cannot_do(lib):
    """K % 32 and N % 4 (and, with a residual, ldr % 4: epilogue 1 reads it as 16-byte rows): QST_ERR_UNSUPPORTED;
    epilogue 4 without C2, 5 without aux, an unknown epilogue: QST_ERR_BAD_ARG. Nothing is launched."""
    M, N, K = 64, 64, 64
    A, B = torch.zeros(M, K, device="cuda"), torch.zeros(N, K, device="cuda")
    Cd, C2, aux = torch.zeros(M, N + 4, device="cuda"), torch.zeros(M, N, device="cuda"), torch.zeros(M, N, device="cuda")
    resid = torch.zeros(M, N + 4, device="cuda")
    base = dict(A=A, B=B, C=Cd, M=M, N=N, K=K, lda=K, ldb=K, ldc=N)
    assert lib.qst_gemm_nt_x3(gemm_args(**{**base, "K": 48}), 0, stream()) == UNSUPPORTED
    assert lib.qst_gemm_nt_x3(gemm_args(**{**base, "N": 62}), 0, stream()) == UNSUPPORTED
    for ldr in (N + 2, N + 1):
        assert lib.qst_gemm_nt_x3(gemm_args(**base, resid=resid, ldr=ldr), 1, stream()) == UNSUPPORTED
    assert lib.qst_gemm_nt_x3(gemm_args(**base), 4, stream()) == BAD_ARG
    assert lib.qst_gemm_nt_x3(gemm_args(**base, C2=C2), 5, stream()) == BAD_ARG
    for epi in (6, 7, -1):
        assert lib.qst_gemm_nt_x3(gemm_args(**base, C2=C2, aux=aux), epi, stream()) == BAD_ARG


# ------------------------------------------------------------------ transpose
SENT32 = 0x7FC0ABCD      # a NaN payload no copy of a finite value produces


@pytest.mark.parametrize("R", [1, 31, 33, 1000])
@pytest.mark.parametrize("Cn", [1, 31, 33, 1000])
def test_transpose_f32_is_exact(lib, R, Cn):
    """qst_transpose_f32 with ld_src > C and ld_dst > R: bit for bit, and the padding columns of dst keep their sentinel"""
    g = torch.Generator().manual_seed(R * 1000 + Cn)
    lds, ldd = Cn + 3, R + 5
    src = torch.randn(R, lds, generator=g)
    sd = src.cuda()
    dst = torch.full((Cn, ldd), SENT32, dtype=torch.int32, device="cuda")
    _lib.check(lib.qst_transpose_f32(sd.data_ptr(), R, Cn, lds, dst.data_ptr(), ldd, stream()))
    got = dst.cpu()
    assert torch.equal(got[:, :R], src[:, :Cn].t().contiguous().view(torch.int32))
    assert bool((got[:, R:] == SENT32).all())
    assert lib.qst_transpose_f32(sd.data_ptr(), R, Cn, Cn - 1, dst.data_ptr(), ldd, stream()) == BAD_ARG
    assert lib.qst_transpose_f32(sd.data_ptr(), R, Cn, lds, dst.data_ptr(), R - 1, stream()) == BAD_ARG


# ------------------------------------------------------------------ GELU
def gelu_inputs(g):
    n = 256 * 40 + 77                                               # not a multiple of the 256-thread block
    x = torch.empty(n)
    x[: n - 200] = torch.linspace(-12, 12, n - 200)
    x[n - 200: n - 12] = torch.randn(188, generator=g) * 4
    x[n - 12:] = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1e-40, -1e-40, 1e4, -1e4, 3e38, -3e38, -0.7518, 0.7518])
    return x


def ulp32(x):
    e = torch.frexp(x.abs().clamp_min(1e-300)).exponent - 1
    return torch.ldexp(torch.ones_like(x), e.clamp_min(-126) - 23)


def check_gelu_bounds(got, ref, x, parts, torch32, what):
    """Bound 1: 4 fp32 ulps relative where |ref| > 1e-6; bound 2: 1e-7 absolute below; plus the error the fp32 formula itself
    carries: erf rounded to fp32 near +-1 is off by up to 2^-24 absolutely (erff: a few of them), and 1 + erf does not shrink
    that error where erf -> -1 (x < -3), so the result may be off by a few 2^-24 times the magnitude of the terms that cancel
    (`parts`). torch's own fp32 gelu has the same cancellation; bound 3: the kernel's largest error is at most 4 times torch's."""
    err = (got.double() - ref).abs()
    bound = torch.where(ref.abs() > 1e-6, 4 * ulp32(ref), torch.full_like(ref, 1e-7))
    bound = torch.maximum(bound, 4 * 2.0 ** -24 * parts)
    bad = err > bound
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements out of bound, worst x = {float(x[(err / bound).argmax()])}"
    terr = (torch32.double() - ref).abs()
    assert float(err.max()) <= 4 * float(terr.max()) + 1e-30, f"{what}: {float(err.max())} vs torch fp32 {float(terr.max())}"


def test_gelu_f32_and_its_derivative_match_fp64(lib):
    """qst_gelu_f32 / qst_gelu_bwd_f32 (exact erf) against fp64 over [-12, 12], 0, +-tiny and +-large"""
    g = torch.Generator().manual_seed(11)
    x = gelu_inputs(g)
    n = x.numel()
    dh = torch.randn(n, generator=g)
    xd, dhd = x.cuda(), dh.cuda()
    h, du = torch.full((n,), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
    _lib.check(lib.qst_gelu_f32(xd.data_ptr(), n, h.data_ptr(), stream()))
    _lib.check(lib.qst_gelu_bwd_f32(dhd.data_ptr(), xd.data_ptr(), n, du.data_ptr(), stream()))
    x64 = x.double()
    erf = torch.erf(x64 * SQRT1_2).abs()
    check_gelu_bounds(h.cpu(), gelu64(x64), x, (0.5 * x64).abs() * erf, torch.nn.functional.gelu(x), "gelu")
    xr = x.clone().requires_grad_(True)
    torch.nn.functional.gelu(xr).backward(dh)
    parts = dh.double().abs() * (0.5 * erf + (x64 * torch.exp(-0.5 * x64 * x64)).abs().nan_to_num(0.0))
    check_gelu_bounds(du.cpu(), dh.double() * gelu_grad64(x64), x, parts, xr.grad, "gelu'")


# ------------------------------------------------------------------ embedding sum
@pytest.mark.parametrize("M", [37, 1001])
@pytest.mark.parametrize("H", [2, 65, 1024])
def test_embed_sum_f32_is_exact(lib, M, H):
    """qst_embed_sum_f32 = fp32 (word + type) + position, bit for bit, with type ids, with NULL type ids (row 0) and without
    a type table"""
    for types in ("ids", "null", "none"):
        g = torch.Generator().manual_seed(M + H)
        x = embed_inputs(M, H, g, types=types)
        d = {k: (v.cuda() if v is not None else None) for k, v in x.items()}
        s = torch.full((M, H), float("nan"), device="cuda")
        _lib.check(lib.qst_embed_sum_f32(ptr(d["ids"]), ptr(d["tid"]), ptr(d["pos"]), ptr(d["word"]), ptr(d["pe"]), ptr(d["te"]), M, H,
                                         s.data_ptr(), stream()))
        assert torch.equal(s.cpu(), embed_sum_ref(x)), types


# ------------------------------------------------------------------ LayerNorm backward from pre-norm rows
@pytest.mark.parametrize("M", [1, 37, 4099])
@pytest.mark.parametrize("H", [2, 100, 384, 1024])
def test_ln_bwd_f32_matches_fp64_autograd(lib, M, H):
    """qst_ln_bwd_f32 (mean / rstd recomputed from the pre-norm rows) against fp64 autograd of layer_norm; dgamma / dbeta are
    added into non-zero buffers. ds is bounded per row by 1e-5 of rstd * max|gamma dy| -- the size of the terms that cancel
    in it (at H = 2 they cancel completely: the true ds is ~0) -- widened by the error of the fp32 x-hat the kernel
    recomputes, a few fp32 ulps of (max|x| + |mean|) * rstd, which matters only in rows whose values nearly agree."""
    eps = 1e-12
    g = torch.Generator().manual_seed(M + H)
    s = torch.randn(M, H, generator=g) * 2 + 0.3
    gamma = 1 + 0.1 * torch.randn(H, generator=g)
    dy = torch.randn(M, H, generator=g)
    g0, b0 = torch.randn(H, generator=g), torch.randn(H, generator=g)
    sr, gr = s.double().requires_grad_(True), gamma.double().requires_grad_(True)
    br = torch.zeros(H, dtype=torch.float64, requires_grad=True)
    (torch.nn.functional.layer_norm(sr, (H,), gr, br, eps) * dy.double()).sum().backward()
    sd, gd, dyd = s.cuda(), gamma.cuda(), dy.cuda()
    ds = torch.full((M, H), float("nan"), device="cuda")
    dg, db = g0.cuda(), b0.cuda()
    _lib.check(lib.qst_ln_bwd_f32(dyd.data_ptr(), sd.data_ptr(), gd.data_ptr(), eps, M, H, ds.data_ptr(), dg.data_ptr(),
                                  db.data_ptr(), stream()))
    rstd = 1.0 / torch.sqrt(s.double().var(-1, unbiased=False) + eps)
    mean = s.double().mean(-1)
    xerr = 8 * 2.0 ** -24 * (s.double().abs().amax(-1) + mean.abs()) * rstd
    scale = (rstd * (1 + xerr / 1e-5))[:, None] * (gamma.double() * dy.double()).abs().amax(-1, keepdim=True)
    err = (ds.cpu().double() - sr.grad).abs()
    assert bool((err <= 1e-4 * sr.grad.abs() + 1e-5 * scale).all()), f"ds off by {float((err / scale).max()):.2e} x scale"
    torch.testing.assert_close(dg.cpu().double() - g0.double(), gr.grad, rtol=1e-5, atol=1e-5 * math.sqrt(M) * 4)
    torch.testing.assert_close(db.cpu().double() - b0.double(), br.grad, rtol=1e-5, atol=1e-5 * math.sqrt(M) * 4)
    assert lib.qst_ln_bwd_f32(dyd.data_ptr(), sd.data_ptr(), gd.data_ptr(), eps, 1, 1026, ds.data_ptr(), dg.data_ptr(),
                              db.data_ptr(), stream()) == UNSUPPORTED


# ------------------------------------------------------------------ attention
def attn_case(n, L, A, d, use_rel, seed):
    g = torch.Generator().manual_seed(seed)
    H = A * d
    qkv = torch.randn(n * L, 3 * H, generator=g)
    lens = torch.randint(max(1, L // 8), L + 1, (n,), generator=g)
    lens[0] = L
    lens[-1] = 1 if n > 1 else L
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    rel = (0.5 * torch.randn(A, L, L, generator=g)) if use_rel else None
    dctx = torch.randn(n * L, H, generator=g)
    qr = qkv.double().requires_grad_(True)
    relr = rel.double().requires_grad_(True) if use_rel else None
    ref = attn_ref(qr, mask, relr, n, L, A, d)
    (ref * dctx.double()).sum().backward()
    return qkv, mask, rel, dctx, ref.detach(), qr.grad, (relr.grad if use_rel else None)


def run_attn_bwd_f32(lib, qkv, ctx, dctx, mask, rel, n, L, A, d):
    H = A * d
    qd, cd, dcd, md, reld = qkv.cuda(), ctx.cuda(), dctx.cuda(), mask.cuda(), (rel.cuda() if rel is not None else None)
    dq = torch.full((n * L, 3 * H), float("nan"), device="cuda")
    drel = torch.zeros(A, L, L, device="cuda") if rel is not None else None
    _lib.check(lib.qst_attention_bwd_f32(qd.data_ptr(), cd.data_ptr(), dcd.data_ptr(), md.data_ptr(), ptr(reld), n, L, A, d,
                                         dq.data_ptr(), ptr(drel), stream()))
    torch.cuda.synchronize()
    return dq.cpu(), (drel.cpu() if rel is not None else None)


def check_attn_grads(dq, drel, gq, grel):
    scale = gq.abs().max().item()
    torch.testing.assert_close(dq.double(), gq, rtol=1e-4, atol=2e-5 * max(1.0, scale))
    if grel is not None:
        torch.testing.assert_close(drel.double(), grel, rtol=1e-4, atol=1e-4 * max(1.0, grel.abs().max().item()))


@pytest.mark.parametrize("L", [32, 288, 512])
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("use_rel", [False, True], ids=["nobias", "bias"])
def test_attention_x3_forward_and_fp32_backward_match_fp64(lib, L, d, use_rel):
    """qst_attention_fwd_x3 and qst_attention_bwd_f32 (no dropout) against fp64 autograd, ragged masks (one sequence with a
    single valid key), the full [A, L, L] bias and its gradient; the backward reads the kernel's own context"""
    n, A = 3, 2
    qkv, mask, rel, dctx, ref, gq, grel = attn_case(n, L, A, d, use_rel, 13 * L + d + int(use_rel))
    qd, md, reld = qkv.cuda(), mask.cuda(), (rel.cuda() if use_rel else None)
    ctx = torch.full((n * L, A * d), float("nan"), device="cuda")
    _lib.check(lib.qst_attention_fwd_x3(qd.data_ptr(), md.data_ptr(), ptr(reld), n, L, A, d, ctx.data_ptr(), stream()))
    ctx_c = ctx.cpu()
    torch.testing.assert_close(ctx_c.double(), ref, rtol=1e-4, atol=2e-5 * max(1.0, ref.abs().max().item()))
    dq, drel = run_attn_bwd_f32(lib, qkv, ctx_c, dctx, mask, rel, n, L, A, d)
    check_attn_grads(dq, drel, gq, grel)


@pytest.mark.parametrize("L", [1, 77, 300])
@pytest.mark.parametrize("d", [32, 64])
def test_attention_bwd_f32_at_lengths_the_x3_kernels_do_not_take(lib, L, d):
    """qst_attention_bwd_f32 accepts any L <= 512: at L = 1, 77, 300 (not multiples of 32; 300 spans two 256-key blocks) with
    the context of the fp64 reference, against fp64 autograd"""
    n, A = 2, 2
    qkv, mask, rel, dctx, ref, gq, grel = attn_case(n, L, A, d, True, 17 * L + d)
    dq, drel = run_attn_bwd_f32(lib, qkv, ref.float(), dctx, mask, rel, n, L, A, d)
    check_attn_grads(dq, drel, gq, grel)


# ------------------------------------------------------------------ hidden-state dropout
@pytest.mark.parametrize("n", [4, 1020, 1 << 20])
def test_dropout_apply_f32_matches_the_oracle_mask(lib, n):
    """qst_dropout_apply_f32: in * mask (+ resid) with the mask of oracle/dropout_ref, bit for bit, out of place and in place
    (out == in, as the parity path calls it)"""
    seed, step, site, prob = 4242, 7, D.site_attn_out(2), 0.1
    g = torch.Generator().manual_seed(n)
    x, r = torch.randn(n, generator=g), torch.randn(n, generator=g)
    mk = torch.from_numpy(D.multipliers(seed, step, site, n, prob))
    st = drop_state(lib, seed, step)
    dd = drop_desc(st, site, prob)
    xd, rd = x.cuda(), r.cuda()
    for resid in (None, rd):
        want = x * mk + (r if resid is not None else 0.0)
        out = torch.full((n,), float("nan"), device="cuda")
        _lib.check(lib.qst_dropout_apply_f32(C.byref(dd), xd.data_ptr(), ptr(resid), n, out.data_ptr(), stream()))
        assert torch.equal(out.cpu(), want)
        inplace = xd.clone()
        _lib.check(lib.qst_dropout_apply_f32(C.byref(dd), inplace.data_ptr(), ptr(resid), n, inplace.data_ptr(), stream()))
        assert torch.equal(inplace.cpu(), want)
    assert lib.qst_dropout_apply_f32(C.byref(dd), xd.data_ptr(), None, n - 2 if n > 4 else 6, xd.data_ptr(), stream()) == BAD_ARG
    assert lib.qst_dropout_apply_f32(None, xd.data_ptr(), None, n, xd.data_ptr(), stream()) == BAD_ARG
