"""The references of tests/test_gpu_ln_exchange.py (ln_exchange_cases) judged on the CPU before a kernel is compared with them:
they are torch's own LayerNorm and its autograd in fp64, and a result that is wrong the way the row-statistics exchange could
make it wrong -- a row normalised with the statistics of one 256-column tile, or with a neighbour row's -- lies outside the
tolerances the GPU tests use."""
import torch

import ln_exchange_cases as X


def operands(M=37, N=512, K=64, seed=3):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16).float()
    B = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).float()
    bias, resid = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    return A, B, bias, resid, gamma, beta


def test_forward_reference_is_torch_layer_norm_in_fp64():
    A, B, bias, resid, gamma, beta = operands()
    y, xhat, rstd = X.ln_fwd_ref(A, B, bias, resid, gamma, beta)
    v = A.double() @ B.double().t() + bias.double() + resid.double()
    ref = torch.nn.functional.layer_norm(v, (v.shape[1],), gamma.double(), beta.double(), X.EPS)
    torch.testing.assert_close(y, ref, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(xhat * gamma.double() + beta.double(), ref, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(rstd, 1 / (v.var(1, unbiased=False) + X.EPS).sqrt(), rtol=1e-12, atol=0)
    assert y.dtype == torch.float64 and rstd.shape == (A.shape[0],)


def test_backward_reference_is_fp64_autograd_where_xhat_and_rstd_are_exact():
    A, B, bias, resid, gamma, beta = operands(seed=4)
    g = torch.Generator().manual_seed(5)
    v = torch.randn(A.shape[0], B.shape[0], generator=g, dtype=torch.float64).requires_grad_(True)
    gm, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    dy = X.ln_bwd_dy(A, B, resid)
    torch.testing.assert_close(dy, A.double() @ B.double().t() + resid.double(), rtol=0, atol=0)
    (torch.nn.functional.layer_norm(v, (v.shape[1],), gm, bt, X.EPS) * dy).sum().backward()
    mu = v.detach().mean(1, keepdim=True)
    rstd = ((v.detach() - mu).square().mean(1) + X.EPS).rsqrt()
    xhat = (v.detach() - mu) * rstd[:, None]
    torch.testing.assert_close(X.ln_bwd_ds_ref(dy, gamma, xhat, rstd), v.grad, rtol=1e-10, atol=1e-12)
    dg, db = X.ln_bwd_param_ref(dy, xhat)
    torch.testing.assert_close(dg, gm.grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(db, bt.grad, rtol=1e-10, atol=1e-12)


def outside(got, ref, rtol, atol):
    return bool(((got - ref).abs() > atol + rtol * ref.abs()).any())


def test_a_row_normalised_with_the_wrong_statistics_lies_outside_the_tolerances():
    A, B, bias, resid, gamma, beta = operands(seed=6)
    y, xhat, rstd = X.ln_fwd_ref(A, B, bias, resid, gamma, beta)
    v = A.double() @ B.double().t() + bias.double() + resid.double()
    # one tile's statistics instead of the row's (a partner's granules never merged)
    t = v[:, :256]
    mu, var = t.mean(1, keepdim=True), t.var(1, unbiased=False, keepdim=True)
    y_tile = (v - mu) / (var + X.EPS).sqrt() * gamma.double() + beta.double()
    assert outside(y_tile, y, 1e-4, 2e-4) and outside(1 / (var[:, 0] + X.EPS).sqrt(), rstd, 1e-5, 0)
    # the neighbour row's statistics (a stale granule of another launch read as this one's)
    mu, rs = v.mean(1, keepdim=True).roll(1, 0), rstd.roll(1, 0)[:, None]
    assert outside((v - mu) * rs * gamma.double() + beta.double(), y, 1e-4, 2e-4)
    # mode 1: the row means of one tile only
    dy = X.ln_bwd_dy(A, B, resid)
    ds = X.ln_bwd_ds_ref(dy, gamma, xhat, rstd)
    g = dy * gamma.double()
    ds_tile = rstd[:, None] * (g - g[:, :256].mean(1, keepdim=True) - xhat * (g * xhat)[:, :256].mean(1, keepdim=True))
    assert outside(ds_tile, ds, 1e-4, 1e-4 * float(ds.abs().max()))


def test_subset_rows_are_the_edges_and_seeded_rows_between_them():
    r = X.subset_rows(33000, 256, 256, 256, seed=1)
    assert r.numel() == 768 and r.unique().numel() == 768 and bool((r[1:] > r[:-1]).all())
    assert r[:256].tolist() == list(range(256)) and r[-256:].tolist() == list(range(33000 - 256, 33000))
    assert torch.equal(r, X.subset_rows(33000, 256, 256, 256, seed=1))
    r = X.subset_rows(262200, 256, 56, 64, seed=2)
    assert r.numel() == 376 and int(r[-56]) == 262144 and 256 <= int(r[256]) and int(r[319]) < 262144
