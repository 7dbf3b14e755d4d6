"""The fp64 references of tests/test_gpu_ln_exchange.py, kept apart from it so that tests/test_ln_exchange_refs_host.py can judge
them on the CPU, against torch's own LayerNorm and its autograd, before any kernel is compared with them. Plain torch only:
nothing here needs the library or a GPU.

The launch under test (qst_gemm_nt8_ln, csrc/gemm8.hip) computes

  mode 0:  v = A.B^T + bias + resid ;  y = LayerNorm(v) = xhat * gamma + beta,  xhat = (v - mean) * rstd,
           rstd = 1 / sqrt(biased variance + eps)
  mode 1:  dy = A.B^T + resid ;  ds = the gradient of sum(dy * LayerNorm(v)) with respect to v, written with the xhat / rstd
           the caller hands in:  ds = rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * gamma ;
           dgamma = sum over rows of dy * xhat,  dbeta = sum over rows of dy.

Mode 1 takes xhat and rstd as DATA (the 16-bit copy a forward has stored), so its reference is that closed form evaluated in
fp64 on the same xhat / rstd: autograd through a LayerNorm would recompute both from some v, and no v has a 16-bit-rounded xhat
as its exact normalisation. The host test shows the closed form to be fp64 autograd of torch.nn.functional.layer_norm wherever
xhat / rstd ARE exact; dgamma / dbeta are taken by autograd as they stand (y = xhat * gamma + beta is linear in both)."""
import torch

EPS = 1e-12            # as test_gemm_nt_fused_layernorm


def ln_fwd_ref(A, B, bias, resid, gamma, beta, eps=EPS):
    """fp64 y, xhat [rows, N] and rstd [rows] of LayerNorm(A.B^T + bias + resid); the operands are taken as they are (the
    caller passes the 16-bit-rounded A and B)."""
    v = A.double() @ B.double().t() + resid.double()
    if bias is not None:
        v = v + bias.double()
    mu = v.mean(1, keepdim=True)
    rstd = ((v - mu).square().mean(1, keepdim=True) + eps).rsqrt()
    xhat = (v - mu) * rstd
    return xhat * gamma.double() + beta.double(), xhat, rstd[:, 0]


def ln_bwd_dy(A, B, resid):
    """fp64 dy = A.B^T + resid (mode 1 adds no bias)."""
    return A.double() @ B.double().t() + resid.double()


def ln_bwd_ds_ref(dy, gamma, xhat, rstd):
    """fp64 ds [rows, N] from dy and the xhat / rstd the kernel is given."""
    g = dy.double() * gamma.double()
    xh = xhat.double()
    return rstd.double()[:, None] * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))


def ln_bwd_param_ref(dy, xhat):
    """fp64 dgamma, dbeta [N] over all the rows given, by autograd of sum(dy * (xhat * gamma + beta))."""
    N = dy.shape[1]
    gamma = torch.ones(N, dtype=torch.float64, requires_grad=True)
    beta = torch.zeros(N, dtype=torch.float64, requires_grad=True)
    (dy.double() * (xhat.double() * gamma + beta)).sum().backward()
    return gamma.grad, beta.grad


def subset_rows(M, first, last, n_seeded, seed):
    """The rows a large case is compared with fp64 on: the first `first`, the last `last` and n_seeded distinct rows drawn
    from between them with a seeded generator; ascending, no row twice."""
    assert M > first + last + n_seeded
    g = torch.Generator().manual_seed(seed)
    mid = first + torch.randperm(M - first - last, generator=g)[:n_seeded].sort().values
    return torch.cat([torch.arange(first), mid, torch.arange(M - last, M)])
