"""GPU: qst_mnrl_stream_loss (csrc/mnrl_stream.hip), MultipleNegativesRankingLoss with no B x N term on the fp32 matrix
cores, against the yardstick of mnrl_helpers (sentence-transformers' formula in fp64 on the CPU with autograd): the cases,
seeds, floors and tolerances of test_gpu_mnrl.py, at one, two, three and five strips; the exact invariants of the plain
form; one shape past the limit of qst_mnrl_loss against a closed form; and the behaviour the old entry's tests pin."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import mnrl_helpers as M  # noqa: E402
from kernel_helpers import lib, ptr, stream  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import st_losses as S  # noqa: E402

SIMS = ("cos", "dot")


def check(out, grads, loss, ga, gc, D, what=""):
    """Prints every figure as a share of its tolerance, then asserts."""
    ev = M.value_error(out.item(), loss, D)
    ea, ec = M.grad_error(grads[0].cpu(), ga), M.grad_error(grads[1].cpu(), gc)
    print(f"  {what}: loss {out.item():.7f} ref {float(loss):.7f}; share of the tolerance: value {ev:.3f} grad_a {ea:.3f} "
          f"grad_c {ec:.3f}")
    assert torch.isfinite(out).all() and torch.isfinite(grads[0]).all() and torch.isfinite(grads[1]).all()
    assert ev <= 1.0 and ea <= 1.0 and ec <= 1.0


# ------------------------------------------------------------------ 1. kernel parity
@pytest.mark.parametrize("strip_rows", [64, 128, 0])
@pytest.mark.parametrize("trained", [0, 1])
@pytest.mark.parametrize("symmetric", [0, 1], ids=["plain", "symmetric"])
@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("B,N,D", M.SHAPES)
def test_kernel_matches_reference(lib, B, N, D, sim, symmetric, trained, strip_rows):
    a, c, loss, ga, gc = M.reference(B, N, D, sim, symmetric, trained)
    if N > 1:       # the softmax of the reference is not saturated: a wrong gradient has nowhere to hide
        assert loss.item() >= M.MIN_REF_LOSS and ga.abs().max().item() >= M.MIN_REF_GRAD
    out, grads = S.mnrl_stream_loss_raw(a.cuda(), c.cuda(), sim, M.SCALE, symmetric, strip_rows, want_grads=True)
    if (B, N, D) == (1, 1, 1):
        assert out.item() == 0.0 and not grads[0].any() and not grads[1].any()
    check(out, grads, loss, ga, gc, D, f"{B}x{N}x{D} {sim} sym={symmetric} trained={trained} strip={strip_rows}")
    # the forward-only call returns the same value
    fwd, none = S.mnrl_stream_loss_raw(a.cuda(), c.cuda(), sim, M.SCALE, symmetric, strip_rows)
    assert none == [None, None] and torch.equal(fwd, out)


# The shapes above are small enough that every product runs on 64 x 64 tiles and grad_a in one K chunk. These two reach the
# rest: (1100, 4100, 24) has 9 x 33 = 297 tiles of 128 x 128 in the score product (the larger tile is chosen from 256 on)
# and N > 4096, so grad_a is summed from two K chunks; (128, 16400, 256) has 129 x 2 such tiles in grad_c, which
# strip_rows 64 writes in the first strip and accumulates in the second. B, N and D end inside a tile.
@pytest.mark.parametrize("symmetric", [0, 1], ids=["plain", "symmetric"])
@pytest.mark.parametrize("B,N,D,sim,strip_rows", [(1100, 4100, 24, "cos", 0), (1100, 4100, 24, "dot", 512),
                                                  (128, 16400, 256, "cos", 64), (100, 16400, 255, "dot", 0)])
def test_large_tiles_and_k_chunks_match_reference(lib, B, N, D, sim, symmetric, strip_rows):
    a, c, loss, ga, gc = M.reference(B, N, D, sim, symmetric, 1)
    assert loss.item() >= M.MIN_REF_LOSS and ga.abs().max().item() >= M.MIN_REF_GRAD
    out, grads = S.mnrl_stream_loss_raw(a.cuda(), c.cuda(), sim, M.SCALE, symmetric, strip_rows, want_grads=True)
    check(out, grads, loss, ga, gc, D, f"{B}x{N}x{D} {sim} sym={symmetric} strip={strip_rows}")


# ------------------------------------------------------------------ 2. the exact invariants of the plain form
@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("B,N,D", [(257, 257, 32), (130, 260, 64)])
def test_plain_loss_and_grad_a_do_not_depend_on_the_strips(lib, B, N, D, sim):
    """A row's statistics and its gradient row depend on that row of the scores alone, and the K order of an output element
    does not depend on the tiling: out_loss and grad_a are the same bits at 5, 3, 2 and 1 strips. grad_c is summed over the
    strips and may move by rounding."""
    a, c, loss, ga, gc = M.reference(B, N, D, sim, 0, 1)
    w = torch.tensor([1.7], device="cuda")
    got = {s: S.mnrl_stream_loss_raw(a.cuda(), c.cuda(), sim, M.SCALE, 0, s, grad_out=w, want_grads=True)
           for s in (64, 128, 192, 0)}
    o0, g0 = got[0]
    assert g0[0].abs().max().item() > 0
    for s, (o, g) in got.items():
        assert torch.equal(o, o0) and torch.equal(g[0], g0[0]), s
        ec = M.grad_error(g[1].cpu() / 1.7, gc)
        print(f"  {B}x{N}x{D} {sim} strip={s}: grad_c share of the tolerance {ec:.3f}")
        assert ec <= 1.0


# ------------------------------------------------------------------ 3. past the limit of qst_mnrl_loss
def test_a_batch_past_the_old_limit_matches_the_closed_form(lib):
    """B = N = 46,344, D = 8, dot, scale 2, a[i] = c[i] = e_(i mod 8): every row of S holds n = 5793 entries of 2 and 7n of
    0, so with Z = n e^2 + 7n the loss is log Z - 2, and with grad_out = B every row of both gradients has
    2 (n e^2 / Z - 1) at its own coordinate and 2 n / Z elsewhere. B * ldS is past 2^31 - 1: the old entry refuses."""
    B = N = 46344
    D, scale = 8, 2.0
    assert B % D == 0
    idx = torch.arange(B, device="cuda") % D
    a = torch.zeros(B, D, device="cuda")
    a[torch.arange(B, device="cuda"), idx] = 1.0
    c = a.clone()
    out = torch.zeros(1, device="cuda")
    old_ws = torch.empty(16, dtype=torch.uint8, device="cuda")
    assert lib.qst_mnrl_loss(ptr(a), ptr(c), B, N, D, S.SCORE_DOT, scale, 0, ptr(out), None, None, None, ptr(old_ws),
                             2 ** 40, stream()) == -2                       # QST_ERR_UNSUPPORTED, before any launch
    w = torch.tensor([float(B)], device="cuda")
    out, grads = S.mnrl_stream_loss_raw(a, c, "dot", scale, False, 0, grad_out=w, want_grads=True)
    n = B // D
    Z = n * math.exp(2.0) + 7 * n
    want_loss = math.log(Z) - 2.0
    own, other = 2.0 * (n * math.exp(2.0) / Z - 1.0), 2.0 * n / Z
    want = torch.full((B, D), other, dtype=torch.float64)
    want[torch.arange(B), idx.cpu()] = own
    ev = M.value_error(out.item(), want_loss, D)
    ea, ec = M.grad_error(grads[0].cpu(), want), M.grad_error(grads[1].cpu(), want)
    print(f"  46344 x 46344 x 8: loss {out.item():.7f} closed form {want_loss:.7f}; share of the tolerance: value {ev:.3f} "
          f"grad_a {ea:.3f} grad_c {ec:.3f}")
    assert ev <= 1.0 and ea <= 1.0 and ec <= 1.0


# ------------------------------------------------------------------ 4. the call itself, at (33, 99, 768) in strips of 64
SHAPE = (33, 99, 768)


def inputs(sim, trained=1):
    B, N, D = SHAPE
    return [t.cuda() for t in M.case(B, N, D, sim, trained, 1000 * B + D)]


def raw_call(lib, a, c, sim, symmetric, out, grad_out, ga, gc, strip_rows=64):
    B, D = a.shape
    N = c.shape[0]
    nbytes = lib.qst_mnrl_stream_workspace_bytes(B, N, D, strip_rows)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    return lib.qst_mnrl_stream_loss(ptr(a), ptr(c), B, N, D, S._SIM_CODE.get(sim, sim), M.SCALE, symmetric, strip_rows,
                                    ptr(out), ptr(grad_out), ptr(ga), ptr(gc), ptr(ws), nbytes, stream())


@pytest.mark.parametrize("sim", SIMS)
def test_forward_only_writes_nothing_else_and_one_null_gradient_is_refused(lib, sim):
    a, c = inputs(sim)
    ga, gc = torch.full_like(a, -7.25), torch.full_like(c, -7.25)
    out = torch.zeros(1, device="cuda")
    assert raw_call(lib, a, c, sim, 1, out, None, None, None) == 0
    torch.cuda.synchronize()
    assert (ga == -7.25).all() and (gc == -7.25).all() and out.item() > 0
    assert raw_call(lib, a, c, sim, 1, out, None, ga, None) == -1
    assert raw_call(lib, a, c, sim, 1, out, None, None, gc) == -1
    assert raw_call(lib, a, c, 2, 1, out, None, ga, gc) == -1          # QST_SCORE_EUCLID
    assert raw_call(lib, a, c, sim, 1, out, None, ga, gc, strip_rows=-64) == -1
    torch.cuda.synchronize()
    assert (ga == -7.25).all() and (gc == -7.25).all()


@pytest.mark.parametrize("symmetric", [0, 1], ids=["plain", "symmetric"])
@pytest.mark.parametrize("sim", SIMS)
def test_grad_out_is_read_on_the_device_and_scales_the_gradients(lib, sim, symmetric):
    """grad_out = 3 gives 3 x the gradients of grad_out = NULL within 1 ulp per element (the upstream gradient multiplies
    the finished gradient), and the loss does not move."""
    a, c = inputs(sim)
    o1, g1 = S.mnrl_stream_loss_raw(a, c, sim, M.SCALE, symmetric, 64, want_grads=True)
    o3, g3 = S.mnrl_stream_loss_raw(a, c, sim, M.SCALE, symmetric, 64, grad_out=torch.tensor([3.0], device="cuda"),
                                    want_grads=True)
    assert torch.equal(o1, o3)
    for x1, x3 in zip(g1, g3):
        want = 3.0 * x1.double()
        ulp = torch.finfo(torch.float32).eps * want.abs().clamp_min(torch.finfo(torch.float32).tiny)
        assert ((x3.double() - want).abs() <= ulp).all()
        assert x1.abs().max().item() > 0


def test_two_identical_calls_are_bit_identical(lib):
    for sim in SIMS:
        for symmetric in (0, 1):
            a, c = inputs(sim)
            w = torch.tensor([1.7], device="cuda")
            o1, g1 = S.mnrl_stream_loss_raw(a, c, sim, M.SCALE, symmetric, 64, grad_out=w, want_grads=True)
            o2, g2 = S.mnrl_stream_loss_raw(a, c, sim, M.SCALE, symmetric, 64, grad_out=w, want_grads=True)
            assert torch.equal(o1, o2) and torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])


def test_non_default_stream_gives_the_same_result(lib):
    a, c = inputs("cos")
    o1, g1 = S.mnrl_stream_loss_raw(a, c, "cos", M.SCALE, 1, 64, want_grads=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        o2, g2 = S.mnrl_stream_loss_raw(a, c, "cos", M.SCALE, 1, 64, want_grads=True)
    side.synchronize()
    assert torch.equal(o1, o2) and torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])


def test_the_call_pair_is_capturable_in_a_graph(lib):
    """No host synchronisation, grad_out read on the device: a captured forward + backward call replays on new inputs and a
    new upstream gradient written into the same buffers."""
    (a1, c1), (a2, c2) = [inputs("cos", tr) for tr in (0, 1)]
    a, c, w = a1.clone(), c1.clone(), torch.tensor([1.0], device="cuda")
    S.mnrl_stream_loss_raw(a, c, "cos", M.SCALE, 1, 64, grad_out=w, want_grads=True)     # code objects loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fwd, _ = S.mnrl_stream_loss_raw(a, c, "cos", M.SCALE, 1, 64)
        out, grads = S.mnrl_stream_loss_raw(a, c, "cos", M.SCALE, 1, 64, grad_out=w, want_grads=True)
    a.copy_(a2), c.copy_(c2), w.fill_(2.5)
    graph.replay()
    torch.cuda.synchronize()
    want, want_g = S.mnrl_stream_loss_raw(a2, c2, "cos", M.SCALE, 1, 64, grad_out=torch.tensor([2.5], device="cuda"),
                                          want_grads=True)
    assert torch.equal(fwd, want) and torch.equal(out, want)
    assert torch.equal(grads[0], want_g[0]) and torch.equal(grads[1], want_g[1])


@pytest.mark.parametrize("symmetric", [0, 1], ids=["plain", "symmetric"])
def test_zero_rows_follow_the_clamp_of_normalize(lib, symmetric):
    """|x| < 1e-12: the normalised row is 0 and its gradient d_hat / 1e-12, as in qst_mnrl_loss."""
    a, c = [t.cpu().clone() for t in inputs("cos", 0)]
    a[2] = 0
    c[7] = 0
    c[70] = 0
    loss, ga, gc = M.reference_of(a, c, "cos", symmetric)
    assert ga[2].abs().max().item() > 1e10 and gc[7].abs().max().item() > 1e6      # the clamp, not a small norm
    out, grads = S.mnrl_stream_loss_raw(a.cuda(), c.cuda(), "cos", M.SCALE, symmetric, 64, want_grads=True)
    check(out, grads, loss, ga, gc, SHAPE[2], f"zero rows sym={symmetric}")
    torch.testing.assert_close(grads[0].cpu().double()[2], ga[2], rtol=1e-4, atol=1e-4 * ga[2].abs().max().item())
    for j in (7, 70):
        torch.testing.assert_close(grads[1].cpu().double()[j], gc[j], rtol=1e-4, atol=1e-4 * gc[j].abs().max().item())


@pytest.mark.parametrize("symmetric", [False, True], ids=["plain", "symmetric"])
@pytest.mark.parametrize("sim", SIMS)
def test_autograd_equals_the_raw_call(lib, sim, symmetric):
    a0, c0 = inputs(sim)
    a, c = a0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
    loss = S.multiple_negatives_ranking_loss_stream(a, c, M.SCALE, sim, symmetric, strip_rows=64)
    assert loss.dim() == 0
    (loss * 1.7).backward()
    out, grads = S.mnrl_stream_loss_raw(a0, c0, sim, M.SCALE, symmetric, 64, grad_out=torch.tensor([1.7], device="cuda"),
                                        want_grads=True)
    assert torch.equal(loss.detach().reshape(1), out) and torch.equal(a.grad, grads[0]) and torch.equal(c.grad, grads[1])
