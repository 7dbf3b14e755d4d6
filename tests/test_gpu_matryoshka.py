"""GPU: MatryoshkaLoss -- qst_mnrl_nested_loss (csrc/mnrl_nested.hip), its autograd, the loss class of st_losses.py on
both of its paths -- and `truncate_dim`, against the yardstick in matryoshka_helpers: sum_k w_k * the MNRL reference of
mnrl_helpers on the first d_k columns, fp64 on the CPU with autograd. The tolerances are those of test_gpu_mnrl.py (the
arithmetic is the same fp32 arithmetic): values within rtol = atol = max(1e-5, 1.5e-8 D), gradients within rtol 1e-4,
atol 1e-6 * max(1, max |reference gradient|)."""
import ctypes as C
import math
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import matryoshka_helpers as MH  # noqa: E402
import mnrl_helpers as M  # noqa: E402
from kernel_helpers import lib, ptr, stream  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import data, evaluation, st_losses as S, util  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import (InputExample, SentenceTransformer,  # noqa: E402
                                                                       encode_columns_fused)

NAN = float("nan")


def shares(out, terms, grads, loss, ref_terms, ga, gc, D):
    """Every figure as a share of its tolerance: (loss, worst term, grad_a, grad_c)."""
    ev = M.value_error(out.item(), loss, D)
    et = max(M.value_error(t, r, D) for t, r in zip(terms.tolist(), ref_terms.tolist()))
    return ev, et, M.grad_error(grads[0].cpu(), ga), M.grad_error(grads[1].cpu(), gc)


def check(out, terms, grads, loss, ref_terms, ga, gc, D, what=""):
    """Prints every figure as a share of its tolerance, then asserts."""
    ev, et, ea, ec = shares(out, terms, grads, loss, ref_terms, ga, gc, D)
    print(f"  {what}: loss {out.item():.7f} ref {loss.item():.7f}; share of the tolerance: value {ev:.3f} terms {et:.3f} "
          f"grad_a {ea:.3f} grad_c {ec:.3f}")
    assert torch.isfinite(out).all() and torch.isfinite(terms).all()
    assert torch.isfinite(grads[0]).all() and torch.isfinite(grads[1]).all()
    assert ev <= 1.0 and et <= 1.0 and ea <= 1.0 and ec <= 1.0


# ------------------------------------------------------------------ 1. kernel parity
@pytest.mark.parametrize("trained", [0, 1])
@pytest.mark.parametrize("symmetric", [0, 1], ids=["plain", "symmetric"])
@pytest.mark.parametrize("case", MH.CASES, ids=MH.case_id)
def test_kernel_matches_reference(lib, case, symmetric, trained):
    B, N, D, dims = case
    a, c, loss, ref_terms, ga, gc, term_grad = MH.reference(B, N, D, dims, symmetric, trained)
    MH.assert_not_saturated(N, ref_terms, term_grad)
    out, terms, grads = S.mnrl_nested_loss_raw(a.cuda(), c.cuda(), dims, MH.weights_of(dims), MH.SCALE, symmetric,
                                               want_grads=True)
    check(out, terms, grads, loss, ref_terms, ga, gc, D, f"{MH.case_id(case)} sym={symmetric} trained={trained}")
    # the forward-only call returns the same values
    fwd, fterms, none = S.mnrl_nested_loss_raw(a.cuda(), c.cuda(), dims, MH.weights_of(dims), MH.SCALE, symmetric)
    assert none == [None, None] and torch.equal(fwd, out) and torch.equal(fterms, terms)


# ------------------------------------------------------------------ 2. agreement with qst_mnrl_loss
@pytest.mark.parametrize("symmetric", [0, 1], ids=["plain", "symmetric"])
@pytest.mark.parametrize("B,N,D", [(7, 14, 33), (65, 195, 384)])
def test_one_full_width_agrees_with_qst_mnrl_loss(lib, B, N, D, symmetric):
    a, c = [t.cuda() for t in M.case(B, N, D, "cos", 1, 1000 * B + D)]
    ws = torch.empty(lib.qst_mnrl_workspace_bytes(B, N, D), dtype=torch.uint8, device="cuda")
    want, wa, wc = torch.empty(1, device="cuda"), torch.empty_like(a), torch.empty_like(c)
    assert lib.qst_mnrl_loss(ptr(a), ptr(c), B, N, D, S.SCORE_COS, MH.SCALE, symmetric, ptr(want), None, ptr(wa), ptr(wc),
                             ptr(ws), ws.numel(), stream()) == 0
    out, terms, grads = S.mnrl_nested_loss_raw(a, c, [D], [1.0], MH.SCALE, symmetric, want_grads=True)
    check(out, terms, grads, want.cpu().double()[0], want.cpu().double(), wa.cpu().double(), wc.cpu().double(), D,
          f"K=1 d=D {B}x{N}x{D} sym={symmetric}")


@pytest.mark.parametrize("symmetric", [0, 1], ids=["plain", "symmetric"])
def test_three_widths_agree_with_three_qst_mnrl_loss_calls(lib, symmetric):
    B, N, D, dims, weights = 33, 99, 384, [384, 100, 6], [1.0, 0.5, 0.25]
    a0, c0 = [t.cuda() for t in M.case(B, N, D, "cos", 1, 1000 * B + D)]
    a, c = a0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
    ref_terms, total = [], None
    for d, w in zip(dims, weights):
        t = S.multiple_negatives_ranking_loss(F.normalize(a[:, :d], p=2, dim=1).contiguous(),
                                              F.normalize(c[:, :d], p=2, dim=1).contiguous(), MH.SCALE, "cos", bool(symmetric))
        ref_terms.append(t.detach().cpu().double())
        total = t * w if total is None else total + t * w
    total.backward()
    loss64 = sum(w * t for w, t in zip(weights, ref_terms))
    out, terms, grads = S.mnrl_nested_loss_raw(a0, c0, dims, weights, MH.SCALE, symmetric, want_grads=True)
    check(out, terms, grads, loss64, torch.stack(ref_terms), a.grad.cpu().double(), c.grad.cpu().double(), D,
          f"K=3 against three calls sym={symmetric}")


# ------------------------------------------------------------------ 3. edges
@pytest.mark.parametrize("symmetric", [0, 1], ids=["plain", "symmetric"])
def test_zero_prefixes_follow_the_clamp_of_normalize(lib, symmetric):
    """An anchor and a candidate whose first d_1 entries are zero while the row is not: the narrow prefix is clamped
    (normalised row 0, gradient d_hat / 1e-12 on those columns), the wide one is an ordinary row."""
    dims, weights = [10, 3], [1.0, 0.5]
    a, c = M.case(5, 10, 10, "cos", 0, 5010)
    a, c = a.clone(), c.clone()
    a[2, :3] = 0
    c[7, :3] = 0
    loss, ref_terms, ga, gc, _ = MH.reference_of(a, c, dims, weights, symmetric)
    assert ga[2, :3].abs().max().item() > 1e10 and gc[7, :3].abs().max().item() > 1e5      # the clamp, not a small norm
    out, terms, grads = S.mnrl_nested_loss_raw(a.cuda(), c.cuda(), dims, weights, MH.SCALE, symmetric, want_grads=True)
    check(out, terms, grads, loss, ref_terms, ga, gc, 10, f"zero prefixes sym={symmetric}")
    ga_got, gc_got = grads[0].cpu().double(), grads[1].cpu().double()
    # the clamped columns on their own, and everything that is not clamped without the huge entries in its tolerance
    torch.testing.assert_close(ga_got[2, :3], ga[2, :3], rtol=1e-4, atol=1e-4 * ga[2, :3].abs().max().item())
    torch.testing.assert_close(gc_got[7, :3], gc[7, :3], rtol=1e-4, atol=1e-4 * gc[7, :3].abs().max().item())
    keep_a, keep_c = torch.ones_like(ga, dtype=torch.bool), torch.ones_like(gc, dtype=torch.bool)
    keep_a[2, :3] = False
    keep_c[7, :3] = False
    assert M.grad_error(ga_got[keep_a], ga[keep_a]) <= 1.0 and M.grad_error(gc_got[keep_c], gc[keep_c]) <= 1.0


@pytest.mark.parametrize("symmetric", [0, 1], ids=["plain", "symmetric"])
def test_width_one_contributes_its_value_and_no_gradient(lib, symmetric):
    B, N, D = 7, 14, 33
    a, c = M.case(B, N, D, "cos", 1, 1000 * B + D)
    loss, ref_terms, ga, gc, term_grad = MH.reference_of(a, c, [D, 1], [1.0, 0.5], symmetric)
    assert ref_terms[1].item() > MH.MIN_REF_LOSS and term_grad[1] < 1e-12
    out, terms, grads = S.mnrl_nested_loss_raw(a.cuda(), c.cuda(), [D, 1], [1.0, 0.5], MH.SCALE, symmetric, want_grads=True)
    check(out, terms, grads, loss, ref_terms, ga, gc, D, f"dims [D, 1] sym={symmetric}")
    # the gradient is that of the full width alone
    _, _, alone = S.mnrl_nested_loss_raw(a.cuda(), c.cuda(), [D], [1.0], MH.SCALE, symmetric, want_grads=True)
    assert M.grad_error(grads[0].cpu(), alone[0].cpu()) <= 1.0 and M.grad_error(grads[1].cpu(), alone[1].cpu()) <= 1.0


@pytest.mark.parametrize("B,N,D,dims", [(7, 14, 33, [17, 4]), (65, 130, 200, [130, 64, 5])])
def test_columns_past_the_widest_prefix_are_exact_zeros(lib, B, N, D, dims):
    a, c = M.case(B, N, D, "cos", 1, 1000 * B + D)
    weights = MH.weights_of(dims)
    loss, ref_terms, ga, gc, _ = MH.reference_of(a, c, dims, weights, 1)
    a, c = a.cuda(), c.cuda()
    out, terms = torch.empty(1, device="cuda"), torch.empty(len(dims), device="cuda")
    g_a, g_c = torch.full_like(a, NAN), torch.full_like(c, NAN)
    assert raw_call(lib, a, c, dims, weights, 1, out, terms, None, g_a, g_c) == 0
    top = max(dims)
    for g in (g_a, g_c):
        tail = g[:, top:]
        assert tail.numel() > 0 and (tail == 0).all() and not torch.signbit(tail).any()
    check(out, terms, [g_a, g_c], loss, ref_terms, ga, gc, D, f"max d {top} < D {D}")


def test_unsorted_dims_give_the_same_result_in_the_callers_order(lib):
    B, N, D = 33, 99, 768
    a, c = [t.cuda() for t in M.case(B, N, D, "cos", 1, 1000 * B + D)]
    dims, weights = [100, 768, 6, 256], [0.5, 1.0, 0.125, 0.25]
    order = [2, 0, 3, 1]                                    # ascending widths
    o1, t1, g1 = S.mnrl_nested_loss_raw(a, c, dims, weights, MH.SCALE, 1, want_grads=True)
    o2, t2, g2 = S.mnrl_nested_loss_raw(a, c, [dims[i] for i in order], [weights[i] for i in order], MH.SCALE, 1,
                                        want_grads=True)
    assert torch.equal(t1[order], t2)                       # the same terms, each where its width stands
    assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])
    assert M.value_error(o1.item(), o2.item(), D) <= 1.0    # the weighted sum runs in the caller's order: rounding only


# ------------------------------------------------------------------ 4. call discipline
def raw_call(lib, a, c, dims, weights, symmetric, out, terms, grad_out, ga, gc, ws=None, nbytes=None, scale=MH.SCALE,
             K=None, B=None, N=None, D=None):
    B = a.shape[0] if B is None else B
    N = c.shape[0] if N is None else N
    D = a.shape[1] if D is None else D
    K = len(dims) if K is None else K
    if ws is None:
        ws = torch.empty(max(lib.qst_mnrl_nested_workspace_bytes(a.shape[0], c.shape[0], a.shape[1], len(dims)), 16),
                         dtype=torch.uint8, device="cuda")
        nbytes = ws.numel() if nbytes is None else nbytes
    hd = None if dims is None else (C.c_int32 * len(dims))(*dims)
    hw = None if weights is None else (C.c_float * len(weights))(*weights)
    return lib.qst_mnrl_nested_loss(ptr(a), ptr(c), B, N, D, hd, hw, K, scale, symmetric, ptr(out), ptr(terms), ptr(grad_out),
                                    ptr(ga), ptr(gc), ws if isinstance(ws, int) else ptr(ws), nbytes, stream())


def banded(n, band=64):
    """(whole, view): n floats with `band` NaN floats on either side, all NaN to begin with."""
    whole = torch.full((n + 2 * band,), NAN, device="cuda")
    return whole, whole[band:band + n]


def bands_untouched(whole, n, band=64):
    return bool(torch.isnan(whole[:band]).all() and torch.isnan(whole[band + n:]).all())


def test_forward_only_writes_its_outputs_and_nothing_else(lib):
    B, N, D, dims = 7, 14, 33, [33, 17, 4]
    a, c = [t.cuda() for t in M.case(B, N, D, "cos", 1, 7033)]
    (wo, out), (wt, terms), (wa, ga), (wc, gc) = banded(1), banded(3), banded(B * D), banded(N * D)
    assert raw_call(lib, a, c, dims, [1.0, 0.5, 0.25], 1, out, terms, None, None, None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(terms).all() and out.item() > 0
    assert bands_untouched(wo, 1) and bands_untouched(wt, 3)
    assert torch.isnan(wa).all() and torch.isnan(wc).all()
    # with gradients: the bands around all four outputs stay
    assert raw_call(lib, a, c, dims, [1.0, 0.5, 0.25], 1, out, terms, None, ga, gc) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(ga).all() and torch.isfinite(gc).all()
    assert bands_untouched(wo, 1) and bands_untouched(wt, 3) and bands_untouched(wa, B * D) and bands_untouched(wc, N * D)
    # out_terms may be NULL
    assert raw_call(lib, a, c, dims, [1.0, 0.5, 0.25], 1, out, None, None, None, None) == 0


def test_bad_arguments_are_refused_and_write_nothing(lib):
    B, N, D, dims, weights = 7, 14, 33, [33, 17, 4], [1.0, 0.5, 0.25]
    a, c = [t.cuda() for t in M.case(B, N, D, "cos", 1, 7033)]
    out, terms = torch.full((1,), -7.25, device="cuda"), torch.full((3,), -7.25, device="cuda")
    ga, gc = torch.full_like(a, -7.25), torch.full_like(c, -7.25)
    nbytes = lib.qst_mnrl_nested_workspace_bytes(B, N, D, 3)
    ws = torch.zeros(nbytes + 16, dtype=torch.uint8, device="cuda")

    def call(a=a, c=c, dims=dims, weights=weights, symmetric=1, out=out, terms=terms, ga=ga, gc=gc, ws=ws, nb=nbytes, **kw):
        kw = {**dict(B=B, N=N, D=D), **kw}                  # a NULL input has no shape to take them from
        return raw_call(lib, a, c, dims, weights, symmetric, out, terms, None, ga, gc, ws=ws, nbytes=nb, **kw)

    assert call() == 0                                      # the arguments the bad ones are varied from are good
    torch.cuda.synchronize()
    out.fill_(-7.25), terms.fill_(-7.25), ga.fill_(-7.25), gc.fill_(-7.25), ws.zero_()
    nine = list(range(1, 10))
    bad = [dict(ga=None), dict(gc=None),                                        # exactly one NULL gradient
           dict(K=0), dict(dims=nine, weights=[1.0] * 9),                       # K outside 1 .. 8
           dict(dims=[33, 0, 4]), dict(dims=[34, 17, 4]), dict(dims=[33, -2, 4]),   # a width outside 1 .. D
           dict(dims=[33, 17, 17]),                                             # a repeated width
           dict(weights=[1.0, math.inf, 0.25]), dict(weights=[1.0, 0.5, math.nan]),
           dict(dims=None, K=3), dict(weights=None),
           dict(nb=nbytes - 1), dict(nb=0), dict(ws=ws.data_ptr() + 1), dict(ws=None, nb=nbytes),
           dict(scale=0.0), dict(scale=-1.0), dict(scale=math.inf), dict(scale=math.nan), dict(symmetric=2),
           dict(symmetric=-1), dict(B=0), dict(N=B - 1), dict(D=0), dict(a=None), dict(c=None), dict(out=None)]
    for kw in bad:
        if kw.get("ws", 0) is None:
            got = lib.qst_mnrl_nested_loss(ptr(a), ptr(c), B, N, D, (C.c_int32 * 3)(*dims), (C.c_float * 3)(*weights), 3,
                                           MH.SCALE, 1, ptr(out), ptr(terms), None, ptr(ga), ptr(gc), None, nbytes, stream())
        else:
            got = call(**kw)
        assert got == -1, kw
    torch.cuda.synchronize()
    assert (out == -7.25).all() and (terms == -7.25).all() and (ga == -7.25).all() and (gc == -7.25).all()
    assert not ws.any()


def test_workspace_of_exactly_the_queried_size(lib):
    B, N, D, dims, weights = 5, 5, 10, [10, 7, 3, 2], [1.0, 0.5, 0.25, 0.125]
    a, c = [t.cuda() for t in M.case(B, N, D, "cos", 1, 5010)]
    nbytes = lib.qst_mnrl_nested_workspace_bytes(B, N, D, 4)
    assert nbytes >= 4 * B * 8 * 4
    whole = torch.full((nbytes + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = whole[256:256 + nbytes]
    out, terms, ga, gc = torch.empty(1, device="cuda"), torch.empty(4, device="cuda"), torch.empty_like(a), torch.empty_like(c)
    assert raw_call(lib, a, c, dims, weights, 1, out, terms, None, ga, gc, ws=ws, nbytes=nbytes - 1) == -1
    assert raw_call(lib, a, c, dims, weights, 1, out, terms, None, ga, gc, ws=ws, nbytes=nbytes) == 0
    torch.cuda.synchronize()
    assert (whole[:256] == 0xA5).all() and (whole[256 + nbytes:] == 0xA5).all()         # nothing beyond what was asked for
    want, _, wg = S.mnrl_nested_loss_raw(a, c, dims, weights, MH.SCALE, 1, want_grads=True)
    assert torch.equal(out, want) and torch.equal(ga, wg[0]) and torch.equal(gc, wg[1])


# ------------------------------------------------------------------ 5. device-side behaviour
CASE5 = (65, 195, 768, [768, 512, 256, 128, 64])


@pytest.mark.parametrize("symmetric", [0, 1], ids=["plain", "symmetric"])
def test_grad_out_is_read_on_the_device_and_scales_the_gradients(lib, symmetric):
    """grad_out = 65536 (the first loss scale of use_amp) gives 65536 x the gradients of grad_out = NULL to fp32 rounding
    -- exactly, as a power of two -- and the loss does not move; so does 3, within 1 ulp per element."""
    B, N, D, dims = CASE5
    a, c = [t.cuda() for t in M.case(B, N, D, "cos", 1, 1000 * B + D)]
    w = MH.weights_of(dims)
    o1, _, g1 = S.mnrl_nested_loss_raw(a, c, dims, w, MH.SCALE, symmetric, want_grads=True)
    for scale in (65536.0, 3.0):
        og, _, gg = S.mnrl_nested_loss_raw(a, c, dims, w, MH.SCALE, symmetric, grad_out=torch.tensor([scale], device="cuda"),
                                           want_grads=True)
        assert torch.equal(o1, og)
        for x1, xg in zip(g1, gg):
            want = scale * x1.double()
            ulp = torch.finfo(torch.float32).eps * want.abs().clamp_min(torch.finfo(torch.float32).tiny)
            assert ((xg.double() - want).abs() <= ulp).all()
            assert x1.abs().max().item() > 0


def test_two_identical_calls_are_bit_identical(lib):
    for case in [MH.CASES[8], MH.CASES[7], MH.CASES[3]]:
        B, N, D, dims = case
        for symmetric in (0, 1):
            a, c = [t.cuda() for t in M.case(B, N, D, "cos", 1, 1000 * B + D)]
            w = torch.tensor([1.7], device="cuda")
            r1 = S.mnrl_nested_loss_raw(a, c, dims, MH.weights_of(dims), MH.SCALE, symmetric, grad_out=w, want_grads=True)
            r2 = S.mnrl_nested_loss_raw(a, c, dims, MH.weights_of(dims), MH.SCALE, symmetric, grad_out=w, want_grads=True)
            assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
            assert torch.equal(r1[2][0], r2[2][0]) and torch.equal(r1[2][1], r2[2][1])


def test_non_default_stream_gives_the_same_result(lib):
    B, N, D, dims = MH.CASES[5]
    a, c = [t.cuda() for t in M.case(B, N, D, "cos", 1, 1000 * B + D)]
    o1, t1, g1 = S.mnrl_nested_loss_raw(a, c, dims, MH.weights_of(dims), MH.SCALE, 1, want_grads=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        o2, t2, g2 = S.mnrl_nested_loss_raw(a, c, dims, MH.weights_of(dims), MH.SCALE, 1, want_grads=True)
    side.synchronize()
    assert torch.equal(o1, o2) and torch.equal(t1, t2) and torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])


def test_the_call_pair_is_capturable_in_a_graph(lib):
    """No host synchronisation, grad_out read on the device: a captured forward + backward call pair replays on new inputs
    and a new upstream gradient written into the same buffers, with the bits of the eager calls."""
    dims, weights = [33, 32, 17, 4], MH.weights_of([33, 32, 17, 4])
    (a1, c1), (a2, c2) = [[t.cuda() for t in M.case(7, 14, 33, "cos", tr, 7033)] for tr in (0, 1)]
    a, c, w = a1.clone(), c1.clone(), torch.tensor([1.0], device="cuda")
    S.mnrl_nested_loss_raw(a, c, dims, weights, MH.SCALE, 1, grad_out=w, want_grads=True)   # code objects loaded first
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fwd, fterms, _ = S.mnrl_nested_loss_raw(a, c, dims, weights, MH.SCALE, 1)
        out, terms, grads = S.mnrl_nested_loss_raw(a, c, dims, weights, MH.SCALE, 1, grad_out=w, want_grads=True)
    a.copy_(a2), c.copy_(c2), w.fill_(2.5)
    graph.replay()
    torch.cuda.synchronize()
    want, want_t, want_g = S.mnrl_nested_loss_raw(a2, c2, dims, weights, MH.SCALE, 1,
                                                  grad_out=torch.tensor([2.5], device="cuda"), want_grads=True)
    assert torch.equal(fwd, want) and torch.equal(out, want) and torch.equal(fterms, want_t) and torch.equal(terms, want_t)
    assert torch.equal(grads[0], want_g[0]) and torch.equal(grads[1], want_g[1])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_autograd_returns_gradients_in_the_input_dtypes(lib, dtype):
    dims = [384, 128, 32]
    a0, c0 = [t.cuda().to(dtype) for t in M.case(8, 16, 384, "cos", 1, 8384)]
    a, c = a0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
    loss = S.matryoshka_mnrl_loss(a, c, dims, None, 20.0, True)
    assert loss.dim() == 0
    (loss * 1.7).backward()
    assert a.grad.dtype == dtype and c.grad.dtype == dtype
    out, _, grads = S.mnrl_nested_loss_raw(a0.float(), c0.float(), dims, [1.0] * 3, 20.0, True,
                                           grad_out=torch.tensor([1.7], device="cuda"), want_grads=True)
    assert torch.equal(loss.detach().reshape(1), out)
    assert torch.equal(a.grad, grads[0].to(dtype)) and torch.equal(c.grad, grads[1].to(dtype))


# ------------------------------------------------------------------ 6. the class on a real encoder
WORDS = "a man rides red horse two dogs play in park woman eats green apple near old bridge small cat sleeps".split()
DIMS, WEIGHTS = [64, 24, 10], [1.0, 0.5, 0.25]             # tiny-bert's embeddings are 64 wide


def sent(i, n):
    rng = np.random.RandomState(i)
    return " ".join(rng.choice(WORDS, size=n))


def examples(n, k, label=None):
    """(anchor, positive that shares the anchor's words[, an unrelated hard negative])."""
    return [InputExample(texts=[sent(i, 9), sent(i, 9) + " now", sent(1000 + i, 5 + i % 7)][:k],
                         **({} if label is None else {"label": label(i)})) for i in range(n)]


class Tap(nn.Module):
    """The model, keeping hold of the sentence embeddings it returns (and of their gradients)."""

    def __init__(self, model):
        super().__init__()
        self.model, self.cfg, self.seen = model, model.cfg, []

    def forward(self, feats):
        out = self.model(feats)
        out["sentence_embedding"].retain_grad()
        self.seen.append(out["sentence_embedding"])
        return out


@pytest.fixture(scope="module")
def model():
    return SentenceTransformer("tiny-bert", device="cuda")


def batch_of(model, k, label=None):
    feats, labels = model.smart_batching_collate(examples(16, k, label))
    return [{key: v.cuda() for key, v in f.items()} for f in feats], labels.cuda()


def one_backward(model, lm, feats, labels):
    enc = model._enc
    enc.ensure_train_state()
    enc.grads.zero_()
    loss = lm([dict(f) for f in feats], labels)
    loss.backward()
    g = torch.cat([v.reshape(-1) for v in enc.grad_views().values()]).clone()
    enc.grads.zero_()
    return loss.detach(), g


BOTH = [S.MultipleNegativesRankingLoss, S.MultipleNegativesSymmetricRankingLoss]


@pytest.mark.parametrize("fused_dims", [True, False], ids=["one_call", "per_width"])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("cls", BOTH, ids=["plain", "symmetric"])
def test_class_equals_torch_ops_on_the_same_embeddings(model, cls, k, fused_dims):
    feats, labels = batch_of(model, k)
    model.train()
    tap = Tap(model)
    lm = S.MatryoshkaLoss(tap, cls(tap), DIMS, WEIGHTS, fused_dims=fused_dims)
    loss, _ = one_backward(model, lm, feats, labels)
    assert len(tap.seen) == 1 and tap.seen[0].shape[0] == 16 * k         # one fused pass whatever the number of widths
    emb = tap.seen[0]
    a64, c64 = emb.detach()[:16].double().requires_grad_(True), emb.detach()[16:].double().requires_grad_(True)
    ref, terms = MH.matryoshka_ref(a64, c64, DIMS, WEIGHTS, cls._symmetric, 20.0)
    ref.backward()
    D = emb.shape[1]
    ev = M.value_error(loss.item(), ref.item(), D)
    eg = M.grad_error(emb.grad, torch.cat([a64.grad, c64.grad], 0))
    print(f"  Matryoshka({cls.__name__}) k={k} fused_dims={fused_dims}: loss {loss.item():.7f} torch ops {ref.item():.7f}; "
          f"share of the tolerance: value {ev:.3f} embedding gradients {eg:.3f}")
    assert min(t.item() for t in terms) > M.MIN_REF_LOSS and ev <= 1.0 and eg <= 1.0


@pytest.mark.parametrize("cls", BOTH, ids=["plain", "symmetric"])
def test_fused_dims_false_equals_fused_dims_true(model, cls):
    feats, labels = batch_of(model, 3)
    model.train()
    got = {}
    for fused_dims in (True, False):
        tap = Tap(model)
        loss, g = one_backward(model, S.MatryoshkaLoss(tap, cls(tap), DIMS, WEIGHTS, fused_dims=fused_dims), feats, labels)
        got[fused_dims] = (loss, tap.seen[0].detach(), tap.seen[0].grad.clone(), g)
    (l1, e1, d1, g1), (l0, e0, d0, g0) = got[True], got[False]
    assert torch.equal(e1, e0)                               # the same embeddings went in
    assert M.value_error(l1.item(), l0.item(), e1.shape[1]) <= 1.0 and M.grad_error(d1, d0) <= 1.0
    assert g1.norm().item() > 0 and (g1 - g0).norm().item() <= 2e-2 * g1.norm().item()


def test_a_foreign_similarity_fct_or_nine_widths_run_per_width(model):
    feats, labels = batch_of(model, 2)
    model.eval()
    seen = []

    def foreign(x, y):
        seen.append(x.shape[1])
        return util.cos_sim(x, y)

    with torch.no_grad():
        got = S.MatryoshkaLoss(model, S.MultipleNegativesRankingLoss(model, similarity_fct=foreign), DIMS, WEIGHTS)(feats, labels)
        want = S.MatryoshkaLoss(model, S.MultipleNegativesRankingLoss(model), DIMS, WEIGHTS)(feats, labels)
        nine = list(range(64, 55, -1))
        many = S.MatryoshkaLoss(model, S.MultipleNegativesRankingLoss(model), nine)
        assert not many._one_call(9) and many._one_call(8)
        v9 = many(feats, labels)
        v8 = S.MatryoshkaLoss(model, S.MultipleNegativesRankingLoss(model), nine[:8])(feats, labels)
        v1 = S.MatryoshkaLoss(model, S.MultipleNegativesRankingLoss(model), nine[8:])(feats, labels)
    assert seen == DIMS
    assert M.value_error(got.item(), want.item(), 64) <= 1.0
    assert M.value_error(v9.item(), v8.item() + v1.item(), 64) <= 1.0


def test_n_dims_per_step_uses_exactly_the_sampled_widths(model):
    feats, labels = batch_of(model, 2)
    model.eval()
    dims, weights = [64, 32, 16, 8], [1.0, 0.5, 0.25, 0.125]
    for fused_dims in (True, False):
        lm = S.MatryoshkaLoss(model, S.MultipleNegativesRankingLoss(model), dims, weights, n_dims_per_step=2,
                              fused_dims=fused_dims)
        picks = set()
        for seed in range(4):
            random.seed(seed)
            idx = random.sample(range(4), 2)
            picks.add(tuple(idx))
            random.seed(seed)
            with torch.no_grad():
                got = lm(feats, labels)
                emb = encode_columns_fused(model, [dict(f) for f in feats])
            ref, _ = MH.matryoshka_ref(emb[0].double(), emb[1].double(), [dims[i] for i in idx], [weights[i] for i in idx],
                                       False, 20.0)
            allw, _ = MH.matryoshka_ref(emb[0].double(), emb[1].double(), dims, weights, False, 20.0)
            assert M.value_error(got.item(), ref.item(), 64) <= 1.0
            assert M.value_error(got.item(), allw.item(), 64) > 100.0
        assert len(picks) > 1


def cos_composition(u, v, labels, dims, weights):
    total = 0
    for d, w in zip(dims, weights):
        cos = (F.normalize(u[:, :d], dim=1) * F.normalize(v[:, :d], dim=1)).sum(1)
        total = total + w * F.mse_loss(cos, labels.to(cos.dtype))
    return total


def triplet_composition(a, p, n, labels, dims, weights):
    total = 0
    for d, w in zip(dims, weights):
        x, y, z = [F.normalize(t[:, :d], dim=1) for t in (a, p, n)]
        total = total + w * torch.relu(F.pairwise_distance(x, y) - F.pairwise_distance(x, z) + 0.5).mean()
    return total


class Composition(nn.Module):
    """The torch composition as a loss of its own: one fused pass, then torch ops only."""

    def __init__(self, model, fn):
        super().__init__()
        self.model, self.fn = model, fn

    def forward(self, feats, labels):
        return self.fn(*encode_columns_fused(self.model, list(feats)), labels, DIMS, WEIGHTS)


@pytest.mark.parametrize("name", ["cosine", "triplet"])
def test_generic_path_equals_the_torch_composition(model, name):
    """Loss and embedding gradients against fp64 torch ops on the same embeddings; the encoder gradients against those of
    the same composition in fp32 torch ops behind the same encoder pass (two bf16 backward passes: the bound of
    test_class_fused_pass_equals_one_pass_per_column)."""
    if name == "cosine":
        feats, labels = batch_of(model, 2, label=lambda i: float(i % 3) / 2)
        make, fn, k = (lambda m: S.CosineSimilarityLoss(m)), cos_composition, 2
    else:
        feats, labels = batch_of(model, 3)
        make, fn, k = (lambda m: S.TripletLoss(m, triplet_margin=0.5)), triplet_composition, 3
    model.train()
    tap = Tap(model)
    loss, g = one_backward(model, S.MatryoshkaLoss(tap, make(tap), DIMS, WEIGHTS), feats, labels)
    assert len(tap.seen) == 1 and tap.seen[0].shape[0] == 16 * k
    emb = tap.seen[0]
    parts = [t.double().requires_grad_(True) for t in emb.detach().split(16, 0)]
    ref = fn(*parts, labels.double(), DIMS, WEIGHTS)
    ref.backward()
    D = emb.shape[1]
    ev = M.value_error(loss.item(), ref.item(), D)
    eg = M.grad_error(emb.grad, torch.cat([t.grad for t in parts], 0))
    print(f"  Matryoshka({name}): loss {loss.item():.7f} torch ops {ref.item():.7f}; share of the tolerance: value {ev:.3f} "
          f"embedding gradients {eg:.3f}")
    assert ref.item() > 1e-3 and emb.grad.abs().max().item() > 0 and ev <= 1.0 and eg <= 1.0
    l2, g2 = one_backward(model, Composition(model, fn), feats, labels)
    assert abs(l2.item() - loss.item()) < 2e-4
    assert g.norm().item() > 0 and (g - g2).norm().item() <= 2e-2 * g.norm().item()


def test_embed_is_restored_after_an_exception_in_the_base_loss(model):
    feats, labels = batch_of(model, 2)
    model.eval()

    class Boom(RuntimeError):
        pass

    def failing(x, y):
        raise Boom()

    base = S.MultipleNegativesRankingLoss(model, similarity_fct=failing)
    lm = S.MatryoshkaLoss(model, base, DIMS)
    with pytest.raises(Boom), torch.no_grad():
        lm(feats, labels)
    assert "_embed" not in base.__dict__ and base._embed.__func__ is S._TupleLoss._embed
    with torch.no_grad():                                   # and the base loss embeds at the full width again
        base.similarity_fct = lambda x, y: util.cos_sim(x, y)
        full = base(feats, labels)
        want = S.MultipleNegativesRankingLoss(model)(feats, labels)
    assert M.value_error(full.item(), want.item(), 64) <= 1.0


@pytest.mark.parametrize("use_amp", [False, True])
@pytest.mark.parametrize("cls", BOTH, ids=["plain", "symmetric"])
def test_fit_lowers_the_loss_on_its_pairs(cls, use_amp):
    """5 epochs over 16 pairs whose positives share their anchors' words; under use_amp the loss scale reaches the kernel
    as grad_out, a device scalar."""
    random.seed(11)
    m = SentenceTransformer("tiny-bert", device="cuda")          # a fresh model: amp schedule counters persist per model
    pairs = examples(16, 2)
    lm = S.MatryoshkaLoss(m, cls(m), DIMS, WEIGHTS)
    feats, labels = m.smart_batching_collate(pairs)

    def value():
        m.eval()
        with torch.no_grad():
            return lm([{k: v.cuda() for k, v in f.items()} for f in feats], labels.cuda()).item()

    before = value()
    dl = data.NoDuplicatesDataLoader(list(pairs), 8)
    m.fit([(dl, lm)], epochs=5, warmup_steps=0, scheduler="constantlr", optimizer_params={"lr": 1e-3}, dropout=0,
          use_amp=use_amp, show_progress_bar=False)
    after = value()
    print(f"  fit Matryoshka({cls.__name__}) amp={use_amp}: loss on the 16 pairs {before:.5f} -> {after:.5f}")
    assert np.isfinite(after) and after < before
    assert torch.isfinite(m._enc.params).all()


# ------------------------------------------------------------------ 7. truncate_dim
SENTS = [sent(i, 3 + i % 9) for i in range(21)]


def test_encode_truncates_bit_for_bit_and_before_normalising(model):
    model.truncate_dim = None
    full = model.encode(SENTS, batch_size=8)
    assert full.shape == (21, 64)
    for d in (1, 24, 64, 100):
        cut = model.encode(SENTS, batch_size=8, truncate_dim=d)
        assert cut.shape == (21, min(d, 64)) and np.array_equal(cut, full[:, :d])
    as_tensor = model.encode(SENTS, batch_size=8, truncate_dim=24, convert_to_tensor=True)
    assert as_tensor.is_cuda and np.array_equal(as_tensor.cpu().numpy(), full[:, :24])
    unit = model.encode(SENTS, batch_size=8, truncate_dim=24, normalize_embeddings=True)
    assert unit.shape == (21, 24)
    np.testing.assert_allclose(np.linalg.norm(unit.astype(np.float64), axis=1), 1.0, atol=1e-6)
    want = full[:, :24].astype(np.float64)
    np.testing.assert_allclose(unit, want / np.linalg.norm(want, axis=1, keepdims=True), rtol=1e-5, atol=1e-6)
    # not the prefix of the normalised full rows
    assert not np.allclose(unit, model.encode(SENTS, batch_size=8, normalize_embeddings=True)[:, :24], atol=1e-3)
    tokens = model.encode(SENTS[:3], output_value="token_embeddings", truncate_dim=24)
    assert all(t.shape[1] == 64 for t in tokens)
    assert model.encode([], truncate_dim=24).shape == (0, 24) and model.encode([]).shape == (0, 64)
    assert model.truncate_dim is None


def test_truncate_dim_attribute_context_manager_and_forward(model):
    full = model.encode(SENTS, batch_size=8)
    assert model.get_sentence_embedding_dimension() == 64
    with model.truncate_sentence_embeddings(16):
        assert model.truncate_dim == 16 and model.get_sentence_embedding_dimension() == 16
        assert np.array_equal(model.encode(SENTS, batch_size=8), full[:, :16])
        assert np.array_equal(model.encode(SENTS, batch_size=8, truncate_dim=8), full[:, :8])     # the keyword wins
        with model.truncate_sentence_embeddings(None):
            assert model.encode(SENTS[:2]).shape == (2, 64)
        assert model.truncate_dim == 16
        # forward, and so training, is never truncated
        feats = {k: v.cuda() for k, v in model.tokenize(SENTS[:4]).items()}
        with torch.no_grad():
            assert model(feats)["sentence_embedding"].shape == (4, 64)
    assert model.truncate_dim is None and model.get_sentence_embedding_dimension() == 64
    with pytest.raises(KeyError):
        with model.truncate_sentence_embeddings(8):
            raise KeyError("inside")
    assert model.truncate_dim is None
    with pytest.raises(ValueError):
        with model.truncate_sentence_embeddings(0):
            pass
    assert model.truncate_dim is None


def test_truncate_dim_constructor_keyword(model):
    m = SentenceTransformer("tiny-bert", device="cuda", truncate_dim=12)
    assert m.truncate_dim == 12 and m.get_sentence_embedding_dimension() == 12
    assert np.array_equal(m.encode(SENTS, batch_size=8), model.encode(SENTS, batch_size=8)[:, :12])    # the same seed
    # a Matryoshka loss on a truncated model still sees its full width
    assert S.MatryoshkaLoss(m, S.MultipleNegativesRankingLoss(m), [64, 12]).matryoshka_dims == [64, 12]


def test_an_evaluator_inside_the_context_manager_scores_the_prefix(model):
    s1, s2 = SENTS[:10], SENTS[10:20]
    gold = [float(i % 5) / 4 for i in range(10)]
    ev = evaluation.EmbeddingSimilarityEvaluator(s1, s2, gold, batch_size=4)
    e1, e2 = [torch.from_numpy(model.encode(s, batch_size=4)[:, :16]).double() for s in (s1, s2)]
    full = ev.pair_scores(model)
    with model.truncate_sentence_embeddings(16):
        cut = ev.pair_scores(model)
        score = ev(model)
    np.testing.assert_allclose(cut["cosine"], F.cosine_similarity(e1, e2).numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(cut["dot"], (e1 * e2).sum(1).numpy(), rtol=1e-5, atol=1e-5)
    assert not np.allclose(cut["cosine"], full["cosine"], atol=1e-4)
    assert -1.0 <= score <= 1.0
