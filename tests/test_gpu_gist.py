"""GPU: qst_gist_loss (csrc/gist.hip), GISTEmbedLoss on the fp32 matrix cores with no B x B tensor outside a strip, against the
yardstick of gist_helpers (sentence-transformers' formula in fp64 on the CPU with autograd, guides whose masks are decided):
parity over shapes, strips and temperatures; masks that are exact; the larger tiles and K chunks; the strip invariants;
grad_out; capture; bad arguments.

Tolerances: mnrl_helpers.value_error / grad_error unchanged at temperature 0.05 (they were set for scale 20 and the same
arithmetic), times 5 at temperature 0.01 (the rounding of a logit scales with 1 / temperature)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import gist_helpers as G  # noqa: E402
import mnrl_helpers as M  # noqa: E402
from kernel_helpers import lib, ptr, stream  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import st_losses as S  # noqa: E402


def factor(temperature):
    return 0.05 / temperature if temperature < 0.05 else 1.0


def check(out, grad, loss, ref_grad, D, temperature, what=""):
    """Prints every figure as a share of its tolerance, then asserts."""
    f = factor(temperature)
    ev, eg = M.value_error(out.item(), loss, D) / f, M.grad_error(grad.cpu(), ref_grad) / f
    print(f"  {what}: loss {out.item():.7f} ref {float(loss):.7f}; share of the tolerance (x {f:g}): value {ev:.3f} "
          f"grad_x {eg:.3f}")
    assert torch.isfinite(out).all() and torch.isfinite(grad).all()
    assert ev <= 1.0 and eg <= 1.0
    return ev, eg


# ------------------------------------------------------------------ 1. kernel parity
@pytest.mark.parametrize("temperature", G.TEMPERATURES)
@pytest.mark.parametrize("strip_rows", [64, 128, 0])
@pytest.mark.parametrize("B,K,D,Dg", G.SHAPES)
def test_kernel_matches_reference(lib, B, K, D, Dg, strip_rows, temperature):
    x, g, loss, ref_grad = G.reference(B, K, D, Dg, temperature)
    xd, gd = x.cuda(), g.cuda()
    out, grad = S.gist_loss_raw(xd, gd, K, temperature, "absolute", 0.0, strip_rows, want_grads=True)
    check(out, grad, loss, ref_grad, D, temperature, f"{B}x{K}x{D}x{Dg} T={temperature} strip={strip_rows}")
    fwd, none = S.gist_loss_raw(xd, gd, K, temperature, "absolute", 0.0, strip_rows)     # forward only: the same bits
    assert none is None and torch.equal(fwd, out)


# ------------------------------------------------------------------ 2. masks are exact
@pytest.mark.parametrize("margin_strategy,margin", G.MARGINS)
def test_margins_match_reference(lib, margin_strategy, margin):
    B, K, D, Dg = G.MARGIN_SHAPE
    for temperature in G.TEMPERATURES:
        x, g, loss, ref_grad = G.reference(B, K, D, Dg, temperature, margin_strategy, margin, G.MARGIN_SEED)
        out, grad = S.gist_loss_raw(x.cuda(), g.cuda(), K, temperature, margin_strategy, margin, 64, want_grads=True)
        check(out, grad, loss, ref_grad, D, temperature, f"{margin_strategy} {margin} T={temperature}")


@pytest.mark.parametrize("margin_strategy,margin", G.MARGINS)
def test_masked_entries_have_exactly_zero_probability(lib, margin_strategy, margin):
    """The student's K * B texts are the first K * B unit vectors, so every logit is 0 but aa[i, i] and pp[i, i] (1 / T, masked:
    guide cosine 1), and the gradients spell the softmax out entry by entry: d loss / d a_i at the coordinate of candidate j is
    P_ap[i, j] / (B T) (hard negatives likewise), at the coordinate of anchor j (P_aa[i, j] + P_aa[j, i]) / (B T), and
    d loss / d p_i at the coordinate of positive j (P_pp[i, j] + P_pp[j, i]) / (B T). Wherever the reference masks, that is
    exactly 0.0, elsewhere it is positive; and the loss is the mean of log(#unmasked entries of row i)."""
    B, K, D, Dg = G.MARGIN_SHAPE
    T = 0.05
    assert D >= K * B
    _, guide_cols = G.case(B, K, D, Dg, G.MARGIN_SEED)
    masks, gaps = G.gist_masks([c.double() for c in guide_cols], margin_strategy, margin)
    assert min(float(gp.min()) for gp in gaps) >= G.MIN_GAP
    eye = torch.eye(B, dtype=torch.bool)
    assert bool(masks[1][eye].all()) and bool(masks[2][eye].all())
    x = torch.zeros(K * B, D)
    x[torch.arange(K * B), torch.arange(K * B)] = 1.0
    out, grad = S.gist_loss_raw(x.cuda(), torch.cat(guide_cols, 0).cuda(), K, T, margin_strategy, margin, 64, want_grads=True)
    grad = grad.cpu()
    count = sum((~m).sum(1) for m in masks).double()
    want = count.log().mean().item()
    assert abs(out.item() - want) <= 1e-5 * want, (out.item(), want)
    ga, gp = grad[:B], grad[B:2 * B]
    ap, aa, pp, ans = masks[0], masks[1], masks[2], masks[3:]
    off_target = ~eye
    assert (ga[:, B:2 * B][ap] == 0).all() and (ga[:, B:2 * B][~ap & off_target] > 0).all()
    assert (ga[:, B:2 * B][eye] < 0).all()                              # the target: P - 1
    for k, an in enumerate(ans):
        blk = ga[:, (2 + k) * B:(3 + k) * B]
        assert (blk[an] == 0).all() and (blk[~an] > 0).all()
    both = aa & aa.t()
    assert (ga[:, :B][both & off_target] == 0).all() and (ga[:, :B][~both] > 0).all()
    both = pp & pp.t()
    assert (gp[:, B:2 * B][both & off_target] == 0).all() and (gp[:, B:2 * B][~both] > 0).all()
    assert int(ap.sum()) > 0 and int((aa & aa.t() & off_target).sum()) > 0 and int((pp & pp.t() & off_target).sum()) > 0
    assert all(int(an.sum()) > 0 for an in ans)


def test_the_target_is_kept_by_index(lib):
    """Guide positives equal to their anchors, and one text twice in the batch: the guide's ap[i, i], aa[i, i] and the
    duplicate's entries are all 1 up to rounding, along different roundings. Whatever the comparison says about them, the
    target stays in the softmax and the loss is finite -- also with a margin that puts the bound below the threshold."""
    B, K, D, Dg = 33, 2, 64, 48
    cols = G.student_case(B, K, D, 5)
    gen = torch.Generator().manual_seed(6)
    ga = torch.randn(B, Dg, generator=gen) * (0.5 + 1.5 * torch.rand(B, 1, generator=gen))
    ga[7] = ga[3] * 1.7
    g = torch.cat([ga, ga * 0.3], 0)
    for margin_strategy, margin in G.MARGINS:
        out, grad = S.gist_loss_raw(torch.cat(cols, 0).cuda(), g.cuda(), K, 0.01, margin_strategy, margin, 64, want_grads=True)
        assert torch.isfinite(out).all() and torch.isfinite(grad).all() and grad.abs().max().item() > 0


def test_a_nan_guide_entry_stays_unmasked(lib):
    """A NaN compares false: a row whose threshold is NaN masks nothing, as upstream (the reference gives the same loss)."""
    B, K, D, Dg = 8, 2, 384, 384
    cols, guide_cols = G.case(B, K, D, Dg)
    guide_cols = [c.clone() for c in guide_cols]
    guide_cols[1][5] = float("nan")
    loss = G.gist_ref([c.double() for c in cols], [c.double() for c in guide_cols], 0.05)
    out, _ = S.gist_loss_raw(torch.cat(cols, 0).cuda(), torch.cat(guide_cols, 0).cuda(), K, 0.05, "absolute", 0.0, 64)
    assert math.isfinite(float(loss)) and M.value_error(out.item(), loss, D) <= 1.0


# ------------------------------------------------------------------ 3. larger tiles and K chunks
# (1100, 2, 24, 256): 9 x 18 tiles of 128 x 128 in the anchors' score product; with strip_rows 64 the column side accumulates
# over 18 strips. (128, 3, 256, 256) in strips of 64: two strips. (1400, 3, 24, 256): K * B = 4200 > 4096, so the anchors'
# row-side product is summed from two K chunks.
@pytest.mark.parametrize("B,K,D,Dg,strip_rows", [(1100, 2, 24, 256, 64), (1100, 2, 24, 256, 0), (128, 3, 256, 256, 64),
                                                 (1400, 3, 24, 256, 512)])
def test_large_tiles_and_k_chunks_match_reference(lib, B, K, D, Dg, strip_rows):
    T = 0.05
    x, g, loss, ref_grad = G.reference(B, K, D, Dg, T)
    out, grad = S.gist_loss_raw(x.cuda(), g.cuda(), K, T, "absolute", 0.0, strip_rows, want_grads=True)
    check(out, grad, loss, ref_grad, D, T, f"{B}x{K}x{D}x{Dg} strip={strip_rows}")


# ------------------------------------------------------------------ 4. strips and determinism
@pytest.mark.parametrize("B,K,D,Dg", [(257, 2, 32, 384), (130, 3, 64, 256)])
def test_loss_does_not_depend_on_the_strips(lib, B, K, D, Dg):
    """A row term depends on that row's logits alone and a logit's K order not on the tiling: out_loss is the same bits at
    5, 3, 2 strips and 1. The gradients are summed over the strips and stay within tolerance; two calls give the same bits."""
    T = 0.01
    x, g, loss, ref_grad = G.reference(B, K, D, Dg, T)
    xd, gd = x.cuda(), g.cuda()
    got = {s: S.gist_loss_raw(xd, gd, K, T, "absolute", 0.0, s, want_grads=True) for s in (64, 128, 192, 0)}
    for s, (o, gr) in got.items():
        assert torch.equal(o, got[0][0]), s
        check(o, gr, loss, ref_grad, D, T, f"{B}x{K}x{D}x{Dg} strip={s}")
        o2, gr2 = S.gist_loss_raw(xd, gd, K, T, "absolute", 0.0, s, want_grads=True)
        assert torch.equal(o, o2) and torch.equal(gr, gr2)


# ------------------------------------------------------------------ 5. grad_out, forward only
SHAPE = (33, 4, 768, 384)


def inputs(seed=G.GUIDE_SEED):
    cols, guide_cols = G.case(*SHAPE, seed)
    return torch.cat(cols, 0).cuda(), torch.cat(guide_cols, 0).cuda()


def raw_call(lib, x, g, out, grad_out, gx, B=None, K=SHAPE[1], D=None, Dg=None, temperature=0.05, strategy=0, margin=0.0,
             strip_rows=64, nbytes=None):
    B = x.shape[0] // SHAPE[1] if B is None else B
    D = x.shape[1] if D is None else D
    Dg = g.shape[1] if Dg is None else Dg
    full = lib.qst_gist_workspace_bytes(x.shape[0] // SHAPE[1], SHAPE[1], x.shape[1], g.shape[1], 64)
    ws = torch.empty(full + 16, dtype=torch.uint8, device="cuda")
    return lib.qst_gist_loss(ptr(x), ptr(g), B, K, D, Dg, temperature, strategy, margin, strip_rows, ptr(out), ptr(grad_out),
                             ptr(gx), ptr(ws), full if nbytes is None else nbytes, stream())


def test_grad_out_scales_the_gradients(lib):
    x, g = inputs()
    K, D, T = SHAPE[1], SHAPE[2], 0.05
    _, _, loss, ref_grad = G.reference(*SHAPE, T)
    o1, g1 = S.gist_loss_raw(x, g, K, T, "absolute", 0.0, 64, want_grads=True)
    o2, g2 = S.gist_loss_raw(x, g, K, T, "absolute", 0.0, 64, grad_out=torch.tensor([1.7], device="cuda"), want_grads=True)
    assert torch.equal(o1, o2)
    check(o2, g2 / 1.7, loss, ref_grad, D, T, "grad_out 1.7")
    want = 1.7 * g1.double()
    assert ((g2.double() - want).abs() <= torch.finfo(torch.float32).eps * want.abs().clamp_min(1e-30)).all()


def test_forward_only_never_writes_grad_x(lib):
    x, g = inputs()
    guard = torch.full((x.numel() + 64,), -7.25, device="cuda")
    out = torch.zeros(1, device="cuda")
    assert raw_call(lib, x, g, out, None, None) == 0
    torch.cuda.synchronize()
    assert out.item() > 0 and (guard == -7.25).all()
    gx = guard[:x.numel()].view_as(x)                                   # with gradients: the guard band behind grad_x is intact
    assert raw_call(lib, x, g, out, None, gx) == 0
    torch.cuda.synchronize()
    assert (guard[x.numel():] == -7.25).all() and torch.isfinite(gx).all() and (gx != -7.25).all()


def test_autograd_equals_the_raw_call(lib):
    x, g = inputs()
    K, B = SHAPE[1], SHAPE[0]
    reps = [r.clone().requires_grad_(True) for r in x.chunk(K, 0)]
    loss = S.gist_embed_loss(reps, list(g.chunk(K, 0)), 0.05, "relative", 0.1, strip_rows=64)
    assert loss.dim() == 0
    (loss * 1.7).backward()
    out, grad = S.gist_loss_raw(x, g, K, 0.05, "relative", 0.1, 64, grad_out=torch.tensor([1.7], device="cuda"), want_grads=True)
    assert torch.equal(loss.detach().reshape(1), out)
    assert all(torch.equal(r.grad, grad[j * B:(j + 1) * B]) for j, r in enumerate(reps))


# ------------------------------------------------------------------ 6. capture
def test_the_call_is_capturable_in_a_graph(lib):
    """No host synchronisation, grad_out read on the device: a captured call (one branch) replays on new inputs and a new
    upstream gradient written into the same buffers, to the bits of a plain call."""
    (x1, g1), (x2, g2) = inputs(), inputs(G.MARGIN_SEED)
    K = SHAPE[1]
    x, g, w = x1.clone(), g1.clone(), torch.tensor([1.0], device="cuda")
    S.gist_loss_raw(x, g, K, 0.05, "absolute", 0.0, 64, grad_out=w, want_grads=True)     # code objects loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, grad = S.gist_loss_raw(x, g, K, 0.05, "absolute", 0.0, 64, grad_out=w, want_grads=True)
    x.copy_(x2 * 1.01), g.copy_(g2), w.fill_(2.5)
    graph.replay()
    torch.cuda.synchronize()
    want, want_g = S.gist_loss_raw(x2 * 1.01, g2, K, 0.05, "absolute", 0.0, 64, grad_out=torch.tensor([2.5], device="cuda"),
                                   want_grads=True)
    assert torch.equal(out, want) and torch.equal(grad, want_g)


# ------------------------------------------------------------------ 7. bad arguments
def test_bad_arguments_are_refused_with_nothing_written(lib):
    x, g = inputs()
    out = torch.full((1,), -7.25, device="cuda")
    gx = torch.full_like(x, -7.25)
    nan, inf = float("nan"), float("inf")
    full = lib.qst_gist_workspace_bytes(SHAPE[0], SHAPE[1], SHAPE[2], SHAPE[3], 64)
    bad = [dict(B=0), dict(K=1), dict(D=0), dict(Dg=0), dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=nan),
           dict(temperature=inf), dict(margin=nan), dict(margin=inf), dict(margin=-inf), dict(strategy=2), dict(strategy=-1),
           dict(strip_rows=-64), dict(strip_rows=32), dict(strip_rows=100), dict(nbytes=full - 1), dict(nbytes=0)]
    for kw in bad:
        assert raw_call(lib, x, g, out, None, gx, **kw) == -1, kw
    B, K, D, Dg = SHAPE
    ws = torch.empty(full + 16, dtype=torch.uint8, device="cuda")

    def call(xp, gp, op, wp):
        return lib.qst_gist_loss(xp, gp, B, K, D, Dg, 0.05, 0, 0.0, 64, op, None, ptr(gx), wp, full, stream())

    assert call(None, ptr(g), ptr(out), ptr(ws)) == -1 and call(ptr(x), None, ptr(out), ptr(ws)) == -1
    assert call(ptr(x), ptr(g), None, ptr(ws)) == -1 and call(ptr(x), ptr(g), ptr(out), None) == -1
    assert call(ptr(x), ptr(g), ptr(out), ptr(ws) + 2) == -1               # a misaligned workspace
    torch.cuda.synchronize()
    assert out.item() == -7.25 and (gx == -7.25).all()
    assert raw_call(lib, x, g, out, None, gx) == 0                          # and the same call without a fault runs
    torch.cuda.synchronize()
    assert out.item() > 0
