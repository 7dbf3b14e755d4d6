"""GPU: the six loss entry points that share csrc/row_loss.h's choice of a kernel form, on both sides of every edge between
two forms.

B = 5 is one full workgroup of four rows plus one row. D = 4, 252, 256 (one float4 per lane, the last lanes idle / all busy),
260, 1024 (two and four float4), 1028 (eight), 2048 (the last D kept in registers), 2050 (element by element), 2052 (past
the registers: the distillation kernels stream 16 bytes a lane, the others go element by element). Each D with every tensor
aligned and with one input viewed one float into its storage, which sends the launch to the element-by-element form.

Value and gradients against the fp64 yardsticks, at the tolerances of the entry points' own tests (the helpers', not restated).
No existing parametrisation has a point at B = 5 with one of these D, so none is left out.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import distill_helpers as DH  # noqa: E402
import tuple_loss_helpers as H  # noqa: E402
from kernel_helpers import lib  # noqa: E402,F401
from oracle import torch_ref as R  # noqa: E402
from quadruplet_sentence_transformer_amd import st_losses as S  # noqa: E402
from quadruplet_sentence_transformer_amd.encoder import quadruplet_loss_raw  # noqa: E402

B = 5
DS = [4, 252, 256, 260, 1024, 1028, 2048, 2050, 2052]
RED = H.RED
form = pytest.mark.parametrize("D,offset", [(D, o) for D in DS for o in (False, True)],
                               ids=lambda x: ("offset" if x else "aligned") if isinstance(x, bool) else str(x))


def place(xs, D, offset):
    """The inputs on the device; with `offset`, one of them (which one turns with D) one float into a storage of its own."""
    out = [t.cuda().contiguous() for t in xs]
    if offset:
        k = DS.index(D) % len(xs)
        flat = torch.empty(xs[k].numel() + 1, device="cuda")
        flat[1:].copy_(xs[k].reshape(-1))
        out[k] = flat[1:].view(xs[k].shape)
        assert out[k].data_ptr() % 16 == 4 and out[k].is_contiguous()
    return out


def quad_hinges(a, p, q, n, norm, swap):
    """The three hinge arguments of the gamma-quadruplet loss per row (margins 1.0, 0.5, 0.5), fp64."""
    d = lambda x, y: F.pairwise_distance(x, y, p=norm)  # noqa: E731
    neg = lambda direct, other: torch.minimum(direct, other) if swap else direct  # noqa: E731
    return torch.stack([1.0 + d(a, p) - neg(d(a, n), d(p, n)), 0.5 + d(a, q) - neg(d(a, n), d(q, n)),
                        0.5 + d(a, p) - neg(d(a, q), d(p, q))])


@form
@pytest.mark.parametrize("p", [2.0, 1.0, 3.0])
@pytest.mark.parametrize("swap", [False, True])
def test_quadruplet_loss(lib, D, offset, p, swap):
    x = H.rows(B, D, 4, B * 1000 + D)
    metric = H.L2 if p == 2.0 else H.L1             # H.value_tol: the tolerance of test_loss_matches_oracle, by the norm
    tol = H.value_tol(metric, D)
    # a condition on the test data: no hinge closer to its kink than five times the error accepted on a distance
    assert quad_hinges(*[t.double() for t in x], p, swap).abs().min() >= 5 * tol
    kw = dict(gamma=0.6, margin_pos_neg=1.0, margin_pos_part=0.5, margin_part_neg=0.5, p=p, swap=swap)
    xd = place(x, D, offset)
    for red_name, red in RED:
        xs = H.f64(x)
        ref = R.gamma_quadruplet_loss_ref(*xs, reduction=red_name, **kw)
        w = H.upstream(B, red)
        (ref * w.double()).sum().backward()
        out, grads = quadruplet_loss_raw(*xd, 0.6, 1.0, 0.5, 0.5, p, swap, red, grad_out=H.dev(w), want_grads=True)
        H.check_value(out, ref, metric, B, D, red)
        H.check_grads(grads, xs)


@form
@pytest.mark.parametrize("metric", sorted(H.METRIC_NAMES), ids=lambda m: H.METRIC_NAMES[m])
def test_pair_metric(lib, D, offset, metric):
    u, v = H.rows(B, D, 2, B * 1000 + D)
    xs = H.f64((u, v))
    ref = H.metric_ref(*xs, metric)
    w = H.upstream(B, 0)
    (ref * w.double()).sum().backward()
    out, grads = S.pair_metric_raw(*place((u, v), D, offset), metric, grad_out=H.dev(w), want_grads=True)
    if metric == H.DOT:
        assert ((out.cpu().double() - ref.detach()).abs() <= DH.dot_bound(u, v)).all()
    else:
        H.check_value(out, ref, metric, B, D, 0)
    H.check_grads(grads, xs)


@form
@pytest.mark.parametrize("kind,metric", [(H.MSE, H.COS_SIM)] + [(H.CONTRASTIVE, m) for m in H.DISTANCES], ids=lambda x: None)
def test_pair_loss(lib, D, offset, kind, metric):
    u, v = H.rows(B, D, 2, B * 1000 + D + 1)
    y = H.pair_labels(B, kind, B + D)
    margin = H.margin_between(H.metric_ref(u.double(), v.double(), metric), metric, D) if kind == H.CONTRASTIVE else 0.0
    ud, vd = place((u, v), D, offset)
    for red_name, red in RED:
        xs = H.f64((u, v))
        ref = H.mse_ref(*xs, y, red_name) if kind == H.MSE else H.contrastive_ref(*xs, y, metric, margin, red_name)
        w = H.upstream(B, red)
        (ref * w.double()).sum().backward()
        out, grads = S.pair_loss_raw(ud, vd, H.dev(y), kind, metric, margin, red, grad_out=H.dev(w), want_grads=True)
        H.check_value(out, ref, metric, B, D, red)
        H.check_grads(grads, xs)


@form
@pytest.mark.parametrize("metric", H.DISTANCES, ids=lambda m: H.METRIC_NAMES[m])
def test_triplet_loss(lib, D, offset, metric):
    a, p, n = H.rows(B, D, 3, B * 1000 + D + 2)
    dap, dan = H.metric_ref(a.double(), p.double(), metric), H.metric_ref(a.double(), n.double(), metric)
    margin = H.margin_between(dan - dap, metric, D)
    xd = place((a, p, n), D, offset)
    for red_name, red in RED:
        xs = H.f64((a, p, n))
        ref = H.triplet_ref(*xs, metric, margin, red_name)
        w = H.upstream(B, red)
        (ref * w.double()).sum().backward()
        out, grads = S.triplet_loss_raw(*xd, metric, margin, red, grad_out=H.dev(w), want_grads=True)
        H.check_value(out, ref, metric, B, D, red)
        H.check_grads(grads, xs)


@form
def test_embed_mse(lib, D, offset):
    x, t = H.rows(B, D, 2, B * 1000 + D + 3)
    xd, td = place((x, t), D, offset)
    for w in (None, torch.tensor([1.7])):
        (xs,) = H.f64((x,))
        ref = DH.embed_mse_ref(xs, t.double())
        (ref * (1.0 if w is None else w.double())).sum().backward()
        out, grad = S.embed_mse_raw(xd, td, grad_out=None if w is None else H.dev(w), want_grads=True)
        assert abs(out.cpu().double().item() - ref.item()) <= DH.mse_rel_bound(D) * ref.item()
        H.check_grads([grad], [xs])


@form
@pytest.mark.parametrize("sim", DH.SIMS, ids=lambda m: H.METRIC_NAMES[m])
def test_margin_mse(lib, D, offset, sim):
    q, p, n = H.rows(B, D, 3, B * 1000 + D + 4)
    y = DH.margin_labels(q, p, n, sim, B + D)
    dm, drow = DH.margin_bounds(q, p, n, y, sim)
    m_ref = DH.margin_ref(q.double(), p.double(), n.double(), sim)
    xd = place((q, p, n), D, offset)
    for red_name, red in RED:
        xs = H.f64((q, p, n))
        ref = DH.margin_mse_ref(*xs, y, sim, red_name)
        w = H.upstream(B, red)
        (ref * w.double()).sum().backward()
        out, grads, margin = S.margin_mse_raw(*xd, H.dev(y), sim, red, grad_out=H.dev(w), want_grads=True, want_margin=True)
        err = (out.cpu().double().view(ref.shape) - ref.detach()).abs()
        assert (err <= DH.reduced_bound(drow, ref, red)).all() and ((margin.cpu().double() - m_ref).abs() <= dm).all()
        H.check_grads(grads, xs)
