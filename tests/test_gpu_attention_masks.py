"""The attention kernels (csrc/attention.hip, csrc/x3.hip, csrc/x3_bwd.hip) at the masks a prefix `arange(L) < len` never
makes -- left padding, a dead leading or interior 32-key tile, holes, one key, no key -- with the padding keys poisoned
(tests/attention_mask_cases.py), so that any weight on a masked key is an error of 10^5 bounds, not of a rounding; at the shapes
that reach each backward kernel and launch branch (the forward's workgroup-id remap, the persistent loop's second item, the
three NC instantiations of the one-workgroup d = 64 kernel, the d = 64 pair with the position bias); against fp64 with bounds
that follow from the kernels' rounding points (tests/test_attention_masks_host.py shows a reference with those roundings is
inside them and wrong references are outside): per element for ctx, against lse_ref for lse, per (sequence, head, part) for
dqkv, per head for drel.

The all-padding sequence: forward = the uniform mean of V (HF's result); backward defined for dctx = 0 only (what an encoder
feeds it: its pooled embedding and gradient are 0), where every dqkv row is exactly 0; with another dctx only finiteness is
asked (include/qst_kernels.h at qst_attention_bwd)."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import _lib  # noqa: E402
from oracle import dropout_ref as D  # noqa: E402
import attention_mask_cases as M  # noqa: E402
from kernel_helpers import OPDT, attn_desc, drop_desc, drop_state, kf, lib, op, ptr, stream  # noqa: E402,F401
from test_gpu_parity_kernels import check_attn_grads  # noqa: E402


@functools.lru_cache(maxsize=None)
def reference(name, op, drop):
    """inputs and fp64 results of a case: computed once, shared by the runs of its backward paths, never written to"""
    case = M.BY_NAME[name]
    inp = M.make_case(case, op, drop)
    return case, inp, M.exact(inp, case)


def lse_bound(inp, case):
    """[n, A, L]: 2^-18 (max_j sum_k |q_ik k_jk| scale + max |bias| + 1) over the valid keys j. Scores are exact 16-bit products
    accumulated in fp32 over d <= 64 terms (64 * 2^-24 = 2^-18); the + 1 covers the hardware exp2 / log2."""
    n, L, A, d = case.n, case.L, case.A, case.d
    H = A * d
    q, k, _ = [M.heads(t, n, L, A, d) for t in inp.qkv.double().split(H, dim=-1)]
    s = (q.abs() @ k.abs().transpose(-1, -2)) / math.sqrt(d) * inp.mask[:, None, None, :]
    bias = float(inp.relpos.abs().max()) if inp.relpos is not None else 0.0
    return 2.0 ** -18 * (s.max(-1).values + bias + 1)


def masked_rows(mask):
    """(padding keys of the sequences that have a valid key, rows of the all-padding sequences), flat [n * L] booleans"""
    L = mask.shape[1]
    has = mask.sum(1, keepdim=True) > 0
    return ((mask == 0) & has).view(-1), (~has).expand(-1, L).reshape(-1)


def worst(err, bound):
    """largest err / bound (0 / 0 = inside)"""
    return float(torch.where(err > 0, err / bound, torch.zeros_like(err)).max())


@pytest.mark.parametrize("name,force_split,drop", M.RUNS,
                         ids=[f"{name}{'-split' if fs else ''}{'-drop' if dr else ''}" for name, fs, dr in M.RUNS])
def test_attention_on_irregular_masks(lib, op, name, force_split, drop):
    case, inp, ex = reference(name, op, drop)
    n, L, A, d = case.n, case.L, case.A, case.d
    H, dt, eps = A * d, OPDT[op], M.EPS[op]
    dead, allpad = masked_rows(inp.mask)
    has = inp.mask.sum(1) > 0

    qd, md, dcd = inp.qkv.to(dt).cuda(), inp.mask.cuda(), inp.dctx.to(dt).cuda()
    reld = inp.relpos.cuda() if case.bias else None
    ctx = torch.full((n * L, H), float("nan"), dtype=dt, device="cuda")
    lse = torch.full((n, A, L), float("nan"), device="cuda")
    st = drop_state(lib, M.DROP_SEED, M.DROP_STEP)                      # (stays referenced until the last launch)
    dsc = drop_desc(st, D.site_probs(M.DROP_LAYER), M.DROP_P) if drop else _lib.QstDrop()
    q = attn_desc(qkv=qd, mask=md, rel_pos=reld, nseq=n, L=L, A=A, d=d, ctx=ctx, lse=lse, drop=dsc)
    _lib.check(kf(lib, "qst_attention_fwd_ex", op)(q, stream()))
    got, got_lse = ctx.float().cpu().double(), lse.cpu().double()

    # ---- forward: every row of every sequence, padded queries and the all-padding sequence included
    f = worst((got - ex.ctx).abs(), M.fwd_bound(op, ex))
    le = worst((got_lse - ex.lse).abs()[has], lse_bound(inp, case)[has])
    print(f"{name} {op}: ctx {f:.3f} of the bound, lse {le:.3f} of the bound")
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(got_lse).all())
    assert f <= 1.0, f"ctx is {f:.3g} times the forward bound away from fp64"
    assert le <= 1.0, f"lse is {le:.3g} times its bound away from the fp64 logsumexp"

    # ---- backward on the chosen path; dctx = 0 on the all-padding sequence
    def backward(dctx_dev):
        dq = torch.full((n * L, 3 * H), float("nan"), dtype=dt, device="cuda")
        drel = torch.zeros(A, 2 * L, device="cuda") if case.bias else None
        delta = torch.empty(n, A, L, device="cuda")
        q.dctx, q.dqkv, q.drel, q.delta_scratch = dctx_dev.data_ptr(), dq.data_ptr(), ptr(drel), delta.data_ptr()
        q.force_split = force_split
        _lib.check(kf(lib, "qst_attention_bwd_ex", op)(q, stream()))
        torch.cuda.synchronize()
        return dq.float().cpu().double(), (drel.cpu().double() if case.bias else None)

    dq, drel = backward(dcd)
    dims = (n, L, A, d)
    b = worst(M.block_norms(dq - ex.dqkv, *dims),
              M.K_BLOCK * eps * M.block_norms(ex.dqkv, *dims) + M.bwd_floor(op, inp, case, ex))
    r = 0.0
    if case.bias:
        r = worst((drel - ex.drel).norm(dim=-1), M.K_DREL * eps * ex.drel.norm(dim=-1) + M.drel_floor(op, inp, case, ex))
    print(f"{name} {op} force_split={force_split}: dqkv blocks {b:.3f} of the bound, drel {r:.3f} of the bound")
    assert bool(torch.isfinite(dq).all())
    assert b <= 1.0, f"a (sequence, head, part) block of dqkv is {b:.3g} times its bound away from fp64 autograd"
    assert float(dq[dead][:, H:].abs().max()) == 0.0, "dK / dV of a masked key is not exactly 0"
    assert float(dq[allpad].abs().max()) == 0.0, "the all-padding sequence with dctx = 0 has a non-zero gradient"
    if case.bias:
        assert bool(torch.isfinite(drel).all())
        assert r <= 1.0, f"drel of a head is {r:.3g} times its bound away from fp64 autograd"
        assert float(drel[:, 0].abs().max()) == 0.0, "drel entry 0 (unused) was written"

    # ---- the all-padding sequence with a gradient of its own: finite, nothing more
    g = torch.Generator().manual_seed(7)
    loud = torch.where(allpad[:, None], torch.randn(n * L, H, generator=g), inp.dctx).to(dt).cuda()
    dq2, drel2 = backward(loud)
    assert bool(torch.isfinite(dq2).all()) and (drel2 is None or bool(torch.isfinite(drel2).all()))
    assert torch.equal(dq2[~allpad], dq[~allpad])                       # ... and it is nobody else's business


@pytest.mark.parametrize("L,d,bias", M.PARITY)
def test_parity_attention_on_irregular_masks(lib, L, d, bias):
    """qst_attention_fwd_x3_drop, qst_attention_bwd_f32_drop and qst_attention_bwd_x3 without dropout, full [A, L, L] bias,
    poisoned padding, against fp64 at the tolerances of tests/test_gpu_parity_kernels.py
    (test_attention_x3_forward_and_fp32_backward_match_fp64 for ctx, check_attn_grads for the gradients)."""
    case = M.Case("parity", 8, L, 2, d, bias)
    n, A, H = case.n, case.A, case.A * d
    inp = M.make_case(case, None, full_bias=True)
    ex = M.exact(inp, case)
    dead, allpad = masked_rows(inp.mask)
    qd, md, dcd = inp.qkv.cuda(), inp.mask.cuda(), inp.dctx.cuda()
    reld = inp.relpos.cuda() if bias else None
    ctx = torch.full((n * L, H), float("nan"), device="cuda")
    _lib.check(lib.qst_attention_fwd_x3_drop(qd.data_ptr(), md.data_ptr(), ptr(reld), n, L, A, d, ctx.data_ptr(), None, stream()))
    torch.testing.assert_close(ctx.cpu().double(), ex.ctx, rtol=1e-4, atol=2e-5 * max(1.0, ex.ctx.abs().max().item()))

    def backward(which, dctx_dev):
        dq = torch.full((n * L, 3 * H), float("nan"), device="cuda")
        drel = torch.zeros(A, L, L, device="cuda") if bias else None
        if which == "f32":
            _lib.check(lib.qst_attention_bwd_f32_drop(qd.data_ptr(), ctx.data_ptr(), dctx_dev.data_ptr(), md.data_ptr(), ptr(reld),
                                                      n, L, A, d, dq.data_ptr(), ptr(drel), None, stream()))
        else:
            scratch = torch.empty(lib.qst_attention_bwd_x3_scratch_bytes(n, L, A) // 4, device="cuda")
            _lib.check(lib.qst_attention_bwd_x3(qd.data_ptr(), ctx.data_ptr(), dctx_dev.data_ptr(), md.data_ptr(), ptr(reld),
                                                n, L, A, d, dq.data_ptr(), ptr(drel), scratch.data_ptr(), None, stream()))
        torch.cuda.synchronize()
        return dq.cpu(), (drel.cpu() if bias else None)

    g = torch.Generator().manual_seed(7)
    loud = torch.where(allpad[:, None], torch.randn(n * L, H, generator=g), inp.dctx).cuda()
    for which in ("f32", "x3"):
        dq, drel = backward(which, dcd)
        check_attn_grads(dq, drel, ex.dqkv, ex.drel)
        assert float(dq[dead][:, H:].abs().max()) == 0.0, f"{which}: dK / dV of a masked key is not exactly 0"
        assert float(dq[allpad].abs().max()) == 0.0, f"{which}: the all-padding sequence with dctx = 0 has a non-zero gradient"
        dq2, drel2 = backward(which, loud)
        assert bool(torch.isfinite(dq2).all()) and (drel2 is None or bool(torch.isfinite(drel2).all()))
        assert torch.equal(dq2[~allpad], dq[~allpad])
