"""The yardsticks of tests/test_gpu_attention_masks.py judged on the CPU, before any kernel is involved: the mask families and
the poisoned padding are what they claim, the reference with the kernels' rounding points emulated (attn_ref_rounded) lies
inside every bound, the constants of the backward bounds are the ones that reference gives, and references that are wrong the
way a kernel could be wrong -- one leaked padding key, the position bias one entry off, the mask one key off, the dropout mask
of another site -- lie outside."""
import functools
import math

import pytest
import torch

import attention_mask_cases as M
from oracle import dropout_ref as D

OPS = ["bf16", "f16"]
HOST_CASES = sorted({(name, drop) for name, _, drop in M.RUNS})


@functools.lru_cache(maxsize=None)
def case_data(name, op, drop):
    case = M.BY_NAME[name]
    inp = M.make_case(case, op, drop)
    return case, inp, M.exact(inp, case), M.attn_ref_rounded(op, inp, case)


def pow2_ceil(x):
    return 2.0 ** math.ceil(math.log2(x))


def block_excess(op, case, inp, ex, dqkv, k=M.K_BLOCK):
    """largest ||got - ref|| / (k eps ||ref|| + floor) over the blocks (0 / 0 counts as inside)"""
    dims = (case.n, case.L, case.A, case.d)
    err = M.block_norms(dqkv - ex.dqkv, *dims)
    bound = k * M.EPS[op] * M.block_norms(ex.dqkv, *dims) + M.bwd_floor(op, inp, case, ex)
    return float(torch.where(err > 0, err / bound, torch.zeros_like(err)).max())


def drel_excess(op, case, inp, ex, drel, k=M.K_DREL):
    err = (drel - ex.drel).flatten(1).norm(dim=-1)
    bound = k * M.EPS[op] * ex.drel.flatten(1).norm(dim=-1) + M.drel_floor(op, inp, case, ex)
    return float(torch.where(err > 0, err / bound, torch.zeros_like(err)).max())


# ------------------------------------------------------------------ the inputs are what they claim
@pytest.mark.parametrize("L", [32, 64, 96, 128, 160, 288, 416, 512])
def test_mask_families(L):
    m = M.mask_families(8, L)
    fam = dict(zip(M.FAMILIES, m))
    assert m.dtype == torch.int64 and m.shape == (8, L)
    assert fam["a"].sum() == L and fam["b"].sum() == L - 5 and fam["f"].sum() == 1 and fam["f"][L - 1] == 1
    assert fam["g"].sum() == 0
    for f in "abcdefh":
        assert fam[f].sum() > 0
    assert fam["c"][0] == 0 and fam["d"][0] == 0 and fam["c"][L - 1] == 1 and fam["d"][L - 1] == 1
    assert (fam["e"][2::3] == 0).all() and fam["e"][0] == 1
    if L >= 64:
        assert fam["c"][:40].sum() == 0 and fam["c"][40] == 1              # a whole dead tile + 8 keys
        assert fam["d"][:32].sum() == 0 and fam["d"][32] == 1              # exactly one dead tile
        assert fam["e"][32:64].sum() == 0                                  # interior dead tile ...
    if L >= 96:
        assert fam["e"][:32].sum() > 0 and fam["e"][64:].sum() > 0         # ... with valid keys on both sides
    if L > 128:
        first = ((L - 1) // 128) * 128
        assert fam["h"][:first].sum() == 0 and fam["h"][first:].sum() == L - first
    assert torch.equal(M.mask_families(19, L)[8:16], m)                    # the families cycle


def test_poison_is_exact_in_both_operand_types_and_invisible_to_the_reference():
    case = M.BY_NAME["c5_L160_pair32"]
    n, L, A, d = case.n, case.L, case.A, case.d
    H = A * d
    g = torch.Generator().manual_seed(5)
    mask = M.mask_families(n, L)
    clean = torch.randn(n * L, 3 * H, generator=g).to(torch.bfloat16).float()
    dirty = M.poison_padding(clean, mask, H, g)
    pad = ((mask == 0) & (mask.sum(1, keepdim=True) > 0)).view(-1)
    assert torch.equal(dirty[:, :H], clean[:, :H])                                       # Q rows stay
    assert torch.equal(dirty[~pad], clean[~pad])                                         # valid keys and the all-padding sequence stay
    assert torch.equal(dirty[pad][:, H:2 * H], clean[pad][:, H:2 * H] * 8)
    assert bool((dirty[pad][:, 2 * H:].abs() == 1000).all()) and dirty[pad][:, 2 * H:].sum().abs() < 1000 * pad.sum() * H * 0.2
    for dt in M.DT.values():
        assert torch.equal(dirty.to(dt).float(), dirty)
    rel = 0.5 * torch.randn(A, L, L, generator=g, dtype=torch.float64)
    for pm in (None, torch.from_numpy(D.multipliers8(1, 2, 3, n * A * L * L, 0.1).reshape(n, A, L, L)).double()):
        assert torch.equal(M.attn_ref(dirty.double(), mask, rel, n, L, A, d, pm), M.attn_ref(clean.double(), mask, rel, n, L, A, d, pm))
    assert torch.equal(M.lse_ref(dirty.double(), mask, rel, n, L, A, d), M.lse_ref(clean.double(), mask, rel, n, L, A, d))
    # the all-padding sequence attends uniformly: its context is the mean of its V rows
    r = M.FAMILIES.index("g")
    ctx = M.attn_ref(dirty.double(), mask, rel, n, L, A, d).view(n, L, H)[r]
    want = dirty.double().view(n, L, 3 * H)[r, :, 2 * H:].mean(0)
    torch.testing.assert_close(ctx, want[None].expand(L, H), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ the rounded reference is inside every bound
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name,drop", HOST_CASES)
def test_rounded_reference_is_inside_the_bounds(name, drop, op):
    case, inp, ex, (ctx, dqkv, drel) = case_data(name, op, drop)
    f = float(((ctx - ex.ctx).abs() / M.fwd_bound(op, ex)).max())
    b = block_excess(op, case, inp, ex, dqkv)
    r = drel_excess(op, case, inp, ex, drel) if case.bias else 0.0
    print(f"{name} {op} drop={drop}: forward {f:.3f}, backward blocks {b:.3f}, drel {r:.3f} of the bound")
    assert f < 1.0 and b < 1.0 and r < 1.0
    # ... and the rows the reference makes exactly zero stay exactly zero under rounding
    n, L, A, d = case.n, case.L, case.A, case.d
    dead = ((inp.mask == 0) & (inp.mask.sum(1, keepdim=True) > 0)).view(-1)
    assert float(ex.dqkv[dead][:, A * d:].abs().max()) == 0.0 and float(dqkv[dead][:, A * d:].abs().max()) == 0.0
    allpad = (inp.mask.sum(1) == 0).repeat_interleave(L)
    assert float(ex.dqkv[allpad].abs().max()) == 0.0 and float(dqkv[allpad].abs().max()) == 0.0
    if case.bias:
        assert float(ex.drel[:, 0].abs().max()) == 0.0 and float(drel[:, 0].abs().max()) == 0.0


def test_backward_constants_come_from_the_rounded_reference():
    """K_BLOCK and K_DREL are three times the largest ratio ||rounded - exact|| / (eps ||exact||) over every backward case and
    both operand types, rounded up to a power of two; the floor is not subtracted, so k alone carries the rounding of a dense
    block. Blocks whose exact gradient is 0 (the one-key family: P = 1, dS = 0) have no ratio: under dropout the rounded
    reference is NOT zero there (O = v * 256 / 230 is rounded, so delta no longer cancels dP), and the floor alone bounds it."""
    kb = kr = 0.0
    for op in OPS:
        for name, drop in HOST_CASES:
            case, inp, ex, (_, dqkv, drel) = case_data(name, op, drop)
            dims = (case.n, case.L, case.A, case.d)
            err, ref = M.block_norms(dqkv - ex.dqkv, *dims), M.block_norms(ex.dqkv, *dims)
            kb = max(kb, float((err[ref > 0] / (M.EPS[op] * ref[ref > 0])).max()))
            if case.bias:
                err, ref = (drel - ex.drel).flatten(1).norm(dim=-1), ex.drel.flatten(1).norm(dim=-1)
                kr = max(kr, float((err / (M.EPS[op] * ref)).max()))
    print(f"largest ratio: blocks {kb:.3f} -> k = {pow2_ceil(3 * kb)}; drel {kr:.3f} -> k = {pow2_ceil(3 * kr)}")
    assert M.K_BLOCK == pow2_ceil(3 * kb) and M.K_DREL == pow2_ceil(3 * kr)


# ------------------------------------------------------------------ mutants are outside
def violations(op, case, inp, ex, mut):
    """(forward, backward blocks, drel) of a wrong reference, each as a multiple of its bound"""
    f = float(((mut.ctx - ex.ctx).abs() / M.fwd_bound(op, ex)).max())
    b = block_excess(op, case, inp, ex, mut.dqkv)
    r = drel_excess(op, case, inp, ex, mut.drel) if case.bias else None
    return f, b, r


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", ["c1_L32_fused", "c5_L160_pair32", "c7_L288_one64_nc3"])
def test_one_leaked_padding_key_is_far_outside(name, op):
    case, inp, ex, _ = case_data(name, op, False)
    leaky = inp.mask.clone()
    r = M.FAMILIES.index("b")
    leaky[r, case.L - 1] = 1                                  # one padding key of one sequence next to L - 5 valid ones
    f, b, _ = violations(op, case, inp, ex, M.exact(inp, case, mask=leaky))
    print(f"{name} {op}: one leaked key: forward {f:.3g}, backward {b:.3g} times the bound")
    assert f > 1000 and b > 1000


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", ["c2_L128_fused_remap", "c5_L160_pair32", "c7_L288_one64_nc3", "c9_L416_pair64_bias"])
def test_bias_off_by_one_entry_and_mask_off_by_one_key_are_outside(name, op):
    case, inp, ex, _ = case_data(name, op, False)
    f, b, r = violations(op, case, inp, ex, M.exact(inp, case, rel_shift=1))
    print(f"{name} {op}: bias at j - i + L + 1: forward {f:.3g}, backward {b:.3g}, drel {r:.3g} times the bound")
    assert f > 1 and b > 1 and r > 1
    f, b, r = violations(op, case, inp, ex, M.exact(inp, case, mask=torch.roll(inp.mask, 1, dims=1)))
    print(f"{name} {op}: mask shifted by one key: forward {f:.3g}, backward {b:.3g}, drel {r:.3g} times the bound")
    assert f > 1 and b > 1 and r > 1


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", sorted({name for name, _ in M.DROPPED}))
def test_dropout_mask_of_another_site_is_outside(name, op):
    case, inp, ex, _ = case_data(name, op, True)
    n, L, A = case.n, case.L, case.A
    other = torch.from_numpy(D.multipliers8(M.DROP_SEED, M.DROP_STEP, D.site_probs(M.DROP_LAYER + 1), n * A * L * L, M.DROP_P)
                             .reshape(n, A, L, L))
    f, b, r = violations(op, case, inp, ex, M.exact(inp, case, pm=other))
    print(f"{name} {op}: dropout mask of the next layer's site: forward {f:.3g}, backward {b:.3g}, drel {r:.3g} times the bound")
    assert f > 1 and b > 1 and (r is None or r > 1)
