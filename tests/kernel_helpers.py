"""What the GPU test files (tests/test_gpu_*.py) share, once each; imported like cross_encoder_fixtures, not a conftest.

  * plumbing: the `lib` and `op` fixtures (`from kernel_helpers import lib, op  # noqa: F401`), stream / ptr, the operand
    types (OPDT, opr, kf) and the ctypes argument structs filled from keywords (gemm_args, ln_epi, ffn_args, attn_desc);
  * references and layouts more than one file compares against: attn_ref (re-exported from attention_mask_cases, which the
    host test imports without the library), the dropout state / descriptor, the MX scale layout (stage_major, row_major) and
    the MXFP8 quantisation of an operand on the device (quant_dev), the real-valued top-k cases with their fp64 yardstick (real_rows, real_case) and the
    streaming top-k call both top-k files compare with (new_topk_state, topk_stream_call);
  * the encoder harness: quad_batch and run_step, one training forward + quadruplet loss + backward of a fresh HipEncoder.

The rule: a helper lives in the test file that uses it; its second user moves it here instead of copying it. What a test
asserts stays in its own file. tests/test_kernel_coverage_host.py reads the test files, not this module: an entry point is
called by name (`lib.NAME`, `kf(lib, "NAME", op)`) from a test, never only from here.
"""
import functools

import pytest
import torch

import topk_stream_cases as T
from attention_mask_cases import attn_ref  # noqa: F401  (moved there with its second user, the host test: re-exported)
from oracle import dropout_ref as D
from quadruplet_sentence_transformer_amd import _lib
from quadruplet_sentence_transformer_amd.encoder import HipEncoder, quadruplet_loss_raw, stacked


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


# The kernels with 16-bit matrix-core operands exist on bf16 (qst_*) and on IEEE half (qst_*_f16: QST_PREC_F16, the same
# sources compiled on the other operand type); their tests run on both.
OPDT = {"bf16": torch.bfloat16, "f16": torch.float16}


@pytest.fixture(params=["bf16", "f16"])
def op(request):
    return request.param


def stream():
    return _lib.current_stream_ptr()


ptr = _lib.ptr                       # data_ptr of a tensor, None for None


def kf(lib, name, op):
    return _lib.kfn(lib, name, op)


def opr(op, t):
    """t rounded to the operand type and back (what the kernel's operand holds)."""
    return t.to(OPDT[op]).to(torch.float32)


# ------------------------------------------------------------------ argument structs
def filled(struct, **kw):
    """struct() with its fields set from keywords; a tensor gives its data pointer and stays referenced by the struct, so the
    device memory lives until the launch that takes the struct is enqueued."""
    s = struct()
    s._keep = [v for v in kw.values() if torch.is_tensor(v)]
    for k, v in kw.items():
        setattr(s, k, v.data_ptr() if torch.is_tensor(v) else v)
    return s


def gemm_args(**kw):
    return filled(_lib.QstGemmArgs, **kw)


def ln_epi(**kw):
    return filled(_lib.QstLnEpi, **kw)


def ffn_args(**kw):
    return filled(_lib.QstFfnArgs, **kw)


def attn_desc(**kw):
    return filled(_lib.QstAttnDesc, **kw)


# ------------------------------------------------------------------ references
def drop_state(lib, seed, step):
    """The four-word dropout state of `seed` after `step` advances, built by the library's own init / advance launches."""
    st = torch.zeros(4, dtype=torch.int32, device="cuda")
    _lib.check(lib.qst_dropout_init(st.data_ptr(), seed, stream()))
    for _ in range(step):
        _lib.check(lib.qst_dropout_advance(st.data_ptr(), stream()))
    return st


def drop_desc(st, site, p):
    d = _lib.QstDrop()
    d.state, d.site, d.thr16 = st.data_ptr(), site, D.thr16_of(p)
    return d


def stage_major(s_rowmajor):
    """[rows, K/32] scale bytes -> the library's layout [ceil(K/128)][rows][4] (zero-padded), flattened."""
    rows, nb = s_rowmajor.shape
    pad = (-nb) % 4
    t = torch.nn.functional.pad(s_rowmajor, (0, pad))
    return t.view(rows, (nb + pad) // 4, 4).permute(1, 0, 2).contiguous().view(-1)


def row_major(s_stage, rows, K):
    nb = K // 32
    return s_stage.view((nb + 3) // 4, rows, 4).permute(1, 0, 2).reshape(rows, -1)[:, :nb]


def quant_dev(lib, x, bf16=False):
    """x [rows, K] as MXFP8 on the device: the e4m3 elements and the stage-major scales qst_quant_mx writes."""
    rows, K = x.shape
    src = x.cuda().to(torch.bfloat16 if bf16 else torch.float32).contiguous()
    q = torch.empty(rows, K, dtype=torch.uint8, device="cuda")
    s = torch.zeros((K + 127) // 128 * rows * 4, dtype=torch.uint8, device="cuda")
    _lib.check(lib.qst_quant_mx(src.data_ptr(), int(bf16), rows, K, q.data_ptr(), s.data_ptr(), stream()))
    return q, s


def real_rows(nq, nc, dim, seed):
    """Gaussian query and corpus rows (host fp32) of a real-valued top-k case: topk_stream_cases.REAL_CASES / REAL_SEED."""
    g = torch.Generator().manual_seed(seed + dim)
    return torch.randn(nq, dim, generator=g), torch.randn(nc, dim, generator=g)


@functools.lru_cache(maxsize=None)
def real_case(nq, nc, k, chunk, dim, mode):
    """One of topk_stream_cases.REAL_CASES with its fp64 yardstick, computed once for every test that judges against it (and
    left unchanged by all of them): (q, c, fp64 score matrix, fp64 top-k values, fp64 top-k ids)."""
    q, c = real_rows(nq, nc, dim, T.REAL_SEED[(nq, nc, k, chunk)])
    full = T.scores_ref(q.numpy(), c.numpy(), mode)
    want_s, want_i = T.topk_ref(full, k)
    return q, c, full, want_s, want_i


def new_topk_state(rows, k):
    """An empty running top-k: scores -inf, ids -1."""
    return (torch.full((rows, k), -float("inf"), dtype=torch.float32, device="cuda"),
            torch.full((rows, k), -1, dtype=torch.int64, device="cuda"))


def topk_stream_call(lib, q, c, k, mode, chunk, query_base=0, corpus_base=0, exclude_self=0, max_score=float("inf"),
                     state=None):
    """qst_topk_stream on q, c (device fp32 [nq, dim], [nc, dim]) with a workspace of exactly the size it asks for; returns
    the running (scores, ids). The streaming tests call the entry point by name themselves as well."""
    nq, dim = q.shape
    nc = c.shape[0]
    rs, ri = new_topk_state(nq, k) if state is None else state
    ws = torch.empty(lib.qst_topk_stream_workspace_bytes(nq, min(chunk, nc), dim), dtype=torch.uint8, device="cuda")
    rc = lib.qst_topk_stream(q.data_ptr(), c.data_ptr(), nq, nc, dim, k, mode, chunk, query_base, corpus_base, exclude_self,
                             max_score, rs.data_ptr(), ri.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    assert rc == 0
    return rs, ri


# ------------------------------------------------------------------ encoder harness
def quad_batch(cfg, ids, mask, types, B, L):
    """The quadruplet batch (numpy or torch, 4 * B * L elements each) as the [4B, L] device tensors HipEncoder takes; no type
    ids for a model without a token-type table."""
    idd, mdd, tdd = [torch.as_tensor(x).view(4 * B, L).cuda() for x in (ids, mask, types)]
    return idd, mdd, (tdd if cfg.type_vocab_size else None)


def run_step(cfg, arena, ids, mask, types, B, L, precision="bf16", want_grads=True, scale=None, want_tokens=False, setup=None):
    """A fresh HipEncoder on `arena` (setup(enc), if given, runs before the forward: dropout, fusion switches), one training
    forward at `precision`, the quadruplet loss at the reference's settings and, with want_grads, the backward under the loss
    scale `scale`. Returns the loss (float), the embeddings [4, B, D] and the UNSCALED gradient arena (None without
    want_grads) on the CPU, and the encoder."""
    enc = HipEncoder(cfg)
    enc.load_arena(arena)
    if setup is not None:
        setup(enc)
    idd, mdd, tdd = quad_batch(cfg, ids, mask, types, B, L)
    emb, _, saved = enc.forward(idd, mdd, tdd, training=True, want_tokens=want_tokens, precision=precision)
    e4 = emb.view(4, B, -1)
    gout = None if scale is None else torch.tensor([float(scale)], dtype=torch.float32, device="cuda")
    loss, g = quadruplet_loss_raw(e4[0], e4[1], e4[2], e4[3], 0.6, 1.0, 0.5, 0.5, 2.0, False, 2, grad_out=gout,
                                  want_grads=want_grads)
    grads = None
    if want_grads:
        enc.ensure_train_state()
        enc.grads.zero_()
        enc.backward(idd, mdd, tdd, stacked(g), saved, precision=precision)
        grads = enc.grads.cpu()
        if scale is not None:
            grads = grads / float(scale)
    return loss.item(), e4.cpu(), grads, enc
