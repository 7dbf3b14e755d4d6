"""GPU: the host state behind the several-tiles-per-row GEMM + LayerNorm launch (csrc/gemm8.hip: gemm_nt8_ln_kernel, lnx_get,
lnx_finish) -- the one kernel here whose workgroups wait on each other inside a launch. Its arithmetic is checked launch by
launch in test_gpu_kernels.py / test_gpu_fp8mx.py; what is checked here is the exchange buffer: one per (device, stream) with an
epoch on the device, launches back to back with no host synchronisation between them while tile, N, mode and operand form
change, two streams in flight, a capture that borrows another stream's buffer, growth past the 16 MiB minimum with an older
graph alive, and the refusals (a capture before any eager launch; a 17th stream).

References (ln_exchange_cases, judged on the CPU by test_ln_exchange_refs_host.py): fp64 on the CPU from the 16-bit-rounded
operands, at the tolerances of test_gemm_nt_fused_layernorm -- y fp32 rtol 1e-4 / atol 2e-4, rstd rtol 1e-5, the 16-bit copies
rtol 8e-3 / atol 1e-2; mode 1 ds rtol 1e-4 / atol 1e-4 max|ds| (16-bit: 8e-3 / 1e-2 max|ds|), the summed partials rtol 1e-4 /
atol 1e-4 sqrt(M) max|dy|.

Bit-exact comparisons between two launches of the same problem cover EVERY output, not only the mode-0 fp32 rows: the kernel
has a fixed summation order throughout. A row's statistics are reduced over a lane's 8 columns, the row's four lanes
(xg_sum), the four wave columns and the N / BN tiles in index order (t = 0 .. ntn - 1, whoever published first); the mode-1
partials are DPP sums over 16 rows, then two wave rows added in LDS; no value is ever accumulated with an atomic, and which
buffer or epoch a launch runs on enters no arithmetic. So x-hat, rstd, the 16-bit copies, ds and the partials of two launches
must agree bit for bit as well.

Every output is filled with NaN before the launch that is to write it. K = 64 throughout (128 for the fp8 form): the
exchange does not depend on K."""
import json
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import _lib  # noqa: E402
import ln_exchange_cases as X  # noqa: E402
from kernel_helpers import OPDT, gemm_args, kf, lib, ln_epi, op, quant_dev, stream  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


# ------------------------------------------------------------------ one launch: operands, outputs, reference
def make_case(op, M, N, mode, seed, K=64):
    """The operands of one launch, drawn on the device (seeded): what test_gemm_nt_fused_layernorm feeds the kernel; mode 1
    with an x-hat / rstd of its own (the kernel takes them as data)."""
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rn(*shape):
        return torch.randn(*shape, generator=g, device="cuda")
    c = SimpleNamespace(op=op, M=M, N=N, K=K, mode=mode)
    c.A = rn(M, K).to(OPDT[op])
    c.B = (rn(N, K) * 0.05).to(OPDT[op])
    c.resid = rn(M, N)
    c.gamma = 1 + 0.1 * rn(N)
    if mode == 0:
        c.bias, c.beta = rn(N), 0.1 * rn(N)
    else:
        c.xhat = rn(M, N).to(OPDT[op])
        c.rstd = 0.5 + torch.rand(M, generator=g, device="cuda")
    return c


def new_outs(lib, c):
    """NaN-filled outputs of one launch of c (partials sized by qst_gemm_nt_ln_block_rows_m)."""
    M, N, dt = c.M, c.N, OPDT[c.op]
    if c.mode == 0:
        return dict(y=torch.full((M, N), NAN, device="cuda"), y16=torch.full((M, N), NAN, dtype=dt, device="cuda"),
                    xhat=torch.full((M, N), NAN, dtype=dt, device="cuda"), rstd=torch.full((M,), NAN, device="cuda"))
    br = lib.qst_gemm_nt_ln_block_rows_m(N, M)
    assert br == kf(lib, "qst_gemm_nt8_ln_block_rows", c.op)(M, N)
    return dict(ds=torch.full((M, N), NAN, device="cuda"), ds16=torch.full((M, N), NAN, dtype=dt, device="cuda"),
                part=torch.full(((M + br - 1) // br, 2, N), NAN, device="cuda"))


def refill(o):
    for t in o.values():
        t.fill_(NAN)


def launch(lib, c, o, st=None):
    """Enqueue c into the outputs o on stream st (the current stream when None); returns the status."""
    M, N, K = c.M, c.N, c.K
    st = stream() if st is None else st
    if c.mode == 0:
        return kf(lib, "qst_gemm_nt8_ln", c.op)(
            gemm_args(A=c.A, B=c.B, C=o["y"], C2=o["y16"], bias=c.bias, resid=c.resid, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, ldr=N),
            ln_epi(gamma=c.gamma, beta=c.beta, eps=X.EPS, xhat=o["xhat"], rstd=o["rstd"]), 0, st)
    return kf(lib, "qst_gemm_nt8_ln", c.op)(
        gemm_args(A=c.A, B=c.B, C=o["ds"], C2=o["ds16"], resid=c.resid, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, ldr=N),
        ln_epi(gamma=c.gamma, xhat=c.xhat, rstd=c.rstd, partials=o["part"]), 1, st)


def launch_ok(lib, c, o, st=None):
    _lib.check(launch(lib, c, o, st), "qst_gemm_nt8_ln")


def alone(lib, c):
    """c launched by itself on the current stream, between two synchronisations."""
    torch.cuda.synchronize()
    o = new_outs(lib, c)
    launch_ok(lib, c, o)
    torch.cuda.synchronize()
    return o


def assert_same(a, b, what=""):
    """Bit for bit, every output (see the module docstring for why that holds beyond the mode-0 fp32 rows)."""
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: output {k!r} differs between two launches of the same problem"


def close(got, ref, rtol, atol, what):
    torch.testing.assert_close(got.double().cpu(), ref, rtol=rtol, atol=atol, msg=lambda m: f"{what}: {m}")


def check_ref(c, o, rows=None, partials=True, what=""):
    """o against fp64 on the CPU: on all rows, or on `rows` (ascending indices); the mode-1 partials are summed over all
    panels and compared with the column sums over ALL rows unless partials is False."""
    what = what or f"{c.op} ({c.M}, {c.N}) mode {c.mode}"
    di = slice(None) if rows is None else rows.cuda()
    A, B, resid, gamma = c.A[di].cpu(), c.B.cpu(), c.resid[di].cpu(), c.gamma.cpu()
    if c.mode == 0:
        y, xhat, rstd = X.ln_fwd_ref(A, B, c.bias.cpu(), resid, gamma, c.beta.cpu())
        close(o["y"][di], y, 1e-4, 2e-4, what + " y")
        close(o["rstd"][di], rstd, 1e-5, 0, what + " rstd")
        close(o["y16"][di], y, 8e-3, 1e-2, what + " y 16-bit")
        close(o["xhat"][di], xhat, 8e-3, 1e-2, what + " xhat")
        return
    xh = c.xhat[di].cpu()
    dy = X.ln_bwd_dy(A, B, resid)
    ds = X.ln_bwd_ds_ref(dy, gamma, xh, c.rstd[di].cpu())
    scale = float(ds.abs().max())
    close(o["ds"][di], ds, 1e-4, 1e-4 * scale, what + " ds")
    close(o["ds16"][di], ds, 8e-3, 1e-2 * scale, what + " ds 16-bit")
    if partials:
        if rows is not None:
            dy, xh = X.ln_bwd_dy(c.A.cpu(), B, c.resid.cpu()), c.xhat.cpu()
        dg, db = X.ln_bwd_param_ref(dy, xh)
        atol = 1e-4 * math.sqrt(c.M) * float(dy.abs().max())
        close(o["part"][:, 0].sum(0), dg, 1e-4, atol, what + " dgamma")
        close(o["part"][:, 1].sum(0), db, 1e-4, atol, what + " dbeta")


def no_timeouts(lib, op):
    assert kf(lib, "qst_gemm_nt8_ln_timeouts", op)() == 0        # no exchange of row statistics ever gave up waiting


# ------------------------------------------------------------------ the fp8 form (shares the bf16 table of buffers)
def make_f8_case(lib, M, N, K, seed):
    """Operands as test_gemm_f8_with_fused_layernorm quantises them (qst_quant_mx)."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g) * (0.5 + torch.rand(M, 1, generator=g) * 2)
    B = torch.randn(N, K, generator=g) * 0.05
    c = SimpleNamespace(M=M, N=N, K=K)
    c.bias, c.resid = (torch.randn(N, generator=g) * 0.3).cuda(), torch.randn(M, N, generator=g).cuda()
    c.gamma, c.beta = (1 + 0.2 * torch.randn(N, generator=g)).cuda(), (0.3 * torch.randn(N, generator=g)).cuda()
    (c.Aq, c.As), (c.Bq, c.Bs) = quant_dev(lib, A), quant_dev(lib, B)
    return c


def new_f8_outs(c):
    M, N = c.M, c.N
    return dict(y=torch.full((M, N), NAN, device="cuda"), y16=torch.full((M, N), NAN, dtype=torch.bfloat16, device="cuda"),
                xhat=torch.full((M, N), NAN, dtype=torch.bfloat16, device="cuda"), rstd=torch.full((M,), NAN, device="cuda"),
                yq=torch.full((M, N), 0xFF, dtype=torch.uint8, device="cuda"),            # 0xFF: e4m3 NaN
                ys=torch.zeros(N // 128 * M * 4, dtype=torch.uint8, device="cuda"))


def launch_f8(lib, c, o):
    M, N, K = c.M, c.N, c.K
    _lib.check(lib.qst_gemm_nt8_f8_ln(
        gemm_args(A=c.Aq, B=c.Bq, aux=c.As, bscale=c.Bs, C=o["y"], C2=o["y16"], C3=o["yq"], C4=o["ys"], bias=c.bias, resid=c.resid,
                  M=M, N=N, K=K, lda=K, ldb=K, ldc=N, ldr=N),
        ln_epi(gamma=c.gamma, beta=c.beta, eps=X.EPS, xhat=o["xhat"], rstd=o["rstd"]), stream()))


def check_f8_pair(lib, c, o):
    """Against the pair the launch replaces, qst_gemm_nt_f8 (residual epilogue) + qst_ln_fwd_mx_train, at the tolerances of
    test_gemm_f8_with_fused_layernorm."""
    M, N, K = c.M, c.N, c.K
    s = torch.empty(M, N, device="cuda")
    _lib.check(lib.qst_gemm_nt_f8(gemm_args(A=c.Aq, B=c.Bq, aux=c.As, bscale=c.Bs, C=s, bias=c.bias, resid=c.resid, M=M, N=N, K=K,
                                            lda=K, ldb=K, ldc=N, ldr=N), 1, stream()))
    p = new_f8_outs(c)
    _lib.check(lib.qst_ln_fwd_mx_train(s.data_ptr(), c.gamma.data_ptr(), c.beta.data_ptr(), X.EPS, M, N, p["y"].data_ptr(),
                                       p["y16"].data_ptr(), p["xhat"].data_ptr(), p["rstd"].data_ptr(), p["yq"].data_ptr(),
                                       p["ys"].data_ptr(), stream()))
    torch.testing.assert_close(o["y"], p["y"], rtol=1e-4, atol=2e-4)
    torch.testing.assert_close(o["rstd"], p["rstd"], rtol=1e-4, atol=0)
    torch.testing.assert_close(o["y16"].float(), p["y16"].float(), rtol=8e-3, atol=1e-2)
    torch.testing.assert_close(o["xhat"].float(), p["xhat"].float(), rtol=8e-3, atol=1e-2)


# ------------------------------------------------------------------ 1. back to back
def test_back_to_back_launches_change_tile_n_mode_and_form_without_a_host_sync(lib, op):
    """One stream, one buffer, consecutive epochs, no host synchronisation in between: (257, 512) mode 0 | (1300, 768) mode 0
    | (33000, 768) mode 0, the 128 x 384 tile | (1300, 768) mode 1 | bf16 only: qst_gemm_nt8_f8_ln at (300, 768, K = 128) |
    (257, 1024) mode 0 | (33000, 768) mode 1 | (600, 512) mode 1. The granules of each launch lie over those of the one
    before at another geometry (tile rows 256 <-> 128, 2 / 3 / 4 tiles per panel), carrying older tags. Every launch is
    compared with fp64 (M = 33000: on its first 256 rows, its last 256 and 256 rows drawn with a seeded generator; its
    partials over all rows) and, over every row and bit for bit in every output, with the same launch made alone."""
    shapes = [(257, 512, 0), (1300, 768, 0), (33000, 768, 0), (1300, 768, 1), (257, 1024, 0), (33000, 768, 1), (600, 512, 1)]
    assert kf(lib, "qst_gemm_nt8_ln_block_rows", op)(33000, 768) == 128 and kf(lib, "qst_gemm_nt8_ln_block_rows", op)(1300, 768) == 256
    cases = [make_case(op, M, N, mode, seed=100 + i) for i, (M, N, mode) in enumerate(shapes)]
    outs = [new_outs(lib, c) for c in cases]
    f8 = make_f8_case(lib, 300, 768, 128, seed=9) if op == "bf16" else None
    f8o = new_f8_outs(f8) if f8 else None
    torch.cuda.synchronize()
    for i, (c, o) in enumerate(zip(cases, outs)):
        launch_ok(lib, c, o)
        if f8 and i == 3:
            launch_f8(lib, f8, f8o)
    torch.cuda.synchronize()
    for c, o in zip(cases, outs):
        rows = X.subset_rows(c.M, 256, 256, 256, seed=c.M) if c.M == 33000 else None
        check_ref(c, o, rows)
        assert_same(o, alone(lib, c), f"{op} ({c.M}, {c.N}) mode {c.mode}, back to back against alone")
    if f8:
        check_f8_pair(lib, f8, f8o)
        torch.cuda.synchronize()
        a = new_f8_outs(f8)
        launch_f8(lib, f8, a)
        torch.cuda.synchronize()
        assert_same(f8o, a, "qst_gemm_nt8_f8_ln, back to back against alone")
    no_timeouts(lib, op)


# ------------------------------------------------------------------ 2. many epochs
def test_three_hundred_consecutive_epochs_on_one_buffer(lib, op):
    """300 launches at (257, 512) back to back, mode 0 and mode 1 in turn, every one over the granules of the one before (the
    same geometry: the only thing that tells a fresh granule from a stale one is the tag). The first and the last mode-0
    launch agree bit for bit; the last of each mode matches fp64."""
    c0, c1 = make_case(op, 257, 512, 0, seed=21), make_case(op, 257, 512, 1, seed=22)
    first, last0, last1 = new_outs(lib, c0), new_outs(lib, c0), new_outs(lib, c1)
    mid0, mid1 = new_outs(lib, c0), new_outs(lib, c1)
    torch.cuda.synchronize()
    for i in range(300):
        if i % 2 == 0:
            launch_ok(lib, c0, first if i == 0 else last0 if i == 298 else mid0)
        else:
            launch_ok(lib, c1, last1 if i == 299 else mid1)
    torch.cuda.synchronize()
    assert_same(first, last0, f"{op}: epoch 1 against epoch 299")
    check_ref(c0, last0)
    check_ref(c1, last1)
    no_timeouts(lib, op)


# ------------------------------------------------------------------ 3. two streams in flight
_SIDE = []


def side_streams():
    """Two streams for the whole module: a (device, stream) slot is never released, so the tests share them."""
    if not _SIDE:
        _SIDE.extend([torch.cuda.Stream(), torch.cuda.Stream()])
    return _SIDE


def test_two_streams_in_flight_keep_their_granules_apart(lib, op):
    """Two streams, each warmed by one eager launch (so each has its own slot, buffer and epoch), then 20 launches of
    (1300, 768) mode 0 on the first and 20 on the second -- (257, 1024) mode 0 and (600, 512) mode 1 in turn -- issued
    interleaved from the host with no synchronisation: panels 0 .. 5 of the first stream's launches and panels 0 .. 2 of the
    second's would land on the same granules of a shared buffer. Every launch has operands of its own. All 40 results
    match fp64 and, bit for bit, the same launch on the default stream."""
    s1, s2 = side_streams()
    assert len({0, s1.cuda_stream, s2.cuda_stream, torch.cuda.default_stream().cuda_stream}) >= 3
    on1 = [make_case(op, 1300, 768, 0, seed=300 + i) for i in range(20)]
    on2 = [make_case(op, 257, 1024, 0, seed=340 + i) if i % 2 == 0 else make_case(op, 600, 512, 1, seed=340 + i) for i in range(20)]
    out1, out2 = [new_outs(lib, c) for c in on1], [new_outs(lib, c) for c in on2]
    warm1, warm2 = new_outs(lib, on1[0]), new_outs(lib, on2[0])
    torch.cuda.synchronize()                    # the operands were drawn on the default stream
    launch_ok(lib, on1[0], warm1, s1.cuda_stream)
    launch_ok(lib, on2[0], warm2, s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    for i in range(20):
        launch_ok(lib, on1[i], out1[i], s1.cuda_stream)
        launch_ok(lib, on2[i], out2[i], s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    no_timeouts(lib, op)
    for c, o in list(zip(on1, out1)) + list(zip(on2, out2)):
        check_ref(c, o)
        assert_same(o, alone(lib, c), f"{op} ({c.M}, {c.N}) mode {c.mode}, two streams in flight against the default stream")
    assert_same(warm1, out1[0], "warm-up launch")
    no_timeouts(lib, op)


# ------------------------------------------------------------------ 4. a capture that borrows
def fresh_stream():
    """A stream this module has not launched on eagerly (torch hands streams out of a pool, round robin)."""
    taken = {0, torch.cuda.default_stream().cuda_stream} | {s.cuda_stream for s in _SIDE}
    for _ in range(64):
        s = torch.cuda.Stream()
        if s.cuda_stream not in taken:
            return s
    raise AssertionError("no stream apart from the ones already used")


def test_capture_on_a_stream_without_a_buffer_borrows_one(lib, op):
    """After an eager warm-up on the default stream at (1300, 768), a stream that has never launched the kernel captures
    one mode-0 and one mode-1 launch: it cannot allocate while capturing and takes the smallest buffer on the device that
    fits, with that buffer's epoch. Three replays with nothing else running, the outputs NaN-filled before each, give the
    eager result bit for bit."""
    c0, c1 = make_case(op, 1300, 768, 0, seed=41), make_case(op, 1300, 768, 1, seed=42)
    e0, e1 = alone(lib, c0), alone(lib, c1)
    check_ref(c0, e0)
    check_ref(c1, e1)
    r0, r1 = new_outs(lib, c0), new_outs(lib, c1)
    s = fresh_stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=s):
        assert stream() == s.cuda_stream
        launch_ok(lib, c0, r0)
        launch_ok(lib, c1, r1)
    for rep in range(3):
        refill(r0)
        refill(r1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert_same(r0, e0, f"{op}: replay {rep}, mode 0")
        assert_same(r1, e1, f"{op}: replay {rep}, mode 1")
    no_timeouts(lib, op)


# ------------------------------------------------------------------ 5. growth past the minimum buffer
def test_growth_past_the_minimum_buffer_keeps_an_older_graph_valid(lib):
    """The exchange needs ceil(M / 256) (N / 256) 256 16 bytes: more than the 16 MiB minimum first at N = 1024, M > 262,144.
    M = 262,200 is 1025 panels, the last of 56 rows. Order: a graph is captured at (1300, 768) (it borrows a 16 MiB buffer);
    the large shape runs eagerly, mode 0 then mode 1 (the default stream's buffer is outgrown and replaced; the old one
    must stay, the graph holds its address); the graph is replayed; (257, 512) runs eagerly on the new buffer. Only results
    are asserted, so the test holds as well in a process whose buffer has grown already. The large launch is compared over
    all rows with the unfused pair (qst_gemm_nt + qst_ln_fwd / qst_ln_bwd) at the tolerances of test_gemm_nt_fused_layernorm,
    and with fp64 on the first panel, the ragged last panel and 64 rows drawn with a seeded generator. Operands are drawn
    on the device; the fp32 tensors are 1.07 GB each."""
    op = "bf16"
    M, N, K = 262200, 1024, 64
    assert (M + 255) // 256 * (N // 256) * 256 * 16 > 16 << 20 and lib.qst_gemm_nt8_ln_block_rows(M, N) == 256
    # 1. the older graph
    g0, g1 = make_case(op, 1300, 768, 0, seed=51), make_case(op, 1300, 768, 1, seed=52)
    e0, e1 = alone(lib, g0), alone(lib, g1)
    check_ref(g0, e0)
    check_ref(g1, e1)
    r0, r1 = new_outs(lib, g0), new_outs(lib, g1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch_ok(lib, g0, r0)
        launch_ok(lib, g1, r1)
    graph.replay()
    torch.cuda.synchronize()
    assert_same(r0, e0, "graph before the growth, mode 0")
    assert_same(r1, e1, "graph before the growth, mode 1")
    # 2. the large shape, mode 0 then mode 1
    c0 = make_case(op, M, N, 0, seed=53)
    o0 = new_outs(lib, c0)
    launch_ok(lib, c0, o0)
    c1 = SimpleNamespace(op=op, M=M, N=N, K=K, mode=1, A=c0.A, B=c0.B, resid=c0.resid, gamma=c0.gamma, xhat=o0["xhat"], rstd=o0["rstd"])
    o1 = new_outs(lib, c1)
    launch_ok(lib, c1, o1)                       # mode 1 on what mode 0 has just written: stream order
    # 3. the old graph, 4. a small launch on the new buffer
    refill(r0)
    refill(r1)
    graph.replay()
    small = make_case(op, 257, 512, 0, seed=54)
    so = new_outs(lib, small)
    launch_ok(lib, small, so)
    torch.cuda.synchronize()
    no_timeouts(lib, op)
    assert_same(r0, e0, "graph after the growth, mode 0")
    assert_same(r1, e1, "graph after the growth, mode 1")
    check_ref(small, so)
    rows = X.subset_rows(M, 256, 56, 64, seed=55)
    check_ref(c0, o0, rows)
    check_ref(c1, o1, rows, partials=False)      # the partials: against the pair below, over all rows
    # the unfused pair, forward
    s = torch.empty(M, N, device="cuda")
    _lib.check(lib.qst_gemm_nt(gemm_args(A=c0.A, B=c0.B, C=s, bias=c0.bias, resid=c0.resid, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, ldr=N),
                               1, stream()))
    p = new_outs(lib, c0)
    _lib.check(lib.qst_ln_fwd(s.data_ptr(), c0.gamma.data_ptr(), c0.beta.data_ptr(), X.EPS, M, N, p["y"].data_ptr(), p["y16"].data_ptr(),
                              p["xhat"].data_ptr(), p["rstd"].data_ptr(), stream()))
    torch.testing.assert_close(o0["y"], p["y"], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(o0["rstd"], p["rstd"], rtol=1e-5, atol=0)
    torch.testing.assert_close(o0["y16"].float(), p["y16"].float(), rtol=8e-3, atol=1e-2)
    torch.testing.assert_close(o0["xhat"].float(), p["xhat"].float(), rtol=8e-3, atol=1e-2)
    del p
    # ... and backward, from the same xhat / rstd the fused launch was given (s: dy = A.B^T + resid)
    _lib.check(lib.qst_gemm_nt(gemm_args(A=c0.A, B=c0.B, C=s, resid=c0.resid, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, ldr=N), 1, stream()))
    ds, ds16 = torch.full((M, N), NAN, device="cuda"), torch.full((M, N), NAN, dtype=OPDT[op], device="cuda")
    dg, db = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    scratch = torch.empty(lib.qst_ln_bwd_scratch_bytes(M, N) // 4, device="cuda")
    _lib.check(lib.qst_ln_bwd(s.data_ptr(), c1.xhat.data_ptr(), c1.rstd.data_ptr(), c1.gamma.data_ptr(), M, N, ds.data_ptr(),
                              ds16.data_ptr(), dg.data_ptr(), db.data_ptr(), scratch.data_ptr(), stream()))
    scale = ds.abs().max().item()
    dymax = s.abs().max().item()
    torch.testing.assert_close(o1["ds"], ds, rtol=1e-4, atol=1e-4 * scale)
    torch.testing.assert_close(o1["ds16"].float(), ds16.float(), rtol=8e-3, atol=1e-2 * scale)
    torch.testing.assert_close(o1["part"][:, 0].sum(0), dg, rtol=1e-4, atol=1e-4 * math.sqrt(M) * dymax)
    torch.testing.assert_close(o1["part"][:, 1].sum(0), db, rtol=1e-4, atol=1e-4 * math.sqrt(M) * dymax)
    no_timeouts(lib, op)
    del s, ds, ds16, o0, o1, c0, c1, scratch
    torch.cuda.empty_cache()                     # some 8 GB back to the device for the tests that follow


# ------------------------------------------------------------------ 6. refusals that need a fresh process
_CHILD_DIED = []

_CHILD_PRELUDE = """
import json, sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch
import test_gpu_ln_exchange as T
from quadruplet_sentence_transformer_amd import _lib
lib = _lib.load()
res = {{}}


def right(c, o):
    try:
        T.check_ref(c, o)
    except AssertionError as e:
        return str(e)[:300]
    return True
"""

_CHILD_CAPTURE_FIRST = _CHILD_PRELUDE + """
c = T.make_case("bf16", 1300, 768, 0, seed=61)
cap, eager, marker = T.new_outs(lib, c), T.new_outs(lib, c), torch.zeros(8, device="cuda")
torch.cuda.synchronize()
s = torch.cuda.Stream()
g1 = torch.cuda.CUDAGraph()
with torch.cuda.graph(g1, stream=s):
    marker.fill_(1.0)                           # the capture is not empty
    res["first_call_in_capture"] = T.launch(lib, c, cap)      # the first call of the process
torch.cuda.synchronize()
res["eager"] = T.launch(lib, c, eager)
torch.cuda.synchronize()
res["eager_right"] = right(c, eager)
# the f16 twin has a table of its own: the bf16 warm-up above does not count for it
h = T.make_case("f16", 1300, 768, 0, seed=62)
hcap, heager = T.new_outs(lib, h), T.new_outs(lib, h)
torch.cuda.synchronize()
g2 = torch.cuda.CUDAGraph()
with torch.cuda.graph(g2, stream=s):
    res["second_capture"] = T.launch(lib, c, cap)
g2.replay()
torch.cuda.synchronize()
res["replay_equals_eager"] = all(torch.equal(cap[k], eager[k]) for k in cap)
g3 = torch.cuda.CUDAGraph()
with torch.cuda.graph(g3, stream=s):
    marker.fill_(2.0)
    res["f16_first_call_in_capture"] = T.launch(lib, h, hcap)
torch.cuda.synchronize()
res["f16_eager"] = T.launch(lib, h, heager)
torch.cuda.synchronize()
res["f16_eager_right"] = right(h, heager)
res["timeouts"] = [lib.qst_gemm_nt8_ln_timeouts(), lib.qst_gemm_nt8_ln_timeouts_f16()]
print("RESULT " + json.dumps(res))
"""

_CHILD_SLOTS = _CHILD_PRELUDE + """
op = sys.argv[1]
c = T.make_case(op, 257, 512, 0, seed=71)
streams = [torch.cuda.Stream() for _ in range(16)]
ptrs = [torch.cuda.default_stream().cuda_stream] + [s.cuda_stream for s in streams]
res["distinct_streams"] = len(set(ptrs))
outs = [T.new_outs(lib, c) for _ in range(17)]
torch.cuda.synchronize()
res["first_round"] = [T.launch(lib, c, o, p) for o, p in zip(outs[:16], ptrs[:16])]
torch.cuda.synchronize()
res["first_round_right"] = [right(c, o) for o in outs[:16]]
res["seventeenth"] = T.launch(lib, c, outs[16], ptrs[16])
torch.cuda.synchronize()
res["seventeenth_untouched"] = bool(torch.isnan(outs[16]["y"]).all())
try:
    _lib.check(res["seventeenth"], "qst_gemm_nt8_ln")
    res["wrapper"] = "no error"
except _lib.QstError as e:
    res["wrapper"] = str(e)
for o in outs[:16]:
    T.refill(o)
res["second_round"] = [T.launch(lib, c, o, p) for o, p in zip(outs[:16], ptrs[:16])]
torch.cuda.synchronize()
res["second_round_right"] = [right(c, o) for o in outs[:16]]
res["all_equal"] = all(torch.equal(o[k], outs[0][k]) for o in outs[:16] for k in o)
res["timeouts"] = T.kf(lib, "qst_gemm_nt8_ln_timeouts", op)()
print("RESULT " + json.dumps(res))
"""


def run_child(code, *args, limit=150):
    """One fresh process, alone, under its own time limit; its JSON result line. A child that ends on a signal or at its
    limit fails the test, and no further child is started in this session."""
    if _CHILD_DIED:
        pytest.fail(f"not started: an earlier child process {_CHILD_DIED[0]}")
    src = code.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    try:
        r = subprocess.run([sys.executable, "-c", src, *args], capture_output=True, text=True, timeout=limit, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _CHILD_DIED.append(f"ran into its time limit of {limit} s")
        pytest.fail(f"the child process {_CHILD_DIED[0]}")
    if r.returncode < 0:
        _CHILD_DIED.append(f"ended on signal {-r.returncode}")
        pytest.fail(f"the child process {_CHILD_DIED[0]}:\n{r.stderr[-2000:]}")
    assert r.returncode == 0, f"child exit status {r.returncode}:\n{r.stderr[-2000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0][len("RESULT "):])


def test_capture_before_any_eager_launch_is_refused_and_works_after_one():
    """In a fresh process the first call ever of qst_gemm_nt8_ln is made inside a stream capture: QST_ERR_UNSUPPORTED (-2),
    nothing recorded, and the capture ends normally. After one eager launch a new capture of the same launch succeeds and
    replays to the eager result bit for bit. The f16 twin keeps a table of its own: with the bf16 buffer there, its first
    call inside a capture is refused all the same, and it launches eagerly afterwards."""
    res = run_child(_CHILD_CAPTURE_FIRST)
    assert res["first_call_in_capture"] == -2
    assert res["eager"] == 0 and res["eager_right"] is True
    assert res["second_capture"] == 0 and res["replay_equals_eager"] is True
    assert res["f16_first_call_in_capture"] == -2
    assert res["f16_eager"] == 0 and res["f16_eager_right"] is True
    assert res["timeouts"] == [0, 0]


def test_a_seventeenth_stream_is_refused_and_the_sixteen_go_on(op):
    """Sixteen (device, stream) pairs per process and operand type, the default stream among them, never released -- hence a
    child process. Eager launches at (257, 512) on the default stream and 15 others are all right; on a 17th stream the
    launch returns QST_ERR_UNSUPPORTED (-2) and writes nothing, which _lib.check raises as the library's "unsupported" error;
    a further launch on each of the sixteen is right again."""
    res = run_child(_CHILD_SLOTS, op)
    assert res["distinct_streams"] == 17
    assert res["first_round"] == [0] * 16 and res["first_round_right"] == [True] * 16
    assert res["seventeenth"] == -2 and res["seventeenth_untouched"] is True
    assert "unsupported" in res["wrapper"] and res["wrapper"].startswith("qst_gemm_nt8_ln")
    assert res["second_round"] == [0] * 16 and res["second_round_right"] == [True] * 16 and res["all_equal"] is True
    assert res["timeouts"] == 0
