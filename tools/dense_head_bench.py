#!/usr/bin/env python
"""Time of models.Dense's kernels (csrc/dense_head.hip): one qst_dense_head_fwd and one qst_dense_head_bwd (tanh, with the
normalisation and a bias: every stage runs) at the shapes a training step meets.

After a warm-up call, REPEATS windows of INNER calls between two device events (outputs and workspace allocated once, outside
the window; INNER chosen so that a window lasts about half a second); the median window over INNER is reported with the
smallest and the largest. The results are compared with the fp64 reference of tests/dense_head_helpers.py first, so a time
is only printed for calls that computed the right numbers. GFLOP = 2 * B * Din * Dout for the forward, twice that for the
backward's two products.

    python tools/dense_head_bench.py --out profiles/dense_head_bench.txt
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import dense_head_helpers as H  # noqa: E402
from quadruplet_sentence_transformer_amd import _lib  # noqa: E402

SHAPES = [(256, 384, 384), (256, 768, 768), (1024, 768, 128)]


def windows_of(call, repeats, window):
    call()                                                  # warm-up: code objects, clocks
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):                                     # a first estimate, without the first call's set-up
        call()
    torch.cuda.synchronize()
    est = (time.perf_counter() - t0) / 50
    inner = int(min(max(window / max(est, 1e-6), 1), 100000))
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            call()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / inner * 1e3)       # microseconds a call
    return out, inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    lib = _lib.load()
    st = _lib.current_stream_ptr()
    lines = [f"qst_dense_head_fwd / qst_dense_head_bwd (tanh, normalize, bias; fp32) on {torch.cuda.get_device_name(0)}: "
             f"microseconds a call, median of {args.repeats} windows (min - max), calls per window",
             f"{'B':>6} {'Din':>5} {'Dout':>5} {'fwd us':>9} {'(min - max)':>17} {'bwd us':>9} {'(min - max)':>17} "
             f"{'fwd+bwd us':>11} {'calls':>7} {'GFLOP':>7} {'TFLOP/s':>8}"]
    for B, Din, Dout in SHAPES:
        x, w, b, dy = H.case(B, Din, Dout, True, 77)
        _, _, ref_y, *ref_g = H.reference_of(x, w, b, dy, H.TANH, 1)
        x, w, b, dy = [t.cuda() for t in (x, w, b, dy)]
        y, norm, gx, gw, gb = H.run_all(lib, x, w, b, dy, H.TANH, 1, st)
        assert H.value_error(y, ref_y, Din) <= 1.0 and max(H.grad_error(g.cpu(), r) for g, r in zip((gx, gw, gb), ref_g)) <= 1.0
        nbytes = lib.qst_dense_head_bwd_workspace_bytes(B, Din, Dout)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        p = lambda t: t.data_ptr()  # noqa: E731
        fwd = lambda: lib.qst_dense_head_fwd(p(x), Din, p(w), p(b), B, Din, Dout, H.TANH, 1, p(y), p(norm), st)  # noqa: E731
        bwd = lambda: lib.qst_dense_head_bwd(p(x), Din, p(w), p(y), p(norm), p(dy), B, Din, Dout, H.TANH, 1, p(gx), p(gw),  # noqa: E731
                                             p(gb), p(ws), nbytes, st)
        assert fwd() == 0 and bwd() == 0
        f, nf = windows_of(fwd, args.repeats, args.window)
        g, ng = windows_of(bwd, args.repeats, args.window)
        mf, mg = statistics.median(f), statistics.median(g)
        gflop = 6.0 * B * Din * Dout / 1e9
        lines.append(f"{B:>6} {Din:>5} {Dout:>5} {mf:>9.2f} {f'({min(f):.2f} - {max(f):.2f})':>17} {mg:>9.2f} "
                     f"{f'({min(g):.2f} - {max(g):.2f})':>17} {mf + mg:>11.2f} {min(nf, ng):>7} {gflop:>7.3f} "
                     f"{gflop / ((mf + mg) * 1e-6) / 1e3:>8.2f}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
