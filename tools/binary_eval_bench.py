#!/usr/bin/env python
"""Time of one qst_binary_eval call (csrc/binary_eval.hip) for the four score rows BinaryClassificationEvaluator hands it,
next to the host time of what it replaces: sentence-transformers' sort-and-loop scoring, as tests/binary_eval_helpers.py
restates it (sorted + a Python loop for the best accuracy, the same for the best F1, the average precision in numpy), on
the same scores and labels.

Device: after a warm-up call, REPEATS windows of INNER calls between two device events (workspace and output allocated once,
outside the window; INNER chosen so that a window lasts about half a second, at least one call); the median window over
INNER is reported with the smallest and the largest. Host: a wall clock around the three routines over the four rows, once
(it takes seconds). The two results are compared as the GPU test compares them, so a time is only printed for a call that
computed the right numbers. The pair steps of a call are nsets * n^2.

    python tools/binary_eval_bench.py --out profiles/binary_eval.txt
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import binary_eval_helpers as BH  # noqa: E402
from quadruplet_sentence_transformer_amd import _lib  # noqa: E402

FLAGS = (1, 0, 0, 1)                # cosine, Manhattan, Euclidean, dot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 14, 1 << 17, 1 << 20])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of calls per timed window")
    ap.add_argument("--no-host", action="store_true", help="skip the host loops (and the comparison with them)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    lib = _lib.load()
    st = _lib.current_stream_ptr()
    lines = [f"qst_binary_eval, nsets = 4 (flags {FLAGS}), on {torch.cuda.get_device_name(0)}; host = the sort-and-loop "
             f"routines of tests/binary_eval_helpers.py on the same inputs",
             f"{'n':>8} {'device ms (median)':>19} {'min':>10} {'max':>10} {'calls/window':>13} {'Gpair-steps/s':>14} "
             f"{'host s':>9} {'host / device':>14}"]
    for n in args.sizes:
        rng = np.random.RandomState(n)
        labels = (rng.rand(n) < 0.4).astype(np.int64)
        # similar pairs score higher (lower for the two distances), with overlap, rounded so that equal scores occur
        sim = np.round(rng.randn(n) + 1.5 * labels, 3).astype(np.float32)
        rows = np.stack([sim, -sim + 8, np.abs(sim - 4), 3 * sim]).astype(np.float32)
        scores, y = torch.from_numpy(rows).cuda(), torch.from_numpy(labels).cuda()
        nbytes = lib.qst_binary_eval_workspace_bytes(n, 4)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        out = torch.empty(4, 8, dtype=torch.float64, device="cuda")
        flags = (ctypes.c_int32 * 4)(*FLAGS)
        call = lambda: lib.qst_binary_eval(scores.data_ptr(), y.data_ptr(), n, 4, flags, out.data_ptr(), ws.data_ptr(),  # noqa: E731
                                           nbytes, st)
        t0 = time.perf_counter()
        assert call() == 0                                  # warm-up: code objects, clocks; and a first estimate
        torch.cuda.synchronize()
        est = time.perf_counter() - t0
        assert call() == 0
        torch.cuda.synchronize()
        inner = int(min(max(args.window / max(est, 1e-6), 1), 200))
        windows = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                call()
            e1.record()
            e1.synchronize()
            windows.append(e0.elapsed_time(e1) / inner)
        got = out.cpu().numpy()
        med = statistics.median(windows)
        host_s = float("nan")
        if not args.no_host:
            t0 = time.perf_counter()
            want = np.array([BH.expected(r, labels, bool(f)) for r, f in zip(rows, FLAGS)])
            host_s = time.perf_counter() - t0
            exact = [BH.ACC, BH.ACC_THR, BH.F1, BH.PREC, BH.REC, BH.F1_THR, BH.POS]
            assert np.array_equal(got[:, exact], want[:, exact]), (n, got, want)
            assert (np.abs(got[:, BH.AP] - want[:, BH.AP]) <= BH.ap_bound(n)).all(), (n, got, want)
        lines.append(f"{n:>8} {med:>19.3f} {min(windows):>10.3f} {max(windows):>10.3f} {inner:>13} "
                     f"{4.0 * n * n / (med * 1e-3) / 1e9:>14.1f} {host_s:>9.3f} {host_s / (med * 1e-3):>14.1f}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
