#!/usr/bin/env python
"""Time of one qst_rerank_scores + qst_rerank_metrics call (csrc/rerank.hip) for what RerankingEvaluator hands them -- nq
queries, each with its own group of candidate documents in one flat array -- next to the host time of what it replaces:
sentence-transformers' per-query scoring and ranking, as tests/rerank_helpers.py restates it (a cosine per group, a stable
argsort and a walk, the average precision as sklearn takes it, NDCG), on the same embeddings.

Device: embeddings generated on the device from a seed; after a warm-up call, REPEATS windows of INNER calls between two
device events (scores, workspace and outputs allocated once, outside the window; INNER chosen so that a window lasts about
half a second, at least one call); the median window over INNER is reported with the smallest and the largest, and the two
entry points also on their own. Host: a wall clock around the cosine (fp32 numpy, one matrix-vector product per group) and
the yardstick over the first --host-queries groups, whose embeddings are copied to the host beforehand -- the whole set at
group size 1,000 is 15 GB of documents; both sides are reported per query. The device's numbers for those groups are
compared with the yardstick on the device's own scores as the GPU test compares them, so a time is only printed for a call
that computed the right numbers.

    python tools/rerank_bench.py --out profiles/rerank.txt
"""
import argparse
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
import rerank_helpers as RH  # noqa: E402
from quadruplet_sentence_transformer_amd import _lib, util  # noqa: E402

K = 10


def windows_of(call, window, repeats):
    """The median, smallest and largest time of one call in ms, and the calls per window."""
    t0 = time.perf_counter()
    call()                                              # warm-up: code objects, clocks; and a first estimate
    torch.cuda.synchronize()
    est = time.perf_counter() - t0
    call()
    torch.cuda.synchronize()
    inner = int(min(max(window / max(est, 1e-6), 1), 2000))
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / inner)
    return statistics.median(times), min(times), max(times), inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--group-sizes", type=int, nargs="+", default=[30, 1000])
    ap.add_argument("--positives", type=int, default=3)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of calls per timed window")
    ap.add_argument("--host-queries", type=int, default=200, help="groups the host routines run over (0: skip them)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    lib = _lib.load()
    st = _lib.current_stream_ptr()
    nq, D, P = args.queries, args.dim, args.positives
    lines = [f"qst_rerank_scores (cos) + qst_rerank_metrics (k = {K}), nq = {nq}, D = {D}, {P} positives per group, on "
             f"{torch.cuda.get_device_name(0)}; host = a cosine per group in numpy and the yardstick of tests/rerank_helpers.py "
             f"on the same embeddings, over the first {args.host_queries} groups",
             f"{'group':>6} {'nd':>9} {'both ms (median)':>17} {'min':>9} {'max':>9} {'calls/window':>13} {'scores ms':>10} "
             f"{'metrics ms':>11} {'device us/query':>16} {'host us/query':>14} {'host / device':>14}"]
    for size in args.group_sizes:
        nd = nq * size
        gen = torch.Generator(device="cuda").manual_seed(size)
        q = torch.randn(nq, D, device="cuda", generator=gen)
        d = torch.randn(nd, D, device="cuda", generator=gen)
        d.view(nq, size, D)[:, :P] += q[:, None, :]     # a group's positives lean towards its query
        offsets = torch.arange(nq + 1, dtype=torch.int64, device="cuda") * size
        num_pos = torch.full((nq,), P, dtype=torch.int32, device="cuda")
        scores = torch.empty(nd, dtype=torch.float32, device="cuda")
        per_query = torch.empty(nq, 3, dtype=torch.float64, device="cuda")
        out = torch.empty(5, dtype=torch.float64, device="cuda")
        nbytes = lib.qst_rerank_workspace_bytes(nq, nd)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

        def score():
            rc = lib.qst_rerank_scores(q.data_ptr(), d.data_ptr(), offsets.data_ptr(), nq, nd, D, util.SCORE_COS,
                                       scores.data_ptr(), st)
            assert rc == 0

        def metrics():
            rc = lib.qst_rerank_metrics(scores.data_ptr(), offsets.data_ptr(), num_pos.data_ptr(), nq, nd, K,
                                        per_query.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, st)
            assert rc == 0

        both = windows_of(lambda: (score(), metrics()), args.window, args.repeats)
        only_scores = windows_of(score, args.window, args.repeats)
        only_metrics = windows_of(metrics, args.window, args.repeats)
        totals = out.cpu().numpy()
        assert totals[3] == 0 and totals[4] == 0, totals
        host_us = float("nan")
        h = min(args.host_queries, nq)
        if h > 0:
            qh, dh = q[:h].cpu().numpy(), d[:h * size].cpu().numpy().reshape(h, size, D)
            off_h, pos_h = np.arange(h + 1, dtype=np.int64) * size, np.full(h, P, dtype=np.int32)
            t0 = time.perf_counter()
            s = np.concatenate([(dh[g] @ qh[g]) / (np.maximum(np.linalg.norm(dh[g], axis=1), 1e-12) *
                                                   max(np.linalg.norm(qh[g]), 1e-12)) for g in range(h)])
            RH.expected(s, off_h, pos_h, K)
            host_us = (time.perf_counter() - t0) / h * 1e6
            # the device's numbers for those groups against the yardstick on the device's own scores
            want = RH.expected(scores[:h * size].cpu().numpy(), off_h, pos_h, K)
            got = per_query[:h].cpu().numpy()
            assert np.array_equal(got[:, RH.RR], want[:, RH.RR]), size
            assert (np.abs(got[:, RH.AP] - want[:, RH.AP]) <= RH.ap_bound(P)).all(), size
            assert (np.abs(got[:, RH.NDCG] - want[:, RH.NDCG]) <= RH.ndcg_bound(K)).all(), size
        dev_us = both[0] * 1e3 / nq
        lines.append(f"{size:>6} {nd:>9} {both[0]:>17.3f} {both[1]:>9.3f} {both[2]:>9.3f} {both[3]:>13} {only_scores[0]:>10.3f} "
                     f"{only_metrics[0]:>11.3f} {dev_us:>16.3f} {host_us:>14.1f} {host_us / dev_us:>14.1f}")
        print(lines[-1], flush=True)
        del q, d, scores, ws
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
