#!/usr/bin/env python
"""Achieved bytes/s of qst_margin_mse_loss (csrc/distill.hip) next to qst_triplet_loss (csrc/tuple_loss.hip), which moves
exactly the same bytes with gradients -- three rows in, three rows out -- and of qst_embed_mse (two in, one out), on one
GPU, same process, the two three-row kernels alternated repeat by repeat.

Per repeat: INNER launches between two device events (outputs allocated once, outside the window), after a warm-up of
every shape; the median over the repeats is reported with its quartiles. The bytes are the ones the algorithm needs,
computed from the shapes: rows read once and gradients written once, 4 bytes an element; the [B] side arrays (labels,
per-row values, the second stage) are counted too. At these sizes (19 to 38 MB a call) the rows of one call are still in
the Infinity Cache when the next call reads them, so the rate is that of the cache hierarchy, not of HBM: it compares the
kernels with one another, which is what it is for.

    python tools/distill_bench.py --out profiles/distill_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quadruplet_sentence_transformer_amd  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import _lib, st_losses as S  # noqa: E402

SHAPES = [(4096, 384), (4096, 768)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    lib = _lib.load()
    st = _lib.current_stream_ptr()
    rows = []
    for B, D in SHAPES:
        g = torch.Generator().manual_seed(B + D)
        q, p, n = [torch.randn(B, D, generator=g).cuda() for _ in range(3)]
        y = torch.randn(B, generator=g).cuda()
        gq, gp, gn = [torch.empty_like(q) for _ in range(3)]
        out, scratch, up = torch.empty(1, device="cuda"), torch.empty(B, device="cuda"), torch.ones(1, device="cuda")
        P = lambda t: t.data_ptr()  # noqa: E731
        calls = {
            "qst_margin_mse_loss_dot": lambda: lib.qst_margin_mse_loss(P(q), P(p), P(n), P(y), B, D, S.METRIC_DOT, 2, P(out),
                                                                       None, P(up), P(gq), P(gp), P(gn), P(scratch), st),
            "qst_margin_mse_loss_cos": lambda: lib.qst_margin_mse_loss(P(q), P(p), P(n), P(y), B, D, S.METRIC_COS_SIM, 2,
                                                                       P(out), None, P(up), P(gq), P(gp), P(gn), P(scratch), st),
            "qst_triplet_loss_cos": lambda: lib.qst_triplet_loss(P(q), P(p), P(n), B, D, S.METRIC_COS_DIST, 0.5, 2, P(out),
                                                                 P(up), P(gq), P(gp), P(gn), P(scratch), st),
            "qst_triplet_loss_l2": lambda: lib.qst_triplet_loss(P(q), P(p), P(n), B, D, S.METRIC_L2, 5.0, 2, P(out),
                                                                P(up), P(gq), P(gp), P(gn), P(scratch), st),
            "qst_embed_mse": lambda: lib.qst_embed_mse(P(q), P(p), B, D, P(out), P(up), P(gq), P(scratch), st),
        }
        side = 4 * (2 * B + 2)                          # per-row values written and read again, the result, grad_out
        nbytes = {k: 6 * B * D * 4 + side + (4 * B if "margin" in k else 0) for k in calls}
        nbytes["qst_embed_mse"] = 3 * B * D * 4 + side
        for fn in calls.values():                       # warm-up: code objects, clocks
            for _ in range(20):
                assert fn() == 0
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(args.repeats):
            for k, fn in calls.items():                 # alternated: drift of the box hits all of them alike
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.inner):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / args.inner)
        for k in calls:
            q1, med, q3 = statistics.quantiles(times[k], n=4)
            rows.append({"call": k, "B": B, "D": D, "bytes": nbytes[k], "median_us": round(med, 3),
                         "quartiles_us": [round(q1, 3), round(med, 3), round(q3, 3)],
                         "achieved_TB_per_s": round(nbytes[k] / (med * 1e-6) / 1e12, 3)})
            print(json.dumps(rows[-1]))
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "inner_launches_per_repeat": args.inner,
           "what": "median microseconds of one call with gradients (row kernel + one-workgroup second stage), device events "
                   "around INNER calls, calls alternated repeat by repeat; bytes = rows read once + gradients written once + "
                   "the [B] side arrays", "rows": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
