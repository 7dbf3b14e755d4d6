#!/usr/bin/env python
"""Achieved bytes/s of qst_margin_mse_loss (csrc/distill.hip) next to qst_triplet_loss (csrc/tuple_loss.hip), which moves
exactly the same bytes with gradients -- three rows in, three rows out -- and of qst_embed_mse (two in, one out), on one
GPU, same process, the two three-row kernels alternated repeat by repeat. The other two row-wise losses built on
csrc/row_loss.h run under the same scheme: qst_quadruplet_loss (p = 2, swap on, mean: four rows in, four out) and
qst_pair_loss (contrastive on the cosine distance, mean: two in, two out).

Per repeat: INNER launches between two device events (outputs allocated once, outside the window), after a warm-up of
every shape; the median over the repeats is reported with its quartiles. The bytes are the ones the algorithm needs,
computed from the shapes: rows read once and gradients written once, 4 bytes an element; the [B] side arrays (labels,
per-row values, the second stage) are counted too. At these sizes (19 to 38 MB a call) the rows of one call are still in
the Infinity Cache when the next call reads them, so the rate is that of the cache hierarchy, not of HBM: it compares the
kernels with one another, which is what it is for.

    python tools/distill_bench.py --out profiles/distill_bench.json
    python tools/distill_bench.py --lib /path/to/another/libqst.so --out ...     (the same calls on another build)
    python tools/distill_bench.py --lib A/libqst.so --out a.json --lib B/libqst.so --out b.json

The last form compares two builds: both libraries are loaded into this one process and take turns repeat by repeat (which
of them goes first turns too), one result file each. Two separate runs of the SAME build differ by several times a run's
interquartile spread (placement of the process's buffers, the state of the box), so only this form can tell a build's
effect from that offset.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quadruplet_sentence_transformer_amd  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import _lib, st_losses as S  # noqa: E402

SHAPES = [(4096, 384), (4096, 768)]


def bind(path):
    """A build of the library of its own (not _lib's one per process), with the signatures of the five entry points."""
    lib = ctypes.CDLL(path)
    for name in ("qst_margin_mse_loss", "qst_triplet_loss", "qst_embed_mse", "qst_quadruplet_loss", "qst_pair_loss"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--out", action="append", default=None, help="result file; with several --lib, one per build, in order")
    ap.add_argument("--lib", action="append", default=None,
                    help="a build of libqst.so to measure instead of the tree's; give it more than once to alternate builds")
    args = ap.parse_args()
    paths = [os.path.abspath(x) for x in (args.lib or [_lib.LIB_PATH])]
    assert args.out is None or len(args.out) == len(paths), "one --out per --lib"
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    libs = [bind(x) for x in paths]
    st = _lib.current_stream_ptr()
    rows = [[] for _ in libs]
    for B, D in SHAPES:
        g = torch.Generator().manual_seed(B + D)
        q, p, n = [torch.randn(B, D, generator=g).cuda() for _ in range(3)]
        y = torch.randn(B, generator=g).cuda()
        x4, y01 = torch.randn(B, D, generator=g).cuda(), (torch.rand(B, generator=g) < 0.5).float().cuda()
        gq, gp, gn, g4 = [torch.empty_like(q) for _ in range(4)]
        out, scratch, up = torch.empty(1, device="cuda"), torch.empty(B, device="cuda"), torch.ones(1, device="cuda")
        P = lambda t: t.data_ptr()  # noqa: E731
        calls_of = lambda lib: {  # noqa: E731
            "qst_margin_mse_loss_dot": lambda: lib.qst_margin_mse_loss(P(q), P(p), P(n), P(y), B, D, S.METRIC_DOT, 2, P(out),
                                                                       None, P(up), P(gq), P(gp), P(gn), P(scratch), st),
            "qst_margin_mse_loss_cos": lambda: lib.qst_margin_mse_loss(P(q), P(p), P(n), P(y), B, D, S.METRIC_COS_SIM, 2,
                                                                       P(out), None, P(up), P(gq), P(gp), P(gn), P(scratch), st),
            "qst_triplet_loss_cos": lambda: lib.qst_triplet_loss(P(q), P(p), P(n), B, D, S.METRIC_COS_DIST, 0.5, 2, P(out),
                                                                 P(up), P(gq), P(gp), P(gn), P(scratch), st),
            "qst_triplet_loss_l2": lambda: lib.qst_triplet_loss(P(q), P(p), P(n), B, D, S.METRIC_L2, 5.0, 2, P(out),
                                                                P(up), P(gq), P(gp), P(gn), P(scratch), st),
            "qst_embed_mse": lambda: lib.qst_embed_mse(P(q), P(p), B, D, P(out), P(up), P(gq), P(scratch), st),
            "qst_quadruplet_loss_p2_swap": lambda: lib.qst_quadruplet_loss(P(q), P(p), P(x4), P(n), B, D, 0.6, 1.0, 0.5, 0.5, 2.0,
                                                                           1, 2, P(out), P(up), P(gq), P(gp), P(g4), P(gn),
                                                                           P(scratch), st),
            "qst_pair_loss_contrastive_cos": lambda: lib.qst_pair_loss(P(q), P(p), P(y01), B, D, S.PAIR_CONTRASTIVE,
                                                                       S.METRIC_COS_DIST, 1.0, 2, P(out), P(up), P(gq), P(gp),
                                                                       P(scratch), st),
        }
        calls = [calls_of(lib) for lib in libs]
        side = 4 * (2 * B + 2)                          # per-row values written and read again, the result, grad_out
        nbytes = {k: 6 * B * D * 4 + side + (4 * B if "margin" in k else 0) for k in calls[0]}
        nbytes["qst_embed_mse"] = 3 * B * D * 4 + side
        nbytes["qst_quadruplet_loss_p2_swap"] = 8 * B * D * 4 + side
        nbytes["qst_pair_loss_contrastive_cos"] = 4 * B * D * 4 + side + 4 * B
        for c in calls:                                 # warm-up: code objects, clocks
            for fn in c.values():
                for _ in range(20):
                    assert fn() == 0
        torch.cuda.synchronize()
        times = [{k: [] for k in c} for c in calls]
        for r in range(args.repeats):
            order = list(range(len(libs)))
            order = order[r % len(libs):] + order[:r % len(libs)]      # which build goes first turns with the repeat
            for k in calls[0]:                          # alternated: drift of the box hits all of them alike
                for i in order:
                    fn = calls[i][k]
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.inner):
                        fn()
                    e1.record()
                    e1.synchronize()
                    times[i][k].append(e0.elapsed_time(e1) * 1e3 / args.inner)
        for i in range(len(libs)):
            for k in calls[i]:
                q1, med, q3 = statistics.quantiles(times[i][k], n=4)
                rows[i].append({"call": k, "B": B, "D": D, "bytes": nbytes[k], "median_us": round(med, 3),
                                "quartiles_us": [round(q1, 3), round(med, 3), round(q3, 3)],
                                "achieved_TB_per_s": round(nbytes[k] / (med * 1e-6) / 1e12, 3)})
                print(json.dumps(dict(rows[i][-1], build=i)))
    for i in range(len(libs)):
        res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "inner_launches_per_repeat": args.inner,
               "builds_alternated_in_this_process": len(libs),
               "what": "median microseconds of one call with gradients (row kernel + one-workgroup second stage), device "
                       "events around INNER calls, calls (and builds) alternated repeat by repeat; bytes = rows read once + "
                       "gradients written once + the [B] side arrays", "rows": rows[i]}
        if args.out:
            with open(args.out[i], "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
