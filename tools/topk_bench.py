#!/usr/bin/env python3
"""Time libqst's retrieval scoring (normalise + split-bf16 x3 GEMM + radix-select top-k) at the reference's evaluation
shape (corpus_chunk_size 50000, training/main.py:178) against torch (cos_sim + topk), yardstick only.

--stream CHUNK (repeatable) times the streaming path instead (util.topk_stream: the same scoring, merged chunk by chunk
into a running top-k) beside util.topk_scores where that can run the size, and prints one JSON line per measurement:
    tools/topk_bench.py --stream 16384 --stream 65536 --stream 262144 --nq 2048 --nc 262144 --dim 384 --k 10 --k 100
Medians of --repeats timed calls after --warmup untimed ones, each call between two events on the stream, the variants
in turn within every repeat."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quadruplet_sentence_transformer_amd  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import _lib, util  # noqa: E402


def timeit(fn, reps=5):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def time_call(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stream_bench(args):
    """Per k: the variants (topk_scores where it runs the size, topk_stream per chunk) are warmed up, then timed in turn
    within every repeat, so that drift of the machine falls on all of them alike."""
    lib = _lib.load()
    nq, nc, dim = args.nq, args.nc, args.dim
    q = torch.randn(nq, dim, device="cuda")
    c = torch.randn(nc, dim, device="cuda")
    base = dict(nq=nq, nc=nc, dim=dim, mode="cos", warmup=args.warmup, repeats=args.repeats,
                device=torch.cuda.get_device_name(0))
    for k in args.k:
        variants = []                                      # (row, fn)
        try:
            util.topk_scores(q, c, k, mode="cos")
            variants.append((dict(base, path="qst_topk_scores", k=k,
                                  workspace_bytes=int(lib.qst_topk_workspace_bytes(nq, nc, dim))),
                             lambda: util.topk_scores(q, c, k, mode="cos")))
        except _lib.QstError as e:
            print(json.dumps(dict(base, path="qst_topk_scores", k=k, error=str(e))), flush=True)
        for chunk in args.stream:
            ch = min(chunk, nc)
            variants.append((dict(base, path="qst_topk_stream", k=k, chunk=ch,
                                  workspace_bytes=int(lib.qst_topk_stream_workspace_bytes(nq, ch, dim))),
                             lambda ch=ch: util.topk_stream(q, c, k, mode="cos", chunk=ch)))
        for _ in range(args.warmup):
            for _, fn in variants:
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in variants]
        for _ in range(args.repeats):
            for t, (_, fn) in zip(times, variants):
                t.append(time_call(fn))
        parent = statistics.median(times[0]) if variants[0][0]["path"] == "qst_topk_scores" else None
        for t, (row, _) in zip(times, variants):
            row.update(ms_median=round(statistics.median(t), 3), ms_min=round(min(t), 3), ms_max=round(max(t), 3))
            if parent and row["path"] == "qst_topk_stream":
                row["vs_topk_scores"] = round(statistics.median(t) / parent, 4)
            print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--stream", type=int, action="append", metavar="CHUNK",
                    help="time util.topk_stream at this chunk size (repeatable) against util.topk_scores")
    ap.add_argument("--nq", type=int, default=2048)
    ap.add_argument("--nc", type=int, default=262144)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--k", type=int, action="append")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    if args.stream:
        args.k = args.k or [10, 100]
        stream_bench(args)
        return
    for nq, nc, dim, k in [(1000, 50000, 384, 100), (4096, 50000, 768, 100)]:
        q = torch.randn(nq, dim, device="cuda")
        c = torch.randn(nc, dim, device="cuda")
        t_qst = timeit(lambda: util.topk_scores(q, c, k, cosine=True))
        t_torch = timeit(lambda: torch.topk(util.cos_sim(q, c), k, dim=1))
        print(f"nq={nq} nc={nc} dim={dim} k={k}: libqst {t_qst:.2f} ms   torch fp32 matmul + topk {t_torch:.2f} ms")


if __name__ == "__main__":
    main()
