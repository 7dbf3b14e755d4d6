#!/usr/bin/env python3
"""Time util.community_detection (count pass + member rounds + claim, no n x n matrix) on planted data, and the only
yardstick there is: the full score matrix (util.cos_sim) + torch ops the way sentence-transformers 2.2.2 does them, at
the largest n where that matrix fits. One JSON line, printed and appended to --out:
    tools/community_bench.py --n 262144 --dim 384 --upstream-n 32768
The line holds the end-to-end seconds, the count pass, every round (candidates, members, row blocks, seconds of the member
pass and of claim + copy-back), and the time of one [2048, chunk] x3 GEMM panel times the number of panels, which splits
the count pass into scoring and counting. Planted data: clusters of rows of +-1 around random centres (up to --flips
signs flipped) and as many random rows; the threshold takes rows that differ in at most --flips places."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quadruplet_sentence_transformer_amd  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import _lib, util  # noqa: E402


def planted(n, dim, cluster, flips, seed):
    """[n, dim] rows of +-1 on the device: n / (2 cluster) clusters of `cluster` rows, the rest random, permuted."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    ncl = max(1, n // (2 * cluster))
    sign = lambda *shape: torch.randint(0, 2, shape, generator=g, device="cuda", dtype=torch.float32) * 2 - 1  # noqa: E731
    rows = sign(ncl, dim).repeat_interleave(cluster, dim=0)[:n]
    nflip = torch.randint(1, flips + 1, (len(rows), 1), generator=g, device="cuda")
    rank = torch.rand(len(rows), dim, generator=g, device="cuda").argsort(dim=1).argsort(dim=1)
    rows = torch.where(rank < nflip, -rows, rows)
    e = torch.cat([rows, sign(n - len(rows), dim)])
    return e[torch.randperm(n, generator=g, device="cuda")].contiguous()


def upstream_like(e, threshold, min_community_size, init_max_size=1000):
    """sentence-transformers 2.2.2's procedure on the full matrix: topk(min size) per row to find the candidates, a
    topk(init_max_size) or a full row scan per candidate, a host sort by size and the greedy pass over Python sets."""
    cos = util.cos_sim(e, e)
    top, _ = cos.topk(k=min_community_size, largest=True)
    extracted = []
    for i in torch.nonzero(top[:, -1] >= threshold).flatten().tolist():
        val, idx = cos[i].topk(k=min(init_max_size, cos.shape[1]), largest=True)
        if val[-1] < threshold:
            extracted.append(idx[val >= threshold].tolist())
        else:
            extracted.append(torch.nonzero(cos[i] >= threshold).flatten().tolist())
    extracted.sort(key=len, reverse=True)
    unique, seen = [], set()
    for c in extracted:
        if not any(j in seen for j in c):
            unique.append(c)
            seen.update(c)
    return unique


def panel_ms(lib, rows, chunk, dim, reps=20):
    """Median milliseconds of one [rows, chunk] x3 GEMM panel on normalised rows."""
    a = torch.nn.functional.normalize(torch.randn(rows, dim, device="cuda"))
    b = torch.nn.functional.normalize(torch.randn(chunk, dim, device="cuda"))
    c = torch.empty(rows, chunk, device="cuda")
    g = _lib.QstGemmArgs()
    g.A, g.B, g.C = a.data_ptr(), b.data_ptr(), c.data_ptr()
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc = rows, chunk, dim, dim, dim, chunk
    times = []
    for r in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.qst_gemm_nt_x3(g, 0, _lib.current_stream_ptr()), "qst_gemm_nt_x3")
        e1.record()
        e1.synchronize()
        if r >= 3:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--cluster", type=int, default=512)
    ap.add_argument("--flips", type=int, default=40)
    ap.add_argument("--min-size", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=util.STREAM_CHUNK)
    ap.add_argument("--upstream-n", type=int, default=32768, help="rows of the full-matrix yardstick (0: skip it)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "community_bench.json"))
    args = ap.parse_args()
    lib = _lib.load()
    thr = 1.0 - (2 * args.flips + 1) / args.dim
    row = dict(n=args.n, dim=args.dim, cluster=args.cluster, flips=args.flips, threshold=round(thr, 6),
               min_community_size=args.min_size, chunk=min(args.chunk, args.n), device=torch.cuda.get_device_name(0),
               round_budget_members=util.COMMUNITY_ROUND_MEMBERS)
    e = planted(args.n, args.dim, args.cluster, args.flips, seed=7)
    chunk = min(args.chunk, args.n)
    row["workspace_bytes"] = int(lib.qst_community_workspace_bytes(args.n, chunk, args.dim))
    util.community_detection(e[:4096], thr, args.min_size)                   # warm-up: library load, allocator
    row["total_s"], out = wall(lambda: util.community_detection(e, thr, args.min_size, corpus_chunk_size=chunk))
    row["communities"] = len(out)
    row["clustered_rows"] = sum(len(c) for c in out)
    stats = {}
    row["total_s_with_stage_syncs"], _ = wall(lambda: util._community_detection(e, thr, args.min_size, chunk, stats=stats))
    row["count_s"] = round(stats["count_s"], 4)
    row["rounds"] = [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()} for r in stats["rounds"]]
    pm = panel_ms(lib, min(2048, args.n), chunk, args.dim)
    panels = -(-args.n // 2048) * -(-args.n // chunk)
    row.update(panel_gemm_ms=round(pm, 4), panels_per_pass=panels, scoring_s_per_pass=round(pm * panels / 1e3, 4),
               panel_bytes=min(2048, args.n) * chunk * 4)
    if args.upstream_n:
        m = min(args.upstream_n, args.n)
        em = e[:m].contiguous()
        ours_s, ours = wall(lambda: util.community_detection(em, thr, args.min_size, corpus_chunk_size=chunk))
        up_s, up = wall(lambda: upstream_like(em, thr, args.min_size))
        row["yardstick"] = dict(n=m, community_detection_s=round(ours_s, 4), full_matrix_torch_s=round(up_s, 4),
                                same_communities=sorted(map(sorted, ours)) == sorted(map(sorted, up)),
                                matrix_bytes=m * ((m + 3) // 4 * 4) * 4)
    for k in ("total_s", "total_s_with_stage_syncs"):
        row[k] = round(row[k], 4)
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
