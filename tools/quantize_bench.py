"""The quantized searches (csrc/quantize.hip) next to the fp32 streaming top-k on the same device, which must be otherwise
idle: util.hamming_topk on packed sign bits, util.int8_topk on int8 codes and util.topk_stream(mode="dot") on the fp32 rows
they were made from, at 2,048 queries x 262,144 corpus rows, dim 384 and 1,024, k 10 and 100, each at chunk 16,384 / 65,536 /
262,144. All in one process, the three alternated repeat by repeat, each repeat between two synchronisations, the median
after a warm-up. Also: the device bytes of each form of the corpus, quantize_embeddings of the corpus, and
semantic_search_quantized(rescore=True) end to end (float queries in, Python lists out) next to util.semantic_search.
No ratio is promised: what is measured is what is written. Writes profiles/quantize_bench.json.

    python tools/quantize_bench.py [--repeats 30] [--warmup 5] [--out profiles/quantize_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import _lib, quantization, util  # noqa: E402

NQ, NC = 2048, 262144
DIMS = (384, 1024)
KS = (10, 100)
CHUNKS = (16384, 65536, 262144)


def timed_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def medians(fns, warmup, repeats):
    """{name: (median, min, max)} of the callables, alternated repeat by repeat."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    times = {name: [] for name in fns}
    for _ in range(repeats):
        for name, f in fns.items():
            times[name].append(timed_ms(f))
    return {name: (round(statistics.median(t), 4), round(min(t), 4), round(max(t), 4)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantize_bench.json"))
    ap.add_argument("--once", action="store_true", help="one call of each search at dim 1024, k 10, the default chunk (for a profiler)")
    args = ap.parse_args()
    lib = _lib.load()
    searches, corpora, end_to_end = [], [], []
    for dim in DIMS if not args.once else (1024,):
        g = torch.Generator(device="cuda").manual_seed(dim)
        corpus = torch.randn(NC, dim, generator=g, device="cuda")
        queries = (corpus[torch.randperm(NC, generator=g, device="cuda")[:NQ]] + 0.1 * torch.randn(NQ, dim, generator=g, device="cuda"))
        ranges = quantization.column_ranges(corpus)
        c_bits = quantization.quantize_embeddings(corpus, "ubinary")
        q_bits = quantization.quantize_embeddings(queries, "ubinary")
        c_i8 = quantization.quantize_embeddings(corpus, "int8", ranges=ranges)
        q_i8 = quantization.quantize_embeddings(queries, "int8", ranges=ranges)
        if args.once:
            util.hamming_topk(q_bits, c_bits, 10)
            util.int8_topk(q_i8, c_i8, 10)
            util.topk_stream(queries, corpus, 10, mode="dot")
            quantization.semantic_search_quantized(queries, c_bits, "ubinary", top_k=10)
            torch.cuda.synchronize()
            return
        q_times = medians({"ubinary": lambda: quantization.quantize_embeddings(corpus, "ubinary"),
                           "int8": lambda: quantization.quantize_embeddings(corpus, "int8", ranges=ranges),
                           "column_ranges": lambda: quantization.column_ranges(corpus)}, args.warmup, args.repeats)
        row = {"dim": dim, "rows": NC,
               "bytes_fp32": corpus.numel() * corpus.element_size(), "bytes_int8": c_i8.numel() * c_i8.element_size(),
               "bytes_ubinary": c_bits.numel() * c_bits.element_size(),
               **{f"quantize_{n}_ms": t[0] for n, t in q_times.items()}}
        print(json.dumps(row), flush=True)
        corpora.append(row)
        for k in KS:
            for chunk in CHUNKS:
                t = medians({"hamming_topk": lambda: util.hamming_topk(q_bits, c_bits, k, chunk=chunk),
                             "int8_topk": lambda: util.int8_topk(q_i8, c_i8, k, chunk=chunk),
                             "topk_stream_dot": lambda: util.topk_stream(queries, corpus, k, mode="dot", chunk=chunk)},
                            args.warmup, args.repeats)
                row = {"nq": NQ, "nc": NC, "dim": dim, "k": k, "chunk": chunk}
                for name, (med, lo, hi) in t.items():
                    row[f"{name}_ms"] = med
                    row[f"{name}_ms_min_max"] = [lo, hi]
                row["fp32_over_hamming"] = round(t["topk_stream_dot"][0] / t["hamming_topk"][0], 3)
                row["fp32_over_int8"] = round(t["topk_stream_dot"][0] / t["int8_topk"][0], 3)
                print(json.dumps(row), flush=True)
                searches.append(row)
        t = medians({"quantized_ubinary": lambda: quantization.semantic_search_quantized(queries, c_bits, "ubinary", top_k=10),
                     "quantized_int8": lambda: quantization.semantic_search_quantized(queries, c_i8, "int8", top_k=10, ranges=ranges),
                     "semantic_search_fp32": lambda: util.semantic_search(queries, corpus, top_k=10, score_function=util.dot_score)},
                    args.warmup, args.repeats)
        row = {"nq": NQ, "nc": NC, "dim": dim, "top_k": 10, "rescore_multiplier": 4,
               "what": "float queries in, Python result lists out; the corpus already quantized",
               **{f"{n}_ms": v[0] for n, v in t.items()}, **{f"{n}_ms_min_max": [v[1], v[2]] for n, v in t.items()}}
        print(json.dumps(row), flush=True)
        end_to_end.append(row)
        del corpus, queries, c_bits, q_bits, c_i8, q_i8
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "qst_version": lib.qst_version(), "repeats": args.repeats, "warmup": args.warmup,
           "what": "median ms per call, one process, alternated; chunks 16,384 / 65,536 / 262,144 for all three searches",
           "stream_chunk_default": quantization.STREAM_CHUNK, "corpora": corpora, "searches": searches, "end_to_end": end_to_end}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
