#!/usr/bin/env python3
"""The weight gradients of TWO layers: two four-problem launches of qst_gemm_tn_group against one eight-problem launch, in ONE
process, alternated, best of three (DESIGN.md finding 48).
usage: ab_wgrad_pairs.py [--H 384,768] [--M 8192,16384,32768] [--skew=-1,1,2,3]
--skew: QstTnGroup.skew of the paired launch (-1 = equal ranges, 0 = the library's choice); the two single launches always run
at the library's choice. Each layer has its own operands and outputs, as in a backward."""
import argparse
import os
import sys
from dataclasses import replace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quadruplet_sentence_transformer_amd  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import _lib  # noqa: E402
from quadruplet_sentence_transformer_amd.config import PRESETS  # noqa: E402
from ab_wgrad import ints, timeit  # noqa: E402
from one_wgrad import make_group  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=ints, default=[384])
    ap.add_argument("--M", type=ints, default=[32768])
    ap.add_argument("--skew", type=ints, default=[0])
    a = ap.parse_args()
    lib, st = _lib.load(), _lib.current_stream_ptr()
    for H in a.H:
        for M in a.M:
            (g0, keep0, flops), (g1, keep1, _) = make_group(M=M, H=H, I=4 * H), make_group(M=M, H=H, I=4 * H)
            pair = _lib.QstTnGroup()
            pair.nprob, pair.splits = 8, 0
            for i in range(4):
                pair.prob[i], pair.prob[4 + i] = g1.prob[i], g0.prob[i]
            cfg = _lib.make_config(replace(PRESETS["all-MiniLM-L6-v2"], hidden_size=H, intermediate_size=4 * H, num_heads=H // 32))
            tiles = [lib.qst_wgrad_tiles(cfg, M, k) for k in (1, 2)]

            def singles():
                _lib.check(lib.qst_gemm_tn_group(g1, st))
                _lib.check(lib.qst_gemm_tn_group(g0, st))

            for skew in a.skew:
                pair.skew = skew
                best = [1e9, 1e9]
                for _ in range(3):
                    best[0] = min(best[0], timeit(singles))
                    best[1] = min(best[1], timeit(lambda: _lib.check(lib.qst_gemm_tn_group(pair, st))))
                print(f"H={H} M={M} tiles {tiles[0]} x 2 / {tiles[1]}  pair skew={skew:2d}: two launches {best[0]:7.1f} us "
                      f"({2 * flops / best[0] / 1e6:6.1f} TF)   one launch {best[1]:7.1f} us ({2 * flops / best[1] / 1e6:6.1f} TF)   "
                      f"({best[1] / best[0] - 1:+.1%})", flush=True)
            del keep0, keep1


if __name__ == "__main__":
    main()
