#!/usr/bin/env python3
"""A/B two builds of libqst.so on the grouped wgrad launch (MiniLM and mpnet layer shapes) in ONE process.
usage: ab_wgrad.py old.so [new.so] [--skew S[,S...]] [--order O[,O...]] [--H 384,768] [--M 32768]
--skew / --order (QstTnGroup.skew / .order; a library built before them ignores the fields): every combination is timed
against old.so at the library's default; without them one row per H at the library's choice."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quadruplet_sentence_transformer_amd  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import _lib  # noqa: E402
from one_wgrad import make_group  # noqa: E402


def bind(path):
    lib = C.CDLL(path)
    res, args = _lib.SIGNATURES["qst_gemm_tn_group"]
    lib.qst_gemm_tn_group.restype, lib.qst_gemm_tn_group.argtypes = res, args
    return lib


def timeit(fn, reps=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def ints(s):
    return [int(x) for x in s.split(",")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new", nargs="?", default=_lib.LIB_PATH)
    ap.add_argument("--skew", type=ints, default=[0])
    ap.add_argument("--order", type=ints, default=[0])
    ap.add_argument("--H", type=ints, default=[384, 768])
    ap.add_argument("--M", type=int, default=32768)
    a = ap.parse_args()
    libs = [bind(os.path.abspath(a.old)), bind(os.path.abspath(a.new))]
    st = _lib.current_stream_ptr()
    for H in a.H:
        grp, keep, flops = make_group(M=a.M, H=H, I=4 * H)
        for skew in a.skew:
            for order in a.order:
                best = [1e9, 1e9]
                for _ in range(3):
                    for i, lib in enumerate(libs):
                        grp.skew, grp.order = (skew, order) if i == 1 else (0, 0)
                        best[i] = min(best[i], timeit(lambda: _lib.check(lib.qst_gemm_tn_group(grp, st))))
                print(f"H={H} skew={skew} order={order}: old {best[0]:7.1f} us ({flops / best[0] / 1e6:6.1f} TF)   "
                      f"new {best[1]:7.1f} us ({flops / best[1] / 1e6:6.1f} TF)   ({best[1] / best[0] - 1:+.1%})", flush=True)


if __name__ == "__main__":
    main()
