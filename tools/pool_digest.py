#!/usr/bin/env python
"""One SHA-256 per case over the raw bytes of everything a pooling forward + backward writes (csrc/rowops.hip behind
qst_pool_fwd / qst_pool_bwd): emb, pooled, argmax where the head has max, dtok. The cases, their integer-built inputs and the
pre-filled outputs are tests/pool_digest_cases.py; two builds that give the same file compute the same bits.

The tool binds the two entry points itself, so it depends on nothing but the C ABI: --lib points it at another build of
libqst.so (say, one of the parent commit). A build that still exports qst_pool_norm_fwd / qst_pool_norm_bwd (the mean-only
pair before version 114) has its mean cases run through those two, every other case through qst_pool_fwd / qst_pool_bwd.

    python tools/pool_digest.py --lib OLD/libqst.so --commit HASH --out tests/golden/pool_digests.json     # record
    python tools/pool_digest.py --check tests/golden/pool_digests.json                                     # the tree's build
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pool_digest_cases as P  # noqa: E402

vp, ci = C.c_void_p, C.c_int


def bind(path):
    """(fwd, bwd, which) with the argument lists of qst_pool_fwd / qst_pool_bwd; mean cases go to the old pair where it exists."""
    lib = C.CDLL(path)
    lib.qst_pool_fwd.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp]
    lib.qst_pool_bwd.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, vp]
    old = hasattr(lib, "qst_pool_norm_fwd") and hasattr(lib, "qst_pool_norm_bwd")
    if old:
        lib.qst_pool_norm_fwd.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, vp]
        lib.qst_pool_norm_bwd.argtypes = [vp, vp, vp, ci, ci, ci, ci, vp, vp]

    def fwd(tok, mask, n, L, H, mode, normalize, emb, pooled, argmax, stream):
        if old and mode == P.MEAN:
            return lib.qst_pool_norm_fwd(tok, mask, n, L, H, normalize, emb, pooled, stream)
        return lib.qst_pool_fwd(tok, mask, n, L, H, mode, normalize, emb, pooled, argmax, stream)

    def bwd(demb, pooled, argmax, mask, n, L, H, mode, normalize, dtok, stream):
        if old and mode == P.MEAN:
            return lib.qst_pool_norm_bwd(demb, pooled, mask, n, L, H, normalize, dtok, stream)
        return lib.qst_pool_bwd(demb, pooled, argmax, mask, n, L, H, mode, normalize, dtok, stream)

    return fwd, bwd, lib.qst_version(), old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "quadruplet-sentence-transformer_amd", "libqst.so"))
    ap.add_argument("--commit", default=None, help="the commit --lib was built from (recorded in --out)")
    ap.add_argument("--out", default=None, help="write the digests as JSON")
    ap.add_argument("--check", default=None, help="compare with a recorded JSON; exit status 1 on any difference")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool needs a HIP device"
    fwd, bwd, version, old = bind(os.path.abspath(args.lib))
    rec = {"commit": args.commit, "qst_version": version, "mean_cases_through": "qst_pool_norm_fwd/bwd" if old else "qst_pool_fwd/bwd",
           "cases": {}}
    want = json.load(open(args.check))["cases"] if args.check else None
    bad = 0
    for H, L, mode, normalize in P.CASES:
        name = P.case_name(H, L, mode, normalize)
        d = rec["cases"][name] = P.run_case(fwd, bwd, H, L, mode, normalize)
        verdict = ""
        if want is not None:
            verdict = " | same" if want.get(name) == d else " | DIFFERENT"
            bad += want.get(name) != d
        print(name + " | " + " ".join(f"{k} {v[:16]}" for k, v in d.items()) + verdict, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    if want is not None:
        bad += len(set(want) - set(rec["cases"]))
        print(f"{len(rec['cases'])} cases, {bad} different from {args.check}")
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
