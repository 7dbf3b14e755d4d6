#!/usr/bin/env python
"""One SHA-256 per case over the raw bytes of everything the row-wise loss entry points write (csrc/loss.hip,
csrc/tuple_loss.hip, csrc/distill.hip): qst_quadruplet_loss, qst_pair_metric, qst_pair_loss, qst_triplet_loss,
qst_quadruplet_eval, qst_embed_mse, qst_margin_mse_loss. Seeded inputs; every output goes into the hash: loss, per-row values,
margins, distances, flags, counts, all gradients. Two builds that print the same file compute the same bits.

The tool goes through the *_raw wrappers only, so it depends on nothing but the C ABI: --lib points it at another build of
libqst.so (say, one of the parent commit) and the same file runs against that.

Grid: B 1, 5, 1025; D on both sides of every edge between two forms of the kernels; forward only and with gradients; every
reduction, metric and kind an entry point takes; p = 1, 2, 3 and swap off / on for the quadruplet loss; every tensor
aligned, then each row input in turn viewed one float into its storage (the element-by-element form); the passes of a
case go into one hash.

--group folds the 5,292 case lines into one line per shape and entry point (294): the SHA-256 over the case hashes of
the group, in order. That is the form kept under profiles/; where a group differs between two builds, the run without
--group names the cases.

    python tools/row_loss_digest.py --group --out profiles/row_loss_digest_after.txt
"""
import argparse
import hashlib
import itertools
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quadruplet_sentence_transformer_amd  # noqa: E402,F401
from quadruplet_sentence_transformer_amd import _lib, losses as Q, st_losses as S  # noqa: E402

BS = [1, 5, 1025]
DS = [1, 33, 64, 252, 256, 260, 384, 768, 1024, 1028, 2048, 2050, 2052, 5120]
DIST = [S.METRIC_COS_DIST, S.METRIC_L2, S.METRIC_L1]


def absorb(h, *outs):
    for t in outs:
        for x in (t if isinstance(t, (list, tuple)) else [t]):
            if x is not None:
                h.update(x.detach().cpu().contiguous().numpy().tobytes())


def grouped(lines):
    """One line per (B, D, entry point): the SHA-256 over the hex digests of its case lines, in the order they were printed."""
    groups = {}
    for line in lines:
        f = line.split()
        groups.setdefault(" ".join(f[:3]), hashlib.sha256()).update(f[-1].encode())
    return [f"{k} cases={sum(1 for l in lines if l.startswith(k + ' '))} {h.hexdigest()}" for k, h in groups.items()]


def margin_for(metric, D):
    """a hinge that is active for about half of the rows of unit-normal inputs"""
    return {S.METRIC_COS_DIST: 1.0, S.METRIC_L2: math.sqrt(2.0 * D), S.METRIC_L1: 1.128 * D}[metric]


def cases(B, D, lab01, labf, up_b, up_1):
    """(name, callable over the four row tensors' current views) of every case at one shape"""
    out = []
    for grads in (False, True):
        g = int(grads)
        up = lambda red: (up_b if red == 0 else up_1) if grads else None  # noqa: E731
        for red, p, swap in itertools.product(range(3), (1.0, 2.0, 3.0), (0, 1)):
            out.append((f"quadruplet_loss red={red} p={p:g} swap={swap} grads={g}", 4,
                        lambda v, red=red, p=p, swap=swap: Q._launch(v, (0.6, 1.0, 0.5, 0.5, p, swap), red, up(red), grads)))
        for metric in range(7):
            out.append((f"pair_metric metric={metric} grads={g}", 2,
                        lambda v, metric=metric: S.pair_metric_raw(v[0], v[1], metric, up(0), grads)))
        kinds = [(S.PAIR_MSE, S.METRIC_COS_SIM)] + [(k, m) for k in (S.PAIR_CONTRASTIVE, S.PAIR_ONLINE_CONTRASTIVE) for m in DIST]
        for (kind, metric), red in itertools.product(kinds, range(3)):
            margin = 0.5 if kind == S.PAIR_MSE else margin_for(metric, D)
            u = up(red if kind != S.PAIR_ONLINE_CONTRASTIVE else 1)
            out.append((f"pair_loss kind={kind} metric={metric} red={red} grads={g}", 2,
                        lambda v, kind=kind, metric=metric, red=red, margin=margin, u=u:
                        S.pair_loss_raw(v[0], v[1], lab01, kind, metric, margin, red, u, grads)))
        for metric, red in itertools.product(DIST, range(3)):
            margin = 0.1 * margin_for(metric, D)
            out.append((f"triplet_loss metric={metric} red={red} grads={g}", 3,
                        lambda v, metric=metric, red=red, margin=margin:
                        S.triplet_loss_raw(v[0], v[1], v[2], metric, margin, red, up(red), grads)))
        out.append((f"quadruplet_eval dist={g}", 4, lambda v: S.quadruplet_eval_raw(v[0], v[1], v[2], v[3], want_dist=grads)))
        out.append((f"embed_mse grads={g}", 2, lambda v: S.embed_mse_raw(v[0], v[1], up(1), grads)))
        for sim, red in itertools.product((S.METRIC_DOT, S.METRIC_COS_SIM), range(3)):
            out.append((f"margin_mse sim={sim} red={red} grads={g}", 3,
                        lambda v, sim=sim, red=red: S.margin_mse_raw(v[0], v[1], v[2], labf, sim, red, up(red), grads, True)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libqst.so to load instead of the tree's")
    ap.add_argument("--out", default=None)
    ap.add_argument("--group", action="store_true", help="one line per shape and entry point instead of one per case")
    args = ap.parse_args()
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    assert torch.cuda.is_available(), "this tool needs a HIP device"
    _lib.load()
    lines = []
    for B, D in itertools.product(BS, DS):
        gen = torch.Generator().manual_seed(1000 * B + D)
        host = [torch.randn(B, D, generator=gen) for _ in range(4)]
        aligned = [h.cuda() for h in host]
        # the same values one float into a storage of their own: 4 bytes past torch's allocation alignment
        shifted = []
        for h in host:
            flat = torch.empty(B * D + 1, device="cuda")
            flat[1:].copy_(h.reshape(-1))
            shifted.append(flat[1:].view(B, D))
        lab01 = (torch.rand(B, generator=gen) < 0.5).float().cuda()
        labf = torch.randn(B, generator=gen).cuda()
        up_b, up_1 = (0.5 + torch.rand(B, generator=gen)).cuda(), (0.5 + torch.rand(1, generator=gen)).cuda()
        for name, nx, fn in cases(B, D, lab01, labf, up_b, up_1):
            h = hashlib.sha256()                 # one hash per case over its alignment passes, to keep the file small
            for off in range(-1, nx):            # -1: every tensor aligned; k: input k at the offset
                absorb(h, *fn([shifted[k] if k == off else aligned[k] for k in range(nx)]))
            lines.append(f"B={B} D={D} {name} {h.hexdigest()}")
        print(f"B={B} D={D}: {len(lines)} cases so far", file=sys.stderr, flush=True)
    text = "\n".join(grouped(lines) if args.group else lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
