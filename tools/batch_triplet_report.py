"""qst_batch_triplet_loss against the fp64 CPU reference, per loss, metric and shape: the share of the value tolerance and
of the gradient tolerance that the kernels use, and whether the counts are equal (tests/batch_triplet_helpers.py holds the
recipe, the tie-free seed search, the reference and the tolerances; tests/test_gpu_batch_triplet.py asserts them on the
same cases). Needs a HIP device.

    python tools/batch_triplet_report.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import batch_triplet_helpers as T  # noqa: E402
from quadruplet_sentence_transformer_amd import st_losses as S  # noqa: E402


def row(name, x, labels, loss, grad, counts, kind, metric, seed_k):
    out, g, c = S.batch_triplet_loss_raw(x.cuda(), labels.cuda(), kind, metric, T.MARGIN[metric], want_grads=True)
    ev = T.value_error(out.item(), loss, metric, x.shape[1])
    eg = T.grad_error(g.cpu(), grad)
    print(f"  {T.KIND_NAMES[kind]:>4} {T.METRIC_NAMES[metric]:>6} {name:>10} {seed_k:>4}   {ev:7.3f} {eg:7.3f}   "
          f"{'equal' if c.tolist() == list(counts) else 'DIFFER'} {list(counts)}")
    return ev, eg


def main():
    print(f"# qst_batch_triplet_loss vs the fp64 CPU reference, margin {T.MARGIN[T.EUCLID]:g}; device {torch.cuda.get_device_name(0)}")
    print("# share of the tolerance used (1.00 = at the tolerance): value rtol = atol = max(1e-5, 1.5e-8 D); gradient rtol 1e-4,")
    print("# atol 1e-6 max(1, max |reference|). k: the seed 1000 B + D + 7919 k, the first whose every mining decision is >= 1e-5")
    print("# from flipping. counts: {terms of the denominator's population, terms > 0}.")
    print(f"# {'loss':>4} {'metric':>6} {'B x D':>10} {'k':>4}   {'value':>7} {'grad':>7}   counts")
    top_v = top_g = 0.0
    for kind in T.KINDS:
        for metric in T.METRICS:
            for (B, D) in T.shapes_of(kind):
                x, labels, loss, grad, counts, k = T.reference(B, D, kind, metric)
                ev, eg = row(f"{B}x{D}", x, labels, loss, grad, counts, kind, metric, k)
                top_v, top_g = max(top_v, ev), max(top_g, eg)
            if kind in T.BIG_KINDS:
                x, labels, loss, grad, counts = T.big_reference(kind, metric)
                ev, eg = row("%dx%d" % T.BIG, x, labels, loss, grad, counts, kind, metric, "-")
                top_v, top_g = max(top_v, ev), max(top_g, eg)
    print(f"# largest share: value {top_v:.3f}, gradient {top_g:.3f}")


if __name__ == "__main__":
    main()
