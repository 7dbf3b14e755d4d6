"""qst_mnrl_nested_loss against the fp64 CPU reference, per case: the largest share of the value tolerance (the loss and
every term) and of the gradient tolerance that the kernel uses over both losses and trained in {0, 1}
(tests/matryoshka_helpers.py holds the cases, the reference and the weights, tests/mnrl_helpers.py the tolerances;
tests/test_gpu_matryoshka.py asserts them on the listed cases). Needs a HIP device.

    python tools/matryoshka_report.py > profiles/matryoshka_parity.txt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import matryoshka_helpers as MH  # noqa: E402
import mnrl_helpers as M  # noqa: E402
from quadruplet_sentence_transformer_amd import st_losses as S  # noqa: E402

EXTRA = [(256, 512, 768, [768, 512, 256, 128, 64]), (64, 128, 384, [384, 256, 128, 64, 32])]     # the shapes of the bench tool


def main():
    print(f"# qst_mnrl_nested_loss vs the fp64 CPU reference, scale {MH.SCALE:g}, weights 1 / (k + 1); "
          f"device {torch.cuda.get_device_name(0)}")
    print("# share of the tolerance used (1.00 = at the tolerance): values rtol = atol = max(1e-5, 1.5e-8 D); gradients rtol 1e-4,")
    print("# atol 1e-6 max(1, max |reference|). Maximum over plain / symmetric and trained in (0, 1); worst gradient case named.")
    print(f"# {'B':>4} {'N':>5} {'D':>5}   {'loss':>7} {'terms':>7} {'grad_a':>7} {'grad_c':>7}   widths; worst gradient case")
    top_v = top_g = 0.0
    for (B, N, D, dims) in MH.CASES + EXTRA:
        ev = et = ea = ec = 0.0
        worst = ""
        for symmetric in (0, 1):
            for trained in (0, 1):
                a, c, loss, ref_terms, ga, gc, _ = MH.reference(B, N, D, dims, symmetric, trained)
                out, terms, grads = S.mnrl_nested_loss_raw(a.cuda(), c.cuda(), dims, MH.weights_of(dims), MH.SCALE, symmetric,
                                                           want_grads=True)
                v = M.value_error(out.item(), loss, D)
                t = max(M.value_error(x, y, D) for x, y in zip(terms.tolist(), ref_terms.tolist()))
                xa, xc = M.grad_error(grads[0].cpu(), ga), M.grad_error(grads[1].cpu(), gc)
                if max(xa, xc) > max(ea, ec):
                    worst = f"{'symmetric' if symmetric else 'plain'} trained={trained}"
                ev, et, ea, ec = max(ev, v), max(et, t), max(ea, xa), max(ec, xc)
        print(f"  {B:>4} {N:>5} {D:>5}   {ev:7.3f} {et:7.3f} {ea:7.3f} {ec:7.3f}   {dims}; {worst}")
        top_v, top_g = max(top_v, ev, et), max(top_g, ea, ec)
    print(f"# largest share: values {top_v:.3f}, gradients {top_g:.3f}")


if __name__ == "__main__":
    main()
