"""qst_mnrl_loss against the fp64 CPU reference, per shape: the largest share of the value tolerance and of the gradient
tolerance that the kernel uses over both similarity functions, both losses and trained in {0, 1} (tests/mnrl_helpers.py
holds the recipe, the reference and the tolerances; tests/test_gpu_mnrl.py asserts them on the listed shapes). Needs a
HIP device.

    python tools/mnrl_report.py > profiles/mnrl_parity.txt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import mnrl_helpers as M  # noqa: E402
from quadruplet_sentence_transformer_amd import st_losses as S  # noqa: E402

EXTRA = [(256, 768, 384), (512, 1024, 768)]     # training shapes past the test list


def main():
    print(f"# qst_mnrl_loss vs the fp64 CPU reference, scale {M.SCALE:g}; device {torch.cuda.get_device_name(0)}")
    print("# share of the tolerance used (1.00 = at the tolerance): value rtol = atol = max(1e-5, 1.5e-8 D); gradients rtol 1e-4,")
    print("# atol 1e-6 max(1, max |reference|). Maximum over sim in (cos, dot), plain / symmetric, trained in (0, 1); worst case named.")
    print(f"# {'B':>4} {'N':>5} {'D':>5}   {'value':>7} {'grad_a':>7} {'grad_c':>7}   worst gradient case")
    top_v = top_g = 0.0
    for (B, N, D) in M.SHAPES + EXTRA:
        ev = ea = ec = 0.0
        worst = ""
        for sim in ("cos", "dot"):
            for symmetric in (0, 1):
                for trained in (0, 1):
                    a, c, loss, ga, gc = M.reference(B, N, D, sim, symmetric, trained)
                    out, grads = S.mnrl_loss_raw(a.cuda(), c.cuda(), sim, M.SCALE, symmetric, want_grads=True)
                    v = M.value_error(out.item(), loss, D)
                    xa, xc = M.grad_error(grads[0].cpu(), ga), M.grad_error(grads[1].cpu(), gc)
                    if max(xa, xc) > max(ea, ec):
                        worst = f"{sim} {'symmetric' if symmetric else 'plain'} trained={trained}"
                    ev, ea, ec = max(ev, v), max(ea, xa), max(ec, xc)
        print(f"  {B:>4} {N:>5} {D:>5}   {ev:7.3f} {ea:7.3f} {ec:7.3f}   {worst}")
        top_v, top_g = max(top_v, ev), max(top_g, ea, ec)
    print(f"# largest share: value {top_v:.3f}, gradients {top_g:.3f}")


if __name__ == "__main__":
    main()
