"""CoSENTLoss / AnglELoss on given embeddings: the kernel path (qst_cosent_loss through its autograd function: O(B) memory,
3 launches forward and 4 backward) next to the torch-op composition sentence-transformers runs (the pairwise score in torch
ops, the B x B differences, the mask, logsumexp, and autograd back through all of it), on the same device tensors.

    python tools/cosent_bench.py [--repeats 30] [--inner 20] [--out profiles/cosent_bench.json]
    python tools/cosent_bench.py --report [--out profiles/cosent_parity.txt]

The benchmark alternates the two paths repeat by repeat after a warm-up; a repeat is INNER forward + backward passes between
two device events, and the figures are the median and the quartiles over the repeats. The kernel path did not exist before
this file did, so the composed path is the yardstick. Peak device memory of one pass of each path is taken at the largest
shape. --report writes, per test case of tests/cosent_helpers.py, the share of the value, score and gradient tolerances
the kernel uses against the fp64 CPU reference.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import cosent_helpers as CH  # noqa: E402
from quadruplet_sentence_transformer_amd import st_losses as S  # noqa: E402

SHAPES = [(64, 384), (256, 768), (4096, 768)]


def kernel_pass(u, v, y, sim):
    u, v = u.detach().requires_grad_(True), v.detach().requires_grad_(True)
    S.cosent_loss(u, v, y, CH.SCALE, sim).backward()
    return u.grad, v.grad


def composed_pass(u, v, y, sim):
    u, v = u.detach().requires_grad_(True), v.detach().requires_grad_(True)
    S.cosent_loss_torch(CH.SIM_REF[sim](u, v), y, CH.SCALE).backward()
    return u.grad, v.grad


def timed(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / inner * 1e3           # microseconds a pass


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def bench(args):
    assert args.repeats >= 20, "at least 20 repeats"
    rows = []
    for B, D in SHAPES:
        for sim in CH.SIMS:
            u, v, y = [t.cuda() for t in CH.case(B, D, "graded")]
            gk, gc = kernel_pass(u, v, y, sim), composed_pass(u, v, y, sim)
            diff = max(CH.grad_error(a, b) for a, b in zip(gk, gc))
            for _ in range(3):
                timed(lambda: kernel_pass(u, v, y, sim), args.inner)
                timed(lambda: composed_pass(u, v, y, sim), args.inner)
            tk, tc = [], []
            for _ in range(args.repeats):
                tk.append(timed(lambda: kernel_pass(u, v, y, sim), args.inner))
                tc.append(timed(lambda: composed_pass(u, v, y, sim), args.inner))
            qk, qc = statistics.quantiles(tk, n=4), statistics.quantiles(tc, n=4)
            mk, mc = statistics.median(tk), statistics.median(tc)
            row = {"B": B, "D": D, "sim": sim, "kernel_us": round(mk, 2), "composed_us": round(mc, 2),
                   "kernel_quartiles_us": [round(x, 2) for x in qk], "composed_quartiles_us": [round(x, 2) for x in qc],
                   "composed_interquartile_us": round(qc[2] - qc[0], 2), "saved_us": round(mc - mk, 2),
                   "speedup": round(mc / mk, 3), "kernel_wins": bool(mc - mk > qc[2] - qc[0]),
                   "gradient_difference_share_of_tolerance": round(diff, 4)}
            if (B, D) == SHAPES[-1]:
                row["kernel_peak_bytes"] = peak_bytes(lambda: kernel_pass(u, v, y, sim))
                row["composed_peak_bytes"] = peak_bytes(lambda: composed_pass(u, v, y, sim))
            rows.append(row)
            print(json.dumps(row), flush=True)
    result = {
        "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "inner_passes_per_repeat": args.inner,
        "what": "median microseconds of one forward + backward of the CoSENT / AnglE loss on given fp32 embeddings (autograd, "
                "allocation of outputs and workspaces included); device events around INNER passes; the kernel path "
                "(qst_cosent_loss) and the torch-op composition alternated; peak bytes: device memory one pass allocates "
                "beyond its inputs",
        "rows": rows,
        "rule": "kernel_wins: kernel_us < composed_us - composed_interquartile_us",
    }
    with open(args.out or os.path.join(ROOT, "profiles", "cosent_bench.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def report(args):
    up = 1.7
    lines = [f"# qst_cosent_loss vs the fp64 CPU reference, scale {CH.SCALE:g}, grad_out {up}; device {torch.cuda.get_device_name(0)}",
             "# share of the tolerance used (1.00 = at the tolerance): values and scores rtol = atol = max(1e-5, 1.5e-8 D);",
             "# gradients rtol 1e-4, atol 1e-6 max(1, max |reference|). Maximum over the three label sets; worst gradient set named.",
             "#    B     D    sim      loss  scores  grad_u  grad_v   worst gradient set"]
    worst_v = worst_g = 0.0
    for B, D, sim in CH.cases():
        e, name = [0.0] * 4, ""
        for kind in CH.LABEL_SETS:
            u, v, y, loss, scores, gu, gv = CH.reference(B, D, sim, kind)
            out, sc, grads = S.cosent_loss_raw(u.cuda(), v.cuda(), y.cuda(), sim, CH.SCALE,
                                               grad_out=torch.tensor([up], device="cuda"), want_grads=True)
            got = [CH.value_error(out.item(), loss, D), CH.score_error(sc.cpu(), scores, D),
                   CH.grad_error(grads[0].cpu(), up * gu), CH.grad_error(grads[1].cpu(), up * gv)]
            if max(got[2:]) >= max(e[2:]):
                name = kind
            e = [max(a, b) for a, b in zip(e, got)]
        worst_v, worst_g = max(worst_v, e[0], e[1]), max(worst_g, e[2], e[3])
        lines.append(f"{B:6d} {D:5d} {sim:>6s}   {e[0]:7.3f} {e[1]:7.3f} {e[2]:7.3f} {e[3]:7.3f}   {name}")
    lines.append(f"# largest share: values and scores {worst_v:.3f}, gradients {worst_g:.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    with open(args.out or os.path.join(ROOT, "profiles", "cosent_parity.txt"), "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--report", action="store_true", help="write the parity report instead of the timings")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    (report if args.report else bench)(args)


if __name__ == "__main__":
    main()
