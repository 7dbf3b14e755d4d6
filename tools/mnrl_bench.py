"""Time of one forward + backward call pair of qst_mnrl_loss (what the autograd Function of st_losses.py issues per
training step) next to the torch-op path -- fp32 F.normalize, mm, F.cross_entropy and autograd on the same tensors, same
GPU -- at training shapes, cos, plain and symmetric. The two are alternated repeat by repeat; a repeat is INNER pairs between
two full synchronisations (a single pair is tens of microseconds: shorter than the clock is good for), the figure is the
median over the repeats after a warm-up. Also: the call pair as a share of one bf16 training step of the tiny model the
fit tests train (measured here) and of the 4.5 ms MiniLM headline step. Writes profiles/mnrl_bench.json.

    python tools/mnrl_bench.py [--repeats 30] [--inner 50] [--out profiles/mnrl_bench.json]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import mnrl_helpers as M  # noqa: E402
from quadruplet_sentence_transformer_amd import data, st_losses as S  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample, SentenceTransformer  # noqa: E402

SHAPES = [(64, 64, 384), (64, 128, 384), (256, 512, 768), (512, 1024, 768)]
CONDITION_SHAPE = (64, 128, 384)        # one hard negative per anchor: the fused pair must not be slower than torch ops here
HEADLINE_STEP_MS = 4.5


def fused_pair(a, c, symmetric):
    S.mnrl_loss_raw(a, c, "cos", M.SCALE, symmetric)
    return S.mnrl_loss_raw(a, c, "cos", M.SCALE, symmetric, want_grads=True)[1]


def torch_pair(a, c, symmetric):
    a, c = a.detach().requires_grad_(True), c.detach().requires_grad_(True)
    M.mnrl_ref(a, c, "cos", M.SCALE, symmetric).backward()
    return [a.grad, c.grad]


def timed(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e6


def tiny_fit_step_ms(steps=40):
    """One bf16 fit() step of tiny-bert under MultipleNegativesRankingLoss, batches of 8 pairs (the fit test's set-up)."""
    random.seed(11)
    words = "a man rides red horse two dogs play in park woman eats green apple near old bridge small cat sleeps".split()
    pairs = [InputExample(texts=[" ".join(random.choices(words, k=9)) + f" {i}", " ".join(random.choices(words, k=9)) + f" now {i}"])
             for i in range(16)]
    m = SentenceTransformer("tiny-bert", device="cuda")
    lm = S.MultipleNegativesRankingLoss(m)
    kw = dict(warmup_steps=0, scheduler="constantlr", optimizer_params={"lr": 1e-4}, dropout=0, show_progress_bar=False)
    m.fit([(data.NoDuplicatesDataLoader(list(pairs), 8), lm)], epochs=2, **kw)       # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.fit([(data.NoDuplicatesDataLoader(list(pairs), 8), lm)], epochs=steps // 2, **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mnrl_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available() and args.repeats >= 20, "needs a HIP device and at least 20 repeats"
    rows = []
    for (B, N, D) in SHAPES + [(8, 8, 64)]:
        a, c = [t.cuda() for t in M.case(B, N, D, "cos", 1, 1000 * B + D)]
        for symmetric in (0, 1):
            gf, gt = fused_pair(a, c, symmetric), torch_pair(a, c, symmetric)
            diff = max((x - y).abs().max().item() for x, y in zip(gf, gt))
            for _ in range(3):
                timed(lambda: fused_pair(a, c, symmetric), args.inner)
                timed(lambda: torch_pair(a, c, symmetric), args.inner)
            tf, tt = [], []
            for _ in range(args.repeats):
                tf.append(timed(lambda: fused_pair(a, c, symmetric), args.inner))
                tt.append(timed(lambda: torch_pair(a, c, symmetric), args.inner))
            q = lambda xs: [round(v, 2) for v in statistics.quantiles(xs, n=4)]  # noqa: E731
            rows.append({"B": B, "N": N, "D": D, "symmetric": bool(symmetric), "fused_pair_us": round(statistics.median(tf), 2),
                         "torch_ops_us": round(statistics.median(tt), 2), "fused_quartiles_us": q(tf), "torch_quartiles_us": q(tt),
                         "speedup": round(statistics.median(tt) / statistics.median(tf), 3),
                         "max_abs_gradient_difference": diff})
            print(json.dumps(rows[-1]), flush=True)
    find = lambda shape, sym: next(r for r in rows if (r["B"], r["N"], r["D"]) == shape and r["symmetric"] == sym)  # noqa: E731
    cond = [find(CONDITION_SHAPE, s) for s in (False, True)]
    tiny_ms = tiny_fit_step_ms()
    result = {
        "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "inner_pairs_per_repeat": args.inner,
        "what": "median microseconds of one forward call + one backward call, cos, scale 20; host clock around INNER pairs "
                "between two synchronisations, fused and torch ops alternated; allocation of outputs and workspace included",
        "rows": rows,
        "condition": {"shape": list(CONDITION_SHAPE), "fused_not_slower_than_torch_ops": all(r["speedup"] >= 1.0 for r in cond)},
        "tiny_fit_step_ms": round(tiny_ms, 4),
        "pair_share_of_tiny_fit_step": round(find((8, 8, 64), False)["fused_pair_us"] / (tiny_ms * 1e3), 4),
        "headline_step_ms": HEADLINE_STEP_MS,
        "pair_share_of_headline_step": round(cond[0]["fused_pair_us"] / (HEADLINE_STEP_MS * 1e3), 4),
    }
    print(json.dumps({k: v for k, v in result.items() if k != "rows"}), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
