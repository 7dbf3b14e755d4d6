"""Time of the forward + backward of MatryoshkaLoss(MultipleNegativesRankingLoss) on given embeddings, with
`fused_dims=True` (one qst_mnrl_nested_loss call each way) next to `fused_dims=False` (the composed path: per width a
slice, F.normalize and a qst_mnrl_loss call pair, the gradients summed by autograd -- only kernels that were there before
the nested one), in the same process, alternated repeat by repeat. A repeat is INNER forward + backward passes between two
full synchronisations; the figures are the median and the quartiles over the repeats after a warm-up. The encoder is a
stand-in that hands the embeddings through, so only the loss is timed. Also: a fit() step of the tiny model both ways.
Writes profiles/matryoshka_bench.json, with the decision about the default of `fused_dims`: the single call stays the
default only if its median is below the composed path's by more than the composed path's own interquartile spread.

    python tools/matryoshka_bench.py [--repeats 30] [--inner 30] [--out profiles/matryoshka_bench.json]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import mnrl_helpers as M  # noqa: E402
from quadruplet_sentence_transformer_amd import data, st_losses as S  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample, SentenceTransformer  # noqa: E402

CASES = [(64, 128, 384, [384, 256, 128, 64, 32]), (256, 512, 768, [768, 512, 256, 128, 64])]
TINY_DIMS = [64, 32, 16, 8, 4]
HEADLINE_STEP_MS = 4.5


class HandThrough(nn.Module):
    """An encoder stand-in: the embeddings are in the features."""

    def forward(self, feats):
        return {"sentence_embedding": feats["emb"]}


def loss_of(dims, fused_dims):
    m = HandThrough()
    return S.MatryoshkaLoss(m, S.MultipleNegativesRankingLoss(m, fused=False), dims, fused_dims=fused_dims)


def pass_pair(lm, a, c):
    a, c = a.detach().requires_grad_(True), c.detach().requires_grad_(True)
    lm([{"emb": a}, {"emb": c}], None).backward()
    return [a.grad, c.grad]


def timed(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e6


def tiny_fit_steps_ms(rounds=3, steps=40):
    """bf16 fit() steps of tiny-bert under MatryoshkaLoss(MNRL), batches of 8 pairs, both ways alternated: the median of
    `rounds` timings of `steps` steps each."""
    random.seed(11)
    words = "a man rides red horse two dogs play in park woman eats green apple near old bridge small cat sleeps".split()
    pairs = [InputExample(texts=[" ".join(random.choices(words, k=9)) + f" {i}", " ".join(random.choices(words, k=9)) + f" now {i}"])
             for i in range(16)]
    kw = dict(warmup_steps=0, scheduler="constantlr", optimizer_params={"lr": 1e-4}, dropout=0, show_progress_bar=False)
    models, out = {}, {True: [], False: []}
    for fused_dims in (True, False):
        m = SentenceTransformer("tiny-bert", device="cuda")
        lm = S.MatryoshkaLoss(m, S.MultipleNegativesRankingLoss(m), TINY_DIMS, fused_dims=fused_dims)
        m.fit([(data.NoDuplicatesDataLoader(list(pairs), 8), lm)], epochs=2, **kw)       # warm-up
        models[fused_dims] = (m, lm)
    for _ in range(rounds):
        for fused_dims in (True, False):
            m, lm = models[fused_dims]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.fit([(data.NoDuplicatesDataLoader(list(pairs), 8), lm)], epochs=steps // 2, **kw)
            torch.cuda.synchronize()
            out[fused_dims].append((time.perf_counter() - t0) / steps * 1e3)
    return {k: round(statistics.median(v), 4) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matryoshka_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available() and args.repeats >= 20, "needs a HIP device and at least 20 repeats"
    rows = []
    for (B, N, D, dims) in CASES:
        a, c = [t.cuda() for t in M.case(B, N, D, "cos", 1, 1000 * B + D)]
        one, per = loss_of(dims, True), loss_of(dims, False)
        assert one._one_call(len(dims)) and not per._one_call(len(dims))
        g1, g0 = pass_pair(one, a, c), pass_pair(per, a, c)
        diff = max((x - y).abs().max().item() for x, y in zip(g1, g0))
        for _ in range(3):
            timed(lambda: pass_pair(one, a, c), args.inner)
            timed(lambda: pass_pair(per, a, c), args.inner)
        t1, t0 = [], []
        for _ in range(args.repeats):
            t1.append(timed(lambda: pass_pair(one, a, c), args.inner))
            t0.append(timed(lambda: pass_pair(per, a, c), args.inner))
        q1, q0 = statistics.quantiles(t1, n=4), statistics.quantiles(t0, n=4)
        m1, m0 = statistics.median(t1), statistics.median(t0)
        rows.append({"B": B, "N": N, "D": D, "dims": dims, "one_call_us": round(m1, 2), "composed_us": round(m0, 2),
                     "one_call_quartiles_us": [round(v, 2) for v in q1], "composed_quartiles_us": [round(v, 2) for v in q0],
                     "composed_interquartile_us": round(q0[2] - q0[0], 2), "saved_us": round(m0 - m1, 2),
                     "speedup": round(m0 / m1, 3), "one_call_wins": bool(m0 - m1 > q0[2] - q0[0]),
                     "saved_share_of_headline_step": round((m0 - m1) / (HEADLINE_STEP_MS * 1e3), 4),
                     "max_abs_gradient_difference": diff})
        print(json.dumps(rows[-1]), flush=True)
    tiny = tiny_fit_steps_ms()
    result = {
        "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "inner_passes_per_repeat": args.inner,
        "what": "median microseconds of one forward + backward of MatryoshkaLoss(MultipleNegativesRankingLoss) on given "
                "embeddings (autograd, allocation of outputs and workspaces included); host clock around INNER passes between "
                "two synchronisations; fused_dims=True (one_call) and fused_dims=False (composed) alternated",
        "rows": rows,
        "tiny_fit_step_ms": {"dims": TINY_DIMS, "one_call": tiny[True], "composed": tiny[False]},
        "headline_step_ms": HEADLINE_STEP_MS,
        "rule": "fused_dims=True stays the default only if one_call_us < composed_us - composed_interquartile_us at every shape",
        "fused_dims_default": bool(all(r["one_call_wins"] for r in rows)),
    }
    print(json.dumps({k: v for k, v in result.items() if k != "rows"}), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
