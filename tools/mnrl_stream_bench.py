"""qst_mnrl_stream_loss (csrc/mnrl_stream.hip: no B x N score matrix, products on the fp32 matrix cores) next to
qst_mnrl_loss (csrc/mnrl.hip: the whole score matrix, products on the fp32 VALU tile of fp32_tile.h), and one training step
of CachedMultipleNegativesRankingLoss next to one of plain MultipleNegativesRankingLoss. The device must be otherwise idle.

  kernel  forward + backward in one call (loss and both gradients) on given fp32 embeddings, cos, plain and symmetric, at
          B = N in {4096, 8192, 16384} and D in {384, 768}: the two entries alternated repeat by repeat in one process, each
          repeat between two synchronisations, the median after a warm-up; peak device memory of each call beyond its inputs.
          B = N = 65536, D = 768: the streaming entry alone -- the old one refuses the shape.
  step    MiniLM dimensions (seeded random weights), 128 tokens, dropout 0.1, bf16, forward + backward + AdamW:
          CachedMultipleNegativesRankingLoss at batch 4096 in mini-batches of 64, and MultipleNegativesRankingLoss at batch
          64. Different objectives (4095 against 63 in-batch negatives): the pair is reported, not compared.
Writes profiles/mnrl_stream_bench.json.

    python tools/mnrl_stream_bench.py [--repeats 7] [--steps 3] [--skip-step] [--out profiles/mnrl_stream_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import quadruplet_sentence_transformer_amd  # noqa: E402,F401
import mnrl_helpers as M  # noqa: E402
from quadruplet_sentence_transformer_amd import st_losses as S  # noqa: E402
from quadruplet_sentence_transformer_amd.sentence_transformer import SentenceTransformer  # noqa: E402

SIZES, DIMS = (4096, 8192, 16384), (384, 768)
LARGE = (65536, 65536, 768)


def embeddings(B, N, D):
    """Rows of their own lengths around a unit vector, every positive pulled towards its anchor (mnrl_helpers.case, drawn on
    the device: its fp64 host recipe takes minutes at these sizes)."""
    g = torch.Generator(device="cuda").manual_seed(1000 * B + D)
    nrm = torch.nn.functional.normalize
    a = nrm(torch.randn(B, D, generator=g, device="cuda"), dim=1)
    c = nrm(torch.randn(N, D, generator=g, device="cuda"), dim=1)
    c[:B] = nrm(a + 3.0 * c[:B], dim=1)
    a *= 0.5 + 1.5 * torch.rand(B, 1, generator=g, device="cuda")
    c *= 0.5 + 1.5 * torch.rand(N, 1, generator=g, device="cuda")
    return a.contiguous(), c.contiguous()


def timed_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def kernel_rows(repeats):
    rows = []
    for n in SIZES:
        for D in DIMS:
            a, c = embeddings(n, n, D)
            for symmetric in (0, 1):
                stream = lambda: S.mnrl_stream_loss_raw(a, c, "cos", M.SCALE, symmetric, 0, want_grads=True)  # noqa: E731
                whole = lambda: S.mnrl_loss_raw(a, c, "cos", M.SCALE, symmetric, want_grads=True)  # noqa: E731
                (ls, gs), (lw, gw) = stream(), whole()
                diff = max(M.grad_error(x.cpu(), y.cpu()) for x, y in zip(gs, gw))
                dloss = abs(ls.item() - lw.item())
                del gs, gw
                for _ in range(2):
                    timed_ms(stream), timed_ms(whole)
                ts, tw = [], []
                for _ in range(repeats):
                    ts.append(timed_ms(stream))
                    tw.append(timed_ms(whole))
                products = 4 if symmetric else 3
                flop = 2.0 * n * n * D
                rows.append({"B": n, "N": n, "D": D, "symmetric": bool(symmetric),
                             "stream_ms": round(statistics.median(ts), 3), "whole_matrix_ms": round(statistics.median(tw), 3),
                             "stream_min_ms": round(min(ts), 3), "whole_matrix_min_ms": round(min(tw), 3),
                             "whole_over_stream": round(statistics.median(tw) / statistics.median(ts), 3),
                             "stream_tflops_of_its_products": round(products * flop / statistics.median(ts) / 1e9, 1),
                             "whole_matrix_tflops_of_its_products": round(3 * flop / statistics.median(tw) / 1e9, 1),
                             "stream_peak_mib": peak_mib(stream), "whole_matrix_peak_mib": peak_mib(whole),
                             "loss_difference": dloss, "gradient_difference_share_of_tolerance": round(diff, 3)})
                print(json.dumps(rows[-1]), flush=True)
            del a, c
    return rows


def large_row(repeats):
    B, N, D = LARGE
    a, c = embeddings(B, N, D)
    assert B * N > 2 ** 31 - 1                          # qst_mnrl_loss answers QST_ERR_UNSUPPORTED
    out = []
    for symmetric in (0, 1):
        stream = lambda: S.mnrl_stream_loss_raw(a, c, "cos", M.SCALE, symmetric, 0, want_grads=True)  # noqa: E731
        loss, _ = stream()
        timed_ms(stream)
        ts = [timed_ms(stream) for _ in range(max(3, repeats // 2))]
        products = 4 if symmetric else 3
        out.append({"B": B, "N": N, "D": D, "symmetric": bool(symmetric), "stream_ms": round(statistics.median(ts), 2),
                    "stream_min_ms": round(min(ts), 2),
                    "stream_tflops_of_its_products": round(products * 2.0 * B * N * D / statistics.median(ts) / 1e9, 1),
                    "stream_peak_mib": peak_mib(stream), "loss": loss.item(), "whole_matrix": "QST_ERR_UNSUPPORTED",
                    "whole_matrix_scores_gib": round(4.0 * B * N / 2 ** 30, 1)})
        print(json.dumps(out[-1]), flush=True)
    return out


def step_rows(steps):
    """Sentences per second and peak memory of whole training steps on token ids drawn from a seed."""
    m = SentenceTransformer("all-MiniLM-L6-v2", device="cuda", allow_random_init=True)
    enc = m._enc
    m.train()
    enc.ensure_train_state()
    enc.set_dropout(0.1, 0.1, 14)
    g = torch.Generator().manual_seed(5)
    rows = []
    try:
        for name, lm, batch in (("CachedMultipleNegativesRankingLoss", S.CachedMultipleNegativesRankingLoss(m, mini_batch_size=64), 4096),
                                ("MultipleNegativesRankingLoss", S.MultipleNegativesRankingLoss(m), 64)):
            feats = [{"input_ids": torch.randint(1000, 20000, (batch, 128), generator=g).cuda(),
                      "attention_mask": torch.ones(batch, 128, dtype=torch.int64).cuda()} for _ in range(2)]
            labels = torch.zeros(batch, device="cuda")

            def step():
                lm([dict(f) for f in feats], labels).backward()
                enc.adamw_step(2e-5)

            reps = steps if batch > 64 else steps * 20
            timed_ms(step)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            for _ in range(reps):
                step()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / reps
            rows.append({"loss": name, "batch": batch, "mini_batch_size": getattr(lm, "mini_batch_size", None), "columns": 2,
                         "tokens": 128, "dropout": 0.1, "precision": "bf16", "step_ms": round(dt * 1e3, 2),
                         "sentences_per_second": round(2 * batch / dt, 1),
                         "peak_memory_mib": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1), "steps_timed": reps})
            print(json.dumps(rows[-1]), flush=True)
    finally:
        enc.set_dropout(0.0, 0.0)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mnrl_stream_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "what": "kernel: median milliseconds of one call that returns the loss and both gradients, cos, scale 20, host "
                      "clock between two synchronisations, the two entries alternated; allocation of outputs and workspace "
                      "included; peak = device memory beyond the inputs. step: forward + backward + AdamW",
              "kernel": kernel_rows(args.repeats), "past_the_old_limit": large_row(args.repeats)}
    if not args.skip_step:
        result["step"] = step_rows(args.steps)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
