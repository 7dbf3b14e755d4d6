"""qst_listwise_distill_loss (csrc/listwise.hip: the K similarities of a query, both softmaxes, the divergence or the K - 1
squared errors, and the gradients of all 1 + K columns in one launch) next to sentence-transformers' DistillKLDivLoss and
multi-negative MarginMSELoss composed of torch ops on the same device (listwise_helpers.kl_upstream / margin_upstream: K
pairwise similarities, a stack, log_softmax, softmax, KLDivLoss or mse_loss, autograd). The device must be otherwise idle.

Forward + backward on given fp32 embeddings, for both kinds and both similarities, at B x K x D = 64 x 8 x 384,
256 x 16 x 768 and 4096 x 32 x 768: the kernel path as training runs it (the autograd function: one call forward, one with
gradients in backward), the single call with gradients on its own, and the torch composition, alternated repeat by repeat in
one process, each repeat between two synchronisations, the median after a warm-up; peak device memory of each beyond its
inputs. No ratio is promised: what is measured is what is written.
Writes profiles/listwise_bench.json.

    python tools/listwise_bench.py [--repeats 30] [--warmup 5] [--out profiles/listwise_bench.json]
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
import listwise_helpers as LH  # noqa: E402
import tuple_loss_helpers as H  # noqa: E402
from quadruplet_sentence_transformer_amd import _lib, st_losses as S  # noqa: E402

SHAPES = [(64, 8, 384), (256, 16, 768), (4096, 32, 768)]
TEMPERATURE = 2.0


def embeddings(B, K, D):
    """Unit rows drawn on the device, and a teacher a few units apart (scores) or off by half a unit (margins)."""
    g = torch.Generator(device="cuda").manual_seed(1000 * B + 10 * K + D)
    nrm = torch.nn.functional.normalize
    q = nrm(torch.randn(B, D, generator=g, device="cuda"), dim=1).contiguous()
    docs = nrm(torch.randn(K, B, D, generator=g, device="cuda"), dim=2).contiguous()
    scores = 3.0 * torch.randn(B, K, generator=g, device="cuda")
    margins = 0.5 * torch.randn(B, K - 1, generator=g, device="cuda")
    return q, docs, scores, margins


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


def med(xs):
    return round(statistics.median(xs), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "listwise_bench.json"))
    args = ap.parse_args()
    lib = _lib.load()
    rows = []
    for B, K, D in SHAPES:
        q, docs, scores, margins = embeddings(B, K, D)
        for kind in (LH.KL, LH.MARGIN):
            y = scores if kind == LH.KL else margins
            for sim in LH.SIMS:
                fct = lambda a, b, sim=sim: H.metric_ref(a, b, sim)  # noqa: E731

                def autograd_path():
                    xq, xd = q.clone().requires_grad_(True), docs.clone().requires_grad_(True)
                    loss = S.listwise_distill(xq, xd, y, kind, sim, TEMPERATURE, "mean")
                    loss.backward()
                    return loss.detach(), xq.grad, xd.grad

                def one_call():
                    return S.listwise_distill_raw(q, docs, y, kind, sim, TEMPERATURE, 2, want_grads=True)

                def torch_ops():
                    xq, xd = q.clone().requires_grad_(True), docs.clone().requires_grad_(True)
                    if kind == LH.KL:
                        loss = LH.kl_upstream(xq, xd, y, fct, TEMPERATURE)
                    else:
                        loss = LH.margin_upstream(xq, xd, y, fct)
                    loss.backward()
                    return loss.detach(), xq.grad, xd.grad

                (lk, gqk, gdk), (lt, gqt, gdt) = autograd_path(), torch_ops()
                agree = {"loss_kernel": lk.item(), "loss_torch": lt.item(),
                         "grad_q_rel_diff": ((gqk - gqt).norm() / gqt.norm()).item(),
                         "grad_docs_rel_diff": ((gdk - gdt).norm() / gdt.norm()).item()}
                del gqk, gdk, gqt, gdt
                for _ in range(args.warmup):
                    autograd_path(), one_call(), torch_ops()
                ta, tc, tt = [], [], []
                for _ in range(args.repeats):
                    ta.append(timed_ms(autograd_path))
                    tc.append(timed_ms(one_call))
                    tt.append(timed_ms(torch_ops))
                row = {"B": B, "K": K, "D": D, "kind": LH.KIND_NAMES[kind], "sim": H.METRIC_NAMES[sim],
                       "temperature": TEMPERATURE if kind == LH.KL else None,
                       "kernel_autograd_ms": med(ta), "kernel_one_call_ms": med(tc), "torch_ms": med(tt),
                       "kernel_autograd_ms_min_max": [round(min(ta), 4), round(max(ta), 4)],
                       "kernel_one_call_ms_min_max": [round(min(tc), 4), round(max(tc), 4)],
                       "torch_ms_min_max": [round(min(tt), 4), round(max(tt), 4)],
                       "torch_over_kernel_autograd": round(statistics.median(tt) / statistics.median(ta), 2),
                       "kernel_autograd_peak_mib": peak_mib(autograd_path), "kernel_one_call_peak_mib": peak_mib(one_call),
                       "torch_peak_mib": peak_mib(torch_ops),
                       "one_call_bytes": 4 * ((1 + K) * B * D + K * B * D + (1 + K) * B * D),
                       "launches_one_call": 2, **agree}
                row["one_call_gbytes_per_s"] = round(row["one_call_bytes"] / (row["kernel_one_call_ms"] * 1e-3) / 1e9, 1)
                print(json.dumps(row), flush=True)
                rows.append(row)
        del q, docs, scores, margins
    out = {"device": torch.cuda.get_device_name(0), "qst_version": lib.qst_version(), "repeats": args.repeats,
           "warmup": args.warmup,
           "what": "forward + backward, median ms per call; peak MiB beyond the inputs; one_call_bytes = rows read for the "
                   "scores, read again and written by the gradient pass", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
