"""qst_gist_loss (csrc/gist.hip: guide scores, student logits, mask, loss and the gradients of every column in one call, no
B x B tensor outside a strip) next to sentence-transformers' GISTEmbedLoss formula composed of torch ops on the same device
(gist_helpers.gist_ref: eight B x B blocks, boolean masks, torch.cat, F.cross_entropy, autograd). The device must be otherwise
idle.

Forward + backward on given fp32 embeddings, two text columns, temperature 0.01, margin 0, at B x D (guide width) =
64 x 384 (768), 256 x 768 (1024) and 4096 x 768 (1024): the two alternated repeat by repeat in one process, each repeat
between two synchronisations, the median after a warm-up; peak device memory of each call beyond its inputs; the kernel's
launch count and workspace. No ratio is promised: what is measured is what is written.
Writes profiles/gist_bench.json.

    python tools/gist_bench.py [--repeats 30] [--warmup 5] [--out profiles/gist_bench.json]
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
import gist_helpers as G  # noqa: E402
from quadruplet_sentence_transformer_amd import _lib, st_losses as S  # noqa: E402

SHAPES = [(64, 2, 384, 768), (256, 2, 768, 1024), (4096, 2, 768, 1024)]
TEMPERATURE = 0.01


def embeddings(B, K, D, Dg):
    """Student rows of their own lengths in random directions; a guide with clusters of four and alternating positives
    (the recipe of gist_helpers.guide_case, drawn on the device)."""
    g = torch.Generator(device="cuda").manual_seed(1000 * B + D)
    nrm = torch.nn.functional.normalize

    def unit(n, d):
        return nrm(torch.randn(n, d, generator=g, device="cuda"), dim=1)

    x = unit(K * B, D) * (0.5 + 1.5 * torch.rand(K * B, 1, generator=g, device="cuda"))
    cl = torch.arange(B, device="cuda") // 4
    c1, c2 = unit(int(cl.max()) + 1, Dg), unit(int(cl.max()) + 1, Dg)
    a = nrm(c1[cl] + 0.3 * unit(B, Dg), dim=1)
    far = (torch.arange(B, device="cuda") % 2 == 0).view(-1, 1)
    p = torch.where(far, nrm(a + 1.1 * nrm(c2[cl] + 0.3 * unit(B, Dg), dim=1), dim=1), nrm(a + 0.15 * unit(B, Dg), dim=1))
    cols = [a, p] + [nrm(a + 0.35 * unit(B, Dg), dim=1) for _ in range(K - 2)]
    return x.contiguous(), torch.cat(cols, 0).contiguous()


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


def launches(B, K, with_grads):
    """The launch count of one call at the library's own strip (include/qst.h)."""
    ld = (K + 1) * B + (-(K + 1) * B) % 4
    rows = max(64, ((64 << 20) // 4 // 2 // ld) // 64 * 64)
    rows = min(rows, (B + 63) // 64 * 64)
    strips = -(-B // rows)
    chunked = (1 if K * B > 4096 else 0) + (1 if B > 4096 else 0)
    return (4 + (9 + chunked) * strips if with_grads else 3 + 5 * strips), strips


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gist_bench.json"))
    args = ap.parse_args()
    lib = _lib.load()
    rows = []
    for B, K, D, Dg in SHAPES:
        x, g = embeddings(B, K, D, Dg)

        def kernel():
            return S.gist_loss_raw(x, g, K, TEMPERATURE, "absolute", 0.0, 0, want_grads=True)

        def torch_ops():
            xs = x.clone().requires_grad_(True)
            loss = G.gist_ref(list(xs.chunk(K, 0)), list(g.chunk(K, 0)), TEMPERATURE)
            loss.backward()
            return loss.detach(), xs.grad

        (lk, gk), (lt, gt) = kernel(), torch_ops()
        agree = {"loss_kernel": lk.item(), "loss_torch": lt.item(),
                 "grad_rel_diff": ((gk - gt).norm() / gt.norm()).item()}
        for _ in range(args.warmup):
            kernel(), torch_ops()
        tk, tt = [], []
        for _ in range(args.repeats):
            tk.append(timed_ms(kernel))
            tt.append(timed_ms(torch_ops))
        n_launch, strips = launches(B, K, True)
        row = {"B": B, "K": K, "D": D, "Dg": Dg, "temperature": TEMPERATURE,
               "kernel_ms": round(statistics.median(tk), 4), "torch_ms": round(statistics.median(tt), 4),
               "kernel_ms_min_max": [round(min(tk), 4), round(max(tk), 4)],
               "torch_ms_min_max": [round(min(tt), 4), round(max(tt), 4)],
               "torch_over_kernel": round(statistics.median(tt) / statistics.median(tk), 2),
               "kernel_peak_mib": peak_mib(kernel), "torch_peak_mib": peak_mib(torch_ops),
               "workspace_bytes": int(lib.qst_gist_workspace_bytes(B, K, D, Dg, 0)), "strips": strips,
               "launches_forward": launches(B, K, False)[0], "launches_with_gradients": n_launch, **agree}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x, g
    out = {"device": torch.cuda.get_device_name(0), "qst_version": lib.qst_version(), "repeats": args.repeats,
           "warmup": args.warmup, "what": "forward + backward, median ms per call; peak MiB beyond the inputs", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
