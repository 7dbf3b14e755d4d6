"""Launch the grouped wgrad kernel at BASELINE configs[1] shapes (for rocprofv3 --pmc passes).
usage: one_wgrad.py [--skew S] [--order O]   (QstTnGroup.skew / .order; QST_M, QST_H, QST_SPLITS from the environment)"""
import argparse, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quadruplet_sentence_transformer_amd
from quadruplet_sentence_transformer_amd import _lib


def make_group(M=32768, H=384, I=1536, dev="cuda", skew=0, order=0):
    bf = torch.bfloat16
    keep = []
    grp = _lib.QstTnGroup()
    grp.nprob, grp.splits = 4, int(__import__("os").environ.get("QST_SPLITS", "0"))
    grp.skew, grp.order = skew, order
    for i, (N, K) in enumerate([(H, I), (I, H), (H, H), (3 * H, H)]):
        A = torch.randn(M, N, device=dev).to(bf); B = torch.randn(M, K, device=dev).to(bf)
        C = torch.zeros(N, K, device=dev); cs = torch.zeros(N, device=dev)
        q = grp.prob[i]
        q.A, q.B, q.C, q.colsum = A.data_ptr(), B.data_ptr(), C.data_ptr(), cs.data_ptr()
        q.M, q.N, q.K, q.lda, q.ldb, q.ldc = M, N, K, N, K, K
        keep += [A, B, C, cs]
    flops = 2.0 * M * (H * I + I * H + H * H + 3 * H * H)
    return grp, keep, flops


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skew", type=int, default=0)
    ap.add_argument("--order", type=int, default=0)
    a = ap.parse_args()
    lib = _lib.load(); st = _lib.current_stream_ptr()
    H = int(os.environ.get("QST_H", "384"))
    grp, keep, flops = make_group(M=int(os.environ.get("QST_M", "16384")), H=H, I=4 * H, skew=a.skew, order=a.order)
    for _ in range(5):
        _lib.check(lib.qst_gemm_tn_group(grp, st))
    torch.cuda.synchronize()
