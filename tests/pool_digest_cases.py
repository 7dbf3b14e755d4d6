"""The cases behind tests/golden/pool_digests.json: one SHA-256 per buffer a pooling forward + backward writes (emb, pooled,
argmax where the head has max, dtok), recorded on the library of the commit before rowops.hip went from two kernel pairs to
one. tools/pool_digest.py records and prints them, tests/test_gpu_pooling.py requires the tree's library to reproduce them:
equal digests are equal bits. Needs numpy and torch only, so the tool can drive any build of libqst.so through ctypes.

Inputs come from integer arithmetic, not from a library's random stream: element i of a tensor with seed s is
(k >> 8) / 2^23 - 1 with k = (i * 2654435761 + s * 40503) mod 2^32, exact in float32. Four sequences per case: all padding,
full, one valid token, L // 2 + 1 valid tokens (right-padded). Outputs are pre-filled with NaN (argmax with -7), so bytes a
kernel leaves unwritten show in the digest.
"""
import hashlib

import numpy as np
import torch

NSEQ = 4
MEAN, ALL = 4, 31
TOK_SEED, DEMB_SEED = 1, 2
# (H, L, modes): the smallest shapes at which each loop of the kernels can go wrong
SHAPES = [
    (64, 32, (MEAN,)),                    # one column group, one trip
    (96, 40, tuple(range(1, 32))),        # fewer vector columns than lanes; second trip of the four-in-flight loop, rows past L
    (770, 33, tuple(range(1, 32))),       # c < nv inside the last column group; partial second pass of tid + 512 k
    (384, 128, (MEAN,)),                  # headline shape
    (1024, 512, (MEAN, ALL)),             # both limits, full VPL, largest LDS
]
CASES = [(H, L, mode, normalize) for H, L, modes in SHAPES for mode in modes for normalize in (0, 1)]


def case_name(H, L, mode, normalize):
    return f"H={H} L={L} mode={mode} normalize={normalize}"


def values(n, seed):
    k = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(seed * 40503)) & np.uint64(0xFFFFFFFF)
    return (k >> np.uint64(8)).astype(np.float32) / np.float32(2 ** 23) - np.float32(1)


def mask_of(L):
    lens = np.array([0, L, 1, L // 2 + 1])
    return (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_case(fwd, bwd, H, L, mode, normalize, stream=None):
    """fwd / bwd: callables with the argument lists of qst_pool_fwd / qst_pool_bwd (raw pointers). Returns the digests of the
    case: inputs, emb, pooled, [argmax,] dtok."""
    D = bin(mode).count("1") * H
    tok, mask, demb = values(NSEQ * L * H, TOK_SEED), mask_of(L), values(NSEQ * D, DEMB_SEED + mode)
    out = {"inputs": sha(tok, mask, demb)}
    tok_d, mask_d, demb_d = torch.from_numpy(tok).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(demb).cuda()
    emb = torch.full((NSEQ, D), float("nan"), device="cuda")
    pooled = torch.full((NSEQ, D), float("nan"), device="cuda")
    argmax = torch.full((NSEQ, H), -7, dtype=torch.int32, device="cuda")
    dtok = torch.full((NSEQ, L, H), float("nan"), device="cuda")
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    st = fwd(tok_d.data_ptr(), mask_d.data_ptr(), NSEQ, L, H, mode, normalize, emb.data_ptr(), pooled.data_ptr(), argmax.data_ptr(),
             stream)
    assert st == 0, f"qst_pool_fwd returned {st}"
    st = bwd(demb_d.data_ptr(), pooled.data_ptr(), argmax.data_ptr(), mask_d.data_ptr(), NSEQ, L, H, mode, normalize,
             dtok.data_ptr(), stream)
    assert st == 0, f"qst_pool_bwd returned {st}"
    torch.cuda.synchronize()
    out["emb"], out["pooled"] = sha(emb.cpu().numpy()), sha(pooled.cpu().numpy())
    if mode & 2:
        out["argmax"] = sha(argmax.cpu().numpy())
    out["dtok"] = sha(dtok.cpu().numpy())
    return out
