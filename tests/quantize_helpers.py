"""The yardstick of embedding quantization (tests/test_quantize_host.py, tests/test_gpu_quantize.py): numpy references for
the column ranges, the bit packing, the 8-bit codes with the library's saturation rules, the two first-stage scores and the
rescoring products. numpy only, so the host test imports it without the library. Imported like topk_stream_cases.

Everything integer is exact, so the tests compare with ==. The float32 formula of the 8-bit codes is evaluated operation by
operation on float32 arrays, which is what upstream's numpy expression does."""
import numpy as np

INT8, UINT8, BINARY, UBINARY = 0, 1, 2, 3
KIND = {"int8": INT8, "uint8": UINT8, "binary": BINARY, "ubinary": UBINARY}


def ranges_ref(x):
    """[2, dim]: np.min / np.max over the rows (a NaN in a column makes both NaN)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.stack([x.min(axis=0), x.max(axis=0)])


def pack_bits(bits):
    """[n, dim] of 0 / 1 -> uint8 [n, ceil(dim / 8)], first bit most significant, written out by hand (the host test
    holds it against np.packbits)."""
    bits = np.asarray(bits).astype(np.uint8)
    n, dim = bits.shape
    nbytes = (dim + 7) // 8
    padded = np.zeros((n, nbytes * 8), dtype=np.uint8)
    padded[:, :dim] = bits
    out = np.zeros((n, nbytes), dtype=np.uint8)
    for e in range(8):
        out |= (padded[:, e::8] << (7 - e)).astype(np.uint8)
    return out


def bits_ref(x, kind):
    """ubinary: packbits(x > 0) as uint8; binary: the same byte - 128 as int8."""
    with np.errstate(invalid="ignore"):
        packed = pack_bits(np.asarray(x, dtype=np.float32) > 0)
    if kind == UBINARY:
        return packed
    return (packed.astype(np.int16) - 128).astype(np.int8)


def codes_ref(x, ranges, kind):
    """uint8: trunc((x - lo) / ((hi - lo) / 255)) saturated to [0, 255]; int8: trunc(that - 128) saturated to [-128, 127];
    every operation in float32. A NaN quotient, or hi == lo, gives the lowest code."""
    x = np.asarray(x, dtype=np.float32)
    lo, hi = np.asarray(ranges, dtype=np.float32)
    with np.errstate(all="ignore"):
        step = (hi - lo) / np.float32(255.0)
        t = (x - lo[None, :]) / step[None, :]
        assert step.dtype == np.float32 and t.dtype == np.float32
        t = np.where((hi == lo)[None, :], np.float32(np.nan), t)
        if kind == INT8:
            t = t - np.float32(128.0)
            low, high, dtype = -128, 127, np.int8
        else:
            low, high, dtype = 0, 255, np.uint8
        bad = np.isnan(t)
        v = np.trunc(np.where(bad, np.float32(low), t))
        v = np.clip(v, low, high)
    return v.astype(np.int64).astype(dtype)


def unpack(codes, kind, dim):
    """The values the rescoring multiplies the query with, int64 [n, dim]: the bit for the bit kinds, else the integer."""
    codes = np.asarray(codes)
    if kind in (BINARY, UBINARY):
        raw = codes.view(np.uint8) ^ np.uint8(0x80 if kind == BINARY else 0)
        return np.unpackbits(raw, axis=1)[:, :dim].astype(np.int64)
    return codes.astype(np.int64)


def hamming_scores(q, c):
    """float32 [nq, nc] of -(differing bits) of packed rows (either kind: the xor cancels 0x80). Exact: the counts come from
    float32 matrix products of 0 / 1 values, integers far below 2^24."""
    qb = np.unpackbits(np.asarray(q).view(np.uint8), axis=1).astype(np.float32)
    cb = np.unpackbits(np.asarray(c).view(np.uint8), axis=1).astype(np.float32)
    return -(qb @ (1.0 - cb).T + (1.0 - qb) @ cb.T).astype(np.float32)


def int8_scores(q, c):
    """float32 [nq, nc] of the exact integer dot products (|.| <= 2^24 for widths up to 1024: exact in float32)."""
    s = np.asarray(q).astype(np.int64) @ np.asarray(c).astype(np.int64).T
    assert np.abs(s).max() <= 1 << 24
    return s.astype(np.float32)


def rescore_ref(q, codes, kind, dim):
    """(fp64 [nq, nc] of sum_j q_j v_j, fp64 [nq, nc] of sum_j |q_j v_j|) against every corpus row."""
    q = np.asarray(q, dtype=np.float64)
    v = unpack(codes, kind, dim).astype(np.float64)
    return q @ v.T, np.abs(q) @ np.abs(v).T


def rescore_bound(dim, abs_sum):
    """fp32 accumulation of dim products in any order: |error| <= dim * 2^-24 * sum_j |q_j v_j| (each of at most dim
    roundings is relative 2^-24 of a partial sum no larger than the sum of magnitudes)."""
    return dim * 2.0 ** -24 * abs_sum


SALT = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45], dtype=np.float32)


def salted(n, dim, seed):
    """Gaussian rows with 0.0, -0.0, NaN, +-inf and the smallest denormals of either sign scattered over them."""
    rng = np.random.RandomState(seed)
    x = rng.randn(n, dim).astype(np.float32)
    where = rng.rand(n, dim) < 0.3
    x[where] = SALT[rng.randint(0, len(SALT), size=int(where.sum()))]
    return x


def random_codes(n, nbytes, seed, duplicates=True):
    """uint8 [n, nbytes]; with duplicates the second half repeats rows of the first (equal distances to every query)."""
    rng = np.random.RandomState(seed)
    c = rng.randint(0, 256, size=(n, nbytes)).astype(np.uint8)
    if duplicates and n >= 2:
        c[n // 2:] = c[rng.randint(0, n // 2, size=n - n // 2)]
    return c
