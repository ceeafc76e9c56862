"""numpy restatement of the device sampler's rule (llm.f90_amd/csrc/sample.h, include/llmk.h llmk_forward_sample):

    token = 1 + argmax_i ( logits[i] * invT + g(seed, pos, i) )      first maximum wins, i 0-based
    g     = -log(-log(u)),  u = float((w >> 8) | 1) * 2^-24
    w     = Philox4x32-10(counter = (i >> 2, pos, 0, 0), key = (seed & 0xffffffff, seed >> 32))[i & 3]
    invT  = f32(1 / T)

w and u are bit-exact; g is computed in f64 and rounded to f32 (the device's logf may differ by an ulp or so)."""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: 4 arrays of uint32 (broadcast together), key: 2 of them -> the 4 output words as uint32 arrays."""
    c = [np.asarray(x, np.uint64) for x in ctr]
    k0, k1 = (np.asarray(x, np.uint64) for x in key)
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(_W0)) & _MASK
            k1 = (k1 + np.uint64(_W1)) & _MASK
        p0 = _M0 * c[0]
        p1 = _M1 * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return [x.astype(np.uint32) for x in c]


def bits(seed: int, pos, i):
    """w for row(s) i at position(s) pos (pos 1-based, i 0-based)."""
    i = np.asarray(i, np.int64)
    pos = np.asarray(pos, np.int64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    z = np.zeros(np.broadcast(i, pos).shape, np.uint64)
    out = philox4x32_10([(i >> 2) + z, pos + z, z, z], [seed & 0xFFFFFFFF, seed >> 32])
    return np.choose(np.broadcast_to(i & 3, z.shape), out)


def uniform(w):
    """u = odd multiple of 2^-24 in (0, 1), f32 (exact)."""
    return ((np.asarray(w, np.uint32) >> np.uint32(8)) | np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -24)


def gumbel(w):
    return (-np.log(-np.log(uniform(w).astype(np.float64)))).astype(np.float32)


def inv_temperature(T: float):
    return np.float32(1.0) / np.float32(T)


def scores(logits, T: float, seed: int, pos: int):
    """logits[i] * invT + g, each operation rounded to f32."""
    lg = np.asarray(logits, np.float32)
    s = (lg * inv_temperature(T)).astype(np.float32)
    return (s + gumbel(bits(seed, pos, np.arange(lg.size)))).astype(np.float32)


def sample(logits, T: float, seed: int, pos: int):
    """(1-based token, relative margin between the top two scores)."""
    s = scores(logits, T, seed, pos).astype(np.float64)
    j = int(np.argmax(s))
    top2 = np.partition(s, -2)[-2:]
    margin = (top2[1] - top2[0]) / max(abs(top2[1]), 1.0)
    return j + 1, margin
