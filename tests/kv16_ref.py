"""TEST INFRASTRUCTURE -- the yardstick of a batch with f16 K/V caches (llmk_cache_*).

Rounding K and V to f16 where the cache is written moves the logits of the test models by 3e-4 .. 5e-4 of max |logit|: the oracle at
REL_TOL = 1e-4 cannot judge such a batch.  A reference that rounds its OWN K/V cannot either: arithmetic noise of 1e-6 flips single
f16 roundings from layer 1 on, and two such references (float64, float32) differ by up to 1e-4.  So forward_fed() is the pass
of tests/ref_pass.py with one thing added: each layer's attention reads GIVEN cache rows -- the rows the device stored, read back with
llmk_cache_peek, the current position's row included.  All that then remains between the device and the reference is f32 arithmetic,
and the bar is REL_TOL again.  tests/test_batch_kv16_cpu.py proves the yardstick without a device.

half_mirror() is the stored-value contract in numpy integers, checked against np.float16 by the same file."""
from __future__ import annotations

import numpy as np

from ref_pass import Given, RefPass

F16_MAX = 65504.0


def stored_half(x) -> np.ndarray:
    """what an f16 batch stores for the f32 value x: clamp to +-65504, then round to nearest even (NaN stays NaN), as f32"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return np.clip(x, np.float32(-F16_MAX), np.float32(F16_MAX)).astype(np.float16).astype(np.float32)


def half_mirror(x) -> np.ndarray:
    """The contract spelled out on the bits of f32 values, without numpy's own conversion: h = NaN for NaN, else RNE_f16(clamp(x,
    -65504, 65504)), f16 subnormals kept.  Returns the uint16 bit patterns."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    sign = ((u >> 31) & 1).astype(np.uint16) << 15
    mag = u & 0x7FFFFFFF
    nan = mag > 0x7F800000
    mag = np.minimum(mag, np.uint64(np.float32(F16_MAX).view(np.uint32)))            # the clamp (+-inf included)
    ex = (mag >> 23).astype(np.int64)                                                # biased f32 exponent
    man = (mag & 0x7FFFFF) | np.where(ex > 0, 0x800000, 0).astype(np.uint64)         # 24-bit significand (f32 subnormals: no hidden bit)
    # value = man * 2^(max(ex, 1) - 150); an f16's unit in the last place is 2^max(e - 25, -24) with e the unbiased exponent + 1:
    # shift = bits to drop from man so that the result counts f16 ulps
    e = np.maximum(ex, 1) - 127                                                      # unbiased exponent of the hidden bit
    shift = np.where(e >= -14, 13, 13 + (-14 - e)).astype(np.int64)                  # normal f16: 10 mantissa bits of 23; below: more
    shift = np.minimum(shift, 40)
    q = man >> shift.astype(np.uint64)
    rem = man & ((np.uint64(1) << shift.astype(np.uint64)) - np.uint64(1))
    half = np.uint64(1) << (shift - 1).astype(np.uint64)
    q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1))).astype(np.uint64)      # nearest, ties to even
    # q counts ulps: a normal f16 is (1024 + m) * 2^(e - 10), so bits = (e + 14) * 1024 + q (a carry out of the mantissa moves on to
    # the next exponent by itself); a subnormal is q * 2^-24, bits = q (q = 1024 is the smallest normal, again by itself)
    bits = np.where(e >= -14, ((e + 14) * 1024).astype(np.int64) + q.astype(np.int64), q.astype(np.int64)).astype(np.uint16)
    return np.where(nan, np.uint16(0x7E00), bits | sign).astype(np.uint16)


def forward_fed(fw, tokens, K, V, pos=None):
    """The float64 pass of ref_pass.RefPass over f32 FusedWeights, except that layer l's attention reads the GIVEN cache rows K[l],
    V[l] ([rows][kv_dim], cache row r = position r + 1) and never its own keys and values (ref_pass.Given): row i feeds tokens[i]
    (1-based id) at position pos[i] (1-based; None: 1 .. n) and attends over cache rows 0 .. pos[i] - 1, its own position's row
    included.  Returns logits [n][V]."""
    return RefPass(fw).feed(tokens, pos, Given(K, V))


def peek_all(b, n_layers: int, slot: int, n: int):
    """(K, V) of `slot`'s cache rows 0 .. n-1 of every layer, as forward_fed takes them: [L][n][kv_dim] f32"""
    return tuple(np.stack([b.peek_kv(which, l, slot, 1, n) for l in range(n_layers)]) for which in (0, 1))
