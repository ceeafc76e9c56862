"""TEST INFRASTRUCTURE -- the yardstick of a batch with q8_0 K/V caches (llmk_cache_create with LLMK_TYPE_Q8_0).

stored_q8() is the stored-value contract of include/llmk.h in numpy f32: blocks of 32 consecutive elements of a position's kv_dim row,
    c = clamp(x, +-65504); amax = max |c|; d32 = amax / 127; d = RNE_f16(d32); id = d32 != 0 ? 1 / d32 : 0
    q = clamp(round_half_away(c * id), +-127), every q = 0 where d == 0; a NaN in the block: d = NaN, every q = 0
    value = (float)q * (float)d
Quantising moves the logits of the test models by about 1e-2 of max |logit| (tests/test_batch_kvq8_cpu.py prints it per shape), so
the bar of a q8_0 batch is the one of an f16 batch: kv16_ref.forward_fed, the float64 pass fed the rows the device stored, at REL_TOL.
Quantised is the attention of a float64 pass that quantises its OWN rows -- the movement figure, and the rows the CPU file feeds
forward_fed to prove the yardstick."""
from __future__ import annotations

import numpy as np

import kv16_ref as kr
from kv16_ref import forward_fed, peek_all      # noqa: F401  (the yardstick is type-agnostic: re-exported)
from ref_pass import RefPass, attention

BLOCK = 32


def stored_q8(x) -> np.ndarray:
    """what a q8_0 batch stores for the f32 values x ([..., n], n a multiple of 32: blocks of 32 along the last axis), as f32.
    Every quotient and product is one f32 operation; the rounding to an integer is done in float64 on the f32 product; q becomes an
    int8 BEFORE the product with d, so no -0.0 appears."""
    x = np.asarray(x, np.float32)
    assert x.shape[-1] % BLOCK == 0, x.shape
    b = x.reshape(-1, BLOCK)
    nan = np.isnan(b).any(axis=1)
    with np.errstate(all="ignore"):
        c = np.clip(np.where(np.isnan(b), np.float32(0), b), np.float32(-kr.F16_MAX), np.float32(kr.F16_MAX))
        amax = np.abs(c).max(axis=1)
        d32 = amax / np.float32(127.0)
        assert d32.dtype == np.float32
        d = d32.astype(np.float16)
        inv = np.where(d32 != 0, np.float32(1.0) / d32, np.float32(0)).astype(np.float32)      # (infinite for the smallest subnormals)
        p = (c * inv[:, None]).astype(np.float32).astype(np.float64)
        r = np.sign(p) * np.floor(np.abs(p) + 0.5)                                              # nearest, ties away from zero
        zero = nan | (d.astype(np.float32) == 0)
        q = np.where(zero[:, None], 0.0, np.clip(np.nan_to_num(r, nan=0.0), -127.0, 127.0)).astype(np.int8)
        df = np.where(nan, np.float32(np.nan), d.astype(np.float32)).astype(np.float32)
        out = q.astype(np.float32) * df[:, None]
    return out.reshape(x.shape)


def idempotent(rows) -> bool:
    """how a test recognises q8_0 rows without a raw-bits hook: quantising stored values returns them bit for bit (every non-zero
    block holds a +-127), and none is infinite or NaN"""
    rows = np.ascontiguousarray(rows, np.float32)
    return bool(np.isfinite(rows).all()) and np.array_equal(stored_q8(rows).view(np.uint32), rows.view(np.uint32))


class Quantised:
    """RefPass.feed's attention over the pass's own keys and values as a q8_0 cache would hold them.  K, V: the quantised rows per
    layer, [rows][kv_dim] f32, as forward_fed takes them."""

    def __init__(self, n_layers: int):
        self.K, self.V = [None] * n_layers, [None] * n_layers

    def __call__(self, l, q, pos, own):
        K, V = own()
        self.K[l], self.V[l] = (stored_q8(z.reshape(len(z), -1)) for z in (K, V))
        return attention(q, self.K[l].astype(q.dtype).reshape(K.shape), self.V[l].astype(q.dtype).reshape(V.shape), pos)


def forward_quantised(fw, tokens):
    """(logits [n][V], K, V [L][n][kv_dim]) of the float64 pass that quantises its own K/V rows"""
    att = Quantised(fw.shape.n_layers)
    logits = RefPass(fw).feed(tokens, None, att)
    return logits, np.stack(att.K), np.stack(att.V)
