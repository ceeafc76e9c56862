"""What the yardsticks rely on in tests/ref_pass.py, pinned (no device): feeding in pieces, forks, attention over given rows, eps,
the wrappers' agreement with each other, and float32 staying float32.  "Equal" is 1e-12 of the position's max |logit| (of the
array's max |value| for a tap): the old copies of the pass were 2e-15 apart on these shapes, a BLAS that sums in another order has
room, and the bar is eight orders under REL_TOL."""
import dataclasses
import functools

import numpy as np
import pytest

import attn_needle as an
import weight_edge as we
from conftest import rel_err
from llm_f90_amd.tools import gguf
from ref_pass import Causal, Given, RefPass, rope_freqs

SHAPES = ("tiny-gqa", "tiny-hs128")       # hs 16 with kv_mul 4, hs 128 with kv_mul 1
N = 40
EQUAL = 1e-12


def fed(p, tokens, **kw):
    """(logits, {tap name: [L][m][...]}) of one feed"""
    got = {}
    logits = p.feed(tokens, tap=lambda l, name, a: got.setdefault(name, []).append(a), **kw)
    return logits, {name: np.stack(a) for name, a in got.items()}


@functools.lru_cache(maxsize=None)
def whole(shape):
    """(weights, tokens, logits, taps) of the N positions fed at once in float64: shared, read-only"""
    s = gguf.SHAPES[shape]
    fw = gguf.synth_fused(s, 7)
    tokens = np.random.default_rng(11).integers(1, s.vocab_size + 1, N)
    logits, taps = fed(RefPass(fw), tokens)
    for a in (tokens, logits, *taps.values()):
        a.setflags(write=False)
    return fw, tokens, logits, taps


def same(a, b):
    return np.abs(a - b).max() <= EQUAL * np.abs(b).max()


@pytest.mark.parametrize("shape", SHAPES)
def test_feeding_in_pieces_is_feeding_at_once(shape):
    fw, tokens, logits, taps = whole(shape)
    p = RefPass(fw)
    parts = [fed(p, t) for t in (tokens[:1], tokens[1:8], tokens[8:])]
    assert p.n == N
    assert rel_err(np.concatenate([lg for lg, _ in parts]), logits).max() <= EQUAL
    for name in ("k", "v"):
        assert same(np.concatenate([t[name] for _, t in parts], axis=1), taps[name])
        assert same(np.stack(getattr(p, name)), taps[name])


@pytest.mark.parametrize("shape", SHAPES)
def test_forks_leave_the_parent_and_each_other_alone(shape):
    fw, tokens, logits, _ = whole(shape)
    rng = np.random.default_rng(12)
    alt1, alt2 = (rng.integers(1, fw.shape.vocab_size + 1, m) for m in (15, 8))
    base = RefPass(fw)
    base.feed(tokens[:20])
    before = [a.copy() for a in base.k + base.v]
    f1, f2 = base.fork(10), base.fork(10)
    l1 = f1.feed(alt1[:9])
    l2 = f2.feed(alt2)
    l1 = np.concatenate([l1, f1.feed(alt1[9:])])
    assert (f1.n, f2.n, base.n) == (25, 18, 20)
    assert all(np.array_equal(a, b) for a, b in zip(base.k + base.v, before))
    assert rel_err(base.feed(tokens[20:]), logits[20:]).max() <= EQUAL
    for got, alt in ((l1, alt1), (l2, alt2)):
        alone = RefPass(fw).feed(np.concatenate([tokens[:10], alt]))
        assert rel_err(got, alone[10:]).max() <= EQUAL


@pytest.mark.parametrize("shape", SHAPES)
def test_given_rows_of_a_causal_run_give_the_causal_run(shape):
    fw, tokens, logits, taps = whole(shape)
    K, V = (taps[name].reshape(fw.shape.n_layers, N, -1) for name in ("k", "v"))
    assert rel_err(RefPass(fw).feed(tokens, attend=Given(K, V)), logits).max() <= EQUAL
    pick = np.array([N, 1, 17, 33, 6])                                   # ragged rows: not consecutive, one of them position 1
    p = RefPass(fw)
    got, gt = fed(p, tokens[pick - 1], pos=pick, attend=Given(K, V))
    assert rel_err(got, logits[pick - 1]).max() <= EQUAL
    assert p.n == 0 and "k" not in gt and "v" not in gt                  # nothing joins the pass's own cache
    # ... whose keys and values are not computed at all: a NaN in the wk | wv rows cannot leak
    w = fw.wqkv.copy()
    w[:, fw.shape.emb_dim:] = np.nan
    nan = RefPass(dataclasses.replace(fw, wqkv=w)).feed(tokens[pick - 1], pick, Given(K, V))
    assert np.array_equal(nan, got)


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_fed_the_c_oracles_rows_gives_the_c_oracles_logits(shape):
    """test_batch_kv16_cpu.py compares forward_fed with forward_all: one pass on both sides.  Here the rows come from an independent
    implementation, so a convention broken in the shared pass (the queries' RoPE, the positions) shows in this family too.  The bar
    is the one test_attn_needle_cpu.py sets for forward_all against the same f32 oracle."""
    import kv16_ref as kr
    from conftest import REL_TOL
    from oracle.oracle import Oracle
    fw, tokens, _, _ = whole(shape)
    o = Oracle(fw, "strict")
    ol = np.array([o.forward(int(t), pos) for pos, t in enumerate(tokens, 1)])
    e = rel_err(kr.forward_fed(fw, tokens, o.key_cache[:, :N], o.value_cache[:, :N]), ol).max()
    print(f"{shape}: forward_fed on the oracle's f32 rows against the oracle's logits: rel_err {e:.2e}")
    assert e <= REL_TOL / 10


@pytest.mark.parametrize("shape", SHAPES)
def test_eps_is_honoured(shape):
    fw, tokens, logits, taps = whole(shape)
    lg, t = fed(RefPass(fw, eps=1e-5), tokens)
    assert np.array_equal(lg, logits) and np.array_equal(t["x"], taps["x"])
    _, t6 = fed(RefPass(fw, eps=1e-6), tokens)
    assert np.abs(t6["x"] - taps["x"]).max() > 1e-9 * np.abs(taps["x"]).max()


@pytest.mark.parametrize("shape", SHAPES)
def test_forward64_and_forward_all_are_one_pass(shape):
    fw, tokens, logits, taps = whole(shape)
    cache = {}
    la, att0 = an.forward_all(fw, tokens, cache=cache)
    f = we.forward64(fw, tokens)
    assert rel_err(f["logits"], la).max() <= EQUAL and rel_err(la, logits).max() <= EQUAL
    for name in ("k", "v"):
        assert same(f[name], np.stack(cache[name]).reshape(f[name].shape))
    for name in ("q", "xb", "hb", "x"):                                  # forward64's other outputs are the last layer's taps
        assert same(f[name], taps[name][-1].reshape(N, -1))
    assert np.allclose(att0.sum(axis=2), 1) and not np.triu(att0, 1).any()


@pytest.mark.parametrize("shape", SHAPES)
def test_a_float32_pass_is_float32_throughout(shape):
    fw, tokens, logits, taps = whole(shape)
    att = Causal(keep_att0=True)
    p = RefPass(fw, np.float32)
    lg, t = fed(p, tokens, attend=att)
    assert set(t) == {"q", "k", "v", "xb", "hb", "x"}
    assert {a.dtype for a in (lg, att.att0, *t.values(), *p.k, *p.v)} == {np.dtype(np.float32)}
    K, V = (t[name].reshape(fw.shape.n_layers, N, -1) for name in ("k", "v"))
    lg2, t2 = fed(RefPass(fw, np.float32), tokens, attend=Given(K.astype(np.float64), V.astype(np.float64)))
    assert {a.dtype for a in (lg2, *t2.values())} == {np.dtype(np.float32)}
    assert rel_err(lg, logits).max() <= 1e-5 and rel_err(lg2, logits).max() <= 1e-5      # (the same model: f32 rounding apart)


def test_rope_freqs_are_the_oracles_f32_values():
    """f32 powf of the f32 exponent (2j+1)/hs: what llmk.py hands the library, not the float64 expression rounded"""
    for hs in (16, 128):
        fr = rope_freqs(hs)
        assert fr.dtype == np.float32 and fr.shape == (hs // 2,) and rope_freqs(hs) is fr
        f64 = 1.0 / 10000.0 ** ((2 * np.arange(hs // 2) + 1) / hs)
        # rounding the exponent (<= 1) to f32 moves the power by up to ln(10000) = 9.2 half-ulps, powf and the division one each
        assert np.abs(fr / f64 - 1).max() < 12 * 2.0 ** -24
