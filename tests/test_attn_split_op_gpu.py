"""The decode attention kernels as an OPERATOR: after llmk_forward on the multi-kernel path, llmk_peek 1 | 2 hold the last layer's
rotated q and its attention output and 4 | 5 its K / V rows, and the output is compared with the float64 softmax of those very
inputs (tests/attn_op_ref.py).  One-layer needle models, f32 weights; every case runs under attn_kernel (LLMK_ATTN_SPLIT unset, the
established kernel and the non-finite rule's origin) and under the split pair of csrc/attn_split.h (LLMK_ATTN_SPLIT=1).

What the whole-model comparison of tests/test_attn_split_gpu.py cannot see: head size 32 and kv_mul 16 (all 16 MFMA columns live),
a query 16,400 rows deep at 64 parts (17 tiles per part, waves with 3 and 2 tiles, a part with 5, three empty parts), and the
non-finite rule -- one NaN anywhere makes every logit NaN, but an operator's NaN pattern is head by head and element by element.
The bar is the project's REL_TOL, of the position's max |xb|."""
import numpy as np
import pytest

import attn_needle as an
import attn_op_ref as ao
from conftest import REL_TOL, rel_err
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf

pytestmark = pytest.mark.gpu

S_GRID = 424
GRID = [(32, 1, 2), (32, 5, 2), (16, 16, 2), (64, 16, 1), (128, 2, 4), (64, 9, 2)]      # (head size, kv_mul, kv heads)
KERNELS = [None, "1"]                                                                   # LLMK_ATTN_SPLIT: attn_kernel, the split pair
KERNEL_NAMES = {None: "attn_kernel", "1": "split"}


def needle_model(hs, kv_mul, nkv, S, layout, beta=an.BETA):
    """one-layer needle weights and the S tokens; layout: kv head -> needle rows (kv head 1's join head 0's where there is one head)"""
    s = gguf.LlamaShape(hs * kv_mul * nkv, 64, 1, kv_mul * nkv, nkv, 320, S)
    if nkv == 1:
        layout = {0: sorted(layout[0] + layout[1])}
    tokens, needle_tokens = an.needle_sequence(s, layout, 20261127)
    return an.shape_needles(gguf.synth_fused(s, 4242), needle_tokens, beta), tokens


def set_kernel(monkeypatch, value):
    monkeypatch.delenv("LLMK_ATTN_SPLIT", raising=False) if value is None else monkeypatch.setenv("LLMK_ATTN_SPLIT", value)


def peek_op(m):
    """(q [nh][hs], xb [nh][hs]) of the last layer at the position just fed"""
    s = m.shape
    return m.peek(1, s.emb_dim).reshape(s.n_heads, s.head_size), m.peek(2, s.emb_dim).reshape(s.n_heads, s.head_size)


def op_err(xb, ref):
    return float(rel_err(xb.reshape(1, -1), ref.reshape(1, -1))[0])


@pytest.mark.parametrize("hs,kv_mul,nkv", GRID, ids=lambda v: str(v))
def test_finite_operator_grid(hs, kv_mul, nkv, monkeypatch):
    P = an.ats_parts(nkv, S_GRID)
    fw, tokens = needle_model(hs, kv_mul, nkv, S_GRID, {0: [0, 15, 16 * P, S_GRID - 1], 1: [16, 17, 16 * P - 1]})
    at = sorted({1, 15, 16, 17, 16 * P - 16, 16 * P, 16 * P + 1, S_GRID - 1, S_GRID})
    worst = {}
    for kernel in KERNELS:
        set_kernel(monkeypatch, kernel)
        m = llmk.Llmk(fw, flags=llmk.FLAG_MULTI_KERNEL)
        errs = {}
        for pos, tok in enumerate(tokens, 1):
            m.forward(int(tok), pos)
            if pos in at:
                q, xb = peek_op(m)
                K, V = ao.peek_rows(m, 0, pos, fw.shape.kv_dim)
                ao.assert_modest(q, K, V)
                errs[pos] = op_err(xb, ao.attn_op(q, K, V, kv_mul))
        m.close()
        worst[kernel] = max(errs.values())
        print(f"hs {hs} kv_mul {kv_mul} nkv {nkv} P {P} {KERNEL_NAMES[kernel]}: max rel err {worst[kernel]:.2e} {errs}")
    print(f"hs {hs} kv_mul {kv_mul} nkv {nkv}: split / attn_kernel = {worst['1'] / max(worst[None], 1e-30):.2f}")
    assert worst[None] <= REL_TOL and worst["1"] <= REL_TOL, worst


# 65,536 positions, 64 parts.  Position 16,400: 1,025 tiles, 17 per part -- parts 0 .. 59 full (wave 0 takes 3 tiles, the others 2),
# part 60 holds 5, parts 61 .. 63 are empty.
DEEP_S, DEEP_POS = 65536, 16400
# At head size 16 the needles' RoPE pair turns by 2.9 rad over this depth: only the needles near the query score high (3 * beta), and
# at attn_needle.BETA they would hold all of the mass -- a tile lost in part 1 would move nothing.  At beta 3 they score 9 and hold
# about as much as the 16,400 fillers together, so every part's 272 rows carry ~0.5% of the mass and a needle still a third of it.
DEEP_BETA = 3.0


def test_a_deep_position_at_64_parts():
    hs, kv_mul, nkv = 16, 4, 2
    P = an.ats_parts(nkv, DEEP_S)
    tiles = -(-DEEP_POS // 16)
    tpp = -(-tiles // P)
    assert (P, tiles, tpp, tiles - 60 * tpp) == (64, 1025, 17, 5)
    rpp = 16 * tpp                                                      # rows per part: 272
    layout = {0: [0] + [rpp * p - 1 for p in (1, 30, 60)] + [16384, DEEP_POS - 1], 1: [rpp * p for p in (1, 30, 60)] + [16383]}
    fw, tokens = needle_model(hs, kv_mul, nkv, DEEP_S, layout, DEEP_BETA)
    KV = fw.shape.kv_dim
    m = llmk.Llmk(fw, flags=llmk.FLAG_MULTI_KERNEL)                     # (attn_kernel cannot hold this context: the split pair runs)
    m.prefill(tokens[:DEEP_POS - 1], 1)
    K = np.zeros((DEEP_POS + 17, KV), np.float32)
    V = np.zeros_like(K)
    K[:DEEP_POS - 1], V[:DEEP_POS - 1] = ao.peek_rows(m, 0, DEEP_POS - 1, KV)
    errs, have = {}, DEEP_POS - 1
    for pos in range(DEEP_POS, DEEP_POS + 18):
        m.forward(int(tokens[pos - 1]), pos)
        if pos in (DEEP_POS, DEEP_POS + 1, DEEP_POS + 17):
            K[have:pos], V[have:pos] = ao.peek_rows(m, 0, pos, KV, first=have + 1)
            have = pos
            q, xb = peek_op(m)
            ao.assert_modest(q, K[:pos], V[:pos])
            errs[pos] = op_err(xb, ao.attn_op(q, K[:pos], V[:pos], kv_mul))
    m.close()
    print(f"depth {DEEP_POS}, P {P}, {tpp} tiles per part: max rel err {max(errs.values()):.2e} {errs}")
    assert max(errs.values()) <= REL_TOL, errs


def check_against_rule(xb, ref, where):
    """a position's device output against the plain softmax's: the NaN pattern element for element, infinities with sign, finite
    elements within the bar of the position's largest finite |ref|"""
    assert np.array_equal(np.isnan(xb).any(axis=1), np.isnan(ref).any(axis=1)), (where, "heads with a NaN", xb, ref)
    assert np.array_equal(np.isnan(xb), np.isnan(ref)), (where, "NaN pattern", np.argwhere(np.isnan(xb) != np.isnan(ref)))
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(xb), inf) and np.array_equal(xb[inf], ref[inf]), (where, "infinities")
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0
    err = float(np.abs(xb[fin] - ref[fin]).max() / np.abs(ref[fin]).max())
    assert err <= REL_TOL, (where, err)
    return err


@pytest.mark.parametrize("kernel", KERNELS, ids=lambda k: KERNEL_NAMES[k])
@pytest.mark.parametrize("layout", list(ao.POISON_LAYOUTS))
@pytest.mark.parametrize("hs", [16, 64])
def test_the_non_finite_rule_is_the_plain_softmaxes(hs, layout, kernel, monkeypatch):
    """Every position of the poison sequence (attn_op_ref.shape_poison) is a query.  At each, heads 0 .. 3 of kv group 0 stand in
    different classes in ONE MFMA tile of the split form; kv group 1 stays finite: one column's NaN must not reach another kv head.
    Layout "late" puts the first poison in row 16: at position 17 head 2's NaN score is alone in its tile, in a wave that has seen
    nothing finite, beside a wave with finite scores only (attn_tiles' STRICT).

    The last position is apart: its newest row holds +inf in one V element of kv head 1 and every score of the group is finite, so
    the plain softmax gives +inf in that element.  Neither kernel does.  Both read the rows of a ragged batch with the row index
    clamped to the newest row and give the rows past it the weight 0: 0 * inf is NaN.  attn_kernel's batch is 1,024 | 256 rows at
    head sizes 16 | 64 and attn_split's tile 16, so the element is NaN at any position that is no multiple of that; position 79 is
    none of either.  Measured on an MI355X for both kernels and both head sizes: NaN in that element of all four heads, every other
    element within the bar.  Non-finite V in the newest row is in nobody's contract (csrc/attn_split.h, NON-FINITE SCORES)."""
    fw, tokens = ao.build_poison(hs, layout)
    KV, kv_mul = fw.shape.kv_dim, 4
    set_kernel(monkeypatch, kernel)
    m = llmk.Llmk(fw, flags=llmk.FLAG_MULTI_KERNEL)
    K = np.zeros((len(tokens), KV), np.float32)
    V = np.zeros_like(K)
    seen, worst = set(), 0.0
    for pos, tok in enumerate(tokens, 1):
        m.forward(int(tok), pos)
        K[pos - 1], V[pos - 1] = m.peek(4, KV, 0, pos), m.peek(5, KV, 0, pos)
        q, xb = peek_op(m)
        ao.assert_modest(q, K[:pos], V[:pos])
        ref = ao.attn_op(q, K[:pos], V[:pos], kv_mul)
        cls = ao.classify(q, K[:pos], kv_mul)
        for h, c in enumerate(cls):
            seen.add((c, bool(np.isfinite(xb[h]).all())))
        assert np.isfinite(K[:pos].reshape(pos, 2, hs)[:, 1]).all() and cls[5:] == ["finite"] * 3
        if pos < ao.POISON_N:
            worst = max(worst, check_against_rule(xb, ref, (pos, cls)))
            assert np.isfinite(xb[4:]).all() == (cls[4] == "finite") and np.isfinite(xb[5:]).all(), (pos, "kv group 1")
        else:
            d1 = ao.POISON_D1
            assert V[pos - 1, hs + d1] == np.inf and (ref[4:, d1] == np.inf).all() and pos % 16 and pos % an.attn_kernel_tiles(hs)[1]
            print(f"newest row's V element is +inf, scores finite: xb[4:8][{d1}] = {xb[4:, d1]}, the plain softmax's {ref[4:, d1]}")
            assert np.isnan(xb[4:, d1]).all(), xb[4:, d1]
            rest = np.ones(hs, bool)
            rest[d1] = False
            worst = max(worst, check_against_rule(xb[:, rest], ref[:, rest], (pos, cls)))
    m.close()
    print(f"hs {hs} {layout} {KERNEL_NAMES[kernel]}: max rel err of the finite elements {worst:.2e}; classes seen {sorted(seen)}")
    ao.coverage(seen)
