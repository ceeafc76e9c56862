"""Spans for the batched decode (llmk_span_*): several consecutive positions of a slot in one pass.  What is
new on the device is bd_attn_span_kernel -- (position of the span, query head) pairs as the MFMA columns, a causal predicate per
column, a tile range that starts at the slot's first own row; every test reaches it through the public entry points.

  1  ragged spans (1, rg-1, rg, rg+1, 2 rg+1 rows and one that crosses a tile boundary mid-slot) against the float64 pass
  2  a long slot fed in spans of 125 next to three decoding slots; the last passes run several parts
  3  the causal edge: later rows of a span do not reach earlier ones; needles on every group, tile and part boundary
  4  attached slots (P = 15, 16, 17) against the forked form; f16 caches against the stored-row contract and the fed float64 pass
  5  code-path claims: len 1 IS llmk_batch_forward, the same call twice, LLMK_SPAN_ATTN=0, LLMK_SPAN_LAST
  6  the verification flow: 12 drafted tokens in one pass; a rejected tail costs nothing
  7  refusals
"""
import ctypes as C
import os

import numpy as np
import pytest

import attn_needle as an
import batch_tiles as bt
import kv16_ref as kr
import prefix_tiles as pt
import span_tiles as st
from conftest import REL_TOL, rel_err, top8_elementwise
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf
from ref_pass import RefPass

pytestmark = pytest.mark.gpu


def first_max(rows):
    return np.argmax(np.asarray(rows), axis=-1).astype(np.int32) + 1      # (np.argmax: the first maximum)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def model(shape, wtype=gguf.GGML_F32, q6k=False, seed=777):
    """(weights for the device, the same decoded to f32 for the reference)"""
    fw = gguf.synth_fused(gguf.SHAPES[shape] if isinstance(shape, str) else shape, seed, wtype)
    if q6k:
        fw = gguf.with_q6k_classifier(fw)
    return fw, (fw.as_f32() if (wtype or q6k) else fw)


def within_the_bar(what, got, ref):
    err, e8 = rel_err(got, ref), top8_elementwise(got, ref=ref)
    print(f"{what}: {len(err)} rows, rel_err max {err.max():.2e} at row {int(np.argmax(err))}, top-8 max {e8.max():.2e}")
    assert err.max() <= REL_TOL, (what, err.max(), int(np.argmax(err)))
    assert e8.max() <= REL_TOL, (what, e8.max(), int(np.argmax(e8)))


def random_seq(rng, V, n):
    return [2] + (rng.integers(3, V, n - 1) + 1).tolist()


def run_passes(b, seqs, passes, V):
    """passes: [[(slot, pos0, len)]]; slot j feeds seqs[j].  Returns the logits of every position of every slot (NaN: not fed)."""
    got = [np.full((len(seq), V), np.nan, np.float32) for seq in seqs]
    for t, spans in enumerate(passes):
        toks = [seqs[slot][pos0 - 1 + j] for slot, pos0, n in spans for j in range(n)]
        lg, am = b.forward_spans(spans, toks)
        assert np.array_equal(am, first_max(lg)), (t, spans)
        row = 0
        for slot, pos0, n in spans:
            got[slot][pos0 - 1:pos0 - 1 + n] = lg[row:row + n]
            row += n
    return got


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
ROW_CASES = {
    "tiny-hs128w-f32": ("tiny-hs128w", gguf.GGML_F32, False),      # kv_mul 1: 16 rows per column group
    "tiny-hs64-f32": ("tiny-hs64", gguf.GGML_F32, False),          # 2: 8
    "tiny-kvmul3-f32": ("tiny-kvmul3", gguf.GGML_F32, False),      # 3: 5 and one padded column
    "tiny-gqa-f32": ("tiny-gqa", gguf.GGML_F32, False),            # 4: 4
    "tiny-70bish-f32": ("tiny-70bish", gguf.GGML_F32, False),      # 8: 2, one kv head
    "tk-small-f16": ("tk-small", gguf.GGML_F16, False),
    "tk-small-q4_0": ("tk-small", gguf.GGML_Q4_0, False),
    "tk-small-q4_0-q6k": ("tk-small", gguf.GGML_Q4_0, True),
}
MID = (15, 3)          # a span at pos0 15 of 3 rows: cache rows 14, 15 | 16 -- it crosses the first tile boundary


def ragged_passes(s):
    """Slots 0..4 take spans of 1, rg-1, rg, rg+1 and 2 rg+1 rows from position 1 in pass 1, slot 5 -- 14 positions into its sequence
    after pass 0 -- the span MID; passes 2 and 3 continue every slot with the lengths rotated (cut at seq_len).  Spans are listed by
    DESCENDING slot.  Returns (sequence lengths, passes)."""
    rg = pt.rg(s.n_heads // s.n_kv_heads)
    lens = [1, max(1, rg - 1), rg, rg + 1, 2 * rg + 1]
    at = [0] * 5 + [MID[0] - 1]
    passes = [[(5, 1, MID[0] - 1)]]
    for t in range(3):
        spans = []
        for j in range(6):
            n = min(MID[1] if j == 5 else lens[(j + t) % 5], s.seq_len - at[j])
            if n > 0:
                spans.append((j, at[j] + 1, n))
                at[j] += n
        passes.append(sorted(spans, key=lambda x: -x[0]))
    assert sorted(n for _, _, n in passes[1][1:]) == sorted(lens) and passes[1][0] == (5,) + MID
    assert all(sum(n for _, _, n in p) <= 128 for p in passes)
    return at, passes


@pytest.mark.parametrize("cid", list(ROW_CASES))
def test_ragged_spans_match_the_float64_pass_on_each_sequence_alone(cid):
    shape, wtype, q6k = ROW_CASES[cid]
    fw, fw32 = model(shape, wtype, q6k)
    s = fw.shape
    lens, passes = ragged_passes(s)
    rng = np.random.default_rng(5)
    seqs = [random_seq(rng, s.vocab_size, n) for n in lens]
    ref = [RefPass(fw32).feed(seq) for seq in seqs]
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 6)
    got = run_passes(b, seqs, passes, s.vocab_size)
    b.close()
    m.close()
    assert not np.isnan(np.concatenate(got)).any()
    for j in range(6):
        within_the_bar(f"{cid} slot {j}", got[j], ref[j])


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def test_a_long_slot_in_spans_of_125_next_to_three_decoding_slots():
    """tk-small-long: 700 tokens into slot 0 in spans of 125 (the last one 75) while slots 1..3 take one row each in the same passes;
    every row against the float64 pass.  The last passes run more than one part (tests/span_tiles.py)."""
    fw, fw32 = model("tk-small-long")
    s = fw.shape
    rng = np.random.default_rng(11)
    n_long, chunk = 700, 125
    n_pass = -(-n_long // chunk)
    seqs = [random_seq(rng, s.vocab_size, n_long)] + [random_seq(rng, s.vocab_size, n_pass) for _ in range(3)]
    ref = [RefPass(fw32).feed(seq) for seq in seqs]
    passes = [[(3, t + 1, 1), (2, t + 1, 1), (1, t + 1, 1), (0, t * chunk + 1, min(chunk, n_long - t * chunk))] for t in range(n_pass)]
    parts = [st.span_parts(p, s.n_kv_heads, s.n_heads // s.n_kv_heads)[0] for p in passes]
    print("parts per pass", parts)
    assert parts[0] == 1 and min(parts[-2:]) > 1, parts
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 4)
    got = run_passes(b, seqs, passes, s.vocab_size)
    b.close()
    m.close()
    for j in range(4):
        assert not np.isnan(got[j]).any()
        within_the_bar(f"slot {j}", got[j], ref[j])


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def test_later_rows_of_a_span_do_not_reach_earlier_ones():
    """[a, b, c, d] against [a, b, x, y] into fresh slots: rows 0 and 1 bit-identical, rows 2 and 3 different"""
    fw, _ = model("tiny-hs64")
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 2)
    one = b.forward_spans([(0, 1, 4)], [2, 50, 60, 70], want_argmax=False)
    two = b.forward_spans([(1, 1, 4)], [2, 50, 61, 71], want_argmax=False)
    b.close()
    m.close()
    assert np.array_equal(bits(one[:2]), bits(two[:2]))
    assert (bits(one[2]) != bits(two[2])).any() and (bits(one[3]) != bits(two[3])).any()


NEEDLE_SHAPES = {"tk-small-long": 704, "tiny-hs128w-long": 320}
NEEDLE_CHUNK = 125
NEEDLE_SEED = 20261021


def needle_case(shape):
    """The sequence goes into one slot in spans of 125; the last span is the one under test.  Needles of kv heads 0 | 1 on the two
    sides of: the first tile boundary (15 | 16); the last pass's first two part boundaries; the last span's first row (the row before
    it came from an earlier pass | the span's own first row); its first two group boundaries (own earlier rows of the span on both
    sides); and the sink and the last row."""
    S = NEEDLE_SHAPES[shape]
    s0 = gguf.SHAPES[shape]
    s = gguf.LlamaShape(s0.emb_dim, s0.hidden_dim, s0.n_layers, s0.n_heads, s0.n_kv_heads, s0.vocab_size, S)
    kv_mul = s.n_heads // s.n_kv_heads
    rg = pt.rg(kv_mul)
    passes = [[(0, p0, min(NEEDLE_CHUNK, S - p0 + 1))] for p0 in range(1, S + 1, NEEDLE_CHUNK)]
    parts, tpp = st.span_parts(passes[-1], s.n_kv_heads, kv_mul)
    assert parts >= 3, parts
    r0 = passes[-1][0][1] - 1                            # the last span's first cache row
    assert passes[-1][0][2] > 2 * rg + 1
    pb = [p * tpp * bt.BD_TILE for p in (1, 2)]
    lay = {0: {0, bt.BD_TILE - 1, pb[0] - 1, pb[1] - 1, r0 - 1, r0 + rg - 1, r0 + 2 * rg - 1, S - 1},
           1: {bt.BD_TILE, pb[0], pb[1], r0, r0 + rg, r0 + 2 * rg}}
    assert not lay[0] & lay[1] and max(pb) < r0, (lay, pb, r0)
    layout = {g: sorted(ts) for g, ts in lay.items()}
    tokens, needle_tokens = an.needle_sequence(s, layout, NEEDLE_SEED)
    fw = an.shape_needles(gguf.synth_fused(s, 4242), needle_tokens, an.BETA)
    return s, layout, tokens, fw, passes


@pytest.mark.parametrize("shape", list(NEEDLE_SHAPES))
def test_span_attention_on_needles(shape):
    s, layout, tokens, fw, passes = needle_case(shape)
    S = s.seq_len
    ref, att0 = an.forward_all(fw, tokens)
    for g, ts in layout.items():                     # the needles do hold the mass where a query sees one of its head
        h = g * (s.n_heads // s.n_kv_heads)
        assert att0[h, S - 1, ts].sum() > 0.999, (g, att0[h, S - 1, ts].sum())
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 1)
    got = run_passes(b, [tokens.tolist()], passes, s.vocab_size)[0]
    b.close()
    m.close()
    within_the_bar(f"{shape} needles {layout}", got, ref)
    safe = an.safe_argmax_positions(ref)
    assert safe.sum() > len(safe) // 2
    assert np.array_equal(np.argmax(got, axis=1)[safe], np.argmax(ref, axis=1)[safe])


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["tiny-hs64", "tiny-kvmul3"])
def test_a_span_behind_a_prefix_against_the_forked_form_and_the_float64_pass(shape):
    """P = 15, 16, 17: slot 0 attached, slot 1 forked at P, slot 2 fresh; spans of 2 rg + 1 rows at P+1.., then rg + 1 more, the
    attached and the unattached slots in ONE pass (a mixed pass folds part states for every row)."""
    fw, fw32 = model(shape)
    s = fw.shape
    rg = pt.rg(s.n_heads // s.n_kv_heads)
    n1, n2 = 2 * rg + 1, rg + 1
    rng = np.random.default_rng(9)
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 3)
    for P in (15, 16, 17):
        seq = random_seq(rng, s.vocab_size, P + n1 + n2)
        other = random_seq(rng, s.vocab_size, 3)
        ref, oref = RefPass(fw32).feed(seq), RefPass(fw32).feed(other)
        m.prefill(seq[:P], 1)
        for j in range(3):
            b.fork(j, P if j == 1 else 0)
        b.set_prefix(P)
        b.attach(0)
        a = b.forward_spans([(2, 1, 3), (1, P + 1, n1), (0, P + 1, n1)], other + seq[P:P + n1] * 2, want_argmax=False)
        c = b.forward_spans([(0, P + n1 + 1, n2), (1, P + n1 + 1, n2)], seq[P + n1:] * 2, want_argmax=False)
        within_the_bar(f"{shape} P {P} fresh", a[:3], oref)
        frk, att = np.concatenate([a[3:3 + n1], c[n2:]]), np.concatenate([a[3 + n1:], c[:n2]])
        within_the_bar(f"{shape} P {P} forked", frk, ref[P:])
        within_the_bar(f"{shape} P {P} attached", att, ref[P:])
        within_the_bar(f"{shape} P {P} attached against forked", att, frk)
        b.fork(0, 0)
        b.set_prefix(0)
    b.close()
    m.close()


def test_an_f16_batch_stores_the_rounded_rows_and_matches_the_float64_pass_fed_them():
    fw, fw32 = model("tk-small")
    s = fw.shape
    lens, passes = ragged_passes(s)
    rng = np.random.default_rng(6)
    seqs = [random_seq(rng, s.vocab_size, n) for n in lens]
    m = llmk.Llmk(fw)
    b32, b16 = llmk.Batch(m, 6), llmk.Batch(m, 6, kv_type="f16")
    run_passes(b32, seqs, passes, s.vocab_size)
    got = run_passes(b16, seqs, passes, s.vocab_size)
    moved = 0
    for j, seq in enumerate(seqs):
        for which in (0, 1):      # layer 0's rows depend on token and position only: there the f16 batch holds exactly the rounded f32 rows
            x, h = b32.peek_kv(which, 0, j, 1, len(seq)), b16.peek_kv(which, 0, j, 1, len(seq))
            assert np.array_equal(bits(h), bits(kr.stored_half(x))), (j, which)
            moved += int((bits(h) != bits(x)).sum())
        K, V = kr.peek_all(b16, s.n_layers, j, len(seq))
        within_the_bar(f"f16 caches slot {j}", got[j], kr.forward_fed(fw32, seq, K, V))
    assert moved > 0
    b16.close()
    b32.close()
    m.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def test_code_path_claims():
    fw, _ = model("tiny-hs64")
    s = fw.shape
    rng = np.random.default_rng(3)
    seqs = [random_seq(rng, s.vocab_size, 30) for _ in range(3)]
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 6)
    # spans of one row each ARE llmk_batch_forward
    for pos in (1, 2, 3):
        toks = [seqs[j][pos - 1] for j in range(3)]
        lg, am = b.forward([2, 0, 1], [toks[2], toks[0], toks[1]], [pos] * 3)
        lg2, am2 = b.forward_spans([(5, pos, 1), (3, pos, 1), (4, pos, 1)], [toks[2], toks[0], toks[1]])
        assert np.array_equal(bits(lg), bits(lg2)) and np.array_equal(am, am2), pos
    # the same call twice from the same state; LLMK_SPAN_LAST against the full call
    spans = [(1, 4, 20), (0, 4, 9), (2, 4, 1)]
    toks = seqs[1][3:23] + seqs[0][3:12] + seqs[2][3:4]
    lg, am = b.forward_spans(spans, toks)
    lg2, am2 = b.forward_spans(spans, toks)
    assert np.array_equal(bits(lg), bits(lg2)) and np.array_equal(am, am2)
    last = [19, 28, 29]
    lgl, aml = b.forward_spans(spans, toks, last_only=True)
    assert lgl.shape == (3, s.vocab_size) and np.array_equal(bits(lgl), bits(lg[last])) and np.array_equal(aml, am[last])
    assert np.array_equal(b.forward_spans(spans, toks, last_only=True, want_logits=False), am[last])
    # the per-row attention kernels under the same entry point
    os.environ["LLMK_SPAN_ATTN"] = "0"
    try:
        b0 = llmk.Batch(m, 6)
    finally:
        del os.environ["LLMK_SPAN_ATTN"]
    for pos in (1, 2, 3):
        b0.forward([0, 1, 2], [seqs[j][pos - 1] for j in range(3)], [pos] * 3)
    lg0, am0 = b0.forward_spans(spans, toks)
    within_the_bar("LLMK_SPAN_ATTN=0 against the default", lg0, lg.astype(np.float64))
    assert b.time_spans(2, 9, 4, 2) > 0.0 and b0.time_spans(2, 9, 4, 2) > 0.0
    # ingest = the same positions in spans: the last position's logits
    b.fork(3, 0)
    assert np.array_equal(bits(b.ingest(3, seqs[1][:23])), bits(b.forward_spans([(4, 1, 23)], seqs[1][:23], want_argmax=False)[-1]))
    b0.close()
    b.close()
    m.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
PROMPT = [2, 40, 41, 42, 43, 44]
DRAFT = 12


@pytest.mark.parametrize("shape,seed", [("tk-small", 777), ("tiny-hs128w", 31)])
def test_verification_flow(shape, seed):
    """12 greedy ids from llmk_batch_decode; [last prompt token] + ids[:11] as one span into a fresh fork: argmax_out == ids (the
    float64 reference's smallest top-1 margin over these steps is 2.9e-2 | 1.0e-2 of max |logit|, far above the 4e-4 rule).  Then
    drafts that are wrong from index 5 on: the accepted rows' picks stand, and continuing from the accepted position with the right
    token stays within the bar of the clean sequence -- the dead rows were rewritten."""
    fw, _ = model(shape, seed=seed)
    s = fw.shape
    P = len(PROMPT) - 1
    m = llmk.Llmk(fw)
    m.prefill(PROMPT[:P], 1)
    b = llmk.Batch(m, 3)
    for j in range(3):
        b.fork(j, P)
    ids = b.decode([0], [PROMPT[P]], [P + 1], DRAFT)[0]
    clean, am = b.forward_spans([(1, P + 1, DRAFT)], [PROMPT[P]] + ids[:DRAFT - 1].tolist())
    assert np.array_equal(am, ids), (am, ids)
    drafts = ids[:DRAFT - 1].copy()
    drafts[5:] = (drafts[5:] + 6) % s.vocab_size + 1
    assert (drafts[5:] != ids[5:DRAFT - 1]).all()
    am = b.forward_spans([(2, P + 1, DRAFT)], [PROMPT[P]] + drafts.tolist(), want_logits=False)
    assert np.array_equal(am[:6], ids[:6])               # rows 0..5 fed the right tokens; the caller accepts positions P+1 .. P+6
    lg = b.forward_spans([(2, P + 7, DRAFT - 6)], ids[5:DRAFT - 1].tolist(), want_argmax=False)
    within_the_bar(f"{shape} behind a rejected tail", lg, clean[6:].astype(np.float64))
    b.close()
    m.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def raw_forward(b, spans, tokens, flags=0, logits=True, argmax=True, null_spans=False, null_tokens=False, n_spans=None):
    """llmk_span_forward with nothing checked on the way: the return code"""
    n = len(spans) if n_spans is None else n_spans
    sp = (llmk.Span * max(1, len(spans)))(*[llmk.Span(*x) for x in spans])
    tok = (C.c_int * max(1, len(tokens)))(*tokens)
    lg = np.zeros((256, b.V), np.float32)
    am = np.zeros(256, np.int32)
    return llmk.lib().llmk_span_forward(b._h, n, None if null_spans else sp, None if null_tokens else tok, flags,
                                        lg.ctypes.data_as(C.POINTER(C.c_float)) if logits else None,
                                        am.ctypes.data_as(C.POINTER(C.c_int)) if argmax else None)


def test_refusals_leave_the_caches_unchanged():
    E_ARG = 1
    fw, _ = model("tk-small", seed=1)
    s = fw.shape
    V = s.vocab_size
    m = llmk.Llmk(fw)
    prompt = [2] + list(range(40, 58))
    P = len(prompt)
    m.prefill(prompt, 1)
    b = llmk.Batch(m, 5, 32)
    b.forward_spans([(0, 1, 8), (1, 1, 8)], [5] * 16)

    def snapshot():
        return [bits(b.peek_kv(w, l, j, 1, 32)) for w in (0, 1) for l in range(s.n_layers) for j in range(5)]
    ms = C.c_float()
    tm = lambda *a: llmk.lib().llmk_span_time(b._h, *a, C.byref(ms))
    before = snapshot()
    # 129 rows: four slots of 32 positions and one row more (a pass of 128 rows runs: the last check of this test)
    assert raw_forward(b, [(j, 1, 32) for j in (4, 3, 1, 0)] + [(2, 1, 1)], [5] * 129) == E_ARG
    assert tm(5, 26, 1, 1) == E_ARG
    assert all(np.array_equal(x, y) for x, y in zip(before, snapshot()))
    b.set_prefix(P)
    b.attach(2)
    b.forward_spans([(2, P + 1, 4)], [7] * 4)
    before = snapshot()
    ok = [(0, 9, 2)]
    cases = {
        "null spans": dict(spans=ok, tokens=[5, 5], null_spans=True),
        "null tokens": dict(spans=ok, tokens=[5, 5], null_tokens=True),
        "no span": dict(spans=ok, tokens=[5, 5], n_spans=0),
        "negative span count": dict(spans=ok, tokens=[5, 5], n_spans=-1),
        "len 0": dict(spans=[(0, 9, 0), (1, 9, 2)], tokens=[5, 5]),
        "len -1": dict(spans=[(0, 9, -1)], tokens=[5, 5]),
        "slot 5": dict(spans=[(5, 9, 2)], tokens=[5, 5]),
        "slot -1": dict(spans=[(-1, 9, 2)], tokens=[5, 5]),
        "a slot twice": dict(spans=[(0, 9, 2), (0, 11, 2)], tokens=[5] * 4),
        "pos0 0": dict(spans=[(0, 0, 2)], tokens=[5, 5]),
        "past seq_len": dict(spans=[(0, 31, 3)], tokens=[5] * 3),
        "pos0 past seq_len": dict(spans=[(0, 33, 1), (1, 9, 2)], tokens=[5] * 3),
        "attached at P": dict(spans=[(2, P, 2)], tokens=[5, 5]),
        "attached at 1": dict(spans=[(2, 1, 2)], tokens=[5, 5]),
        "token 0": dict(spans=ok, tokens=[5, 0]),
        "token V+1": dict(spans=ok, tokens=[V + 1, 5]),
        "flag 2": dict(spans=ok, tokens=[5, 5], flags=2),
        "flag 3": dict(spans=ok, tokens=[5, 5], flags=3),
        "no output": dict(spans=ok, tokens=[5, 5], logits=False, argmax=False),
    }
    for what, kw in cases.items():
        assert raw_forward(b, **kw) == E_ARG, what
        assert all(np.array_equal(x, y) for x, y in zip(before, snapshot())), what
    for what, a in {"no span": (0, 2, 9, 1), "6 slots": (6, 2, 20, 1), "len 0": (1, 0, 9, 1), "pos0 0": (1, 2, 0, 1), "past seq_len": (1, 3, 31, 1),
                    "no iteration": (1, 2, 9, 0), "slot 2 is attached": (3, 2, P, 1)}.items():
        assert tm(*a) == E_ARG, what
        assert all(np.array_equal(x, y) for x, y in zip(before, snapshot())), what
    assert llmk.lib().llmk_span_time(b._h, 1, 2, 9, 1, None) == E_ARG
    assert raw_forward(b, ok, [5, 5]) == 0 and raw_forward(b, [(2, P + 5, 2), (1, 9, 2)], [5] * 4, flags=1) == 0      # the batch stays usable
    assert tm(2, 2, 9, 1) == 0 and ms.value > 0.0
    b.fork(2, 0)
    assert raw_forward(b, [(j, 1, 32) for j in (4, 3, 1, 0)], [5] * 128, flags=1) == 0                                 # 128 rows in 5 slots
    b.close()
    m.close()
