"""A batch with q8_0 K/V caches (llmk_cache_create with LLMK_TYPE_Q8_0).  What is new on the device: the K/V
write that quantises a block of 32 across 8 lanes (bd_epi_qkv_q8_kernel), the converting copy of fork and prefix (bd_to_q8_kernel),
the loader that dequantises in registers (AttnAhead<HS, KvQ8>) and the four attention kernels over it (bd_q8_attn_*).  Stored rows
are compared BIT FOR BIT with kvq8_ref.stored_q8 of what the f32 path stores; logits are compared at REL_TOL with forward_fed, the
float64 forward pass fed the rows the device stored (tests/test_batch_kvq8_cpu.py proves that yardstick and prints the movement).
The tests of tests/test_batch_kv16_gpu.py, restated with stored_half -> stored_q8 and "representable" -> "idempotent under stored_q8":

   1  stored rows of ragged passes: layer 0 exactly stored_q8 of the f32 rows, every layer idempotent
   2  ragged rows, joining and leaving, against forward_fed
   3  fork and prefix conversion, all layers exact; an emptied slot is a fresh slot
   4  tile and part boundaries: the wide transcript passes, each twice
   5  needles where a wave's second tile and a wide pass's parts begin
   6  a shared prefix of 15 | 16 | 17 | 33 positions, 1 | RG | RG + 1 attached rows next to a forked one
   7  spans: ragged spans against forward_fed, later rows do not reach earlier ones, LLMK_SPAN_ATTN=0
   8  decode: picks and records are what the hooks answer on a replay's logits
   9  an f32 and an f16 batch next to a q8_0 one keep their bits; bytes; another computation of the same model
  10  saturation: values beyond 65504 are stored as +-127 d with d finite
  11  a redone call rewrites q8_0 rows; refusals
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import attn_needle as an
import batch_tiles as bt
import kvq8_ref as kq
import prefix_tiles as pt
from conftest import REL_TOL, ROOT, load_golden, rel_err
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf
from test_batch_kv16_gpu import (PENALTIES, PROMPT, ROW_CASES, SAMPLERS, STEPS, TOP_N, bits, code_of, first_max, model, ragged, run_ragged,
                                 small_weights, within_the_bar)
from test_batch_kvq8_cpu import movement
from test_batch_span_gpu import ragged_passes, random_seq, run_passes

pytestmark = pytest.mark.gpu

Q8 = "q8_0"


def cache_units(s, n_slots, seq_len=None):
    """K and V elements of a batch's caches"""
    return 2 * s.n_layers * n_slots * (seq_len or s.seq_len) * s.kv_dim


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
STORED_CASES = {"tiny-gqa": ("tiny-gqa", gguf.GGML_F32), "tiny-kvmul3": ("tiny-kvmul3", gguf.GGML_F32), "tiny-hs64": ("tiny-hs64", gguf.GGML_F32),
                "tiny-hs128w": ("tiny-hs128w", gguf.GGML_F32), "tk-small-q4_0": ("tk-small", gguf.GGML_Q4_0)}


@pytest.mark.parametrize("cid", list(STORED_CASES))
def test_stored_rows_are_stored_q8_of_the_f32_rows(cid):
    """an f32 batch and a q8_0 batch on one context, the same ragged passes through both.  Layer 0's K/V rows depend on token and
    position only, so there the q8_0 batch holds EXACTLY stored_q8(f32 row): a wrong block maximum (tiny-gqa: kv_dim 32, ONE block
    over two heads of size 16), an id taken from the rounded d, rintf in the place of roundf, a divergent shuffle or another RoPE
    arithmetic in the quantising form of the K/V write fails here.  Deeper layers read quantised rows and differ; they must be q8_0
    rows (idempotent under stored_q8)."""
    shape, wtype = STORED_CASES[cid]
    fw, _ = model(shape, wtype)
    s = fw.shape
    seqs, passes = ragged(s)
    m = llmk.Llmk(fw)
    b32, b8 = llmk.Batch(m, 5), llmk.Batch(m, 5, kv_type=Q8)
    assert (b32.kv_type, b8.kv_type) == ("f32", Q8)
    for b in (b32, b8):
        run_ragged(b, seqs, passes, s.vocab_size)
    moved = 0
    for j, seq in enumerate(seqs):
        for which in (0, 1):
            x = b32.peek_kv(which, 0, j, 1, len(seq))
            h = b8.peek_kv(which, 0, j, 1, len(seq))
            assert np.array_equal(bits(h), bits(kq.stored_q8(x))), (cid, j, which)
            moved += int((bits(h) != bits(x)).sum())
            for l in range(s.n_layers):
                assert kq.idempotent(b8.peek_kv(which, l, j, 1, len(seq))), (cid, j, which, l)
            assert not b8.peek_kv(which, 1, j, len(seq) + 1, s.seq_len - len(seq)).any()      # rows nothing wrote stay zero
    assert moved > 0
    b8.close()
    b32.close()
    m.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
Q8_ROW_CASES = dict(ROW_CASES, **{"tiny-kvmul3-f32": ("tiny-kvmul3", gguf.GGML_F32, False)})      # + hs 32, kv_mul 3


@pytest.mark.parametrize("cid", list(Q8_ROW_CASES))
def test_ragged_rows_match_the_float64_pass_fed_the_stored_rows(cid):
    """Measured worst rel_err / top-8 error per case: DESIGN.md section 3i (printed here)."""
    shape, wtype, q6k = Q8_ROW_CASES[cid]
    fw, fw32 = model(shape, wtype, q6k)
    s = fw.shape
    seqs, passes = ragged(s)
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 5, kv_type=Q8)
    got = run_ragged(b, seqs, passes, s.vocab_size)
    ref = []
    for j, seq in enumerate(seqs):
        K, V = kq.peek_all(b, s.n_layers, j, len(seq))
        assert kq.idempotent(K) and kq.idempotent(V)
        ref.append(kq.forward_fed(fw32, seq, K, V))
    b.close()
    m.close()
    assert not np.isnan(np.concatenate(got)).any()
    within_the_bar(f"{cid}, q8_0 K/V, ragged rows", np.concatenate(got), np.concatenate(ref))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def test_fork_and_prefix_convert_the_context_s_rows_exactly_and_an_emptied_slot_is_a_fresh_slot():
    fw, _ = model("tk-small", seed=31)
    s = fw.shape
    rng = np.random.default_rng(9)
    prompt = [2] + (rng.integers(3, s.vocab_size, 18) + 1).tolist()
    n, P, nxt = len(prompt), 17, 77
    m = llmk.Llmk(fw)
    m.prefill(prompt, 1)
    ctx = {(which, l): np.stack([m.peek(4 + which, s.kv_dim, l, p) for p in range(1, n + 1)]) for which in (0, 1) for l in range(s.n_layers)}
    b = llmk.Batch(m, 5, kv_type=Q8)
    b.fork(0, n)
    b.fork(3, n)
    b.set_prefix(P)
    assert b.prefix_len == P
    for (which, l), rows in ctx.items():
        want = kq.stored_q8(rows)
        assert not np.array_equal(bits(want), bits(rows))
        for slot in (0, 3):
            assert np.array_equal(bits(b.peek_kv(which, l, slot, 1, n)), bits(want)), (which, l, slot)
            assert np.array_equal(bits(b.peek_kv(which, l, slot, n + 1, s.seq_len - n)), np.zeros((s.seq_len - n, s.kv_dim), np.uint32))      # +0.0
        assert np.array_equal(bits(b.peek_kv(which, l, -1, 1, P)), bits(want[:P])), (which, l)
        assert not b.peek_kv(which, l, 1, 1, s.seq_len).any()                           # a slot nothing was forked into
    lg = b.forward([3, 0], [nxt, nxt], [n + 1] * 2, want_argmax=False)
    assert np.array_equal(bits(lg[0]), bits(lg[1]))                                     # (the same rows in two caches)
    fresh = b.forward([1], [nxt], [1], want_argmax=False)
    b.fork(0, 0)
    assert np.array_equal(bits(b.peek_kv(0, 1, 0, 1, s.seq_len)), np.zeros((s.seq_len, s.kv_dim), np.uint32))
    assert np.array_equal(bits(b.peek_kv(1, 0, 0, 1, s.seq_len)), np.zeros((s.seq_len, s.kv_dim), np.uint32))
    emptied = b.forward([0], [nxt], [1], want_argmax=False)
    assert np.array_equal(bits(fresh), bits(emptied))
    b.close()
    m.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def fed_rows(b, fw32, slots, toks, ks):
    """forward_fed for every row of a pass on its own slot's stored rows: logits [n][V]"""
    L = fw32.shape.n_layers
    out = []
    for slot, tok, k in zip(slots, toks, ks):
        K, V = kq.peek_all(b, L, slot, k)
        assert kq.idempotent(K) and kq.idempotent(V), (slot, k)
        out.append(kq.forward_fed(fw32, [tok], K, V, pos=[k])[0])
    return np.stack(out)


@pytest.mark.parametrize("tag,counts", [("tk-small-long", (32, 33, 64, 65, 128)), ("tiny-hs128w-long", (33,))])
def test_tile_and_part_boundaries_on_q8_0_caches(tag, counts):
    """bt.wide_transcript_passes, unchanged, on a q8_0 batch: 32 | 33 | 64 | 65 | 128 rows with a row of 704 positions, forked at
    ragged k (the converting copy), 2, 3 and 6 tiles per wave; every row's cache is read back and the row compared with forward_fed
    on it; each pass twice: the same bits.  A wrong stride, fragment, scale index or clamped look-ahead in the packed loads fails here."""
    g = load_golden(tag)
    s = gguf.SHAPES[str(g["shape"])]
    fw = gguf.synth_fused(s, int(g["seed"]))
    fed = [2] + g["tokens"].tolist()
    n_pos = len(g["logits"])
    passes = bt.wide_transcript_passes(tag)
    assert set(counts) <= set(passes) and max(max(ks) for ks in passes.values()) == n_pos
    m = llmk.Llmk(fw)
    m.prefill(fed[:n_pos - 1], 1)
    b = llmk.Batch(m, 128, kv_type=Q8)
    for n in counts:
        ks = passes[n]
        slots = list(range(n))[::-1]
        toks = [fed[k - 1] for k in ks]
        out = []
        for _ in range(2):
            for slot, k in zip(slots, ks):
                b.fork(slot, k - 1)
            out.append(b.forward(slots, toks, ks, want_argmax=False))
        assert np.array_equal(bits(out[0]), bits(out[1])), n
        parts = bt.bd_parts(n, s.n_kv_heads, n_pos)
        within_the_bar(f"{tag} q8_0 K/V, {n} rows ({parts} parts, {bt.max_tiles_per_wave(n, s.n_kv_heads, n_pos)} tiles per wave)", out[0],
                       fed_rows(b, fw, slots, toks, ks))
    b.close()
    m.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def test_wide_pass_attention_on_needles_on_q8_0_caches():
    s, layout, tokens, fw = bt.wide_needle_case()
    S = s.seq_len
    m = llmk.Llmk(fw)
    m.prefill(tokens[:S - 1].tolist(), 1)
    b = llmk.Batch(m, 128, kv_type=Q8)
    for n, ks in bt.wide_needle_passes().items():
        slots = list(range(n))[::-1]
        toks = [int(tokens[k - 1]) for k in ks]
        for slot, k in zip(slots, ks):
            b.fork(slot, k - 1)
        logits = b.forward(slots, toks, ks, want_argmax=False)
        within_the_bar(f"needles {layout} on q8_0 K/V, {n} rows ({bt.bd_parts(n, s.n_kv_heads, S)} parts)", logits, fed_rows(b, fw, slots, toks, ks))
    b.close()
    m.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [15, 16, 17, 33])
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hs128w"])
def test_attached_rows_behind_a_q8_0_prefix(shape, P):
    """needles of kv heads 0 | 1 at cache rows P-1 | P; 1, RG and RG + 1 slots attached next to a slot forked at P; three passes.  An
    attached row reads the prefix rows (slot -1), then its own; the forked row its own alone."""
    s = gguf.SHAPES[shape]
    kv_mul = s.n_heads // s.n_kv_heads
    RG = pt.rg(kv_mul)
    layout = {0: [0, P - 1], 1: [P]}
    tokens, needle_tokens = an.needle_sequence(s, layout, 20261020)
    fw = an.shape_needles(gguf.synth_fused(s, 4242), needle_tokens, an.BETA)
    run = 3
    assert P + run <= s.seq_len
    m = llmk.Llmk(fw)
    m.prefill(tokens[:P].tolist(), 1)
    for n_att in (1, RG, RG + 1):
        b = llmk.Batch(m, n_att + 1, kv_type=Q8)
        b.set_prefix(P)
        for slot in range(n_att):
            b.attach(slot)
        b.fork(n_att, P)
        assert code_of(b.forward, [0], [int(tokens[P - 1])], [P]) == 1            # an attached slot's positions 1..P are the prefix
        slots = list(range(n_att + 1))[::-1]                                      # (the unattached row first)
        got = []
        for t in range(run):
            lg, am = b.forward(slots, [int(tokens[P + t])] * len(slots), [P + 1 + t] * len(slots))
            assert np.array_equal(am, first_max(lg)), (n_att, t)
            got.append(lg)
        pre = [np.stack([b.peek_kv(which, l, -1, 1, P) for l in range(s.n_layers)]) for which in (0, 1)]
        assert kq.idempotent(pre[0]) and kq.idempotent(pre[1])
        ref = np.empty_like(np.stack(got), dtype=np.float64)
        for i, slot in enumerate(slots):
            if slot < n_att:
                own = [np.stack([b.peek_kv(which, l, slot, P + 1, run) for l in range(s.n_layers)]) for which in (0, 1)]
                assert not b.peek_kv(0, 0, slot, 1, P).any()                       # (its own rows below P stay zero: the prefix is read)
                K, V = (np.concatenate([p, o], axis=1) for p, o in zip(pre, own))
            else:
                K, V = kq.peek_all(b, s.n_layers, slot, P + run)
            ref[:, i] = kq.forward_fed(fw, tokens[P:P + run], K, V, pos=np.arange(P + 1, P + run + 1))
        b.close()
        within_the_bar(f"{shape} q8_0 P {P}, {n_att} attached + 1 forked", np.stack(got).reshape(-1, s.vocab_size), ref.reshape(-1, s.vocab_size))
    m.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-kvmul3", "tiny-hs128w"])
def test_ragged_spans_match_the_float64_pass_fed_the_stored_rows(shape):
    """tests/test_batch_span_gpu.py's ragged schedule on a q8_0 batch: spans of 1, rg-1, rg, rg+1 and 2 rg+1 rows and one across the
    first tile boundary, the lengths rotating over three passes (bd_q8_attn_span_kernel, its causal edge per column), against
    forward_fed on each slot's stored rows"""
    fw, fw32 = model(shape)
    s = fw.shape
    lens, passes = ragged_passes(s)
    rng = np.random.default_rng(6)
    seqs = [random_seq(rng, s.vocab_size, n) for n in lens]
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 6, kv_type=Q8)
    got = run_passes(b, seqs, passes, s.vocab_size)
    for j, seq in enumerate(seqs):
        K, V = kq.peek_all(b, s.n_layers, j, len(seq))
        assert kq.idempotent(K) and kq.idempotent(V) and K.any() and V.any()
        within_the_bar(f"{shape} q8_0 spans, slot {j}", got[j], kq.forward_fed(fw32, seq, K, V))
    b.close()
    m.close()


def test_later_rows_of_a_span_do_not_reach_earlier_ones_and_the_per_row_kernels_serve_spans_too():
    fw, fw32 = model("tiny-hs64")
    s = fw.shape
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 6, kv_type=Q8)
    one = b.forward_spans([(0, 1, 4)], [2, 50, 60, 70], want_argmax=False)
    two = b.forward_spans([(1, 1, 4)], [2, 50, 61, 71], want_argmax=False)
    assert np.array_equal(bits(one[:2]), bits(two[:2])) and not np.array_equal(bits(one[2:]), bits(two[2:]))
    # LLMK_SPAN_ATTN=0 at create: the same spans through bd_q8_attn_kernel, within the bar of forward_fed on ITS stored rows
    rng = np.random.default_rng(3)
    seqs = [random_seq(rng, s.vocab_size, 30) for _ in range(3)]
    spans = [(1, 1, 23), (0, 1, 12), (2, 1, 4)]
    toks = seqs[1][:23] + seqs[0][:12] + seqs[2][:4]
    os.environ["LLMK_SPAN_ATTN"] = "0"
    try:
        b0 = llmk.Batch(m, 3, kv_type=Q8)
    finally:
        del os.environ["LLMK_SPAN_ATTN"]
    for name, bb in (("bd_q8_attn_span_kernel", b), ("LLMK_SPAN_ATTN=0", b0)):
        for slot in range(3):
            bb.fork(slot, 0)
        lg, am = bb.forward_spans(spans, toks)
        assert np.array_equal(am, first_max(lg))
        row = 0
        for slot, _, n in spans:
            K, V = kq.peek_all(bb, s.n_layers, slot, n)
            assert kq.idempotent(K) and kq.idempotent(V)
            within_the_bar(f"tiny-hs64 q8_0 spans, {name}, slot {slot}", lg[row:row + n], kq.forward_fed(fw32, seqs[slot][:n], K, V))
            row += n
        assert bb.time_spans(2, 9, 4, 2) > 0.0
    b0.close()
    b.close()
    m.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------
def test_decode_on_q8_0_caches_picks_and_records_what_the_hooks_answer_on_a_replay():
    """llmk_batch_decode and llmk_rows_decode on a q8_0 batch, 12 steps; the ids replayed through llmk_batch_forward on a second q8_0
    batch: every id is what llmk_sample_logits_pen answers on the replay's logits, every record what llmk_logprob_logits answers"""
    fw, _ = model("tk-small", seed=4242)
    m = llmk.Llmk(fw)
    S = m.shape.seq_len
    m.prefill(PROMPT, 1)

    def batch():
        b = llmk.Batch(m, 4, kv_type=Q8)
        for slot in (1, 2):
            b.fork(slot, len(PROMPT))
            b.set_history(slot, PROMPT)
        return b
    rows = dict(slots=[3, 1, 0, 2], tokens=[2, 50, 7, 60], pos0=[1, len(PROMPT) + 1, 1, len(PROMPT) + 1])
    before = {3: [], 1: PROMPT, 0: [], 2: PROMPT}
    args = (rows["slots"], rows["tokens"], rows["pos0"], STEPS)

    def replay(ids):
        b = batch()
        lgs = [b.forward(rows["slots"], rows["tokens"] if st == 0 else ids[:, st - 1].tolist(), [p + st for p in rows["pos0"]], want_argmax=False)
               for st in range(STEPS)]
        for slot in range(4):
            assert kq.idempotent(b.peek_kv(0, 1, slot, 1, S)) and kq.idempotent(b.peek_kv(1, 1, slot, 1, S))
        b.close()
        return np.stack(lgs)
    sps = [llmk.sampler(**sp) for sp in SAMPLERS]
    b = batch()
    ids = b.decode(*args, sps)
    b.close()
    assert ids.shape == (4, STEPS) and ids.min() >= 1 and ids.max() <= m.V
    lgs = replay(ids)
    for i, sp in enumerate(SAMPLERS):
        for st in range(STEPS):
            want = m.sample_logits(lgs[st, i], rows["pos0"][i] + st, **sp)[0]
            assert ids[i, st] == want, (i, st, ids[i, st], want)
    assert np.array_equal(ids[0], first_max(lgs[:, 0]))                   # top_k = 1 is the first maximum
    b = batch()
    greedy = b.decode(*args)
    b.close()
    assert np.array_equal(greedy, first_max(replay(greedy)).T)
    b = batch()
    rids, tlp, tt, tv = b.decode_rows(*args, sps, [llmk.penalties(**pn) for pn in PENALTIES], top_n=TOP_N, want_token_logprob=True)
    b.close()
    lgs = replay(rids)
    for i, slot in enumerate(rows["slots"]):
        fed = list(before[slot]) + [rows["tokens"][i]] + rids[i, :-1].tolist()
        m.set_history(np.array(fed + [0] * (S - len(fed)), np.int32))
        for st in range(STEPS):
            z = lgs[st, i]
            want = m.sample_logits_pen(z, rows["pos0"][i] + st, **SAMPLERS[i], **PENALTIES[i])[0]
            assert rids[i, st] == want, (i, st, rids[i, st], want)
            tl, wt, wv = m.logprob_logits(z, int(rids[i, st]), TOP_N)
            assert bits(tlp[i, st]) == bits(np.float32(tl)), (i, st)
            assert np.array_equal(tt[i, st], wt) and np.array_equal(bits(tv[i, st]), bits(wv)), (i, st)
    m.close()


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------
def test_an_f32_and_an_f16_batch_next_to_a_q8_0_batch_keep_their_bits_and_the_bytes_are_17_64ths():
    fw, _ = model("tk-small", seed=4242)
    s = fw.shape
    m = llmk.Llmk(fw)
    m.prefill(PROMPT, 1)
    rows = ([3, 1, 0, 2], [2, 50, 7, 60], [1, len(PROMPT) + 1, 1, len(PROMPT) + 1])

    def filled(**kw):
        b = llmk.Batch(m, 4, **kw)
        for slot in (1, 2):
            b.fork(slot, len(PROMPT))
        return b
    b32, b16, b8 = filled(), filled(kv_type="f16"), filled(kv_type=llmk.KV_CACHE_TYPES[Q8])
    assert (b32.kv_type, b16.kv_type, b8.kv_type) == ("f32", "f16", Q8) and llmk.lib().llmk_cache_type(b8._h) == 8
    cache = cache_units(s, 4)
    # as allocated: 32 quants and one f16 scale per 32 elements, nothing padded: 34 bytes per 32 elements = 17/64 of the f32 bytes
    assert b32.cache_bytes() == 4 * cache and b16.cache_bytes() == 2 * cache and b8.cache_bytes() == cache // 32 * 34 == 4 * cache * 17 // 64
    before = [b.forward(*rows) for b in (b32, b16)]
    ids0 = [b.decode(*rows, 5) for b in (b32, b16)]
    q8, _ = b8.forward(*rows)
    b8.decode(*rows, 5, [llmk.sampler(temperature=0.9, seed=3)] * 4)
    b8.set_prefix(4)
    b8.attach(3)
    b8.forward([3], [9], [5])
    b8.forward_spans([(0, 3, 4)], [5, 6, 7, 8])
    for b, (lg0, am0), ids in zip((b32, b16), before, ids0):
        lg1, am1 = b.forward(*rows)
        assert np.array_equal(bits(lg0), bits(lg1)) and np.array_equal(am0, am1) and np.array_equal(ids, b.decode(*rows, 5)), b.kv_type
    assert not np.array_equal(bits(before[0][0]), bits(q8))                # (the q8_0 batch is another computation)
    far = rel_err(q8, before[0][0].astype(np.float64)).max()
    mv = movement("tk-small")
    print(f"tk-small: q8_0 batch against the f32 batch: rel_err {far:.2e}; the reference's own movement {mv:.2e}")
    assert REL_TOL < far < 4 * mv                                          # ... of the same model (the CPU file's figure, x 4)
    # with a prefix: still exactly 17/64
    b32.set_prefix(4)
    pre = 2 * s.n_layers * 4 * s.kv_dim
    assert b32.cache_bytes() == 4 * (cache + pre) and b8.cache_bytes() == (cache + pre) // 32 * 34
    for b in (b32, b16, b8):
        b.close()
    m.close()


# ---- 10 -----------------------------------------------------------------------------------------------------------------------------
def test_values_beyond_the_f16_range_saturate():
    """the construction of tests/test_batch_kv16_gpu.py: layer 0's V rows of wqkv scaled so that about half of layer 0's V entries
    exceed 65504.  The q8_0 batch stores exactly stored_q8 of the f32 batch's rows -- the block maximum clamped to 65504, d =
    RNE_f16(65504 / 127) finite -- nothing non-finite, and the logits stay finite."""
    fw, _ = model("tk-small")
    s = fw.shape
    E, KV = s.emb_dim, s.kv_dim
    seq = [2] + (np.random.default_rng(5).integers(3, s.vocab_size, 19) + 1).tolist()
    cache = {}
    an.forward_all(fw, np.array(seq), cache=cache)
    scale = np.float32(2.0 ** np.ceil(np.log2(65504.0 / np.median(np.abs(cache["v"][0])))))
    w = np.array(fw.wqkv, np.float32, copy=True)
    w[0, E + KV:] *= scale
    fw.wqkv = w
    m = llmk.Llmk(fw)
    b32, b8 = llmk.Batch(m, 2), llmk.Batch(m, 2, kv_type=Q8)
    for b in (b32, b8):
        lg = np.stack([b.forward([1], [tok], [pos], want_argmax=False)[0] for pos, tok in enumerate(seq, 1)])
        assert np.isfinite(lg).all()
    v32, v8 = b32.peek_kv(1, 0, 1, 1, len(seq)), b8.peek_kv(1, 0, 1, 1, len(seq))
    over = np.abs(v32) > 65504.0
    print(f"scale 2^{int(np.log2(scale))}: {int(over.sum())} of {over.size} layer-0 V entries beyond 65504, max |v| {np.abs(v32).max():.3g}")
    assert over.any() and not over.all() and np.isfinite(v32).all()
    assert np.array_equal(bits(v8), bits(kq.stored_q8(v32)))
    top = np.float32(127.0) * np.float32(np.float16(np.float32(65504.0) / np.float32(127.0)))
    assert (np.abs(v8[over]) == top).all() and np.abs(v8).max() == top
    assert np.array_equal(bits(b8.peek_kv(0, 0, 1, 1, len(seq))), bits(kq.stored_q8(b32.peek_kv(0, 0, 1, 1, len(seq)))))
    for which in (0, 1):
        for l in range(s.n_layers):
            assert kq.idempotent(b8.peek_kv(which, l, 1, 1, len(seq))), (which, l)
    b8.close()
    b32.close()
    m.close()


# ---- 11 -----------------------------------------------------------------------------------------------------------------------------
REDO_CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import llm_f90_amd
from llm_f90_amd import llmk
import kvq8_ref as kq
from conftest import rel_err, top8_elementwise
from test_batch_kv16_gpu import small_weights
fw = small_weights()
s = fw.shape
rng = np.random.default_rng(15)
seqs = [[2] + (rng.integers(3, s.vocab_size, n - 1) + 1).tolist() for n in (6, 4, 5)]
m = llmk.Llmk(fw)
b = llmk.Batch(m, 3, kv_type="q8_0")
got = [[] for _ in seqs]
for t in range(6):
    slots = [j for j in (2, 1, 0) if t < len(seqs[j])]
    lg = b.forward(slots, [seqs[j][t] for j in slots], [t + 1] * len(slots), want_argmax=False)
    for i, j in enumerate(slots):
        got[j].append(lg[i])
worst = 0.0
for j, seq in enumerate(seqs):
    K, V = kq.peek_all(b, s.n_layers, j, len(seq))
    assert kq.idempotent(K) and kq.idempotent(V) and K.any() and V.any()
    ref = kq.forward_fed(fw, seq, K, V)
    worst = max(worst, rel_err(np.array(got[j]), ref).max(), top8_elementwise(np.array(got[j]), ref=ref).max())
print("worst", worst)
b.close()
m.close()
'''


def test_a_redone_call_rewrites_q8_0_rows():
    """llmk_batch_forward on a q8_0 batch with the "small" model, in a process of its own (the note is printed once per process): the
    redo happens, the rows it rewrote are q8_0 rows, and the logits meet the bar against forward_fed"""
    r = subprocess.run([sys.executable, "-c", REDO_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "llmk: llmk_batch_forward met a position whose activations are all below 2^-7" in r.stderr, r.stderr[-2000:]
    worst = float(r.stdout.split("worst")[1].split()[0])
    print(f"small, q8_0 K/V, redone calls: worst rel_err / top-8 {worst:.2e}")
    assert worst <= REL_TOL


def test_refusals_carry_the_documented_codes_and_leave_the_context_working():
    E_ARG, E_SHAPE, E_TYPE = 1, 2, 4
    fw, _ = model("tk-small", seed=1)
    s = fw.shape
    m = llmk.Llmk(fw)
    for bad in (2, 14, -1):                                                       # q4_0, q6_K, nothing
        assert code_of(llmk.Batch, m, 2, None, bad) == E_TYPE, bad
    assert code_of(llmk.Batch, m, 0, None, Q8) == E_ARG and code_of(llmk.Batch, m, llmk.MAX_BATCH + 1, None, Q8) == E_ARG
    assert code_of(llmk.Batch, m, 2, s.seq_len + 1, Q8) == E_ARG
    # kv_dim 48 (3 kv heads of size 16): an f32 batch exists, a q8_0 batch is LLMK_E_SHAPE
    odd = llmk.Llmk(gguf.synth_fused(gguf.LlamaShape(192, 512, 2, 12, 3, 400, 64), 1))
    assert odd.shape.kv_dim == 48
    assert code_of(llmk.Batch, odd, 2, None, Q8) == E_SHAPE
    ok = llmk.Batch(odd, 2, None, "f16")
    assert np.isfinite(ok.forward([1], [5], [1], want_argmax=False)).all()
    ok.close()
    odd.close()
    L = llmk.lib()
    b = llmk.Batch(m, 3, 32, Q8)
    assert L.llmk_cache_bytes(b._h, None) == E_ARG and L.llmk_cache_peek(b._h, 0, 0, 0, 1, 1, None) == E_ARG
    for bad in ((2, 0, 0, 1, 1), (-1, 0, 0, 1, 1), (0, s.n_layers, 0, 1, 1), (0, -1, 0, 1, 1), (0, 0, 3, 1, 1), (0, 0, -2, 1, 1),
                (0, 0, 0, 0, 1), (0, 0, 0, 1, 0), (0, 0, 0, 1, 33), (0, 0, 0, 33, 1), (0, 0, 0, 32, 2),
                (0, 0, -1, 1, 1)):                                                # no prefix yet
        assert code_of(b.peek_kv, *bad) == E_ARG, bad
    assert b.peek_kv(1, s.n_layers - 1, 2, 32, 1).shape == (1, s.kv_dim)
    m.prefill([2, 5, 6, 7, 8], 1)
    b.set_prefix(4)
    assert b.peek_kv(0, 0, -1, 1, 4).shape == (4, s.kv_dim) and b.peek_kv(1, 1, -1, 4, 1).any()
    assert code_of(b.peek_kv, 0, 0, -1, 1, 5) == E_ARG and code_of(b.peek_kv, 0, 0, -1, 5, 1) == E_ARG
    lg = b.forward([2], [5], [1], want_argmax=False)
    assert np.isfinite(lg).all()
    b.close()
    ref = m.forward(5, 1)
    assert np.isfinite(ref).all()
    assert L.llmk_destroy(m._h) == 0
    m._h = C.c_void_p()
