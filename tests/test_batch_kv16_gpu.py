"""A batch with f16 K/V caches (llmk_cache_*).  What is new on the device: the K/V write that rounds
(bd_epi_qkv_h_kernel), the converting copy of fork and prefix (bd_to_half_kernel) and the half instantiations of the attention kernels
(bd_attn_kernel / bd_attn_prefix_kernel / bd_attn_own_kernel over AttnAhead's packed half loads).  Stored rows are compared BIT FOR BIT
with clamp-then-round of what the f32 path stores; logits are compared at REL_TOL with kv16_ref.forward_fed, the float64 forward pass
fed the rows the device stored (tests/test_batch_kv16_cpu.py shows why the oracle cannot judge such a batch, and that this can).

   1  stored rows of ragged passes: layer 0 exactly the rounded f32 rows, every layer f16-representable
   2  ragged rows, joining and leaving, against forward_fed
   3  fork and prefix conversion, all layers exact; an emptied slot is a fresh slot
   4  tile and part boundaries: the wide transcript passes, each twice
   5  needles where a wave's second tile and a wide pass's parts begin
   6  a shared prefix of 15 | 16 | 17 | 33 positions, 1 | RG | RG + 1 attached rows next to a forked one, needles at rows P-1 | P
   7  decode: picks and records are what the hooks answer on a replay's logits
   8  an f32 batch next to an f16 one keeps its bits; llmk_cache_create(F32) is llmk_batch_create; bytes halve
   9  saturation: values beyond 65504 are stored as +-65504, nothing infinite
  10  a redone call rewrites f16 rows
  11  refusals
"""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

import attn_needle as an
import batch_tiles as bt
import kv16_ref as kr
import prefix_tiles as pt
from conftest import REL_TOL, ROOT, load_golden, rel_err, top8_elementwise
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf

pytestmark = pytest.mark.gpu


def first_max(rows):
    return np.argmax(np.asarray(rows), axis=-1).astype(np.int32) + 1      # (np.argmax: the first maximum)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def within_the_bar(what, got, ref):
    """rel_err and the top-8 element-wise error of rows against their reference, printed, then asserted at REL_TOL"""
    err, e8 = rel_err(got, ref), top8_elementwise(got, ref=ref)
    print(f"{what}: {len(err)} rows, rel_err max {err.max():.2e}, top-8 max {e8.max():.2e}")
    assert err.max() <= REL_TOL, (what, int(np.argmax(err)), err.max())
    assert e8.max() <= REL_TOL, (what, int(np.argmax(e8)), e8.max())


def representable(rows):
    """every value survives a round trip through np.float16 unchanged (and none is infinite)"""
    rows = np.asarray(rows, np.float32)
    return np.isfinite(rows).all() and np.array_equal(bits(rows.astype(np.float16).astype(np.float32)), bits(rows))


def model(shape, wtype=gguf.GGML_F32, q6k=False, seed=777):
    """(weights for the device, the same decoded to f32 for the reference)"""
    fw = gguf.synth_fused(gguf.SHAPES[shape], seed, wtype)
    if q6k:
        fw = gguf.with_q6k_classifier(fw)
    return fw, (fw.as_f32() if (wtype or q6k) else fw)


# ---- the ragged schedule of tests/test_batch_gpu.py test 1, restated ------------------------------------------------------------------
def ragged(s):
    """5 slots, pseudo-prompts of 1, 2, 17, 33 and seq_len - 1 tokens that start at different passes: the row count goes 2 .. 5 and
    back to 1, rows are listed by DESCENDING slot; yields (slots, tokens, positions) per pass.  Returns (seqs, passes)."""
    lens = [1, 2, 17, 33, s.seq_len - 1]
    starts = [3, 2, 1, 0, 0]
    rng = np.random.default_rng(5)
    seqs = [[2] + (rng.integers(3, s.vocab_size, n - 1) + 1).tolist() for n in lens]
    passes = []
    for t in range(max(st + n for st, n in zip(starts, lens))):
        slots = [j for j in (4, 3, 2, 1, 0) if starts[j] <= t < starts[j] + lens[j]]
        pos = [t - starts[j] + 1 for j in slots]
        passes.append((slots, [seqs[j][p - 1] for j, p in zip(slots, pos)], pos))
    assert {len(p[0]) for p in passes} == {1, 2, 3, 4, 5}
    return seqs, passes


def run_ragged(b, seqs, passes, V):
    got = [np.full((len(seq), V), np.nan, np.float32) for seq in seqs]
    for t, (slots, toks, pos) in enumerate(passes):
        lg, am = b.forward(slots, toks, pos)
        assert np.array_equal(am, first_max(lg)), (t, slots)
        for i, (j, p) in enumerate(zip(slots, pos)):
            got[j][p - 1] = lg[i]
    return got


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
STORED_CASES = {"tiny-gqa": ("tiny-gqa", gguf.GGML_F32), "tiny-hs64": ("tiny-hs64", gguf.GGML_F32), "tiny-hs128w": ("tiny-hs128w", gguf.GGML_F32),
                "tk-small-q4_0": ("tk-small", gguf.GGML_Q4_0)}


@pytest.mark.parametrize("cid", list(STORED_CASES))
def test_stored_rows_are_the_f32_rows_clamped_and_rounded_to_nearest_even(cid):
    """an f32 batch and an f16 batch on one context, the same passes through both.  Layer 0's K/V rows depend on token and position
    only, so there the f16 batch holds EXACTLY np.float16(clip(f32 row)): a conversion that rounds toward zero, or another RoPE
    arithmetic in the f16 form of the K/V write, fails here.  Deeper layers read rounded rows and differ; they must be halves."""
    shape, wtype = STORED_CASES[cid]
    fw, _ = model(shape, wtype)
    s = fw.shape
    seqs, passes = ragged(s)
    m = llmk.Llmk(fw)
    b32, b16 = llmk.Batch(m, 5), llmk.Batch(m, 5, kv_type="f16")
    assert (b32.kv_type, b16.kv_type) == ("f32", "f16")
    for b in (b32, b16):
        run_ragged(b, seqs, passes, s.vocab_size)
    moved = 0
    for j, seq in enumerate(seqs):
        for which in (0, 1):
            x = b32.peek_kv(which, 0, j, 1, len(seq))
            h = b16.peek_kv(which, 0, j, 1, len(seq))
            assert np.array_equal(bits(h), bits(kr.stored_half(x))), (cid, j, which)
            moved += int((bits(h) != bits(x)).sum())
            for l in range(s.n_layers):
                assert representable(b16.peek_kv(which, l, j, 1, len(seq))), (cid, j, which, l)
    assert moved > 0                                   # (the f32 rows are not halves to begin with)
    b16.close()
    b32.close()
    m.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
ROW_CASES = {
    "tk-small-f32": ("tk-small", gguf.GGML_F32, False),
    "tk-small-f16": ("tk-small", gguf.GGML_F16, False),
    "tk-small-q4_0-q6k": ("tk-small", gguf.GGML_Q4_0, True),
    "tiny-gqa-f32": ("tiny-gqa", gguf.GGML_F32, False),            # hs 16, kv_mul 4
    "tiny-hs64-f32": ("tiny-hs64", gguf.GGML_F32, False),          # kv_mul 2
    "tiny-hs128w-f32": ("tiny-hs128w", gguf.GGML_F32, False),      # hs 128, kv_mul 1
}


@pytest.mark.parametrize("cid", list(ROW_CASES))
def test_ragged_rows_match_the_float64_pass_fed_the_stored_rows(cid):
    """Measured worst rel_err / top-8 error per case: DESIGN.md section 3i (printed here)."""
    shape, wtype, q6k = ROW_CASES[cid]
    fw, fw32 = model(shape, wtype, q6k)
    s = fw.shape
    seqs, passes = ragged(s)
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 5, kv_type="f16")
    got = run_ragged(b, seqs, passes, s.vocab_size)
    ref = []
    for j, seq in enumerate(seqs):
        K, V = kr.peek_all(b, s.n_layers, j, len(seq))
        assert representable(K) and representable(V)
        ref.append(kr.forward_fed(fw32, seq, K, V))
    b.close()
    m.close()
    assert not np.isnan(np.concatenate(got)).any()
    within_the_bar(f"{cid}, ragged rows", np.concatenate(got), np.concatenate(ref))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def test_fork_and_prefix_convert_the_context_s_rows_exactly_and_an_emptied_slot_is_a_fresh_slot():
    fw, _ = model("tk-small", seed=31)
    s = fw.shape
    rng = np.random.default_rng(9)
    prompt = [2] + (rng.integers(3, s.vocab_size, 18) + 1).tolist()
    n, P, nxt = len(prompt), 17, 77
    assert n == 19
    m = llmk.Llmk(fw)
    m.prefill(prompt, 1)
    ctx = {(which, l): np.stack([m.peek(4 + which, s.kv_dim, l, p) for p in range(1, n + 1)]) for which in (0, 1) for l in range(s.n_layers)}
    b = llmk.Batch(m, 5, kv_type="f16")
    b.fork(0, n)
    b.fork(3, n)
    b.set_prefix(P)
    assert b.prefix_len == P
    for (which, l), rows in ctx.items():
        want = kr.stored_half(rows)
        assert not np.array_equal(bits(want), bits(rows))
        for slot in (0, 3):
            assert np.array_equal(bits(b.peek_kv(which, l, slot, 1, n)), bits(want)), (which, l, slot)
            assert not b.peek_kv(which, l, slot, n + 1, s.seq_len - n).any()            # rows beyond n_pos: as in a fresh slot
        assert np.array_equal(bits(b.peek_kv(which, l, -1, 1, P)), bits(want[:P])), (which, l)
        assert not b.peek_kv(which, l, 1, 1, s.seq_len).any()                           # a slot nothing was forked into
    lg = b.forward([3, 0], [nxt, nxt], [n + 1] * 2, want_argmax=False)
    assert np.array_equal(bits(lg[0]), bits(lg[1]))                                     # (the same rows in two caches)
    fresh = b.forward([1], [nxt], [1], want_argmax=False)
    b.fork(0, 0)
    assert not b.peek_kv(0, 1, 0, 1, s.seq_len).any() and not b.peek_kv(1, 0, 0, 1, s.seq_len).any()
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
        K, V = kr.peek_all(b, L, slot, k)
        assert representable(K) and representable(V), (slot, k)
        out.append(kr.forward_fed(fw32, [tok], K, V, pos=[k])[0])
    return np.stack(out)


@pytest.mark.parametrize("tag,counts", [("tk-small-long", (32, 33, 64, 65, 128)), ("tiny-hs128w-long", (33,))])
def test_tile_and_part_boundaries_on_f16_caches(tag, counts):
    """bt.wide_transcript_passes, unchanged, on an f16 batch: 32 | 33 | 64 | 65 | 128 rows with a row of 704 positions, forked at ragged
    k (the converting copy), 2, 3 and 6 tiles per wave, the 40-timestep row; every row's cache is read back and the row compared
    with forward_fed on it; each pass twice: the same bits.  Head size 128: one pass of 33 rows.  A wrong stride, fragment or clamped
    look-ahead in the packed loads fails here."""
    g = load_golden(tag)
    s = gguf.SHAPES[str(g["shape"])]
    fw = gguf.synth_fused(s, int(g["seed"]))
    fed = [2] + g["tokens"].tolist()                     # the token fed at position p (1-based) is fed[p - 1]
    n_pos = len(g["logits"])
    passes = bt.wide_transcript_passes(tag)
    assert set(counts) <= set(passes) and max(max(ks) for ks in passes.values()) == n_pos
    m = llmk.Llmk(fw)
    m.prefill(fed[:n_pos - 1], 1)
    b = llmk.Batch(m, 128, kv_type="f16")
    for n in counts:
        ks = passes[n]
        slots = list(range(n))[::-1]                     # (row index != slot)
        toks = [fed[k - 1] for k in ks]
        out = []
        for _ in range(2):
            for slot, k in zip(slots, ks):
                b.fork(slot, k - 1)
            out.append(b.forward(slots, toks, ks, want_argmax=False))
        assert np.array_equal(bits(out[0]), bits(out[1])), n
        parts = bt.bd_parts(n, s.n_kv_heads, n_pos)
        within_the_bar(f"{tag} f16 K/V, {n} rows ({parts} parts, {bt.max_tiles_per_wave(n, s.n_kv_heads, n_pos)} tiles per wave)", out[0],
                       fed_rows(b, fw, slots, toks, ks))
    b.close()
    m.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def test_wide_pass_attention_on_needles_on_f16_caches():
    """bt.wide_needle_case: needles of kv heads 0 | 1 at cache rows 127 | 128, 255 | 256, 351 | 352, 479 | 480 and 687 | 688; one pass
    of 128 rows and one of 64 with positions t + 1 and t + 2 of every needle row t, and S"""
    s, layout, tokens, fw = bt.wide_needle_case()
    S = s.seq_len
    m = llmk.Llmk(fw)
    m.prefill(tokens[:S - 1].tolist(), 1)
    b = llmk.Batch(m, 128, kv_type="f16")
    for n, ks in bt.wide_needle_passes().items():
        slots = list(range(n))[::-1]
        toks = [int(tokens[k - 1]) for k in ks]
        for slot, k in zip(slots, ks):
            b.fork(slot, k - 1)
        logits = b.forward(slots, toks, ks, want_argmax=False)
        within_the_bar(f"needles {layout} on f16 K/V, {n} rows ({bt.bd_parts(n, s.n_kv_heads, S)} parts)", logits, fed_rows(b, fw, slots, toks, ks))
    b.close()
    m.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [15, 16, 17, 33])
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hs128w"])
def test_attached_rows_behind_an_f16_prefix(shape, P):
    """needles of kv heads 0 | 1 at cache rows P-1 | P (the prefix's last row, the first own row); 1, RG and RG + 1 slots attached
    (one column group, a full one, a second one) next to a slot forked at P; three passes.  An attached row reads the prefix rows
    (slot -1), then its own; the forked row its own alone."""
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
        b = llmk.Batch(m, n_att + 1, kv_type="f16")
        b.set_prefix(P)
        for slot in range(n_att):
            b.attach(slot)
        b.fork(n_att, P)
        with pytest.raises(llmk.LlmkError) as e:
            b.forward([0], [int(tokens[P - 1])], [P])                      # an attached slot's positions 1..P are the prefix
        assert e.value.code == 1
        slots = list(range(n_att + 1))[::-1]                               # (the unattached row first)
        got = []
        for t in range(run):
            lg, am = b.forward(slots, [int(tokens[P + t])] * len(slots), [P + 1 + t] * len(slots))
            assert np.array_equal(am, first_max(lg)), (n_att, t)
            got.append(lg)
        pre = [np.stack([b.peek_kv(which, l, -1, 1, P) for l in range(s.n_layers)]) for which in (0, 1)]
        assert representable(pre[0]) and representable(pre[1])
        ref = np.empty_like(np.stack(got), dtype=np.float64)
        for i, slot in enumerate(slots):
            if slot < n_att:
                own = [np.stack([b.peek_kv(which, l, slot, P + 1, run) for l in range(s.n_layers)]) for which in (0, 1)]
                assert not b.peek_kv(0, 0, slot, 1, P).any()                # (its own rows below P stay zero: the prefix is read)
                K, V = (np.concatenate([p, o], axis=1) for p, o in zip(pre, own))
            else:
                K, V = kr.peek_all(b, s.n_layers, slot, P + run)
            ref[:, i] = kr.forward_fed(fw, tokens[P:P + run], K, V, pos=np.arange(P + 1, P + run + 1))
        b.close()
        within_the_bar(f"{shape} P {P}, {n_att} attached + 1 forked", np.stack(got).reshape(-1, s.vocab_size), ref.reshape(-1, s.vocab_size))
    m.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
SAMPLERS = [dict(temperature=1.0, seed=11, top_k=1),                       # greedy through the sampler
            dict(temperature=0.9, seed=12),
            dict(temperature=0.8, seed=13, top_k=5),
            dict(temperature=1.1, seed=14, top_p=0.9, min_p=0.05)]
PENALTIES = [dict(), dict(last_n=4, repeat=1.3), dict(), dict()]           # one penalties row
STEPS, TOP_N = 12, 5
PROMPT = [2, 40, 41, 42, 43, 44]


def test_decode_on_f16_caches_picks_and_records_what_the_hooks_answer_on_a_replay():
    """llmk_batch_decode and llmk_rows_decode on an f16 batch, 12 steps; the ids replayed through llmk_batch_forward on a second f16
    batch: every id is what llmk_sample_logits_pen answers on the replay's logits, every record what llmk_logprob_logits answers"""
    fw, _ = model("tk-small", seed=4242)
    m = llmk.Llmk(fw)
    S = m.shape.seq_len
    m.prefill(PROMPT, 1)

    def batch():
        b = llmk.Batch(m, 4, kv_type="f16")
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
            assert representable(b.peek_kv(0, 1, slot, 1, S)) and representable(b.peek_kv(1, 1, slot, 1, S))
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
    assert len({tuple(r) for r in ids.tolist()}) == 4                      # four samplers, four texts
    b = batch()
    greedy = b.decode(*args)
    b.close()
    assert np.array_equal(greedy, first_max(replay(greedy)).T)
    # the rows form: one penalties row, top_n 5
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


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------
def test_an_f32_batch_next_to_an_f16_batch_keeps_its_bits_and_the_bytes_halve():
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
    b32, b16, c32 = filled(), filled(kv_type="f16"), filled(kv_type=llmk.KV_TYPES["f32"])      # (the last one through llmk_cache_create)
    assert (b32.kv_type, b16.kv_type, c32.kv_type) == ("f32", "f16", "f32")
    cache = 2 * s.n_layers * 4 * s.seq_len * s.kv_dim
    assert b32.cache_bytes() == c32.cache_bytes() == 4 * cache and b16.cache_bytes() == 2 * cache
    before, am0 = b32.forward(*rows)
    ids0 = b32.decode(*rows, 5)
    half, _ = b16.forward(*rows)
    b16.decode(*rows, 5, [llmk.sampler(temperature=0.9, seed=3)] * 4)
    b16.set_prefix(4)
    b16.attach(3)
    b16.forward([3], [9], [5])
    after, am1 = b32.forward(*rows)
    assert np.array_equal(bits(before), bits(after)) and np.array_equal(am0, am1) and np.array_equal(ids0, b32.decode(*rows, 5))
    other, am2 = c32.forward(*rows)
    assert np.array_equal(bits(before), bits(other)) and np.array_equal(am0, am2) and np.array_equal(ids0, c32.decode(*rows, 5))
    for which in (0, 1):
        for l in range(s.n_layers):
            assert np.array_equal(bits(b32.peek_kv(which, l, 1, 1, s.seq_len)), bits(c32.peek_kv(which, l, 1, 1, s.seq_len)))
    assert not np.array_equal(bits(before), bits(half))                    # (the f16 batch is another computation)
    assert rel_err(half, before.astype(np.float64)).max() < 1e-2           # ... of the same model
    # with a prefix: still exactly half
    b32.set_prefix(4)
    pre = 2 * s.n_layers * 4 * s.kv_dim
    assert b32.cache_bytes() == 4 * (cache + pre) and b16.cache_bytes() == 2 * (cache + pre)
    for b in (b32, b16, c32):
        b.close()
    m.close()


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------
def test_values_beyond_the_f16_range_saturate():
    """tk-small f32 with layer 0's V rows of wqkv scaled by a power of two chosen on the float64 reference so that about half of
    layer 0's V entries exceed 65504.  One outlier must not make a row's softmax NaN: the f16 batch stores +-65504 there -- exactly
    clip-then-round of the f32 batch's row -- nothing infinite, and the logits stay finite.  (The GEMMs' own f16-range redo may fire
    on the next layer's activations.)"""
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
    b32, b16 = llmk.Batch(m, 2), llmk.Batch(m, 2, kv_type="f16")
    for b in (b32, b16):
        lg = np.stack([b.forward([1], [tok], [pos], want_argmax=False)[0] for pos, tok in enumerate(seq, 1)])
        assert np.isfinite(lg).all()
    v32, v16 = b32.peek_kv(1, 0, 1, 1, len(seq)), b16.peek_kv(1, 0, 1, 1, len(seq))
    over = np.abs(v32) > 65504.0
    print(f"scale 2^{int(np.log2(scale))}: {int(over.sum())} of {over.size} layer-0 V entries beyond 65504, max |v| {np.abs(v32).max():.3g}")
    assert over.any() and not over.all() and np.isfinite(v32).all()
    assert np.array_equal(bits(v16), bits(kr.stored_half(v32)))
    assert (np.abs(v16[over]) == 65504.0).all() and np.abs(v16).max() == 65504.0
    assert np.array_equal(bits(b16.peek_kv(0, 0, 1, 1, len(seq))), bits(kr.stored_half(b32.peek_kv(0, 0, 1, 1, len(seq)))))
    for which in (0, 1):
        for l in range(s.n_layers):
            assert representable(b16.peek_kv(which, l, 1, 1, len(seq))), (which, l)
    b16.close()
    b32.close()
    m.close()


# ---- 10 -----------------------------------------------------------------------------------------------------------------------------
def small_weights():
    """the "small" construction of tests/test_prefill_gpu.py, restated: attention norm gains x 2^-10 and wo x 2^10 on tk-small16 -- whole
    rows below 2^-7, every batched call is redone on the f32 matrix instruction"""
    fw = gguf.synth_fused(gguf.SHAPES["tk-small16"], 78)
    fw.rms_att_weight = (fw.rms_att_weight * np.float32(2.0 ** -10)).astype(np.float32)
    fw.wo = (fw.wo * fw.wo.dtype.type(1024)).astype(fw.wo.dtype)
    return fw


REDO_CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import llm_f90_amd
from llm_f90_amd import llmk
import kv16_ref as kr
from conftest import rel_err, top8_elementwise
from test_batch_kv16_gpu import representable, small_weights
fw = small_weights()
s = fw.shape
rng = np.random.default_rng(15)
seqs = [[2] + (rng.integers(3, s.vocab_size, n - 1) + 1).tolist() for n in (6, 4, 5)]
m = llmk.Llmk(fw)
b = llmk.Batch(m, 3, kv_type="f16")
got = [[] for _ in seqs]
for t in range(6):
    slots = [j for j in (2, 1, 0) if t < len(seqs[j])]
    lg = b.forward(slots, [seqs[j][t] for j in slots], [t + 1] * len(slots), want_argmax=False)
    for i, j in enumerate(slots):
        got[j].append(lg[i])
worst = 0.0
for j, seq in enumerate(seqs):
    K, V = kr.peek_all(b, s.n_layers, j, len(seq))
    assert representable(K) and representable(V) and K.any() and V.any()
    ref = kr.forward_fed(fw, seq, K, V)
    worst = max(worst, rel_err(np.array(got[j]), ref).max(), top8_elementwise(np.array(got[j]), ref=ref).max())
print("worst", worst)
b.close()
m.close()
'''


def test_a_redone_call_rewrites_f16_rows():
    """llmk_batch_forward on an f16 batch with the "small" model, in a process of its own (the note is printed once per process): the
    redo happens, the rows it rewrote are halves, and the logits meet the bar against forward_fed.  (The "large" construction is left
    out: saturation changes its values.)"""
    r = subprocess.run([sys.executable, "-c", REDO_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "llmk: llmk_batch_forward met a position whose activations are all below 2^-7" in r.stderr, r.stderr[-2000:]
    worst = float(r.stdout.split("worst")[1].split()[0])
    print(f"small, f16 K/V, redone calls: worst rel_err / top-8 {worst:.2e}")
    assert worst <= REL_TOL


# ---- 11 -----------------------------------------------------------------------------------------------------------------------------
def code_of(fn, *a, **kw):
    with pytest.raises(llmk.LlmkError) as e:
        fn(*a, **kw)
    return e.value.code


def test_refusals_carry_the_documented_codes_and_leave_the_context_working():
    E_ARG, E_SHAPE, E_TYPE = 1, 2, 4
    fw, _ = model("tk-small", seed=1)
    s = fw.shape
    m = llmk.Llmk(fw)
    for bad in (2, 14, -1):                                                       # q4_0, q6_K, nothing
        assert code_of(llmk.Batch, m, 2, None, bad) == E_TYPE, bad
    assert code_of(llmk.Batch, m, 0, None, "f16") == E_ARG and code_of(llmk.Batch, m, llmk.MAX_BATCH + 1, None, "f16") == E_ARG
    assert code_of(llmk.Batch, m, 2, s.seq_len + 1, "f16") == E_ARG
    mha = llmk.Llmk(gguf.synth_fused(gguf.SHAPES["tiny-mha"], 1))               # H = 352: the batch's shape rule, whatever the type
    assert code_of(llmk.Batch, mha, 2, None, "f16") == E_SHAPE
    mha.close()
    L = llmk.lib()
    assert L.llmk_cache_type(None) == -E_ARG and L.llmk_cache_bytes(None, C.byref(C.c_ulonglong())) == E_ARG
    out = np.zeros((4, s.kv_dim), np.float32)
    assert L.llmk_cache_peek(None, 0, 0, 0, 1, 1, out.ctypes.data_as(C.POINTER(C.c_float))) == E_ARG
    for kv_type in ("f32", "f16"):
        b = llmk.Batch(m, 3, 32, kv_type)
        assert L.llmk_cache_bytes(b._h, None) == E_ARG and L.llmk_cache_peek(b._h, 0, 0, 0, 1, 1, None) == E_ARG
        for bad in ((2, 0, 0, 1, 1), (-1, 0, 0, 1, 1), (0, s.n_layers, 0, 1, 1), (0, -1, 0, 1, 1), (0, 0, 3, 1, 1), (0, 0, -2, 1, 1),
                    (0, 0, 0, 0, 1), (0, 0, 0, 1, 0), (0, 0, 0, 1, 33), (0, 0, 0, 33, 1), (0, 0, 0, 32, 2),
                    (0, 0, -1, 1, 1)):                                            # no prefix yet
            assert code_of(b.peek_kv, *bad) == E_ARG, (kv_type, bad)
        assert b.peek_kv(1, s.n_layers - 1, 2, 32, 1).shape == (1, s.kv_dim)
        m.prefill([2, 5, 6, 7, 8], 1)
        b.set_prefix(4)
        assert b.peek_kv(0, 0, -1, 1, 4).shape == (4, s.kv_dim) and b.peek_kv(1, 1, -1, 4, 1).any()
        assert code_of(b.peek_kv, 0, 0, -1, 1, 5) == E_ARG and code_of(b.peek_kv, 0, 0, -1, 5, 1) == E_ARG
        # nothing of the above ran or broke anything: the batch and its context still work
        lg = b.forward([2], [5], [1], want_argmax=False)
        assert np.isfinite(lg).all()
        b.close()
    ref = m.forward(5, 1)
    assert np.isfinite(ref).all()
    assert L.llmk_destroy(m._h) == 0
    m._h = C.c_void_p()
