"""Batched decode (llmk_batch_*): several sequences, each with a K/V cache of its own, through one pass over
the weights.  What is new on the device is the per-row position (bd_epi_qkv_kernel) and the attention over many caches
(bd_attn_kernel, split into parts and merged): every test here reaches them through the public entry points.

  1  rows of ragged sequences, joining and leaving, against the f32 C oracle on each sequence alone
  2  fork: the context's prompt rows in two slots; an emptied slot is a fresh slot
  3  attention tile and part boundaries against the real reference's long transcripts
  4  needle models (tests/attn_needle.py) with the needles on this kernel's boundaries, against the float64 reference
  5  llmk_batch_decode's picks are llmk_sample_logits' on the same logits
  6  the same call twice is bit-identical; batches do not disturb each other or their context
  7  refusals
"""
import ctypes as C

import numpy as np
import pytest

import attn_needle as an
import batch_tiles as bt
from conftest import REL_TOL, load_golden, rel_err, top8_elementwise
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf

pytestmark = pytest.mark.gpu


def first_max(rows):
    return np.argmax(np.asarray(rows), axis=-1).astype(np.int32) + 1      # (np.argmax: the first maximum)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
ROW_CASES = {
    "tiny-gqa-f32": ("tiny-gqa", gguf.GGML_F32, False),            # hs 16, kv_mul 4
    "tiny-hs64-f32": ("tiny-hs64", gguf.GGML_F32, False),          # kv_mul 2
    # tiny-hs128 itself (hidden_dim 1376 = 21.5 x 64) is off the GEMMs' 64-column step, like tiny-mha: the batch refuses it (test 7),
    # and there is no token-by-token form.  tiny-hs128w is that shape with hidden_dim 1408: head size 128, kv_mul 1
    "tiny-hs128w-f32": ("tiny-hs128w", gguf.GGML_F32, False),
    "tiny-70bish-f32": ("tiny-70bish", gguf.GGML_F32, False),      # one kv head, kv_mul 8
    "tk-small-f16": ("tk-small", gguf.GGML_F16, False),
    "tk-small-q4_0": ("tk-small", gguf.GGML_Q4_0, False),
    "tk-small-q4_0-q6k": ("tk-small", gguf.GGML_Q4_0, True),
}


@pytest.mark.parametrize("cid", list(ROW_CASES))
def test_rows_of_ragged_sequences_match_the_oracle_on_each_sequence_alone(cid):
    """5 slots, pseudo-prompts of 1, 2, 17, 33 and seq_len - 1 tokens that start at different passes: the row count goes
    2 .. 5 and back to 1, rows are listed by DESCENDING slot (row index != slot), positions next to each other are unrelated"""
    from oracle.oracle import Oracle
    shape, wtype, q6k = ROW_CASES[cid]
    s = gguf.SHAPES[shape]
    fw = gguf.synth_fused(s, 777, wtype)
    if q6k:
        fw = gguf.with_q6k_classifier(fw)
    lens = [1, 2, 17, 33, s.seq_len - 1]
    starts = [3, 2, 1, 0, 0]
    rng = np.random.default_rng(5)
    seqs = [[2] + (rng.integers(3, s.vocab_size, n - 1) + 1).tolist() for n in lens]
    o = Oracle(fw.as_f32() if (wtype or q6k) else fw, "omp")
    ref = []
    for seq in seqs:
        o.reset()
        ref.append(np.array([o.forward(tok, pos) for pos, tok in enumerate(seq, 1)]))
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 5)
    got = [np.empty_like(r) for r in ref]
    counts = set()
    for t in range(max(st + n for st, n in zip(starts, lens))):
        slots = [j for j in (4, 3, 2, 1, 0) if starts[j] <= t < starts[j] + lens[j]]
        pos = [t - starts[j] + 1 for j in slots]
        lg, am = b.forward(slots, [seqs[j][p - 1] for j, p in zip(slots, pos)], pos)
        assert np.array_equal(am, first_max(lg)), (t, slots)
        for i, (j, p) in enumerate(zip(slots, pos)):
            got[j][p - 1] = lg[i]
        counts.add(len(slots))
    b.close()
    m.close()
    assert counts == {1, 2, 3, 4, 5}, counts
    for j in range(5):
        err, e8 = rel_err(got[j], ref[j]), top8_elementwise(got[j], ref=ref[j])
        print(f"{cid} slot {j} ({lens[j]} positions): rel_err max {err.max():.2e}, top-8 max {e8.max():.2e}")
        assert err.max() <= REL_TOL, (j, int(np.argmax(err)), err.max())
        assert e8.max() <= REL_TOL, (j, int(np.argmax(e8)), e8.max())


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def test_fork_copies_the_context_s_prompt_rows_and_an_emptied_slot_is_a_fresh_slot():
    s = gguf.SHAPES["tk-small"]
    fw = gguf.synth_fused(s, 31)
    rng = np.random.default_rng(9)
    prompt = [2] + (rng.integers(3, s.vocab_size, 19) + 1).tolist()
    nxt = 77
    m = llmk.Llmk(fw)
    m.prefill(prompt, 1)
    b = llmk.Batch(m, 5)
    b.fork(0, len(prompt))
    b.fork(3, len(prompt))
    lg = b.forward([3, 0], [nxt, nxt], [len(prompt) + 1] * 2, want_argmax=False)
    ref = m.forward(nxt, len(prompt) + 1)
    assert rel_err(lg, np.stack([ref, ref])).max() <= REL_TOL
    assert top8_elementwise(lg, ref=np.stack([ref, ref])).max() <= REL_TOL
    assert np.array_equal(lg[0], lg[1])             # (the same rows in two caches)
    fresh = b.forward([1], [nxt], [1], want_argmax=False)
    b.fork(0, 0)
    emptied = b.forward([0], [nxt], [1], want_argmax=False)
    assert np.array_equal(fresh, emptied)
    with pytest.raises(llmk.LlmkError):
        b.fork(0, s.seq_len + 1)
    with pytest.raises(llmk.LlmkError):
        b.fork(5, 1)
    b.close()
    m.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["tk-small-long", "tiny-hs128w-long"])
def test_attention_tile_and_part_boundaries_match_the_real_reference(tag):
    """The real reference's transcript is prefilled once on the context; for every k at, below and above a multiple of the
    kernel's 16-timestep tile (every part boundary is one) rows 1..k-1 are forked into slot 0 and position k is fed through the
    batch -- alone (the split rule cuts the row into up to 6 parts here) and next to four rows at positions 1..4.
    tiny-hs128w-long (tests/golden/make_golden_batch.py): the real reference on tiny-hs128-long's geometry with hidden_dim 1408 --
    the batched passes refuse tiny-hs128-long's 1376."""
    g = load_golden(tag)
    s = gguf.SHAPES[str(g["shape"])]
    fw = gguf.synth_fused(s, int(g["seed"]))
    fed = [2] + g["tokens"].tolist()                     # the token fed at position p (1-based) is fed[p - 1]
    n = len(g["logits"])
    ks = bt.boundary_positions(n)
    assert len(ks) >= 3 * (n // bt.BD_TILE) - 2
    split = sorted({bt.bd_parts(1, s.n_kv_heads, k) for k in ks})
    assert split[0] == 1 and split[-1] >= 3, split       # the cases do cross the split rule
    m = llmk.Llmk(fw)
    m.prefill(fed[:n - 1], 1)
    b = llmk.Batch(m, 5)
    for j in range(1, 5):
        b.fork(j, j - 1)
    worst = 0.0
    for k in ks:
        b.fork(0, k - 1)
        alone = b.forward([0], [fed[k - 1]], [k], want_argmax=False)
        b.fork(0, k - 1)
        among = b.forward([1, 2, 0, 3, 4], [fed[0], fed[1], fed[k - 1], fed[2], fed[3]], [1, 2, k, 3, 4], want_argmax=False)
        ref = g["logits"][k - 1][None]
        ea, eb = rel_err(alone, ref).max(), rel_err(among[2:3], ref).max()
        worst = max(worst, ea, eb)
        assert ea <= REL_TOL and eb <= REL_TOL, (k, ea, eb)
        assert top8_elementwise(alone, ref=ref).max() <= REL_TOL and top8_elementwise(among[2:3], ref=ref).max() <= REL_TOL, k
        short = rel_err(among[[0, 1, 3, 4]], g["logits"][:4]).max()
        assert short <= REL_TOL, (k, short)
    print(f"{tag}: {len(ks)} boundary positions, worst rel_err {worst:.2e}, part counts met {split}")
    b.close()
    m.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def needle_layout(s, S):
    """needles of kv heads 0 / 1 on both sides of this kernel's boundaries for a row that runs alone: rows 15 | 16 (two tiles), the
    last row of part 0 | the first of part 1 and the last part's first row and the one before it, at the full context and at two
    thirds of it (the parts move with the position), the sink and the last row"""
    lay = {0: {0, bt.BD_TILE - 1, S - 1}, 1: {bt.BD_TILE}}
    for pos in (S, 2 * S // 3):
        bounds = bt.part_boundaries(pos, 1, s.n_kv_heads)
        assert len(bounds) >= 1, (pos, bounds)
        for t in (bounds[0], bounds[-1]):
            lay[0].add(t - 1)
            lay[1].add(t)
    assert not lay[0] & lay[1], lay
    return {g: sorted(ts) for g, ts in lay.items()}


@pytest.mark.parametrize("shape,S", [("tk-small-long", 704), ("tiny-hs128w-long", 320)])
def test_batch_attention_on_needles(shape, S):
    """tests/attn_needle.py's construction (layer 0's softmax mass on a few chosen timesteps: one of them dropped, duplicated or read
    from the wrong kv head moves every later position's logits by > 0.1 of max |logit|) with the needles on bd_attn_kernel's tile and
    part boundaries; the whole sequence through one slot, every position against the float64 reference, with the assertions
    tests/test_attn_needle_gpu.py makes for the other kernels"""
    s0 = gguf.SHAPES[shape]
    s = gguf.LlamaShape(s0.emb_dim, s0.hidden_dim, s0.n_layers, s0.n_heads, s0.n_kv_heads, s0.vocab_size, S)
    layout = needle_layout(s, S)
    tokens, needle_tokens = an.needle_sequence(s, layout, 20261019)
    fw = an.shape_needles(gguf.synth_fused(s, 4242), needle_tokens, an.BETA)
    ref, att0 = an.forward_all(fw, tokens)
    for g, ts in layout.items():                     # the needles do hold the mass where a query sees one of its head
        h = g * (s.n_heads // s.n_kv_heads)
        assert att0[h, S - 1, ts].sum() > 0.999, (g, att0[h, S - 1, ts].sum())
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 2)
    logits = np.stack([b.forward([1], [int(tok)], [pos], want_argmax=False)[0] for pos, tok in enumerate(tokens, 1)])
    b.close()
    m.close()
    err, e8 = rel_err(logits, ref), top8_elementwise(logits, ref=ref)
    safe = an.safe_argmax_positions(ref)
    print(f"{shape} needles {layout}: rel_err max {err.max():.2e} at {int(np.argmax(err))}, top-8 max {e8.max():.2e}, "
          f"{int(safe.sum())} of {len(safe)} positions safe for argmax")
    assert err.max() <= REL_TOL, (err.max(), int(np.argmax(err)))
    assert e8.max() <= REL_TOL, (e8.max(), int(np.argmax(e8)))
    assert safe.sum() > len(safe) // 2
    assert np.array_equal(np.argmax(logits, axis=1)[safe], np.argmax(ref, axis=1)[safe])


# ---- 5, 6 ---------------------------------------------------------------------------------------------------------------------------
SAMPLERS = [dict(temperature=1.0, seed=11, top_k=1),                       # greedy through the sampler
            dict(temperature=0.9, seed=12),
            dict(temperature=0.8, seed=13, top_k=5),
            dict(temperature=1.1, seed=14, top_p=0.9, min_p=0.05)]
STEPS = 12


@pytest.fixture(scope="module")
def decode_setup():
    """tk-small f32 with a 6-token prompt on the context; rows 0, 1 start in fresh slots, rows 2, 3 behind the forked prompt"""
    s = gguf.SHAPES["tk-small"]
    m = llmk.Llmk(gguf.synth_fused(s, 4242))
    prompt = [2, 40, 41, 42, 43, 44]
    m.prefill(prompt, 1)

    def batch():
        b = llmk.Batch(m, 4)
        b.fork(1, len(prompt))
        b.fork(2, len(prompt))
        return b
    rows = dict(slots=[3, 1, 0, 2], tokens=[2, 50, 7, 60], pos0=[1, len(prompt) + 1, 1, len(prompt) + 1])
    yield m, batch, rows
    m.close()


def replay(b, rows, ids):
    """feed a decode's ids step by step through llmk_batch_forward: (logits [steps][n][V], argmax [steps][n])"""
    lgs, ams = [], []
    for st in range(ids.shape[1]):
        toks = rows["tokens"] if st == 0 else ids[:, st - 1].tolist()
        lg, am = b.forward(rows["slots"], toks, [p + st for p in rows["pos0"]])
        lgs.append(lg)
        ams.append(am)
    return np.stack(lgs), np.stack(ams)


def test_decode_picks_what_the_verification_hook_picks_on_the_same_logits(decode_setup):
    m, batch, rows = decode_setup
    b = batch()
    ids = b.decode(rows["slots"], rows["tokens"], rows["pos0"], STEPS, [llmk.sampler(**sp) for sp in SAMPLERS])
    b.close()
    assert ids.shape == (4, STEPS) and ids.min() >= 1 and ids.max() <= m.V
    b2 = batch()
    lgs, ams = replay(b2, rows, ids)
    b2.close()
    for i, sp in enumerate(SAMPLERS):
        for st in range(STEPS):
            want = m.sample_logits(lgs[st, i], rows["pos0"][i] + st, **sp)[0]
            assert ids[i, st] == want, (i, st, ids[i, st], want)
    assert np.array_equal(ids[0], ams[:, 0])                        # top_k = 1 is the first maximum
    assert len({tuple(r) for r in ids.tolist()}) == 4               # four samplers, four texts
    b3 = batch()
    greedy = b3.decode(rows["slots"], rows["tokens"], rows["pos0"], STEPS)
    b3.close()
    b4 = batch()
    _, ams = replay(b4, rows, greedy)
    b4.close()
    assert np.array_equal(greedy, ams.T)


def test_the_same_call_twice_is_bit_identical_and_batches_leave_each_other_and_the_context_alone(decode_setup):
    m, batch, rows = decode_setup
    before = m.forward(45, 7)
    b1, b2 = batch(), batch()
    sps = [llmk.sampler(**sp) for sp in SAMPLERS]
    args = (rows["slots"], rows["tokens"], rows["pos0"])
    lg1, am1 = b1.forward(*args)
    ids1 = b1.decode(*args, STEPS, sps)
    other = b2.decode([0, 1], [9, 10], [1, 7], 5)                   # another batch in between, on the same workspaces
    lg2, am2 = b1.forward(*args)
    ids2 = b1.decode(*args, STEPS, sps)
    assert np.array_equal(lg1, lg2) and np.array_equal(am1, am2) and np.array_equal(ids1, ids2)
    lg3, am3 = b2.forward(*args)                                     # ... and the same rows in the other batch's caches
    assert np.array_equal(lg1, lg3) and np.array_equal(am1, am3)
    assert np.array_equal(other, b2.decode([0, 1], [9, 10], [1, 7], 5))
    after = m.forward(45, 7)
    assert np.array_equal(before, after)
    assert np.array_equal(b1.decode(*args, STEPS), b2.decode(*args, STEPS))
    b1.close()
    b2.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def code_of(fn, *a, **kw):
    with pytest.raises(llmk.LlmkError) as e:
        fn(*a, **kw)
    return e.value.code


def test_refusals_carry_the_documented_codes_and_leave_the_context_working():
    E_ARG, E_SHAPE, E_STATE = 1, 2, 5
    mha = llmk.Llmk(gguf.synth_fused(gguf.SHAPES["tiny-mha"], 1))               # H = 352: not on the GEMMs' 64-column step
    assert code_of(llmk.Batch, mha, 2) == E_SHAPE
    assert np.all(np.isfinite(mha.forward(2, 1)))
    mha.close()
    hs128 = llmk.Llmk(gguf.synth_fused(gguf.SHAPES["tiny-hs128"], 1))           # H = 1376: the same
    assert code_of(llmk.Batch, hs128, 2) == E_SHAPE
    hs128.close()
    s = gguf.SHAPES["tk-small"]
    fw = gguf.synth_fused(s, 1)
    tp = llmk.Llmk(fw, tp_rank=0, tp_size=2)
    assert code_of(llmk.Batch, tp, 2) == E_SHAPE
    tp.close()
    empty = llmk.Llmk.create_empty(s, gguf.GGML_F32)
    assert code_of(llmk.Batch, empty, 2) == E_STATE
    empty.close()
    m = llmk.Llmk(fw)
    assert code_of(llmk.Batch, m, 0) == E_ARG and code_of(llmk.Batch, m, llmk.MAX_BATCH + 1) == E_ARG
    assert code_of(llmk.Batch, m, 2, s.seq_len + 1) == E_ARG
    b = llmk.Batch(m, 3, 32)
    assert code_of(b.forward, [1, 1], [5, 6], [1, 1]) == E_ARG                  # a duplicate slot
    assert code_of(b.forward, [0, 1, 2, 0], [5, 6, 7, 8], [1, 1, 1, 1]) == E_ARG  # n > n_slots
    assert code_of(b.forward, [0, 3], [5, 6], [1, 1]) == E_ARG                  # no such slot
    assert code_of(b.forward, [0], [5], [33]) == E_ARG                          # a position beyond the batch's seq_len
    assert code_of(b.forward, [0], [5], [0]) == E_ARG
    assert code_of(b.forward, [0], [0], [1]) == E_ARG                           # token 0
    assert code_of(b.forward, [0], [s.vocab_size + 1], [1]) == E_ARG
    assert code_of(b.forward, [0], [5], [1], want_logits=False, want_argmax=False) == E_ARG      # both outputs NULL
    assert code_of(b.decode, [0, 1], [5, 6], [1, 30], 4) == E_ARG              # steps running past the cache (30 + 4 - 1 = 33)
    assert b.decode([0, 1], [5, 6], [1, 29], 4).shape == (2, 4)                 # ... and up to its last row
    assert code_of(b.decode, [0], [5], [1], 0) == E_ARG
    for bad in (dict(temperature=0.0, seed=1), dict(temperature=1.0, seed=1, top_k=-1), dict(temperature=1.0, seed=1, top_p=0.0),
                dict(temperature=1.0, seed=1, min_p=1.5), dict(temperature=float("nan"), seed=1)):
        assert code_of(b.decode, [0, 1], [5, 6], [1, 1], 2, [llmk.sampler(temperature=1.0, seed=3), llmk.sampler(**bad)]) == E_ARG, bad
    assert llmk.lib().llmk_destroy(m._h) == E_STATE                             # a live batch
    # nothing of the above ran or broke anything: the context and the batch still work
    ref = m.forward(5, 1)
    lg = b.forward([2], [5], [1], want_argmax=False)
    assert rel_err(lg, ref[None]).max() <= REL_TOL
    assert b.time(3, 7, 2) > 0.0
    b.close()
    assert llmk.lib().llmk_destroy(m._h) == 0
    m._h = C.c_void_p()
