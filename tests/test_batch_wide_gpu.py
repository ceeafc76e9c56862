"""Batched decode where it is used: WIDE passes, waves that take several tiles, and calls that are redone --
against references that are not the batch itself.  The sibling files compare logits with a reference at 5 rows per pass at the most,
where a wave of bd_attn_kernel never takes a second tile; the case tables here come from tests/batch_tiles.py and
tests/prefix_tiles.py, and tests/test_batch_wide_cpu.py proves without a device what they reach.

  1  128 slots with sequences of their OWN through passes of 128, 17, 113, 16, ... 1 rows, against the f32 C oracle on each alone
  2  ragged passes of 32 .. 128 rows with a row of 704 (320) positions, against the real reference's long transcripts
  3  needle models with the needles where a wave's second tile and a wide pass's parts begin, against the float64 reference
  4  127 slots behind a shared prefix of 560 | 690 positions next to a long unattached row; 128 behind 19, through 10 own tiles
  5  calls that are redone on the f32 matrix instruction, in a batch: logits and ids against the oracle; the redo really happens
"""
import subprocess
import sys

import numpy as np
import pytest

import attn_needle as an
import batch_tiles as bt
import prefix_tiles as pt
from conftest import REL_TOL, ROOT, load_golden, rel_err, top8_elementwise
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf

pytestmark = pytest.mark.gpu


def first_max(rows):
    return np.argmax(np.asarray(rows), axis=-1).astype(np.int32) + 1      # (np.argmax: the first maximum)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def oracle_rows(o, seq):
    """the oracle teacher-forced on one sequence alone: logits [len(seq)][V]"""
    o.reset()
    return np.array([o.forward(int(tok), pos) for pos, tok in enumerate(seq, 1)])


def within_the_bar(what, got, ref):
    """rel_err and the top-8 element-wise error of rows against their reference, printed, then asserted at REL_TOL"""
    err, e8 = rel_err(got, ref), top8_elementwise(got, ref=ref)
    print(f"{what}: {len(err)} rows, rel_err max {err.max():.2e}, top-8 max {e8.max():.2e}")
    assert err.max() <= REL_TOL, (what, int(np.argmax(err)), err.max())
    assert e8.max() <= REL_TOL, (what, int(np.argmax(e8)), e8.max())


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
WIDTH_CASES = {
    "tk-small-f32": ("tk-small", gguf.GGML_F32, False),
    "tk-small-f16": ("tk-small", gguf.GGML_F16, False),
    "tk-small-q4_0": ("tk-small", gguf.GGML_Q4_0, False),
    "tk-small-q4_0-q6k": ("tk-small", gguf.GGML_Q4_0, True),
    "tiny-gqa-f32": ("tiny-gqa", gguf.GGML_F32, False),            # hs 16, kv_mul 4
    "tiny-hs128w-f32": ("tiny-hs128w", gguf.GGML_F32, False),      # hs 128, kv_mul 1
}


@pytest.mark.parametrize("cid", list(WIDTH_CASES))
def test_wide_passes_of_distinct_sequences_match_the_oracle_on_each_sequence_alone(cid):
    """128 slots, each with a random sequence of its own of 19 or 20 positions, built by batched passes alone (no fork: bd_epi_qkv_kernel
    writes every K/V row that is read later, and a row that reads another slot's cache gets another answer).  43 passes of
    bt.WIDTH_SCHEDULE rows -- 128, 17, 113, 16, 112, 33, 97, 32, 96, 3, 65, 2, 64, 1, three times, and 128: the edges of the GEMM's
    16-row groups and its plan switches at 96 and 113 rows, a narrow pass behind a wide one's workspace rows and part states -- each
    over the slots that have advanced least, listed in a seeded permutation.  2,465 rows, and as many oracle forwards, per case."""
    from oracle.oracle import Oracle
    shape, wtype, q6k = WIDTH_CASES[cid]
    s = gguf.SHAPES[shape]
    fw = gguf.synth_fused(s, 777, wtype)
    if q6k:
        fw = gguf.with_q6k_classifier(fw)
    passes = bt.width_passes()
    lens = [max(p for rows in passes for j, p in rows if j == slot) for slot in range(128)]
    assert max(lens) <= s.seq_len
    rng = np.random.default_rng(6)
    seqs = [[2] + (rng.integers(3, s.vocab_size, n - 1) + 1).tolist() for n in lens]
    o = Oracle(fw.as_f32() if (wtype or q6k) else fw, "omp")
    ref = [oracle_rows(o, seq) for seq in seqs]
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 128)
    got = [np.full_like(r, np.nan) for r in ref]
    widths = set()
    for t, rows in enumerate(passes):
        slots, pos = [j for j, _ in rows], [p for _, p in rows]
        lg, am = b.forward(slots, [seqs[j][p - 1] for j, p in rows], pos)
        assert np.array_equal(am, first_max(lg)), (t, len(rows))
        for i, (j, p) in enumerate(rows):
            got[j][p - 1] = lg[i]
        widths.add(len(rows))
    b.close()
    m.close()
    assert widths == set(bt.WIDTHS) and {128, 113, 112, 97, 96, 65, 64, 33, 32, 17, 16, 3, 2, 1} <= widths, widths
    got, ref = np.concatenate(got), np.concatenate(ref)
    assert not np.isnan(got).any()
    within_the_bar(f"{cid}, {len(passes)} passes of {sorted(widths)} rows", got, ref)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(bt.WIDE_SHAPES))
def test_long_ragged_wide_passes_match_the_real_reference(tag):
    """The real reference's transcript is prefilled once on the context.  For every pass of bt.wide_transcript_passes -- 32, 33, 64, 65
    and 128 rows (32, 33, 128 for head size 128): 4, 3, 2, 1 and 1 parts, 2 .. 6 tiles per wave -- rows 1..k-1 are forked into one slot
    per row at ragged k and position k of every row is fed in ONE pass.  Every pass holds the longest row, the 128-row pass a row of
    every tile count, the passes together every k at, below and above a multiple of 16; a 2-part pass holds a row of 40 timesteps
    (empty parts, empty waves).  Each pass runs twice: the same bits.
    The slots of this test share one sequence: a row that read a longer neighbour's cache would go unnoticed here -- test 1 sees that."""
    g = load_golden(tag)
    s = gguf.SHAPES[str(g["shape"])]
    fw = gguf.synth_fused(s, int(g["seed"]))
    fed = [2] + g["tokens"].tolist()                     # the token fed at position p (1-based) is fed[p - 1]
    n_pos = len(g["logits"])
    assert n_pos == bt.WIDE_SHAPES[tag][1] and s.n_kv_heads == bt.WIDE_SHAPES[tag][0]
    m = llmk.Llmk(fw)
    m.prefill(fed[:n_pos - 1], 1)
    b = llmk.Batch(m, 128)
    for n, ks in sorted(bt.wide_transcript_passes(tag).items()):
        slots = list(range(n))[::-1]                     # (row index != slot)
        out = []
        for _ in range(2):
            for slot, k in zip(slots, ks):
                b.fork(slot, k - 1)
            out.append(b.forward(slots, [fed[k - 1] for k in ks], ks, want_argmax=False))
        assert np.array_equal(bits(out[0]), bits(out[1])), n
        parts = bt.bd_parts(n, s.n_kv_heads, n_pos)
        within_the_bar(f"{tag}, {n} rows ({parts} parts, {bt.max_tiles_per_wave(n, s.n_kv_heads, n_pos)} tiles per wave)", out[0],
                       g["logits"][np.array(ks) - 1])
    b.close()
    m.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def test_wide_pass_attention_on_needles():
    """tests/attn_needle.py's construction on tk-small-long's geometry, S = 704, with the needles of kv heads 0 | 1 at cache rows 127 |
    128 and 255 | 256 (a wave's second and third tile at one part), 351 | 352 and 479 | 480 (the part boundary of a 64-row pass and its
    part 1's second round of tiles) and 687 | 688 (the last tile: the clamped look-ahead's target).  The sequence is prefilled on the
    context and forked at ragged k; one pass of 128 rows and one of 64, each with positions t + 1 (the needle is the row the pass
    writes) and t + 2 (it comes from the fork) of every needle row t, and S; against the float64 reference with the assertions of
    test_batch_attention_on_needles.  (tests/test_batch_wide_cpu.py checks mass and safe-argmax condition on the reference alone.)"""
    s, layout, tokens, fw = bt.wide_needle_case()
    S, kv_mul = s.seq_len, s.n_heads // s.n_kv_heads
    ref, att0 = an.forward_all(fw, tokens)
    for g, ts in layout.items():                     # the needles do hold the mass where a query sees one of its head
        assert att0[g * kv_mul, S - 1, ts].sum() > 0.999, (g, att0[g * kv_mul, S - 1, ts].sum())
    m = llmk.Llmk(fw)
    m.prefill(tokens[:S - 1].tolist(), 1)
    b = llmk.Batch(m, 128)
    for n, ks in bt.wide_needle_passes().items():
        slots = list(range(n))[::-1]
        for slot, k in zip(slots, ks):
            b.fork(slot, k - 1)
        logits = b.forward(slots, [int(tokens[k - 1]) for k in ks], ks, want_argmax=False)
        want = ref[np.array(ks) - 1]
        safe = an.safe_argmax_positions(want)
        print(f"{n} rows, {int(safe.sum())} of {len(safe)} safe for argmax")
        within_the_bar(f"needles {layout}, {n} rows ({bt.bd_parts(n, s.n_kv_heads, S)} parts)", logits, want)
        assert safe.sum() > len(safe) // 2
        assert np.array_equal(np.argmax(logits, axis=1)[safe], np.argmax(want, axis=1)[safe])
    b.close()
    m.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(pt.WIDE_PREFIX_CASES))
def test_many_rows_behind_a_long_prefix_and_long_own_ranges_match_the_oracle(case):
    """tiny-gqa's geometry (4 rows per column group) with seq_len 704, f32; ONE oracle sequence of P + run positions, the first P of
    it prefilled on the context and set as the prefix.
    P560, P690 (run 40 and -- seq_len is 704 -- 14): 127 attached slots join over the first 8 passes, all fed the sequence's own
    continuation, so a pass has ragged positions and a last column group of 3 rows; with 65 attached rows or more
    bd_attn_prefix_kernel runs 4 parts of 9 | 11 tiles: a wave's second tile.  Slot 127 is forked at P, NOT attached, and joins at pass
    8 (127 rows, then 128): bd_attn_own_kernel with first = 0 through 35 tiles or more in one part, 5 or 6 per wave, folded by
    bd_attn_fold_kernel behind no prefix state.
    P19-own: 128 attached slots through 150 positions: own rows 19 .. 168 are 10 tiles, 2 per wave, the first masked below P.
    Every row of every pass against the oracle at its position; the whole case twice: the same bits."""
    from oracle.oracle import Oracle
    P, run, join = pt.WIDE_PREFIX_CASES[case]
    s0 = gguf.SHAPES["tiny-gqa"]
    s = gguf.LlamaShape(s0.emb_dim, s0.hidden_dim, s0.n_layers, s0.n_heads, s0.n_kv_heads, s0.vocab_size, pt.WIDE_SEQ_LEN)
    fw = gguf.synth_fused(s, 777)
    rng = np.random.default_rng(7)
    seq = [2] + (rng.integers(3, s.vocab_size, P + run - 1) + 1).tolist()
    ref = oracle_rows(Oracle(fw, "omp"), seq)
    passes = pt.wide_prefix_passes(case)
    m = llmk.Llmk(fw)
    last = m.prefill(seq[:P], 1)
    assert rel_err(last[None], ref[P - 1][None]).max() <= REL_TOL
    b = llmk.Batch(m, 128)
    b.set_prefix(P)
    runs = []
    for _ in range(2):
        firsts = {}
        for rows in passes:
            firsts.update({slot: first for slot, first, _ in rows})
        for slot, first in firsts.items():
            b.attach(slot) if first else b.fork(slot, P)
        got, want, free = [], [], []
        for t, rows in enumerate(passes):
            pos = [p for _, _, p in rows]
            lg, am = b.forward([r[0] for r in rows], [seq[p - 1] for p in pos], pos)
            assert np.array_equal(am, first_max(lg)), (case, t)
            got.append(lg)
            want.append(ref[np.array(pos) - 1])
            free += [first == 0 for _, first, _ in rows]
        runs.append((np.concatenate(got), np.concatenate(want), np.array(free)))
    b.close()
    m.close()
    assert np.array_equal(bits(runs[0][0]), bits(runs[1][0]))
    got, want, free = runs[0]
    within_the_bar(f"{case}: {len(passes)} passes, attached rows", got[~free], want[~free])
    if join is not None:
        assert free.sum() == run
        within_the_bar(f"{case}: the unattached row behind {P} positions of its own", got[free], want[free])


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def redo_weights(case, wtype=gguf.GGML_F32):
    """tk-small16 with the constructions of tests/test_prefill_gpu.py.  "large": FFN norm gains x 1e5, activations beyond 65504: the
    first batched call is redone and the context stays on the f32 matrix instruction.  "small": attention norm gains x 2^-10 and wo x
    2^10, whole rows below 2^-7: EVERY batched call is redone, the next one tries the f16 instruction again.  "plain": neither."""
    s = gguf.SHAPES["tk-small16"]
    fw = gguf.synth_fused(s, {"large": 77, "small": 78, "plain": 79}[case], wtype)
    if case == "large":
        fw.rms_ffn_weight = (fw.rms_ffn_weight * np.float32(1e5)).astype(np.float32)
    elif case == "small":
        fw.rms_att_weight = (fw.rms_att_weight * np.float32(2.0 ** -10)).astype(np.float32)
        fw.wo = (fw.wo * fw.wo.dtype.type(1024)).astype(fw.wo.dtype)
    return fw


REDO_FORWARD = [("large", gguf.GGML_F32), ("large", gguf.GGML_F16), ("large", gguf.GGML_Q4_0), ("small", gguf.GGML_F32),
                ("small", gguf.GGML_F16)]


@pytest.mark.parametrize("case,wtype", REDO_FORWARD, ids=[f"{c}-{('f32', 'f16', 'q4_0')[w]}" for c, w in REDO_FORWARD])
def test_redone_forward_calls_match_the_oracle(case, wtype):
    """5 slots with sequences of their own of 8, 3, 6, 4 and 7 tokens that start at passes 0, 2, 1, 3 and 0: 8 passes of 2, 3, 4, 5, 5,
    4, 4 and 1 rows, every K/V row written by a pass.  "small": every pass is redone; "large": the first.  Either way every later
    pass reads K/V rows that a redone call rewrote, and every pass's logits are the oracle's."""
    from oracle.oracle import Oracle
    fw = redo_weights(case, wtype)
    s = fw.shape
    lens, starts = [8, 3, 6, 4, 7], [0, 2, 1, 3, 0]
    rng = np.random.default_rng(15)
    seqs = [[2] + (rng.integers(3, s.vocab_size, n - 1) + 1).tolist() for n in lens]
    o = Oracle(fw.as_f32() if wtype else fw, "omp")
    ref = [oracle_rows(o, seq) for seq in seqs]
    assert all(np.isfinite(r).all() for r in ref)
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 5)
    got = [np.full_like(r, np.nan) for r in ref]
    counts = []
    for t in range(max(st + n for st, n in zip(starts, lens))):
        slots = [j for j in (4, 3, 2, 1, 0) if starts[j] <= t < starts[j] + lens[j]]
        pos = [t - starts[j] + 1 for j in slots]
        lg, am = b.forward(slots, [seqs[j][p - 1] for j, p in zip(slots, pos)], pos)
        assert np.array_equal(am, first_max(lg)), (t, slots)
        for i, (j, p) in enumerate(zip(slots, pos)):
            got[j][p - 1] = lg[i]
        counts.append(len(slots))
    b.close()
    m.close()
    assert counts == [2, 3, 4, 5, 5, 4, 4, 1], counts
    within_the_bar(f"{case}, ggml type {wtype}, passes of {counts} rows", np.concatenate(got), np.concatenate(ref))


DECODE_SAMPLERS = [dict(temperature=0.9, seed=21), dict(temperature=0.8, seed=22, top_k=5), dict(temperature=1.1, seed=23, top_p=0.9, min_p=0.05)]
# two calls: rows of fresh slots 2, 0, 1 through 3 steps; then slots 1 and 2 go on from what they picked next to a fresh slot 3, 4 steps
DECODE_CALLS = [dict(slots=[2, 0, 1], first=[2, 40, 41], pos0=[1, 1, 1], steps=3), dict(slots=[1, 3, 2], first=[None, 42, None], pos0=[4, 1, 4], steps=4)]


@pytest.mark.parametrize("entry", ["batch_decode", "rows_decode"])
@pytest.mark.parametrize("case", ["large", "small"])
def test_redone_decode_calls_pick_what_a_replay_implies_and_the_replay_matches_the_oracle(case, entry):
    """llmk_batch_decode (greedy) and llmk_rows_decode (three samplers) on the "large" and "small" models, f32.  Two calls: the first is
    redone on both models, the second -- ragged: two rows go on at position 4, one starts -- on "small".  A redone call that started
    from the row words the flawed call left advanced on the device, or that kept an id of it, feeds other tokens than the replay: the
    ids are those a replay through llmk_batch_forward implies (first maximum, or llmk_sample_logits), and the replay's logits are the
    oracle's on the sequences so fed."""
    from oracle.oracle import Oracle
    fw = redo_weights(case)
    m = llmk.Llmk(fw)
    sps = None if entry == "batch_decode" else DECODE_SAMPLERS

    def calls(b, run):
        """the two calls through run(b, slots, tokens, pos0, steps) -> ids [n][steps]; (slot -> tokens fed, ids per call)"""
        fed, last, out = {}, {}, []
        for c in DECODE_CALLS:
            toks = [last[slot] if tok is None else tok for slot, tok in zip(c["slots"], c["first"])]
            ids = run(b, c["slots"], toks, c["pos0"], c["steps"])
            out.append(ids)
            for i, slot in enumerate(c["slots"]):
                assert len(fed.get(slot, [])) == c["pos0"][i] - 1
                fed.setdefault(slot, []).extend([toks[i]] + ids[i, :-1].tolist())
                last[slot] = int(ids[i, -1])
        return fed, out

    def decode(b, slots, toks, pos0, steps):
        if entry == "batch_decode":
            return b.decode(slots, toks, pos0, steps)
        return b.decode_rows(slots, toks, pos0, steps, [llmk.sampler(**sp) for sp in sps])
    b = llmk.Batch(m, 4)
    fed, ids = calls(b, decode)
    b.close()
    assert all(x.min() >= 1 and x.max() <= m.V for x in ids)
    replayed = iter(ids)
    logits = {}

    def replay(b, slots, toks, pos0, steps):
        want = next(replayed)
        for st in range(steps):
            lg, am = b.forward(slots, toks if st == 0 else want[:, st - 1].tolist(), [p + st for p in pos0])
            for i, slot in enumerate(slots):
                pick = am[i] if sps is None else m.sample_logits(lg[i], pos0[i] + st, **sps[i])[0]
                assert want[i, st] == pick, (slot, pos0[i] + st, want[i, st], pick)
                logits.setdefault(slot, []).append(lg[i])
        return want
    b2 = llmk.Batch(m, 4)
    fed2, _ = calls(b2, replay)
    b2.close()
    m.close()
    assert fed2 == fed and sorted(len(v) for v in fed.values()) == [3, 4, 7, 7]
    o = Oracle(fw, "omp")
    ref = np.concatenate([oracle_rows(o, fed[slot]) for slot in sorted(fed)])
    assert np.isfinite(ref).all()
    within_the_bar(f"{case} {entry}: replay of {sum(x.size for x in ids)} picks", np.concatenate([np.array(logits[slot]) for slot in sorted(fed)]), ref)


@pytest.mark.parametrize("wtype", [gguf.GGML_F32, gguf.GGML_F16], ids=["f32", "f16"])
def test_redone_calls_on_attached_slots_match_the_oracle(wtype):
    """"small": 19 positions prefilled (redone) and set as the prefix; slots 0, 1 and 2 attached -- slot 2 from the second pass on --
    and slot 3 forked behind the same 19 positions, each with a continuation of its own; 6 passes, each redone: the prefix's rows are
    the prefill's and are not rewritten, the rows' own K/V rows are.  Every row against the oracle on its sequence alone."""
    from oracle.oracle import Oracle
    fw = redo_weights("small", wtype)
    s = fw.shape
    P, passes = 19, 6
    rng = np.random.default_rng(16)
    prompt = [2] + (rng.integers(3, s.vocab_size, P - 1) + 1).tolist()
    starts = [0, 0, 1, 0]
    conts = [(rng.integers(3, s.vocab_size, passes - st) + 1).tolist() for st in starts]
    o = Oracle(fw.as_f32() if wtype else fw, "omp")
    ref = [oracle_rows(o, prompt + c)[P:] for c in conts]
    m = llmk.Llmk(fw)
    m.prefill(prompt, 1)
    b = llmk.Batch(m, 4)
    b.set_prefix(P)
    for slot in (0, 1, 2):
        b.attach(slot)
    b.fork(3, P)
    got = [np.full_like(r, np.nan) for r in ref]
    for t in range(passes):
        slots = [j for j in (3, 2, 1, 0) if starts[j] <= t]
        lg, am = b.forward(slots, [conts[j][t - starts[j]] for j in slots], [P + 1 + t - starts[j] for j in slots])
        assert np.array_equal(am, first_max(lg)), t
        for i, j in enumerate(slots):
            got[j][t - starts[j]] = lg[i]
    b.close()
    m.close()
    within_the_bar(f"small, ggml type {wtype}: 3 attached slots and a forked one behind {P} positions", np.concatenate(got), np.concatenate(ref))


REDO_CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import llm_f90_amd
from llm_f90_amd import llmk
from test_batch_wide_gpu import redo_weights
case, entry = sys.argv[2], sys.argv[3]
m = llmk.Llmk(redo_weights(case))
b = llmk.Batch(m, 3)
rows = ([2, 0, 1], [2, 40, 41], [1, 1, 1])
if entry in ("llmk_batch_forward", "all"):
    assert np.isfinite(b.forward(*rows, want_argmax=False)).all()
if entry in ("llmk_batch_decode", "all"):
    assert b.decode(*rows, 2).min() >= 1
if entry in ("llmk_rows_decode", "all"):
    assert b.decode_rows(*rows, 2, [llmk.sampler(temperature=0.9, seed=5)] * 3).min() >= 1
b.close()
m.close()
'''
REDO_NOTES = {"large": "met an activation beyond the f16 range", "small": "met a position whose activations are all below 2^-7"}
REDO_CHILDREN = [(case, entry) for case in REDO_NOTES for entry in ("llmk_batch_forward", "llmk_batch_decode", "llmk_rows_decode")]


@pytest.mark.parametrize("case,entry", REDO_CHILDREN + [("plain", "all")])
def test_the_redo_really_happens_in_a_batch(case, entry):
    """the models of the tests above in a process of their own per entry point (the note is printed once per process and entry
    point): the redo branch says on stderr who met which bit of the flag; ordinary weights raise nothing in any of the three"""
    r = subprocess.run([sys.executable, "-c", REDO_CHILD, ROOT, case, entry], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    if case in REDO_NOTES:
        assert f"llmk: {entry} {REDO_NOTES[case]}" in r.stderr, r.stderr[-2000:]
    else:
        assert not any(note in r.stderr for note in REDO_NOTES.values()), r.stderr[-2000:]
