"""A shared prefix for the batched decode (llmk_prefix_*): slots attached to ONE copy of the prompt's K/V rows.
What is new on the device is bd_attn_prefix_kernel (the prefix rows against the query heads of several rows at once), bd_attn_own_kernel
(a row's own rows P .. pos-1) and bd_attn_fold_kernel; every test reaches them through the public entry points.

  1  ragged rows behind a prefix, joining and leaving, next to an unattached row, against the f32 C oracle on each sequence alone
  2  prefix lengths at, below and above tile and part boundaries against the real reference's long transcripts
  3  needle models (tests/attn_needle.py) with the needles on the two ragged edges and the prefix's tile and part boundaries
  4  llmk_batch_decode and llmk_rows_decode on attached slots pick and record what the hooks answer on the same logits
  5  the same call twice is bit-identical; a prefix leaves unattached rows and the context alone
  6  an attached slot against the same slot filled by llmk_batch_fork
  7  refusals
"""
import numpy as np
import pytest

import attn_needle as an
import batch_tiles as bt
import prefix_tiles as pt
from conftest import REL_TOL, load_golden, rel_err, top8_elementwise
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf

pytestmark = pytest.mark.gpu


def first_max(rows):
    return np.argmax(np.asarray(rows), axis=-1).astype(np.int32) + 1      # (np.argmax: the first maximum)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
ROW_CASES = {
    "tiny-gqa-f32": ("tiny-gqa", gguf.GGML_F32, False),            # hs 16, kv_mul 4: 4 rows per column group
    "tiny-hs64-f32": ("tiny-hs64", gguf.GGML_F32, False),          # kv_mul 2: 8
    "tiny-hs128w-f32": ("tiny-hs128w", gguf.GGML_F32, False),      # hs 128, kv_mul 1: 16, so 17 attached rows
    "tiny-70bish-f32": ("tiny-70bish", gguf.GGML_F32, False),      # one kv head, kv_mul 8: 2, so 3
    "tk-small-f16": ("tk-small", gguf.GGML_F16, False),
    "tk-small-q4_0": ("tk-small", gguf.GGML_Q4_0, False),
    "tk-small-q4_0-q6k": ("tk-small", gguf.GGML_Q4_0, True),
}
PREFIX_LENS = (1, 15, 16, 17, 33)
PASSES = 6


@pytest.mark.parametrize("cid", list(ROW_CASES))
def test_ragged_rows_behind_a_prefix_match_the_oracle_on_each_sequence_alone(cid):
    """For every P: RG + 1 attached slots (RG = rows per column group) continue the P-token prompt with tokens of their own -- slot 0
    through all 6 passes, slots 1 .. RG-1 through passes 1..3, slot RG through passes 2..4, so a pass has 1, RG, RG + 1, RG + 1, 2 and
    1 attached rows at unrelated positions -- and one unattached slot runs a sequence of its own from position 1 (passes 0..4: mixed
    passes).  Rows are listed by DESCENDING slot.  Every position of every sequence against the oracle on that sequence alone."""
    from oracle.oracle import Oracle
    shape, wtype, q6k = ROW_CASES[cid]
    s = gguf.SHAPES[shape]
    fw = gguf.synth_fused(s, 777, wtype)
    if q6k:
        fw = gguf.with_q6k_classifier(fw)
    rg = pt.rg(s.n_heads // s.n_kv_heads)
    natt = rg + 1
    spans = [(0, PASSES)] + [(1, 4)] * (rg - 1) + [(2, 5)]       # [first pass, last pass + 1) of attached slot j
    free = natt                                                  # the unattached slot
    o = Oracle(fw.as_f32() if (wtype or q6k) else fw, "omp")
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, natt + 1)
    rng = np.random.default_rng(5)
    for P in PREFIX_LENS:
        assert P + PASSES <= s.seq_len
        prompt = [2] + (rng.integers(3, s.vocab_size, P - 1) + 1).tolist()
        conts = [(rng.integers(3, s.vocab_size, t1 - t0) + 1).tolist() for t0, t1 in spans]
        other = [2] + (rng.integers(3, s.vocab_size, PASSES - 2) + 1).tolist()
        ref = []
        for seq in [prompt + c for c in conts] + [other]:
            o.reset()
            ref.append(np.array([o.forward(tok, pos) for pos, tok in enumerate(seq, 1)]))
        last = m.prefill(prompt, 1)
        assert rel_err(last[None], ref[0][P - 1][None]).max() <= REL_TOL, P          # the prompt itself, as the context computed it
        for j in range(natt):
            b.fork(j, 0)
        b.fork(free, 0)
        b.set_prefix(P)
        assert b.prefix_len == P
        for j in range(natt):
            b.attach(j)
        got = [np.full_like(r, np.nan) for r in ref]
        counts = []
        for t in range(PASSES):
            rows = [(free, other[t], t + 1)] if t < len(other) else []
            rows += [(j, conts[j][t - spans[j][0]], P + 1 + t - spans[j][0]) for j in range(natt) if spans[j][0] <= t < spans[j][1]]
            rows.sort(key=lambda r: -r[0])
            lg, am = b.forward([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
            assert np.array_equal(am, first_max(lg)), (P, t)
            for i, (slot, _, pos) in enumerate(rows):
                got[slot][pos - 1] = lg[i]
            counts.append(sum(1 for r in rows if r[0] != free))
        assert counts == [1, rg, rg + 1, rg + 1, 2, 1] and {1, rg, rg + 1} <= set(counts), counts
        worst = 0.0
        for j in range(natt + 1):
            lo = 0 if j == free else P                           # (an attached slot's positions 1..P are the context's)
            assert not np.isnan(got[j][lo:]).any(), (P, j)
            err, e8 = rel_err(got[j][lo:], ref[j][lo:]), top8_elementwise(got[j][lo:], ref=ref[j][lo:])
            worst = max(worst, err.max(), e8.max())
            assert err.max() <= REL_TOL, (P, j, int(np.argmax(err)), err.max())
            assert e8.max() <= REL_TOL, (P, j, int(np.argmax(e8)), e8.max())
        print(f"{cid} P {P}: {natt} attached slots + 1, attached rows per pass {counts}, worst {worst:.2e}")
    b.close()
    m.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
RUN = 34          # positions behind the prefix: two own-tile boundaries


@pytest.mark.parametrize("tag", ["tk-small-long", "tiny-hs128w-long"])
def test_prefix_lengths_on_tile_and_part_boundaries_match_the_real_reference(tag):
    """The real reference's transcript is prefilled once on the context.  P runs at, one below and one above three multiples of the
    16-row tile: 16, 144 (the prefix of a row that runs alone splits in two parts from 129 on) and the largest that leaves 34
    positions.  Positions P+1 .. P+34 go through an attached slot -- alone, and next to four unattached rows at positions 1..4."""
    g = load_golden(tag)
    s = gguf.SHAPES[str(g["shape"])]
    kv_mul = s.n_heads // s.n_kv_heads
    fw = gguf.synth_fused(s, int(g["seed"]))
    fed = [2] + g["tokens"].tolist()                     # the token fed at position p (1-based) is fed[p - 1]
    n = len(g["logits"])
    mults = [bt.BD_TILE, 9 * bt.BD_TILE, (n - RUN - 1) // bt.BD_TILE * bt.BD_TILE]
    Ps = [k for k in bt.boundary_positions(n) if any(abs(k - mm) <= 1 for mm in mults)]
    assert len(Ps) == 9 and max(Ps) + RUN <= n, Ps
    alone = sorted({pt.prefix_parts(1, s.n_kv_heads, kv_mul, P) for P in Ps})
    assert alone[0] == 1 and alone[-1] >= 2, alone       # the cases do cross the prefix's split rule
    m = llmk.Llmk(fw)
    m.prefill(fed[:n - 1], 1)
    b = llmk.Batch(m, 5)
    for j in range(1, 5):
        b.fork(j, j - 1)
    worst = 0.0
    for P in Ps:
        b.fork(0, 0)
        b.set_prefix(P)
        for among in (False, True):
            b.attach(0)                                   # (again: a new sequence behind the prefix, own rows zeroed)
            for k in range(P + 1, P + RUN + 1):
                if among:
                    lg = b.forward([1, 2, 0, 3, 4], [fed[0], fed[1], fed[k - 1], fed[2], fed[3]], [1, 2, k, 3, 4], want_argmax=False)
                    short = rel_err(lg[[0, 1, 3, 4]], g["logits"][:4]).max()
                    assert short <= REL_TOL, (P, k, short)
                    lg = lg[2:3]
                else:
                    lg = b.forward([0], [fed[k - 1]], [k], want_argmax=False)
                ref = g["logits"][k - 1][None]
                e = rel_err(lg, ref).max()
                worst = max(worst, e)
                assert e <= REL_TOL, (P, k, among, e)
                assert top8_elementwise(lg, ref=ref).max() <= REL_TOL, (P, k, among)
    print(f"{tag}: prefix lengths {Ps}, worst rel_err {worst:.2e}, prefix part counts met {alone}")
    b.close()
    m.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(pt.NEEDLE_CASES))
def test_prefix_attention_on_needles(shape):
    """tests/attn_needle.py's construction with the needles of kv heads 0 | 1 at cache rows P-1 | P (the prefix's last row, masked in
    nobody's tile but its own; the first own row, in a tile whose rows below P are masked), 15 | 16 and the last row of prefix part 0 |
    the first of part 1; P % 16 = 5.  The first P tokens are prefilled on the context, the rest of the sequence goes through one
    attached slot; every such position against the float64 reference, with test_batch_attention_on_needles' assertions.
    (tests/test_batch_prefix_cpu.py checks the safe-argmax condition of this seed on the reference alone.)"""
    s, P, layout, tokens, fw = pt.needle_case(shape)
    S = s.seq_len
    ref, att0 = an.forward_all(fw, tokens)
    for g, ts in layout.items():                     # the needles do hold the mass where a query sees one of its head
        h = g * (s.n_heads // s.n_kv_heads)
        assert att0[h, S - 1, ts].sum() > 0.999, (g, att0[h, S - 1, ts].sum())
    assert pt.prefix_parts(1, s.n_kv_heads, s.n_heads // s.n_kv_heads, P) >= 2
    m = llmk.Llmk(fw)
    m.prefill(tokens[:P].tolist(), 1)
    b = llmk.Batch(m, 2)
    b.set_prefix(P)
    b.attach(1)
    logits = np.stack([b.forward([1], [int(tokens[pos - 1])], [pos], want_argmax=False)[0] for pos in range(P + 1, S + 1)])
    b.close()
    m.close()
    ref = ref[P:]
    err, e8 = rel_err(logits, ref), top8_elementwise(logits, ref=ref)
    safe = an.safe_argmax_positions(ref)
    print(f"{shape} P {P} needles {layout}: rel_err max {err.max():.2e} at {P + 1 + int(np.argmax(err))}, top-8 max {e8.max():.2e}, "
          f"{int(safe.sum())} of {len(safe)} positions safe for argmax")
    assert err.max() <= REL_TOL, (err.max(), int(np.argmax(err)))
    assert e8.max() <= REL_TOL, (e8.max(), int(np.argmax(e8)))
    assert safe.sum() > len(safe) // 2
    assert np.array_equal(np.argmax(logits, axis=1)[safe], np.argmax(ref, axis=1)[safe])


# ---- 4, 5, 6 ------------------------------------------------------------------------------------------------------------------------
SAMPLERS = [dict(temperature=1.0, seed=11, top_k=1),                       # greedy through the sampler
            dict(temperature=0.9, seed=12),
            dict(temperature=0.8, seed=13, top_k=5),
            dict(temperature=1.1, seed=14, top_p=0.9, min_p=0.05)]
STEPS = 8
PROMPT = [2] + list(range(40, 58))          # 19 positions: the prefix's second tile is ragged, the own rows start mid-tile


@pytest.fixture(scope="module")
def decode_setup():
    """tk-small f32 with a 19-token prompt on the context; rows 0, 1 and 3 sit in slots attached to it (the prompt recorded as a
    context's caller records it), row 2 starts in a fresh slot"""
    s = gguf.SHAPES["tk-small"]
    m = llmk.Llmk(gguf.synth_fused(s, 4242))
    m.prefill(PROMPT, 1)
    P = len(PROMPT)

    def batch(share=True):
        b = llmk.Batch(m, 4)
        if share:
            b.set_prefix(P)
        for slot in (3, 1, 2):
            b.attach(slot) if share else b.fork(slot, P)
            b.set_history(slot, PROMPT)
        return b
    rows = dict(slots=[3, 1, 0, 2], tokens=[70, 50, 2, 60], pos0=[P + 1, P + 1, 1, P + 1])
    before = {3: PROMPT, 1: PROMPT, 0: [], 2: PROMPT}
    yield m, batch, rows, before
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


def test_batch_decode_on_attached_slots_picks_what_the_hook_picks_on_the_same_logits(decode_setup):
    m, batch, rows, _ = decode_setup
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
    b3 = batch()
    greedy = b3.decode(rows["slots"], rows["tokens"], rows["pos0"], STEPS)
    b3.close()
    b4 = batch()
    _, ams = replay(b4, rows, greedy)
    b4.close()
    assert np.array_equal(greedy, ams.T)


def test_rows_decode_on_attached_slots_picks_and_records_what_the_hooks_answer(decode_setup):
    """sampled, a repeat penalty over a window that reaches into the recorded prompt, top-3 records"""
    m, batch, rows, before = decode_setup
    S, n, top_n = m.shape.seq_len, 4, 3
    pens = [dict(last_n=8, repeat=1.3), dict(last_n=64, repeat=1.5), dict(), dict(last_n=4, repeat=1.2, presence=0.4)]
    b = batch()
    ids, tlp, tt, tv = b.decode_rows(rows["slots"], rows["tokens"], rows["pos0"], STEPS, [llmk.sampler(**sp) for sp in SAMPLERS],
                                     [llmk.penalties(**pn) for pn in pens], top_n=top_n, want_token_logprob=True)
    hist = [b.get_history(slot, S) for slot in rows["slots"]]
    b.close()
    assert ids.shape == (n, STEPS) and ids.min() >= 1 and ids.max() <= m.V
    b2 = batch()
    lgs, _ = replay(b2, rows, ids)
    b2.close()
    for i, slot in enumerate(rows["slots"]):
        fed = list(before[slot]) + [rows["tokens"][i]] + ids[i, :-1].tolist()      # the prompt, the first token, the ids but the last
        record = np.array(fed + [0] * (S - len(fed)), np.int32)
        assert np.array_equal(hist[i], record), (i, hist[i], record)                # records are per slot, by absolute position
        m.set_history(record)
        for st in range(STEPS):
            z = lgs[st, i]
            want = m.sample_logits_pen(z, rows["pos0"][i] + st, **SAMPLERS[i], **pens[i])[0]
            assert ids[i, st] == want, (i, st, ids[i, st], want)
            tl, wt, wv = m.logprob_logits(z, int(ids[i, st]), top_n)
            assert bits(tlp[i, st]) == bits(np.float32(tl)), (i, st)
            assert np.array_equal(tt[i, st], wt) and np.array_equal(bits(tv[i, st]), bits(wv)), (i, st)
    m.set_history([0] * S)


def test_the_same_call_twice_is_bit_identical_and_a_prefix_leaves_other_rows_and_the_context_alone(decode_setup):
    m, batch, rows, _ = decode_setup
    P = len(PROMPT)
    golden = m.forward(45, P + 1)
    m.prefill(PROMPT, 1)                                             # (position P + 1 of the context's cache is not the prefix's business)
    b1, b2 = batch(), batch()
    args = (rows["slots"], rows["tokens"], rows["pos0"])
    lg1, am1 = b1.forward(*args)
    lg2, am2 = b1.forward(*args)                                     # the same forward on the same state
    assert np.array_equal(bits(lg1), bits(lg2)) and np.array_equal(am1, am2)
    lg3, _ = b2.forward(*args)                                       # ... and in another batch with the same prefix
    assert np.array_equal(bits(lg1), bits(lg3))
    sps = [llmk.sampler(**sp) for sp in SAMPLERS]
    assert np.array_equal(b1.decode(*args, STEPS, sps), b2.decode(*args, STEPS, sps))
    b1.close()
    b2.close()
    # unattached rows of a batch WITH a prefix: the bits of a batch that never had one
    with_prefix, never = llmk.Batch(m, 4), llmk.Batch(m, 4)
    with_prefix.set_prefix(P)
    for b in (with_prefix, never):
        b.fork(2, 7)
    plain = ([2, 0, 1], [61, 2, 9], [8, 1, 1])
    a = [with_prefix.forward(*plain, want_argmax=False), with_prefix.decode(*plain, STEPS)]
    c = [never.forward(*plain, want_argmax=False), never.decode(*plain, STEPS)]
    assert np.array_equal(bits(a[0]), bits(c[0])) and np.array_equal(a[1], c[1])
    with_prefix.close()
    never.close()
    # the prefix is a copy: the context goes on as if nothing had been set
    m.prefill(PROMPT, 1)
    assert np.array_equal(bits(m.forward(45, P + 1)), bits(golden))
    g = load_golden("tk-small-long")
    s = gguf.SHAPES[str(g["shape"])]
    mg = llmk.Llmk(gguf.synth_fused(s, int(g["seed"])))
    fed = [2] + g["tokens"].tolist()
    mg.prefill(fed[:40], 1)
    bg = llmk.Batch(mg, 2)
    bg.set_prefix(33)
    bg.attach(0)
    bg.forward([0], [fed[33]], [34], want_argmax=False)
    after = np.stack([mg.forward(fed[k - 1], k) for k in range(41, 49)])       # llmk_forward on the context after llmk_prefix_set
    assert rel_err(after, g["logits"][40:48]).max() <= REL_TOL
    bg.close()
    mg.close()


def test_an_attached_slot_against_the_same_slot_filled_by_fork(decode_setup):
    m, batch, rows, _ = decode_setup
    P = len(PROMPT)
    rng = np.random.default_rng(3)
    cont = (rng.integers(3, m.V, 40) + 1).tolist()
    out = {}
    for share in (True, False):
        b = batch(share)
        out[share] = np.stack([b.forward([1, 2], [tok, tok], [P + 1 + i] * 2, want_argmax=False)[0] for i, tok in enumerate(cont)])
        b.close()
    att, frk = out[True], out[False]
    assert rel_err(att, frk).max() <= REL_TOL and rel_err(frk, att).max() <= REL_TOL
    assert top8_elementwise(att, ref=frk).max() <= REL_TOL
    top2 = np.sort(frk, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 4 * REL_TOL * np.abs(frk).max(axis=1)      # the project's near-tie rule: 4e-4 x max |logit|
    assert clear.sum() > len(clear) // 2
    assert np.array_equal(np.argmax(att, axis=1)[clear], np.argmax(frk, axis=1)[clear])


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def code_of(fn, *a, **kw):
    with pytest.raises(llmk.LlmkError) as e:
        fn(*a, **kw)
    return e.value.code


def test_refusals_carry_the_documented_codes_and_leave_the_batch_working():
    E_ARG, E_STATE = 1, 5
    s = gguf.SHAPES["tk-small"]
    m = llmk.Llmk(gguf.synth_fused(s, 1))
    m.prefill(PROMPT, 1)
    P = len(PROMPT)
    b = llmk.Batch(m, 3, 32)
    fresh = b.forward([2], [5], [1], want_argmax=False)
    assert b.prefix_len == 0
    assert code_of(b.attach, 0) == E_STATE                                       # no prefix
    assert code_of(b.set_prefix, 32) == E_ARG                                    # n_pos = the batch's seq_len: no position left
    assert code_of(b.set_prefix, -1) == E_ARG
    b.set_prefix(31)                                                             # ... and up to seq_len - 1
    b.set_prefix(P)
    assert b.prefix_len == P
    assert code_of(b.attach, 3) == E_ARG and code_of(b.attach, -1) == E_ARG
    b.attach(0)
    assert code_of(b.set_prefix, 4) == E_STATE and code_of(b.set_prefix, 0) == E_STATE      # a slot is attached
    for pos in (1, P):                                                           # a row of an attached slot inside the prefix
        assert code_of(b.forward, [0], [5], [pos]) == E_ARG
        assert code_of(b.forward, [1, 0], [5, 5], [1, pos]) == E_ARG
        assert code_of(b.decode, [0], [5], [pos], 2) == E_ARG
        assert code_of(b.decode_rows, [0], [5], [pos], 2) == E_ARG
        assert code_of(b.sample_logits_rows, [0], [pos], np.zeros((1, m.V), np.float32), [llmk.sampler(temperature=1.0, seed=1)]) == E_ARG
    assert code_of(b.time, 1, P, 1) == E_ARG
    ref = m.forward(5, P + 1)                                                    # the batch stays usable
    lg = b.forward([0, 1], [5, 5], [P + 1, 1], want_argmax=False)
    assert rel_err(lg[0:1], ref[None]).max() <= REL_TOL
    assert b.time(2, P + 1, 2) > 0.0
    b.fork(0, 0)                                                                 # a fork detaches
    assert np.array_equal(bits(b.forward([0], [5], [1], want_argmax=False)), bits(fresh))
    b.set_prefix(0)                                                              # every slot detached: the prefix can go
    assert b.prefix_len == 0 and code_of(b.attach, 0) == E_STATE
    assert np.array_equal(bits(b.forward([2], [5], [1], want_argmax=False)), bits(fresh))
    b.close()
    m.close()
