"""The rows functions (llmk_rows_*): the three sampler kernels with one workgroup per row of a batched pass, and
the batch entry points that take per-row penalties, logit bias and log-prob requests.  A row's pick and record are DEFINED as what the
context's single-vector hooks (llmk_sample_logits_pen, llmk_logprob_logits) answer for that row's logits, so every comparison here is
exact: ints as ints, floats as their 32-bit patterns (NaN and the sign of zero count).

  1  the grid against the single-vector hooks on crafted logits, 128 rows in a permutation of the slots
  2  decode against the hooks: four rows, four samplers, four kinds of penalties, records; the greedy form
  3  decode_rows with samplers only IS Batch.decode
  4  a wide pass: 128 ragged rows, 3 steps
  5  the other classifier forms (q6_K per row and as a GEMM, f16)
  6  a call that is redone on the f32 matrix instruction
  7  refusals; fork zeroes a slot's record
"""
import ctypes as C

import numpy as np
import pytest

from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf

pytestmark = pytest.mark.gpu

E_ARG, E_NONFINITE = 1, 11


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def first_max(row):
    """0-based index of the first maximum among the rows that are not NaN"""
    row = np.asarray(row)
    return int(np.argmax(np.where(np.isnan(row), -np.inf, row)))


def sampler_cycle(i):
    """row i's sampler: no filter; top_k = 1; top_k = 40; top_p = 0.9; min_p = 0.05; all three"""
    extra = [dict(), dict(top_k=1), dict(top_k=40), dict(top_p=0.9), dict(min_p=0.05), dict(top_k=40, top_p=0.9, min_p=0.05)][i % 6]
    return dict(temperature=0.9, seed=100 + i, **extra)


def penalty_cycle(i, banned, shared):
    """row i's penalties: nothing on; repeat over 8; frequency and presence over 16; a bias list that bans `banned` (1-based); a bias
    and a penalty on the same token `shared` (1-based, inside the row's window)"""
    return [dict(),
            dict(last_n=8, repeat=1.3),
            dict(last_n=16, frequency=0.7, presence=0.4),
            dict(bias=[(banned, -np.inf)]),
            dict(last_n=8, repeat=1.5, bias=[(shared, 2.5)])][i % 5]


def hooks(m, logits, pos, sp, pen, top_n):
    """what the context's two hooks answer for one vector (the context's record is already loaded): the pick, kept, tau, the adjusted
    vector, and the record of the RAW vector for that pick"""
    tok, kept, tau, adj = m.sample_logits_pen(logits, pos, **sp, **pen)
    tl, tt, tv = m.logprob_logits(logits, tok, top_n)
    return tok, kept, tau, adj, tl, tt, tv


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
def test_the_grid_matches_the_single_vector_hooks_on_crafted_logits():
    """tk-small's geometry with V = 2500 (more than two sweeps of the 1,024 threads, no multiple of 1,024, a multiple of 4 as the f32
    classifier GEMM needs) and seq_len 16; 128 slots, 128 rows in a seeded permutation of the slots"""
    V, S, N = 2500, 16, 128
    shape = gguf.LlamaShape(256, 768, 2, 4, 2, V, S)
    m = llmk.Llmk(gguf.synth_fused(shape, 99))
    b = llmk.Batch(m, N)
    rng = np.random.default_rng(20261019)
    slots = rng.permutation(N).astype(np.int32)
    pos = (1 + (np.arange(N) * 5) % S).astype(np.int32)
    assert set(pos.tolist()) == set(range(1, S + 1))
    logits = (rng.standard_normal((N, V)) * 3).astype(np.float32)
    logits[10, 0] = logits[10, 1024] = np.nan                  # (row 10: penalties off, min_p)
    logits[21, [300, 2047]] = np.inf                           # two +inf maxima (repeat penalty, top_p)
    logits[32, :] = np.float32(1.25)                           # all rows equal (frequency / presence, top_k 40)
    logits[44, :] = -np.inf                                    # -inf everywhere but one (bias + penalty, top_k 40)
    logits[44, 1500] = np.float32(0.5)
    logits[53, :] = -np.abs(logits[53])                        # a mix of -0.0 and +0.0 at the maximum (the first one banned)
    logits[53, [7, 1100, 2499]] = np.float32(-0.0)
    logits[53, [600, 2048]] = np.float32(0.0)
    # the slots' records: small ids, so zeros (none) and repeats are common
    records = rng.integers(0, 40, (N, S)).astype(np.int32)
    sps, pens = [], []
    for i in range(N):
        if records[slots[i], pos[i] - 1] == 0:
            records[slots[i], pos[i] - 1] = 1 + i % 37        # the row's window holds a token at its own position
        sps.append(sampler_cycle(i))
        pens.append(penalty_cycle(i, first_max(logits[i]) + 1, int(records[slots[i], pos[i] - 1])))
    assert (records == 0).any() and pens[44]["bias"][0][0] != 1501
    for j in range(N):
        b.set_history(j, records[j])
    bsp = [llmk.sampler(**sp) for sp in sps]
    bpn = [llmk.penalties(**pn) for pn in pens]

    want = {}
    for tn in (0, 5, 20):
        tok, kept, tau, adj, tlp, *tops = b.sample_logits_rows(slots, pos, logits, bsp, bpn, top_n=tn, want_token_logprob=True)
        again = b.sample_logits_rows(slots, pos, logits, bsp, bpn, top_n=tn, want_token_logprob=True)
        for x, y in zip((tok, kept, tau, adj, tlp, *tops), again):      # a count left behind by the first call would show here
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), tn
        for i in range(N):
            m.set_history(records[slots[i]])
            if tn == 0:
                want[i] = m.sample_logits_pen(logits[i], int(pos[i]), **sps[i], **pens[i])
            wtok, wkept, wtau, wadj = want[i]
            assert (tok[i], kept[i]) == (wtok, wkept), (tn, i, tok[i], wtok, kept[i], wkept)
            assert bits(tau[i]) == bits(np.float32(wtau)), (tn, i)
            assert np.array_equal(bits(adj[i]), bits(wadj)), (tn, i)
            tl, tt, tv = m.logprob_logits(logits[i], wtok, tn)
            assert bits(tlp[i]) == bits(np.float32(tl)), (tn, i)
            if tn:
                assert np.array_equal(tops[0][i], tt) and np.array_equal(bits(tops[1][i]), bits(tv)), (tn, i)
        if tn == 20:
            wide = (tok, kept, tau, adj, tlp, *tops)
    for j in range(N):                                         # the hook reads the records and writes none
        assert np.array_equal(b.get_history(j, S), records[j]), j
    where = {int(s): i for i, s in enumerate(slots)}
    for few in ([97], [97, 2, 41]):                            # fewer rows, other row indices, the same slots: the same answers
        idx = [where[s] for s in few]
        got = b.sample_logits_rows(few, pos[idx], logits[idx], [bsp[i] for i in idx], [bpn[i] for i in idx], top_n=20, want_token_logprob=True)
        for x, y in zip(got, wide):
            assert np.array_equal(x.view(np.uint32), y[idx].view(np.uint32)), few
    b.close()
    m.close()


# ---- 2, 3 ---------------------------------------------------------------------------------------------------------------------------
SAMPLERS = [dict(temperature=1.0, seed=11, top_k=1),                       # greedy through the sampler
            dict(temperature=0.9, seed=12),
            dict(temperature=0.8, seed=13, top_k=5),
            dict(temperature=1.1, seed=14, top_p=0.9, min_p=0.05)]
STEPS = 12
PROMPT = [2, 40, 41, 42, 43, 44]


@pytest.fixture(scope="module")
def decode_setup():
    """tk-small f32 with a 6-token prompt on the context; rows 0, 1 start in fresh slots, rows 2, 3 behind the forked prompt, whose
    tokens are recorded as the caller of a context records them"""
    s = gguf.SHAPES["tk-small"]
    m = llmk.Llmk(gguf.synth_fused(s, 4242))
    m.prefill(PROMPT, 1)

    def batch():
        b = llmk.Batch(m, 4)
        for slot in (1, 2):
            b.fork(slot, len(PROMPT))
            b.set_history(slot, PROMPT)
        return b
    rows = dict(slots=[3, 1, 0, 2], tokens=[2, 50, 7, 60], pos0=[1, len(PROMPT) + 1, 1, len(PROMPT) + 1])
    before = {3: [], 1: PROMPT, 0: [], 2: PROMPT}
    yield m, batch, rows, before
    m.close()


def replay(b, rows, ids):
    """feed a decode's ids step by step through llmk_batch_forward: logits [steps][n][V]"""
    lgs = []
    for st in range(ids.shape[1]):
        toks = rows["tokens"] if st == 0 else ids[:, st - 1].tolist()
        lgs.append(b.forward(rows["slots"], toks, [p + st for p in rows["pos0"]], want_argmax=False))
    return np.stack(lgs)


def check_decode(m, batch, rows, before, S, steps, sps, pens, top_n):
    """decode_rows on a fresh batch() against the hooks on the logits of a replay through another fresh batch(); sps None: the greedy
    form.  before[slot]: what the slot's record holds in front of the call.  Returns the ids."""
    n = len(rows["slots"])
    b = batch()
    ids, tlp, tt, tv = b.decode_rows(rows["slots"], rows["tokens"], rows["pos0"], steps, [llmk.sampler(**sp) for sp in sps] if sps else None,
                                     [llmk.penalties(**pn) for pn in pens] if pens else None, top_n=top_n, want_token_logprob=True)
    hist = [b.get_history(slot, S) for slot in rows["slots"]]
    b.close()
    assert ids.shape == (n, steps) and ids.min() >= 1 and ids.max() <= m.V
    b2 = batch()
    lgs = replay(b2, rows, ids)
    b2.close()
    for i, slot in enumerate(rows["slots"]):
        fed = list(before[slot]) + [rows["tokens"][i]] + ids[i, :-1].tolist()      # the prompt, the first token, the ids but the last
        assert len(fed) == rows["pos0"][i] + steps - 1
        record = np.array(fed + [0] * (S - len(fed)), np.int32)
        if pens:
            assert np.array_equal(hist[i], record), (i, hist[i], record)
        else:                                                                       # (no penalties: no record is touched)
            assert np.array_equal(hist[i], np.array(list(before[slot]) + [0] * (S - len(before[slot])), np.int32)), i
        m.set_history(record)
        for st in range(steps):
            z = lgs[st, i]
            if sps:
                want = m.sample_logits_pen(z, rows["pos0"][i] + st, **sps[i], **(pens[i] if pens else {}))[0]
            else:
                want = first_max(z) + 1
            assert ids[i, st] == want, (i, st, ids[i, st], want)
            tl, wt, wv = m.logprob_logits(z, int(ids[i, st]), top_n)
            assert bits(tlp[i, st]) == bits(np.float32(tl)), (i, st)
            assert np.array_equal(tt[i, st], wt) and np.array_equal(bits(tv[i, st]), bits(wv)), (i, st)
    return ids


def test_decode_rows_picks_and_records_what_the_hooks_answer(decode_setup):
    m, batch, rows, before = decode_setup
    S = m.shape.seq_len
    sps = [llmk.sampler(**sp) for sp in SAMPLERS]
    b = batch()
    plain = b.decode(rows["slots"], rows["tokens"], rows["pos0"], STEPS, sps)
    b.close()
    pens = [dict(),                                                             # nothing on: still recorded
            dict(last_n=4, repeat=1.3),                                         # a window shorter than the history
            dict(last_n=64, frequency=0.7, presence=0.4, bias=[(3, 1.5), (500, -2.0), (1024, 0.25)]),
            dict(bias=[(int(plain[3, 0]), -np.inf)])]                           # bans what the row picks at step 0 without penalties
    ids = check_decode(m, batch, rows, before, S, STEPS, SAMPLERS, pens, 3)
    assert ids[3, 0] != plain[3, 0]                                             # the ban did bite
    # the greedy form with records: Batch.decode's greedy ids
    b = batch()
    greedy = b.decode(rows["slots"], rows["tokens"], rows["pos0"], STEPS)
    b.close()
    assert np.array_equal(check_decode(m, batch, rows, before, S, STEPS, None, None, 3), greedy)


def test_decode_rows_with_samplers_only_is_batch_decode(decode_setup):
    m, batch, rows, _ = decode_setup
    sps = [llmk.sampler(**sp) for sp in SAMPLERS]
    args = (rows["slots"], rows["tokens"], rows["pos0"], STEPS)
    b = batch()
    old, new = b.decode(*args, sps), b.decode_rows(*args, sps)
    assert np.array_equal(old, new)
    assert np.array_equal(old, b.decode(*args, sps)) and np.array_equal(new, b.decode_rows(*args, sps))
    assert np.array_equal(b.decode(*args), b.decode_rows(*args))               # ... and greedy
    b.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def test_a_wide_pass_of_ragged_rows():
    """128 rows, 3 steps; slot j sits behind the first j % 8 tokens of an 8-token prefill, so the positions of a pass are ragged"""
    s = gguf.SHAPES["tk-small"]
    N, steps = 128, 3
    m = llmk.Llmk(gguf.synth_fused(s, 777))
    prompt = [2, 90, 91, 92, 93, 94, 95, 96]
    m.prefill(prompt, 1)
    before = {j: prompt[:j % 8] for j in range(N)}

    def batch():
        b = llmk.Batch(m, N)
        for j in range(N):
            b.fork(j, j % 8)
            if j % 8:
                b.set_history(j, before[j])
        return b
    rng = np.random.default_rng(4)
    slots = rng.permutation(N).tolist()
    rows = dict(slots=slots, tokens=[3 + i for i in range(N)], pos0=[j % 8 + 1 for j in slots])
    b = batch()
    lg0 = b.forward(rows["slots"], rows["tokens"], rows["pos0"], want_argmax=False)      # the first step's logits: what to ban
    b.close()
    sps = [sampler_cycle(i) for i in range(N)]
    pens = [penalty_cycle(i, first_max(lg0[i]) + 1, rows["tokens"][i]) for i in range(N)]
    check_decode(m, batch, rows, before, s.seq_len, steps, sps, pens, 2)
    m.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["tk-small-q4_0-q6k", "tk-small-f16"])
def test_other_classifier_forms(cid):
    s = gguf.SHAPES["tk-small"]
    fw = gguf.synth_fused(s, 777, gguf.GGML_Q4_0 if "q4_0" in cid else gguf.GGML_F16)
    if "q6k" in cid:
        fw = gguf.with_q6k_classifier(fw)
    m = llmk.Llmk(fw)
    forms = {n: m.cls_form(n) for n in (2, 4)}
    print(f"{cid}: classifier forms {forms} (1 = GEMM, 2 = per row)")
    if "q6k" in cid:
        assert forms[2] == llmk.CLS_ROWS
    for n in (2, 4):
        rows = dict(slots=list(range(n))[::-1], tokens=[20 + i for i in range(n)], pos0=[1 + i for i in range(n)])
        before = {slot: [0] * (p - 1) for slot, p in zip(rows["slots"], rows["pos0"])}      # (fresh slots: nothing fed before pos0)
        sps = [sampler_cycle(i + 2) for i in range(n)]
        pens = [dict(last_n=8, repeat=1.3)] * n
        check_decode(m, lambda: llmk.Batch(m, 4), rows, before, s.seq_len, 4, sps, pens, 2)
    m.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
def test_a_redone_call_leaves_the_records_of_the_tokens_fed():
    """FFN gains of 1e5 put activations beyond 65504 (the "large" construction of tests/test_score_gpu.py): the first call raises the
    f16-range flag and is redone on the f32 matrix instruction, where the context then stays -- for the replay too"""
    s = gguf.SHAPES["tk-small16"]
    fw = gguf.synth_fused(s, 77, 0)
    fw.rms_ffn_weight = (fw.rms_ffn_weight * np.float32(1e5)).astype(np.float32)
    m = llmk.Llmk(fw)
    rows = dict(slots=[1, 0], tokens=[2, 417], pos0=[1, 3])
    before = {0: [0, 0], 1: []}                                 # (slot 0 starts at position 3 of an empty cache: nothing fed before)
    sps = [sampler_cycle(2), sampler_cycle(3)]
    pens = [dict(last_n=8, repeat=1.3), dict(last_n=4, frequency=0.5, presence=0.2, bias=[(9, 1.0)])]
    check_decode(m, lambda: llmk.Batch(m, 2), rows, before, s.seq_len, 4, sps, pens, 2)
    m.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def code_of(fn, *a, **kw):
    with pytest.raises(llmk.LlmkError) as e:
        fn(*a, **kw)
    return e.value.code


def test_refusals_carry_the_documented_codes_and_leave_the_batch_working():
    s = gguf.SHAPES["tk-small"]
    m = llmk.Llmk(gguf.synth_fused(s, 1))
    b = llmk.Batch(m, 3, 32)
    L = llmk.lib()
    ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
    rows = ([2, 0], [5, 6], [1, 4])
    sps = [llmk.sampler(0.9, 1, top_k=40), llmk.sampler(1.1, 2)]
    pens = [llmk.penalties(last_n=8, repeat=1.3), llmk.penalties(bias=[(7, -1.0)])]
    ref = b.decode_rows(*rows, 5, sps, pens, top_n=2, want_token_logprob=True)

    assert code_of(b.decode_rows, *rows, 5, None, pens) == E_ARG                                     # penalties without samplers
    assert code_of(b.decode_rows, *rows, 5, sps, [pens[0], llmk.penalties(bias=[(5, 1.0), (5, 2.0)])]) == E_ARG      # a bias id twice
    assert code_of(b.decode_rows, *rows, 5, sps, [pens[0], llmk.penalties(bias=[(s.vocab_size + 1, 1.0)])]) == E_ARG
    assert code_of(b.decode_rows, *rows, 5, sps, [llmk.penalties(last_n=33, repeat=1.2), pens[1]]) == E_ARG         # beyond the BATCH's seq_len
    assert code_of(b.decode_rows, *rows, 5, sps, pens, top_n=21) == E_ARG
    assert code_of(b.sample_logits_rows, [0], [1], np.zeros((1, m.V), np.float32), sps[:1], None, top_n=21) == E_ARG
    a = [np.ascontiguousarray(x, np.int32) for x in rows]
    ids = np.zeros((2, 5), np.int32)
    need = llmk.Logprobs(3, None, None, None)                                                        # a NULL array that top_n needs
    arr = (llmk.Sampler * 2)(*sps)
    assert L.llmk_rows_decode(b._h, 2, *[x.ctypes.data_as(ip) for x in a], 5, arr, None, C.byref(need), ids.ctypes.data_as(ip)) == E_ARG
    nothing = llmk.Logprobs(0, None, None, None)                                                     # nothing asked for
    assert L.llmk_rows_decode(b._h, 2, *[x.ctypes.data_as(ip) for x in a], 5, arr, None, C.byref(nothing), ids.ctypes.data_as(ip)) == E_ARG
    assert code_of(b.set_history, 3, [1, 2]) == E_ARG and code_of(b.set_history, -1, [1, 2]) == E_ARG  # no such slot
    assert code_of(b.get_history, 3, 2) == E_ARG
    assert code_of(b.set_history, 0, [1] * 33) == E_ARG and code_of(b.set_history, 0, [s.vocab_size + 1]) == E_ARG
    z = np.zeros((1, m.V), np.float32)
    one, tok = np.array([0], np.int32), np.zeros(1, np.int32)
    assert L.llmk_rows_sample_logits(b._h, 1, one.ctypes.data_as(ip), (one + 1).ctypes.data_as(ip), z.ctypes.data_as(fp), None, None, None,
                                     tok.ctypes.data_as(ip), None, None, None) == E_ARG              # the hook without samplers
    z2 = np.zeros((2, m.V), np.float32)
    z2[1, :] = -np.inf                                                                               # a row with no row above -inf
    assert code_of(b.sample_logits_rows, [0, 1], [1, 1], z2, sps) == E_NONFINITE
    assert b.sample_logits_rows([0, 1], [1, 1], np.zeros((2, m.V), np.float32), sps)[0].min() >= 1   # ... and the batch stays usable

    # fork empties the slot's record, and only that slot's
    b.set_history(1, [5, 6, 7])
    b.set_history(0, [8, 9])
    b.fork(1, 0)
    assert not b.get_history(1, 32).any() and b.get_history(0, 3).tolist() == [8, 9, 0]
    b.fork(0, 0)
    b.fork(2, 0)
    # nothing of the above broke anything: the same call gives the same bits as before
    again = b.decode_rows(*rows, 5, sps, pens, top_n=2, want_token_logprob=True)
    for x, y in zip(ref, again):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    b.close()
    m.close()
