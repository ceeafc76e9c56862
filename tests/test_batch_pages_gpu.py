"""Paged K/V caches for the batched decode (llmk_pages_*): one pool of pages, a table per slot.  What is new on the
device is bd_attn_paged_kernel (the tiles of a row found through the table), the paged QKV epilogues and the page copies; every test
reaches them through the public entry points.  f16 pools are held to the stored-row contract of tests/kv16_ref.py."""
import numpy as np
import pytest

import kv16_ref as kr
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf
from ref_pass import RefPass
from test_batch_span_gpu import bits, first_max, model, random_seq, within_the_bar

pytestmark = pytest.mark.gpu

E_ARG, E_TYPE, E_NOMEM = 1, 4, 7


def feed(b, slot, seq, pos0=1):
    """seq into `slot` one position per pass from pos0 on: logits [len][V]"""
    return np.stack([b.forward([slot], [t], [pos0 + i], want_argmax=False)[0] for i, t in enumerate(seq)])


def reference(b, fw32, kv, slot, seq):
    """the float64 pass on the sequence alone; an f16 pool: the pass fed the rows the slot stored, read back through its table"""
    if kv == "f32":
        return RefPass(fw32).feed(seq)
    return kr.forward_fed(fw32, seq, *kr.peek_all(b, fw32.shape.n_layers, slot, len(seq)))


def code_of(fn, *a, **kw):
    with pytest.raises(llmk.LlmkError) as e:
        fn(*a, **kw)
    return e.value.code


CASES = {
    "tiny-hs128w-f32": ("tiny-hs128w", gguf.GGML_F32, False, "f32"),
    "tiny-hs64-f16kv": ("tiny-hs64", gguf.GGML_F32, False, "f16"),
    "tiny-kvmul3-f32": ("tiny-kvmul3", gguf.GGML_F32, False, "f32"),        # head size 32, kv_mul 3: a padded column
    "tiny-gqa-f32": ("tiny-gqa", gguf.GGML_F32, False, "f32"),              # head size 16, kv_mul 4
    "tiny-gqa-f16kv": ("tiny-gqa", gguf.GGML_F32, False, "f16"),
    "tk-small-q4_0-q6k": ("tk-small", gguf.GGML_Q4_0, True, "f32"),
}


@pytest.mark.parametrize("page_len", [16, 48])
@pytest.mark.parametrize("cid", list(CASES))
def test_lockstep_slots_match_the_float64_pass_on_each_sequence_alone(cid, page_len):
    """positions 1 .. 2 * page_len + 1 of five slots, one pass per position: slot j's pages are j, j + 5, j + 10"""
    shape, wtype, q6k, kv = CASES[cid]
    fw, fw32 = model(shape, wtype, q6k)
    n, V = 2 * page_len + 1, fw.shape.vocab_size
    rng = np.random.default_rng(3)
    seqs = [random_seq(rng, V, n) for _ in range(5)]
    m = llmk.Llmk(fw, seq_len=n)
    b = llmk.Batch(m, 5, n, kv, page_len=page_len, n_pages=15)
    assert b.kv_type == kv and b.free_pages() == 15
    got = np.stack([b.forward(range(5), [s[t] for s in seqs], [t + 1] * 5, want_argmax=False) for t in range(n)], axis=1)
    tables = [b.page_table(j) for j in range(5)]
    assert tables == [[j, j + 5, j + 10] for j in range(5)] and b.free_pages() == 0
    assert any(np.any(np.diff(t) != 1) for t in tables)
    ref = [reference(b, fw32, kv, j, seqs[j]) for j in range(5)]
    b.close()
    m.close()
    for j in range(5):
        within_the_bar(f"{cid} page_len {page_len} slot {j}", got[j], ref[j])


def test_a_long_slot_runs_several_parts_next_to_two_short_slots():
    """tk-small-long, page_len 16: 300 positions into slot 0 by spans, then three passes of rows at positions 301.. | 1.. | 1..: 19
    tiles, 6 (row, kv head) pairs -- bd_parts gives 3 parts on a 256-CU device"""
    fw, fw32 = model("tk-small-long")
    s = fw.shape
    rng = np.random.default_rng(11)
    seqs = [random_seq(rng, s.vocab_size, 303), random_seq(rng, s.vocab_size, 3), random_seq(rng, s.vocab_size, 3)]
    ref = [RefPass(fw32).feed(seq) for seq in seqs]
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 3, page_len=16, n_pages=21)
    b.ingest(0, seqs[0][:300])
    got = np.stack([b.forward([2, 0, 1], [seqs[2][t], seqs[0][300 + t], seqs[1][t]], [t + 1, 301 + t, t + 1], want_argmax=False) for t in range(3)], axis=1)
    assert b.free_pages() == 0
    b.close()
    m.close()
    within_the_bar("long slot", got[1], ref[0][300:])
    within_the_bar("short slot 1", got[2], ref[1])
    within_the_bar("short slot 2", got[0], ref[2])


@pytest.mark.parametrize("kv", ["f32", "f16"])
def test_a_sequence_on_a_non_monotonic_table_gives_the_bits_of_a_fresh_batch(kv):
    fw, _ = model("tiny-gqa")
    rng = np.random.default_rng(5)
    seq = random_seq(rng, fw.shape.vocab_size, 40)
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 3, kv_type=kv, page_len=16, n_pages=4)
    feed(b, 0, seq[:1])                                  # page 0
    feed(b, 1, seq[:1])                                  # page 1
    got = [feed(b, 2, seq[:16])]                         # page 2
    b.release(0)
    got.append(feed(b, 2, seq[16:32], 17))               # page 0
    b.release(1)
    got.append(feed(b, 2, seq[32:], 33))                 # page 1
    assert b.page_table(2) == [2, 0, 1] and b.page_table(0) == [] and b.free_pages() == 1
    b.close()
    fresh = llmk.Batch(m, 3, kv_type=kv, page_len=16, n_pages=4)
    want = feed(fresh, 2, seq)
    assert fresh.page_table(2) == [0, 1, 2]
    fresh.close()
    m.close()
    assert np.array_equal(bits(np.concatenate(got)), bits(want))


@pytest.mark.parametrize("kv", ["f32", "f16"])
def test_share_maps_full_pages_and_a_write_into_a_shared_page_copies_it(kv):
    fw, fw32 = model("tiny-hs64")
    V, pl = fw.shape.vocab_size, 16
    n_pos = 2 * pl + 5
    rng = np.random.default_rng(7)
    a = random_seq(rng, V, n_pos + 9)
    d = a[:n_pos] + random_seq(rng, V, 10)[1:]           # dst: the stem, then tokens of its own
    m = llmk.Llmk(fw)

    def run(rewind):
        b = llmk.Batch(m, 2, kv_type=kv, page_len=pl, n_pages=8)
        out = {"src": feed(b, 0, a[:n_pos])}
        free = b.free_pages()
        b.share(1, 0, n_pos)
        assert b.free_pages() == free - 1                # dst newly owns the partial page alone
        assert b.page_table(0) == [0, 1, 2] and b.page_table(1) == [0, 1, 3]
        out["src"] = np.concatenate([out["src"], feed(b, 0, a[n_pos:n_pos + 8], n_pos + 1)])
        out["dst"] = feed(b, 1, d[n_pos:n_pos + 8], n_pos + 1)
        assert b.page_table(0) == [0, 1, 2] and b.page_table(1) == [0, 1, 3] and b.free_pages() == free - 1
        out["ref"] = [reference(b, fw32, kv, 0, a[:n_pos + 8]), reference(b, fw32, kv, 1, d[:n_pos + 8])]
        if rewind:                                       # src back into page 1, which dst holds too: src gets a copy
            feed(b, 0, [5, 6, 7], pl + 4)
            assert b.page_table(0) == [0, 4, 2] and b.page_table(1) == [0, 1, 3] and b.free_pages() == free - 2
        out["next"] = feed(b, 1, d[n_pos + 8:], n_pos + 9)
        b.close()
        return out
    got, plain = run(True), run(False)
    m.close()
    within_the_bar(f"{kv} src", got["src"], got["ref"][0])
    within_the_bar(f"{kv} dst", got["dst"], got["ref"][1][n_pos:])
    assert np.array_equal(bits(got["next"]), bits(plain["next"]))


def test_decode_crosses_a_page_boundary_without_the_host():
    """tk-small, page_len 16: 7 steps from positions 13 and 3 -- the first row crosses into its second page at step 4.  Greedy ids are
    the first maxima of step-by-step passes; llmk_rows_decode's picks and records are what the context's hooks answer on the logits of a
    replay, bit for bit (the rule of tests/test_batch_rows_gpu.py)."""
    fw = gguf.synth_fused(gguf.SHAPES["tk-small"], 4242)
    m = llmk.Llmk(fw)
    S, steps, stem = fw.shape.seq_len, 7, [2, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50]
    rows = dict(slots=[1, 0], tokens=[60, 7], pos0=[len(stem) + 1, 3])

    def batch():
        b = llmk.Batch(m, 2, page_len=16, n_pages=4)
        b.ingest(1, stem)
        b.ingest(0, stem[:2])
        return b

    def replay(ids):
        b = batch()
        lg = [b.forward(rows["slots"], rows["tokens"] if st == 0 else ids[:, st - 1].tolist(), [p + st for p in rows["pos0"]], want_argmax=False)
              for st in range(steps)]
        b.close()
        return np.stack(lg)
    b = batch()
    greedy = b.decode(rows["slots"], rows["tokens"], rows["pos0"], steps)
    assert b.page_table(1) == [0, 2] and b.page_table(0) == [1]
    assert np.array_equal(greedy, first_max(replay(greedy)).T)
    sps = [dict(temperature=0.9, seed=12), dict(temperature=0.8, seed=13, top_k=5)]
    pens = [dict(last_n=4, repeat=1.3), dict(last_n=64, frequency=0.7, presence=0.4)]
    b.set_history(1, stem)
    b.set_history(0, stem[:2])
    ids, tlp, tt, tv = b.decode_rows(rows["slots"], rows["tokens"], rows["pos0"], steps, [llmk.sampler(**sp) for sp in sps],
                                     [llmk.penalties(**pn) for pn in pens], top_n=3, want_token_logprob=True)
    b.close()
    lgs = replay(ids)
    for i, n in enumerate((len(stem), 2)):
        fed = stem[:n] + [rows["tokens"][i]] + ids[i, :-1].tolist()
        m.set_history(np.array(fed + [0] * (S - len(fed)), np.int32))
        for st in range(steps):
            assert ids[i, st] == m.sample_logits_pen(lgs[st, i], rows["pos0"][i] + st, **sps[i], **pens[i])[0], (i, st)
            tl, wt, wv = m.logprob_logits(lgs[st, i], int(ids[i, st]), 3)
            assert bits(tlp[i, st]) == bits(np.float32(tl)), (i, st)
            assert np.array_equal(tt[i, st], wt) and np.array_equal(bits(tv[i, st]), bits(wv)), (i, st)
    m.close()


def test_a_pool_one_page_short_answers_nomem_and_changes_nothing():
    fw, _ = model("tiny-gqa")
    rng = np.random.default_rng(9)
    seqs = [random_seq(rng, fw.shape.vocab_size, 34), random_seq(rng, fw.shape.vocab_size, 18)]
    m = llmk.Llmk(fw)

    def run(fail):
        b = llmk.Batch(m, 2, page_len=16, n_pages=4)
        feed(b, 0, seqs[0][:32])                          # pages 0, 1
        feed(b, 1, seqs[1][:16])                          # page 2
        tables = [b.page_table(0), b.page_table(1)]
        assert b.free_pages() == 1
        if fail:      # both rows need a page: the first takes the last one, the second finds none -- the first gives it back
            assert code_of(b.forward, [0, 1], [seqs[0][32], seqs[1][16]], [33, 17]) == E_NOMEM
            assert code_of(b.decode, [1], [seqs[1][15]], [16], 18) == E_NOMEM      # a decode asks for all its steps up front
            assert [b.page_table(0), b.page_table(1)] == tables and b.free_pages() == 1
        lg = b.forward([1, 0], [seqs[1][16], seqs[0][31]], [17, 32], want_argmax=False)      # fits: one page
        assert b.page_table(1) == [2, 3] and b.free_pages() == 0
        if fail:
            b.release(0, 16)
            assert b.page_table(0) == [0] and b.free_pages() == 1
            b.release(0)
            assert b.page_table(0) == [] and b.free_pages() == 2
        b.close()
        return lg
    assert np.array_equal(bits(run(True)), bits(run(False)))
    m.close()


def test_refusals_carry_the_documented_codes():
    fw, _ = model("tiny-gqa")
    m = llmk.Llmk(fw)
    m.prefill([2, 3, 4, 5], 1)
    assert code_of(llmk.Batch, m, 2, kv_type="q8_0", page_len=16, n_pages=4) == E_TYPE
    assert code_of(llmk.Batch, m, 2, page_len=24, n_pages=4) == E_ARG
    assert code_of(llmk.Batch, m, 2, page_len=16, n_pages=0) == E_ARG
    b = llmk.Batch(m, 2, page_len=16, n_pages=4)
    assert code_of(b.set_prefix, 2) == E_ARG and code_of(b.attach, 0) == E_ARG
    assert code_of(b.forward_tree, [(0, 1, 3)], [2, 3, 4], [-1, 0, 0]) == E_ARG
    assert code_of(b.accept, 0, 1, [0, 2]) == E_ARG
    assert b.free_pages() == 4 and b.page_table(0) == []                       # ... before anything ran
    lg, am = b.forward_tree([(0, 1, 3)], [2, 3, 4], [-1, 0, 1])                 # a chain is a span pass
    assert np.array_equal(am, first_max(lg)) and b.page_table(0) == [0]
    b.fork(1, 4)                                                                # the context's rows into a fresh page
    forked = [b.peek_kv(which, 1, 1, 1, 4) for which in (0, 1)]
    assert b.page_table(1) == [1]
    b.close()
    dense = llmk.Batch(m, 2)
    dense.fork(1, 4)
    assert all(np.array_equal(bits(forked[which]), bits(dense.peek_kv(which, 1, 1, 1, 4))) for which in (0, 1))
    assert code_of(dense.release, 0) == E_ARG and code_of(dense.share, 1, 0, 1) == E_ARG
    assert code_of(dense.free_pages) == E_ARG and code_of(dense.page_table, 0) == E_ARG
    dense.close()
    m.close()
