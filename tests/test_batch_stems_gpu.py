"""Stem reads of a paged batch (llmk_stems_*) through the public entry points, against the float64 pass on each
sequence alone (an f16 pool: fed the rows the slot stored, tests/kv16_ref.py)."""
import numpy as np
import pytest

import batch_tiles as bt
import kv16_ref as kr
import prefix_tiles as pt
from llm_f90_amd import llmk
from ref_pass import RefPass
from test_batch_span_gpu import bits, first_max, model, random_seq, within_the_bar

pytestmark = pytest.mark.gpu

PL = 16
STEM = 2 * PL + 5          # two full pages and a partial one: the partial page of a share is a copy and is not shared
KVS = pytest.mark.parametrize("kv", ["f32", "f16"])


def refs(b, fw32, kv, seqs, n0s):
    """the float64 logits of positions n0s[j] + 1 .. of seqs[j], which slot j holds, one sequence behind the other"""
    L = fw32.shape.n_layers
    return np.concatenate([RefPass(fw32).feed(s)[n0:] if kv == "f32" else
                           kr.forward_fed(fw32, s[n0:], *kr.peek_all(b, L, j, len(s)), pos=np.arange(n0 + 1, len(s) + 1))
                           for j, (s, n0) in enumerate(zip(seqs, n0s))])


def shared(m, kv, stem, n, share=True, extra=0):
    """a paged batch of n (+ extra) slots, the first n behind `stem`: slot 0 fed, the others sharing its pages (share=False: each fed it)"""
    b = llmk.Batch(m, n + extra, kv_type=kv, page_len=PL, n_pages=(n + extra) * -(-(len(stem) + 8) // PL))
    b.ingest(0, stem)
    for j in range(1, n):
        b.share(j, 0, len(stem)) if share else b.ingest(j, stem)
    return b


def passes(b, tails, pos0):
    """one pass per position of the tails, row j = slot j from pos0[j] on: logits [rows][len][V]"""
    return np.stack([b.forward(range(len(tails)), [t[k] for t in tails], [p + k for p in pos0], want_argmax=False) for k in range(len(tails[0]))], axis=1)


def case(shape, seed=21):
    fw, fw32 = model(shape)
    s, rng = fw.shape, np.random.default_rng(seed)
    n = pt.rg(s.n_heads // s.n_kv_heads) + 1
    return fw, fw32, n, random_seq(rng, s.vocab_size, STEM), [(rng.integers(3, s.vocab_size, 3) + 1).tolist() for _ in range(n)]


@KVS
@pytest.mark.parametrize("shape", ["tiny-gqa", "tiny-hs64"])
def test_a_full_group_and_a_leftover_match_the_float64_pass(shape, kv):
    """RG + 1 rows behind one stem of 37 positions: the first RG are a group with a stem of 32, the leftover row leads no one"""
    fw, fw32, n, stem, tails = case(shape)
    m = llmk.Llmk(fw)
    b = shared(m, kv, stem, n)
    b.stem_reads(True)
    assert [x.tolist() for x in b.stem_plan(range(n), [STEM + 1] * n)] == [[0] * (n - 1) + [-1], [2 * PL] * (n - 1) + [0]]
    got = passes(b, tails, [STEM + 1] * n)
    ref = refs(b, fw32, kv, [stem + t for t in tails], [STEM] * n)
    b.close()
    m.close()
    within_the_bar(f"{shape} {kv}", np.concatenate(got), ref)


@KVS
def test_a_tree_of_stems_and_a_stranger(kv):
    """A and B share 3 pages, C only the first of them, D nothing: {A, B} with a stem of 48, C and D on their own, in one pass"""
    fw, fw32 = model("tiny-gqa")
    V = fw.shape.vocab_size
    rng = np.random.default_rng(23)
    a = random_seq(rng, V, 3 * PL + 6)
    seqs = [a, a[:-1] + [a[-1] % (V - 3) + 3], a[:PL + 3] + random_seq(rng, V, 25)[1:], random_seq(rng, V, 3 * PL + 6)]
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 4, kv_type=kv, page_len=PL, n_pages=16)
    b.ingest(0, a[:-1])
    b.share(1, 0, len(a) - 1)
    b.share(2, 0, PL + 3)
    b.ingest(2, seqs[2][PL + 3:-1], PL + 4)
    b.ingest(3, seqs[3][:-1])
    pos = [len(s) for s in seqs]
    b.stem_reads(True)
    assert [x.tolist() for x in b.stem_plan(range(4), pos)] == [[0, 0, -1, -1], [3 * PL, 3 * PL, 0, 0]]
    got = b.forward(range(4), [s[-1] for s in seqs], pos, want_argmax=False)
    ref = refs(b, fw32, kv, seqs, [p - 1 for p in pos])
    b.close()
    m.close()
    within_the_bar(f"tree of stems {kv}", got, ref)


def test_a_long_stem_runs_several_stem_parts_next_to_a_short_one():
    """tk-small-long: 3 rows behind 309 positions and 2 behind 37 -- stems of 19 and 2 tiles, 2 groups, 2 kv heads: bd_parts gives
    more than one part of the longest stem, and the parts behind the short stem's tiles are empty"""
    fw, fw32 = model("tk-small-long")
    s, rng = fw.shape, np.random.default_rng(11)
    stems_ = [random_seq(rng, s.vocab_size, 19 * PL + 5)] * 3 + [random_seq(rng, s.vocab_size, STEM)] * 2
    tails = [(rng.integers(3, s.vocab_size, 2) + 1).tolist() for _ in range(5)]
    pos0 = [len(st) + 1 for st in stems_]
    m = llmk.Llmk(fw)
    b = shared(m, "f32", stems_[0], 3, extra=2)
    b.ingest(3, stems_[3])
    b.share(4, 3, STEM)
    b.stem_reads(True)
    assert [x.tolist() for x in b.stem_plan(range(5), pos0)] == [[0, 0, 0, 1, 1], [19 * PL] * 3 + [2 * PL] * 2]
    parts = bt.bd_parts(2, s.n_kv_heads, 19 * PL)              # the split rule on (groups, kv heads, longest stem): several parts,
    assert parts > 1 and -(-19 // parts) >= 2                  # the short stem's two tiles all in the first
    got = passes(b, tails, pos0)
    ref = refs(b, fw32, "f32", [st + t for st, t in zip(stems_, tails)], [p - 1 for p in pos0])
    b.close()
    m.close()
    within_the_bar("long and short stem", np.concatenate(got), ref)


@KVS
def test_off_is_the_parent_and_no_group_is_the_parent(kv):
    """never enabled | enabled and disabled | enabled with nothing shared: the bits of a fresh paged batch; shared and on: two runs of
    the same calls give the same bits, within the bar of stem reads off"""
    fw, _, n, stem, tails = case("tiny-gqa")
    m = llmk.Llmk(fw)

    def run(share, *switch):
        b = shared(m, kv, stem, n, share)
        for on in switch:
            b.stem_reads(on)
        out = passes(b, tails, [STEM + 1] * n)
        b.close()
        return out
    plain, alone = run(True), run(False)
    assert np.array_equal(bits(run(True, True, False)), bits(plain))
    assert np.array_equal(bits(run(False, True)), bits(alone))
    on = run(True, True)
    assert np.array_equal(bits(run(True, True)), bits(on))
    m.close()
    within_the_bar(f"{kv} on against off", np.concatenate(on), np.concatenate(plain))


def test_decode_groups_once_and_crosses_a_page():
    """7 steps behind the three passes of the first test, stem reads on; row 1, five positions further on than the others, crosses
    from its partial page into a new one at step 4 (position 49).  The ids are the first maxima of a step-by-step replay"""
    fw, _, n, stem, tails = case("tiny-gqa")
    m = llmk.Llmk(fw)
    steps, toks, pos0 = 7, [5 + j for j in range(n)], [STEM + 4 + 5 * (j == 1) for j in range(n)]

    def batch():
        b = shared(m, "f32", stem, n)
        b.stem_reads(True)
        passes(b, tails, [STEM + 1] * n)
        b.ingest(1, [9, 10, 11, 12, 13], STEM + 4)
        assert b.stem_plan(range(n), pos0)[0].tolist() == [0] * (n - 1) + [-1]
        return b
    b = batch()
    ids = b.decode(range(n), toks, pos0, steps)
    assert [len(b.page_table(j)) for j in range(n)] == [3, 4] + [3] * (n - 2)
    b.close()
    b = batch()
    lg = [b.forward(range(n), toks if st == 0 else ids[:, st - 1].tolist(), [p + st for p in pos0], want_argmax=False) for st in range(steps)]
    b.close()
    m.close()
    assert np.array_equal(ids, first_max(np.stack(lg)).T)


@KVS
def test_a_write_into_a_shared_page_copies_it_and_the_stem_ends_in_front(kv):
    """slot 1 shares 3 full pages with slot 0 and is fed at position 2 * PL + 4, inside the third: the plan says 2 pages before and
    after the copy, the table then shows a fresh page, and both rows match the float64 pass"""
    fw, fw32 = model("tiny-gqa")
    a = random_seq(np.random.default_rng(29), fw.shape.vocab_size, 3 * PL + 1)
    d = a[:2 * PL + 3] + [a[2 * PL + 3] % (fw.shape.vocab_size - 3) + 3]
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 2, kv_type=kv, page_len=PL, n_pages=8)
    b.ingest(0, a[:-1])
    b.share(1, 0, 3 * PL)
    b.stem_reads(True)
    pos, before = [len(a), len(d)], [x.tolist() for x in b.stem_plan([0, 1], [len(a), len(d)])]
    got = b.forward([0, 1], [a[-1], d[-1]], pos, want_argmax=False)
    assert b.page_table(0) == [0, 1, 2, 3] and b.page_table(1) == [0, 1, 4]
    assert before == [x.tolist() for x in b.stem_plan([0, 1], pos)] == [[0, 0], [2 * PL, 2 * PL]]
    ref = refs(b, fw32, kv, (a, d), [len(a) - 1, len(d) - 1])
    b.close()
    m.close()
    within_the_bar(f"copy on write {kv}", got, ref)
