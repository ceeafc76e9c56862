"""Span passes of a paged batch run bd_attn_span_paged_kernel (csrc/paged.h): bd_attn_span_kernel's groups, parts and
tile order with every tile found through the slot's table -- so they owe the BITS of the dense span kernel on the same rows."""
import os

import numpy as np
import pytest

import kv16_ref as kr
import span_tiles as st
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf
from ref_pass import RefPass
from test_batch_span_gpu import bits, first_max, model, random_seq, within_the_bar

pytestmark = pytest.mark.gpu

# (shape, weights, q6_K classifier, K/V type, positions slot three holds before the pass, rows of its span)
CASES = {
    "tiny-gqa-f32": ("tiny-gqa", gguf.GGML_F32, False, "f32", 29, 37),          # head size 16, kv_mul 4: 4 rows per group
    "tiny-kvmul3-f32": ("tiny-kvmul3", gguf.GGML_F32, False, "f32", 29, 37),    # head size 32, kv_mul 3: 5 rows and a padded column
    "tiny-hs128w-f32": ("tiny-hs128w", gguf.GGML_F32, False, "f32", 29, 37),    # kv_mul 1: 16 rows per group
    "tiny-hs64-f16kv": ("tiny-hs64", gguf.GGML_F32, False, "f16", 29, 37),
    "tk-small-q4_0-q6k": ("tk-small", gguf.GGML_Q4_0, True, "f32", 29, 37),
    "tk-small-long-wide": ("tk-small-long", gguf.GGML_F32, False, "f32", 300, 100),      # 110 rows, 25 tiles: 4 parts over 16 groups
}


@pytest.mark.parametrize("page_len", [16, 48])
@pytest.mark.parametrize("cid", list(CASES))
def test_ragged_spans_give_the_bits_of_the_dense_span_kernel(cid, page_len):
    """Slots two and three hold 13 and 29 positions; ONE pass of spans of 1, rg + 1 and 37 rows at 1, 14 and 30 (groups, tiles and pages
    break inside a span) on a dense and a paged batch of one context: the same bits.  The per-row kernel the paged pass ran before
    happens to sum in the span kernel's order while a pass has ONE part, so the five small shapes agreed bit for bit then too;
    tk-small-long-wide did not: four parts on a 256-CU device where the per-row split of its 110 rows has one."""
    shape, wtype, q6k, kv, held, rows = CASES[cid]
    fw, _ = model(shape, wtype, q6k)
    rg, S = max(1, 16 // (fw.shape.n_heads // fw.shape.n_kv_heads)), held + rows
    rng = np.random.default_rng(17)
    seqs = [random_seq(rng, fw.shape.vocab_size, n) for n in (1, 14 + rg, S)]
    m = llmk.Llmk(fw, seq_len=S)
    got = []
    for pool in ({}, dict(page_len=page_len, n_pages=3 * -(-S // page_len))):
        b = llmk.Batch(m, 3, S, kv, **pool)
        b.ingest(1, seqs[1][:13])
        b.ingest(2, seqs[2][:held])
        got.append(b.forward_spans([(0, 1, 1), (1, 14, rg + 1), (2, held + 1, rows)], seqs[0] + seqs[1][13:] + seqs[2][held:]))
        b.close()
    m.close()
    (lg, am), (plg, pam) = got
    assert np.array_equal(pam, first_max(plg)) and np.array_equal(pam, am)
    assert np.array_equal(bits(plg), bits(lg)), np.flatnonzero((bits(plg) != bits(lg)).any(axis=1)).tolist()


@pytest.mark.parametrize("kv", ["f32", "f16"])
def test_spans_on_a_non_monotonic_table_with_used_pages_give_the_bits_of_a_fresh_batch(kv):
    """tiny-gqa, 4 pages of 16: slots 0 and 1 fill pages 0 and 1 with another sequence's rows and release them while slot 2 takes 40
    positions in spans of 16, 16 and 8 -- table [2, 0, 1], and behind what it has written lie rows the page's last owner left"""
    fw, fw32 = model("tiny-gqa")
    rng = np.random.default_rng(5)
    seq, other = random_seq(rng, fw.shape.vocab_size, 40), random_seq(rng, fw.shape.vocab_size, 16)
    m = llmk.Llmk(fw)
    b, fresh = (llmk.Batch(m, 3, kv_type=kv, page_len=16, n_pages=4) for _ in range(2))
    b.forward_spans([(0, 1, 16), (1, 1, 16)], other * 2)                       # pages 0, 1
    got, want = [], []
    for p0, n, free in ((1, 16, None), (17, 16, 0), (33, 8, 1)):               # pages 2, 0, 1: rows 8 .. 15 of page 1 stay the other sequence's
        if free is not None:
            b.release(free)
        got.append(b.forward_spans([(2, p0, n)], seq[p0 - 1:p0 - 1 + n], want_argmax=False))
        want.append(fresh.forward_spans([(2, p0, n)], seq[p0 - 1:p0 - 1 + n], want_argmax=False))
    assert b.page_table(2) == [2, 0, 1] and fresh.page_table(2) == [0, 1, 2] and b.free_pages() == 1
    ref = RefPass(fw32).feed(seq) if kv == "f32" else kr.forward_fed(fw32, seq, *kr.peek_all(b, fw.shape.n_layers, 2, 40))
    b.close(), fresh.close(), m.close()
    assert np.array_equal(bits(np.concatenate(got)), bits(np.concatenate(want)))
    within_the_bar(f"{kv} table [2, 0, 1]", np.concatenate(got), ref)


@pytest.mark.parametrize("shape", ["tk-small-long"])
def test_a_long_span_pass_runs_several_parts_and_folds_them(shape):
    """page_len 16, 300 positions in slot 0, then 20 rows at 301 next to 3 rows at position 1 of slot 1: four groups, 20 tiles -- three
    parts on a 256-CU device, the short group's later parts empty, bd_attn_fold_kernel over the states"""
    fw, fw32 = model(shape)
    rng = np.random.default_rng(11)
    seqs = [random_seq(rng, fw.shape.vocab_size, 320), random_seq(rng, fw.shape.vocab_size, 3)]
    spans, toks = [(0, 301, 20), (1, 1, 3)], seqs[0][300:] + seqs[1]
    assert st.span_parts(spans, fw.shape.n_kv_heads, fw.shape.n_heads // fw.shape.n_kv_heads)[0] > 1
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 2, page_len=16, n_pages=21)
    b.ingest(0, seqs[0][:300])
    (lg, am), (lg2, am2) = b.forward_spans(spans, toks), b.forward_spans(spans, toks)
    assert b.free_pages() == 0
    b.close(), m.close()
    assert np.array_equal(bits(lg), bits(lg2)) and np.array_equal(am, am2) and np.array_equal(am, first_max(lg))
    within_the_bar("long span", lg[:20], RefPass(fw32).feed(seqs[0])[300:])
    within_the_bar("short span", lg[20:], RefPass(fw32).feed(seqs[1]))


@pytest.mark.parametrize("page_len", [16, 48])
def test_the_switch_keeps_the_per_row_form_and_a_chain_is_a_span(page_len):
    """LLMK_SPAN_ATTN=0 at llmk_pages_create: within the bar of the default form, with the bits of a dense batch created under the same
    switch (it held on the parent commit).  A chain llmk_tree_forward on the default paged batch IS the span pass."""
    fw, _ = model("tiny-hs64")
    rng = np.random.default_rng(3)
    seqs = [random_seq(rng, fw.shape.vocab_size, 30) for _ in range(2)]
    spans, toks = [(1, 4, 20), (0, 4, 9)], seqs[1][3:23] + seqs[0][3:12]
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 2, page_len=page_len, n_pages=4)
    os.environ["LLMK_SPAN_ATTN"] = "0"
    try:
        b0, d0 = llmk.Batch(m, 2, page_len=page_len, n_pages=4), llmk.Batch(m, 2)
    finally:
        del os.environ["LLMK_SPAN_ATTN"]
    out = []
    for x in (b, b0, d0):
        x.forward_spans([(0, 1, 3), (1, 1, 3)], seqs[0][:3] + seqs[1][:3])
        out.append(x.forward_spans(spans, toks))
    chain = b.forward_tree(spans, toks, list(range(-1, 19)) + list(range(-1, 8)))
    assert b0.time_spans(2, 9, 4, 2) > 0.0 and b.time_spans(2, 9, 4, 2) > 0.0
    b.close(), b0.close(), d0.close(), m.close()
    (lg, am), (lg0, am0), (lgd, amd) = out
    assert np.array_equal(am, first_max(lg)) and np.array_equal(am0, first_max(lg0))
    within_the_bar(f"page_len {page_len} LLMK_SPAN_ATTN=0 against the default", lg0, lg.astype(np.float64))
    assert np.array_equal(bits(lg0), bits(lgd)) and np.array_equal(am0, amd)
    assert np.array_equal(bits(chain[0]), bits(lg)) and np.array_equal(chain[1], am)
