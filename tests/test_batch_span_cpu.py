"""Spans for the batched decode (llmk_span_*) without a device: the header declares the new names and the
library exports them, null handles are refused before anything touches a GPU, and the mirrored group and split arithmetic
(tests/span_tiles.py) visits every visible (column, timestep) exactly once across parts and waves and no invisible one, never lets a
group cross a slot, and keeps every part state inside the buffers the first span call sizes."""
import collections
import os
import random
import re

import pytest

import batch_tiles as bt
import prefix_tiles as pt
import span_tiles as st
from conftest import ROOT
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf

NAMES = ["llmk_span_forward", "llmk_span_time"]
KV_MULS = (1, 2, 3, 4, 8, 16)
LOS = (0, 5, 16, 33)


@pytest.fixture(scope="module")
def lib():
    llmk.build_lib()
    return llmk.lib()


def test_header_declares_the_three_new_names_and_the_library_exports_them(lib):
    hdr = open(os.path.join(ROOT, "include", "llmk.h")).read()
    assert set(re.findall(r"^int (llmk_span_[a-z_]+)\(", hdr, re.M)) == set(NAMES)
    assert re.search(r"typedef struct llmk_span \{ int32_t slot, pos0, len; \} llmk_span;", hdr)
    assert re.search(r"#define LLMK_SPAN_LAST 1\b", hdr) and llmk.SPAN_LAST == 1
    f90 = open(os.path.join(ROOT, "llm.f90_amd", "host", "llmk_binding.f90")).read()
    for name in NAMES:
        assert name in llmk.SYMBOLS and hasattr(lib, name), name
        assert f'bind(C, name="{name}")' in f90, name
    assert lib.llmk_version() >= 408
    assert "LLMK_SPAN_ATTN=0" in hdr


def test_the_python_methods_exist():
    for attr in ("forward_spans", "ingest", "time_spans"):
        assert callable(getattr(llmk.Batch, attr)), attr
    assert [f[0] for f in llmk.Span._fields_] == ["slot", "pos0", "len"]


def test_null_handles_are_refused_without_a_device(lib):
    import ctypes as C
    sp = (llmk.Span * 1)(llmk.Span(0, 1, 2))
    tok = (C.c_int * 2)(1, 1)
    am = (C.c_int * 2)()
    ms = C.c_float()
    assert lib.llmk_span_forward(None, 1, sp, tok, 0, None, am) == 1
    assert lib.llmk_span_time(None, 1, 2, 1, 1, C.byref(ms)) == 1


def test_the_new_shape_has_three_query_heads_per_kv_head():
    s = gguf.SHAPES["tiny-kvmul3"]
    assert (s.emb_dim, s.head_size, s.n_heads, s.n_kv_heads) == (192, 32, 6, 2)
    assert pt.rg(3) == 5 and bt.BD_MAX_GROUP - 5 * 3 == 1            # five rows per group and one padded column
    assert s.emb_dim % 64 == 0 and s.hidden_dim % 64 == 0 and s.kv_dim % 16 == 0 and s.vocab_size % 4 == 0
    assert all(16 % (z.n_heads // z.n_kv_heads) == 0 for name, z in gguf.SHAPES.items() if name != "tiny-kvmul3")


def test_mirrors_follow_the_kernel_s_rule():
    src = open(os.path.join(ROOT, "llm.f90_amd", "csrc", "batch.h")).read()
    assert "return bd_parts(groups, n_kv_heads, own_tiles * BD_TILE, n_cu);" in src                    # bd_span_parts
    assert "[&](int r) { return lo <= r && r < vis; }" in src and "const int vis = row0.pos + c / kv_mul;" in src
    assert "t0 = lo / BD_TILE + part * tpp, t1 = min(t0 + tpp, ntile);" in src
    hip = open(os.path.join(ROOT, "llm.f90_amd", "csrc", "llmk.hip")).read()
    assert "b->sn->h_groups[ng++] = BdGroup{row + j, std::min(rg, spans[i].len - j)};" in hip
    assert hip.count("states = nb * c->nkv * 2 * BD_MAX_PARTS * c->kv_mul") == 2      # the span part states are sized as the prefix's


def random_spans(rng, kv_mul, lo, seq_len=400):
    """a pass of up to 128 rows: spans of 1 .. 2 rg + 1 rows (and one long one now and then) at positions behind lo"""
    rg = pt.rg(kv_mul)
    spans, rows, slot = [], 0, 0
    while rows < 128 and slot < 40:
        n = rng.choice([1, max(1, rg - 1), rg, rg + 1, 2 * rg + 1, rng.randint(1, 60)])
        n = min(n, 128 - rows)
        pos0 = rng.randint(lo + 1, seq_len - n)
        spans.append((slot, pos0, n))
        rows += n
        slot += 1
        if rng.random() < 0.15:
            break
    rng.shuffle(spans)
    return spans


@pytest.mark.parametrize("kv_mul", KV_MULS)
@pytest.mark.parametrize("lo", LOS)
def test_every_visible_timestep_of_every_column_is_visited_once_and_no_other(kv_mul, lo):
    rng = random.Random(1000 * kv_mul + lo)
    part_counts = set()
    for trial in range(12):
        nkv = rng.choice([1, 2, 4, 32])
        spans = random_spans(rng, kv_mul, lo)
        if trial == 0:
            spans = [(0, max(lo + 1, 300), 2 * pt.rg(kv_mul) + 1)]          # few groups at a long position: several parts
        if trial == 1:
            spans = [(3, lo + 1, pt.rg(kv_mul) + 1), (1, lo + 2, 1)]        # a few tiles behind lo: one part
        rows = st.rows_of(spans)
        lo_of = (lambda slot: lo)
        seen = collections.Counter(st.visits(spans, nkv, kv_mul, lo_of))
        want = {((i, q), r) for i, (slot, pos) in enumerate(rows) for q in range(kv_mul) for r in range(lo, pos)}
        assert set(seen) == want, (spans, nkv)
        assert set(seen.values()) == {1}, (spans, nkv)
        parts, tpp = st.span_parts(spans, nkv, kv_mul, lo_of)
        part_counts.add(parts)
        # every part state inside the buffers: states of (row, kv head) are prefix parts (at most BD_MAX_PARTS) then own parts
        np_ = bt.BD_MAX_PARTS + parts
        top = st.state_index(len(rows) - 1, nkv - 1, np_ - 1, kv_mul - 1, nkv, np_, kv_mul)
        assert parts <= bt.BD_MAX_PARTS and top < pt.state_capacity(nkv, kv_mul)
    assert max(part_counts) > 1 and 1 in part_counts, part_counts


@pytest.mark.parametrize("kv_mul", KV_MULS)
def test_the_group_table_never_crosses_a_slot_and_covers_every_row_once(kv_mul):
    rng = random.Random(77 + kv_mul)
    rg = pt.rg(kv_mul)
    for _ in range(50):
        spans = random_spans(rng, kv_mul, 0)
        rows = st.rows_of(spans)
        table = st.group_table(spans, kv_mul)
        covered = []
        for first, n in table:
            assert 1 <= n <= rg and first + n <= len(rows)
            grp = rows[first:first + n]
            assert len({slot for slot, _ in grp}) == 1, (spans, first, n)
            assert [pos for _, pos in grp] == list(range(grp[0][1], grp[0][1] + n))
            covered += range(first, first + n)
            cols, live = st.columns((first, n), kv_mul)
            assert live == n * kv_mul <= bt.BD_MAX_GROUP and len(cols) == 16
            assert cols[:live] == [(first + c // kv_mul, c % kv_mul) for c in range(live)]
            assert all(c == cols[live - 1] for c in cols[live:])
        assert covered == list(range(len(rows)))
        assert len(table) == sum(-(-n // rg) for _, _, n in spans)
