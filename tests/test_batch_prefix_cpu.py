"""A shared prefix for the batched decode (llmk_prefix_*) without a device: the header declares the three symbols
and the bindings list them, null handles are refused before anything touches a GPU, and the mirrored split / column arithmetic
(tests/prefix_tiles.py) visits every prefix row once per part sweep, puts every (attached row, query head) in one live column, keeps
every part state inside the buffers llmk_prefix_set sizes, and covers an own range P .. pos-1 once and nothing below P."""
import collections
import functools
import os
import re

import pytest

import batch_tiles as bt
import prefix_tiles as pt
from conftest import ROOT
from llm_f90_amd import llmk

NAMES = ["llmk_prefix_set", "llmk_prefix_attach", "llmk_prefix_len"]
KV_MULS = (1, 2, 4, 8, 16)
KV_HEADS = (1, 4, 8, 32)


@pytest.fixture(scope="module")
def lib():
    llmk.build_lib()
    return llmk.lib()


def test_header_declares_the_three_prefix_symbols_and_the_bindings_list_them(lib):
    hdr = open(os.path.join(ROOT, "include", "llmk.h")).read()
    assert set(re.findall(r"^int (llmk_prefix_[a-z_]+)\(", hdr, re.M)) == set(NAMES)
    f90 = open(os.path.join(ROOT, "llm.f90_amd", "host", "llmk_binding.f90")).read()
    for name in NAMES:
        assert name in llmk.SYMBOLS and hasattr(lib, name), name
        assert f'bind(C, name="{name}")' in f90, name
    assert lib.llmk_version() >= 406
    for attr in ("set_prefix", "attach", "prefix_len"):
        assert hasattr(llmk.Batch, attr), attr


def test_null_handles_are_refused_without_a_device(lib):
    assert lib.llmk_prefix_set(None, 4) == 1
    assert lib.llmk_prefix_set(None, 0) == 1
    assert lib.llmk_prefix_attach(None, 0) == 1
    assert lib.llmk_prefix_len(None) == -1


def test_mirrors_follow_the_header_s_rule():
    src = open(os.path.join(ROOT, "llm.f90_amd", "csrc", "batch.h")).read()
    assert "BD_MAX_GROUP / kv_mul < 1 ? 1 : BD_MAX_GROUP / kv_mul" in src                       # bd_prefix_rg
    assert "return bd_parts(bd_prefix_groups(n_att, kv_mul), n_kv_heads, P, n_cu);" in src      # bd_prefix_parts
    hip = open(os.path.join(ROOT, "llm.f90_amd", "csrc", "llmk.hip")).read()
    assert "states = nb * c->nkv * 2 * BD_MAX_PARTS * c->kv_mul" in hip and re.search(r"#define LLMK_MAX_BATCH 128\b", open(
        os.path.join(ROOT, "include", "llmk.h")).read())
    # the issue's rule, written out, against the mirror
    for n_att, nkv, kv_mul, P in ((1, 4, 1, 1000), (128, 32, 1, 1000), (17, 8, 8, 200), (3, 1, 8, 33), (128, 1, 16, 4096)):
        cg = -(-n_att // max(1, 16 // kv_mul))
        want = max(1, min(bt.N_CU // (nkv * cg), -(-(-(-P // 16)) // 8), bt.BD_MAX_PARTS))
        assert pt.prefix_parts(n_att, nkv, kv_mul, P) == want, (n_att, nkv, kv_mul, P)
    assert pt.prefix_parts(128, 32, 1, 1000) == 1 and pt.groups(128, 1) == 8       # Llama-2-7B, 128 rows: 8 reads of the prompt per kv head
    assert pt.prefix_parts(1, 4, 1, 1000) == 8


@functools.lru_cache(maxsize=None)
def sweep_ok(P, parts):
    c = collections.Counter(pt.prefix_covered(P, parts))
    return sorted(c) == list(range(P)) and set(c.values()) == {1}


@functools.lru_cache(maxsize=None)
def columns_ok(n_att, kv_mul):
    """every (attached row, query head) in exactly one live column; at most 16 columns per group; the map's cells inside its buffer"""
    rows = list(range(100, 100 + n_att))            # (row indices of the pass: any distinct numbers)
    cmap = pt.column_map(rows, kv_mul)
    if len(cmap) > pt.MAX_BATCH + bt.BD_MAX_GROUP:
        return False
    seen = collections.Counter()
    for g in range(pt.groups(n_att, kv_mul)):
        live = pt.live_columns(cmap, g, kv_mul)
        if not 1 <= len(live) <= 16:
            return False
        seen.update(live)
    return set(seen) == {(r, q) for r in rows for q in range(kv_mul)} and set(seen.values()) == {1}


def test_prefix_sweeps_columns_and_states_over_every_combination():
    """P in 1..200 x attached rows in 1..128 x kv_mul x kv heads at 256 CUs"""
    met = set()
    for kv_mul in KV_MULS:
        for n_att in range(1, 129):
            assert columns_ok(n_att, kv_mul), (n_att, kv_mul)
            cg = pt.groups(n_att, kv_mul)
            for nkv in KV_HEADS:
                cap = pt.state_capacity(nkv, kv_mul)
                for P in range(1, 201):
                    parts = pt.prefix_parts(n_att, nkv, kv_mul, P)
                    met.add(parts)
                    assert 1 <= parts <= bt.BD_MAX_PARTS
                    assert parts == 1 or nkv * cg * parts <= bt.N_CU, (n_att, nkv, kv_mul, P)       # workgroups: one wave of the device
                    assert sweep_ok(P, parts), (P, parts)
                    # the last state any workgroup of the pass writes: last row, last kv head, last own part behind the prefix parts
                    np_ = parts + bt.BD_MAX_PARTS
                    assert pt.state_index(pt.MAX_BATCH - 1, nkv - 1, np_ - 1, kv_mul - 1, nkv, np_, kv_mul) < cap
    assert met == {1, 2}, met            # 200 positions are 13 tiles: two parts of 8 waves at the most


def test_longer_prefixes_split_further_and_still_sweep_once():
    for P in (201, 255, 256, 257, 1000, 1024, 2047):
        for parts in range(1, bt.BD_MAX_PARTS + 1):
            assert sweep_ok(P, parts), (P, parts)
    assert pt.prefix_parts(1, 2, 2, 704) == 6 and pt.prefix_part_boundaries(704, 1, 2, 2) == [128, 256, 384, 512, 640]


@pytest.mark.parametrize("shape", list(pt.NEEDLE_CASES))
def test_the_needle_cases_hold_on_the_float64_reference_alone(shape):
    """what tests/test_batch_prefix_gpu.py test 3 relies on, before any GPU run: the needles sit on both sides of the two ragged edges
    and of the prefix's first part boundary, they hold the mass, and more than half of the positions behind P are safe for argmax"""
    import attn_needle as an
    s, P, layout, tokens, fw = pt.needle_case(shape)
    S = s.seq_len
    b0 = pt.prefix_part_boundaries(P, 1, s.n_kv_heads, s.n_heads // s.n_kv_heads)[0]
    assert {P - 1, bt.BD_TILE - 1, b0 - 1} <= set(layout[0]) and {P, bt.BD_TILE, b0} <= set(layout[1]) and P % bt.BD_TILE
    ref, att0 = an.forward_all(fw, tokens)
    for g, ts in layout.items():
        assert att0[g * (s.n_heads // s.n_kv_heads), S - 1, ts].sum() > 0.999
    safe = an.safe_argmax_positions(ref[P:])
    assert safe.sum() > len(safe) // 2, (int(safe.sum()), len(safe))


def test_own_ranges_cover_p_to_pos_once_and_nothing_below_p():
    """an attached row alone and next to an unattached long row (the tiles per part then come from THAT row's range), every own part
    count the rule can give; P on, below and above tile boundaries"""
    for P in range(0, 201):
        for pos in sorted({P + 1, P + 2, P + 15, P + 16, P + 17, P + 34, P + 129, P + 300}):
            for other in (None, (0, 704), (P, P + 500)):
                rows = [(P, pos)] + ([other] if other else [])
                for nkv in (1, 4):
                    parts, tpp = pt.own_parts(rows, nkv)
                    for first, p in rows:
                        c = collections.Counter(pt.own_covered(first, p, parts, tpp))
                        assert sorted(c) == list(range(first, p)) and set(c.values()) == {1}, (P, pos, other, nkv, parts, tpp)
                    assert 1 <= parts <= bt.BD_MAX_PARTS and (parts == 1 or len(rows) * nkv * parts <= bt.N_CU)
