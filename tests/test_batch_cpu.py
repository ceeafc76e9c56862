"""Batched decode (llmk_batch_*) without a device: the header declares the symbols and the binding lists them,
null handles are refused before anything touches a GPU, and the mirrored tile / part arithmetic of the attention kernel
(tests/batch_tiles.py) visits every timestep of a row exactly once."""
import collections
import ctypes as C
import os
import re

import pytest

import batch_tiles as bt
from conftest import ROOT
from llm_f90_amd import llmk

NAMES = ["llmk_batch_create", "llmk_batch_destroy", "llmk_batch_fork", "llmk_batch_forward", "llmk_batch_decode", "llmk_batch_time"]


@pytest.fixture(scope="module")
def lib():
    llmk.build_lib()
    return llmk.lib()


def test_header_declares_the_batch_symbols_and_the_binding_lists_them(lib):
    hdr = open(os.path.join(ROOT, "include", "llmk.h")).read()
    declared = set(re.findall(r"^int (llmk_batch_[a-z_]+)\(", hdr, re.M))
    assert declared == set(NAMES)
    assert re.search(r"#define LLMK_MAX_BATCH 128\b", hdr) and llmk.MAX_BATCH == 128
    for name in NAMES:
        assert name in llmk.SYMBOLS and hasattr(lib, name), name
    # what the issue asks the header to say
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    assert "NO token-by-token fallback" in flat
    assert "Penalties, logit bias and log-prob records are out of scope" in flat


def test_null_handles_are_refused_without_a_device(lib):
    h = C.c_void_p()
    assert lib.llmk_batch_create(None, 4, 64, C.byref(h)) == 1 and not h.value
    one = (C.c_int * 1)(1)
    out = (C.c_int * 1)(0)
    assert lib.llmk_batch_forward(None, 1, one, one, one, None, out) == 1
    assert lib.llmk_batch_decode(None, 1, one, one, one, 1, None, out) == 1
    assert lib.llmk_batch_fork(None, 0, 0) == 1
    assert lib.llmk_batch_time(None, 1, 1, 1, None) == 1
    assert lib.llmk_batch_destroy(None) == 1


def test_mirrors_are_the_header_s_constants():
    src = open(os.path.join(ROOT, "llm.f90_amd", "csrc", "batch.h")).read()
    for name in ("BD_TILE", "BD_WAVES", "BD_MAX_PARTS", "BD_MAX_GROUP"):
        m = re.search(rf"constexpr int {name} = (\d+);", src)
        assert m and int(m.group(1)) == getattr(bt, name), name


def test_tiles_and_parts_cover_every_timestep_exactly_once():
    """every pos in 1..704 at every part count, alone (tiles per part from its own length) and next to a longer row (from 704)"""
    for pos in range(1, 705):
        for parts in range(1, bt.BD_MAX_PARTS + 1):
            for max_pos in (None, 704):
                c = collections.Counter(bt.covered_timesteps(pos, parts, max_pos))
                assert sorted(c) == list(range(pos)) and set(c.values()) == {1}, (pos, parts, max_pos)


def test_split_rule_keeps_the_part_states_inside_their_workspace():
    """parts > 1 only while rows x kv heads x parts <= CUs (the part workspace is sized by the CU count), and every part of the
    longest row has a tile for each of its waves but possibly the last"""
    for n in (1, 2, 3, 5, 8, 32, 128):
        for nkv in (1, 2, 4, 8, 32):
            for pos in (1, 16, 17, 128, 129, 704, 2048, 4096):
                p = bt.bd_parts(n, nkv, pos)
                assert 1 <= p <= bt.BD_MAX_PARTS
                assert p == 1 or n * nkv * p <= bt.N_CU
                tpp = bt.bd_tiles_per_part(pos, p)
                assert p == 1 or (p - 1) * tpp < (pos + bt.BD_TILE - 1) // bt.BD_TILE      # no part of the longest row but the last can be empty... and not that one
    assert bt.bd_parts(1, 2, 704) == 6 and bt.bd_tiles_per_part(704, 6) == 8
    assert bt.part_boundaries(704, 1, 2) == [128, 256, 384, 512, 640]


def test_boundary_positions_hold_every_part_boundary():
    ks = set(bt.boundary_positions(704))
    for pos in range(2, 705):
        for n in (1, 5):
            for b in bt.part_boundaries(pos, n, 2):
                assert {b - 1, b, b + 1} & set(range(2, 705)) <= ks
