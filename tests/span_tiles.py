"""TEST INFRASTRUCTURE -- mirrors of the span passes' group and split arithmetic (llm.f90_amd/csrc/batch.h, the llmk_span_* section;
span_upload and bd_pass_of in csrc/llmk.hip), as tests/batch_tiles.py and tests/prefix_tiles.py mirror the other attention kernels.
Used by tests/test_batch_span_cpu.py (is every visible (column, timestep) visited once and no other, does a group stay inside a
slot?) and tests/test_batch_span_gpu.py (how many parts did a pass run, where do groups, tiles and parts begin?)."""
from __future__ import annotations

import batch_tiles as bt
import prefix_tiles as pt


def rows_of(spans):
    """the rows of a pass, in span order: [(slot, pos)]; spans = [(slot, pos0, len)]"""
    return [(slot, pos0 + j) for slot, pos0, n in spans for j in range(n)]


def group_table(spans, kv_mul: int):
    """span_upload: [(first row index, rows)] -- every span cut into groups of rg consecutive rows, the last one possibly shorter"""
    rg, out, row = pt.rg(kv_mul), [], 0
    for _, _, n in spans:
        out += [(row + j, min(rg, n - j)) for j in range(0, n, rg)]
        row += n
    return out


def columns(group, kv_mul: int):
    """bd_attn_span_kernel: the (row index, query head of the kv group) pair of each of the 16 MFMA columns, and how many are live
    (columns from the last live one on repeat it and are not written)"""
    first, n = group
    live = n * kv_mul
    cols = [(first + min(c, live - 1) // kv_mul, min(c, live - 1) % kv_mul) for c in range(bt.BD_MAX_GROUP)]
    return cols, live


def own_tiles(spans, kv_mul: int, lo_of=lambda slot: 0) -> int:
    """bd_pass_of: the longest group's tile count, from the tile that holds row lo to the one of the group's last row"""
    rows = rows_of(spans)
    most = 0
    for first, n in group_table(spans, kv_mul):
        slot, pos = rows[first + n - 1]
        most = max(most, (pos + bt.BD_TILE - 1) // bt.BD_TILE - lo_of(slot) // bt.BD_TILE)
    return most


def span_parts(spans, n_kv_heads: int, kv_mul: int, lo_of=lambda slot: 0, n_cu: int = bt.N_CU):
    """(parts, tiles per part) of a span pass: bd_parts with the groups in the place of the rows, on the longest group's tiles"""
    own = own_tiles(spans, kv_mul, lo_of) * bt.BD_TILE
    parts = bt.bd_parts(len(group_table(spans, kv_mul)), n_kv_heads, own, n_cu)
    return parts, bt.bd_tiles_per_part(own, parts)


def visits(spans, n_kv_heads: int, kv_mul: int, lo_of=lambda slot: 0, n_cu: int = bt.N_CU):
    """every ((row index, query head), cache row) the kernel's live columns accumulate over all groups, parts and waves of a pass,
    with multiplicity: the tile sweep of a (group, part, wave) and the lane's predicate lo <= r < pos(column's row)"""
    rows = rows_of(spans)
    parts, tpp = span_parts(spans, n_kv_heads, kv_mul, lo_of, n_cu)
    seen = []
    for group in group_table(spans, kv_mul):
        first, n = group
        slot, last_pos = rows[first + n - 1]
        lo = lo_of(slot)
        ntile = (last_pos + bt.BD_TILE - 1) // bt.BD_TILE
        cols, live = columns(group, kv_mul)
        for p in range(parts):
            t0 = lo // bt.BD_TILE + p * tpp
            t1 = min(t0 + tpp, ntile)
            for w in range(bt.BD_WAVES):
                for kt in bt.wave_tiles(t0, t1, w):
                    for c in range(live):
                        vis = rows[cols[c][0]][1]
                        seen += [(cols[c], r) for r in range(kt * bt.BD_TILE, (kt + 1) * bt.BD_TILE) if lo <= r < vis]
    return seen


def state_index(row: int, kvh: int, state: int, q: int, n_kv_heads: int, np_: int, kv_mul: int) -> int:
    """where state `state` (prefix parts first, then own parts) of (row, kv head), query head q lives in the span part states"""
    return pt.state_index(row, kvh, state, q, n_kv_heads, np_, kv_mul)
