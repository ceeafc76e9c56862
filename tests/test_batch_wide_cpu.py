"""The case tables of tests/test_batch_wide_gpu.py without a device: do the passes they describe reach what they
are there for -- a wave that takes several tiles in bd_attn_kernel, bd_attn_prefix_kernel and bd_attn_own_kernel, at one part and at
several -- and does every pass visit every timestep of every row once?  The numbers come from the mirrors tests/batch_tiles.py and
tests/prefix_tiles.py at 256 CUs: when BD_WAVES or the split rule moves, these fail before the GPU tests silently stop covering it."""
import collections

import numpy as np
import pytest

import attn_needle as an
import batch_tiles as bt
import prefix_tiles as pt


def once(seen, lo, hi):
    c = collections.Counter(seen)
    return sorted(c) == list(range(lo, hi)) and set(c.values()) <= {1}


# ---- the tile counts a wide pass reaches ----------------------------------------------------------------------------------------------
PLANS = {"tk-small-long": {32: (4, 11, 2), 33: (3, 15, 2), 64: (2, 22, 3), 65: (1, 44, 6), 128: (1, 44, 6)},       # rows: (parts, tiles
         "tiny-hs128w-long": {32: (2, 10, 2), 33: (1, 20, 3), 128: (1, 20, 3)}}                                    # per part, per wave)


@pytest.mark.parametrize("shape", list(bt.WIDE_SHAPES))
def test_wide_passes_give_a_wave_several_tiles_and_the_existing_cases_never_do(shape):
    nkv, n_pos, counts = bt.WIDE_SHAPES[shape]
    assert set(counts) == set(PLANS[shape])
    for n, (parts, tpp, per_wave) in PLANS[shape].items():
        assert bt.bd_parts(n, nkv, n_pos) == parts, n
        assert bt.bd_tiles_per_part(n_pos, parts) == tpp, n
        assert bt.max_tiles_per_wave(n, nkv, n_pos) == per_wave, n
    got = {n: (bt.bd_parts(n, nkv, n_pos), bt.max_tiles_per_wave(n, nkv, n_pos)) for n in counts}
    assert any(p == 1 and w >= 3 for p, w in got.values()), got          # the direct-normalise path behind more than 8 tiles
    assert any(p >= 2 and w >= 2 for p, w in got.values()), got          # part states left by waves that rescaled
    # tests/test_batch_gpu.py test 3 and tests/test_batch_prefix_gpu.py: a row alone, or among 5: never a second tile
    for k in range(1, n_pos + 1):
        assert bt.max_tiles_per_wave(1, nkv, k) == 1 and bt.max_tiles_per_wave(5, nkv, k) == 1, k


@pytest.mark.parametrize("shape", list(bt.WIDE_SHAPES))
def test_transcript_passes_hold_the_rows_their_docstring_names_and_visit_every_timestep_once(shape):
    nkv, n_pos, counts = bt.WIDE_SHAPES[shape]
    passes = bt.wide_transcript_passes(shape)
    assert passes == bt.wide_transcript_passes(shape)                       # seeded: the same table in every process
    assert set(passes) == set(counts)
    met = set()
    for n, ks in passes.items():
        assert len(ks) == n and len(set(ks)) == n and min(ks) >= 1 and max(ks) == n_pos, n      # the longest row: the table's plan
        parts = bt.bd_parts(n, nkv, n_pos)
        for k in ks:
            assert once(bt.covered_timesteps(k, parts, n_pos), 0, k), (n, k)
        if parts >= 2:                                                       # a short row: empty parts, empty waves
            assert bt.SHORT_ROW in ks
            per = bt.tiles_per_wave(n, nkv, n_pos, bt.SHORT_ROW)
            assert all(not ts for part in per[1:] for ts in part) and not per[0][bt.BD_WAVES - 1] and per[0][0]
        met |= set(ks)
    ntile = n_pos // bt.BD_TILE
    assert {(k + bt.BD_TILE - 1) // bt.BD_TILE for k in passes[max(counts)]} == set(range(1, ntile + 1))
    assert set(bt.boundary_positions(n_pos)) <= met
    assert {128, 129, 256, 257} <= met                                       # where a wave's second and third tiles begin
    assert any(bt.bd_parts(n, nkv, n_pos) == 2 for n in counts)


# ---- needles ------------------------------------------------------------------------------------------------------------------------
def test_the_wide_needle_layout_sits_on_second_tiles_and_part_boundaries():
    nkv, S = 2, bt.WIDE_NEEDLE_S
    lay = bt.WIDE_NEEDLES
    assert not set(lay[0]) & set(lay[1])
    assert bt.wide_needle_passes() == bt.wide_needle_passes()
    # 128 rows: one part; row 127 is the last of wave 7's first tile, 128 the first of wave 0's second, 256 of its third
    per = bt.tiles_per_wave(128, nkv, S, S)
    assert len(per) == 1 and per[0][7][0] == 127 // 16 and per[0][0][1] == 128 // 16 and per[0][0][2] == 256 // 16
    # 64 rows: two parts of 22 tiles; 351 | 352 is the part boundary, 480 the first row of part 1's wave 0's second tile
    per = bt.tiles_per_wave(64, nkv, S, S)
    assert len(per) == 2 and per[1][0][0] * 16 == 352 and per[1][0][1] * 16 == 480
    assert {127, 255, 351, 479} <= set(lay[0]) and {128, 256, 352, 480} <= set(lay[1])
    # the last tile of the context: the target of every clamped look-ahead load
    last = (S - 1) // 16 * 16
    assert last - 1 in lay[0] and last in lay[1] and S - 1 in lay[0]
    for n, ks in bt.wide_needle_passes().items():
        assert len(ks) == n and len(set(ks)) == n and max(ks) == S
        for ts in lay.values():
            for t in ts:
                assert t + 1 in ks and (t + 2 in ks or t + 2 > S), (n, t)
        for k in ks:
            assert once(bt.covered_timesteps(k, bt.bd_parts(n, nkv, S), S), 0, k), (n, k)


def test_the_wide_needle_case_holds_on_the_float64_reference_alone():
    """what test 3 of tests/test_batch_wide_gpu.py relies on: the needles hold the mass -- for the last query as the sibling tests
    assert it, and for every row of the two passes over the needles that row sees -- and more than half of the rows are safe for argmax"""
    s, layout, tokens, fw = bt.wide_needle_case()
    S, kv_mul = s.seq_len, s.n_heads // s.n_kv_heads
    ref, att0 = an.forward_all(fw, tokens)
    for g, ts in layout.items():
        assert att0[g * kv_mul, S - 1, ts].sum() > 0.999
    for n, ks in bt.wide_needle_passes().items():
        for k in ks:
            for g, ts in layout.items():
                vis = [t for t in ts if t < k]
                assert not vis or att0[g * kv_mul, k - 1, vis].sum() > 0.999, (n, k, g)
        safe = an.safe_argmax_positions(ref[np.array(ks) - 1])
        assert safe.sum() > len(safe) // 2, (n, int(safe.sum()))


# ---- the shared prefix ----------------------------------------------------------------------------------------------------------------
def test_the_prefix_kernel_takes_two_tiles_per_wave_only_at_this_shape():
    nkv, kv_mul = 2, 4                                                       # tiny-gqa
    for P, tpp in ((560, 9), (690, 11)):
        for natt in (127, 128):
            assert pt.prefix_parts(natt, nkv, kv_mul, P) == 4
            assert bt.bd_tiles_per_part(P, 4) == tpp
            assert pt.most(pt.prefix_tiles_per_wave(natt, nkv, kv_mul, P)) == 2
    for P in range(1, 691):
        for natt in range(1, 65):                                                            # 64 attached rows or fewer
            assert pt.most(pt.prefix_tiles_per_wave(natt, nkv, kv_mul, P)) == 1, (natt, P)
        for natt in (1, 64, 128):
            assert pt.most(pt.prefix_tiles_per_wave(natt, 2, 2, P)) == 1, (natt, P)          # tk-small
            assert pt.most(pt.prefix_tiles_per_wave(natt, 4, 1, P)) == 1, (natt, P)          # tiny-hs128w


def test_the_own_kernel_s_tiles_per_wave():
    rows = [(19, 19 + 16 * 8 + 1)] * 128                                     # 128 rows x 2 kv heads: one own part
    assert pt.own_parts(rows, 2)[0] == 1
    assert pt.own_span_tiles(rows) == 9 and pt.most(pt.own_tiles_per_wave(rows, *rows[0], 2)) == 2
    rows = [(0, 16 * 17)] * 128
    assert pt.own_span_tiles(rows) == 17 and pt.most(pt.own_tiles_per_wave(rows, *rows[0], 2)) == 3


@pytest.mark.parametrize("case", list(pt.WIDE_PREFIX_CASES))
def test_prefix_passes_reach_several_tiles_per_wave_and_visit_every_timestep_once(case):
    nkv, kv_mul = 2, 4
    P, run, join = pt.WIDE_PREFIX_CASES[case]
    assert P + run <= pt.WIDE_SEQ_LEN
    passes = pt.wide_prefix_passes(case)
    widths, prefix_most, own_most, own_most_free, fed = set(), 0, 0, 0, collections.Counter()
    for rows in passes:
        assert 1 <= len(rows) <= pt.MAX_BATCH and len({r[0] for r in rows}) == len(rows)
        widths.add(len(rows))
        att = [r for r in rows if r[1] > 0]
        for slot, first, pos in rows:
            assert first < pos <= pt.WIDE_SEQ_LEN
            fed[slot, pos] += 1
        if not att:                                                          # no attached row: bd_attn_kernel, as in a batch without a prefix
            for slot, first, pos in rows:
                assert once(bt.covered_timesteps(pos, bt.bd_parts(len(rows), nkv, pos), pos), 0, pos)
            continue
        pparts = pt.prefix_parts(len(att), nkv, kv_mul, P)
        assert once(pt.prefix_covered(P, pparts), 0, P)
        prefix_most = max(prefix_most, pt.most(pt.prefix_tiles_per_wave(len(att), nkv, kv_mul, P)))
        span = [(first, pos) for _, first, pos in rows]
        parts, tpp = pt.own_parts(span, nkv)
        for first, pos in set(span):
            assert once(pt.own_covered(first, pos, parts, tpp), first, pos), (first, pos)
            m = pt.most(pt.own_tiles_per_wave(span, first, pos, nkv))
            own_most = max(own_most, m)
            if first == 0:
                own_most_free = max(own_most_free, m)
        groups = pt.groups(len(att), kv_mul)
        cmap = pt.column_map([i for i, r in enumerate(rows) if r[1] > 0], kv_mul)
        assert sum(len(pt.live_columns(cmap, g, kv_mul)) for g in range(groups)) == len(att) * kv_mul
    slots = {slot for slot, _ in fed}
    assert set(fed.values()) == {1} and all((slot, pos) in fed for slot in slots for pos in range(P + 1, P + run + 1))
    if join is not None:
        assert len(slots) == 128 and {127, 128} <= widths
        assert prefix_most == 2                                              # bd_attn_prefix_kernel: a wave's second tile
        assert own_most_free >= 5                                            # bd_attn_own_kernel with first = 0 behind >= 35 tiles
        assert pt.WIDE_ATTACHED % pt.rg(kv_mul) != 0                         # the last column group is not full
    else:
        assert len(slots) == 128 and 128 in widths and P % bt.BD_TILE != 0
        assert own_most == 2 and prefix_most == 1                            # own rows 19 .. 168: 10 tiles, the first masked below P


# ---- widths ---------------------------------------------------------------------------------------------------------------------------
def test_the_width_schedule_shrinks_between_wide_passes_and_builds_every_row_in_order():
    need = {128, 113, 112, 97, 96, 65, 64, 33, 32, 17, 16, 3, 2, 1}
    assert need <= set(bt.WIDTHS)
    sch = bt.WIDTH_SCHEDULE
    for w in need - {128}:                                                   # behind a wider pass: stale workspace rows, stale part states
        assert any(sch[i] == w and max(sch[:i]) > w for i in range(1, len(sch))), w
        if w <= 33:                                                          # ... the narrow ones directly behind one of 64 rows or more
            assert any(sch[i] == w and sch[i - 1] >= 64 for i in range(1, len(sch))), w
    assert (sch[0], sch[1], sch[2]) == (128, 17, 113)
    passes = bt.width_passes()
    assert passes == bt.width_passes() and [len(r) for r in passes] == list(sch)
    fed = [0] * 128
    for rows in passes:
        assert len({j for j, _ in rows}) == len(rows)
        for j, pos in rows:
            assert pos == fed[j] + 1                                         # every K/V row a later pass reads was written by a pass
            fed[j] = pos
        assert [j for j, _ in rows] != sorted(j for j, _ in rows) or len(rows) == 1      # row index != slot order
    assert min(fed) >= 19 and max(fed) <= 20 and sum(fed) == sum(sch)       # what the oracle is asked for, per case
    assert any(len({p for _, p in rows}) > 1 for rows in passes)             # ragged positions inside a pass
