"""TEST INFRASTRUCTURE -- mirrors of the shared prefix's split and column arithmetic (llm.f90_amd/csrc/batch.h, the llmk_prefix_*
section; bd_pass in csrc/llmk.hip for the own parts), as tests/batch_tiles.py mirrors bd_attn_kernel's.  Used by
tests/test_batch_prefix_cpu.py (is every timestep visited once, every query head in one live column, every state inside its buffer?)
and tests/test_batch_prefix_gpu.py (which prefix lengths split, where do the parts begin?); the last section holds the case table of
tests/test_batch_wide_gpu.py test 4, which tests/test_batch_wide_cpu.py checks on these mirrors."""
from __future__ import annotations

import batch_tiles as bt

MAX_BATCH = 128       # include/llmk.h LLMK_MAX_BATCH: the rows the part-state buffers are sized for


def rg(kv_mul: int) -> int:
    """bd_prefix_rg: rows per column group"""
    return max(1, bt.BD_MAX_GROUP // kv_mul)


def groups(n_att: int, kv_mul: int) -> int:
    """bd_prefix_groups: column groups of n_att attached rows"""
    return (n_att + rg(kv_mul) - 1) // rg(kv_mul)


def prefix_parts(n_att: int, n_kv_heads: int, kv_mul: int, P: int, n_cu: int = bt.N_CU) -> int:
    """bd_prefix_parts: max(1, min(n_cu / (kv heads x column groups), ceil(ceil(P / 16) / 8), BD_MAX_PARTS))"""
    return bt.bd_parts(groups(n_att, kv_mul), n_kv_heads, P, n_cu)


def prefix_covered(P: int, parts: int):
    """every prefix cache row one column group's part sweep visits, with multiplicity (predicate: row < P)"""
    return bt.covered_timesteps(P, parts)


def prefix_part_boundaries(P: int, n_att: int, n_kv_heads: int, kv_mul: int):
    """the first cache row of prefix parts 1.. for n_att attached rows behind P positions"""
    parts = prefix_parts(n_att, n_kv_heads, kv_mul, P)
    tpp = bt.bd_tiles_per_part(P, parts)
    return [p * tpp * bt.BD_TILE for p in range(1, parts) if p * tpp * bt.BD_TILE < P]


def column_map(att_rows, kv_mul: int):
    """bd_upload_rows: [groups][RG] row indices of the pass's attached rows in row order, -1 behind the last"""
    cells = groups(len(att_rows), kv_mul) * rg(kv_mul)
    return list(att_rows) + [-1] * (cells - len(att_rows))


def live_columns(cmap, group: int, kv_mul: int):
    """bd_attn_prefix_kernel: the (row, query head of the kv group) pair of every LIVE column of a group, in column order"""
    cm = cmap[group * rg(kv_mul):(group + 1) * rg(kv_mul)]
    nr = 0
    while nr < len(cm) and cm[nr] >= 0:
        nr += 1
    return [(cm[c // kv_mul], c % kv_mul) for c in range(nr * kv_mul)]


def own_span_tiles(rows):
    """bd_pass: the longest own range of a pass in whole tiles, counted from the tile that holds row `first`; rows = [(first, pos)]"""
    return max((pos + bt.BD_TILE - 1) // bt.BD_TILE - first // bt.BD_TILE for first, pos in rows)


def own_parts(rows, n_kv_heads: int, n_cu: int = bt.N_CU):
    """(own parts, tiles per part) of a pass: bd_parts / bd_tiles_per_part on the longest own range"""
    span = own_span_tiles(rows) * bt.BD_TILE
    parts = bt.bd_parts(len(rows), n_kv_heads, span, n_cu)
    return parts, bt.bd_tiles_per_part(span, parts)


def own_covered(first: int, pos: int, parts: int, tpp: int):
    """every own cache row bd_attn_own_kernel visits for a row at `pos` whose first own row is `first`, with multiplicity"""
    ntile = (pos + bt.BD_TILE - 1) // bt.BD_TILE
    seen = []
    for p in range(parts):
        t0 = first // bt.BD_TILE + p * tpp
        t1 = min(t0 + tpp, ntile)
        for w in range(bt.BD_WAVES):
            for kt in bt.wave_tiles(t0, t1, w):
                seen += [r for r in range(kt * bt.BD_TILE, (kt + 1) * bt.BD_TILE) if first <= r < pos]      # the predicate
    return seen


def needle_layout(s, S: int, P: int):
    """tests/attn_needle.py layout for a sequence whose first P positions are the prefix and which then runs alone through an attached
    slot: needles of kv heads 0 | 1 on both sides of the two ragged edges (cache rows P-1 | P: the prefix's last row, the first own
    row), of the prefix's first tile boundary (15 | 16) and of its first part boundary (the last row of part 0 | the first of part 1);
    the sink and the last row as tests/test_batch_gpu.py has them"""
    assert P % bt.BD_TILE != 0
    bounds = prefix_part_boundaries(P, 1, s.n_kv_heads, s.n_heads // s.n_kv_heads)
    assert len(bounds) >= 1, (P, bounds)
    lay = {0: {0, bt.BD_TILE - 1, bounds[0] - 1, P - 1, S - 1}, 1: {bt.BD_TILE, bounds[0], P}}
    assert not lay[0] & lay[1], lay
    return {g: sorted(ts) for g, ts in lay.items()}


NEEDLE_CASES = {"tk-small-long": (704, 469), "tiny-hs128w-long": (320, 213)}      # shape: (S, P); P % 16 = 5, the prefix in 4 | 2 parts
NEEDLE_SEED = 20261019


def needle_case(shape: str):
    """(shape with seq_len S, P, layout, tokens, needle-shaped f32 weights) of a needle case"""
    import attn_needle as an
    from llm_f90_amd.tools import gguf
    S, P = NEEDLE_CASES[shape]
    s0 = gguf.SHAPES[shape]
    s = gguf.LlamaShape(s0.emb_dim, s0.hidden_dim, s0.n_layers, s0.n_heads, s0.n_kv_heads, s0.vocab_size, S)
    layout = needle_layout(s, S, P)
    tokens, needle_tokens = an.needle_sequence(s, layout, NEEDLE_SEED)
    fw = an.shape_needles(gguf.synth_fused(s, 4242), needle_tokens, an.BETA)
    return s, P, layout, tokens, fw


def state_index(row: int, kvh: int, state: int, q: int, n_kv_heads: int, np_: int, kv_mul: int) -> int:
    """where state `state` (prefix parts first, then own parts) of (row, kv head), query head q lives in d_xpml"""
    return ((row * n_kv_heads + kvh) * np_ + state) * kv_mul + q


def state_capacity(n_kv_heads: int, kv_mul: int) -> int:
    """llmk_prefix_set: {M, L} entries of the part-state buffers"""
    return MAX_BATCH * n_kv_heads * 2 * bt.BD_MAX_PARTS * kv_mul


# ---- wide passes (tests/test_batch_wide_cpu.py, tests/test_batch_wide_gpu.py test 4) --------------------------------------------------
def prefix_tiles_per_wave(n_att: int, n_kv_heads: int, kv_mul: int, P: int, n_cu: int = bt.N_CU):
    """[part][wave] -> the prefix tiles that wave of bd_attn_prefix_kernel multiplies in a pass with n_att attached rows"""
    parts = prefix_parts(n_att, n_kv_heads, kv_mul, P, n_cu)
    tpp = bt.bd_tiles_per_part(P, parts)
    return [[bt.wave_tiles(*bt.part_tiles(P, p, tpp), w) for w in range(bt.BD_WAVES)] for p in range(parts)]


def own_tiles_per_wave(rows, first: int, pos: int, n_kv_heads: int, n_cu: int = bt.N_CU):
    """[part][wave] -> the tiles that wave of bd_attn_own_kernel multiplies for the row (first, pos) inside the pass `rows`"""
    parts, tpp = own_parts(rows, n_kv_heads, n_cu)
    ntile = (pos + bt.BD_TILE - 1) // bt.BD_TILE
    out = []
    for p in range(parts):
        t0 = first // bt.BD_TILE + p * tpp
        out.append([bt.wave_tiles(t0, min(t0 + tpp, ntile), w) for w in range(bt.BD_WAVES)])
    return out


def most(per_wave) -> int:
    return max(len(ts) for part in per_wave for ts in part)


# tiny-gqa's geometry (kv_mul 4: 4 rows per column group, 2 kv heads) with room for a long prefix
WIDE_SEQ_LEN = 704
WIDE_ATTACHED = 127       # slots 0 .. 126; slot 127 is forked, not attached
WIDE_STAGGER = 8          # attached slot j joins at pass j % 8
# case: (P, positions behind P that every row runs through, pass at which the unattached row joins -- None: there is none and slot
# 127 is attached too).  P + run <= seq_len: behind P = 690 there are 14 positions
WIDE_PREFIX_CASES = {"P560": (560, 40, WIDE_STAGGER), "P690": (690, 14, WIDE_STAGGER), "P19-own": (19, 150, None)}


def wide_prefix_passes(case: str):
    """test 4: [[(slot, first, pos) of every row, in row order]].  Attached slot j feeds positions P + 1 .. P + run in passes j % 8 ..;
    the unattached slot (first = 0), forked at P, feeds the same positions from pass `join` on: the pass before it has 127 rows, that
    pass 128.  Rows are listed by DESCENDING slot (the unattached row first: row index != column)."""
    P, run, join = WIDE_PREFIX_CASES[case]
    natt = WIDE_ATTACHED if join is not None else MAX_BATCH
    start = {j: j % WIDE_STAGGER for j in range(natt)}
    first = {j: P for j in range(natt)}
    if join is not None:
        start[WIDE_ATTACHED], first[WIDE_ATTACHED] = join, 0
    passes = []
    for t in range(max(start.values()) + run):
        passes.append([(j, first[j], P + 1 + t - start[j]) for j in sorted(start, reverse=True) if start[j] <= t < start[j] + run])
    return passes
