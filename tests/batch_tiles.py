"""TEST INFRASTRUCTURE -- mirrors of the batched decode attention's tile and part arithmetic (llm.f90_amd/csrc/batch.h), as
tests/attn_needle.py keeps them for the other attention kernels.  Used by tests/test_batch_cpu.py (does the arithmetic cover every
timestep once?) and tests/test_batch_gpu.py (which positions sit on a boundary?); the last section holds the case tables of
tests/test_batch_wide_gpu.py, which tests/test_batch_wide_cpu.py checks on these mirrors."""
from __future__ import annotations

BD_TILE = 16          # csrc/batch.h: cache rows per MFMA tile
BD_WAVES = 8          # waves of a workgroup; a part's tiles go round robin
BD_MAX_PARTS = 8      # workgroups a row's timesteps are split over, at most
BD_MAX_GROUP = 16     # query heads per kv head, at most
N_CU = 256            # MI355X (what the library reads from the device properties)


def bd_parts(n: int, n_kv_heads: int, max_pos: int, n_cu: int = N_CU) -> int:
    """bd_parts (batch.h): parts of a pass of n rows whose longest has max_pos timesteps"""
    ntile = (max_pos + BD_TILE - 1) // BD_TILE
    parts = min(n_cu // (n * n_kv_heads), (ntile + BD_WAVES - 1) // BD_WAVES, BD_MAX_PARTS)
    return max(parts, 1)


def bd_tiles_per_part(max_pos: int, parts: int) -> int:
    ntile = (max_pos + BD_TILE - 1) // BD_TILE
    return (ntile + parts - 1) // parts


def part_tiles(pos: int, part: int, tpp: int):
    """tiles [t0, t1) of a row of `pos` timesteps that part `part` takes (bd_attn_kernel): possibly none"""
    ntile = (pos + BD_TILE - 1) // BD_TILE
    t0 = part * tpp
    return t0, max(t0, min(t0 + tpp, ntile))


def wave_tiles(t0: int, t1: int, wave: int):
    """the tiles of a part that wave `wave` multiplies (kt = t0 + wave; kt < t1; kt += BD_WAVES)"""
    return list(range(t0 + wave, t1, BD_WAVES))


def covered_timesteps(pos: int, parts: int, max_pos: int | None = None):
    """every (timestep) a pass visits for a row of `pos` timesteps, with multiplicity, at a part count chosen for max_pos >= pos"""
    tpp = bd_tiles_per_part(pos if max_pos is None else max_pos, parts)
    seen = []
    for p in range(parts):
        t0, t1 = part_tiles(pos, p, tpp)
        for w in range(BD_WAVES):
            for kt in wave_tiles(t0, t1, w):
                seen += [r for r in range(kt * BD_TILE, (kt + 1) * BD_TILE) if r < pos]      # the predicate row < pos
    return seen


def boundary_positions(limit: int, lo: int = 2):
    """positions k in [lo, limit] at, one below and one above every multiple of BD_TILE -- every part boundary of every part count
    is a multiple of BD_TILE (a part is whole tiles), so these cover the split rule's boundaries too"""
    ks = set()
    for m in range(BD_TILE, limit + 2, BD_TILE):
        ks |= {m - 1, m, m + 1}
    return sorted(k for k in ks if lo <= k <= limit)


def part_boundaries(pos: int, n: int, n_kv_heads: int):
    """the first timestep (0-based cache row) of parts 1.. of a row of `pos` timesteps run alone among n rows"""
    parts = bd_parts(n, n_kv_heads, pos)
    tpp = bd_tiles_per_part(pos, parts)
    return [p * tpp * BD_TILE for p in range(1, parts) if p * tpp * BD_TILE < pos]


# ---- wide passes (tests/test_batch_wide_cpu.py, tests/test_batch_wide_gpu.py) ---------------------------------------------------------
def tiles_per_wave(n: int, n_kv_heads: int, max_pos: int, pos: int, n_cu: int = N_CU):
    """[part][wave] -> the tiles that wave multiplies for a row of `pos` timesteps inside a pass of n rows whose longest has max_pos"""
    parts = bd_parts(n, n_kv_heads, max_pos, n_cu)
    tpp = bd_tiles_per_part(max_pos, parts)
    return [[wave_tiles(*part_tiles(pos, p, tpp), w) for w in range(BD_WAVES)] for p in range(parts)]


def max_tiles_per_wave(n: int, n_kv_heads: int, max_pos: int, pos: int | None = None) -> int:
    """the most tiles any wave of a row takes (the longest row's, unless `pos` names another)"""
    return max(len(ts) for part in tiles_per_wave(n, n_kv_heads, max_pos, max_pos if pos is None else pos) for ts in part)


# tests 2 and 3 of tests/test_batch_wide_gpu.py: shape -> (kv heads, positions of the transcript, row counts of the passes)
WIDE_SHAPES = {"tk-small-long": (2, 704, (32, 33, 64, 65, 128)), "tiny-hs128w-long": (4, 320, (32, 33, 128))}
WIDE_SEED = 20261020
SHORT_ROW = 40        # a row of 3 tiles next to the longest one: parts >= 1 are empty for it, and so are waves 3..7 of part 0


def wide_transcript_passes(shape: str):
    """test 2: {row count: [k of every row, in row order]}.  Every pass holds the longest row; the widest pass holds a row of every
    tile count 1 .. ntile (k = 16 c); the positions of boundary_positions() are dealt out over the passes, the widest first; every
    pass of two or more parts holds a row of SHORT_ROW timesteps; what is left is filled with other positions.  Rows are shuffled
    (seeded): the longest row is not row 0."""
    import random
    nkv, n_pos, counts = WIDE_SHAPES[shape]
    rng = random.Random(WIDE_SEED)
    ntile = n_pos // BD_TILE
    widest = max(counts)
    every_count = [BD_TILE * c for c in range(1, ntile)] + [n_pos]
    pool = [k for k in boundary_positions(n_pos) if k not in every_count]
    rng.shuffle(pool)
    others = [k for k in range(1, n_pos) if k not in every_count and k not in pool and k != SHORT_ROW]
    rng.shuffle(others)
    pool += others
    passes = {}
    for n in sorted(counts, reverse=True):
        ks = list(every_count) if n == widest else [n_pos]
        if bd_parts(n, nkv, n_pos) >= 2:
            ks.append(SHORT_ROW)
        while len(ks) < n:
            k = pool.pop(0)
            if k not in ks:
                ks.append(k)
        rng.shuffle(ks)
        passes[n] = ks
    return passes


# test 3: needles of kv heads 0 | 1 on the two sides of boundaries that only a wave's SECOND tile or a wide pass's parts have
# (tk-small-long geometry, S = 704): 127 | 128 (wave 7's first tile, wave 0's second) and 255 | 256 (its third) at one part; 351 | 352
# (the part boundary of a 64-row pass: 22 tiles per part) and 479 | 480 (part 1, wave 0's second tile); 687 | 688 (the last tile of the
# context: what every clamped look-ahead load reads); the sink and the last row as tests/test_batch_gpu.py has them
WIDE_NEEDLE_S = 704
WIDE_NEEDLES = {0: [0, 127, 255, 351, 479, 687, 703], 1: [128, 256, 352, 480, 688]}
WIDE_NEEDLE_ROWS = (128, 64)


def wide_needle_passes():
    """test 3: {row count: [k of every row]}: for every needle row t the positions t + 1 (the needle is the row this pass writes) and
    t + 2 (it comes from the fork), and S; filled up with other positions (seeded), shuffled"""
    import random
    S = WIDE_NEEDLE_S
    rng = random.Random(WIDE_SEED + 1)
    must = sorted({k for ts in WIDE_NEEDLES.values() for t in ts for k in (t + 1, t + 2) if k <= S} | {S})
    others = [k for k in range(1, S) if k not in must]
    rng.shuffle(others)
    passes = {}
    for n in WIDE_NEEDLE_ROWS:
        ks = must + [others.pop(0) for _ in range(n - len(must))]
        rng.shuffle(ks)
        passes[n] = ks
    return passes


def wide_needle_case():
    """(shape with seq_len S, layout, tokens, needle-shaped f32 weights) of test 3"""
    import attn_needle as an
    from llm_f90_amd.tools import gguf
    s0 = gguf.SHAPES["tk-small-long"]
    s = gguf.LlamaShape(s0.emb_dim, s0.hidden_dim, s0.n_layers, s0.n_heads, s0.n_kv_heads, s0.vocab_size, WIDE_NEEDLE_S)
    layout = {g: sorted(ts) for g, ts in WIDE_NEEDLES.items()}
    tokens, needle_tokens = an.needle_sequence(s, layout, WIDE_SEED)
    fw = an.shape_needles(gguf.synth_fused(s, 4242), needle_tokens, an.BETA)
    return s, layout, tokens, fw


# test 1: the row counts of the passes, three times over and a last full pass.  Every edge of the GEMM's 16-row groups (16 | 17 ..
# 112 | 113), the plan switches at T = 96 and at (T + 15) / 16 == 8 (113 .. 128), and 1, 2, 3; a wide pass is followed by a narrow one
WIDTHS = (128, 17, 113, 16, 112, 33, 97, 32, 96, 3, 65, 2, 64, 1)
WIDTH_SCHEDULE = WIDTHS * 3 + (128,)


def width_passes(n_slots: int = 128, schedule=WIDTH_SCHEDULE, seed: int = WIDE_SEED + 2):
    """test 1: [[(slot, pos) of every row, in row order]] -- pass t feeds the schedule[t] slots that have advanced least (ties by
    DESCENDING slot), listed in a seeded permutation"""
    import random
    rng = random.Random(seed)
    fed = [0] * n_slots
    passes = []
    for w in schedule:
        slots = sorted(range(n_slots), key=lambda j: (fed[j], -j))[:w]
        rng.shuffle(slots)
        rows = []
        for j in slots:
            fed[j] += 1
            rows.append((j, fed[j]))
        passes.append(rows)
    return passes
