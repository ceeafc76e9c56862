"""TEST INFRASTRUCTURE -- mirrors of the batched decode attention's tile and part arithmetic (llm.f90_amd/csrc/batch.h), as
tests/attn_needle.py keeps them for the other attention kernels.  Used by tests/test_batch_cpu.py (does the arithmetic cover every
timestep once?) and tests/test_batch_gpu.py (which positions sit on a boundary?)."""
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
