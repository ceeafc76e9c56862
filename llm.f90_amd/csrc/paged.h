// Paged K/V caches (llmk_pages_*): a batch made by llmk_pages_create keeps ONE pool of pages,
// [L][n_pages][page_len][KV] per K and V in f32 or f16, and a table per slot, [n_slots][width] with width = ceil(seq_len / page_len):
// entry i of a slot is the physical page of its positions i * page_len + 1 .. (i + 1) * page_len, -1 for none.  page_len is a multiple
// of BD_TILE, so a 16-row MFMA tile never straddles a page.  Here:
//   PagePool                 the host's allocator: lowest free page first, a reference count per page, every change undoable
//   bd_attn_paged_kernel     bd_attn_kernel's work split over a slot's pages: the tiles' physical rows staged in LDS, then the shared
//                            tile loop of attn_tiles.h with the tile's pointer taken from there
//   bd_attn_span_paged_kernel   bd_attn_span_kernel's column groups over a slot's pages: a span's rows read the slot once per group
//   pg_stem_groups / bd_attn_stem / bd_attn_paged_own      stem reads (llmk_stems_*): pages that rows share read once per group
//   bd_epi_qkv_paged[_h]     bd_epi_qkv[_h]_kernel with the store row taken through the table
//   bd_page_copy / bd_to_pages / bd_from_pages      copy on write and the partial page of a share; llmk_batch_fork; llmk_cache_peek
// The rows of a page behind its slot's position hold whatever the page's last owner left: no kernel reads them (the tile loop clamps
// every row index to the row's last position).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstddef>
#include <vector>

#include "batch.h"

namespace llmk {

constexpr int PG_MIN_LEN = BD_TILE, PG_MAX_LEN = 256;

// what the kernels know of the tables
struct BdPages {
    const int* table;      // [n_slots][width]
    int width, page_len, n_pages;
};
// the physical cache row of position row + 1 of `slot`, -1 where the slot has no page there
__device__ __forceinline__ int pg_row(const BdPages& pg, int slot, int row) {
    const int e = pg.table[(size_t)slot * pg.width + row / pg.page_len];
    return (unsigned)e < (unsigned)pg.n_pages ? e * pg.page_len + row % pg.page_len : -1;
}

// ---- the allocator (host, plain C++: nothing here touches the device)                                                  ------------
// Deterministic: a fresh page is the lowest-numbered free one.  A page's count is the table entries that name it.  Every change of an
// entry goes through set(), which keeps the counts and writes the undo log; undo() takes the tables and counts back to a mark, so a
// call that runs out of pages leaves them exactly as it found them.
struct PagePool {
    struct Copy { int src, dst; };                 // page src is to be copied onto the fresh page dst (copy on write)
    struct Change { int at, was, now; };
    int page_len = 0, n_pages = 0, width = 0, n_free = 0;
    std::vector<int> table, ref;                   // [n_slots][width], -1: none; [n_pages]
    std::vector<Change> log;

    void init(int n_slots, int seq_len, int page_len_, int n_pages_) {
        page_len = page_len_; n_pages = n_free = n_pages_;
        width = (seq_len + page_len - 1) / page_len;
        table.assign((size_t)n_slots * width, -1);
        ref.assign(n_pages, 0);
        log.clear();
    }
    int* of(int slot) { return table.data() + (size_t)slot * width; }
    int lowest_free() const {
        for (int p = 0; p < n_pages; ++p)
            if (ref[p] == 0) return p;
        return -1;
    }
    void set(int at, int now) {
        const int was = table[at];
        if (was == now) return;
        if (was >= 0 && --ref[was] == 0) ++n_free;
        if (now >= 0 && ref[now]++ == 0) --n_free;
        table[at] = now;
        log.push_back(Change{at, was, now});
    }
    size_t mark() const { return log.size(); }
    void undo(size_t to) {
        while (log.size() > to) {
            const Change c = log.back();
            log.pop_back();
            if (c.now >= 0 && --ref[c.now] == 0) ++n_free;
            if (c.was >= 0 && ref[c.was]++ == 0) --n_free;
            table[c.at] = c.was;
        }
    }
    // Positions pos0 .. pos0+len-1 (1-based) of `slot` are about to be written: every page up to the last of them becomes present,
    // and those the positions lie in exclusively owned -- a shared one is replaced by a fresh page and the copy is noted.  false: out
    // of pages (the caller undoes).
    bool ensure(int slot, int pos0, int len, std::vector<Copy>& copies) {
        const int first = (pos0 - 1) / page_len, last = (pos0 + len - 2) / page_len;
        for (int i = 0; i <= last; ++i) {
            const int at = slot * width + i, was = table[at];
            if (was >= 0 && (i < first || ref[was] == 1)) continue;
            const int fresh = lowest_free();
            if (fresh < 0) return false;
            set(at, fresh);
            if (was >= 0) copies.push_back(Copy{was, fresh});
        }
        return true;
    }
    // the slot keeps positions 1..n_keep: the pages wholly behind them go
    void release(int slot, int n_keep) {
        for (int i = (n_keep + page_len - 1) / page_len; i < width; ++i) set(slot * width + i, -1);
    }
    // mapped entries of a slot: always a run from entry 0 (ensure fills from there, release cuts a tail)
    int count(int slot) const {
        int n = 0;
        while (n < width && table[(size_t)slot * width + n] >= 0) ++n;
        return n;
    }
};

// ---- decode attention through the table                                                                                ------------
// bd_attn_kernel's work split: one workgroup per (kv head, row, part), bd_parts / bd_tiles_per_part, 8 waves round robin, the kv group's
// query heads as the 16 columns, the part states and the fold of that kernel (stride BD_MAX_GROUP; parts == 1: normalised to `out`).
// What is new is where a tile lies: logical tile kt of the row's slot starts at physical row table[slot][kt / tpg] * page_len +
// (kt % tpg) * 16, tpg = page_len / 16.  The K/V loads would hang on a table load each; so the workgroup first stages the physical rows
// of ITS tiles -- [t0, t1) and the NW look-ahead tiles behind them, clamped as the loop clamps -- in LDS behind the merge's block (the
// merge of a fast wave must not overwrite what a slow one still reads), one global round trip next to the Q load, and the loop takes a
// tile's pointer from an LDS word, the same for the whole wave.  The tile loop IS attn_tiles (the statements of bd_attn_kernel in that
// order): a row's arithmetic does not depend on where its pages lie.  An entry out of range reads page n_pages - 1 (the host maps every
// page of a row before a pass).  Dynamic LDS: pg_attn_smem.
constexpr size_t pg_attn_smem(int hs, int seq_len) { return attn_smem(BD_WAVES, hs) + (size_t)((seq_len + BD_TILE - 1) / BD_TILE) * sizeof(int); }
constexpr size_t PG_MAX_SMEM = 160 * 1024;      // a gfx950 workgroup's LDS: llmk_pages_create refuses a seq_len whose tiles do not fit behind the merge
template <int HS, class T>
__global__ __launch_bounds__(BD_WAVES * WAVE) void bd_attn_paged_kernel(const float* __restrict__ Q, const T* __restrict__ kc,
                                                                        const T* __restrict__ vc, float* __restrict__ out,
                                                                        float* __restrict__ po, float2* __restrict__ pml, BdCaches bc,
                                                                        BdPages pg, int KV, int kv_mul, int E, int tpp) {
    constexpr int DG = HS / 4, NT = HS / 16, NW = BD_WAVES;
    extern __shared__ __attribute__((aligned(16))) char pf_smem[];
    int* tile_row = reinterpret_cast<int*>(pf_smem + attn_smem(NW, HS));      // [tiles of seq_len], this workgroup's filled in
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 15, g = lane >> 4;
    const int kvh = blockIdx.x, b = blockIdx.y, part = blockIdx.z, parts = gridDim.z, nkv = gridDim.x;
    const BdRow row = bc.rows[b];
    if (!bd_row_ok(bc, row)) return;                  // whole workgroup: no barrier is pending
    const int nrows = row.pos;
    const int ntile = (nrows + BD_TILE - 1) / BD_TILE, t0 = part * tpp, t1 = min(t0 + tpp, ntile);
    {
        const int tpg = pg.page_len / BD_TILE;
        const int* tab = pg.table + (size_t)row.slot * pg.width;
        for (int t = min(t0, ntile - 1) + tid; t < min(t1 + NW, ntile); t += NW * WAVE) {
            const unsigned e = min((unsigned)tab[t / tpg], (unsigned)(pg.n_pages - 1));
            tile_row[t] = (int)e * pg.page_len + (t % tpg) * BD_TILE;
        }
    }
    const int h = kvh * kv_mul + min(li, kv_mul - 1);
    float qf[DG];
    attn_load_q<HS>(qf, Q + (size_t)b * E + (size_t)h * HS + g * DG);
    __syncthreads();
    float m_run, l_run;
    pf_v4f O[NT];
    attn_tiles<HS, T, NW>(qf, kc + (size_t)kvh * HS + g * DG, vc + (size_t)kvh * HS + NT * li, KV, nrows - 1, ntile, t0, t1, wid, li, g,
                          [&](int r) { return r < nrows; }, m_run, l_run, O,
                          [&](const T* p, int tile) { return p + (ptrdiff_t)(tile_row[tile] - tile * BD_TILE) * KV; });
    const size_t pbase = ((size_t)b * nkv + kvh) * parts + part;
    attn_merge_waves<HS, NW>(m_run, l_run, O, kv_mul, [&](int q, int d, float M, float L, float val) {
        if (parts == 1) {
            out[(size_t)b * E + (size_t)(kvh * kv_mul + q) * HS + d] = val / L;
        } else {
            po[(pbase * BD_MAX_GROUP + q) * HS + d] = val;
            if (d == 0) pml[pbase * BD_MAX_GROUP + q] = make_float2(M, L);
        }
    });
}

// ---- span attention through the table                                                                                  ------------
// bd_attn_span_body's work split over a slot's pages: one workgroup per (kv head, column group, part), the groups of span_upload
// (BdGroup: up to bd_prefix_rg(kv_mul) consecutive rows of one span), the ONE split rule of the pass (bd_span_parts, part p of a group
// takes tiles [p * tpp, (p + 1) * tpp) cut at the group's last tile -- possibly none), 8 waves round robin.  Column c is (row first +
// c / kv_mul, query head c % kv_mul of the kv head); columns from the last live one on repeat it and are not written out.  The lane
// of column c sees cache rows 0 .. pos(c's row) - 1: a paged batch has no attached slots, so every range starts at row 0.  The slot's
// pages cross L2 once per group instead of once per row.
// Where a tile lies is bd_attn_paged_kernel's answer: the physical rows of the workgroup's tiles [t0, t1) and of the NW look-ahead
// tiles behind them (clamped to the group's last tile, as the loop clamps; an empty part stages that last tile alone, which the loop's
// first request names) go to LDS behind the merge's block in one global round trip next to the Q load, and the loop takes a tile's
// pointer from one LDS word.  Two kinds of rows are in reach and must stay unread:
//   rows of the last tile behind the group's last position -- whatever the page's last owner left: the loop clamps every row index
//       to rowl.pos - 1, and that row lies in the tile the clamp is applied in (tile <= ntile - 1 <= (rowl.pos - 1) / 16);
//   rows of the span's later columns -- bd_epi_qkv_paged[_h]_kernel of this same pass has written them: the predicate r < vis alone
//       keeps them out, as in the dense kernel.
// direct (one part in the pass): the normalised output goes to `out`; else part `part` leaves state `part` of every (row, kv head) of
// the group (stride kv_mul, np states) for bd_attn_fold_kernel.  Groups, parts, tile order and every statement of the arithmetic are
// those of bd_attn_span_kernel on a dense batch that holds the same rows: the results are the same bits.  Dynamic LDS: pg_attn_smem.
template <int HS, class T>
__global__ __launch_bounds__(BD_WAVES * WAVE) void bd_attn_span_paged_kernel(const float* __restrict__ Q, const T* __restrict__ kc,
                                                                             const T* __restrict__ vc, float* __restrict__ out,
                                                                             float* __restrict__ po, float2* __restrict__ pml, BdCaches bc,
                                                                             const BdGroup* __restrict__ groups, BdPages pg, int n, int KV,
                                                                             int kv_mul, int E, int tpp, int np, int direct) {
    constexpr int DG = HS / 4, NT = HS / 16, NW = BD_WAVES;
    extern __shared__ __attribute__((aligned(16))) char pf_smem[];
    int* tile_row = reinterpret_cast<int*>(pf_smem + attn_smem(NW, HS));      // [tiles of seq_len], this workgroup's filled in
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 15, g = lane >> 4;
    const int kvh = blockIdx.x, part = blockIdx.z, nkv = gridDim.x;
    const BdGroup gr = groups[blockIdx.y];
    if (gr.first < 0 || gr.rows < 1 || gr.rows > bd_prefix_rg(kv_mul) || gr.rows > n - gr.first) return;      // whole workgroup: no barrier is pending
    const BdRow row0 = bc.rows[gr.first], rowl = bc.rows[gr.first + gr.rows - 1];
    if (!bd_row_ok(bc, row0) || !bd_row_ok(bc, rowl) || rowl.slot != row0.slot || rowl.pos != row0.pos + gr.rows - 1) return;
    const int ntile = (rowl.pos + BD_TILE - 1) / BD_TILE, t0 = part * tpp, t1 = min(t0 + tpp, ntile);
    {
        const int tpg = pg.page_len / BD_TILE;
        const int* tab = pg.table + (size_t)row0.slot * pg.width;
        for (int t = min(t0, ntile - 1) + tid; t < min(t1 + NW, ntile); t += NW * WAVE) {
            const unsigned e = min((unsigned)tab[t / tpg], (unsigned)(pg.n_pages - 1));
            tile_row[t] = (int)e * pg.page_len + (t % tpg) * BD_TILE;
        }
    }
    const int live = gr.rows * kv_mul, c = min(li, live - 1);
    const int vis = row0.pos + c / kv_mul;            // this lane's column sees cache rows 0 .. vis-1
    float qf[DG];
    attn_load_q<HS>(qf, Q + (size_t)(gr.first + c / kv_mul) * E + (size_t)(kvh * kv_mul + c % kv_mul) * HS + g * DG);
    __syncthreads();
    float m_run, l_run;
    pf_v4f O[NT];
    attn_tiles<HS, T, NW>(qf, kc + (size_t)kvh * HS + g * DG, vc + (size_t)kvh * HS + NT * li, KV, rowl.pos - 1, ntile, t0, t1, wid, li, g,
                          [&](int r) { return r < vis; }, m_run, l_run, O,
                          [&](const T* p, int tile) { return p + (ptrdiff_t)(tile_row[tile] - tile * BD_TILE) * KV; });
    attn_merge_waves<HS, NW>(m_run, l_run, O, live, [&](int col, int d, float M, float L, float val) {
        const int b = gr.first + col / kv_mul, q = col % kv_mul;
        if (direct) {
            out[(size_t)b * E + (size_t)(kvh * kv_mul + q) * HS + d] = val / L;
        } else {
            const size_t s = (((size_t)b * nkv + kvh) * np + part) * kv_mul + q;
            po[s * HS + d] = val;
            if (d == 0) pml[s] = make_float2(M, L);
        }
    });
}

// ---- stem reads (llmk_stems_*): slots that name the same pages at the head of their tables read them once per pass     ------------
// The structure of a dense pass with attached rows (batch.h: prefix kernel, own kernel, fold) over pages: any number of stems in one
// pass, a stem length per group, and every tile found through a table.
//   pg_stem_groups            the grouping rule: host, plain C++, a function of (tables, rows) alone
//   bd_attn_stem_kernel       a group's shared pages against the query heads of up to RG member rows at once: one read per group
//   bd_attn_paged_own_kernel  bd_attn_own_kernel through the row's table: cache rows first[slot] .. pos-1, never normalising
// and bd_attn_fold_kernel (batch.h) as it stands: stride kv_mul, `first` telling which rows have stem parts.

// The rule.  rg = bd_prefix_rg(kv_mul).  cand(i) = (pos[i] - 1) / page_len: the entries of row i's table wholly in front of the page
// the row writes.  common(i, j): the leading entries equal (and present) in both slots' tables, at most min(cand(i), cand(j)).  Rows
// are walked in row order; an unassigned row i leads: G = max common(i, j) over the later unassigned rows j; G == 0: i is in no
// group.  Else its members are i and, in row order, the later unassigned rows with common(i, j) >= (G + 1) / 2, up to rg rows in all
// -- a row that shares one page with the leader does not pull down a group that shares ten, one that diverged a page earlier still
// joins -- and the group's stem is the minimum of common(i, j) over them, in pages.  Rows left over when a group is full lead in their
// turn.  A stem is whole pages in front of every member's write page: no ragged tile, no causal edge, every member sees all of it.
// group[i]: the row's group, numbered in the order the leaders appear, -1 for none; stem[i]: the positions the stem kernel reads for
// it, 0 for none.  Returns the number of groups.
inline int pg_stem_groups(const PagePool& pl, int rg, int n, const int* slots, const int* pos, int* group, int* stem) {
    constexpr int OPEN = -2;
    const auto common = [&](int i, int j) {
        const int cap = std::min((pos[i] - 1) / pl.page_len, (pos[j] - 1) / pl.page_len);
        const int *a = pl.table.data() + (size_t)slots[i] * pl.width, *b = pl.table.data() + (size_t)slots[j] * pl.width;
        int k = 0;
        while (k < cap && a[k] >= 0 && a[k] == b[k]) ++k;
        return k;
    };
    for (int i = 0; i < n; ++i) { group[i] = OPEN; stem[i] = 0; }
    int ng = 0;
    for (int i = 0; i < n; ++i) {
        if (group[i] != OPEN) continue;
        int G = 0;
        for (int j = i + 1; rg > 1 && j < n; ++j)
            if (group[j] == OPEN) G = std::max(G, common(i, j));
        if (G == 0) { group[i] = -1; continue; }
        int members = 1, pages = INT_MAX;
        group[i] = ng;
        for (int j = i + 1; j < n && members < rg; ++j) {
            if (group[j] != OPEN) continue;
            const int c = common(i, j);
            if (c < (G + 1) / 2) continue;
            group[j] = ng;
            pages = std::min(pages, c);
            ++members;
        }
        for (int j = i; j < n; ++j)
            if (group[j] == ng) stem[j] = pages * pl.page_len;
        ++ng;
    }
    return ng;
}

// a group of the pass: the slot whose table the stem is read through (the leader's), the stem's tiles, and the members' rows of the
// pass in row order, -1 behind the last
struct BdStem { int slot, tiles; int col[BD_MAX_GROUP]; };

// One workgroup per (kv head, group, stem part), 8 waves round robin.  Column c is (member c / kv_mul, query head c % kv_mul of the kv
// head); columns from the last live one on repeat it and are not written out, as in bd_attn_prefix_body.  Tile kt of the stem starts
// at physical row table[leader slot][kt / tpg] * page_len + (kt % tpg) * 16; the workgroup stages the rows of ITS tiles and of the
// look-ahead tiles behind them in LDS behind the merge's block, as bd_attn_paged_kernel does, and the shared loop takes a tile's
// pointer from one LDS word.  The split rule is ONE for the pass -- bd_parts(groups, n_kv_heads, the longest stem, n_cu) and
// bd_tiles_per_part of the longest stem -- so a part can lie wholly behind a shorter group's stem: it leaves M = -inf, L = 0 and zeros
// for every live column, which is what the fold accepts from an empty span part.  Part states: stride kv_mul, np per (row, kv head),
// the stem's in front (batch.h, a pass with attached rows).  Dynamic LDS: pg_attn_smem.
template <int HS, class T>
__global__ __launch_bounds__(BD_WAVES * WAVE) void bd_attn_stem_kernel(const float* __restrict__ Q, const T* __restrict__ kc,
                                                                       const T* __restrict__ vc, float* __restrict__ po,
                                                                       float2* __restrict__ pml, BdCaches bc,
                                                                       const BdStem* __restrict__ stems, BdPages pg, int n, int KV,
                                                                       int kv_mul, int E, int tpp, int np) {
    constexpr int DG = HS / 4, NT = HS / 16, NW = BD_WAVES;
    extern __shared__ __attribute__((aligned(16))) char pf_smem[];
    int* tile_row = reinterpret_cast<int*>(pf_smem + attn_smem(NW, HS));      // [tiles of seq_len], this workgroup's filled in
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 15, g = lane >> 4;
    const int kvh = blockIdx.x, part = blockIdx.z, nkv = gridDim.x, rg = bd_prefix_rg(kv_mul);
    const BdStem& st = stems[blockIdx.y];
    const int ntile = st.tiles;
    int nr = 0;
    while (nr < rg && (unsigned)st.col[nr] < (unsigned)n) ++nr;
    // whole workgroup: no barrier is pending (a stem lies in front of a position of the slot, so it is shorter than seq_len)
    if (nr == 0 || (unsigned)st.slot >= (unsigned)bc.n_slots || ntile < 1 || ntile * BD_TILE >= bc.seq_len) return;
    const int live = nr * kv_mul, c = min(li, live - 1);
    const int t0 = part * tpp, t1 = min(t0 + tpp, ntile);
    const auto state = [&](int col) { return (((size_t)st.col[col / kv_mul] * nkv + kvh) * np + part) * kv_mul + col % kv_mul; };
    if (t0 >= ntile) {
        for (int idx = tid; idx < live * HS; idx += NW * WAVE) {
            const size_t s = state(idx / HS);
            po[s * HS + idx % HS] = 0.f;
            if (idx % HS == 0) pml[s] = make_float2(-INFINITY, 0.f);
        }
        return;
    }
    {
        const int tpg = pg.page_len / BD_TILE;
        const int* tab = pg.table + (size_t)st.slot * pg.width;
        for (int t = t0 + tid; t < min(t1 + NW, ntile); t += NW * WAVE) {
            const unsigned e = min((unsigned)tab[t / tpg], (unsigned)(pg.n_pages - 1));
            tile_row[t] = (int)e * pg.page_len + (t % tpg) * BD_TILE;
        }
    }
    float qf[DG];
    attn_load_q<HS>(qf, Q + (size_t)st.col[c / kv_mul] * E + (size_t)(kvh * kv_mul + c % kv_mul) * HS + g * DG);
    __syncthreads();
    float m_run, l_run;
    pf_v4f O[NT];
    const int P = ntile * BD_TILE;
    attn_tiles<HS, T, NW>(qf, kc + (size_t)kvh * HS + g * DG, vc + (size_t)kvh * HS + NT * li, KV, P - 1, ntile, t0, t1, wid, li, g,
                          [&](int r) { return r < P; }, m_run, l_run, O,
                          [&](const T* p, int tile) { return p + (ptrdiff_t)(tile_row[tile] - tile * BD_TILE) * KV; });
    attn_merge_waves<HS, NW>(m_run, l_run, O, live, [&](int col, int d, float M, float L, float val) {
        const size_t s = state(col);
        po[s * HS + d] = val;
        if (d == 0) pml[s] = make_float2(M, L);
    });
}

// bd_attn_own_body's split and predicate through the row's table: cache rows lo .. pos-1 of the row's slot, lo = first[slot] (the
// row's stem in rows, 0 for a row in no group), tiles counted from lo / 16 and staged as above; part `part` leaves state p0 + part,
// never normalised.  One workgroup per (kv head, row, own part).  Dynamic LDS: pg_attn_smem.
template <int HS, class T>
__global__ __launch_bounds__(BD_WAVES * WAVE) void bd_attn_paged_own_kernel(const float* __restrict__ Q, const T* __restrict__ kc,
                                                                            const T* __restrict__ vc, float* __restrict__ po,
                                                                            float2* __restrict__ pml, BdCaches bc, BdPages pg,
                                                                            const int* __restrict__ first, int KV, int kv_mul, int E,
                                                                            int tpp, int np, int p0) {
    constexpr int DG = HS / 4, NT = HS / 16, NW = BD_WAVES;
    extern __shared__ __attribute__((aligned(16))) char pf_smem[];
    int* tile_row = reinterpret_cast<int*>(pf_smem + attn_smem(NW, HS));
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 15, g = lane >> 4;
    const int kvh = blockIdx.x, b = blockIdx.y, part = blockIdx.z, nkv = gridDim.x;
    const BdRow row = bc.rows[b];
    if (!bd_row_ok(bc, row)) return;                  // whole workgroup: no barrier is pending
    const int lo = first[row.slot], nrows = row.pos;
    if ((unsigned)lo >= (unsigned)nrows) return;      // (the host ends a stem in front of the row's position)
    const int ntile = (nrows + BD_TILE - 1) / BD_TILE, t0 = lo / BD_TILE + part * tpp, t1 = min(t0 + tpp, ntile);
    {
        const int tpg = pg.page_len / BD_TILE;
        const int* tab = pg.table + (size_t)row.slot * pg.width;
        for (int t = min(t0, ntile - 1) + tid; t < min(t1 + NW, ntile); t += NW * WAVE) {
            const unsigned e = min((unsigned)tab[t / tpg], (unsigned)(pg.n_pages - 1));
            tile_row[t] = (int)e * pg.page_len + (t % tpg) * BD_TILE;
        }
    }
    const int h = kvh * kv_mul + min(li, kv_mul - 1);
    float qf[DG];
    attn_load_q<HS>(qf, Q + (size_t)b * E + (size_t)h * HS + g * DG);
    __syncthreads();
    float m_run, l_run;
    pf_v4f O[NT];
    attn_tiles<HS, T, NW>(qf, kc + (size_t)kvh * HS + g * DG, vc + (size_t)kvh * HS + NT * li, KV, nrows - 1, ntile, t0, t1, wid, li, g,
                          [&](int r) { return lo <= r && r < nrows; }, m_run, l_run, O,
                          [&](const T* p, int tile) { return p + (ptrdiff_t)(tile_row[tile] - tile * BD_TILE) * KV; });
    attn_merge_waves<HS, NW>(m_run, l_run, O, kv_mul, [&](int q, int d, float M, float L, float val) {
        const size_t s = (((size_t)b * nkv + kvh) * np + p0 + part) * kv_mul + q;
        po[s * HS + d] = val;
        if (d == 0) pml[s] = make_float2(M, L);
    });
}

// ---- the QKV epilogues through the table                                                                               ------------
// bd_epi_qkv[_h]_kernel: rotated at the row's position, stored at the physical row of that position -- pf_epi_qkv_pair[_h] store at cache
// row a.pos0 + t - 1, so they are handed the layer's pool moved on by (physical row - logical row) rows, as the tree epilogues are
// (batch.h), with their arithmetic untouched.  A row without a page there is not written (the host maps it before the pass).
__global__ void bd_epi_qkv_paged_kernel(PfEpiArgs a, BdCaches bc, BdPages pg) {
    const int p4 = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    pf_low_check(a, blockIdx.x == 0 && blockIdx.y == 0);
    if (p4 >= a.rows / 4) return;
    const BdRow r = bc.rows[t];
    if (!bd_row_ok(bc, r)) return;
    const int at = pg_row(pg, r.slot, r.pos - 1);
    if (at < 0) return;
    const float4 s4 = pf_sum4(a, t, 4 * p4);
    a.pos0 = r.pos - t;
    a.kc += (ptrdiff_t)(at - (r.pos - 1)) * a.KV;
    a.vc += (ptrdiff_t)(at - (r.pos - 1)) * a.KV;
    pf_epi_qkv_pair(a, t, 4 * p4, s4.x / a.xn[t], s4.y / a.xn[t]);
    pf_epi_qkv_pair(a, t, 4 * p4 + 2, s4.z / a.xn[t], s4.w / a.xn[t]);
}
__global__ void bd_epi_qkv_paged_h_kernel(PfEpiArgs a, BdCaches bc, BdPages pg, _Float16* __restrict__ kc, _Float16* __restrict__ vc) {
    const int p4 = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    pf_low_check(a, blockIdx.x == 0 && blockIdx.y == 0);
    if (p4 >= a.rows / 4) return;
    const BdRow r = bc.rows[t];
    if (!bd_row_ok(bc, r)) return;
    const int at = pg_row(pg, r.slot, r.pos - 1);
    if (at < 0) return;
    const float4 s4 = pf_sum4(a, t, 4 * p4);
    a.pos0 = r.pos - t;
    kc += (ptrdiff_t)(at - (r.pos - 1)) * a.KV;
    vc += (ptrdiff_t)(at - (r.pos - 1)) * a.KV;
    pf_epi_qkv_pair_h(a, kc, vc, t, 4 * p4, s4.x / a.xn[t], s4.y / a.xn[t]);
    pf_epi_qkv_pair_h(a, kc, vc, t, 4 * p4 + 2, s4.z / a.xn[t], s4.w / a.xn[t]);
}

// ---- copies                                                                                                            ------------
// The first n 16-byte words of page src onto page dst in every layer (blockIdx.y) of K (blockIdx.z 0) and V (1), bit for bit: a whole
// page for copy on write, the rows in use for the partial page of llmk_pages_share.  k / v: the pools as 16-byte words, `layer` and
// `page` of them per layer and per page.
__global__ void bd_page_copy_kernel(uint4* __restrict__ k, uint4* __restrict__ v, size_t layer, size_t page, int src, int dst, size_t n) {
    uint4* p = (blockIdx.z ? v : k) + blockIdx.y * layer;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[dst * page + i] = p[src * page + i];
}

// four elements on their way into a pool: f32 as they are, f16 by the stored-value rule (pf_kv_half, as bd_to_half_kernel)
__device__ __forceinline__ void pg_store4(float* dst, const float4& x) { *reinterpret_cast<float4*>(dst) = x; }
__device__ __forceinline__ void pg_store4(_Float16* dst, const float4& x) {
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    *reinterpret_cast<h4*>(dst) = (h4){pf_kv_half(x.x), pf_kv_half(x.y), pf_kv_half(x.z), pf_kv_half(x.w)};
}
// llmk_batch_fork: rows 0 .. n / KV - 1 of the context's f32 caches (layers src_layer elements apart) into the pages of `slot`, every
// layer and K (blockIdx.z 0) and V (1); n elements, a multiple of KV, KV a multiple of 4
template <class T>
__global__ void bd_to_pages_kernel(const float* __restrict__ sk, const float* __restrict__ sv, T* __restrict__ dk, T* __restrict__ dv,
                                   BdPages pg, int slot, size_t n, int KV, size_t src_layer, size_t dst_layer) {
    const float* src = (blockIdx.z ? sv : sk) + blockIdx.y * src_layer;
    T* dst = (blockIdx.z ? dv : dk) + blockIdx.y * dst_layer;
    for (size_t i = 4 * ((size_t)blockIdx.x * blockDim.x + threadIdx.x); i < n; i += 4 * (size_t)gridDim.x * blockDim.x) {
        const int at = pg_row(pg, slot, (int)(i / KV));
        if (at >= 0) pg_store4(dst + (size_t)at * KV + i % KV, *reinterpret_cast<const float4*>(src + i));
    }
}
// llmk_cache_peek: n elements (whole rows) of `slot` from cache row row0 on, out of one layer's pool `src` into the block `dst`, as
// they are stored; a position without a page reads +0.0, as in a fresh slot of a dense batch
template <class T>
__global__ void bd_from_pages_kernel(const T* __restrict__ src, T* __restrict__ dst, BdPages pg, int slot, int row0, size_t n, int KV) {
    typedef T t4 __attribute__((ext_vector_type(4)));
    for (size_t i = 4 * ((size_t)blockIdx.x * blockDim.x + threadIdx.x); i < n; i += 4 * (size_t)gridDim.x * blockDim.x) {
        const int at = pg_row(pg, slot, row0 + (int)(i / KV));
        *reinterpret_cast<t4*>(dst + i) = at >= 0 ? *reinterpret_cast<const t4*>(src + (size_t)at * KV + i % KV) : (t4){0, 0, 0, 0};
    }
}

}  // namespace llmk
