// LoRA adapters for the batched decode (llmk_lora_*): every slot of a batch may run the base model plus a low-rank
// correction of its own, y += s . B (A x), in the ONE pass over the base weights.  A q4_0 base cannot be merged with an adapter on the
// host (the sum does not requantise), so the correction is computed beside the quantised GEMM.
//
// Where it goes.  Every base GEMM of pf_layers (llmk.hip) leaves split-K partial tiles P[slot][Tp][rows] and its epilogue adds a strip's
// partials in slot order (prefill.h pf_sum4).  Every strip has a slot 0 (pf_nslots >= 1) and both GEMM kernels -- the f16 and the f32
// instruction -- write it at P[t * rows + r].  The correction is ADDED INTO slot 0 between the GEMM and its epilogue: no existing kernel
// changes, no call kind has code of its own, and what the epilogue does to the sum (the division by xn[t] behind QKV and w1|w3, whose
// input is the un-normalised x * gains) it does to the correction too.  The lowcnt votes are the base GEMM's alone.
//
// Column groups.  The host sorts the pass rows that have an adapter into groups of at most 16 rows of ONE adapter (LoraGroup: the
// adapter's piece table, its scale, 16 pass-row indices padded with -1): the 16 columns of v_mfma_f32_16x16x4_f32, the instruction
// attn_tiles.h uses -- full f32 operands, so the correction is as exact as an f32 dot.  Rows on the base model are in no group: nothing is
// computed for them.  A piece is a row range of a fused tensor with its own A [rank][K] and B [rows][rank] (LoraPiece; q, k and v are
// three pieces of wqkv over the same input); a tensor and layer hold at most LORA_MAX_PIECES of them.  On the device A is [R16][K] and B
// [rows][R16], R16 = the rank rounded up to 16, the padding zero: no kernel tests the rank.
//
// Two launches per tensor and layer, both on the pass's stream behind the base GEMM:
//   lora_shrink_kernel   S = A . X^T.  Grid (K chunk, group, piece), 4 waves.  The output is tiny ([R16][16]) and the reduction is long
//                        (K = E or H), so K is cut into nch <= LORA_MAX_CHUNKS chunks of a multiple of 64 columns (lora_chunk) and the
//                        chunk's 16-column steps are dealt to the four waves.  Lane l holds A[16 t + l%16][k + 4 (l/16) .. +3] of each of
//                        the R16/16 rank tiles t and X[col[l%16]][the same columns] -- gathered by index from the GEMM's own input, a
//                        -1 column is zeros -- and MFMA step j multiplies component j of both (k is a summation index: prefill.h).  One
//                        X fragment feeds every rank tile.  The four waves' accumulators meet in LDS and are added in wave order; the
//                        workgroup leaves the partial S[chunk][group][piece][R16][16].  A and X come straight from global memory: A is
//                        read once per group (rank x K x 4 bytes, 256 KB at rank 16 and K 4096) and X is L2-resident behind the GEMM.
//   lora_expand_kernel   D = s . B . S.  Grid (strip of 256 output rows, group, piece), 4 waves of four 16-row tiles.  The workgroup
//                        folds the chunks' partials of S in chunk order into LDS, times s; a wave multiplies its tiles with the
//                        contraction over R16 (lane l: B[row0 + 16 tile + l%16][16 kb + 4 (l/16) .. +3] against S from LDS).  In the
//                        accumulators lane l holds rows 4 (l/16) .. +3 of column l%16: four consecutive output rows of one pass row,
//                        so the add into P is one 16-byte read-modify-write (row0 and rows are multiples of 4).
// The (pass row, output row) sets of different groups, pieces and strips are disjoint, so neither launch has a race; there is no float
// atomic, and every sum has a fixed order: the same call on the same state gives the same bits.
// Both kernels: no scratch, 4 waves per workgroup, LDS 16 KB / 4 KB (-Rpass-analysis=kernel-resource-usage, recorded in profiles/batch_lora.txt).
// Measured (profiles/batch_lora.txt): 7.5 to 8 us per shrink and 10 to 11 us per expand on Llama-2-7B at rank 16 WHATEVER the rows --
// both are bound by their own latency chains (group -> piece table -> A before the first load, dependent load + MFMA steps, the fold
// of the chunks), not by the bytes they move.  Not done: the pass's pieces by value in the launch arguments, loads issued a step
// ahead, shrink on the second lane's stream beside the base GEMM (both only read the input).
#pragma once
#include <hip/hip_runtime.h>

#include "prefill.h"

namespace llmk {

constexpr int LORA_MAX_RANK = 64;
constexpr int LORA_MAX_PIECES = 4;       // pieces of one tensor and layer (q | k | v, gate | up, and one to spare)
constexpr int LORA_COLS = 16;            // pass rows per column group: the MFMA's columns
constexpr int LORA_MAX_CHUNKS = 16;      // K chunks of the shrink
constexpr int LORA_CHUNK_MIN = 256;      // ... of at least this many columns
constexpr int LORA_WAVES = 4;
constexpr int LORA_STRIP = 256;          // output rows per expand workgroup: four 16-row tiles per wave
constexpr int LORA_S = LORA_MAX_RANK * LORA_COLS;      // floats of one partial S (the stride whatever the rank)
constexpr int LORA_TENSORS = 4;          // wqkv, wo, w13, w2

struct LoraPiece {
    const float* A;      // [R16][K]
    const float* B;      // [rows][R16]
    int row0, rows;      // rows == 0: no piece here
};
struct LoraGroup {
    const LoraPiece* table;      // the adapter's [L][LORA_TENSORS][LORA_MAX_PIECES]
    float scale;
    int r16;
    int col[LORA_COLS];          // pass rows, -1: no column
};

// columns per K chunk (a multiple of 64, as K is) and the chunks that makes
__host__ __device__ inline int lora_chunk(int K) {
    const int n = (K + LORA_CHUNK_MIN - 1) / LORA_CHUNK_MIN, nch = n < LORA_MAX_CHUNKS ? n : LORA_MAX_CHUNKS;
    return ((K + nch - 1) / nch + 63) / 64 * 64;
}
__host__ __device__ inline int lora_nchunks(int K) { return (K + lora_chunk(K) - 1) / lora_chunk(K); }

// X: the GEMM's input [T][K]; Sp: [nch][groups][LORA_MAX_PIECES][LORA_S]; slot = layer * LORA_TENSORS + tensor
__global__ __launch_bounds__(LORA_WAVES * WAVE) void lora_shrink_kernel(const LoraGroup* groups, int slot, const float* X, int K, int kc, float* Sp) {
    __shared__ __attribute__((aligned(16))) float red[LORA_WAVES][LORA_MAX_RANK / 16][4][WAVE];
    const LoraGroup& g = groups[blockIdx.y];
    const LoraPiece pc = g.table[slot * LORA_MAX_PIECES + blockIdx.z];
    if (pc.rows == 0) return;                                  // whole workgroup: no barrier is pending
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, li = lane & 15, lq = lane >> 4;
    const int nt = g.r16 >> 4;
    const int k0 = blockIdx.x * kc, nsteps = (min(kc, K - k0)) >> 4;
    const int col = g.col[li];
    const float* xp = X + (size_t)max(col, 0) * K + k0 + 4 * lq;
    const float* ap = pc.A + (size_t)li * K + k0 + 4 * lq;
    pf_v4f acc[LORA_MAX_RANK / 16];
#pragma unroll
    for (int t = 0; t < LORA_MAX_RANK / 16; ++t) acc[t] = (pf_v4f){0.f, 0.f, 0.f, 0.f};
    for (int s = wid; s < nsteps; s += LORA_WAVES) {
        float4 x = *reinterpret_cast<const float4*>(xp + 16 * s);
        if (col < 0) x = make_float4(0.f, 0.f, 0.f, 0.f);
        const float xv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int t = 0; t < LORA_MAX_RANK / 16; ++t) {
            if (t < nt) {
                const float4 a = *reinterpret_cast<const float4*>(ap + (size_t)16 * t * K + 16 * s);
                const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], xv[j], acc[t], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < LORA_MAX_RANK / 16; ++t)
#pragma unroll
        for (int v = 0; v < 4; ++v) red[wid][t][v][lane] = acc[t][v];
    __syncthreads();
    // D layout: lane l, register v <-> rank 16 t + 4 (l/16) + v, column l%16; the waves' shares add in wave order
    float* out = Sp + (((size_t)blockIdx.x * gridDim.y + blockIdx.y) * LORA_MAX_PIECES + blockIdx.z) * LORA_S;
    for (int i = threadIdx.x; i < nt * 4 * WAVE; i += LORA_WAVES * WAVE) {
        const int t = i >> 8, v = (i >> 6) & 3, l = i & 63;
        float s = red[0][t][v][l];
#pragma unroll
        for (int w = 1; w < LORA_WAVES; ++w) s += red[w][t][v][l];
        out[(16 * t + 4 * (l >> 4) + v) * LORA_COLS + (l & 15)] = s;
    }
}

// P: slot 0 of the GEMM's partial tiles, [Tp][prows]; nch: the shrink's chunks
__global__ __launch_bounds__(LORA_WAVES * WAVE) void lora_expand_kernel(const LoraGroup* groups, int slot, const float* Sp, int nch, float* P, int prows) {
    __shared__ __attribute__((aligned(16))) float S[LORA_S];
    const LoraGroup& g = groups[blockIdx.y];
    const LoraPiece pc = g.table[slot * LORA_MAX_PIECES + blockIdx.z];
    const int r0 = blockIdx.x * LORA_STRIP;
    if (r0 >= pc.rows) return;                                 // (rows == 0 too) whole workgroup
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, li = lane & 15, lq = lane >> 4;
    const int r16 = g.r16;
    const size_t pitch = (size_t)gridDim.y * LORA_MAX_PIECES * LORA_S;
    const float* sp = Sp + ((size_t)blockIdx.y * LORA_MAX_PIECES + blockIdx.z) * LORA_S;
    for (int i = threadIdx.x; i < r16 * LORA_COLS; i += LORA_WAVES * WAVE) {
        float s = 0.f;
        for (int c = 0; c < nch; ++c) s += sp[(size_t)c * pitch + i];      // chunk order
        S[i] = s * g.scale;
    }
    __syncthreads();
    const int col = g.col[li];
#pragma unroll
    for (int tt = 0; tt < LORA_STRIP / 16 / LORA_WAVES; ++tt) {
        const int rt = r0 + (wid * (LORA_STRIP / 16 / LORA_WAVES) + tt) * 16;      // the tile's first row within the piece
        if (rt >= pc.rows) break;                              // wave-uniform
        const float* bp = pc.B + (size_t)min(rt + li, pc.rows - 1) * r16 + 4 * lq;      // (a ragged tile re-reads the last row: its D rows are not stored)
        pf_v4f acc = (pf_v4f){0.f, 0.f, 0.f, 0.f};
        for (int kb = 0; kb < r16; kb += 16) {
            const float4 b = *reinterpret_cast<const float4*>(bp + kb);
            const float bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(bv[j], S[(kb + 4 * lq + j) * LORA_COLS + li], acc, 0, 0, 0);
        }
        // lane l: rows rt + 4 (l/16) .. +3 of pass row col[l%16]
        if (col >= 0 && rt + 4 * lq < pc.rows) {
            pf_v4f* dst = reinterpret_cast<pf_v4f*>(P + (size_t)col * prows + pc.row0 + rt + 4 * lq);
            *dst = *dst + acc;
        }
    }
}

}  // namespace llmk
