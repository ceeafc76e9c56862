// Decode attention of the context's own sequence, split over the whole chip: attn_split_kernel and
// attn_split_fold_kernel, launched by launch_attn (llmk.hip) in attn_kernel's place for a context whose seq_len attn_kernel's in-LDS
// score row cannot hold, or for any context created under LLMK_ATTN_SPLIT=1.  Nothing here has a term in seq_len: LDS is
// attn_smem(ATS_WAVES, HS), the part states are [n_heads][P][HS + 2] floats, and the grid is fixed at llmk_create -- the position
// arrives in tokpos[1], so a captured graph replays the same two launches at every position.
//
// THE SPLIT.  One workgroup per (kv head, part), grid (n_kv_local, P), P = ats_parts(): as many parts as give every CU one workgroup,
// at most ATS_MAX_PARTS, and no more than leave each wave of a part a tile at the full context.  The nrows = tokpos[1] visible cache
// rows are ceil(nrows / 16) tiles of 16 rows (the last one ragged: its rows from nrows on are masked, their loads clamped to row
// nrows - 1); part p takes tiles [p * tpp, min((p + 1) * tpp, tiles)), tpp = ceil(tiles / P), computed on the device.  A part with no
// tile writes the neutral state {m = -inf, l = 0, o = 0} for its heads and returns; no workgroup waits for another and nothing is
// accumulated with atomics: every state word is written by exactly one thread per launch, and the fold reads them in part order.
//
// INSIDE A PART (attn_tiles.h has the lane arithmetic).  The kv_mul query heads of the kv head are the 16 B columns of
// v_mfma_f32_16x16x4_f32 (padded by repeating the last, as in bd_attn_kernel), so a K tile and a V tile cross L2 ONCE for the whole
// group where attn_kernel reads them once per query head.  Q is loaded once into registers.  The 8 waves take the part's tiles round
// robin; a wave requests its next tile's K and V fragments (HS / 8 loads of 16 bytes per lane at head sizes 64 and 128: 8 KB and
// 16 KB per wave) before it multiplies the current one, so a CU has 64 .. 128 KB on its way at any time -- the bandwidth-delay
// product of HBM over 256 CUs is below 64 KB each.  Scores go through the running softmax per tile (attn_tiles: the rescale is stated
// there, once), the V tile through the second MFMA into o[HS][heads]; the waves' {m, l, o} meet in LDS once, at the end, and are
// merged in wave order (attn_merge_waves).
//
// THE FOLD.  attn_split_fold_kernel, one workgroup per query head: M = max_p m_p, then L = sum_p l_p e^(m_p - M) and
// o = sum_p o_p e^(m_p - M) in part order (a state with m = -inf has the factor 0), and xb = o / L: ONE division, at the end.
//
// NON-FINITE SCORES.  attn_kernel's softmax is e_t = expf(s_t - max_t s_t), p_t = e_t / sum e (fmaxf skips NaN).  Its head output is
// NaN in every element iff some visible score is NaN or +inf, or all of them are -inf; otherwise a -inf score has the weight 0
// exactly.  The same holds here.  NaN: the weight expf(NaN - m) is NaN in the wave that meets it (STRICT: also while that wave has
// seen nothing finite), l becomes NaN and stays NaN through the rescales, and the merges multiply it by a factor -- even 0 -- and add
// it: L is NaN.  +inf: m becomes +inf and the row's own weight expf(inf - inf) is NaN.  All -inf: every state keeps m = -inf, l = 0,
// o = 0 and the fold divides 0 by 0.  A -inf score beside finite ones: weight 0 (it is not exponentiated at all).  As in attn_kernel,
// a weight of 0 times a non-finite V element is NaN.  That reaches the NEWEST row's V too, and is in no contract: the masked rows of the
// ragged last tile load it (the clamp) and weigh it 0, so an infinite element there gives NaN, not +-inf, at every position that is no
// multiple of 16 -- as attn_kernel does at every position that is no multiple of its batch (measured: tests/test_attn_split_op_gpu.py).
// NOT a stand-alone header in spirit: it is prefill.h's MFMA attention pieces (attn_tiles.h) around a split rule and two kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "prefill.h"

namespace llmk {

constexpr int ATS_TILE = 16;          // cache rows per MFMA tile
constexpr int ATS_WAVES = 8;          // waves of a part's workgroup
constexpr int ATS_MAX_PARTS = 64;     // 32 heads x 64 parts x 130 floats: the part states stay at 1 MB
constexpr int ATS_MAX_GROUP = 16;     // query heads per kv head, at most (the B operand's 16 columns)

// parts of a context of seq_len S on n_cu CUs, n_kv_local kv heads on this rank
__host__ __device__ inline int ats_parts(int n_kv_local, int S, int n_cu) {
    const int ntile = (S + ATS_TILE - 1) / ATS_TILE, full = (ntile + ATS_WAVES - 1) / ATS_WAVES;
    int parts = n_cu / n_kv_local;
    parts = parts < full ? parts : full;
    parts = parts < ATS_MAX_PARTS ? parts : ATS_MAX_PARTS;
    return parts < 1 ? 1 : parts;
}
// floats of one (query head, part) state: m, l, o[hs]; state (h, p) of P parts starts at (h * P + p) * ats_state(hs)
__host__ __device__ constexpr size_t ats_state(int hs) { return (size_t)hs + 2; }

template <int HS>
__global__ __launch_bounds__(ATS_WAVES * WAVE) void attn_split_kernel(const float* __restrict__ q, const float* __restrict__ kc,
                                                                      const float* __restrict__ vc, float* __restrict__ ps,
                                                                      const int* __restrict__ tokpos, int KV, int kv_mul) {
    constexpr int DG = HS / 4, NT = HS / 16, NS = (int)ats_state(HS);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 15, g = lane >> 4;
    const int kvh = blockIdx.x, part = blockIdx.y, P = gridDim.y;
    const int nrows = tokpos[1];                      // cache rows 0 .. nrows-1 are visible (this position's own row among them)
    const int ntile = (nrows + ATS_TILE - 1) / ATS_TILE, tpp = (ntile + P - 1) / P;
    const int t0 = part * tpp, t1 = min(t0 + tpp, ntile);
    float* st = ps + ((size_t)kvh * kv_mul * P + part) * NS;      // head kvh * kv_mul + c: st + c * P * NS
    if (t0 >= t1) {                                   // whole workgroup: no barrier is pending
        for (int idx = tid; idx < kv_mul * NS; idx += ATS_WAVES * WAVE)
            st[(size_t)(idx / NS) * P * NS + idx % NS] = idx % NS == 0 ? -INFINITY : 0.f;
        return;
    }
    float qf[DG];
    attn_load_q<HS>(qf, q + (size_t)(kvh * kv_mul + min(li, kv_mul - 1)) * HS + g * DG);
    float m_run, l_run;
    pf_v4f O[NT];
    const auto visible = [&](int r) { return r < nrows; };
    attn_tiles<HS, float, ATS_WAVES, decltype(visible), AttnDense, true>(qf, kc + (size_t)kvh * HS + g * DG, vc + (size_t)kvh * HS + NT * li, KV, nrows - 1,
                                                                         ntile, t0, t1, wid, li, g, visible, m_run, l_run, O);
    attn_merge_waves<HS, ATS_WAVES>(m_run, l_run, O, kv_mul, [&](int c, int d, float M, float L, float val) {
        float* s = st + (size_t)c * P * NS;
        s[2 + d] = val;
        if (d == 0) {
            s[0] = M;
            s[1] = L;
        }
    });
}

// One workgroup per query head.  The head's P states are contiguous: all ATS_FOLD_THREADS threads bring them into LDS with independent
// 8-byte loads first (read one after the other by the thread that needs them they cost P dependent trips to another XCD's writes: a
// floor of 30 us at 64 parts, measured), then thread d < HS folds element d in part order.
constexpr int ATS_FOLD_THREADS = 256;
template <int HS>
__global__ __launch_bounds__(ATS_FOLD_THREADS) void attn_split_fold_kernel(const float* __restrict__ ps, float* __restrict__ xb, int P) {
    constexpr int NS = (int)ats_state(HS);
    static_assert(NS % 2 == 0, "a head's states are whole float2s");
    __shared__ float2 st2[ATS_MAX_PARTS * NS / 2];
    const int h = blockIdx.x, d = threadIdx.x;
    const float2* src = reinterpret_cast<const float2*>(ps + (size_t)h * P * NS);
    for (int i = d; i < P * NS / 2; i += ATS_FOLD_THREADS) st2[i] = src[i];
    __syncthreads();
    if (d >= HS) return;
    const float* st = reinterpret_cast<const float*>(st2);
    float M = -INFINITY;
    for (int p = 0; p < P; ++p) M = fmaxf(M, st[(size_t)p * NS]);
    float L = 0.f, val = 0.f;
    for (int p = 0; p < P; ++p) {
        const float mp = st[(size_t)p * NS];
        const float e = mp == -INFINITY ? 0.f : expf(mp - M);
        L += st[(size_t)p * NS + 1] * e;
        val += st[(size_t)p * NS + 2 + d] * e;
    }
    xb[(size_t)h * HS + d] = val / L;
}

}  // namespace llmk
