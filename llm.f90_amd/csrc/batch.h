// Batched decode (llmk_batch_*): up to PF_TMAX ROWS -- one position each of DIFFERENT sequences -- go through every
// layer together, so the weights cross HBM once per pass instead of once per token per sequence (q6_K classifier rows too, through the
// GEMM of prefill.h; sc_batch runs the decode classifier per row only where llmk.hip sc_plan says so).  The GEMMs, the residual and SwiGLU epilogues and the classifier are the prefill's (prefill.h); what a
// row's POSITION touches is here:
//   row words      {slot, pos} per row (pos 1-based): which of the batch's K/V caches the row lives in, and where
//   bd_epi_qkv     pf_epi_qkv_pair's arithmetic with the position and the cache base taken from the row words
//   bd_attn        decode attention over many caches: one workgroup per (kv head, row, part of the row's timesteps)
//   bd_attn_fold   the parts of a row folded in part order
//   bd_advance     llmk_batch_decode: the picked id becomes the row's next token, its position moves on -- on the device
//   bd_attn_prefix / bd_attn_own   a pass with rows ATTACHED to the batch's shared prefix (llmk_prefix_*, below)
//   bd_attn_span   a pass with SEVERAL consecutive positions of a slot (llmk_span_*, below): (position, query head) pairs as columns
// bd_attn_prefix / bd_attn_own / bd_attn_span are setup around attn_tiles.h's tile loop, wave merge and look-ahead loads (shared with pf_attn_kernel);
// bd_attn keeps the same statements written out (the reason stands at the kernel).
// The caches are [L][n_slots][seq_len][KV], f32 or -- a batch of llmk_cache_create(.., LLMK_TYPE_F16) -- IEEE half, or -- LLMK_TYPE_Q8_0 --
// int8 quants in that order with the f16 scales of their blocks of 32 behind them (the q8_0 sections below).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "prefill.h"

namespace llmk {

constexpr int BD_TILE = 16;          // cache rows per MFMA tile (the A operand's 16 rows)
constexpr int BD_WAVES = 8;          // waves of an attention workgroup: tiles of a part go round robin
constexpr int BD_MAX_PARTS = 8;      // workgroups a row's timesteps are split over, at most
constexpr int BD_MAX_GROUP = 16;     // query heads per kv head, at most (the B operand's 16 columns)

// The split rule.  A pass has n * n_kv_heads (row, kv head) pairs; with fewer of them than CUs a row's tiles are split over `parts`
// workgroups, as long as every part still has a tile for each of its waves.  tiles per part (tpp) is ONE value for the pass, from its
// longest row: part p of a row of `pos` timesteps takes tiles [p * tpp, min((p + 1) * tpp, ceil(pos / BD_TILE))) -- possibly none.
__host__ __device__ inline int bd_parts(int n, int n_kv_heads, int max_pos, int n_cu) {
    const int ntile = (max_pos + BD_TILE - 1) / BD_TILE;
    int parts = n_cu / (n * n_kv_heads);
    parts = parts < (ntile + BD_WAVES - 1) / BD_WAVES ? parts : (ntile + BD_WAVES - 1) / BD_WAVES;
    parts = parts < BD_MAX_PARTS ? parts : BD_MAX_PARTS;
    return parts < 1 ? 1 : parts;
}
__host__ __device__ inline int bd_tiles_per_part(int max_pos, int parts) {
    const int ntile = (max_pos + BD_TILE - 1) / BD_TILE;
    return (ntile + parts - 1) / parts;
}

struct BdRow { int slot, pos; };      // pos 1-based; {slot, pos} is read as tokpos[1] = pos by the sampler kernels
static_assert(sizeof(BdRow) == 2 * sizeof(int) && offsetof(BdRow, pos) == sizeof(int), "the sampler kernels read a row's words as int tokpos[2]");

// where the rows live: a layer's caches are kc + slot * slot_stride, seq_len rows of KV floats each
struct BdCaches {
    const BdRow* rows;
    size_t slot_stride;      // seq_len * KV
    int n_slots, seq_len;
};
__device__ __forceinline__ bool bd_row_ok(const BdCaches& bc, const BdRow& r) {
    return (unsigned)r.slot < (unsigned)bc.n_slots && r.pos >= 1 && r.pos <= bc.seq_len;
}

// RoPE + K/V write of pf_epi_qkv_kernel; row t's position and cache come from its row words.  The arithmetic IS pf_epi_qkv_pair:
// it is handed the same arguments with pos0 + t = the row's position and the slot's caches.
__global__ void bd_epi_qkv_kernel(PfEpiArgs a, BdCaches bc) {
    const int p4 = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    pf_low_check(a, blockIdx.x == 0 && blockIdx.y == 0);
    if (p4 >= a.rows / 4) return;
    const BdRow r = bc.rows[t];
    if (!bd_row_ok(bc, r)) return;       // (the host checks every row before a pass; a decode cannot run past seq_len)
    const float4 s4 = pf_sum4(a, t, 4 * p4);
    a.pos0 = r.pos - t;
    a.kc += (size_t)r.slot * bc.slot_stride;
    a.vc += (size_t)r.slot * bc.slot_stride;
    pf_epi_qkv_pair(a, t, 4 * p4, s4.x / a.xn[t], s4.y / a.xn[t]);
    pf_epi_qkv_pair(a, t, 4 * p4 + 2, s4.z / a.xn[t], s4.w / a.xn[t]);
}
// The same for a batch with f16 caches (llmk_cache_create): the layer's caches are kc / vc (a.kc, a.vc are not read), Q still goes out
// in f32, and a K / V element is stored as pf_kv_half of the value the kernel above stores (pf_epi_qkv_pair_h: the same expressions up
// to the store).
__global__ void bd_epi_qkv_h_kernel(PfEpiArgs a, BdCaches bc, _Float16* __restrict__ kc, _Float16* __restrict__ vc) {
    const int p4 = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    pf_low_check(a, blockIdx.x == 0 && blockIdx.y == 0);
    if (p4 >= a.rows / 4) return;
    const BdRow r = bc.rows[t];
    if (!bd_row_ok(bc, r)) return;
    const float4 s4 = pf_sum4(a, t, 4 * p4);
    a.pos0 = r.pos - t;
    kc += (size_t)r.slot * bc.slot_stride;
    vc += (size_t)r.slot * bc.slot_stride;
    pf_epi_qkv_pair_h(a, kc, vc, t, 4 * p4, s4.x / a.xn[t], s4.y / a.xn[t]);
    pf_epi_qkv_pair_h(a, kc, vc, t, 4 * p4 + 2, s4.z / a.xn[t], s4.w / a.xn[t]);
}

// f32 rows of the context's cache into an f16 batch (llmk_batch_fork, llmk_prefix_set): n elements (a multiple of 4) of every layer
// and of K (blockIdx.z 0) and V (1), element i of layer l from src[l * src_layer + i] to dst[l * dst_layer + i], as pf_kv_half.
__global__ void bd_to_half_kernel(const float* __restrict__ sk, const float* __restrict__ sv, _Float16* __restrict__ dk,
                                  _Float16* __restrict__ dv, size_t n, size_t src_layer, size_t dst_layer) {
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    const float* src = (blockIdx.z ? sv : sk) + blockIdx.y * src_layer;
    _Float16* dst = (blockIdx.z ? dv : dk) + blockIdx.y * dst_layer;
    for (size_t i = 4 * ((size_t)blockIdx.x * blockDim.x + threadIdx.x); i < n; i += 4 * (size_t)gridDim.x * blockDim.x) {
        const float4 x = *reinterpret_cast<const float4*>(src + i);
        *reinterpret_cast<h4*>(dst + i) = (h4){pf_kv_half(x.x), pf_kv_half(x.y), pf_kv_half(x.z), pf_kv_half(x.w)};
    }
}

// ---- q8_0 caches (llmk_cache_create(.., LLMK_TYPE_Q8_0); layout: attn_tiles.h Q8Rows)                                 ------------
// THE stored-value rule (include/llmk.h), for the K/V write and the converting copy alike.  EIGHT ADJACENT LANES, the first at a
// multiple of 8 in its wave, hold a block's 32 values, four each in element order; every lane of the eight must call (three xor
// shuffles inside the group).  Leaves this lane's four quants packed in element order and the block's scale (the same in all eight).
//   c = clamp(x, +-65504); amax = max |c|; d32 = amax / 127; d = RNE_f16(d32); id = d32 != 0 ? 1 / d32 : 0 (from d32, as ggml's
//   quantize_row_q8_0_ref); q = clamp(roundf(c * id), +-127); d == 0 (amax below the f16 subnormals: id may be infinite): every q = 0;
//   a NaN among the 32: d = NaN, every q = 0.
// Every product and quotient is one IEEE f32 operation (no fast-math in this build; nothing here can be contracted).
__device__ __forceinline__ void bd_q8_block(const float (&x)[4], unsigned& quants, _Float16& scale) {
#pragma clang fp contract(off)
    float c[4], amax = 0.f;
    int nan = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        nan |= x[i] != x[i];
        c[i] = fminf(fmaxf(x[i], -65504.f), 65504.f);
        amax = fmaxf(amax, fabsf(c[i]));
    }
#pragma unroll
    for (int s = 1; s < 8; s <<= 1) {
        amax = fmaxf(amax, __shfl_xor(amax, s, 64));
        nan |= __shfl_xor(nan, s, 64);
    }
    const float d32 = amax / 127.0f;
    const _Float16 d = (_Float16)d32;
    const float id = d32 != 0.f ? 1.0f / d32 : 0.f;
    const bool zero = nan || (float)d == 0.f;
    quants = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = zero ? 0 : (int)fminf(fmaxf(roundf(c[i] * id), -127.f), 127.f);
        quants |= (unsigned)(q & 0xFF) << (8 * i);
    }
    scale = nan ? (_Float16)__builtin_nanf("") : d;
}

// bd_epi_qkv_h_kernel for a batch with q8_0 caches: Q goes out in f32, a K / V block is stored by the rule above from the values the
// f32 kernel stores (the expressions of pf_epi_qkv_pair_h up to the store: keep them in step).  A thread owns rows 4 * p4 .. + 3 (two
// RoPE pairs), so a block of 32 K or V elements is 8 adjacent threads: Q starts at row 0, K at E and V at E + KV, all multiples of 32
// (E % 64 == 0: pf_shape_ok; KV % 32 == 0: llmk_cache_create), and a workgroup starts at a multiple of 4 * 256 rows -- a block never
// straddles Q | K | V, a wave or the end of the rows (rows / 4 is a multiple of 8).  NO LANE RETURNS in front of bd_q8_block: a lane
// beyond the rows, or of a bad row (uniform: the row is the workgroup's), computes on zeros and stores nothing, so the shuffles run
// with the whole wave active.
__global__ void bd_epi_qkv_q8_kernel(PfEpiArgs a, BdCaches bc, Q8Rows kc, Q8Rows vc) {
    const int p4 = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y, r0 = 4 * p4;
    pf_low_check(a, blockIdx.x == 0 && blockIdx.y == 0);
    const BdRow r = bc.rows[t];
    const bool live = p4 < a.rows / 4 && bd_row_ok(bc, r);
    float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) s4 = pf_sum4(a, t, r0);
    const float xn = a.xn[t];
    float x[4] = {s4.x / xn, s4.y / xn, s4.z / xn, s4.w / xn};
    const int i0 = r0 < a.E ? r0 : r0 < a.E + a.KV ? r0 - a.E : r0 - a.E - a.KV;      // the element in Q, K or V
    if (live && r0 < a.E + a.KV) {
#pragma unroll
        for (int k = 0; k < 4; k += 2) {
            const float rval = (float)r.pos * a.rope[((i0 + k) % a.hs) >> 1];
            const float fcr = cosf(rval), fci = sinf(rval);
            {
#pragma clang fp contract(off)
                const float p00 = x[k] * fcr, p11 = x[k + 1] * fci, p01 = x[k] * fci, p10 = x[k + 1] * fcr;
                x[k] = p00 - p11;
                x[k + 1] = p01 + p10;
            }
        }
    }
    unsigned quants;
    _Float16 scale;
    bd_q8_block(x, quants, scale);
    if (!live) return;
    if (r0 < a.E) {
        *reinterpret_cast<float4*>(a.out + (size_t)t * a.E + i0) = make_float4(x[0], x[1], x[2], x[3]);
        return;
    }
    const Q8Rows dst = attn_at(r0 < a.E + a.KV ? kc : vc, (size_t)r.slot * bc.slot_stride + (size_t)(r.pos - 1) * a.KV + (i0 & ~31));
    *reinterpret_cast<unsigned*>(dst.q + (i0 & 31)) = quants;
    if ((i0 & 31) == 0) *dst.d = scale;
}

// f32 rows of the context's cache into a q8_0 batch (llmk_batch_fork, llmk_prefix_set), bd_to_half_kernel's arguments: n elements (a
// multiple of 32: whole rows) of every layer and of K (blockIdx.z 0) and V (1), by the same rule.  The loop's bound is the
// WORKGROUP's, so every lane of a wave runs every trip and the shuffles meet the whole wave; a lane beyond n converts zeros and
// stores nothing (n % 32 == 0: the eight lanes of a block are beyond n together).
__global__ void bd_to_q8_kernel(const float* __restrict__ sk, const float* __restrict__ sv, Q8Rows dk, Q8Rows dv, size_t n,
                                size_t src_layer, size_t dst_layer) {
    const float* src = (blockIdx.z ? sv : sk) + blockIdx.y * src_layer;
    const Q8Rows dst = attn_at(blockIdx.z ? dv : dk, blockIdx.y * dst_layer);
    for (size_t i0 = 4 * (size_t)blockIdx.x * blockDim.x; i0 < n; i0 += 4 * (size_t)gridDim.x * blockDim.x) {
        const size_t i = i0 + 4 * threadIdx.x;
        const bool live = i < n;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) v = *reinterpret_cast<const float4*>(src + i);
        const float x[4] = {v.x, v.y, v.z, v.w};
        unsigned quants;
        _Float16 scale;
        bd_q8_block(x, quants, scale);
        if (live) {
            *reinterpret_cast<unsigned*>(dst.q + i) = quants;
            if ((i & 31) == 0) dst.d[i >> 5] = scale;
        }
    }
}

// ---- decode attention over many caches                                                      llama2.f90:572-598 ------------
// pf_attn_kernel's layout with the 16 MFMA query columns holding the kv_mul QUERY HEADS OF ONE KV GROUP (padded by repeating the
// last) instead of 16 prompt positions: row b's K/V rows 0 .. pos_b-1 of slot_b cross L2 once for the whole group.  One workgroup
// per (kv head, row, part); its 8 waves take the part's 16-row tiles round robin, each with a running softmax, and merge through LDS.
// parts == 1: the normalised output goes to `out`.  Otherwise the part leaves its state -- the maximum M, the sum L and the
// unnormalised output relative to M, per query head -- in po / pml, and bd_attn_fold_kernel folds a row's parts in part order.
// An empty part (a short row next to a long one) leaves M = -inf, L = 0.
// T: the caches' element type, float or _Float16.
// THE ONE KERNEL THAT DOES NOT CALL attn_tiles.h's attn_tiles / attn_merge_waves: the statements below are those functions', written
// out (only the look-ahead types are shared).  On the shared text the f32 instantiation at head size 64 had the same registers and
// one instruction fewer, but another order of the look-ahead loads among the MFMAs, and the unshared pass measured 0.9 % slower at
// position 1,024 (profiles/attn_tiles_ab.txt); every smaller step towards the shared text -- the Q loader, the f32 load, the take,
// the merge, each alone -- moved the schedule of some instantiation too.  As it stands all eight instantiations compile to the
// instructions they had before attn_tiles.h.  A change to the attention arithmetic is made there AND here; tests/test_build_cpu.py
// holds this to the one exception.
template <int HS, class T = float>
__global__ __launch_bounds__(BD_WAVES * WAVE) void bd_attn_kernel(const float* __restrict__ Q, const T* __restrict__ kc,
                                                                  const T* __restrict__ vc, float* __restrict__ out,
                                                                  float* __restrict__ po, float2* __restrict__ pml, BdCaches bc,
                                                                  int KV, int kv_mul, int E, int tpp) {
    constexpr int DG = HS / 4, NT = HS / 16, NW = BD_WAVES;
    extern __shared__ __attribute__((aligned(16))) char pf_smem[];
    float* so = reinterpret_cast<float*>(pf_smem);   // [NW][16][HS]
    float* sm = so + NW * 16 * HS;                    // [NW][16]
    float* sl = sm + NW * 16;                         // [NW][16]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 15, g = lane >> 4;
    const int kvh = blockIdx.x, b = blockIdx.y, part = blockIdx.z, parts = gridDim.z, nkv = gridDim.x;
    const BdRow row = bc.rows[b];
    if (!bd_row_ok(bc, row)) return;                  // whole workgroup: no barrier is pending
    const int nrows = row.pos;                        // cache rows 0 .. nrows-1 are visible
    const int h = kvh * kv_mul + min(li, kv_mul - 1); // this lane's query head
    const float scale = sqrtf((float)HS);
    float qf[DG];
    {
        const float* qp = Q + (size_t)b * E + (size_t)h * HS + g * DG;
#pragma unroll
        for (int m = 0; m < DG; m += 4) {
            const float4 v = *reinterpret_cast<const float4*>(qp + m);
            qf[m] = v.x; qf[m + 1] = v.y; qf[m + 2] = v.z; qf[m + 3] = v.w;
        }
    }
    float m_run = -INFINITY, l_run = 0.f;
    pf_v4f O[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) O[t] = (pf_v4f){0.f, 0.f, 0.f, 0.f};
    const T* kb = kc + (size_t)row.slot * bc.slot_stride + (size_t)kvh * HS + g * DG;
    const T* vb = vc + (size_t)row.slot * bc.slot_stride + (size_t)kvh * HS + NT * li;
    const int ntile = (nrows + BD_TILE - 1) / BD_TILE;
    const int t0 = part * tpp, t1 = min(t0 + tpp, ntile);
    // K / V fragments of a tile are requested one tile ahead (unconditional loads of a clamped row index)
    typename AttnAhead<HS, T>::K kn;
    typename AttnAhead<HS, T>::V vn;
#define BD_ATT_LOAD(R0_)                                                                                      \
    do {                                                                                                      \
        if constexpr (std::is_same_v<T, float>) {                                                             \
            const float* kp_ = kb + (size_t)min((R0_) + li, nrows - 1) * KV;                                  \
            _Pragma("unroll") for (int m = 0; m < DG; m += 4) {                                               \
                const float4 v_ = *reinterpret_cast<const float4*>(kp_ + m);                                  \
                kn[m] = v_.x; kn[m + 1] = v_.y; kn[m + 2] = v_.z; kn[m + 3] = v_.w;                           \
            }                                                                                                 \
            _Pragma("unroll") for (int v = 0; v < 4; ++v) {                                                   \
                const float* vp_ = vb + (size_t)min((R0_) + 4 * g + v, nrows - 1) * KV;                       \
                if constexpr (NT % 4 == 0) {                                                                  \
                    _Pragma("unroll") for (int t = 0; t < NT; t += 4) {                                       \
                        const float4 x_ = *reinterpret_cast<const float4*>(vp_ + t);                          \
                        vn[v][t] = x_.x; vn[v][t + 1] = x_.y; vn[v][t + 2] = x_.z; vn[v][t + 3] = x_.w;       \
                    }                                                                                         \
                } else if constexpr (NT == 2) {                                                               \
                    const float2 x_ = *reinterpret_cast<const float2*>(vp_);                                  \
                    vn[v][0] = x_.x; vn[v][1] = x_.y;                                                         \
                } else {                                                                                      \
                    vn[v][0] = vp_[0];                                                                        \
                }                                                                                             \
            }                                                                                                 \
        } else {                                                                                              \
            AttnAhead<HS, _Float16>::load(kn, vn, kb, vb, KV, (R0_), li, g, nrows - 1);                               \
        }                                                                                                     \
    } while (0)
    BD_ATT_LOAD(min(t0 + wid, ntile - 1) * BD_TILE);
    for (int kt = t0 + wid; kt < t1; kt += NW) {
        const int r0 = kt * BD_TILE;
        float kf[DG], vf[4][NT];
        if constexpr (std::is_same_v<T, float>) {
#pragma unroll
            for (int m = 0; m < DG; ++m) kf[m] = kn[m];
#pragma unroll
            for (int v = 0; v < 4; ++v)
#pragma unroll
                for (int t = 0; t < NT; ++t) vf[v][t] = vn[v][t];
        } else {
            AttnAhead<HS, _Float16>::take(kn, vn, kf, vf);
        }
        BD_ATT_LOAD(min(kt + NW, ntile - 1) * BD_TILE);
        pf_v4f acc = (pf_v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < DG; ++m) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[m], qf[m], acc, 0, 0, 0);
        float sc[4], mx = -INFINITY;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const bool vis = r0 + 4 * g + v < nrows;
            sc[v] = vis ? acc[v] / scale : -INFINITY;
            mx = fmaxf(mx, sc[v]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const bool any = m_new != -INFINITY;
        const float alpha = !any ? 1.f : (m_run == -INFINITY ? 0.f : expf(m_run - m_new));
        float p[4], rs = 0.f;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            p[v] = (any && sc[v] != -INFINITY) ? expf(sc[v] - m_new) : 0.f;
            rs += p[v];
        }
        rs += __shfl_xor(rs, 16, 64);
        rs += __shfl_xor(rs, 32, 64);
        l_run = l_run * alpha + rs;
        m_run = m_new;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float ar = __shfl(alpha, 4 * g + r, 64);                     // O rows are query heads 4g+r
#pragma unroll
            for (int t = 0; t < NT; ++t) O[t][r] *= ar;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int v = 0; v < 4; ++v) O[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[v], vf[v][t], O[t], 0, 0, 0);
    }
#undef BD_ATT_LOAD
    if (g == 0) {
        sm[wid * 16 + li] = m_run;
        sl[wid * 16 + li] = l_run;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int t = 0; t < NT; ++t) so[(size_t)(wid * 16 + 4 * g + r) * HS + NT * li + t] = O[t][r];
    __syncthreads();
    const size_t pbase = ((size_t)b * nkv + kvh) * parts + part;      // this part's state: po [.][BD_MAX_GROUP][HS], pml [.][BD_MAX_GROUP]
    for (int idx = tid; idx < kv_mul * HS; idx += NW * WAVE) {
        const int q = idx / HS, d = idx % HS;
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < NW; ++w) M = fmaxf(M, sm[w * 16 + q]);
        float L = 0.f, val = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float mw = sm[w * 16 + q];
            const float e = mw == -INFINITY ? 0.f : expf(mw - M);
            L += sl[w * 16 + q] * e;
            val += so[(size_t)(w * 16 + q) * HS + d] * e;
        }
        if (parts == 1) {
            out[(size_t)b * E + (size_t)(kvh * kv_mul + q) * HS + d] = val / L;
        } else {
            po[(pbase * BD_MAX_GROUP + q) * HS + d] = val;
            if (d == 0) pml[pbase * BD_MAX_GROUP + q] = make_float2(M, L);
        }
    }
}

// ---- a shared prefix (llmk_prefix_*)                                                                                  ------------
// A batch can hold ONE copy of the K/V rows of positions 1..P, [L][P][KV]; an ATTACHED slot's sequence is those rows and then its own
// cache rows P .. pos-1 (still indexed by absolute position).  A pass with at least one attached row runs three kernels per layer
// instead of bd_attn_kernel (+ fold); a pass with none runs exactly what it ran before.
//   bd_attn_prefix_kernel  the prefix rows against the query heads of up to RG attached rows at once: one read per column group
//   bd_attn_own_kernel     bd_attn_kernel over a row's OWN rows first[slot] .. pos-1 (first = P attached, 0 not), never normalising
//   bd_attn_fold_kernel    a (row, kv head)'s prefix parts in part order, then its own parts in part order
// Part states in such a pass: np = prefix parts + own parts per (row, kv head), kv_mul query heads each (NOT padded to BD_MAX_GROUP:
// the buffers hold LLMK_MAX_BATCH rows); state s of (b, kvh), head q: pml[((b * nkv + kvh) * np + s) * kv_mul + q], po that * HS.

// rows per column group: the 16 MFMA columns hold (row, query head) pairs of one kv head
__host__ __device__ inline int bd_prefix_rg(int kv_mul) { return BD_MAX_GROUP / kv_mul < 1 ? 1 : BD_MAX_GROUP / kv_mul; }
__host__ __device__ inline int bd_prefix_groups(int n_att, int kv_mul) { return (n_att + bd_prefix_rg(kv_mul) - 1) / bd_prefix_rg(kv_mul); }
// The prefix's split rule: bd_parts with the column groups of the attached rows in the place of the rows and P in the place of the
// longest row.  Tiles per part: bd_tiles_per_part(P, parts).
__host__ __device__ inline int bd_prefix_parts(int n_att, int n_kv_heads, int kv_mul, int P, int n_cu) {
    return bd_parts(bd_prefix_groups(n_att, kv_mul), n_kv_heads, P, n_cu);
}

// One workgroup per (kv head, column group, prefix part).  colmap [groups][RG]: the pass's attached rows, in row order, -1 behind the
// last.  Column c of a group is (row colmap[c / kv_mul], query head c % kv_mul of the kv head); columns from the last live one on
// repeat it and are not written out.  Every attached row sees the whole prefix: the predicate is cache row < P alone.
// (the kernels' text is a __device__ function over the cache type T and its view AttnAhead<HS, T>::Ptr, so that the q8_0 kernels below
// -- __global__ names of their own -- are the same statements)
template <int HS, class T>
__device__ __forceinline__ void bd_attn_prefix_body(const float* __restrict__ Q, typename AttnAhead<HS, T>::Ptr pk, typename AttnAhead<HS, T>::Ptr pv,
                                                    float* __restrict__ po, float2* __restrict__ pml, const int* __restrict__ colmap, int n,
                                                    int P, int KV, int kv_mul, int E, int tpp, int np) {
    constexpr int DG = HS / 4, NT = HS / 16;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 15, g = lane >> 4;
    const int kvh = blockIdx.x, part = blockIdx.z, nkv = gridDim.x, rg = bd_prefix_rg(kv_mul);
    const int* cm = colmap + blockIdx.y * rg;
    int nr = 0;
    while (nr < rg && (unsigned)cm[nr] < (unsigned)n) ++nr;
    if (nr == 0 || P < 1) return;                     // whole workgroup: no barrier is pending
    const int live = nr * kv_mul, c = min(li, live - 1);
    float qf[DG];
    attn_load_q<HS>(qf, Q + (size_t)cm[c / kv_mul] * E + (size_t)(kvh * kv_mul + c % kv_mul) * HS + g * DG);
    float m_run, l_run;
    pf_v4f O[NT];
    const int ntile = (P + BD_TILE - 1) / BD_TILE, t0 = part * tpp, t1 = min(t0 + tpp, ntile);
    attn_tiles<HS, T, BD_WAVES>(qf, attn_at(pk, (size_t)kvh * HS + g * DG), attn_at(pv, (size_t)kvh * HS + NT * li), KV, P - 1, ntile, t0, t1, wid, li, g,
                                [&](int r) { return r < P; }, m_run, l_run, O);
    attn_merge_waves<HS, BD_WAVES>(m_run, l_run, O, live, [&](int col, int d, float M, float L, float val) {
        const size_t s = (((size_t)cm[col / kv_mul] * nkv + kvh) * np + part) * kv_mul + col % kv_mul;
        po[s * HS + d] = val;
        if (d == 0) pml[s] = make_float2(M, L);
    });
}
template <int HS, class T = float>
__global__ __launch_bounds__(BD_WAVES * WAVE) void bd_attn_prefix_kernel(const float* __restrict__ Q, const T* __restrict__ pk,
                                                                         const T* __restrict__ pv, float* __restrict__ po,
                                                                         float2* __restrict__ pml, const int* __restrict__ colmap, int n,
                                                                         int P, int KV, int kv_mul, int E, int tpp, int np) {
    bd_attn_prefix_body<HS, T>(Q, pk, pv, po, pml, colmap, n, P, KV, kv_mul, E, tpp, np);
}

// bd_attn_kernel for a pass with attached rows: the row's own cache rows first[slot] .. pos-1, tiles counted from the one that holds
// row `first` (that tile masks the rows below it); part `part` leaves state p0 + part, never normalised.  One workgroup per (kv head,
// row, own part).
template <int HS, class T>
__device__ __forceinline__ void bd_attn_own_body(const float* __restrict__ Q, typename AttnAhead<HS, T>::Ptr kc, typename AttnAhead<HS, T>::Ptr vc,
                                                 float* __restrict__ po, float2* __restrict__ pml, const BdCaches& bc, const int* __restrict__ first,
                                                 int KV, int kv_mul, int E, int tpp, int np, int p0) {
    constexpr int DG = HS / 4, NT = HS / 16;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 15, g = lane >> 4;
    const int kvh = blockIdx.x, b = blockIdx.y, part = blockIdx.z, nkv = gridDim.x;
    const BdRow row = bc.rows[b];
    if (!bd_row_ok(bc, row)) return;                  // whole workgroup: no barrier is pending
    const int lo = first[row.slot], nrows = row.pos;  // (the host refuses an attached row at pos <= P)
    const int h = kvh * kv_mul + min(li, kv_mul - 1);
    float qf[DG];
    attn_load_q<HS>(qf, Q + (size_t)b * E + (size_t)h * HS + g * DG);
    float m_run, l_run;
    pf_v4f O[NT];
    const int ntile = (nrows + BD_TILE - 1) / BD_TILE, t0 = lo / BD_TILE + part * tpp, t1 = min(t0 + tpp, ntile);
    const size_t base = (size_t)row.slot * bc.slot_stride + (size_t)kvh * HS;
    attn_tiles<HS, T, BD_WAVES>(qf, attn_at(kc, base + g * DG), attn_at(vc, base + NT * li), KV, nrows - 1, ntile, t0, t1, wid, li, g,
                                [&](int r) { return lo <= r && r < nrows; }, m_run, l_run, O);
    attn_merge_waves<HS, BD_WAVES>(m_run, l_run, O, kv_mul, [&](int q, int d, float M, float L, float val) {
        const size_t s = (((size_t)b * nkv + kvh) * np + p0 + part) * kv_mul + q;
        po[s * HS + d] = val;
        if (d == 0) pml[s] = make_float2(M, L);
    });
}
template <int HS, class T = float>
__global__ __launch_bounds__(BD_WAVES * WAVE) void bd_attn_own_kernel(const float* __restrict__ Q, const T* __restrict__ kc,
                                                                      const T* __restrict__ vc, float* __restrict__ po,
                                                                      float2* __restrict__ pml, BdCaches bc, const int* __restrict__ first,
                                                                      int KV, int kv_mul, int E, int tpp, int np, int p0) {
    bd_attn_own_body<HS, T>(Q, kc, vc, po, pml, bc, first, KV, kv_mul, E, tpp, np, p0);
}

// ---- spans (llmk_span_*): several consecutive positions of a slot in one pass                                         ------------
// The rows of a span pass are cut into COLUMN GROUPS of up to bd_prefix_rg(kv_mul) consecutive rows of one span (so of one slot, at
// consecutive positions); the last group of a span may be shorter.  bd_attn_span_kernel is bd_attn_prefix_kernel's layout over the
// slot's OWN cache: column c of a group is (row first + c / kv_mul, query head c % kv_mul of the kv head), columns from the last live
// one on repeat it and are not written out, and the slot's K/V rows cross L2 once per group instead of once per row.  What is new is
// the CAUSAL edge per column: the lane of column c sees cache row r iff lo <= r < pos(c's row), lo = first[slot] (P attached, 0 not).
// bd_epi_qkv_kernel has written every row's K/V before this kernel runs, so the rows of the same pass at columns <= c are in the
// cache and the predicate alone keeps the later ones out.
struct BdGroup { int first, rows; };      // rows first .. first+rows-1 of the pass
// groups a span of `len` rows is cut into
__host__ __device__ inline int bd_span_groups(int len, int kv_mul) { return bd_prefix_groups(len, kv_mul); }
// A group's tiles are [lo / BD_TILE, ceil(pos of its last row / BD_TILE)).  The split rule is ONE for the pass: bd_parts with the groups
// in the place of the rows and the longest group's tile count (own_tiles) in the place of the longest row; part p of a group takes
// tiles lo / BD_TILE + [p * tpp, (p + 1) * tpp), cut at the group's last tile -- possibly none.
__host__ __device__ inline int bd_span_parts(int groups, int n_kv_heads, int own_tiles, int n_cu) {
    return bd_parts(groups, n_kv_heads, own_tiles * BD_TILE, n_cu);
}
// One workgroup per (kv head, group, part).  direct (one part and no attached row in the pass): the normalised output goes to `out`.
// Otherwise part `part` leaves state p0 + part of every (row, kv head) of the group in the layout of a pass with attached rows
// (stride kv_mul, np states), and bd_attn_fold_kernel folds them.  A column all of whose rows lie before the part's tiles leaves
// M = -inf, L = 0; the part that holds row lo is never empty for any column (pos > lo).
template <int HS, class T>
__device__ __forceinline__ void bd_attn_span_body(const float* __restrict__ Q, typename AttnAhead<HS, T>::Ptr kc, typename AttnAhead<HS, T>::Ptr vc,
                                                  float* __restrict__ out, float* __restrict__ po, float2* __restrict__ pml, const BdCaches& bc,
                                                  const BdGroup* __restrict__ groups, const int* __restrict__ first, int n, int KV, int kv_mul,
                                                  int E, int tpp, int np, int p0, int direct) {
    constexpr int DG = HS / 4, NT = HS / 16;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 15, g = lane >> 4;
    const int kvh = blockIdx.x, part = blockIdx.z, nkv = gridDim.x;
    const BdGroup gr = groups[blockIdx.y];
    if (gr.first < 0 || gr.rows < 1 || gr.rows > bd_prefix_rg(kv_mul) || gr.rows > n - gr.first) return;      // whole workgroup: no barrier is pending
    const BdRow row0 = bc.rows[gr.first], rowl = bc.rows[gr.first + gr.rows - 1];
    if (!bd_row_ok(bc, row0) || !bd_row_ok(bc, rowl) || rowl.slot != row0.slot || rowl.pos != row0.pos + gr.rows - 1) return;
    const int lo = first ? first[row0.slot] : 0;      // (the host refuses an attached row at pos <= P)
    const int live = gr.rows * kv_mul, c = min(li, live - 1);
    const int vis = row0.pos + c / kv_mul;            // this lane's column sees cache rows lo .. vis-1
    float qf[DG];
    attn_load_q<HS>(qf, Q + (size_t)(gr.first + c / kv_mul) * E + (size_t)(kvh * kv_mul + c % kv_mul) * HS + g * DG);
    float m_run, l_run;
    pf_v4f O[NT];
    const int ntile = (rowl.pos + BD_TILE - 1) / BD_TILE, t0 = lo / BD_TILE + part * tpp, t1 = min(t0 + tpp, ntile);
    const size_t base = (size_t)row0.slot * bc.slot_stride + (size_t)kvh * HS;
    attn_tiles<HS, T, BD_WAVES>(qf, attn_at(kc, base + g * DG), attn_at(vc, base + NT * li), KV, rowl.pos - 1, ntile, t0, t1, wid, li, g,
                                [&](int r) { return lo <= r && r < vis; }, m_run, l_run, O);
    attn_merge_waves<HS, BD_WAVES>(m_run, l_run, O, live, [&](int col, int d, float M, float L, float val) {
        const int b = gr.first + col / kv_mul, q = col % kv_mul;
        if (direct) {
            out[(size_t)b * E + (size_t)(kvh * kv_mul + q) * HS + d] = val / L;
        } else {
            const size_t s = (((size_t)b * nkv + kvh) * np + p0 + part) * kv_mul + q;
            po[s * HS + d] = val;
            if (d == 0) pml[s] = make_float2(M, L);
        }
    });
}
template <int HS, class T = float>
__global__ __launch_bounds__(BD_WAVES * WAVE) void bd_attn_span_kernel(const float* __restrict__ Q, const T* __restrict__ kc,
                                                                       const T* __restrict__ vc, float* __restrict__ out,
                                                                       float* __restrict__ po, float2* __restrict__ pml, BdCaches bc,
                                                                       const BdGroup* __restrict__ groups, const int* __restrict__ first,
                                                                       int n, int KV, int kv_mul, int E, int tpp, int np, int p0, int direct) {
    bd_attn_span_body<HS, T>(Q, kc, vc, out, po, pml, bc, groups, first, n, KV, kv_mul, E, tpp, np, p0, direct);
}

// The part states of (row, kv head) folded in part order: out = sum_p O_p e^(M_p - M) / sum_p L_p e^(M_p - M).  State s of np, head q,
// is pml[((b * nkv + kvh) * np + s) * stride + q], po that * HS.
//   a pass without attached rows (launched only when it has more than one part): stride BD_MAX_GROUP, p0 = 0, first = null: parts
//       0 .. np-1; part 0 is never empty;
//   a pass with attached rows: stride kv_mul; the prefix parts 0 .. p0-1 -- an unattached row (first[slot] == 0) has none: nothing
//       wrote them, they are skipped, which is what folding M = -inf, L = 0 does -- then the own parts p0 .. np-1.  The row's last
//       own row is always visible;
//   a span pass (bd_attn_span_kernel; launched unless it ran one part with no attached row): stride kv_mul; p0 = 0 and first = null
//       without attached rows, else as above.  The part that holds row first[slot] is never empty for any row.
// Either way L > 0.
template <int HS>
__global__ __launch_bounds__(256) void bd_attn_fold_kernel(const float* __restrict__ po, const float2* __restrict__ pml,
                                                           float* __restrict__ out, BdCaches bc, const int* __restrict__ first,
                                                           int kv_mul, int E, int stride, int np, int p0) {
    const int kvh = blockIdx.x, b = blockIdx.y, nkv = gridDim.x;
    const BdRow row = bc.rows[b];
    if (!bd_row_ok(bc, row)) return;
    const size_t sbase = ((size_t)b * nkv + kvh) * np;
    const int pa = first && first[row.slot] > 0 ? 0 : p0;
    for (int idx = threadIdx.x; idx < kv_mul * HS; idx += 256) {
        const int q = idx / HS, d = idx % HS;
        float M = -INFINITY;
        for (int p = pa; p < np; ++p) M = fmaxf(M, pml[(sbase + p) * stride + q].x);
        float L = 0.f, val = 0.f;
        for (int p = pa; p < np; ++p) {
            const float2 ml = pml[(sbase + p) * stride + q];
            const float e = ml.x == -INFINITY ? 0.f : expf(ml.x - M);
            L += ml.y * e;
            val += po[((sbase + p) * stride + q) * HS + d] * e;
        }
        out[(size_t)b * E + (size_t)(kvh * kv_mul + q) * HS + d] = val / L;
    }
}

// ---- the attention of a batch with q8_0 caches                                                                        ------------
// Four kernels with __global__ names of their own (tests/test_build_cpu.py counts the instantiations of the names above), each
// setup + attn_tiles + attn_merge_waves over AttnAhead<HS, KvQ8>: the bytes and scales are converted in registers, then the f32
// statements run unchanged.  prefix / own / span ARE the bodies above; the per-row kernel is bd_attn_kernel's setup and part states
// (stride BD_MAX_GROUP; parts == 1: normalised to `out`) on the shared loop -- that kernel's exception is not extended.
// bd_attn_fold_kernel folds the parts of either.
template <int HS>
__global__ __launch_bounds__(BD_WAVES * WAVE) void bd_q8_attn_kernel(const float* __restrict__ Q, Q8Rows kc, Q8Rows vc, float* __restrict__ out,
                                                                     float* __restrict__ po, float2* __restrict__ pml, BdCaches bc, int KV,
                                                                     int kv_mul, int E, int tpp) {
    constexpr int DG = HS / 4, NT = HS / 16;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 15, g = lane >> 4;
    const int kvh = blockIdx.x, b = blockIdx.y, part = blockIdx.z, parts = gridDim.z, nkv = gridDim.x;
    const BdRow row = bc.rows[b];
    if (!bd_row_ok(bc, row)) return;                  // whole workgroup: no barrier is pending
    const int nrows = row.pos;
    const int h = kvh * kv_mul + min(li, kv_mul - 1);
    float qf[DG];
    attn_load_q<HS>(qf, Q + (size_t)b * E + (size_t)h * HS + g * DG);
    float m_run, l_run;
    pf_v4f O[NT];
    const int ntile = (nrows + BD_TILE - 1) / BD_TILE, t0 = part * tpp, t1 = min(t0 + tpp, ntile);
    const size_t base = (size_t)row.slot * bc.slot_stride + (size_t)kvh * HS;
    attn_tiles<HS, KvQ8, BD_WAVES>(qf, attn_at(kc, base + g * DG), attn_at(vc, base + NT * li), KV, nrows - 1, ntile, t0, t1, wid, li, g,
                                   [&](int r) { return r < nrows; }, m_run, l_run, O);
    const size_t pbase = ((size_t)b * nkv + kvh) * parts + part;
    attn_merge_waves<HS, BD_WAVES>(m_run, l_run, O, kv_mul, [&](int q, int d, float M, float L, float val) {
        if (parts == 1) {
            out[(size_t)b * E + (size_t)(kvh * kv_mul + q) * HS + d] = val / L;
        } else {
            po[(pbase * BD_MAX_GROUP + q) * HS + d] = val;
            if (d == 0) pml[pbase * BD_MAX_GROUP + q] = make_float2(M, L);
        }
    });
}
template <int HS>
__global__ __launch_bounds__(BD_WAVES * WAVE) void bd_q8_attn_prefix_kernel(const float* __restrict__ Q, Q8Rows pk, Q8Rows pv, float* __restrict__ po,
                                                                            float2* __restrict__ pml, const int* __restrict__ colmap, int n,
                                                                            int P, int KV, int kv_mul, int E, int tpp, int np) {
    bd_attn_prefix_body<HS, KvQ8>(Q, pk, pv, po, pml, colmap, n, P, KV, kv_mul, E, tpp, np);
}
template <int HS>
__global__ __launch_bounds__(BD_WAVES * WAVE) void bd_q8_attn_own_kernel(const float* __restrict__ Q, Q8Rows kc, Q8Rows vc, float* __restrict__ po,
                                                                         float2* __restrict__ pml, BdCaches bc, const int* __restrict__ first,
                                                                         int KV, int kv_mul, int E, int tpp, int np, int p0) {
    bd_attn_own_body<HS, KvQ8>(Q, kc, vc, po, pml, bc, first, KV, kv_mul, E, tpp, np, p0);
}
template <int HS>
__global__ __launch_bounds__(BD_WAVES * WAVE) void bd_q8_attn_span_kernel(const float* __restrict__ Q, Q8Rows kc, Q8Rows vc, float* __restrict__ out,
                                                                          float* __restrict__ po, float2* __restrict__ pml, BdCaches bc,
                                                                          const BdGroup* __restrict__ groups, const int* __restrict__ first,
                                                                          int n, int KV, int kv_mul, int E, int tpp, int np, int p0, int direct) {
    bd_attn_span_body<HS, KvQ8>(Q, kc, vc, out, po, pml, bc, groups, first, n, KV, kv_mul, E, tpp, np, p0, direct);
}

// The kernels by cache type, for the host's one dispatch (llmk.hip with_kv_type): T = float | _Float16 | KvQ8
template <int HS, class T>
struct BdAttn {
    static constexpr auto row = bd_attn_kernel<HS, T>;
    static constexpr auto prefix = bd_attn_prefix_kernel<HS, T>;
    static constexpr auto own = bd_attn_own_kernel<HS, T>;
    static constexpr auto span = bd_attn_span_kernel<HS, T>;
};
template <int HS>
struct BdAttn<HS, KvQ8> {
    static constexpr auto row = bd_q8_attn_kernel<HS>;
    static constexpr auto prefix = bd_q8_attn_prefix_kernel<HS>;
    static constexpr auto own = bd_q8_attn_own_kernel<HS>;
    static constexpr auto span = bd_q8_attn_span_kernel<HS>;
};

// llmk_batch_decode, between two passes: row i's pick (1-based; greedy: the classifier's first maximum, else what the sampler left)
// is recorded, becomes the token the row feeds next (0-based, as pf_embed_kernel reads it) and the row moves one position on.
// No pick (no finite logit): the error word is raised and the row feeds token 0 -- the call answers LLMK_E_NONFINITE.
__global__ void bd_advance_kernel(const int* __restrict__ picked, int n, int V, int step, int steps, int* __restrict__ ids,
                                  int* __restrict__ tok0, BdRow* __restrict__ rows, unsigned* __restrict__ err) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int id = picked[i];
    const bool ok = id >= 1 && id <= V;
    if (!ok) atomicOr(err, 1u);
    ids[(size_t)i * steps + step] = ok ? id : 0;
    tok0[i] = ok ? id - 1 : 0;
    rows[i].pos += 1;
}

}  // namespace llmk
