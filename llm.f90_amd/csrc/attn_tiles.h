// The MFMA attention the batched paths share (DESIGN.md sections 3c, 3i): pf_attn_kernel (prefill.h), bd_attn_prefix_kernel and
// bd_attn_own_kernel (batch.h) are setup + attn_tiles + attn_merge_waves; bd_attn_kernel (batch.h) shares the look-ahead types and
// keeps the loop and the merge written out (the reason stands at that kernel); the four bd_q8_attn_* kernels of a q8_0 batch are
// setup + these calls as well, over AttnAhead<HS, KvQ8>.  A workgroup owns 16 query COLUMNS
// (prompt positions, or the query heads of a kv group) and a range of 16-row tiles of one K/V cache; its NW waves take the tiles round
// robin, each with its own running softmax (max m, sum l, unnormalised output O), and merge through LDS at the end.
//
// Per tile and wave, with v_mfma_f32_16x16x4_f32 (D[i][j] += sum_k A[i][k] B[k][j]; lane l gives A[l%16][l/16] and
// B[l/16][l%16], and receives D[4*(l/16)+v][l%16] in register v):
//   S^T = K Q^T : A = K tile (i = cache row), B = Q (j = query), HS/4 steps; lane (q = l%16, g = l/16) holds head
//         dimensions 16g' .. of both (the contraction index can be any permutation as long as A and B agree), and ends up
//         with S[q][row 4g+v], v = 0..3 -- a query's 16 scores sit in 4 lanes x 4 registers: max and sum need two
//         cross-lane steps (xor 16, 32);
//   O += P V   : A = P (i = query): lane (q, g) feeds P[q][row 4g+v] in step v -- exactly the registers it holds, no
//         transpose; B = V: lane (c = l%16, g) feeds V[row 4g+v][NT*c + t] for output tile t (NT = HS/16 adjacent floats:
//         one vector load per row), and receives O[query 4g+r][NT*c + t] in register r.
// NOT a stand-alone header: prefill.h includes it behind its pf_v4f (the MFMA accumulator type) and kernels.h's WAVE.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace llmk {

static_assert(WAVE == 64 && sizeof(pf_v4f) == 16, "included behind kernels.h (WAVE) and prefill.h's pf_v4f; the lane arithmetic below is wave64's");

// LDS of a workgroup of `waves` waves: the waves' O [waves][16][hs], m and l [waves][16] each
constexpr size_t attn_smem(int waves, int hs) { return ((size_t)waves * 16 * hs + 2 * waves * 16) * sizeof(float); }

// ---- a tile's K / V fragments, requested one tile ahead                                                               ------------
// Lane (li, g) of a wave holds, of the tile at cache row r0: K row r0 + li, elements g * DG .. + DG (kb points at the lane's first);
// V rows r0 + 4g + v, v = 0..3, elements NT * li .. + NT (vb likewise).  load: unconditional loads of a row index clamped to `last`
// into the look-ahead registers K / V; take: those registers as the MFMA's f32 operands.  f32 caches: float[DG] and float[4][NT],
// 16-byte loads (V: 4 | 8 | 16 bytes at head sizes 16 | 32 | 64 and up).  f16 caches: the halves stay PACKED in the look-ahead
// registers (half the VGPRs) and are converted at use, exactly; the loads are as wide as the fragment: K 16 bytes (8 halves) a piece
// at head sizes 32 .. 128 and one 8-byte load at 16, V 2 | 4 | 8 | 16 bytes.  kv_dim % 16 == 0 keeps every row 32-byte aligned in
// either type.
template <int HS, class T>
struct AttnAhead;
template <int HS>
struct AttnAhead<HS, float> {
    static constexpr int DG = HS / 4, NT = HS / 16;
    typedef const float* __restrict__ Ptr;
    typedef float K[DG];
    typedef float V[4][NT];
    static __device__ __forceinline__ void load(K& kn, V& vn, const float* kb, const float* vb, int KV, int r0, int li, int g, int last) {
        const float* kp = kb + (size_t)min(r0 + li, last) * KV;
#pragma unroll
        for (int m = 0; m < DG; m += 4) {
            const float4 v = *reinterpret_cast<const float4*>(kp + m);
            kn[m] = v.x; kn[m + 1] = v.y; kn[m + 2] = v.z; kn[m + 3] = v.w;
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const float* vp = vb + (size_t)min(r0 + 4 * g + v, last) * KV;
            if constexpr (NT % 4 == 0) {
#pragma unroll
                for (int t = 0; t < NT; t += 4) {
                    const float4 x = *reinterpret_cast<const float4*>(vp + t);
                    vn[v][t] = x.x; vn[v][t + 1] = x.y; vn[v][t + 2] = x.z; vn[v][t + 3] = x.w;
                }
            } else if constexpr (NT == 2) {
                const float2 x = *reinterpret_cast<const float2*>(vp);
                vn[v][0] = x.x; vn[v][1] = x.y;
            } else {
                vn[v][0] = vp[0];
            }
        }
    }
    static __device__ __forceinline__ void take(const K& kn, const V& vn, float (&kf)[DG], float (&vf)[4][NT]) {
#pragma unroll
        for (int m = 0; m < DG; ++m) kf[m] = kn[m];
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int t = 0; t < NT; ++t) vf[v][t] = vn[v][t];
    }
};
template <int N>
struct AttnHalves { typedef _Float16 type __attribute__((ext_vector_type(N))); };
template <>
struct AttnHalves<1> { typedef _Float16 type; };
template <int HS>
struct AttnAhead<HS, _Float16> {
    static constexpr int DG = HS / 4, NT = HS / 16, KW = DG < 8 ? DG : 8;      // KW: halves per K load
    typedef const _Float16* __restrict__ Ptr;
    typedef typename AttnHalves<KW>::type K[DG / KW];
    typedef typename AttnHalves<NT>::type V[4];
    static __device__ __forceinline__ void load(K& kn, V& vn, const _Float16* kb, const _Float16* vb, int KV, int r0, int li, int g, int last) {
        const _Float16* kp = kb + (size_t)min(r0 + li, last) * KV;
#pragma unroll
        for (int m = 0; m < DG / KW; ++m) kn[m] = *reinterpret_cast<const typename AttnHalves<KW>::type*>(kp + m * KW);
#pragma unroll
        for (int v = 0; v < 4; ++v)
            vn[v] = *reinterpret_cast<const typename AttnHalves<NT>::type*>(vb + (size_t)min(r0 + 4 * g + v, last) * KV);
    }
    static __device__ __forceinline__ void take(const K& kn, const V& vn, float (&kf)[DG], float (&vf)[4][NT]) {
#pragma unroll
        for (int m = 0; m < DG; ++m) kf[m] = (float)kn[m / KW][m % KW];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            if constexpr (NT == 1) {
                vf[v][0] = (float)vn[v];
            } else {
#pragma unroll
                for (int t = 0; t < NT; ++t) vf[v][t] = (float)vn[v][t];
            }
        }
    }
};

// q8_0 caches (llmk_cache_create(.., LLMK_TYPE_Q8_0)): a position's kv_dim row is blocks of 32 consecutive elements, a
// block is 32 int8 quants and one f16 scale d, value = (float)q * (float)d (exact in f32: 7 x 11 significant bits).  Quants and scales
// lie in SEPARATE arrays of the same index order -- quant of element e at q[e], its block's scale at d[e / 32] -- so that a fragment's
// quants load at their natural width and alignment.  Q8Rows is a view of both at a block boundary; attn_at moves a view (or a plain
// pointer) on by e elements.
struct KvQ8 {};      // the element "type" of such a batch, where the f32 / f16 batches say float / _Float16
struct Q8Rows {
    int8_t* q;
    _Float16* d;
};
__host__ __device__ __forceinline__ Q8Rows attn_at(Q8Rows p, size_t e) { return Q8Rows{p.q + e, p.d + (e >> 5)}; }      // (p at a block boundary)
template <class T>
__host__ __device__ __forceinline__ T* attn_at(T* p, size_t e) { return p + e; }
// The look-ahead registers hold the PACKED bytes -- K: DG / 4 words, V: a word (two at head size 128) per row, the bytes in front
// zero-extended -- and the scales as loaded: one for the K fragment (DG <= 32 elements inside one block; at head size 16 a block spans
// two kv heads and the fragment still lies inside it), one per V row.  take dequantises in registers, each operand exactly
// (float)q * (float)d.  Loads: K 4 | 8 | 16 | 2 x 16 bytes, V 1 | 2 | 4 | 8 bytes, naturally aligned (kv_dim % 32 == 0).
template <int HS>
struct AttnAhead<HS, KvQ8> {
    static constexpr int DG = HS / 4, NT = HS / 16, KW = DG / 4, VW = (NT + 3) / 4;
    static_assert(DG <= 32, "a K fragment lies inside one q8_0 block");
    typedef Q8Rows Ptr;      // q at the lane's first quant, d at that quant's block
    struct K { unsigned w[KW]; _Float16 d; };
    struct V { unsigned w[4][VW]; _Float16 d[4]; };
    typedef unsigned u2 __attribute__((ext_vector_type(2)));
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ void load(K& kn, V& vn, Q8Rows kb, Q8Rows vb, int KV, int r0, int li, int g, int last) {
        const size_t rk = (size_t)min(r0 + li, last);
        const int8_t* kp = kb.q + rk * KV;
        kn.d = kb.d[rk * (KV >> 5)];
        if constexpr (KW == 1) {
            kn.w[0] = *reinterpret_cast<const unsigned*>(kp);
        } else if constexpr (KW == 2) {
            const u2 x = *reinterpret_cast<const u2*>(kp);
            kn.w[0] = x.x; kn.w[1] = x.y;
        } else {
#pragma unroll
            for (int m = 0; m < KW; m += 4) {
                const u4 x = *reinterpret_cast<const u4*>(kp + 4 * m);
                kn.w[m] = x.x; kn.w[m + 1] = x.y; kn.w[m + 2] = x.z; kn.w[m + 3] = x.w;
            }
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const size_t rv = (size_t)min(r0 + 4 * g + v, last);
            const int8_t* vp = vb.q + rv * KV;
            vn.d[v] = vb.d[rv * (KV >> 5)];
            if constexpr (NT == 1) {
                vn.w[v][0] = *reinterpret_cast<const uint8_t*>(vp);
            } else if constexpr (NT == 2) {
                vn.w[v][0] = *reinterpret_cast<const uint16_t*>(vp);
            } else if constexpr (NT == 4) {
                vn.w[v][0] = *reinterpret_cast<const unsigned*>(vp);
            } else {
                const u2 x = *reinterpret_cast<const u2*>(vp);
                vn.w[v][0] = x.x; vn.w[v][1] = x.y;
            }
        }
    }
    static __device__ __forceinline__ float value(unsigned w, int k, float d) { return (float)(int)(int8_t)(w >> (8 * k)) * d; }
    static __device__ __forceinline__ void take(const K& kn, const V& vn, float (&kf)[DG], float (&vf)[4][NT]) {
        const float dk = (float)kn.d;
#pragma unroll
        for (int m = 0; m < DG; ++m) kf[m] = value(kn.w[m / 4], m % 4, dk);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const float dv = (float)vn.d[v];
#pragma unroll
            for (int t = 0; t < NT; ++t) vf[v][t] = value(vn.w[v][t / 4], t % 4, dv);
        }
    }
};

// lane (li, g)'s fragment of its query column: elements g * DG .. + DG of the column's head (qp points at the first)
template <int HS>
__device__ __forceinline__ void attn_load_q(float (&qf)[HS / 4], const float* __restrict__ qp) {
#pragma unroll
    for (int m = 0; m < HS / 4; m += 4) {
        const float4 v = *reinterpret_cast<const float4*>(qp + m);
        qf[m] = v.x; qf[m + 1] = v.y; qf[m + 2] = v.z; qf[m + 3] = v.w;
    }
}

// ---- the tile loop                                                                          llama2.f90:572-598 ------------
// Wave `wid` of NW takes tiles t0 + wid, t0 + wid + NW, .. < t1 of the cache at kb / vb (already at this lane's kv head and fragment)
// and leaves its running state in m_run, l_run, O.  visible(r): does this lane's query column see cache row r?  Loads clamp the row
// index to `last` and the tile index to ntile - 1 (a tile's two dozen MFMAs and its softmax take far less than an L2 round trip, so
// the next tile is requested before this one is multiplied).  A wave without a visible row leaves m = -inf, l = 0, O = 0.
template <int HS, class T, int NW, class Visible>
__device__ __forceinline__ void attn_tiles(const float (&qf)[HS / 4], typename AttnAhead<HS, T>::Ptr kb, typename AttnAhead<HS, T>::Ptr vb, int KV,
                                           int last, int ntile, int t0, int t1, int wid, int li, int g, Visible visible, float& m_run,
                                           float& l_run, pf_v4f (&O)[HS / 16]) {
    constexpr int DG = HS / 4, NT = HS / 16;
    typedef AttnAhead<HS, T> Ahead;
    const float scale = sqrtf((float)HS);
    m_run = -INFINITY;
    l_run = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) O[t] = (pf_v4f){0.f, 0.f, 0.f, 0.f};
    typename Ahead::K kn;
    typename Ahead::V vn;
    Ahead::load(kn, vn, kb, vb, KV, min(t0 + wid, ntile - 1) * 16, li, g, last);
    for (int kt = t0 + wid; kt < t1; kt += NW) {
        const int r0 = kt * 16;
        float kf[DG], vf[4][NT];
        Ahead::take(kn, vn, kf, vf);
        Ahead::load(kn, vn, kb, vb, KV, min(kt + NW, ntile - 1) * 16, li, g, last);
        pf_v4f acc = (pf_v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < DG; ++m) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[m], qf[m], acc, 0, 0, 0);
        float sc[4], mx = -INFINITY;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            sc[v] = visible(r0 + 4 * g + v) ? acc[v] / scale : -INFINITY;
            mx = fmaxf(mx, sc[v]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const bool any = m_new != -INFINITY;                                   // false: nothing of this column seen so far
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
            const float ar = __shfl(alpha, 4 * g + r, 64);                     // O rows are columns 4g+r
#pragma unroll
            for (int t = 0; t < NT; ++t) O[t][r] *= ar;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int v = 0; v < 4; ++v) O[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[v], vf[v][t], O[t], 0, 0, 0);
    }
}

// ---- the waves' running states through LDS into one state per column                                                  ------------
// For element d of each of the first `live` columns c: emit(c, d, M, L, val) with M = max_w m_w, L = sum_w l_w e^(m_w - M) and
// val = sum_w O_w e^(m_w - M), in wave order.  The caller stores val / L, or leaves {M, L, val} as a part state (a part without a
// visible row: M = -inf, L = 0, val = 0).  Dynamic LDS: attn_smem(NW, HS).
template <int HS, int NW, class Emit>
__device__ __forceinline__ void attn_merge_waves(float m_run, float l_run, const pf_v4f (&O)[HS / 16], int live, Emit emit) {
    constexpr int NT = HS / 16;
    extern __shared__ __attribute__((aligned(16))) char pf_smem[];
    float* so = reinterpret_cast<float*>(pf_smem);   // [NW][16][HS]
    float* sm = so + NW * 16 * HS;                    // [NW][16]
    float* sl = sm + NW * 16;                         // [NW][16]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 15, g = lane >> 4;
    if (g == 0) {
        sm[wid * 16 + li] = m_run;
        sl[wid * 16 + li] = l_run;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int t = 0; t < NT; ++t) so[(size_t)(wid * 16 + 4 * g + r) * HS + NT * li + t] = O[t][r];
    __syncthreads();
    for (int idx = tid; idx < live * HS; idx += NW * WAVE) {
        const int c = idx / HS, d = idx % HS;
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < NW; ++w) M = fmaxf(M, sm[w * 16 + c]);
        float L = 0.f, val = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float mw = sm[w * 16 + c];
            const float e = mw == -INFINITY ? 0.f : expf(mw - M);
            L += sl[w * 16 + c] * e;
            val += so[(size_t)(w * 16 + c) * HS + d] * e;
        }
        emit(c, d, M, L, val);
    }
}

}  // namespace llmk
