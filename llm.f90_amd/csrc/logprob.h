// Decode log-probs: the log-probability of the token a sampling call returns, and the top-N alternatives of its position
// (llmk_forward_sample_lp / llmk_decode_sample_lp / llmk_logprob_logits).
//
//   z[i]   the V RAW logits of the position: what the classifier wrote, before bias, penalties, temperature and truncation
//   L    = llmk_lse_value(state) (score.h), the state built in ONE order: thread t of 1,024 steps rows t, t + 1024, ... from the
//          empty state (llmk_lse_step); a wave of 64 threads folds by xor-butterfly (offsets 32, 16, ... 1; llmk_lse_merge is
//          symmetric, so every lane holds the same bits); the 16 waves merge in ascending order
//   token_logprob = z[id - 1] - L            id: the 1-based token the call returns for the position (0: none, 0.0f)
//   alternatives: the LISTABLE rows are those with z > -inf (NaN rows are not), ordered by z descending, then index ascending --
//          the IEEE comparison, so -0.0 and +0.0 tie and the lower index comes first.  Entry j < top_n is the j-th listable row,
//          {1-based id, z - L}; with fewer than top_n listable rows the remaining entries are {0, -inf}.
// Nothing is an error here: a +inf or NaN logit makes L, and with it the values, whatever score.h's arithmetic gives in this order
// (NaN, except that an EMPTY state drops a NaN it meets first: llmk_lse_step / llmk_lse_merge); the ids stay defined.
//
// The top_n-th largest listable row is found without a sort, by the count descent of sample_filter.h on its order-preserving key
// (llmk_filter_key, llmk_filter_walk_count); the rows above that key and the first rows equal to it, in ascending index order,
// are the list.  Everything here is plain f32 arithmetic with contraction off, no HIP API: a host program compiles the same
// functions (tests/test_logprob_cpu.py), and llmk_logprob_rule below is the whole rule, serially; sample_logprob_kernel
// (kernels.h) is the same by one workgroup.
#ifndef LLMK_LOGPROB_H
#define LLMK_LOGPROB_H

#include "score.h"
#include "sample_filter.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LLMK_HD __host__ __device__ __forceinline__
#else
#define LLMK_HD static inline
#endif

constexpr int LLMK_LOGPROB_MAX_TOP = 20;      // (llmk.h LLMK_MAX_TOP_LOGPROBS)
constexpr int LLMK_LOGPROB_THREADS = 1024, LLMK_LOGPROB_WAVE = 64;

// What the kernel leaves per position (device memory, read back in one copy)
struct llmk_logprob_record {
    float token_logprob;
    int32_t top_tokens[LLMK_LOGPROB_MAX_TOP];      // 1-based, 0 = none
    float top_logprobs[LLMK_LOGPROB_MAX_TOP];
};

LLMK_HD bool llmk_logprob_listable(float z) { return z > -INFINITY; }      // (false for NaN)
// z - L, rounded once
LLMK_HD float llmk_logprob_value(float z, float L) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return z - L;
}
// the order of the list: row a comes before row b
LLMK_HD bool llmk_logprob_before(float za, int ia, float zb, int ib) { return za > zb || (za == zb && ia < ib); }

#if !defined(__HIP_DEVICE_COMPILE__)
// L in the kernel's order
static inline float llmk_logprob_lse(const float* z, int V) {
    llmk_lse wave[LLMK_LOGPROB_THREADS / LLMK_LOGPROB_WAVE];
    for (int w = 0; w < LLMK_LOGPROB_THREADS / LLMK_LOGPROB_WAVE; ++w) {
        llmk_lse lane[LLMK_LOGPROB_WAVE], next[LLMK_LOGPROB_WAVE];
        for (int l = 0; l < LLMK_LOGPROB_WAVE; ++l) {
            lane[l] = llmk_lse_empty();
            for (int i = w * LLMK_LOGPROB_WAVE + l; i < V; i += LLMK_LOGPROB_THREADS) lane[l] = llmk_lse_step(lane[l], z[i]);
        }
        for (int o = LLMK_LOGPROB_WAVE / 2; o > 0; o >>= 1) {
            for (int l = 0; l < LLMK_LOGPROB_WAVE; ++l) next[l] = llmk_lse_merge(lane[l], lane[l ^ o]);
            for (int l = 0; l < LLMK_LOGPROB_WAVE; ++l) lane[l] = next[l];
        }
        wave[w] = lane[0];
    }
    llmk_lse st = wave[0];
    for (int w = 1; w < LLMK_LOGPROB_THREADS / LLMK_LOGPROB_WAVE; ++w) st = llmk_lse_merge(st, wave[w]);
    return llmk_lse_value(st);
}
// The whole rule, serially (the host's statement of it; the kernel is checked against this and against tests/logprob_ref.py).
// id in [0, V] (0: no token, *token_logprob = 0); top_n in [0, LLMK_LOGPROB_MAX_TOP]; token_logprob may be null, and so may the
// two lists when top_n == 0.  Returns the number of listed rows (<= top_n).
static inline int llmk_logprob_rule(const float* z, int V, int id, int top_n, float* token_logprob, int32_t* top_tokens, float* top_logprobs) {
    const float L = llmk_logprob_lse(z, V);
    if (token_logprob) *token_logprob = (id >= 1 && id <= V) ? llmk_logprob_value(z[id - 1], L) : 0.f;
    uint32_t listable = 0;
    for (int i = 0; i < V; ++i) listable += llmk_logprob_listable(z[i]) ? 1u : 0u;
    const uint32_t k = (uint32_t)top_n < listable ? (uint32_t)top_n : listable;
    int idx[LLMK_LOGPROB_MAX_TOP];
    float val[LLMK_LOGPROB_MAX_TOP];
    if (k > 0) {
        // the key of the k-th largest listable row: four levels of 256 counts (-inf rows are counted too: they lie below every
        // listable row, and k does not reach them)
        uint32_t prefix = 0, ca = 0;
        for (int level = 0; level < 4; ++level) {
            const int shift = 24 - 8 * level;
            llmk_filter_bins b;
            for (int d = 0; d < 256; ++d) { b.cnt[d] = 0; b.sum[d] = 0; }
            for (int i = 0; i < V; ++i) {
                if (z[i] != z[i]) continue;
                const uint32_t key = llmk_filter_key(z[i]);
                if (level > 0 && (key >> (shift + 8)) != prefix) continue;
                b.cnt[(key >> shift) & 255u] += 1;
            }
            const llmk_filter_walk w = llmk_filter_walk_count(&b, ca, 0, k);
            prefix = (prefix << 8) | (uint32_t)w.digit;
            ca = w.cnt_above;
        }
        // the rows above that key, then the first rows equal to it
        uint32_t got = 0, need = k - ca;
        for (int i = 0; i < V; ++i) {
            if (!llmk_logprob_listable(z[i])) continue;
            const uint32_t key = llmk_filter_key(z[i]);
            if (key > prefix || (key == prefix && need > 0)) {
                if (key == prefix) --need;
                idx[got] = i;
                val[got] = z[i];
                ++got;
            }
        }
    }
    for (uint32_t j = 0; j < k; ++j) {
        int rank = 0;
        for (uint32_t e = 0; e < k; ++e) rank += llmk_logprob_before(val[e], idx[e], val[j], idx[j]) ? 1 : 0;
        top_tokens[rank] = idx[j] + 1;
        top_logprobs[rank] = llmk_logprob_value(val[j], L);
    }
    for (int j = (int)k; j < top_n; ++j) { top_tokens[j] = 0; top_logprobs[j] = -INFINITY; }
    return (int)k;
}
#endif

#undef LLMK_HD
#endif  // LLMK_LOGPROB_H
