// Truncated sampling: top-k, top-p (nucleus) and min-p filters in front of the Gumbel-max rule of sample.h
// (llmk_forward_sample_ex / llmk_decode_sample_ex / llmk_sample_logits).
//
//   z[i]   the V logits of the position (-0.0f counts as +0.0f);  invT = f32(1 / T)
//   s[i] = z[i] * invT (rounded once),  m = max_i s[i],  e[i] = expf(s[i] - m),  Q[i] = (uint64) floorf(e[i] * 2^32)  (<= 2^32)
//
// All three filters are monotone in z, so the kept set is { i : z[i] >= tau } for ONE threshold tau = max(tau_k, tau_p, tau_m):
//   top-k  (top_k >= 1; 0 = off, and so is top_k >= the number of non-NaN rows): tau_k = the k-th largest logit counting duplicates;
//          rows that tie with it are ALL kept (the rule knows no index order and needs no sort);
//   top-p  (0 < top_p < 1; exactly 1 = off): with S = sum of Q[j] over z[j] >= tau_k and G(t) = sum of Q[j] over z[j] > t, row i is
//          kept iff (double)G(z[i]) < (double)top_p * (double)S -- the nucleus of the distribution that is sampled, after top-k and
//          renormalised over it.  The sums are 64-bit integers below 2^49: exact, free of any order of addition, exact in double;
//          the row of the maximum is always kept (G = 0 < top_p * S);
//   min-p  (0 <= min_p <= 1; 0 = off): row i is kept iff e[i] >= min_p;
//   token = 1 + argmax over the kept rows of llmk_sample_score(z[i], invT, seed, pos, i), first maximum wins.
// NaN and -inf rows are never kept.  A maximum of +inf (or a scaled maximum beyond the f32 range) keeps the rows equal to the
// maximum.  No row above -inf: no token (id 0, kept 0, tau = +inf) -- LLMK_E_NONFINITE on the host.
//
// The thresholds are found by a radix descent on the order-preserving 32-bit key of z: four levels of 256 bins, each a count and a
// sum of Q.  Walking the bins from the top resolves tau_k by count and tau_p by mass; the bin that straddles the bound is descended
// into.  Everything here is plain arithmetic with contraction off, no HIP API: a host program compiles the same functions
// (tests/test_sample_filter_cpu.py), and llmk_filter_rule below is the whole rule, serially; sample_filter_kernel (kernels.h) is
// the same descent by one workgroup.
#ifndef LLMK_SAMPLE_FILTER_H
#define LLMK_SAMPLE_FILTER_H

#include "sample.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LLMK_HD __host__ __device__ __forceinline__
#else
#define LLMK_HD static inline
#endif

// The sampler as the device reads it (behind llmk_sample_params in device memory: scratch_layout.h TkDevWords::filt)
struct llmk_filter_params {
    float invT;
    uint32_t seed_lo, seed_hi;
    int32_t top_k;
    float top_p, min_p;
    uint32_t pad[2];
};

constexpr uint32_t LLMK_FILTER_KEY_NINF = 0x007fffffu;      // llmk_filter_key(-inf): below every row that can be kept

LLMK_HD uint32_t llmk_filter_bits(float z) {
    uint32_t b;
    __builtin_memcpy(&b, &z, 4);
    return b;
}
LLMK_HD float llmk_filter_float(uint32_t b) {
    float z;
    __builtin_memcpy(&z, &b, 4);
    return z;
}
// order-preserving key of a non-NaN logit: a < b  <=>  key(a) < key(b);  -0.0f and +0.0f share one key
LLMK_HD uint32_t llmk_filter_key(float z) {
    uint32_t b = llmk_filter_bits(z);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
LLMK_HD float llmk_filter_unkey(uint32_t k) { return llmk_filter_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// m from the largest logit (z -> z * invT is monotone, so this is max_i s[i])
LLMK_HD float llmk_filter_m(float zmax, float invT) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return zmax * invT;
}
// e[i]: the product and the difference each rounded to f32 (never contracted to an fma)
LLMK_HD float llmk_filter_e(float z, float invT, float m) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float s = z * invT;
    const float d = s - m;
    return expf(d);
}
// Q[i]: the scaling by 2^32 is exact
LLMK_HD uint64_t llmk_filter_q(float e) { return (uint64_t)floorf(e * 4294967296.0f); }
// the top-p bound as the rule compares it
LLMK_HD double llmk_filter_target(float top_p, uint64_t S) { return (double)top_p * (double)S; }

// The 256 bins of one level: rows whose key agrees with the descent's prefix above the level's digit
struct llmk_filter_bins {
    uint32_t cnt[256];
    uint64_t sum[256];
};
// What a walk from the top of the bins settles on: the digit to descend into, and what lies above it (within the prefix and before it)
struct llmk_filter_walk {
    int digit;
    uint32_t cnt_above;
    uint64_t sum_above;
};
// by count: the bin that holds the k-th largest row (cnt_above < k <= cnt_above + cnt[digit])
LLMK_HD llmk_filter_walk llmk_filter_walk_count(const llmk_filter_bins* b, uint32_t cnt_above, uint64_t sum_above, uint32_t k) {
    llmk_filter_walk w;
    w.digit = 0;
    for (int d = 255; d >= 0; --d) {
        if (b->cnt[d] != 0 && cnt_above + b->cnt[d] >= k) { w.digit = d; break; }
        cnt_above += b->cnt[d];
        sum_above += b->sum[d];
    }
    w.cnt_above = cnt_above;
    w.sum_above = sum_above;
    return w;
}
// by mass: the LOWEST non-empty bin whose largest row is still kept ((double)sum_above < target); every row above it is kept, every
// row below it is not, so the threshold lies inside.  The walk starts on a kept row (the maximum has nothing above it).
LLMK_HD llmk_filter_walk llmk_filter_walk_mass(const llmk_filter_bins* b, uint64_t sum_above, double target) {
    llmk_filter_walk w;
    w.digit = 0;
    w.cnt_above = 0;
    w.sum_above = sum_above;
    for (int d = 255; d >= 0; --d) {
        if (!((double)sum_above < target)) break;
        if (b->cnt[d] != 0) { w.digit = d; w.sum_above = sum_above; }
        sum_above += b->sum[d];
    }
    return w;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The whole rule, serially (the host's statement of it; the kernel is checked against this and against tests/filter_ref.py).
// Returns the 1-based token, 0 = no token; *kept_out = rows kept, *tau_out = the threshold.
static inline void llmk_filter_fill(const float* z, int V, float invT, float m, int level, uint32_t prefix, llmk_filter_bins* b) {
    const int shift = 24 - 8 * level;
    for (int d = 0; d < 256; ++d) { b->cnt[d] = 0; b->sum[d] = 0; }
    for (int i = 0; i < V; ++i) {
        if (z[i] != z[i]) continue;
        const uint32_t key = llmk_filter_key(z[i]);
        if (level > 0 && (key >> (shift + 8)) != prefix) continue;
        const int d = (int)((key >> shift) & 255u);
        b->cnt[d] += 1;
        b->sum[d] += llmk_filter_q(llmk_filter_e(z[i], invT, m));
    }
}
static inline int llmk_filter_rule(const float* z, int V, const llmk_filter_params* p, int pos, int* kept_out, float* tau_out) {
    const float invT = p->invT;
    const uint64_t seed = (uint64_t)p->seed_lo | ((uint64_t)p->seed_hi << 32);
    float zmax = -INFINITY;
    uint32_t valid = 0;
    for (int i = 0; i < V; ++i)
        if (z[i] == z[i]) { ++valid; if (z[i] > zmax) zmax = z[i]; }
    *kept_out = 0;
    *tau_out = INFINITY;
    if (valid == 0 || zmax == -INFINITY) return 0;
    const float m = llmk_filter_m(zmax, invT);
    uint32_t tau = LLMK_FILTER_KEY_NINF;
    if (!isfinite(m)) {
        tau = llmk_filter_key(zmax);
    } else {
        llmk_filter_bins b;
        if (p->min_p > 0.f) {
            uint32_t tm = llmk_filter_key(zmax);
            for (int i = 0; i < V; ++i)
                if (z[i] == z[i] && llmk_filter_e(z[i], invT, m) >= p->min_p) { const uint32_t k = llmk_filter_key(z[i]); if (k < tm) tm = k; }
            if (tm > tau) tau = tm;
        }
        const bool k_on = p->top_k > 0 && (uint32_t)p->top_k < valid;
        uint64_t S = 0, ties = 0;
        if (k_on) {
            uint32_t prefix = 0, ca = 0;
            uint64_t sa = 0;
            for (int level = 0; level < 4; ++level) {
                llmk_filter_fill(z, V, invT, m, level, prefix, &b);
                const llmk_filter_walk w = llmk_filter_walk_count(&b, ca, sa, (uint32_t)p->top_k);
                prefix = (prefix << 8) | (uint32_t)w.digit;
                ca = w.cnt_above;
                sa = w.sum_above;
                ties = b.sum[w.digit];
            }
            S = sa + ties;
            if (prefix > tau) tau = prefix;
        } else if (p->top_p < 1.f) {
            llmk_filter_fill(z, V, invT, m, 0, 0, &b);
            for (int d = 0; d < 256; ++d) S += b.sum[d];
        }
        if (p->top_p < 1.f) {
            const double target = llmk_filter_target(p->top_p, S);
            if (!(k_on && (double)(S - ties) < target)) {       // (else every row of the top-k set is inside the nucleus: tau_p <= tau_k)
                uint32_t prefix = 0;
                uint64_t sa = 0;
                for (int level = 0; level < 4; ++level) {
                    llmk_filter_fill(z, V, invT, m, level, prefix, &b);
                    const llmk_filter_walk w = llmk_filter_walk_mass(&b, sa, target);
                    prefix = (prefix << 8) | (uint32_t)w.digit;
                    sa = w.sum_above;
                }
                if (prefix > tau) tau = prefix;
            }
        }
    }
    float best = -INFINITY;
    int idx = -1, kept = 0;
    for (int i = 0; i < V; ++i) {
        if (z[i] != z[i] || z[i] == -INFINITY || llmk_filter_key(z[i]) < tau) continue;
        ++kept;
        const float v = llmk_sample_score(z[i], invT, seed, pos, i);
        if (v > best) { best = v; idx = i; }
    }
    *kept_out = kept;
    *tau_out = llmk_filter_unkey(tau);
    return idx + 1;
}
#endif

#undef LLMK_HD
#endif  // LLMK_SAMPLE_FILTER_H
