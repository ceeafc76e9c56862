// Per-position scoring arithmetic of llmk_score: the running log-sum-exp of a row of logits, the first
// maximum with its index, and the rules that merge two partial results.
//
//   lse(z) = m + log(sum_j exp(z[j] - m)),  m = max_j z[j]        logprob(target) = z[target] - lse(z)
//
// A partial state is (m, s) = (maximum so far, sum of exp(z - m) so far); the empty state is (-inf, 0).  Everything here is
// plain f32 arithmetic, no HIP API, so a host program compiles the same functions (tests/test_score_cpu.py); every kernel that
// scores (prefill.h pf_score_kernel / pf_score_merge_kernel) goes through these and nothing else, in a fixed order, with
// contraction off: the same logits give the same bits on every path.
#ifndef LLMK_SCORE_H
#define LLMK_SCORE_H

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LLMK_HD __host__ __device__ __forceinline__
#else
#define LLMK_HD static inline
#endif

struct llmk_lse { float m, s; };          // running maximum, sum of exp(z - m)
struct llmk_amax { float v; int i; };     // first maximum and its 0-based index; i < 0: no element above -inf yet

LLMK_HD llmk_lse llmk_lse_empty(void) {
    llmk_lse a;
    a.m = -INFINITY; a.s = 0.f;
    return a;
}

// the element step: one more logit.  z = -inf adds exp(-inf) = 0 (and must not reach expf as -inf - -inf); a NaN logit makes s,
// and with it the row's lse, NaN (m never becomes NaN: it only takes a z that compares greater)
LLMK_HD llmk_lse llmk_lse_step(llmk_lse a, float z) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (z == -INFINITY) return a;
    if (!(z > a.m)) {                     // (a.m > -inf here, or z is NaN)
        a.s += expf(z - a.m);
        return a;
    }
    // a new maximum: what was summed is rescaled to it.  First element above -inf: a.m = -inf, nothing summed yet
    const float old = a.m == -INFINITY ? 0.f : a.s * expf(a.m - z);
    a.s = old + 1.0f;
    a.m = z;
    return a;
}

// (m1, s1) + (m2, s2) = (M, s1 exp(m1 - M) + s2 exp(m2 - M)), M = max(m1, m2).  An empty side (m = -inf) contributes 0 whatever
// its s; two empty sides give the empty state (no -inf - -inf anywhere)
LLMK_HD llmk_lse llmk_lse_merge(llmk_lse a, llmk_lse b) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float M = a.m > b.m ? a.m : b.m;
    if (M == -INFINITY) return llmk_lse_empty();
    const float sa = a.m == -INFINITY ? 0.f : a.s * expf(a.m - M);
    const float sb = b.m == -INFINITY ? 0.f : b.s * expf(b.m - M);
    llmk_lse r;
    r.m = M; r.s = sa + sb;
    return r;
}

// lse of everything summed; -inf for the empty state
LLMK_HD float llmk_lse_value(llmk_lse a) { return a.m == -INFINITY ? -INFINITY : a.m + logf(a.s); }

LLMK_HD llmk_amax llmk_amax_empty(void) {
    llmk_amax a;
    a.v = -INFINITY; a.i = -1;
    return a;
}
// elements arrive in ascending index order: a later equal value does not replace the first maximum (llama2.f90:388, maxloc)
LLMK_HD llmk_amax llmk_amax_step(llmk_amax a, float z, int i) {
    if (z > a.v) { a.v = z; a.i = i; }
    return a;
}
// any two partial results: the larger value, the smaller index among equals; an empty side (i < 0) never wins
LLMK_HD llmk_amax llmk_amax_merge(llmk_amax a, llmk_amax b) {
    if (b.i >= 0 && (a.i < 0 || b.v > a.v || (b.v == a.v && b.i < a.i))) return b;
    return a;
}

#undef LLMK_HD
#endif  // LLMK_SCORE_H
