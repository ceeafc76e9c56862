// Repetition, frequency and presence penalties and the logit bias, in front of the truncated sampler of sample_filter.h
// (llmk_forward_sample_pen / llmk_decode_sample_pen / llmk_sample_logits_pen).
//
//   z[t]   the V logits of position pos (t 0-based);  r the repeat penalty, inv_r = f32(1 / r) rounded once on the host (as invT is);
//   f, p   the frequency and the presence penalty;
//   W      the window: the tokens fed at positions max(1, pos - last_n + 1) .. pos according to the context's token record
//          (hist[q - 1] = the 1-based token fed at position q, 0 = none: skipped);  c[t] = how often token t occurs in W
//
//   1. bias       for every entry (t, b) of the bias list:  z[t] <- z[t] + b            (b = -inf bans the token; ids distinct)
//   2. penalties  for every t with c[t] > 0:                z[t] <- (z[t] > 0 ? z[t] * inv_r : z[t] * r)
//                                                           z[t] <- z[t] - ((float)c[t] * f + p)
//   3. the adjusted vector goes through the rule of sample_filter.h unchanged (filters, Gumbel-max, first maximum wins, the same
//      stateless noise keyed by (seed, pos, row)).
//
// Each product, sum and difference is rounded to f32 (never contracted).  Bias comes before the penalties on a row that gets both:
// llama.cpp's order.  A NaN row stays NaN, a -inf row stays -inf, -0.0f takes the `<= 0` branch.  The product with inv_r stands in
// for llama.cpp's division by r ON PURPOSE: a rounded reciprocal and one product are a bit-exact function that numpy float32
// reproduces on any machine (tests/penalty_ref.py), where a device division need not be correctly rounded; the result differs from
// llama.cpp's quotient by at most 1 ulp.
//
// Everything here is plain arithmetic with contraction off, no HIP API: a host program compiles the same functions
// (tests/test_sample_penalty_cpu.py), and llmk_penalty_rule below is steps 1 and 2, serially; sample_penalty_kernel (kernels.h) is
// the same by one workgroup, with the counts kept by integer atomics.
#ifndef LLMK_SAMPLE_PENALTY_H
#define LLMK_SAMPLE_PENALTY_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LLMK_HD __host__ __device__ __forceinline__
#else
#define LLMK_HD static inline
#endif

#define LLMK_PENALTY_MAX_BIAS 256      // == LLMK_MAX_LOGIT_BIAS (include/llmk.h; llmk.hip holds the two together)

// The penalties as the device reads them (a buffer of their own, copied out of pinned memory like the filter's parameters)
struct llmk_penalty_bias {
    int32_t token;      // 1-based
    float bias;
};
struct llmk_penalty_params {
    float repeat, inv_repeat;
    float frequency, presence;
    int32_t last_n;     // window in positions; 0 = no penalties
    int32_t n_bias;
    uint32_t pad[2];
    llmk_penalty_bias bias[LLMK_PENALTY_MAX_BIAS];
};

// step 1 on one row
LLMK_HD float llmk_penalty_bias_row(float z, float b) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return z + b;
}
// step 2 on one row that occurs c > 0 times in the window
LLMK_HD float llmk_penalty_row(float z, int c, float r, float inv_r, float f, float p) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float s = z > 0.f ? z * inv_r : z * r;
    const float cf = (float)c * f;
    const float d = cf + p;
    return s - d;
}
// the first position of the window of `pos` (1-based, inclusive; the window ends at pos)
LLMK_HD int llmk_penalty_window_lo(int pos, int last_n) { return pos - last_n + 1 > 1 ? pos - last_n + 1 : 1; }

#if !defined(__HIP_DEVICE_COMPILE__)
// Steps 1 and 2, serially, in place on z (the host's statement of the rule; the kernel is checked against this and against
// tests/penalty_ref.py).  hist: the token record, at least `pos` entries; cnt: V ints of scratch, all zero on entry and on return.
static inline void llmk_penalty_rule(float* z, int V, const llmk_penalty_params* pp, const int* hist, int pos, int* cnt) {
    for (int j = 0; j < pp->n_bias; ++j) {
        const int t = pp->bias[j].token;
        if (t >= 1 && t <= V) z[t - 1] = llmk_penalty_bias_row(z[t - 1], pp->bias[j].bias);
    }
    if (pp->last_n <= 0) return;
    const int lo = llmk_penalty_window_lo(pos, pp->last_n);
    for (int q = lo; q <= pos; ++q) {
        const int t = hist[q - 1];
        if (t >= 1 && t <= V) cnt[t - 1] += 1;
    }
    for (int q = lo; q <= pos; ++q) {
        const int t = hist[q - 1];
        if (t < 1 || t > V) continue;
        const int c = cnt[t - 1];
        cnt[t - 1] = 0;
        if (c > 0) z[t - 1] = llmk_penalty_row(z[t - 1], c, pp->repeat, pp->inv_repeat, pp->frequency, pp->presence);
    }
}
#endif

#undef LLMK_HD
#endif  // LLMK_SAMPLE_PENALTY_H
