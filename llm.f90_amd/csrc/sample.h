// Temperature sampling by the Gumbel-max rule (llmk_forward_sample / llmk_decode_sample).
//
//   token = 1 + argmax_i ( logits[i] * invT + g(seed, pos, i) )      first maximum wins, i 0-based
//   g     = -log(-log(u)),  u = float((w >> 8) | 1) * 2^-24          (odd / 2^24: exact in f32, never 0 or 1)
//   w     = Philox4x32-10(counter = (i >> 2, pos, 0, 0), key = (seed & 0xffffffff, seed >> 32))[i & 3]
//   invT  = f32(1 / T), rounded once on the host; pos 1-based
//
// draws token ~ softmax(logits / T) (llama2.f90:390) in exact arithmetic.  The noise is stateless, keyed by (seed, pos, row):
// every path that sees the same logits -- the persistent kernel's pipelined launches, the one-block sampling kernel behind any
// other token pass, a redone position -- picks the same token.  Everything here is plain arithmetic, no HIP API, so a host
// program compiles the same functions (tests/test_sample_cpu.py); every kernel scores through llmk_sample_score and nothing
// else, with contraction off, so the pipelined and the per-position ids are bit-identical.
#ifndef LLMK_SAMPLE_H
#define LLMK_SAMPLE_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LLMK_HD __host__ __device__ __forceinline__
#else
#define LLMK_HD static inline
#endif

struct llmk_u32x4 { uint32_t v[4]; };

LLMK_HD uint32_t llmk_mulhilo32(uint32_t a, uint32_t b, uint32_t* hi) {
    const uint64_t p = (uint64_t)a * (uint64_t)b;
    *hi = (uint32_t)(p >> 32);
    return (uint32_t)p;
}

// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants)
LLMK_HD llmk_u32x4 llmk_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        uint32_t hi0, hi1;
        const uint32_t lo0 = llmk_mulhilo32(0xD2511F53u, c0, &hi0);
        const uint32_t lo1 = llmk_mulhilo32(0xCD9E8D57u, c2, &hi1);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    }
    llmk_u32x4 o;
    o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
    return o;
}

// w: the 32 random bits of row i at position pos
LLMK_HD uint32_t llmk_sample_bits(uint64_t seed, int pos, int i) {
    const llmk_u32x4 o = llmk_philox4x32_10((uint32_t)i >> 2, (uint32_t)pos, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
    const int k = i & 3;
    return k == 0 ? o.v[0] : k == 1 ? o.v[1] : k == 2 ? o.v[2] : o.v[3];
}

// u in (0, 1): an odd multiple of 2^-24 (the conversion and the scaling are exact)
LLMK_HD float llmk_sample_u(uint32_t w) { return (float)((w >> 8) | 1u) * 5.9604644775390625e-8f; }

// g = -log(-log(u)): standard Gumbel noise, in (-2.8, 16.7)
LLMK_HD float llmk_sample_gumbel(uint32_t w) { return -logf(-logf(llmk_sample_u(w))); }

// the score of row i: logit * invT + g, rounded after each operation (never contracted to an fma)
LLMK_HD float llmk_sample_score(float logit, float invT, uint64_t seed, int pos, int i) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float g = llmk_sample_gumbel(llmk_sample_bits(seed, pos, i));
    const float s = logit * invT;
    return s + g;
}

// The sampling parameters in device memory (behind the candidate buffers of the pipelined decode: scratch_layout.h TkDevWords::samp): invT == 0 is greedy
struct llmk_sample_params {
    float invT;
    uint32_t seed_lo, seed_hi;
    uint32_t pad;
};

#undef LLMK_HD
#endif  // LLMK_SAMPLE_H
