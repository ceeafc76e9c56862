// The context's scratch words: the small values that live behind the logits vectors and in the pinned "next token" block, as
// ONE set of structs that the host (llmk.hip) and the kernels (token_kernel.h) both read.  The static_asserts hold every byte
// where the kernels expect it: a field added in the wrong place fails the build.  Included by token_kernel.h, behind its TK_NCU.
#ifndef LLMK_SCRATCH_LAYOUT_H
#define LLMK_SCRATCH_LAYOUT_H

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "sample.h"
#include "sample_filter.h"

namespace llmk {

// Device words behind the V logits of d_logits (TokenArgs::err points at them).  V is even (llmk_create_tp), so they start on
// an 8-byte boundary.
struct TkDevWords {
    unsigned err;                   // sticky error word (0 = ok): token kernel, peer-memory collectives, cand_resolve_kernel
    unsigned pad0[3];
    float2 cand[2][TK_NCU];         // pipelined decode: per-CU classifier maxima {logit, 0-based row}, two buffers by position parity
    llmk_sample_params samp;        // sampling parameters of the pass / the pipelined decode (invT == 0: greedy)
    llmk_filter_params filt;        // the truncated sampler's parameters (sample_filter_kernel)
    unsigned filter_out[2];         // what sample_filter_kernel leaves for verification: rows kept, tau bits
    unsigned lp_top_n;              // the log-prob request's top_n as sample_logprob_kernel reads it (one graph serves every top_n)
    unsigned pad1[5];
};
static_assert(offsetof(TkDevWords, err) == 0 && offsetof(TkDevWords, cand) == 16, "scratch layout");
static_assert(offsetof(TkDevWords, samp) == 16 + 16 * TK_NCU && offsetof(TkDevWords, filt) == 32 + 16 * TK_NCU, "scratch layout");
static_assert(offsetof(TkDevWords, filter_out) == 64 + 16 * TK_NCU && offsetof(TkDevWords, lp_top_n) == 72 + 16 * TK_NCU, "scratch layout");
static_assert(sizeof(TkDevWords) == (24 + 4 * TK_NCU) * 4 && alignof(TkDevWords) == 8, "scratch layout");

// Host words behind the V logits of the pinned, device-mapped h_logits; ids() follow: the S ids of the pipelined decode
// (1-based, 0 = not resolved yet), written by the device through the mapped address (token_kernel.h tk_token: herr + 4 words,
// which the sizeof below holds in place)
struct TkHostWords {
    unsigned err;                   // the error word as the host sees it (direct mode, TAIL_LOGITS copy, pipelined decode)
    unsigned pf_flag;               // f16-range flag of a batched prefill / scoring call (prefill.h), read back at the end of the call
    unsigned pad[2];
    int* ids() { return reinterpret_cast<int*>(this + 1); }
};
static_assert(offsetof(TkHostWords, err) == 0 && offsetof(TkHostWords, pf_flag) == 4 && sizeof(TkHostWords) == 16, "scratch layout");

// The pinned block a GREEDY / SAMPLE / FILTER tail is read back into (llmk_ctx::h_next)
struct TkNext {
    int id;                         // 1-based id, 0 = none
    unsigned err;                   // the device's sticky error word
    int kept;                       // llmk_sample_logits: rows kept, tau (TkDevWords::filter_out, one copy of both)
    float tau;
};
static_assert(offsetof(TkNext, err) == 4 && offsetof(TkNext, kept) == 8 && offsetof(TkNext, tau) == 12 && sizeof(TkNext) == 16, "scratch layout");

// the words behind a logits vector of V floats
template <class W>
inline W* tk_words_behind(float* logits, int V) { return reinterpret_cast<W*>(logits + V); }

}  // namespace llmk

#endif  // LLMK_SCRATCH_LAYOUT_H
