/*
 * llmk -- C-ABI of the MI355X-native (gfx950) decode hot path of rbitr/llm.f90.
 *
 * This is the drop-in boundary.  The reference has no FFI of its own: the
 * seam is the single Fortran call
 *
 *     logits = transformer(token,pos,s,weights)            /root/reference/llama2.f90:380
 *     function transformer(token, pos, s, w) result(logits) /root/reference/llama2.f90:480-485
 *
 * plus the weights it reads (type TransformerWeights, /root/reference/weight_module.f90:13-26)
 * and the per-sequence state it mutates (type RunState, weight_module.f90:33-40, allocated at
 * llama2.f90:311-319).  A Fortran host binds these entry points with ISO_C_BINDING
 * (llm.f90_amd/host/llmk_binding.f90; the stub a reference maintainer would add is in
 * INTEGRATION.md); tests/ and bench.py bind the same symbols with ctypes.
 *
 * Conventions
 *   - plain pointers and sizes only; every function returns 0 on success, nonzero on error
 *     (a LLMK_E_* code or, above 1000, 1000 + the hipError_t).  No exceptions, no exit().
 *     The reference's own convention is print + stop (read_ggml.f90:122-125); the host does that.
 *   - token and pos are 1-BASED exactly as at llama2.f90:380 (BOS is token 2, llama2.f90:376).
 *   - weights are COPIED to the device by llmk_upload; host arrays may be freed afterwards.
 *   - array layout is the reference's: Fortran (in, rows, layer) column-major == C
 *     [layer][row][in].  No transposition anywhere.
 *   - one ctx == one sequence (KV cache inside); calls on a ctx are serialised by the caller,
 *     like the reference's non-reentrant `transformer` (it mutates `s`).
 *   - there is NO CPU fallback: without a usable HIP device llmk_create fails.
 */
#ifndef LLMK_H
#define LLMK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ggml tensor types accepted for the matmul weights (GGUF tensor-info `type`,
 * read_ggml.f90:613-635 reads 0 and 1; 2 is the q4_0 of the four_bit_dev branch). */
#define LLMK_TYPE_F32 0
#define LLMK_TYPE_F16 1
#define LLMK_TYPE_Q4_0 2
#define LLMK_TYPE_Q8_0 8 /* ggml block_q8_0 (34 bytes per 32 values): a batch's K/V caches only, see llmk_cache_create */
#define LLMK_TYPE_Q6_K 14/* ggml block_q6_K (210 bytes per 256 weights): LLMK_WCLS only, see llmk_set_tensor_type */

/* tensor ids for llmk_upload: one per component of TransformerWeights (weight_module.f90:13-26) */
#define LLMK_TOKEN_EMBEDDING_TABLE 0 /* (E,V)        C [V][E]         always f32            */
#define LLMK_RMS_ATT_WEIGHT 1        /* (E,L)        C [L][E]         f32                   */
#define LLMK_RMS_FFN_WEIGHT 2        /* (E,L)        C [L][E]         f32                   */
#define LLMK_WQKV 3                  /* (E,E+2KV,L)  C [L][E+2KV][E]  rows: Q | K | V       */
#define LLMK_WO 4                    /* (E,E,L)      C [L][E][E]                            */
#define LLMK_W13 5                   /* (E,2H,L)     C [L][2H][E]     rows: gate(w1) | up(w3) */
#define LLMK_W2 6                    /* (H,E,L)      C [L][E][H]                            */
#define LLMK_RMS_FINAL_WEIGHT 7      /* (E)                           f32                   */
#define LLMK_WCLS 8                  /* (E,V)        C [V][E]                               */
#define LLMK_N_TENSORS 9

#define LLMK_FLAG_NO_GRAPH 1 /* launch kernels eagerly instead of replaying a hipGraph          */
#define LLMK_FLAG_TIMINGS 2  /* record the reference's 5 section timers (implies NO_GRAPH)      */
#define LLMK_FLAG_MULTI_KERNEL 4 /* never use the persistent whole-token kernel (5 launches/layer) */

/* error codes */
#define LLMK_OK 0
#define LLMK_E_ARG 1       /* bad argument (null pointer, id out of range, token/pos out of range) */
#define LLMK_E_SHAPE 2     /* unsupported or inconsistent model shape                               */
#define LLMK_E_SIZE 3      /* nbytes does not match the tensor's size for its type                  */
#define LLMK_E_TYPE 4      /* unsupported ggml type                                                 */
#define LLMK_E_STATE 5     /* forward before all weights were uploaded                              */
#define LLMK_E_NODEVICE 6  /* no usable HIP device (there is no CPU fallback)                       */
#define LLMK_E_NOMEM 7
#define LLMK_E_TIMEOUT 8   /* an in-kernel exchange timed out (GPU shared with other work?)        */
#define LLMK_E_COMM 9      /* tensor-parallel ctx used before llmk_tp_init_comm, or an RCCL error       */
#define LLMK_E_VERIFY 10   /* an uploaded block's word sum on the device differed from the host's, three times over      */
#define LLMK_E_NONFINITE 11 /* llmk_forward_greedy / llmk_decode_greedy / llmk_score: no logit of the position is finite, there is no greedy token  */
#define LLMK_E_HIP 1000    /* 1000 + hipError_t                                                     */

/* Run-time replacement of the reference's compile-time dims (llama2.f90:102-108) and of
 * type Config (weight_module.f90:28-31). */
typedef struct llmk_config {
    int32_t emb_dim;     /* E  */
    int32_t hidden_dim;  /* H  */
    int32_t n_layers;    /* L  */
    int32_t n_heads;     /* nh */
    int32_t n_kv_heads;  /* nkv */
    int32_t vocab_size;  /* V  */
    int32_t seq_len;     /* S: KV-cache capacity (llama2.f90:311-313) */
    int32_t weight_type; /* LLMK_TYPE_* of wqkv/wo/w13/w2/wcls */
    int32_t device;      /* HIP device ordinal */
    int32_t flags;       /* LLMK_FLAG_* */
} llmk_config;

typedef struct llmk_ctx llmk_ctx;

/* Allocates device weights + RunState (key_cache, value_cache zeroed as at llama2.f90:316-318).
 * Replaces: the allocations at llama2.f90:311-319 and read_ggml.f90:265-410. */
int llmk_create(const llmk_config *cfg, llmk_ctx **out);

/* Tensor-parallel shard `tp_rank` of `tp_size` of the same model (for the 70B configuration,
 * where one GPU's HBM bandwidth is the limit).  Megatron split: wqkv, w13 and wcls by output rows (each rank
 * owns nkv/P kv heads and their query heads, H/P hidden rows, V/P vocabulary rows), wo and w2 by the
 * contraction dimension; per layer two all-reduces of an E-vector, one all-gather of the logits per token.
 * llmk_upload / llmk_upload_rows are handed the FULL tensors (whole layers) and keep only this rank's
 * shard.  Requires n_kv_heads, hidden_dim, vocab_size divisible by tp_size.  One process per GPU:
 * rank 0 calls llmk_tp_unique_id, ships the 128 bytes to the other ranks (any side channel), every rank
 * calls llmk_tp_init_comm; after that llmk_forward / llmk_forward_greedy run the collectives over RCCL. */
int llmk_create_tp(const llmk_config *cfg, int tp_rank, int tp_size, llmk_ctx **out);
int llmk_tp_unique_id(char id_out[128]);
int llmk_tp_init_comm(llmk_ctx *ctx, const char id[128]);

/* The same three collectives as ONE-SHOT exchanges over peer memory (xGMI is a full mesh: every rank writes its partial
 * E-vector straight into every peer's inbox and adds the P partials in rank order -- one hop instead of a ring's
 * 2(P-1); csrc/tp_p2p.h).  Each rank exports its inbox with llmk_tp_p2p_handle (64 bytes, a hipIpcMemHandle_t), the host
 * ships the P handles to every rank (any side channel: files, MPI, torch.distributed) and each rank calls
 * llmk_tp_p2p_connect with all of them, `handles` = tp_size * 64 bytes in rank order (its own entry is ignored).  Ranks
 * that live in ONE process (one host thread per GPU) connect with llmk_tp_p2p_connect_local instead: `ranks[r]` = rank r's
 * ctx.  After either call llmk_forward / llmk_forward_greedy run the token pass with these collectives (the RCCL
 * communicator, if any, is then unused).  All ranks must call llmk_forward for the same token and position. */
int llmk_tp_p2p_handle(llmk_ctx *ctx, char handle_out[64]);
int llmk_tp_p2p_connect(llmk_ctx *ctx, const char *handles);
int llmk_tp_p2p_connect_local(llmk_ctx *ctx, llmk_ctx *const *ranks);
/* Prove the peer-memory path on the hardware it runs on before the first token (all ranks call it together, after the
 * connect): `iters` rounds of both all-reduce halves and the all-gather on known integers, with the real kernels and
 * their bounded spins.  0 = this rank saw only correct sums; LLMK_E_TIMEOUT / LLMK_E_COMM / a HIP code otherwise.  The
 * host gathers the ranks' verdicts over its side channel; unless ALL are 0, every rank calls llmk_tp_p2p_disable and
 * llmk_tp_init_comm, and the token pass runs over RCCL (what `llm --ngpu` and `bench.py --tp` do). */
int llmk_tp_p2p_selftest(llmk_ctx *ctx, int iters);
/* Verification only: the self-test's rounds with pseudo-random delays (seeded by `seed`) injected before and between the
 * sends and the reads of every exchange, so that ranks and wavefronts drift apart by up to a whole exchange -- what a slower
 * link or a time-sliced GPU does to them.  Same verdicts as the self-test; all ranks call it together. */
int llmk_tp_p2p_stress(llmk_ctx *ctx, int iters, unsigned seed);
int llmk_tp_p2p_disable(llmk_ctx *ctx);

/* Single-process stepping of a tensor-parallel ctx, for verification on one GPU (no communicator): the
 * caller plays the collective.  llmk_tp_begin sets token/pos; llmk_tp_segment runs
 *   seg 0 (layer l):  [l>0: x += exchanged]  rmsnorm+qkv, attention, wo   -> partial E-vector
 *   seg 1 (layer l):  x += exchanged          rmsnorm+w1|w3, w2            -> partial E-vector
 *   seg 2:            x += exchanged          final rmsnorm + classifier   -> this rank's V/P logits
 * llmk_tp_read_partial / llmk_tp_write_partial move the E-vector (the caller sums the ranks' partials in
 * rank order and writes the sum back to every rank); llmk_tp_read_logits returns the rank's logits slice. */
int llmk_tp_begin(llmk_ctx *ctx, int token, int pos);
int llmk_tp_segment(llmk_ctx *ctx, int seg, int layer);
int llmk_tp_read_partial(llmk_ctx *ctx, float *out);
int llmk_tp_write_partial(llmk_ctx *ctx, const float *in);
int llmk_tp_read_logits(llmk_ctx *ctx, float *out_slice);

/* Copy one whole TransformerWeights component to the device.  `host` points at the first
 * element of the Fortran array (c_loc(w%wqkv) ...); nbytes must equal the full array size for
 * `ggml_type` (f32: 4 B/weight, f16: 2 B/weight, q4_0: 18 B per 32 weights along `in`).
 * Norm gains and the embedding table must be f32.  Replaces nothing in the reference (it has no
 * device); called once after load_ggml returns (llama2.f90:151). */
int llmk_upload(llmk_ctx *ctx, int tensor_id, const void *host, size_t nbytes, int ggml_type);

/* Same, for `rows` consecutive rows of layer `layer` starting at `row_offset` (lets a loader
 * stream one GGUF tensor at a time, e.g. attn_k into rows E..E+KV-1 of wqkv, read_ggml.f90:286,
 * without materialising the fused array on the host).  Rows and offsets are those of the FULL tensor on a
 * tensor-parallel ctx too: the shim keeps the part of the range its shard holds (possibly nothing), so a rank may hand
 * over whole layers or only its own rows (host/gguf_loader.f90 stream_ggml_matrices reads nothing else from the file). */
int llmk_upload_rows(llmk_ctx *ctx, int tensor_id, int layer, int row_offset, int rows, const void *host,
                     size_t nbytes, int ggml_type);

/* Extensions beyond the reference's behaviour, both OPT-IN (the defaults reproduce llama2.f90):
 *  - llmk_set_tensor_type: give LLMK_WCLS its own ggml type (f32 / f16 / q4_0 / q6_K) before it is uploaded -- stock llama.cpp
 *    q4_0 files keep output.weight in q6_K (the reference stops on it, read_ggml.f90:633-635, :682-684).  Round 6: the raw q6_K
 *    super-blocks are uploaded as they lie in the file (LLMK_TYPE_Q6_K, emb_dim a multiple of 256) and dotted on the device; a
 *    ctx with q4_0 matrices of a shape the persistent kernel serves STAYS on it (llmk_path == 1).  A host may still hand the
 *    classifier over dequantised (LLMK_TYPE_F32): that ctx runs the multi-kernel path, as before;
 *  - llmk_set_rms_eps: rmsnorm epsilon other than the reference's hard-coded 1e-5 (llama2.f90:454), for a host that
 *    honours llama.attention.layer_norm_rms_epsilon. */
int llmk_set_tensor_type(llmk_ctx *ctx, int tensor_id, int ggml_type);
int llmk_set_rms_eps(llmk_ctx *ctx, float eps);

/* RoPE frequency table, n = head_size/2 floats: freqs[j] = 1/10000**((2j+1)/head_size), computed
 * by the HOST with the reference's own expression (llama2.f90:544-545) so the device angle
 * pos*freq starts from bit-identical frequencies.  Optional: llmk_create installs the same
 * table computed with powf. */
int llmk_set_rope_freqs(llmk_ctx *ctx, const float *freqs, int n);

/* The hot path: one token through the whole stack.  Replaces
 * `logits = transformer(token,pos,s,weights)` (llama2.f90:380).  token in [1,V], pos in [1,S],
 * both 1-based; positions must be fed in order 1,2,3,... (each call appends to the KV cache at
 * pos, llama2.f90:564-565).  logits_out: V floats, caller-owned host memory. */
int llmk_forward(llmk_ctx *ctx, int token, int pos, float *logits_out);

/* llmk_forward keeps the next greedy position in flight: once a caller has fed back the first maximum of
 * the logits it received twice in a row, the launch for position pos + 1 is enqueued on the device's own greedy token before
 * the call for pos returns, and a call that comes back with exactly that token and position finds its result under way; any other
 * call drains the stream and runs as if nothing had been launched.  What a call returns does not change.  Whole-model f32 / f16
 * contexts on the persistent kernel only; LLMK_FORWARD_AHEAD=0 in the environment at llmk_create switches it off.
 * out = {speculative launches, hits, misses, 1 while a launch is in flight} since llmk_create. */
int llmk_forward_ahead_stats(llmk_ctx *ctx, int out[4]);

/* The prompt loop of llama2.f90:376-402 as ONE call: tokens[0..n) (1-based ids) sit at
 * positions pos0 .. pos0+n-1 (1-based); their KV-cache rows are written and logits_out[vocab_size] receives the
 * logits of the LAST position -- what n llmk_forward calls would leave behind, within the 1e-4 parity bar (only the
 * order of the dot-product partial sums differs).  single-GPU contexts (f32, f16, q4_0) batch up to 128 positions per pass
 * through MFMA GEMMs (a layer's weights cross HBM once per batch); tensor-parallel contexts, and shapes whose emb_dim /
 * hidden_dim is not a multiple of the GEMM's 64-column step, run the token-by-token pass inside.
 * The GEMMs multiply on the f16 matrix instruction with each f32 activation (and each f32 / q4_0 weight) as two f16 pieces
 * (exact products; |error| <= 2^-20 of an operand of magnitude >= 2^-3, 2^-24 absolute below: csrc/prefill.h); a prompt with an activation of magnitude >= 65504, or with a position whose whole row is below 2^-7, is redone on the
 * f32 instruction inside the same call, and the context stays there.  LLMK_PF_F32_MFMA=1 in the environment selects the
 * f32 instruction from the start. */
int llmk_prefill(llmk_ctx* ctx, const int* tokens, int n, int pos0, float* logits_out);

/* Scoring: llmk_prefill's pass with the classifier and a log-softmax for EVERY position, on the device (DESIGN.md
 * section 3h).  tokens, n, pos0: exactly as for llmk_prefill (same checks, same KV-cache rows written, decode may continue
 * behind it).  With z = the vocab_size logits of position pos0+i:
 *   logprob_out[i] = z[targets[i]-1] - lse(z),  lse(z) = m + log(sum_j exp(z[j] - m)),  m = max_j z[j],  for targets[i] in
 *                    [1, vocab_size]; targets[i] == 0 means "no target here" and gives 0.0f; any other value is LLMK_E_ARG
 *                    before anything runs.  targets may be NULL only if logprob_out is NULL;
 *   argmax_out[i]  = the 1-based first maximum of z (the rule of llmk_forward_greedy, llama2.f90:388);
 *   logits_out[i*vocab_size .. (i+1)*vocab_size) = z.
 * Each of the three outputs may be NULL (what is not asked for is not copied); all three NULL is LLMK_E_ARG.  A position none of
 * whose logits is finite: LLMK_E_NONFINITE (on any error the contents of the outputs are unspecified).  All arithmetic is f32 in a fixed reduction order (llm.f90_amd/csrc/score.h): two
 * calls with the same input on the same context return bit-identical outputs, whichever outputs are asked for.  Contexts that
 * take llmk_prefill's batched path run the classifier as a GEMM over each batch of 128 positions.
 *   An f32, f16 or q4_0 classifier whose vocab_size is not a multiple of 4: the whole call goes token by token inside (said once on stderr).
 *   A q6_K classifier never goes token by token.  It takes the GEMM too, except in three cases, in which the decode classifier runs once
 *   per row of the batch instead: on the f32 matrix instruction (LLMK_PF_F32_MFMA=1, or after an f16-range flag); with a vocab_size that
 *   is not a multiple of 4; in a batch of fewer rows than the crossover.  llmk_cls_form tells which form a batch takes.
 *   The f16-range flag covers the q6_K weights as well: a weight of magnitude >= 65504 or a non-finite super-block scale d raises it, the
 *   call is redone on the f32 instruction, and the note on stderr is the one for activations ("an activation beyond the f16 range").
 * The logits are within the parity bar of llmk_forward's, not bit-identical to them. */
int llmk_score(llmk_ctx *ctx, const int *tokens, int n, int pos0, const int *targets, float *logprob_out, int *argmax_out,
               float *logits_out);

/* Same pass, but the temperature-0 consumer (`token = maxloc(logits,DIM=1)`, llama2.f90:388) runs
 * on the device: returns the 1-based argmax (first maximum wins) and skips the logits copy.
 * SURVEY.md section 8(f) rank 1. */
int llmk_forward_greedy(llmk_ctx *ctx, int token, int pos, int *next_token);

/* The temperature-0 generation loop of llama2.f90:379-396 for n positions in ONE call, without a host round trip per
 * token: position pos0 is fed `token`, every later position the device argmax (first maximum wins, llama2.f90:388) of the
 * position before it.  ids_out[i] = the 1-based token chosen after position pos0+i (= what llmk_forward_greedy returns
 * there).  On the persistent-kernel path the n launches are enqueued back to back: each launch leaves the per-CU maxima
 * of its classifier rows in device memory and the next one folds them at its start, so the token never leaves the
 * device; ids reach the host through mapped memory as they are resolved, and on_token (optional) is called from the
 * calling thread, in order, as each arrives -- the host can stream the text exactly as llama2.f90:396 does.  Other
 * contexts run the same positions through llmk_forward_greedy.  The logits of every position are still computed and
 * written (device memory); only their trip to the host is dropped.  SURVEY.md section 8(f) rank 1. */
typedef void (*llmk_token_fn)(int index, int token, void *user);
int llmk_decode_greedy(llmk_ctx *ctx, int token, int pos0, int n, int *ids_out, llmk_token_fn on_token, void *user);

/* The sampling twins of llmk_forward_greedy / llmk_decode_greedy: the consumer at temperature T > 0
 * (`token ~ softmax(logits / T)`, llama2.f90:390) runs on the device, by the Gumbel-max rule
 *
 *     token = 1 + argmax_i ( logits[i] * invT + g(seed, pos, i) )      first maximum wins, i 0-based
 *     g     = -log(-log(u)),  u = float((w >> 8) | 1) * 2^-24          (odd / 2^24: exact in f32, never 0 or 1)
 *     w     = Philox4x32-10(counter = (i >> 2, pos, 0, 0), key = (seed & 0xffffffff, seed >> 32))[i & 3]
 *     invT  = f32(1 / T), rounded once on the host; pos 1-based (the position whose logits are sampled)
 *
 * (each product and sum rounded to f32; llm.f90_amd/csrc/sample.h holds the arithmetic).  In exact arithmetic this
 * draws from exactly the reference's distribution; it is NOT draw-for-draw the reference's random_number stream.  The
 * noise is stateless, keyed by (seed, pos, row): the pipelined launches of llmk_decode_sample, a chain of
 * llmk_forward_sample calls, the multi-kernel path and a redone position all pick the same token from the same logits,
 * so a transcript is a function of (model, prompt, T, seed).  Positions, callbacks, streaming and errors are those of
 * the greedy functions (LLMK_E_NONFINITE when no score is above -inf).  temperature must be finite and > 0 with 1/T a
 * normal f32, otherwise LLMK_E_ARG (temperature 0 is the greedy functions' job). */
int llmk_forward_sample(llmk_ctx *ctx, int token, int pos, float temperature, uint64_t seed, int *next_token);
int llmk_decode_sample(llmk_ctx *ctx, int token, int pos0, int n, float temperature, uint64_t seed,
                       int *ids_out, llmk_token_fn on_token, void *user);

/* The same two with the truncations stock llama.cpp files are sampled with: top-k, top-p (nucleus) and min-p in front of the
 * Gumbel-max draw (llm.f90_amd/csrc/sample_filter.h holds the rule).  With z the logits of the position
 * (-0.0 counts as +0.0), s[i] = z[i] * invT, m = max s, e[i] = expf(s[i] - m), Q[i] = (uint64) floorf(e[i] * 2^32):
 *   top_k  >= 1 (0 = off; so is top_k >= the number of non-NaN rows): tau_k = the k-th largest logit counting duplicates; rows that
 *          tie with it are ALL kept, so more than k rows may be (the rule knows no index order);
 *   top_p  in (0, 1) (exactly 1 = off): with S = sum of Q[j] over z[j] >= tau_k and G(t) = sum of Q[j] over z[j] > t, row i is kept
 *          iff (double)G(z[i]) < (double)top_p * (double)S -- the nucleus of the distribution after top-k, renormalised over it;
 *          integer sums: exact, whatever the order of the additions.  The row of the maximum is always kept;
 *   min_p  in [0, 1] (0 = off): row i is kept iff e[i] >= min_p;
 *   token = 1 + argmax over the kept rows of the score above (the same stateless noise, first maximum wins): a draw from the
 *          distribution renormalised over the kept rows.
 * All three are monotone in z: the kept set is { i : z[i] >= tau }, tau the largest of the three thresholds.  NaN and -inf rows are
 * never kept; a maximum of +inf keeps the rows equal to it; no row above -inf is LLMK_E_NONFINITE.  top_k < 0, top_p outside (0, 1],
 * min_p outside [0, 1] or a NaN: LLMK_E_ARG before anything runs; temperature as above.  With all filters off the two functions ARE
 * llmk_forward_sample / llmk_decode_sample (same code path, same ids).  With a filter on, one more one-workgroup kernel runs per
 * position (behind each launch of the pipelined decode, which stays pipelined: the token still never leaves the device); every path
 * runs that one kernel, so pipelined and per-position ids are bit-identical. */
typedef struct llmk_sampler {
    float temperature;
    int32_t top_k;
    float top_p;
    float min_p;
    uint64_t seed;
} llmk_sampler;
int llmk_forward_sample_ex(llmk_ctx *ctx, int token, int pos, const llmk_sampler *sampler, int *next_token);
int llmk_decode_sample_ex(llmk_ctx *ctx, int token, int pos0, int n, const llmk_sampler *sampler, int *ids_out,
                          llmk_token_fn on_token, void *user);
/* Verification hook, like llmk_peek: the rule applied by the same kernel to caller-supplied logits (vocab_size floats, host
 * memory) as if they were those of position `pos` -- no token pass, the KV cache is untouched.  token_out = the 1-based pick;
 * kept_out (optional) = the number of rows kept; tau_out (optional) = the threshold (-inf with all filters off).
 * The ctx's logits buffer is overwritten with `logits`: what llmk_forward left there is gone, so a following llmk_peek of the
 * logits (or any other read of them) sees the caller's vector, not the last position's.  The ctx must hold all its tensors
 * (LLMK_E_STATE otherwise) and be a whole-model one: a tensor-parallel rank gives LLMK_E_ARG. */
int llmk_sample_logits(llmk_ctx *ctx, const float *logits, int pos, const llmk_sampler *sampler, int *token_out, int *kept_out,
                       float *tau_out);

/* The same three with what stock llama.cpp files are further sampled with: the repetition, frequency and presence penalties over a
 * window of the tokens fed so far, and a logit bias (llm.f90_amd/csrc/sample_penalty.h holds the rule).  With z
 * the logits of position pos, r = repeat, inv_r = f32(1 / r) rounded once, f = frequency, p = presence, W = the tokens fed at positions
 * max(1, pos - last_n + 1) .. pos according to the context's token record (below; entries 0 = "none" are skipped) and c[t] = how often
 * token t occurs in W, each product, sum and difference rounded to f32:
 *   1. bias:       z[t] <- z[t] + b for every entry (t, b) of the bias list; b = -inf bans the token;
 *   2. penalties:  for every t with c[t] > 0:  z[t] <- (z[t] > 0 ? z[t] * inv_r : z[t] * r), then z[t] <- z[t] - ((float)c[t] * f + p);
 *                  a NaN row stays NaN, a -inf row stays -inf, -0.0 takes the `<= 0` branch;
 *   3. the adjusted vector goes through the rule of llmk_*_sample_ex unchanged (filters, Gumbel-max, first maximum wins, the same
 *      stateless noise keyed by (seed, pos, row)).
 * Bias comes before the penalties on a row that gets both (llama.cpp's order).  The product with inv_r instead of llama.cpp's division
 * by r is deliberate: the adjusted logits are a bit-exact function that float32 arithmetic reproduces anywhere; they differ from
 * llama.cpp's by at most 1 ulp.  top_k = 1 is the greedy form: the maximum of the adjusted logits.  Temperature 0 stays LLMK_E_ARG,
 * as in the _ex functions.
 *
 * The token record: S = seq_len ints on the device, hist[q-1] = the 1-based token fed at position q, 0 = none; zero when it is
 * allocated (by the first call that needs it: a context that never uses these functions allocates nothing) and after llmk_reset.  It is
 * indexed by position: a redone position rewrites its own entry.  llmk_forward, llmk_prefill, llmk_score, the greedy functions and
 * the _ex functions do NOT maintain it: the caller records the prompt once with llmk_set_history (tokens fed at pos0 .. pos0+n-1, 0
 * allowed = none), and llmk_forward_sample_pen / llmk_decode_sample_pen record every token they are fed from there (the pipelined
 * decode on the device, from the id the sampler left there).  llmk_get_history reads it back (verification).
 *
 * Out of range -- last_n < 0 or > seq_len; repeat not finite, <= 0 or with 1/repeat beyond the normal f32 range; frequency or
 * presence not finite; n_bias outside [0, LLMK_MAX_LOGIT_BIAS]; a bias that is NaN or +inf; a bias id outside [1, vocab_size] or given
 * twice: LLMK_E_ARG before anything runs.  The sampler is checked as in the _ex functions.  With nothing on (n_bias == 0, and last_n ==
 * 0 or repeat == 1, frequency == 0, presence == 0) the two functions ARE llmk_forward_sample_ex / llmk_decode_sample_ex: same code
 * path, same ids, and the record is NOT maintained.  Otherwise one more one-workgroup kernel (sample_penalty_kernel) runs per position
 * in front of the filter kernel, which then always runs; the pipelined decode stays pipelined, and every path -- the pipelined
 * launches, the per-position pass, LLMK_FLAG_MULTI_KERNEL, a redone position -- runs the same two kernels, so the ids are
 * bit-identical across them.  The context's logits buffer holds the ADJUSTED logits afterwards.  A tensor-parallel context gets what
 * the _ex functions give it.
 * llmk_sample_logits_pen is the verification hook, with the limits of llmk_sample_logits (whole-model contexts only; the logits buffer
 * is overwritten, here with the adjusted vector): it READS the window from the record, positions up to and including `pos` (so pos <=
 * seq_len), and does not write the record.  adjusted_out (optional): the vocab_size adjusted logits. */
#define LLMK_MAX_LOGIT_BIAS 256
typedef struct llmk_logit_bias { int32_t token; float bias; } llmk_logit_bias;   /* token 1-based */
typedef struct llmk_penalties {
    int32_t last_n;      /* window in positions, 0 = penalties off, at most seq_len */
    float repeat;        /* 1 = off; finite, > 0, 1/repeat a normal f32 */
    float frequency;     /* 0 = off; finite */
    float presence;      /* 0 = off; finite */
    const llmk_logit_bias *bias; int32_t n_bias;   /* 0..LLMK_MAX_LOGIT_BIAS; bias finite or -inf; token ids distinct, in [1, V] */
} llmk_penalties;
int llmk_set_history(llmk_ctx *ctx, const int *tokens, int n, int pos0);
int llmk_get_history(llmk_ctx *ctx, int *tokens_out, int n, int pos0);
int llmk_forward_sample_pen(llmk_ctx *ctx, int token, int pos, const llmk_sampler *sampler, const llmk_penalties *penalties, int *next_token);
int llmk_decode_sample_pen(llmk_ctx *ctx, int token, int pos0, int n, const llmk_sampler *sampler, const llmk_penalties *penalties,
                           int *ids_out, llmk_token_fn on_token, void *user);
int llmk_sample_logits_pen(llmk_ctx *ctx, const float *logits, int pos, const llmk_sampler *sampler, const llmk_penalties *penalties,
                           int *token_out, int *kept_out, float *tau_out, float *adjusted_out);

/* Decode log-probs: what the model thought of the tokens a sampling call returned (llama.cpp's --n-probs, the `logprobs` /
 * `top_logprobs` of the serving APIs), computed on the device behind the kernel that picked each token (csrc/logprob.h,
 * sample_logprob_kernel).  With z the vocab_size RAW logits of a position -- what the classifier wrote, before
 * bias, penalties, temperature and truncation, i.e. what llmk_score reports for the same tokens -- and L their log-sum-exp:
 *   token_logprob[i]         = z[id - 1] - L for the id returned for position i;
 *   top_tokens[i*top_n + j],
 *   top_logprobs[i*top_n + j] = the j-th row in the order z descending, then index ascending (-0.0 and +0.0 tie), over the rows with
 *                              z > -inf that are not NaN: {1-based id, z - L}; {0, -inf} where fewer than top_n such rows exist.
 * A +inf or NaN logit adds no error of its own: L and the values are then what the arithmetic of csrc/score.h gives in the kernel's
 * order -- NaN, except that a NaN which is the first row of a thread's chain is dropped (an empty log-sum-exp state ignores what it
 * holds), so at vocab_size <= 1024 NaN rows do not reach L at all; the ids are defined either way.  LLMK_E_NONFINITE stays what the
 * greedy and sampling functions make of it.
 *
 * sampler == NULL is the greedy form -- the rule of llmk_forward_greedy / llmk_decode_greedy, first maximum wins; penalties must then
 * be NULL as well.  Otherwise sampler and the optional penalties (NULL = none) mean exactly what they mean to the _pen functions, and
 * the ids ARE the ids those return for the same arguments: same kernels, same noise, the token record kept by the same rule.
 * LLMK_E_ARG before anything runs or is allocated: logprobs == NULL; top_n outside [0, LLMK_MAX_TOP_LOGPROBS]; nothing asked for (top_n
 * == 0 and token_logprob == NULL); a NULL array that top_n needs; a tensor-parallel context.  The arrays (n = 1 for
 * llmk_forward_sample_lp) are complete when the call returns; on_token keeps its signature and its timing; on any error the arrays are
 * unspecified.  The pipelined decode stays pipelined: one more one-workgroup kernel per position, the records read back in one copy
 * at the end of the call.  Under penalties the context's logits buffer still holds the ADJUSTED vector afterwards.
 * llmk_logprob_logits is the verification hook, with the limits of llmk_sample_logits (whole-model contexts only; the context's logits
 * buffer is overwritten; no token pass): the same kernel on the caller's logits, for `token` in [0, vocab_size] (0: none,
 * *token_logprob = 0.0f).  token_logprob may be NULL when top_n > 0. */
#define LLMK_MAX_TOP_LOGPROBS 20
typedef struct llmk_logprobs {
    int32_t top_n;          /* 0..LLMK_MAX_TOP_LOGPROBS alternatives per position */
    float *token_logprob;   /* n floats, or NULL */
    int32_t *top_tokens;    /* n * top_n ints (1-based, 0 = none); NULL iff top_n == 0 */
    float *top_logprobs;    /* n * top_n floats; NULL iff top_n == 0 */
} llmk_logprobs;
int llmk_forward_sample_lp(llmk_ctx *ctx, int token, int pos, const llmk_sampler *sampler, const llmk_penalties *penalties,
                           const llmk_logprobs *logprobs, int *next_token);
int llmk_decode_sample_lp(llmk_ctx *ctx, int token, int pos0, int n, const llmk_sampler *sampler, const llmk_penalties *penalties,
                          const llmk_logprobs *logprobs, int *ids_out, llmk_token_fn on_token, void *user);
int llmk_logprob_logits(llmk_ctx *ctx, const float *logits, int token, int top_n, float *token_logprob, int32_t *top_tokens,
                        float *top_logprobs);

/* Batched decode: several sequences go through ONE pass over the weights.  A batch belongs to a context and
 * runs on its weights (nothing is uploaded twice); it owns K/V caches [n_layers][n_slots][seq_len][kv_dim] (f32, zeroed) for n_slots
 * sequences ("slots", numbered from 0).  The context's own sequence and every other entry point are untouched.  A pass runs on the
 * context's stream through the context's prefill workspaces: calls on a batch and calls on its context must be serialised by the
 * caller, as all calls on a context already are.  The layers' weights and the classifier cross HBM once per pass.  A q6_K classifier
 * (a stock llama.cpp q4_0 file's output.weight) is read once per ROW of the pass in three cases only: on the f32 matrix instruction
 * (LLMK_PF_F32_MFMA=1, or after an f16-range flag), with a vocab_size that is not a multiple of 4, and in a pass of fewer rows than the
 * crossover where the per-row form is the faster one (llmk_cls_form tells which form a pass takes).
 *
 * create:  n_slots in [1, LLMK_MAX_BATCH], seq_len in [1, the context's seq_len], else LLMK_E_ARG.  LLMK_E_SHAPE for a context the
 *          batched pass does not serve -- tensor-parallel, emb_dim or hidden_dim not a multiple of 64, kv_dim not a multiple of 16,
 *          more than 16 query heads per kv head, a classifier no row chunk of which fits the pass's workspace.  There is NO
 *          token-by-token fallback (LLMK_PREFILL=0 does not apply).  LLMK_E_STATE before all tensors are uploaded, whatever the
 *          shape.  llmk_destroy of a context with live batches is LLMK_E_STATE: destroy the batches first.
 * fork:    copies the K/V rows of positions 1..n_pos of every layer from the CONTEXT's own cache (filled by llmk_prefill /
 *          llmk_forward) into `slot`; n_pos in [0, min(batch seq_len, context seq_len)], 0 empties the slot.  N completions of one
 *          prompt: prefill once, fork N times.
 * forward: one pass.  Row i feeds tokens[i] (1-based) at position pos[i] (1-based, <= the batch's seq_len) of slot slots[i]: that
 *          slot's K/V row pos[i] is written and the row attends over the slot's rows 1..pos[i].  n in [1, n_slots], slots distinct,
 *          else LLMK_E_ARG before anything runs; the rows' positions are unrelated.  logits_out [n][vocab_size] in row order,
 *          argmax_out [n] the 1-based first maximum (the rule of llmk_forward_greedy); either may be NULL, both NULL is LLMK_E_ARG.
 *          A row with no finite logit: LLMK_E_NONFINITE.  The f16-range rule of llmk_prefill applies (the call is redone on the f32
 *          matrix instruction, its K/V rows rewritten).
 * decode:  `steps` passes with no host round trip between them: ids_out[i*steps + s] is the id picked for row i after position
 *          pos0[i]+s, fed to that row at pos0[i]+s+1 from device memory.  pos0[i]+steps-1 <= seq_len and everything forward checks,
 *          up front.  samplers NULL: greedy.  Else samplers[i] is row i's own llmk_sampler -- temperature, seed, top_k, top_p, min_p,
 *          with the meaning and the checks of llmk_forward_sample_ex -- and the pick is DEFINED as what llmk_sample_logits answers for that
 *          row's logits, that position and that sampler: the same kernel body reads the same bits, in ONE launch per step with a
 *          workgroup per row of the pass (sample_filter_rows_kernel).  Penalties, logit bias and log-prob
 *          records are out of scope of this function: llmk_rows_decode, below, takes them.
 * time:    measurement hook: average milliseconds of one full pass (classifier and greedy pick included) of n rows, slots 0..n-1,
 *          all at position pos.  It OVERWRITES those slots' row pos: fork or refill the slots afterwards.
 * The same call on the same state returns bit-identical outputs.  A row's logits are within the 1e-4 parity bar of llmk_forward's on
 * that sequence alone, and across different batch compositions (the GEMM tiling follows the row count), not bit-identical. */
typedef struct llmk_batch llmk_batch;
#define LLMK_MAX_BATCH 128            /* rows of one pass */
int llmk_batch_create(llmk_ctx *ctx, int n_slots, int seq_len, llmk_batch **out);
int llmk_batch_destroy(llmk_batch *b);
int llmk_batch_fork(llmk_batch *b, int slot, int n_pos);
int llmk_batch_forward(llmk_batch *b, int n, const int *slots, const int *tokens, const int *pos, float *logits_out, int *argmax_out);
int llmk_batch_decode(llmk_batch *b, int n, const int *slots, const int *tokens, const int *pos0, int steps,
                      const llmk_sampler *samplers, int *ids_out);
int llmk_batch_time(llmk_batch *b, int n, int pos, int iters, float *avg_ms);

/* The rows functions: what a context's _pen and _lp functions do for one sequence, for the rows of a batch.
 * ("rows" are the sequences of one pass; the family is not named after the batch only because the list above is closed.)  Each of the
 * three sampler kernels has a rows form with one workgroup per row of the pass, so a step of a decode is ONE launch of each kernel it
 * needs, however many rows it has.  Indexing: logits, samplers, penalties, picks and log-prob records are per ROW i of the call;
 * the token records and the penalty kernel's counts are per SLOT -- a sequence keeps its record whichever row of a call it is.
 *
 * State, all allocated by the first call that needs it (a batch that never uses these functions allocates nothing): a token record per
 * slot, [n_slots][seq_len] ints with the meaning of a context's (hist[q-1] = the 1-based token fed at position q, 0 = none; zero when
 * allocated); llmk_batch_fork zeroes the record of the slot it fills or empties, if the batch has records: a forked slot is a new
 * sequence, and the caller records its prompt with llmk_rows_set_history exactly as a context's caller does with llmk_set_history.
 * set_history / get_history: llmk_set_history / llmk_get_history for `slot` in [0, n_slots), ranges against the BATCH's seq_len.
 *
 * decode:  everything llmk_batch_decode checks and does.  samplers NULL: greedy, else [n].  penalties NULL: none, else [n], entry i
 *          meaning to row i what it means to llmk_decode_sample_pen, with the same checks (last_n at most the batch's seq_len; bias ids
 *          distinct and in [1, vocab_size]); with samplers NULL it must be NULL.  logprobs NULL: none, else ONE request for the call
 *          by the rules of llmk_decode_sample_lp (the greedy form with records is allowed): top_n is shared by all rows,
 *          token_logprob[i*steps + s] belongs to ids_out[i*steps + s], top_tokens and top_logprobs are indexed
 *          [(i*steps + s)*top_n + j].
 *          DEFINITION: ids_out[i*steps + s] is what llmk_sample_logits_pen answers on the context for row i's logits of that step,
 *          position pos0[i]+s, row i's sampler and penalties, with the context's record holding that slot's record; the log-prob
 *          record is what llmk_logprob_logits answers for the RAW logits and that id.  The same kernel bodies read the same bits.
 *          If penalties is given and at least one row has something on (a bias, or last_n > 0 with a penalty that is not neutral),
 *          the record of EVERY row of the call is maintained: the fed token is written at its position at every step, on the
 *          device.  With nothing on in any row, or penalties NULL, the call is the one without penalties and no record is touched
 *          (the context's rule).  With penalties and logprobs both NULL the call IS llmk_batch_decode: same code path, same ids.
 *          The f16-range rule applies: a redone call rewrites the same record entries (records are indexed by position).
 *          LLMK_E_NONFINITE as in llmk_batch_decode; the arrays are then unspecified.
 * sample_logits: the verification hook, like llmk_sample_logits_pen for a context: no pass, no K/V; it READS the slots' records
 *          (positions up to and including pos[i], so pos[i] <= the batch's seq_len) and writes none.  The caller's logits
 *          [n][vocab_size] overwrite the batch's logits rows.  samplers is required (NULL: LLMK_E_ARG); penalties and logprobs are
 *          optional.  tokens_out [n] is required; kept_out [n], tau_out [n] and adjusted_out [n][vocab_size] are optional; the
 *          log-prob arrays are filled as by a decode of one step, for the id the row picked.  A row with no row above -inf gives the
 *          call LLMK_E_NONFINITE: the outputs are then unspecified and the batch stays usable.
 * A NULL batch is LLMK_E_ARG before anything touches a device, in all four. */
int llmk_rows_set_history(llmk_batch *b, int slot, const int *tokens, int n, int pos0);
int llmk_rows_get_history(llmk_batch *b, int slot, int *tokens_out, int n, int pos0);
int llmk_rows_decode(llmk_batch *b, int n, const int *slots, const int *tokens, const int *pos0, int steps,
                     const llmk_sampler *samplers, const llmk_penalties *penalties, const llmk_logprobs *logprobs, int *ids_out);
int llmk_rows_sample_logits(llmk_batch *b, int n, const int *slots, const int *pos, const float *logits,
                            const llmk_sampler *samplers, const llmk_penalties *penalties, const llmk_logprobs *logprobs,
                            int *tokens_out, int *kept_out, float *tau_out, float *adjusted_out);

/* A shared prefix: N completions of one prompt without N copies of its K/V rows.  A batch can hold ONE prefix,
 * a single copy [n_layers][P][kv_dim] (f32) of the K/V rows of positions 1..P; slots are ATTACHED to it.  An attached slot is a
 * sequence whose positions 1..P are the prefix and whose positions P+1.. live in the slot's own cache, still at cache row pos - 1.  In a
 * pass the prefix rows are read once per group of 16 / (query heads per kv head) attached rows, not once per row.  ("prefix", not
 * "batch": the llmk_batch_* list is closed.)
 *
 * set:     copies positions 1..n_pos of every layer from the CONTEXT's own cache into the batch's prefix.  A snapshot: later calls on
 *          the context do not change it.  n_pos in [0, min(batch seq_len, context seq_len) - 1] (an attached row needs a position of
 *          its own), else LLMK_E_ARG; 0 drops the prefix.  LLMK_E_STATE while any slot is attached.  The prefix, the column map, the
 *          slots' `first` words and the part-state buffers of such passes are allocated by the first call that sets a prefix: a batch
 *          that never does allocates and launches exactly what it did without these functions.
 * attach:  LLMK_E_STATE without a prefix, LLMK_E_ARG for a slot out of range.  The slot becomes a new sequence behind the prefix: its
 *          own cache rows are zeroed, and its token record if the batch has records, as llmk_batch_fork does (the caller records the
 *          prompt with llmk_rows_set_history, as after a fork).  llmk_batch_fork on an attached slot detaches it: a forked slot is
 *          self-contained.
 * len:     P, 0 for no prefix, a negative LLMK_E_* on error (as llmk_path).
 * A NULL batch is LLMK_E_ARG before anything touches a device, in all three.
 * llmk_batch_forward, llmk_batch_decode, llmk_rows_decode, llmk_rows_sample_logits and llmk_batch_time take attached slots like any
 * other, with one more check up front: a row of an attached slot must have pos > P, else LLMK_E_ARG before anything runs.  A pass may
 * mix attached and unattached rows; penalties and records work unchanged (per slot, by absolute position).  The f16-range redo rewrites
 * the rows' own K/V rows; the prefix is a copy of what the context's prefill left and is not redone.
 * An attached row's logits are within the 1e-4 parity bar of llmk_forward's on that sequence alone and of the same slot filled by
 * llmk_batch_fork -- not bit-identical to either: the attention folds the prefix's parts, then the row's own.  The same call on the same
 * state returns the same bits (no float atomics, a fixed part order, no waiting across workgroups).  A pass WITHOUT an attached row
 * returns the bits it returned before a prefix was set.
 * Out of scope: more than one prefix per batch, a tree of prefixes, a shorter own cache for attached slots (the memory saving),
 * any automatic choice between fork and attach.  (f16 K/V: llmk_cache_create, below.) */
int llmk_prefix_set(llmk_batch *b, int n_pos);
int llmk_prefix_attach(llmk_batch *b, int slot);
int llmk_prefix_len(llmk_batch *b);

/* A batch whose K/V caches are IEEE half precision: half the bytes the attention reads per pass and half the
 * device memory per slot.  ("cache", not "batch": the llmk_batch_* list is closed.)  The type is the caller's choice at creation and
 * covers the slots' own caches AND the shared prefix -- no mixed types within a batch, no automatic choice.  The context's own cache,
 * llmk_prefill and the persistent kernel stay f32.
 *
 * create:  kv_type LLMK_TYPE_F32, LLMK_TYPE_F16 or LLMK_TYPE_Q8_0 (below), anything else -- 2, 14, .. -- LLMK_E_TYPE; LLMK_TYPE_Q8_0
 *          on a model whose kv_dim is not a multiple of 32 is LLMK_E_SHAPE; every other check is llmk_batch_create's, with the same
 *          codes.  With LLMK_TYPE_F32 it IS llmk_batch_create: same code path, same allocations, same launches, same bits.  The handle
 *          is an llmk_batch: llmk_batch_*, llmk_rows_* and llmk_prefix_* take it with their contracts unchanged (the parity wording
 *          aside, below).  Caches the device has no room for: LLMK_E_NOMEM, nothing is left allocated.
 * type:    LLMK_TYPE_F32 | LLMK_TYPE_F16 | LLMK_TYPE_Q8_0, a negative LLMK_E_* on error (as llmk_path).
 * bytes:   device bytes of the K/V caches plus the prefix rows, if the batch has any (as allocated: a prefix's blocks only grow).  A
 *          q8_0 batch: 34 bytes per 32 elements, 17/64 of the f32 batch's; its layout adds no padding.
 * peek:    verification hook, like llmk_peek: n cache rows of kv_dim floats each -- K (which 0) or V (1) of positions pos0 .. pos0+n-1
 *          (1-based) of `slot` in `layer`, converted to f32 (exact for f16; a q8_0 batch: value[] below, exact too); slot -1 reads the prefix,
 *          positions 1..P.  Out-of-range arguments: LLMK_E_ARG.  Every cache type.
 * A NULL batch is LLMK_E_ARG (llmk_cache_type: -LLMK_E_ARG) before anything touches a device, in all of them.
 *
 * STORED VALUES of an f16 batch: h = (x != x) ? NaN : RNE_f16(clamp(x, -65504, 65504)) -- round to nearest even, f16 subnormals
 * kept, where x is the f32 value the f32 path stores at that place: at a pass's K/V write what the f32 batch's kernel computes (the
 * same function up to the store), at llmk_batch_fork and llmk_prefix_set the context's f32 row.  Values SATURATE at +-65504 instead of
 * becoming infinite: one outlier must not turn a row's softmax into NaN.  The attention converts the loaded halves back to f32 in
 * registers (exact) and from there runs the arithmetic of the f32 kernels unchanged, so an f16 batch's pass is DEFINED as the f32 pass
 * over a cache that holds the rounded values; the determinism rules carry over (no float atomics, fixed part order, no waiting across
 * workgroups: the same call on the same state gives the same bits).  The f16-range redo rewrites the rows' K/V rows in the batch's type.
 * Parity: rounding K/V to f16 moves a row's logits by a few 1e-4 of max |logit| against llmk_forward's on that sequence (measured on
 * the test models), so an f16 batch is NOT within the 1e-4 bar of the f32 paths; it is within it of the float64 forward pass fed the
 * rows the batch stored (tests/kv16_ref.py).
 *
 * A q8_0 BATCH (LLMK_TYPE_Q8_0 = 8, ggml's id; what llama.cpp's -ctk q8_0 -ctv q8_0 asks for): the slots' caches and the shared prefix
 * hold q8_0 blocks of 32 CONSECUTIVE elements of a position's kv_dim row, K and V alike -- block j is elements 32j .. 32j+31 whatever
 * the head size (at head size 16 one block spans two kv heads) -- 34 bytes per 32 values, 17/32 of f16.  On the device the int8
 * quants [L][slots][seq_len][kv_dim] and the f16 scales [L][slots][seq_len][kv_dim / 32] are separate arrays of one allocation (not
 * ggml's interleaved 34-byte records: a lane's fragment of quants loads naturally aligned); the contract is the VALUES.
 * STORED VALUES: let x[0..32) be the f32 values the f32 batch stores at that place (the same expressions up to the store, as for
 * f16; at llmk_batch_fork / llmk_prefix_set the context's f32 rows).
 *     c[i] = clamp(x[i], -65504, 65504)                 (the saturation rule of the f16 cache: one outlier must not make anything infinite)
 *     amax = max |c[i]|;  d32 = amax / 127.0f;  d = RNE_f16(d32)       (f16 subnormals kept; d32 <= 515.8, so it never overflows)
 *     id   = d32 != 0 ? 1.0f / d32 : 0                  (from d32, not from the rounded d: ggml's quantize_row_q8_0_ref)
 *     q[i] = (int8) clamp(roundf(c[i] * id), -127, 127) (nearest, ties away from zero); q[i] = 0 for all i when d == 0 (an amax
 *                                                       below the f16 subnormals, f32 subnormals -- where id is infinite -- included)
 *     a block with a NaN element: d = f16 NaN, every q = 0 (all 32 values read back NaN: the NaN is not hidden)
 *     value[i] = (float)q[i] * (float)d                 (at most 7 x 11 significant bits: EXACT in f32; never -0.0)
 * For finite inputs within +-65504 these are the values of ggml's quantize_row_q8_0_ref followed by dequantize_row_q8_0.  Every
 * non-zero block holds a +-127 and the rule is idempotent: quantising stored values returns them bit for bit.  All divisions and
 * products are IEEE f32, each rounded once.  A zeroed slot, and the rows beyond n_pos of a fork, hold q = 0, d = 0: +0.0.
 * An attention pass of such a batch is DEFINED as the f32 pass over a cache that holds value[]: bytes and scales are converted in
 * registers, then the f32 kernels' statements run unchanged; the determinism rules of the f16 batch carry over, the f16-range redo
 * rewrites the rows in the batch's type, llmk_cache_type answers 8, llmk_cache_peek answers value[].  Everything that takes an
 * llmk_batch keeps its contract on a q8_0 batch (llmk_batch_*, llmk_rows_*, llmk_prefix_*, llmk_span_*, the token records).
 * Parity: q8_0 is about 25 times COARSER than f16.  Movement of the logits, of max |logit|, when the float64 forward pass quantises
 * its own K/V rows by the rule above (63 positions, seed 777; tests/test_batch_kvq8_cpu.py prints it), next to the f16 figure:
 *     tiny-hs64 0.81e-2 (f16 3.2e-4)   tk-small 1.08e-2 (3.4e-4)   tiny-gqa 1.30e-2 (4.5e-4)   tiny-hs128w 0.94e-2 (3.5e-4)
 *     tiny-kvmul3 0.94e-2 (4.9e-4)
 * (uniform-random test weights, which have near-ties everywhere).  So a q8_0 batch is NOT within the 1e-4 bar of the f32 or f16 paths;
 * it is within it of the float64 forward pass fed the rows the batch stored (tests/kvq8_ref.py).  It is the caller's opt-in, never a
 * default, and nothing chooses a cache type automatically.  Out of scope: q8_0 for the context's own cache, llmk_prefill or the
 * persistent kernel; q4_0 / q5 caches; different K and V types; an int8 score product (Q stays f32); a raw-bits peek. */
int llmk_cache_create(llmk_ctx *ctx, int n_slots, int seq_len, int kv_type, llmk_batch **out);
int llmk_cache_type(llmk_batch *b);    /* LLMK_TYPE_F32 | LLMK_TYPE_F16 | LLMK_TYPE_Q8_0, negative LLMK_E_* on error */
int llmk_cache_bytes(llmk_batch *b, unsigned long long *out);   /* device bytes of the K/V caches + the prefix, if any */
int llmk_cache_peek(llmk_batch *b, int which, int layer, int slot, int pos0, int n, float *out);

/* Spans: SEVERAL consecutive positions of a slot in one pass -- a prompt chunk next to decoding rows, per-slot
 * prompts, k drafted tokens checked in one pass over the weights.  ("span", not "batch": the llmk_batch_* list is closed;
 * llmk_batch_forward keeps refusing two rows of one slot.)
 *
 * forward: one pass.  The rows of the pass are the spans' positions in span order, rows = sum of len; tokens[rows] are the 1-based ids
 *          in that order.  Row j of a span feeds its token at position pos0+j of `slot`: that K/V row is written, and the row attends
 *          over the slot's positions 1..pos0+j -- the prefix if the slot is attached, earlier cache rows, and the rows this same pass
 *          wrote for columns <= j of the span; it sees none of the columns > j.
 *          LLMK_E_ARG before anything runs or is allocated: a NULL batch, spans or tokens; n_spans < 1 or a len < 1; rows >
 *          LLMK_MAX_BATCH; a slot out of range or named by two spans; pos0 < 1 or pos0+len-1 > the batch's seq_len; an attached slot
 *          with pos0 <= P; a token outside [1, vocab_size]; flag bits other than LLMK_SPAN_LAST; both outputs NULL.  n_spans is bounded
 *          by slot distinctness only, and rows may exceed n_slots.
 *          logits_out [rows][vocab_size] and argmax_out [rows] (the 1-based first maximum, llmk_forward_greedy's rule) in row order;
 *          with LLMK_SPAN_LAST they are [n_spans][vocab_size] and [n_spans]: ONE row per span, its last position, in span order (the
 *          classifier still runs over all rows).  Either may be NULL.  A row with no finite logit: LLMK_E_NONFINITE.
 *          A call whose spans all have len == 1 IS llmk_batch_forward: same code path, same launches, same bits.
 * time:    measurement hook like llmk_batch_time: average milliseconds of one full pass (classifier and greedy pick included) of
 *          n_spans spans of len rows each, slots 0..n_spans-1, all from pos0, with forward's range checks.  It OVERWRITES those rows.
 * Parity: a row's logits are within the 1e-4 bar of llmk_forward's on that sequence alone, and of the same positions fed one per pass
 * through llmk_batch_forward -- not bit-identical to either.  An f16 batch is defined as elsewhere: the f32 span pass over a cache that
 * holds the rounded rows.  The same call on the same state returns the same bits (no float atomics, a fixed part order, no waiting
 * across workgroups), and a row's bits do not depend on the tokens of LATER rows of its span.
 * The f16-range rule of llmk_prefill applies: the call is redone on the f32 matrix instruction and its K/V rows are rewritten in the
 * batch's type.
 * REJECTED DRAFTS ARE FREE: cache rows beyond the position a caller accepts are dead.  No row of any later pass reads cache row r before
 * a pass at position r+1 of that slot has rewritten it (a row at position p reads rows 0..p-1, and row p-1 is the one it writes), so a
 * caller that accepts j of a span's rows simply continues the slot at position pos0+j; nothing is rolled back.
 * Token records are NOT maintained: the caller records what it fed with llmk_rows_set_history, as after a fork.
 * State the span passes need -- logits rows beyond n_slots, part states, the group table -- is allocated by the first span call that
 * needs it: a batch that never calls these functions allocates and launches exactly what it did without them.
 * In a span pass the slot's K/V rows are read once per GROUP of 16 / (query heads per kv head) consecutive rows of a span
 * (bd_attn_span_kernel), not once per row.  LLMK_SPAN_ATTN=0 in the environment at llmk_batch_create / llmk_cache_create makes span
 * passes run the per-row attention kernels of llmk_batch_forward instead (an A/B switch, like LLMK_PF_F32_MFMA for the prompt GEMMs);
 * the results stay within the parity bar.
 * Out of scope: draft models and acceptance policies (the host compares argmax_out itself), spans inside llmk_batch_decode /
 * llmk_rows_decode, skipping classifier rows under LLMK_SPAN_LAST, more than LLMK_MAX_BATCH rows per pass. */
typedef struct llmk_span { int32_t slot, pos0, len; } llmk_span;   /* positions pos0 .. pos0+len-1 (1-based) of `slot` */
#define LLMK_SPAN_LAST 1   /* the outputs hold ONE row per span, its last position, in span order */
int llmk_span_forward(llmk_batch *b, int n_spans, const llmk_span *spans, const int *tokens, int flags,
                      float *logits_out, int *argmax_out);
int llmk_span_time(llmk_batch *b, int n_spans, int len, int pos0, int iters, float *avg_ms);

/* Zero the KV cache (new sequence), as llama2.f90:316-318; the token record of the penalties, if the context has one, is zeroed too. */
int llmk_reset(llmk_ctx *ctx);

/* The reference's five section timers s%times(1:5) (llama2.f90:538,561,599,622,638), accumulated
 * milliseconds since create/reset; all zero unless LLMK_FLAG_TIMINGS. */
int llmk_timings(llmk_ctx *ctx, float ms[5]);

/* Measurement hook for bench.py: runs `iters` launches of one kernel of the token pass on the
 * ctx's stream with HIP events around them and returns the average milliseconds per launch and
 * the algorithmic bytes one launch moves.  kernel: 0 qkv, 1 attention, 2 wo, 3 w13, 4 w2,
 * 5 classifier (successive launches walk the layers), 6 the persistent whole-token kernel
 * (LLMK_E_ARG when the ctx runs the multi-kernel path), 7..10 the w1|w3, wqkv, wo, w2 GEMMs of llmk_prefill at 128 positions
 * (bytes = that matrix of one layer; flop = 2 * 128 * rows * K), 11 the five per-layer kernels of the multi-kernel path (a
 * tensor-parallel rank's too, without its exchanges) for all layers as one hipGraph: milliseconds and bytes per LAYER,
 * 12 the classifier GEMM of llmk_score at 128 positions (all its row chunks, without the scoring epilogue; bytes = wcls -- q6_K rows as they lie
 * on the device: 210 bytes per 256 weights, rounded up to 16 per row; LLMK_E_ARG where the context has no classifier GEMM:
 * llmk_cls_form(ctx, 128) != LLMK_CLS_GEMM).
 * STATE: a measurement hook, not part of the generation path.  Kernels 0..6 and 11 run real kernels of the pass at the ctx's
 * current position (position 1 if none was run yet): they overwrite x, that position's K/V rows and the exchange state, kernel 11
 * for every layer; kernels 7..10 and 12 overwrite the prefill workspaces.  Call llmk_reset before generating on the ctx again. */
int llmk_time_kernel(llmk_ctx *ctx, int kernel, int iters, float *avg_ms, double *bytes_per_launch);

/* Which form the classifier of a batched pass (llmk_score's batches, llmk_batch_*) of `rows` rows (1..LLMK_MAX_BATCH, else
 * LLMK_E_ARG) takes on this context RIGHT NOW; like llmk_path the answer can change (an f16-range flag moves the context to the f32
 * matrix instruction, where q6_K rows have no GEMM), and like llmk_time_kernel the call may set up the prefill workspaces.  The answer
 * describes the batched pass itself: LLMK_PREFILL=0, which makes llmk_score go token by token and leaves llmk_batch_* as it is, does not
 * change it. */
#define LLMK_CLS_NONE 0   /* this context has no batched pass with `rows` rows (llmk_score goes token by token, llmk_batch_create refuses) */
#define LLMK_CLS_GEMM 1   /* the classifier crosses HBM once per pass (f32 / f16 / q4_0 / q6_K) */
#define LLMK_CLS_ROWS 2   /* q6_K only: the decode classifier once per row of the pass */
int llmk_cls_form(llmk_ctx *ctx, int rows);   /* a negative LLMK_E_* code on error (-LLMK_E_ARG for a NULL context), as llmk_path */

/* Debug/verification: copy internal device vectors to the host. which: 0 = x (residual stream, E),
 * 1 = q (E), 2 = xb (attention output, E), 3 = hb (H), 4 = key_cache row [layer][pos-1] (KV),
 * 5 = value_cache row (KV); debugging aids: 6, 7 = the debug library's trace stamps and a prefill workspace, 8 = the q4_0
 * persistent kernel's per-layer scale records of the last two positions ([2][128] x {max|xb|, max|hb|, pos, pos} as floats /
 * int bits: tests/host_tools/qsc_dump.py; LLMK_E_ARG on a ctx without the persistent kernel). */
int llmk_peek(llmk_ctx *ctx, int which, int layer, int pos, float *out, int n);

/* Which implementation of the token pass this ctx runs RIGHT NOW (it can change: a timed-out persistent kernel retires
 * to the multi-kernel path; llmk_set_tensor_type does the same): one of LLMK_PATH_*, or a negative LLMK_E_* code.
 * For labels in benchmarks and logs -- no reference counterpart. */
#define LLMK_PATH_MULTI_KERNEL 0     /* 5 launches per layer (csrc/kernels.h)                                        */
#define LLMK_PATH_TOKEN_KERNEL 1     /* persistent whole-token kernel (csrc/token_kernel.h)                          */
#define LLMK_PATH_TP_P2P 2           /* tensor-parallel rank: 6 launches per layer + one-shot peer-memory exchanges  */
#define LLMK_PATH_TP_RCCL 3          /* tensor-parallel rank: eager launches + ncclAllReduce / ncclAllGather         */
#define LLMK_PATH_TP_UNCONNECTED 4   /* tensor-parallel rank without collectives yet (llmk_tp_segment stepping only) */

/* The model shapes the persistent whole-token kernel is instantiated for in this build, as text:
 * "E,H,NH,NKV,V,type[+q6_K];..." (type = the matrices' f32 | f16 | q4_0; +q6_K = with a q6_K classifier).  The reference's dims
 * are compile-time parameters (llama2.f90:102-108); so are the kernel's -- `make TK_SHAPES="..."` adds shapes (llm.f90_amd/Makefile).
 * Any other shape runs the multi-kernel path (llmk_path).  LLMK_E_SIZE when `buf` is too small. */
int llmk_tk_shapes(char *buf, size_t n);

/* (one of the LLMK_PATH_* values above: see there) */
int llmk_path(llmk_ctx *ctx);
/* How many ranks this ctx's collective actually spans: ncclCommCount of its RCCL communicator, or the number of mapped
 * peer inboxes (+ itself) on the peer-memory path, or 1.  For the benchmark line of a multi-GPU run (`ranks_seen`). */
int llmk_tp_ranks_seen(llmk_ctx *ctx);

/* Verification: 64-bit sum of the 32-bit words of a tensor's DEVICE image (this rank's shard, device layout).  Equal images
 * give equal sums: two uploads of the same weights, or one context before and after a run, compare without a read-back. */
int llmk_tensor_checksum(llmk_ctx *ctx, int tensor_id, unsigned long long *out);

int llmk_destroy(llmk_ctx *ctx);

/* static string for an error code returned by any function above */
const char *llmk_strerror(int code);

/* library/ABI version: major*10000 + minor*100 + patch */
int llmk_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LLMK_H */
