// llmk C-ABI shim (include/llmk.h): device memory, weight upload, the per-token launch sequence
// (captured once into a hipGraph and replayed), measurement hooks.  gfx950 only; no CPU path.
//
// Token pass (replaces `transformer`, /root/reference/llama2.f90:480-640), 5 launches per layer:
//   embed                                   x = table(:,token)                      :520
//   per layer l:
//     gemv<NORM,ROPE_KV>   rmsnorm -> fused QKV GEMV -> RoPE -> q, key/value cache   :527-565
//     attn                 scores, softmax, PV per head (GQA)                        :572-598
//     gemv<RESID>          x += wo . xb                                              :603-605
//     gemv<NORM,SWIGLU>    rmsnorm -> fused w1|w3 GEMV -> silu(g)*u                  :608-616
//     gemv<RESID>          x += w2 . hb                                              :618-620
//   gemv<NORM,STORE>       final rmsnorm -> classifier                               :627-636
//   (greedy only) argmax                                                             :388
#include "../../include/llmk.h"
#include "kernels.h"
#include "token_kernel.h"
#include "prefill.h"
#include "batch.h"
#include "tp_p2p.h"
#include "forward_ahead.h"
#include "tk_recover.h"
#include "owned.h"

#include <rccl/rccl.h>

#include <algorithm>
#include <memory>
#include <utility>
#include <vector>

#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>

using namespace llmk;

extern "C" int llmk_create_tp(const llmk_config* cfg, int tp_rank, int tp_size, llmk_ctx** out);
static int q16_build(llmk_ctx* c);        // (defined behind the upload helpers it uses)

#define HIPCHK(expr)                                          \
    do {                                                      \
        hipError_t e_ = (expr);                               \
        if (e_ != hipSuccess) return LLMK_E_HIP + (int)e_;    \
    } while (0)

namespace {

struct TensorDesc {
    bool layered;   // has a leading layer dimension
    int rows;       // rows per layer (1 for vectors)
    int K;          // row length
    bool matrix;    // streamed matmul weight (may be f16/q4_0); else always f32
};

struct DevTensor {
    DevBuf<char> own;        // the allocation behind `data`; empty: a view into another tensor's (the rmsnorm gains share one)
    void* data = nullptr;    // f32/f16 rows; q4_0: rows of K/2 nibble bytes followed by the row's K/32 f16 scales
    size_t row_bytes = 0;    // bytes per row in `data` (q4_0: 9K/16 rounded up to 16)
    int type = LLMK_TYPE_F32;
    bool uploaded = false;
    size_t rows_uploaded = 0;
};

// The sampler's lazily created records, one definition for a context (one sequence, one row) and a batch (n_slots sequences,
// LLMK_MAX_BATCH rows).  Each is empty until the first call that needs it (pen_setup, lp_setup), which builds it aside and moves it in
// whole: an empty one reads as null pointers everywhere.
// Penalties and logit bias (sample_penalty.h): the token records (hist[seq][q - 1] = the 1-based token fed at position q, 0 = none), the
// counts of the penalty kernels ([seq][V], all zero between launches), a row's parameters on the device and the pinned words they
// are copied from
struct PenaltyState {
    DevBuf<int> hist, cnt;
    DevBuf<llmk_penalty_params> d_pen;
    PinnedBuf<llmk_penalty_params> h_pen;
};
// Log-prob records (logprob.h): on the device and pinned, the top_n word (pinned; a batch's kernels read a device copy, a context's
// read TkDevWords::lp_top_n) and the raw logits that are set aside in front of the penalty kernel
struct LogprobState {
    DevBuf<llmk_logprob_record> d;
    PinnedBuf<llmk_logprob_record> h;      // (allocated last: its size says that both are there)
    DevBuf<unsigned> d_top;
    PinnedBuf<unsigned> h_top;
    DevBuf<float> raw;
};

// What a token pass hands back: the logits (llmk_forward), the device argmax (llmk_forward_greedy) or the device sample
// (llmk_forward_sample; TAIL_FILTER: the truncated one of sample_filter.h; TAIL_PENALTY: the same behind the penalties and the
// logit bias of sample_penalty.h); all but the first leave the 1-based id in h_next->id and the sticky error word in h_next->err.
// enqueue_sampler has what the last two enqueue.
enum TailMode { TAIL_LOGITS, TAIL_GREEDY, TAIL_SAMPLE, TAIL_FILTER, TAIL_PENALTY, TAIL_COUNT };

// What the device's copy of a set of parameter words holds once the stream has drained, as far as the host knows
template <class T>
struct DevShadow {
    T value = {};
    bool known = false;
    void invalidate() { known = false; }                        // a pass is about to copy words the host cannot vouch for yet
    void confirm(const T& v) { value = v; known = true; }      // ... and has copied v
    template <class F>
    hipError_t push(const T& want, F copy) {                    // copy() enqueues the write of `want`: only where the device holds something else
        if (known && memcmp(&want, &value, sizeof(T)) == 0) return hipSuccess;
        const hipError_t e = copy();
        if (e == hipSuccess) confirm(want);
        return e;
    }
};

}  // namespace

struct llmk_ctx {
    llmk_config cfg;
    int E, H, L, nh, nkv, V, S, hs, KV, kv_mul;
    // (declared before every buffer and event: members are destroyed in reverse order, so the stream outlives what ran on it)
    Stream stream;
    // tensor-parallel shard of this ctx (tp_size == 1: the whole model). Local dims: q columns, kv dim,
    // hidden rows, vocab rows and heads owned by this rank (Megatron split).
    int tp_rank = 0, tp_size = 1;
    int Eq, KVl, Hl, Vl, nhl;
    ncclComm_t comm = nullptr;
    // one-shot peer-memory collectives (tp_p2p.h): this rank's inbox (fine-grained HBM) and the peers' as mapped here
    DevBuf<unsigned long long> d_inbox;
    DevBuf<unsigned> d_tp_bad;            // the self-test's mismatch counter (allocated with the inbox: see tp_selftest_run)
    TpPeers peers = {};
    void* ipc_mapped[TP_MAX_RANKS] = {};
    bool p2p = false;
    DevBuf<float> d_part;          // [E] partial sums of the row-parallel GEMVs (wo, w2) before the all-reduce
    TensorDesc gdesc[LLMK_N_TENSORS];  // the full (unsharded) tensors, what llmk_upload is handed
    TensorDesc desc[LLMK_N_TENSORS];
    DevTensor t[LLMK_N_TENSORS];
    DevBuf<float> d_kc, d_vc;      // [L][S][KV]  (RunState, weight_module.f90:33-40)
    DevBuf<float> d_x, d_q, d_xb, d_hb, d_rope;
    DevBuf<float> d_logits;        // [V], then dev_words()
    DevBuf<int> d_tokpos, d_next;
    PinnedBuf<int> h_tokpos;    // pinned {token0, pos1}
    PinnedBuf<float> h_logits;       // mapped: [V], then host_words(); dev(): as the device sees it (token kernel direct mode)
    bool tk_direct = true;
    PinnedBuf<TkNext> h_next;
    // the scratch words behind the logits vectors (scratch_layout.h): the device's, the host's, the host's as the device sees them
    TkDevWords* dev_words() const { return tk_words_behind<TkDevWords>(d_logits, V); }
    TkHostWords* host_words() const { return tk_words_behind<TkHostWords>(h_logits, V); }
    TkHostWords* host_words_dev() const { return tk_words_behind<TkHostWords>(h_logits.dev(), V); }
    hipGraphExec_t graph[TAIL_COUNT][2] = {};   // the token pass with each tail, without / with the log-prob record, captured at first use (drop_graphs)
    PinnedBuf<llmk_sample_params> h_samp;   // invT and seed of the current sampling call
    // the device's copy of them (TkDevWords::samp): zeros from llmk_create on.  A pipelined decode writes them only when they differ,
    // so a greedy one on a ctx that never sampled enqueues nothing new
    DevShadow<llmk_sample_params> samp_dev = {{}, true};
    // the same pair for the truncated sampler (a filter, a penalty or a bias on): its parameters sit behind the sampling words
    // (TkDevWords::filt)
    PinnedBuf<llmk_filter_params> h_filt;
    DevShadow<llmk_filter_params> filt_dev;
    // penalties and logit bias (llmk_*_sample_pen): one sequence of S positions, one row
    PenaltyState pen;
    // decode log-probs (llmk_*_sample_lp): S + 1 records -- [q - 1]: position q of a pipelined decode; [S]: what the tail of a token
    // pass, or the hook, leaves -- and [V] raw logits
    LogprobState lp;
    int lp_top_n = -1;      // the running call's request (logprob_request .. LpScope), -1: none -- every site enqueues what it always did
    Event ev[8];
    float times[5] = {0, 0, 0, 0, 0};
    int n_cu = 256;
    float eps = 1e-5f;     // rmsnorm epsilon: the reference's constant (llama2.f90:454) unless llmk_set_rms_eps
    // persistent whole-token kernel (token_kernel.h)
    bool use_tk = false;
    bool tk_short_grid = false;   // libllmk_debug.so only (LLMK_TK_INJECT_TIMEOUT)
    TkRecovery tk;                // what the kernel's sticky error word means for this ctx (tk_recover.h; carried out by tk_perform)
    int tk_shape = 0;      // 1-based index into tk_table (the instantiated shapes: LLMK_TK_SHAPES), 0 = none
    DevBuf<unsigned long long> d_gran;     // exchange granules: qkv | xb | xa | hb | x | attention parts
    DevBuf<float4> d_zeros;
    DevBuf<unsigned long long> d_trace;    // debug stamps (LLMK_TK_TRACE=1)
    size_t tk_lds = 0;
    size_t tk_ngran = 0;   // granules in d_gran (the last TK_QSC_GRANULES: the q4_0 kernels' per-layer scale records, tk_qsc_records)
    // pipelined greedy decode (llmk_decode_greedy): per-CU classifier maxima of the last two launches, and the ids as they
    // are resolved (host-mapped; 0 = not there yet)
    // (the candidates sit behind the device error word, the ids behind the host error word: scratch_layout.h)
    // batched prefill (prefill.h), built by the first llmk_prefill (pf_setup) and dropped as a whole (pf.reset()).  Two LANES =
    // workspace set + stream: consecutive 128-position batches of a prompt alternate between them, so one batch's small kernels
    // (epilogues, attention) and launch gaps run under the other's GEMMs.  The only cross-batch dependency is the KV cache: batch
    // k+1's attention in layer l waits for batch k's K/V rows of layer l (event kv[l]).
    struct PfLane {
        Stream own;                        // lane 1's stream (declared first: destroyed after the lane's buffers and events)
        hipStream_t stream = nullptr;      // the lane's stream: lane 0 the ctx stream, lane 1 `own` (a view either way)
        DevBuf<float> X, Xs, Q, XB, HB, P, xn;
        DevBuf<unsigned> lowcnt;           // [2][PF_TMAX]: the GEMM workgroups' votes on positions that are small as a whole (prefill.h pf_low_check)
        std::vector<Event> kv;             // per layer: this lane's batch has written its K/V rows
        Event done;                        // this lane's batch has left the last layer
    };
    struct Prefill {
        PfLane lane[2];
        DevBuf<int> tok;                   // a call's tokens, 0-based
        Event start;                       // tokens are on the device (and everything before the prefill call is done)
        DevBuf<unsigned> flag;             // device word: an activation did not fit f16 (the call is redone on the f32 instruction)
    };
    std::unique_ptr<Prefill> pf;
    std::vector<int> pf_tok0;              // what pf->tok is uploaded from: alive until the call has synchronised
    // uploads are staged through the shim's OWN pinned memory (upload_block), built by the first upload: two buffers, an event each
    struct Upload {
        PinnedBuf<char> stage[2];          // mapped: the kernels read stage[b].dev()
        DevBuf<char> tmp[2];               // device scratch of the q4_0 re-packing (written and read by kernels only)
        Event done[2];
        DevBuf<unsigned long long> acc;    // device word of the upload verification's 16-bit word sums
    };
    std::unique_ptr<Upload> up;
    // q4_0 matrices in the persistent kernel's UNIT layout (q4_units.h: 16 rows x 32 blocks as matrix-core operands), built from
    // the row layout -- which the multi-kernel path, the prefill and the fallback keep reading -- at the first token after an upload
    DevBuf<char> q16[LLMK_N_TENSORS];
    bool q16_dirty = true;
    bool pf_hm = false;                    // GEMMs on v_mfma_f32_16x16x32_f16, activations (and f32 / q4_0 weights) as two f16 pieces (prefill.h)
    size_t pf_pcap = 0;                    // floats in each lane's partial-tile workspace P
    // llmk_score (prefill.h pf_score_kernel), built by the first scoring call (sc_setup): per lane the positions' partial results and
    // target logits (and, for a q6_K classifier, a batch of logits rows); the call's targets and results; the logits of a call that asks for them
    struct Score {
        DevBuf<float4> part[2];
        DevBuf<float> tgt[2], z[2];
        DevBuf<int> targets;               // [S] 0-based, < 0: none
        DevBuf<float> out;                 // [2S]: a call's n log-probs, then its n argmax ids
        PinnedBuf<float> h_out;            // pinned image of `out`
        DevBuf<float> logits;              // [positions][V], grown by the call that asks for more (reserve)
    };
    std::unique_ptr<Score> sc;
    int n_batches = 0;                     // live llmk_batch objects on this context (llmk_destroy refuses while there are any)
    // llmk_forward with the next greedy position in flight (forward_ahead.h).  Position p's logits go to pinned
    // buffer p & 1 -- [0] is h_logits, whose error word and ids() serve both -- so the host copies out of one while the next launch
    // fills the other; fa_ev[p & 1] is recorded right behind position p's launch
    bool fa_on = true;                     // LLMK_FORWARD_AHEAD=0: llmk_forward as it was
    ForwardAhead fa;
    bool fa_inflight = false;              // a speculative launch is on the stream (fa.armed says so too; this one survives fa.miss())
    PinnedBuf<float> fa_second;            // [V], mapped: buffer 1
    float* fa_buf[2] = {nullptr, nullptr};       // views: [0] h_logits, [1] fa_second ...
    float* fa_buf_dev[2] = {nullptr, nullptr};   // ... and as the device sees them
    const float* fa_logits = nullptr;      // where the last llmk_forward's logits still are (what fa.scan_due compares with)
    int fa_tok0 = 0, fa_pos = 0;           // the last DELIVERED call's h_tokpos words (a settled speculation puts them back)
    Event fa_ev[2];
};
typedef llmk_ctx::PfLane PfLane;

// Batched decode (batch.h): K/V caches of its own for n_slots sequences on the context's weights.  A pass runs on
// the context's stream through lane 0 of its prefill workspaces and the scoring partials (calls on a batch and on its context are
// serialised by the caller, as all calls on a context are); what a pass needs beyond them is here.
struct llmk_batch {
    llmk_ctx* ctx = nullptr;
    int n_slots = 0, seq_len = 0;
    int kv_type = LLMK_TYPE_F32;                 // the caches' and the prefix's element type (llmk_cache_create): ONE pair of each is allocated
    DevBuf<float> d_kc, d_vc;                    // [L][n_slots][seq_len][KV], an f32 batch's ...
    DevBuf<_Float16> d_kc16, d_vc16;             // ... and an f16 batch's (BdKv<T> below picks the pair by element type)
    DevBuf<int8_t> d_kc8, d_vc8;                 // a q8_0 batch's: the quants in that order, then the scales [L][n_slots][seq_len][KV / 32] f16 (BdKv<KvQ8>)
    DevBuf<BdRow> d_rows;                        // [LLMK_MAX_BATCH] row words
    DevBuf<int> d_tok;                           // [LLMK_MAX_BATCH] 0-based fed ids
    DevBuf<float> d_out;                         // [2 * LLMK_MAX_BATCH]: (unused log-probs), then the rows' first maxima (1-based ints)
    DevBuf<float> d_logits;                      // [n_slots][V]
    DevBuf<float> d_po;                          // attention parts: [n_cu][BD_MAX_GROUP][hs] unnormalised outputs ...
    DevBuf<float2> d_pml;                        // ... and [n_cu][BD_MAX_GROUP] {M, L}
    DevBuf<int> d_next;                          // [LLMK_MAX_BATCH] the samplers' picks
    DevBuf<llmk_filter_params> d_filt;           // [LLMK_MAX_BATCH] row i's sampler
    DevBuf<unsigned> d_out2;                     // [LLMK_MAX_BATCH][2] sample_filter_kernel's {kept, tau}
    DevBuf<unsigned> d_err;                      // a decode step had no finite logit in some row
    DevBuf<int> d_ids;                           // a decode's ids, row-major; grown by the call that needs more (reserve)
    // pinned: what a call uploads (rows, tokens, samplers) and reads back (first maxima, error word)
    PinnedBuf<BdRow> h_rows;
    PinnedBuf<int> h_tok;
    PinnedBuf<llmk_filter_params> h_filt;
    PinnedBuf<float> h_out;
    PinnedBuf<unsigned> h_err;
    // penalties, logit bias and log-prob records of the rows functions (llmk_rows_*), as a context's.  Logits, parameters, picks and
    // records are per ROW of a call -- the records [row][step], grown by the call that needs more -- the token records and the counts
    // are per SLOT: a sequence keeps its record whichever row of a call it is
    PenaltyState pen;
    LogprobState lp;
    // a shared prefix (llmk_prefix_*, batch.h), built by the first llmk_prefix_set that sets one: a batch without one has none of it
    int P = 0, n_attached = 0;                   // the prefix's positions; slots attached to it
    struct Prefix {
        DevBuf<int> d_first;                     // [n_slots] a slot's first own cache row: P attached, 0 not ...
        PinnedBuf<int> h_first;                  // ... and the pinned words it is copied from
        DevBuf<int> d_colmap;                    // [LLMK_MAX_BATCH + BD_MAX_GROUP] bd_attn_prefix_kernel's column map
        PinnedBuf<int> h_colmap;
        DevBuf<float> d_xpo;                     // part states of a pass with attached rows:
        DevBuf<float2> d_xpml;                   //   [LLMK_MAX_BATCH][n_kv_heads][2 * BD_MAX_PARTS][kv_mul] {M, L}, d_xpo that [hs]
        DevBuf<float> d_pk, d_pv;                // [L][P][KV]: a snapshot of the context's rows of positions 1..P, grown by reserve
        DevBuf<_Float16> d_pk16, d_pv16;         // the same in an f16 batch: the prefix has the batch's type
        DevBuf<int8_t> d_pk8, d_pv8;             // ... and in a q8_0 batch: quants [L][P][KV], then scales [L][P][KV / 32]
    };
    std::unique_ptr<Prefix> px;
    int pass_att = 0;                            // attached rows among the rows bd_upload_rows uploaded last
    // spans (llmk_span_*, batch.h), built by the first span call that runs bd_attn_span_kernel: a batch without one has none of it
    struct Spans {
        DevBuf<BdGroup> d_groups;                // [LLMK_MAX_BATCH] the pass's column groups ...
        PinnedBuf<BdGroup> h_groups;             // ... and the pinned words they are copied from
        DevBuf<float> d_spo;                     // part states of a span pass, in the layout of a pass with attached rows:
        DevBuf<float2> d_spml;                   //   [LLMK_MAX_BATCH][n_kv_heads][2 * BD_MAX_PARTS][kv_mul] {M, L}, d_spo that [hs]
    };
    std::unique_ptr<Spans> sn;
    bool span_attn = true;                       // LLMK_SPAN_ATTN=0 at create: span passes run the per-row attention kernels
    int pass_groups = 0;                         // column groups of the rows span_upload uploaded last; 0: not a span pass
};

namespace {

constexpr size_t TENSOR_SLACK = 64 * 1024;
size_t q4_row_stride(int K) { return (size_t)K / 2 + (size_t)((K / 32 + 63) / 64) * 128; }

size_t row_bytes_for(int type, int K) {
    switch (type) {
        case LLMK_TYPE_F32: return (size_t)K * 4;
        case LLMK_TYPE_F16: return (size_t)K * 2;
        case LLMK_TYPE_Q4_0: return (size_t)K / 32 * 18;
        case LLMK_TYPE_Q6_K: return (size_t)K / Q6K_WEIGHTS * Q6K_BLOCK_BYTES;      // (the classifier only: q6k.h)
    }
    return 0;
}
// bytes between a tensor's rows ON THE DEVICE (q4_0 and q6_K rows are re-packed by the upload: kernels.h, q6k.h)
size_t dev_row_bytes(int type, int K) {
    return type == LLMK_TYPE_Q4_0 ? q4_row_stride(K) : type == LLMK_TYPE_Q6_K ? q6k_row_stride(K) : row_bytes_for(type, K);
}

// llmk_create walks the token pass once with g_prepare set: nothing is launched, but every kernel whose dynamic LDS
// request (the staged activation vector, the attention score row) exceeds the 64 KB default limit gets its limit raised,
// so a long context or a wide contraction fails at create (LLMK_E_SHAPE beyond 160 KB) and never at the first forward.
thread_local bool g_prepare = false;
constexpr size_t LDS_DEFAULT_LIMIT = 64 * 1024, LDS_MAX = 160 * 1024;
template <class F>
bool prepare_only(F kernel, size_t smem, hipError_t* e) {
    if (!g_prepare) return false;
    *e = smem > LDS_MAX ? hipErrorInvalidValue
       : smem > LDS_DEFAULT_LIMIT ? hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)
                                  : hipSuccess;
    return true;
}

template <int WT, int EPI, bool NORM, int ROWS, int NCH>
hipError_t launch_gemv(hipStream_t st, const GemvArgs& a) {
    const int njobs = (EPI == EPI_SWIGLU) ? a.H : a.rows / ROWS;
    const int blocks = (njobs + GEMV_WAVES - 1) / GEMV_WAVES;
    const size_t smem = 16 + (size_t)a.K * sizeof(float);
    hipError_t pe;
    if (prepare_only(gemv_kernel<WT, EPI, NORM, ROWS, NCH>, smem, &pe)) return pe;
    hipLaunchKernelGGL((gemv_kernel<WT, EPI, NORM, ROWS, NCH>), dim3(blocks), dim3(GEMV_THREADS), smem, st, a);
    return hipGetLastError();
}

// Tile shapes: ROWS x NCH 16-byte vectors per lane are requested up front (<= ~88 VGPRs).
//   f32  K=2048: 2 rows x 8 = the whole pair (16 KB/wave);  K=5632 (w2): 1 row x 22 = whole row
//   f16  K=2048: 2 x 4;                                      K=5632: 1 x 11
//   q4_0 K=4096: 2 x 2
template <int EPI, bool NORM>
hipError_t launch_gemv_t(int wt, hipStream_t st, const GemvArgs& a, int n_cu) {
    constexpr bool single_ok = (EPI == EPI_STORE || EPI == EPI_RESID) && !NORM;
    switch (wt) {
        case LLMK_TYPE_F32: {
            const int ncol = a.K / 4 / WAVE;
            if constexpr (single_ok)
                if (ncol % 22 == 0) return launch_gemv<WT_F32, EPI, NORM, 1, 22>(st, a);
            return launch_gemv<WT_F32, EPI, NORM, 2, 8>(st, a);
        }
        case LLMK_TYPE_F16: {
            const int ncol = a.K / 8 / WAVE;
            if constexpr (single_ok)
                if (ncol % 11 == 0) return launch_gemv<WT_F16, EPI, NORM, 1, 11>(st, a);
            return launch_gemv<WT_F16, EPI, NORM, 2, 4>(st, a);
        }
        default: {   // q4_0: dedicated kernel, up to 8 rows per wave (kernels.h); fewer when the matrix is
                     // too small to give every CU at least two workgroups that way
            const int npairs = (EPI == EPI_SWIGLU) ? a.H : a.rows / 2;
            const size_t smem = 16 + (size_t)a.K * sizeof(float) + 8 * 16 + (size_t)(a.K / 32) * sizeof(float);   // x (pitch nblk+1) + block sums
            // workgroups wanted before a wave takes more pairs: two per CU -- one and a half where x is 32 KB or more (K >= 8192: every
            // workgroup stages the whole x; the 70B rank's w1|w3, 3,584 pairs: 896 workgroups of one pair per wave 12.2 us, 448 of
            // two 10.9 us, 224 of four 14.8 us; LLMK_Q4_NP sweep, profiles/r04_tp70_rank_kernels_pairs_per_wave.txt)
            const int want = a.K >= 8192 ? 3 * n_cu / 2 : 2 * n_cu;
#define Q4_LAUNCH(NP_, KS_)                                                                                      \
            do {                                                                                                 \
                const int blocks = (npairs + (GEMV_WAVES / KS_) * NP_ - 1) / ((GEMV_WAVES / KS_) * NP_);         \
                hipError_t pe;                                                                                   \
                if (prepare_only(gemv_q4_kernel<EPI, NORM, NP_, KS_>, smem, &pe)) return pe;                     \
                hipLaunchKernelGGL((gemv_q4_kernel<EPI, NORM, NP_, KS_>), dim3(blocks), dim3(GEMV_THREADS), smem, st, a); \
            } while (0)
            // wide rows (K a multiple of 8192: the Llama-2-70B rank shapes): column slices across the block's waves
            static const int ks_env = getenv("LLMK_Q4_KS") ? atoi(getenv("LLMK_Q4_KS")) : -1;     // measurement aid: 0 = never
            // ... and only where even one pair per wave leaves CUs without a block (measured on rank 0 of 8 of the 70B shape,
            // tests/host_tools/tp_rank_time.py: QKV, 640 pairs, 7.9 -> 6.8 us; w1|w3 13.3 -> 18.8 us and the classifier shard
            // 9.3 -> 12.0 us the OTHER way: four times the blocks each stage the whole x)
            const bool wide = (a.K % 8192) == 0 && ks_env != 0 && (npairs / GEMV_WAVES < n_cu || ks_env > 0);
            static const int np_env = getenv("LLMK_Q4_NP") ? atoi(getenv("LLMK_Q4_NP")) : 0;       // measurement aid: pairs per wave, forced
            if (np_env > 0 && !wide) {          // (in the column-sliced launches below too)
                if (np_env >= 4) Q4_LAUNCH(4, 1);
                else if (np_env >= 2) Q4_LAUNCH(2, 1);
                else Q4_LAUNCH(1, 1);
            }
            else if (wide) {
                if (np_env >= 4) Q4_LAUNCH(4, 4);
                else if (np_env >= 2) Q4_LAUNCH(2, 4);
                else if (np_env == 1) Q4_LAUNCH(1, 4);
                else if (npairs / 4 >= want) Q4_LAUNCH(4, 4);
                else if (npairs / 2 >= want) Q4_LAUNCH(2, 4);
                else Q4_LAUNCH(1, 4);
            }
            else if (npairs / (GEMV_WAVES * 4) >= want) Q4_LAUNCH(4, 1);
            else if (npairs / (GEMV_WAVES * 2) >= want) Q4_LAUNCH(2, 1);
            else Q4_LAUNCH(1, 1);
#undef Q4_LAUNCH
            return hipGetLastError();
        }
    }
}

// f(std::integral_constant<int, hs>()) for the head sizes llmk_create_tp admits: the head size as a compile-time constant
template <class F>
hipError_t with_head_size(int hs, F f) {
    switch (hs) {
        case 16: return f(std::integral_constant<int, 16>());
        case 32: return f(std::integral_constant<int, 32>());
        case 64: return f(std::integral_constant<int, 64>());
        case 128: return f(std::integral_constant<int, 128>());
    }
    return hipErrorInvalidValue;
}
hipError_t launch_attn(llmk_ctx* c, int l) {
    const float* kc = c->d_kc + (size_t)l * c->S * c->KVl;
    const float* vc = c->d_vc + (size_t)l * c->S * c->KVl;
    const size_t smem = (516 + (size_t)c->S) * sizeof(float);
    return with_head_size(c->hs, [&](auto hs) {
        constexpr int HS = decltype(hs)::value;
        hipError_t pe;
        if (prepare_only(attn_kernel<HS>, smem, &pe)) return pe;
        hipLaunchKernelGGL((attn_kernel<HS>), dim3(c->nhl), dim3(256), smem, c->stream, c->d_q, kc, vc, c->d_xb, c->d_tokpos, c->KVl, c->kv_mul);
        return hipGetLastError();
    });
}

GemvArgs base_args(llmk_ctx* c, int tid, int l, const float* x, const float* norm_w, float* y) {
    GemvArgs a;
    memset(&a, 0, sizeof(a));
    const DevTensor& t = c->t[tid];
    const TensorDesc& d = c->desc[tid];
    const size_t lrows = d.layered ? (size_t)l * d.rows : 0;
    a.W = (const char*)t.data + lrows * t.row_bytes;
    a.row_stride = (int)t.row_bytes;
    a.eps = c->eps;
    a.x = x;
    a.norm_w = norm_w;
    a.y = y;
    a.rows = d.rows;
    a.K = d.K;
    a.rope_freqs = c->d_rope;
    a.tokpos = c->d_tokpos;
    a.E = c->Eq;
    a.KV = c->KVl;
    a.hs = c->hs;
    a.H = c->Hl;
    return a;
}

hipError_t launch_qkv(llmk_ctx* c, int l) {
    GemvArgs a = base_args(c, LLMK_WQKV, l, c->d_x, (const float*)c->t[LLMK_RMS_ATT_WEIGHT].data + (size_t)l * c->E, c->d_q);
    a.kc = c->d_kc + (size_t)l * c->S * c->KVl;
    a.vc = c->d_vc + (size_t)l * c->S * c->KVl;
    return launch_gemv_t<EPI_ROPE_KV, true>(c->cfg.weight_type, c->stream, a, c->n_cu);
}
// Row-parallel GEMVs (wo, w2): with tp_size > 1 each rank contracts over ITS slice of the input and
// writes a PARTIAL x-increment to d_part; the all-reduce + `x += part` follow (tp_reduce_add).
hipError_t launch_wo(llmk_ctx* c, int l) {
    if (c->tp_size > 1 || c->comm || c->p2p) {
        GemvArgs a = base_args(c, LLMK_WO, l, c->d_xb, nullptr, c->d_part);
        return launch_gemv_t<EPI_STORE, false>(c->cfg.weight_type, c->stream, a, c->n_cu);
    }
    GemvArgs a = base_args(c, LLMK_WO, l, c->d_xb, nullptr, c->d_x);
    return launch_gemv_t<EPI_RESID, false>(c->cfg.weight_type, c->stream, a, c->n_cu);
}
hipError_t launch_w13(llmk_ctx* c, int l) {
    GemvArgs a = base_args(c, LLMK_W13, l, c->d_x, (const float*)c->t[LLMK_RMS_FFN_WEIGHT].data + (size_t)l * c->E, c->d_hb);
    return launch_gemv_t<EPI_SWIGLU, true>(c->cfg.weight_type, c->stream, a, c->n_cu);
}
hipError_t launch_w2(llmk_ctx* c, int l) {
    if (c->tp_size > 1 || c->comm || c->p2p) {
        GemvArgs a = base_args(c, LLMK_W2, l, c->d_hb, nullptr, c->d_part);
        return launch_gemv_t<EPI_STORE, false>(c->cfg.weight_type, c->stream, a, c->n_cu);
    }
    GemvArgs a = base_args(c, LLMK_W2, l, c->d_hb, nullptr, c->d_x);
    return launch_gemv_t<EPI_RESID, false>(c->cfg.weight_type, c->stream, a, c->n_cu);
}
hipError_t launch_cls(llmk_ctx* c) {
    // vocab-parallel: this rank's V/P rows land in its slice of the full logits vector
    GemvArgs a = base_args(c, LLMK_WCLS, 0, c->d_x, (const float*)c->t[LLMK_RMS_FINAL_WEIGHT].data,
                           c->d_logits + (size_t)c->tp_rank * c->Vl);
    if (c->t[LLMK_WCLS].type == LLMK_TYPE_Q6_K) {      // raw q6_K rows (a stock q4_0 file's output.weight): q6k.h
        const size_t smem = 16 + (size_t)a.K * sizeof(float);
        const int blocks = (a.rows + GEMV_WAVES * Q6K_RPW - 1) / (GEMV_WAVES * Q6K_RPW);
        hipError_t pe;
        if (prepare_only(gemv_q6k_kernel<true>, smem, &pe)) return pe;
        hipLaunchKernelGGL((gemv_q6k_kernel<true>), dim3(blocks), dim3(GEMV_THREADS), smem, c->stream, a);
        return hipGetLastError();
    }
    return launch_gemv_t<EPI_STORE, true>(c->t[LLMK_WCLS].type, c->stream, a, c->n_cu);   // the classifier may have its own type
}
hipError_t launch_embed(llmk_ctx* c) {
    hipLaunchKernelGGL(embed_kernel, dim3((c->E + 255) / 256), dim3(256), 0, c->stream,
                       (const float*)c->t[LLMK_TOKEN_EMBEDDING_TABLE].data, c->d_tokpos, c->d_x, c->E);
    return hipGetLastError();
}

#define HIPRET(expr)                     \
    do {                                 \
        hipError_t e_ = (expr);          \
        if (e_ != hipSuccess) return e_; \
    } while (0)

// direct = true: token/pos/serial travel as kernel arguments and the logits (+ a sticky error word) are written
// straight into the pinned host buffer, so a token is ONE launch and one stream sync (no copy nodes around it)
// what a launch of the pipelined greedy decode adds to the arguments (all null otherwise)
struct TkGreedy { int gflags = 0, id_index = 0; float* logits = nullptr; };      // logits: llmk_forward's pinned buffer of this position (forward_ahead.h)
template <class TK>
hipError_t launch_token_kernel_t(llmk_ctx* c, bool direct, const TkGreedy& g) {
    TokenArgs a;
    a.gflags = g.gflags | ((TK_DEBUG && getenv("LLMK_TK_NOSYNC")) ? TKG_NOSYNC : 0);   // NOSYNC: libllmk_debug.so only
    a.emb = (const float*)c->t[LLMK_TOKEN_EMBEDDING_TABLE].data;
    a.rms = (const float*)c->t[LLMK_RMS_ATT_WEIGHT].data;      // att | ffn | final in one allocation (llmk_create_tp)
    // q4_0: the unit layout (check_ready built it)
    a.wqkv = TK::Q4 ? c->q16[LLMK_WQKV] : c->t[LLMK_WQKV].data;
    a.wo = TK::Q4 ? c->q16[LLMK_WO] : c->t[LLMK_WO].data;
    a.w13 = TK::Q4 ? c->q16[LLMK_W13] : c->t[LLMK_W13].data;
    a.w2 = TK::Q4 ? c->q16[LLMK_W2] : c->t[LLMK_W2].data;
    a.wcls = (TK::Q4 && !TK::CLSQ6) ? c->q16[LLMK_WCLS] : c->t[LLMK_WCLS].data;      // (q6_K classifier rows stay rows: q6k.h)
    a.kc = c->d_kc;
    a.vc = c->d_vc;
    a.rope = c->d_rope;
    a.tokpos = (direct || g.gflags) ? nullptr : c->d_tokpos;   // immediates: direct mode, and every launch of a greedy pipeline (its own pos and serial)
    a.tok_imm = (g.gflags & TKG_CAND_IN) ? g.id_index : c->h_tokpos[0];   // the token comes from the candidates: the word carries the id's slot
    a.pos_imm = c->h_tokpos[1];
    a.serial_imm = c->h_tokpos[2];
    a.g_qkv = c->d_gran;         // qkv | xb | xa | hb | x (token_kernel.h tk_g_xb ...)
    a.logits = g.logits ? g.logits : direct ? c->h_logits.dev() : c->d_logits;
    a.err = &c->dev_words()->err;
    a.herr = (direct || g.gflags) ? &c->host_words_dev()->err : nullptr;
    a.zeros = c->d_zeros;
#ifdef LLMK_TK_DEBUG
    a.trace = c->d_trace;
#endif
    a.L = c->L;
    a.S = c->S;
    a.eps = c->eps;
    const dim3 grid((TK_DEBUG && c->tk_short_grid) ? TK_NCU - 1 : TK_NCU);
    if (g.gflags) hipLaunchKernelGGL((token_kernel<TK, true>), grid, dim3(TK_THREADS), c->tk_lds, c->stream, a);
    else hipLaunchKernelGGL((token_kernel<TK>), grid, dim3(TK_THREADS), c->tk_lds, c->stream, a);
    return hipGetLastError();
}
// ---- the shapes the persistent kernel is instantiated for -------------------------------------------------------------------
// The reference's dims are seven `parameter` lines (llama2.f90:102-108: edit, make, run); the persistent kernel's are template
// arguments, so a shape is one line here: the built-in list below (BASELINE.json's configurations, the parity shapes, the
// stock-file q6_K variants, Llama-2-7B f16) plus whatever the build adds --
//     make -C llm.f90_amd TK_SHAPES="4096,14336,32,8,32000,WT_F16 5120,13824,40,40,32000,WT_F32"
// turns every "E,H,NH,NKV,V,WT[,CLS]" into X(TkShape<...>) (Makefile: LLMK_TK_EXTRA_SHAPES); TkShape's static_asserts say at
// compile time whether a shape fits the kernel (token_kernel.h).  llmk_tk_shapes() lists them; `llm --vx` prints that list.
#ifndef LLMK_TK_EXTRA_SHAPES
#define LLMK_TK_EXTRA_SHAPES(X)
#endif
#define LLMK_TK_SHAPES(X)                                                                                          \
    X(TkTinyLlama) X(TkSmall) X(TkTinyLlamaF16) X(TkSmallF16) X(TkLlama7BQ4) X(TkTinyLlamaQ4) X(TkLlama7BQ4Q6)     \
    X(TkTinyLlamaQ4Q6) X(TkLlama7BF16) X(TkMistral7BQ4Q6) LLMK_TK_EXTRA_SHAPES(X)
struct TkEntry {
    int E, H, NH, NKV, V, WT, CLS;
    bool q4;                                        // units layout (q16_build) before the first token
    hipError_t (*launch)(llmk_ctx*, bool, const TkGreedy&);
    int (*setup)(llmk_ctx*, int);
};
template <class TK> int tk_setup(llmk_ctx* c, int id);
#define TK_ENTRY(...) {__VA_ARGS__::E, __VA_ARGS__::H, __VA_ARGS__::NH, __VA_ARGS__::NKV, __VA_ARGS__::V, __VA_ARGS__::WT, __VA_ARGS__::CLS, \
                       __VA_ARGS__::Q4, launch_token_kernel_t<__VA_ARGS__>, tk_setup<__VA_ARGS__>},
static const TkEntry tk_table[] = {LLMK_TK_SHAPES(TK_ENTRY)};
#undef TK_ENTRY
constexpr int TK_NSHAPES = (int)(sizeof(tk_table) / sizeof(tk_table[0]));
hipError_t launch_token_kernel(llmk_ctx* c, bool direct = false, const TkGreedy& g = TkGreedy()) {
    if (c->tk_shape < 1 || c->tk_shape > TK_NSHAPES) return hipErrorInvalidValue;
    return tk_table[c->tk_shape - 1].launch(c, direct, g);
}
// the last position of a pipelined greedy run has no next launch to fold its candidates: this does (1 wave)
// (no id while the sticky error word is set, and none from candidates without a finite maximum: see tk_token).  Like tk_token it
// adds TK_ERR_NO_FINITE only to a clear word: behind a range event the drained launches leave candidates that need not be finite,
// and the mark on top would make the host retire the kernel instead of redoing the one position (tk_range_only)
__global__ __launch_bounds__(64) void cand_resolve_kernel(const float2* __restrict__ cand, int* id_out, int* next, unsigned* err, int V) {
    float bv;
    int bi;
    cand_fold(cand, TK_NCU, bv, bi);
    if (threadIdx.x == 0) {
        const bool none = (unsigned)bi >= (unsigned)V;
        const unsigned e = *err;
        if (none && e == 0) atomicOr(err, TK_ERR_NO_FINITE);
        if (!none && e == 0) {
            next[0] = bi + 1;
            __hip_atomic_store(id_out, bi + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// Allocate the exchange state of the persistent kernel if cfg matches the instantiated shape TK.
template <class TK>
int tk_setup(llmk_ctx* c, int id) {
    const llmk_config& g = c->cfg;
    if (c->use_tk || g.emb_dim != TK::E || g.hidden_dim != TK::H || g.n_heads != TK::NH || g.n_kv_heads != TK::NKV ||
        g.vocab_size != TK::V || g.weight_type != TK::WT || c->t[LLMK_WCLS].type != TK::CLS)
        return LLMK_OK;
    // scores + exp(scores)
    const size_t lds = ((size_t)TkLds<TK>::ATT_S + 2 * (size_t)c->S * sizeof(float) + 15) & ~(size_t)15;
    c->tk_lds = lds < 96 * 1024 ? 96 * 1024 : lds;   // > 80 KB: never two workgroups on one CU
    if (c->tk_lds > 160 * 1024) return LLMK_OK;      // context too long for the in-LDS score row: multi-kernel path
    // The kernel spins on its peers, so all TK_NCU workgroups must be co-resident: one per CU by construction (the LDS
    // request excludes a second one), which needs n_cu >= TK_NCU (checked by the caller) and a register/LDS budget the
    // hardware admits.  Assert it with the occupancy query instead of assuming it; a part that cannot host the grid takes
    // the multi-kernel path.  (hipLaunchCooperativeKernel would run the same check per launch for +15-19 us each.)
    HIPCHK(hipFuncSetAttribute((const void*)token_kernel<TK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->tk_lds));
    HIPCHK(hipFuncSetAttribute((const void*)token_kernel<TK, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->tk_lds));
    int per_cu = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, token_kernel<TK>, TK_THREADS, c->tk_lds));
    if (per_cu < 1 || (long long)per_cu * c->n_cu < TK_NCU) return LLMK_OK;
    // qkv | xb | xa | hb | x | per head: the (PMAX - 1) other parts of a long context's attention (HS values + maximum + sum each)
    // (+ 4 granule slots per layer behind them (two buffers by position parity): the q4_0 kernels' per-layer records of the previous position's largest xb / hb elements,
    // token_kernel.h tk_qsc; cleared by llmk_reset)
    static_assert(tk_qsc_front<TK>() == (size_t)TK::QKV + 3 * (size_t)TK::E + TK::H + (size_t)TK::NH * (TkAttPlan<TK>::PMAX - 1) * (TK::HS + 2),
                  "tk_qsc_front: the attention parts are TkAttPlan's");
    const size_t ngran = tk_qsc_front<TK>() + TK_QSC_GRANULES;
    c->tk_ngran = ngran;
    if (!c->d_gran) HIPCHK(c->d_gran.alloc(ngran));      // (kept over a re-type of the classifier: same shape)
    if (!c->d_zeros) HIPCHK(c->d_zeros.alloc((size_t)TK_NCU * TK_WAVES * 1024 / sizeof(float4)));
    if (TK_DEBUG && getenv("LLMK_TK_TRACE")) HIPCHK(c->d_trace.alloc((size_t)TK_NCU * TK_TRACE_N));   // libllmk_debug.so only (a re-setup frees the last one)
    HIPCHK(hipMemset(c->d_gran, 0, ngran * sizeof(unsigned long long)));
    HIPCHK(hipMemset(c->d_zeros, 0, (size_t)TK_NCU * TK_WAVES * 1024));
    c->use_tk = true;
    c->tk_shape = id;
    c->tk.cleared();
    return LLMK_OK;
}

// The whole-token persistent kernel serves the shapes it is instantiated for, on a full 256-CU part.  Called at create and again
// when the classifier gets a type of its own (llmk_set_tensor_type: the q6_K instantiations).
int tk_setup_all(llmk_ctx* c) {
    if ((c->cfg.flags & (LLMK_FLAG_MULTI_KERNEL | LLMK_FLAG_TIMINGS)) || c->n_cu != TK_NCU || c->tp_size != 1 || c->tk.retired) return LLMK_OK;
    int rc = LLMK_OK;
    for (int i = 0; i < TK_NSHAPES && rc == LLMK_OK; ++i) rc = tk_table[i].setup(c, i + 1);      // (the first match takes the ctx)
    return rc;
}

__global__ void bump_serial_kernel(int* tokpos) { tokpos[2] += 1; }

// the q4_0 persistent kernels' per-layer scale records (token_kernel.h tk_qsc): the last *n granules of d_gran; null on a context
// that has none
unsigned long long* tk_qsc_records(const llmk_ctx* c, size_t* n) {
    *n = TK_QSC_GRANULES;
    return c->d_gran && c->tk_ngran ? c->d_gran + (c->tk_ngran - TK_QSC_GRANULES) : nullptr;
}
hipError_t tk_qsc_clear(llmk_ctx* c, hipStream_t st) {
    size_t n;
    unsigned long long* rec = tk_qsc_records(c, &n);
    c->tk.cleared();
    return rec ? hipMemsetAsync(rec, 0, n * sizeof(unsigned long long), st) : hipSuccess;
}
// The records are tagged by position only, and a launch with a range event writes none behind the event: the HOST keeps them those of
// the sequence being fed (invariant R), by tk_recover.h's rules; this is their device side.  Every field of both
// buffers whose tag is not `keep` goes back to zero (tk_qsc_filter).  Off the hot path (a rewind, the end of a pipelined call on a
// range event) and on an idle stream: 4 KB to the host and back
hipError_t tk_qsc_keep(llmk_ctx* c, int keep) {
    size_t n;
    unsigned long long* rec = tk_qsc_records(c, &n);
    if (!rec || keep == TK_KEEP_ALL) return hipSuccess;
    TkQscRecord h[2 * TK_QSC_LMAX];
    static_assert(sizeof(h) == TK_QSC_GRANULES * sizeof(unsigned long long), "two buffers of TK_QSC_LMAX records");
    HIPRET(hipMemcpyAsync(h, rec, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPRET(hipStreamSynchronize(c->stream));
    if (!tk_qsc_filter(h, 2 * TK_QSC_LMAX, keep)) return hipSuccess;
    HIPRET(hipMemcpyAsync(rec, h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    return hipStreamSynchronize(c->stream);      // (h is this frame's)
}
// in front of a token-kernel launch at `pos`: TkRecovery::before_launch has the rule
hipError_t tk_qsc_before_launch(llmk_ctx* c, int pos) {
    return tk_qsc_keep(c, c->tk.before_launch(pos, c->use_tk && tk_table[c->tk_shape - 1].q4));
}

// The two sampler kernels on the logits in d_logits, as EVERY site enqueues them -- the tail of a token pass (enqueue_tail), behind
// each launch of the pipelined decode (decode_run), the verification hooks (sample_logits) -- so that all of them pick one id from
// one vector.  With `penalty`, sample_penalty_kernel first: it records the fed token (where the site has a record to write), then
// adjusts the logits in place by the words in d_pen.  Then sample_filter_kernel, by the words in TkDevWords::filt: it leaves its
// single winner in d_next and, behind a launch of the pipelined decode, in place of that launch's candidates, where the next
// launch's fold and cand_resolve_kernel pick it up like any other candidate (those launches score their classifier rows with the
// greedy words, invT = 0: the cheap tail).  The parameter words travel like token and position: copies out of pinned memory, read
// when a graph replays them.  What differs from site to site:
struct SamplerSite {
    const int* tokpos;      // position and fed token are the pass's device words ...
    int pos, token;         // ... or, without them, these (token 0: none) ...
    const int* prev;        // ... with the id the filter kernel of the position before left on the device in place of `token`
    int* record;            // where the fed token is recorded (d_hist), null: the record is read only
    float2* cand;           // the launch's candidates, replaced by the winner; null and 0: none
    int ncand;
    bool copy_pen, copy_filt;      // the parameter words are copied in front of their kernel (the penalties' at every call; the
                                   // filter's here, or before by the site itself: DevShadow)
    llmk_logprob_record* lp;       // where the position's log-prob record goes (null: none): the raw logits are set aside in front of
                                   // the penalties, and sample_logprob_kernel runs behind the filter kernel on the id in d_next
};
// sample_logprob_kernel behind whatever picked the token: the id in id_ptr, or folded from the candidates, or `id`
hipError_t enqueue_logprob(llmk_ctx* c, const float* logits, const int* id_ptr, const float2* cand, int ncand, int id, llmk_logprob_record* out) {
    hipLaunchKernelGGL(sample_logprob_kernel, dim3(1), dim3(SF_THREADS), 0, c->stream, logits, c->V, id_ptr, cand, ncand, id,
                       &c->dev_words()->lp_top_n, out);
    return hipGetLastError();
}
hipError_t copy_logprob_top(llmk_ctx* c) {      // (top_n travels like token and position: a copy out of pinned memory)
    return hipMemcpyAsync(&c->dev_words()->lp_top_n, c->lp.h_top, sizeof(unsigned), hipMemcpyHostToDevice, c->stream);
}
hipError_t enqueue_sampler(llmk_ctx* c, bool penalty, const SamplerSite& s) {
    TkDevWords* dw = c->dev_words();
    if (penalty) {
        if (s.lp) HIPRET(hipMemcpyAsync(c->lp.raw, c->d_logits, (size_t)c->V * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        if (s.copy_pen) HIPRET(hipMemcpyAsync(c->pen.d_pen, c->pen.h_pen, sizeof(llmk_penalty_params), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(sample_penalty_kernel, dim3(1), dim3(SP_THREADS), 0, c->stream, c->d_logits, c->V, s.tokpos, s.pos, s.token, s.prev,
                           c->pen.d_pen, c->pen.hist, s.record, c->pen.cnt);
        HIPRET(hipGetLastError());
    }
    if (s.copy_filt) HIPRET(hipMemcpyAsync(&dw->filt, c->h_filt, sizeof(llmk_filter_params), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(sample_filter_kernel, dim3(1), dim3(SF_THREADS), 0, c->stream, c->d_logits, c->V, s.tokpos, s.pos, &dw->filt, c->d_next,
                       s.cand, s.ncand, dw->filter_out);
    HIPRET(hipGetLastError());
    return s.lp ? enqueue_logprob(c, penalty ? c->lp.raw : c->d_logits, c->d_next, nullptr, 0, 0, s.lp) : hipSuccess;
}

hipError_t enqueue_tail(llmk_ctx* c, TailMode tail) {
    if (tail != TAIL_LOGITS) {
        llmk_logprob_record* lp = c->lp_top_n >= 0 ? c->lp.d + c->S : nullptr;
        if (lp) HIPRET(copy_logprob_top(c));
        if (tail == TAIL_FILTER || tail == TAIL_PENALTY) {
            HIPRET(enqueue_sampler(c, tail == TAIL_PENALTY, {c->d_tokpos, 0, 0, nullptr, c->pen.hist, nullptr, 0, true, true, lp}));
            lp = nullptr;      // (enqueued)
        } else if (tail == TAIL_SAMPLE) {
            // invT and the seed travel like token and position: a copy out of pinned memory, read when the graph replays it
            HIPRET(hipMemcpyAsync(&c->dev_words()->samp, c->h_samp, sizeof(llmk_sample_params), hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(sample_kernel, dim3(1), dim3(1024), 0, c->stream, c->d_logits, c->V, c->d_tokpos, &c->dev_words()->samp, c->d_next);
        } else {
            hipLaunchKernelGGL(argmax_kernel, dim3(1), dim3(1024), 0, c->stream, c->d_logits, c->V, c->d_next);
        }
        HIPRET(hipGetLastError());
        if (lp) HIPRET(enqueue_logprob(c, c->d_logits, c->d_next, nullptr, 0, 0, lp));
        if (c->lp_top_n >= 0) HIPRET(hipMemcpyAsync(c->lp.h + c->S, c->lp.d + c->S, sizeof(llmk_logprob_record), hipMemcpyDeviceToHost, c->stream));
        HIPRET(hipMemcpyAsync(&c->h_next->id, c->d_next, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPRET(hipMemcpyAsync(&c->h_next->err, &c->dev_words()->err, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    } else {      // the logits and, behind them, the error word: TkDevWords::err lands in TkHostWords::err
        HIPRET(hipMemcpyAsync(c->h_logits, c->d_logits, (size_t)c->V * sizeof(float) + sizeof(TkDevWords::err), hipMemcpyDeviceToHost, c->stream));
    }
    return hipSuccess;
}

__global__ void add_kernel(float* __restrict__ x, const float* __restrict__ part, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] += part[i];
}
hipError_t launch_add_partial(llmk_ctx* c) {   // x += all-reduced partial (the residual of wo / w2)
    hipLaunchKernelGGL(add_kernel, dim3((c->E + 255) / 256), dim3(256), 0, c->stream, c->d_x, c->d_part, c->E);
    return hipGetLastError();
}

// Tensor-parallel token pass over RCCL: two all-reduces of E floats per layer (ring order is fixed by the
// communicator, so every rank sees bit-identical sums), one all-gather of the logits.
int enqueue_token_tp(llmk_ctx* c) {
    if (!c->comm) return LLMK_E_COMM;
#define NC(expr) do { if ((expr) != ncclSuccess) return LLMK_E_COMM; } while (0)
    HIPCHK(hipMemcpyAsync(c->d_tokpos, c->h_tokpos, 4 * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_embed(c));
    for (int l = 0; l < c->L; ++l) {
        HIPCHK(launch_qkv(c, l));
        HIPCHK(launch_attn(c, l));
        HIPCHK(launch_wo(c, l));
        NC(ncclAllReduce(c->d_part, c->d_part, c->E, ncclFloat, ncclSum, c->comm, c->stream));
        HIPCHK(launch_add_partial(c));
        HIPCHK(launch_w13(c, l));
        HIPCHK(launch_w2(c, l));
        NC(ncclAllReduce(c->d_part, c->d_part, c->E, ncclFloat, ncclSum, c->comm, c->stream));
        HIPCHK(launch_add_partial(c));
    }
    HIPCHK(launch_cls(c));
    NC(ncclAllGather(c->d_logits + (size_t)c->tp_rank * c->Vl, c->d_logits, c->Vl, ncclFloat, c->comm, c->stream));
#undef NC
    return LLMK_OK;
}

// Enqueue one token pass on c->stream.  timed: bracket the reference's five sections with events.
// jseed != 0: the jittered instantiation (llmk_tp_p2p_stress only)
hipError_t launch_tp_allreduce_add(llmk_ctx* c, int call, unsigned jseed = 0) {   // x += sum over ranks of d_part   (:603-605, :618-620)
    const dim3 grid((c->E + 255) / 256), block(256);
    unsigned* err = &c->dev_words()->err;
    if (jseed) hipLaunchKernelGGL(tp_allreduce_add_kernel<true>, grid, block, 0, c->stream, c->peers, c->d_part, c->d_x, c->d_tokpos, call,
                                  2 * c->L, c->tp_rank, c->tp_size, c->E, err, jseed);
    else hipLaunchKernelGGL(tp_allreduce_add_kernel<false>, grid, block, 0, c->stream, c->peers, c->d_part, c->d_x, c->d_tokpos, call,
                            2 * c->L, c->tp_rank, c->tp_size, c->E, err, 0u);
    return hipGetLastError();
}
hipError_t launch_tp_allgather(llmk_ctx* c, unsigned jseed = 0) {   // every rank's classifier rows into every rank's logits   (:634-636)
    const dim3 grid((c->V + 255) / 256), block(256);
    unsigned* err = &c->dev_words()->err;
    if (jseed) hipLaunchKernelGGL(tp_allgather_kernel<true>, grid, block, 0, c->stream, c->peers, c->d_logits, c->d_tokpos, 2 * c->L,
                                  c->tp_rank, c->tp_size, c->E, c->V, err, jseed);
    else hipLaunchKernelGGL(tp_allgather_kernel<false>, grid, block, 0, c->stream, c->peers, c->d_logits, c->d_tokpos, 2 * c->L,
                            c->tp_rank, c->tp_size, c->E, c->V, err, 0u);
    return hipGetLastError();
}

// One token pass on the stream.  tk: the persistent kernel (the path of a ctx with use_tk), else the multi-kernel launches -- which such
// a ctx also takes, eagerly, for a position its kernel could not hold (token_pass).  Tensor-parallel ranks have one path
hipError_t enqueue_token(llmk_ctx* c, TailMode tail, bool timed, bool tk) {
    HIPRET(hipMemcpyAsync(c->d_tokpos, c->h_tokpos, 4 * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (c->p2p) {   // tensor-parallel over peer memory: the whole token is stream work (replayable from a hipGraph)
        HIPRET(launch_embed(c));
        for (int l = 0; l < c->L; ++l) {
            HIPRET(launch_qkv(c, l));
            HIPRET(launch_attn(c, l));
            HIPRET(launch_wo(c, l));
            HIPRET(launch_tp_allreduce_add(c, 2 * l));
            HIPRET(launch_w13(c, l));
            HIPRET(launch_w2(c, l));
            HIPRET(launch_tp_allreduce_add(c, 2 * l + 1));
        }
        HIPRET(launch_cls(c));
        HIPRET(launch_tp_allgather(c));
        return enqueue_tail(c, tail);
    }
    if (tk) {
        HIPRET(launch_token_kernel(c));
        return enqueue_tail(c, tail);
    }
    HIPRET(launch_embed(c));
    for (int l = 0; l < c->L; ++l) {
        if (timed) HIPRET(hipEventRecord(c->ev[0], c->stream));
        HIPRET(launch_qkv(c, l));
        if (timed) HIPRET(hipEventRecord(c->ev[1], c->stream));
        HIPRET(launch_attn(c, l));
        if (timed) HIPRET(hipEventRecord(c->ev[2], c->stream));
        HIPRET(launch_wo(c, l));
        HIPRET(launch_w13(c, l));
        HIPRET(launch_w2(c, l));
        if (timed) {
            HIPRET(hipEventRecord(c->ev[3], c->stream));
            HIPRET(hipEventSynchronize(c->ev[3]));
            float ms;
            // section 1 = rmsnorm+QKV (:526-538); 2 = RoPE (:541-561) is fused into 1's epilogue;
            // 3 = attention (:570-599); 4 = wo+FFN (:601-622)
            HIPRET(hipEventElapsedTime(&ms, c->ev[0], c->ev[1])); c->times[0] += ms;
            HIPRET(hipEventElapsedTime(&ms, c->ev[1], c->ev[2])); c->times[2] += ms;
            HIPRET(hipEventElapsedTime(&ms, c->ev[2], c->ev[3])); c->times[3] += ms;
        }
    }
    if (timed) HIPRET(hipEventRecord(c->ev[4], c->stream));
    HIPRET(launch_cls(c));
    if (timed) {
        HIPRET(hipEventRecord(c->ev[5], c->stream));
        HIPRET(hipEventSynchronize(c->ev[5]));
        float ms;
        HIPRET(hipEventElapsedTime(&ms, c->ev[4], c->ev[5])); c->times[4] += ms;  // 5 = final norm + classifier
    }
    return enqueue_tail(c, tail);
}

// (the graphs bake in kernel arguments, the path and the tensor types: whatever changes one of those drops them all)
void drop_graphs(llmk_ctx* c) {
    for (auto& per_tail : c->graph)
        for (hipGraphExec_t& g : per_tail)
            if (g) { hipGraphExecDestroy(g); g = nullptr; }
}
int build_graph(llmk_ctx* c, TailMode tail, hipGraphExec_t* out) {
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    hipError_t e = enqueue_token(c, tail, false, c->use_tk);
    hipError_t e2 = hipStreamEndCapture(c->stream, &g);
    if (e != hipSuccess) { if (g) hipGraphDestroy(g); return LLMK_E_HIP + (int)e; }
    HIPCHK(e2);
    e = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
    hipGraphDestroy(g);
    HIPCHK(e);
    return LLMK_OK;
}

int tensors_ready(llmk_ctx* c) {
    for (int i = 0; i < LLMK_N_TENSORS; ++i)
        if (!c->t[i].uploaded) return LLMK_E_STATE;
    if (c->use_tk && tk_table[c->tk_shape - 1].q4 && c->q16_dirty) return q16_build(c);
    return LLMK_OK;
}
// Every entry point that works on a context's stream or buffers passes through here -- or, where it has no use for the tensors,
// calls spec_settle itself -- before it touches them: a position llmk_forward left in flight (forward_ahead.h) is drained first.
// llmk_forward alone goes by tensors_ready.
int spec_settle(llmk_ctx* c);
int check_ready(llmk_ctx* c) {
    if (!c) return LLMK_E_ARG;
    const int rc = spec_settle(c);
    return rc ? rc : tensors_ready(c);
}

// debug library only (LLMK_TK_INJECT_TIMEOUT=pos): the token kernel is launched one workgroup short at this position, so its peers
// really time out
bool tk_inject_timeout(int pos) {
    const char* at = TK_DEBUG ? getenv("LLMK_TK_INJECT_TIMEOUT") : nullptr;
    return at && atoi(at) == pos;
}
// the sticky word a completed pass left on the host: behind the logits, or with the tail's id
unsigned tk_pass_err(const llmk_ctx* c, TailMode tail) { return tail != TAIL_LOGITS ? c->h_next->err : c->host_words()->err; }
int tk_clear_err(llmk_ctx* c) {
    HIPCHK(hipMemsetAsync(&c->dev_words()->err, 0, sizeof(unsigned), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->host_words()->err = 0;
    c->h_next->err = 0;
    return LLMK_OK;
}
// What TkRecovery (tk_recover.h) answered to the word `code` of the launch at `pos`, carried out.  The word is sticky by design (every
// CU drains instead of spinning on), so all but CLEAN clear it.  RETIRE: the kernel reported a timed-out exchange (its workgroups were
// not all running: the GPU was shared, or a wedged peer) or a model it cannot hold -- the ctx leaves the token kernel for good and the
// user is told once.  After REDO and RETIRE the caller runs the SAME position on the multi-kernel path, which rewrites that
// position's KV rows and recomputes x from the embedding: nothing of the failed launch survives.
int tk_perform(llmk_ctx* c, TkVerdict what, unsigned code, int pos) {
    if (what == TkVerdict::CLEAN) return LLMK_OK;
    const int rc = tk_clear_err(c);
    if (rc || what != TkVerdict::RETIRE) return rc;
    c->use_tk = false;
    c->tk.retired = true;
    drop_graphs(c);
    for (DevBuf<char>& units : c->q16) units.reset();       // the q4_0 kernels' second copy of the matrices (3.8 GB at 7B): nobody reads it again
    c->q16_dirty = true;
    fprintf(stderr, "llmk: the persistent token kernel %s (code 0x%x, position %d); this context continues on the multi-kernel path\n",
            tk_err_words(code), code, pos);
    return LLMK_OK;
}

// the sticky word of a timed-out peer-memory exchange (tp_p2p.h tp_err_code), in words
const char* tp_describe_err(const llmk_ctx* c, unsigned code, char* buf, size_t n) {
    if ((code >> 28) != 3u) { snprintf(buf, n, "code 0x%x", code); return buf; }
    const unsigned per = 2u * (unsigned)c->L + 1u, e24 = code & 0xffffffu;
    // the epoch's low 24 bits, completed with the host's serial (the device's can be at most a graph replay ahead)
    const unsigned cur = (unsigned)c->h_tokpos[2] * per + per;
    unsigned epoch = (cur & ~0xffffffu) | e24;
    if (epoch > cur) epoch -= 0x1000000u;
    const unsigned serial = (epoch - 1u) / per, call = (epoch - 1u) % per;
    if (call == per - 1u) snprintf(buf, n, "code 0x%x: rank %u's logits slice never arrived (all-gather of serial %u)", code, (code >> 24) & 15u, serial);
    else snprintf(buf, n, "code 0x%x: rank %u's partial never arrived (all-reduce %u of serial %u: layer %u, %s)", code, (code >> 24) & 15u,
                  call, serial, call / 2u, (call & 1u) ? "w2" : "wo");
    return buf;
}
// A speculative launch of llmk_forward may be in flight: wait for it, look at the sticky word as run_token_pass does, and leave the
// machine IDLE.  A launch nobody waits for is an ordinary token pass: it ends by itself, and all it leaves behind is KV row `next`
// with the guessed token's K/V, which every path rewrites before reading it.  TkRecovery::settled says what its word means: no finite
// candidate clears it, anything else retires the kernel and the next pass runs on the multi-kernel path.
// The device's word is read, not the host's copy: only workgroups that noticed the raised word store it there.
int spec_settle(llmk_ctx* c) {
    c->fa.interrupt();
    if (!c->fa_inflight) return LLMK_OK;
    HIPCHK(hipSetDevice(c->cfg.device));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->fa_inflight = false;
    c->h_tokpos[0] = c->fa_tok0;
    c->h_tokpos[1] = c->fa_pos;
    unsigned err = 0;
    HIPCHK(hipMemcpy(&err, &c->dev_words()->err, sizeof(unsigned), hipMemcpyDeviceToHost));
    return tk_perform(c, TkRecovery::settled(err), err, c->fa_pos + 1);
}

int token_pass(llmk_ctx* c, int token, int pos, TailMode tail);
int run_token_pass(llmk_ctx* c, int token, int pos, TailMode tail) {
    const int rc = check_ready(c);
    return rc ? rc : token_pass(c, token, pos, tail);
}
int token_pass(llmk_ctx* c, int token, int pos, TailMode tail) {
    int rc;
    if (token < 1 || token > c->V || pos < 1 || pos > c->S) return LLMK_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    c->h_tokpos[0] = token - 1;
    c->h_tokpos[1] = pos;
    HIPCHK(tk_qsc_before_launch(c, pos));
    const bool timed = (c->cfg.flags & LLMK_FLAG_TIMINGS) != 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        c->h_tokpos[2] += 1;  // token serial: makes every exchange epoch of this pass unique
        c->tk_short_grid = c->use_tk && tk_inject_timeout(pos);
        if ((c->tp_size > 1 || c->comm) && !c->p2p) {   // tensor-parallel over RCCL: eager launches with the collectives in between
            rc = enqueue_token_tp(c);
            if (rc) return rc;
            HIPCHK(enqueue_tail(c, tail));
        } else if (timed || (c->cfg.flags & LLMK_FLAG_NO_GRAPH)) {
            HIPCHK(enqueue_token(c, tail, timed, c->use_tk));
        } else if (c->use_tk && tail == TAIL_LOGITS && c->tk_direct) {
            c->host_words()->err = 0;
            HIPCHK(launch_token_kernel(c, true));
        } else {
            hipGraphExec_t* g = &c->graph[tail][c->lp_top_n >= 0 ? 1 : 0];
            if (!*g) {
                rc = build_graph(c, tail, g);
                if (rc) return rc;
            }
            HIPCHK(hipGraphLaunch(*g, c->stream));
        }
        HIPCHK(hipStreamSynchronize(c->stream));
        if (c->p2p) {   // a peer never delivered its granules: the sticky word says so (cleared by llmk_reset)
            const unsigned perr = tk_pass_err(c, tail);
            char what[160];
            if (perr) fprintf(stderr, "llmk: rank %d of %d: a peer's granules never arrived (%s; position %d, serial %d)\n",
                              c->tp_rank, c->tp_size, tp_describe_err(c, perr, what, sizeof(what)), pos, c->h_tokpos[2]);
            return perr ? LLMK_E_TIMEOUT : LLMK_OK;
        }
        if (!c->use_tk) return LLMK_OK;
        const unsigned err = tk_pass_err(c, tail);
        const TkRecovery::Single v = c->tk.single(err);
        if (v.first_event)
            fprintf(stderr, "llmk: position %d holds an activation beyond the f16 range of the persistent q4_0 kernel's operands (code 0x%x): that "
                            "position is redone on the multi-kernel path, the kernel stays in use\n", pos, err);
        rc = tk_perform(c, v.what, err, pos);
        if (rc || v.what == TkVerdict::CLEAN) return rc;
        if (v.what == TkVerdict::REDO) {
            // THIS position on the multi-kernel path (f32 activations throughout; eager launches: the ctx's graphs hold the token
            // kernel), the persistent kernel again from the next one
            HIPCHK(enqueue_token(c, tail, false, false));
            HIPCHK(hipStreamSynchronize(c->stream));
            return LLMK_OK;
        }
        // (retired: once more, on the multi-kernel path)
    }
    return LLMK_E_TIMEOUT;
}
// ... and the shadows of the words its tail copies to the device: known again once the pass is through
int run_token(llmk_ctx* c, int token, int pos, TailMode tail) {
    const bool filt = tail == TAIL_FILTER || tail == TAIL_PENALTY, samp = tail == TAIL_SAMPLE;
    if (filt) c->filt_dev.invalidate();
    if (samp) c->samp_dev.invalidate();
    const int rc = run_token_pass(c, token, pos, tail);
    if (rc == LLMK_OK && filt) c->filt_dev.confirm(*c->h_filt);
    if (rc == LLMK_OK && samp) c->samp_dev.confirm(*c->h_samp);
    return rc;
}

// ---- batched prefill (prefill.h) ------------------------------------------------------------------------
// GEMM plan: row groups per wave, units per block and workgroups per CU (prefill.h PfGemmArgs).  Every candidate
// is priced with the measured step times (tests/host_tools/pf_trace.py, round 2): a step of NR row groups at 128
// positions keeps a SIMD's matrix core busy for 1.7*NR us per resident wave, plus ~0.5 us of barrier / staging per step;
// the first weights take ~4 us to arrive and every partial tile costs a write and a read in the epilogue.
// measured step times of pf_gemm_h_kernel at 128 positions, one / two row groups per wave (us; tests/host_tools/pf_trace.py
// --type f16 | q4_0, round 3): the activation tile costs the same either way
#ifndef LLMK_PF_H_STEP1
#define LLMK_PF_H_STEP1 1.00
#define LLMK_PF_H_STEP2 1.32
#define LLMK_PF_HQ_STEP1 1.20
#define LLMK_PF_HQ_STEP2 1.92
#endif
struct PfPlan { int nr, nk, total, U, grid; };
// wt: the matrix's own type where it differs from the context's (the classifier: llmk_set_tensor_type), -1 = the context's
PfPlan pf_plan(const llmk_ctx* c, int rows, int K, int T = PF_TMAX, int wt = -1) {
    if (wt < 0) wt = c->cfg.weight_type;
    // ONE workgroup per CU (pinned by the LDS request), one or two 16-row groups per wave.  Step times measured at 128
    // positions (tests/host_tools/pf_trace.py, profiles/README.md round 2): 2.45 us with one row group, 4.25 us with two;
    // ~4 us until the first weights arrive; every partial tile is written once and read once by the epilogue.  Also
    // measured and dropped: two workgroups per CU (their waves share the SIMDs' matrix cores: same step rate per CU, but
    // the pairs drift apart and the kernel waits for the slower one) and eight waves per workgroup (two per SIMD in step).
    // Four row groups per wave (128 accumulator registers, 256-row strips): step 8.2 us for 512 MFMAs -- 87 % of the matrix rate
    // in the loop against 84 % with two, eaten by the coarser units (TinyLlama w1|w3 67.9 vs 62.2 us; Llama-2-7B q4_0 +0.4 %).
    // f16 weights on the f16 instruction (pf_gemm_h_kernel): a step is 8x less matrix work
    static const double step_f32[2] = {2.45, 4.25}, step_h[2] = {LLMK_PF_H_STEP1, LLMK_PF_H_STEP2}, step_hq[2] = {LLMK_PF_HQ_STEP1, LLMK_PF_HQ_STEP2};
    // (f32 weights: three instructions per chunk, as q4_0; q4_0 at whole batches: the two-group strip runs on eight waves, pf_gemm_launch)
    static const double step_q8[2] = {LLMK_PF_HQ_STEP1, LLMK_PF_HQ_STEP2 * 0.925};
    // q6_K rows (the classifier of a stock q4_0 file, f16 instruction only): the same three instructions per chunk as q4_0 and ~1.3x its
    // integer work per weight (two planes to merge); four waves at every batch length; see pf_gemm_h_kernel.  The factor 1.3 is an ESTIMATE
    // from the instruction counts, not a pf_trace measurement: 2.5 us per step of two row groups, where kernel 12 on Llama-2-7B gives
    // 140.9 us / 64 units = 2.2 us with ring fill and flush included (profiles/q6k_gemm.txt section 4); one row group was not timed alone
    static const double step_q6[2] = {LLMK_PF_HQ_STEP1 * 1.3, LLMK_PF_HQ_STEP2 * 1.3};
    const bool q6 = wt == LLMK_TYPE_Q6_K;
    const double* step_us = !c->pf_hm ? step_f32 : wt == LLMK_TYPE_F16 ? step_h : q6 ? step_q6
                            : (wt == LLMK_TYPE_Q4_0 && (T + 15) / 16 == 8) ? step_q8 : step_hq;
    PfPlan best{};
    double best_t = 1e30;
    for (int nr = 1; nr <= 2; ++nr) {
        const int sr = 64 * nr;
        if (nr == 2 && rows % sr) continue;
#ifdef LLMK_PF_TRACE
        if (const char* f = getenv("LLMK_PF_PLAN"))          // debug build: force the row groups per wave (when the shape allows it)
            if (atoi(f) != nr && !(rows % 128)) continue;
#endif
        PfPlan p;
        p.nr = nr;
        p.nk = K / PF_KSTEP;
        p.total = (rows + sr - 1) / sr * p.nk;
        p.U = (p.total + c->n_cu - 1) / c->n_cu;
        if (q6) p.U = (p.U + 1) & ~1;       // a q6_K ring stage is a pair of steps: every block starts on an even step (total is a multiple of 4)
        p.grid = (p.total + p.U - 1) / p.U;
        // before the first step and after the last: the f16-instruction kernel's ring takes 2.8 / 4.6 us to fill and its last
        // step (the flush) runs 0.5 / 1.4 us over, one / two row groups (block timelines, round 3); the f32 kernel: ~4 us
        const double fixed = !c->pf_hm ? 4.0 : nr == 1 ? 3.3 : 6.0;
        const double t = fixed + p.U * step_us[nr - 1] + 0.15 * ((p.nk - 1) / p.U + 1);
        if (t < best_t) { best_t = t; best = p; }
    }
    return best;
}
int pf_max_slots(const PfPlan& p) { return (p.nk - 1) / p.U + 2; }
hipError_t pf_prepare(const llmk_ctx* c);
// Workspaces, the second lane's stream, the KV events and the kernels' dynamic-LDS limits, built aside: the context gets them only
// after the LAST step succeeded; a failure part-way releases everything again, so a later llmk_prefill starts the setup over
// instead of launching on null buffers.
// choose: a setup from scratch also picks the matrix instruction (the f16 one unless LLMK_PF_F32_MFMA=1) -- llmk_prefill and the
// timing hook both say so, so that a hook called first (or after a redo that dropped the workspaces) cannot leave the context on
// the slow instruction (advisor, round 5); the redo in llmk_prefill sets pf_hm = false itself and does not
int pf_setup(llmk_ctx* c, bool choose = false) {
    if (c->pf) return LLMK_OK;
    if (choose) c->pf_hm = !(getenv("LLMK_PF_F32_MFMA") && getenv("LLMK_PF_F32_MFMA")[0] == '1');
    auto pf = std::make_unique<llmk_ctx::Prefill>();
    const size_t T = PF_TMAX;
    HIPCHK(pf->flag.alloc(1));
    HIPCHK(hipMemset(pf->flag, 0, sizeof(unsigned)));
    const int rows[4] = {c->E + 2 * c->KV, c->E, 2 * c->H, c->E};
    size_t pcap = 0;
    const int Ks[4] = {c->E, c->E, c->E, c->H};
    for (int i = 0; i < 4; ++i)
        for (int t : {(int)PF_TMAX, 96}) pcap = std::max(pcap, (size_t)pf_max_slots(pf_plan(c, rows[i], Ks[i], t)) * T * rows[i]);   // (the plan may depend on the batch length)
    c->pf_pcap = pcap;
    HIPCHK(pf_prepare(c));
    for (int i = 0; i < 2; ++i) {
        PfLane& w = pf->lane[i];
        for (DevBuf<float>* x : {&w.X, &w.Xs, &w.Q, &w.XB}) HIPCHK(x->alloc(T * c->E));
        HIPCHK(w.HB.alloc(T * c->H));
        HIPCHK(w.P.alloc(pcap));
        HIPCHK(w.xn.alloc(T));
        HIPCHK(w.lowcnt.alloc(2 * T));
        HIPCHK(hipMemset(w.lowcnt, 0, 2 * T * sizeof(unsigned)));
        if (i == 1) HIPCHK(w.own.create(hipStreamNonBlocking));
        w.stream = i == 0 ? (hipStream_t)c->stream : (hipStream_t)w.own;
        w.kv.resize(c->L);
        for (Event& e : w.kv) HIPCHK(e.create(hipEventDisableTiming));
        HIPCHK(w.done.create(hipEventDisableTiming));
    }
    HIPCHK(pf->start.create(hipEventDisableTiming));
    HIPCHK(pf->tok.alloc((size_t)c->S));
    c->pf = std::move(pf);
    return LLMK_OK;
}
// dynamic-LDS request of pf_gemm_kernel<NG, *, NR> (> half of the CU's 160 KB: pins one workgroup per CU, so every CU
// gets one block of equal length)
template <int NG, int NR>
constexpr size_t pf_gemm_smem() {
    const size_t need = ((size_t)2 * NG * 16 * PF_LDW + (size_t)NG * 16 * (64 * NR + PF_TPAD)) * sizeof(float);
    return need > (size_t)84 * 1024 ? need : (size_t)84 * 1024;
}
template <int NG, int NR>
constexpr size_t pf_gemm_h_smem() {
    const size_t need = (size_t)4 * NG * 16 * PF_HP * sizeof(_Float16) + (size_t)NG * 16 * (64 * NR + PF_TPAD) * sizeof(float);
    return need > (size_t)84 * 1024 ? need : (size_t)84 * 1024;
}
// The limits are raised ONCE, in pf_setup (as g_prepare does for the decode kernels): a launch is a launch, with no
// runtime call in the 5 us gaps between the prefill's dependent kernels, and an LDS failure surfaces at setup.
template <int NG, int WT>
hipError_t pf_gemm_prepare_one() {
    HIPRET(hipFuncSetAttribute((const void*)pf_gemm_kernel<NG, WT, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pf_gemm_smem<NG, 1>()));
    return hipFuncSetAttribute((const void*)pf_gemm_kernel<NG, WT, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pf_gemm_smem<NG, 2>());
}
template <int NG, int WT>
hipError_t pf_gemm_h_prepare_one() {
    HIPRET(hipFuncSetAttribute((const void*)pf_gemm_h_kernel<NG, 1, WT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pf_gemm_h_smem<NG, 1>()));
    return hipFuncSetAttribute((const void*)pf_gemm_h_kernel<NG, 2, WT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pf_gemm_h_smem<NG, 2>());
}
template <int WT>
hipError_t pf_gemm_h_prepare() {
    if constexpr (WT == WT_Q4_0)      // (the eight-wave form of the 128-row strip: pf_gemm_launch)
        HIPRET(hipFuncSetAttribute((const void*)pf_gemm_h_kernel<8, 1, WT, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pf_gemm_h_smem<8, 2>()));
    HIPRET((pf_gemm_h_prepare_one<1, WT>())); HIPRET((pf_gemm_h_prepare_one<2, WT>())); HIPRET((pf_gemm_h_prepare_one<3, WT>())); HIPRET((pf_gemm_h_prepare_one<4, WT>()));
    HIPRET((pf_gemm_h_prepare_one<5, WT>())); HIPRET((pf_gemm_h_prepare_one<6, WT>())); HIPRET((pf_gemm_h_prepare_one<7, WT>()));
    return pf_gemm_h_prepare_one<8, WT>();
}
template <int WT>
hipError_t pf_gemm_prepare() {
    HIPRET((pf_gemm_prepare_one<1, WT>())); HIPRET((pf_gemm_prepare_one<2, WT>())); HIPRET((pf_gemm_prepare_one<3, WT>()));
    HIPRET((pf_gemm_prepare_one<4, WT>())); HIPRET((pf_gemm_prepare_one<5, WT>())); HIPRET((pf_gemm_prepare_one<6, WT>()));
    HIPRET((pf_gemm_prepare_one<7, WT>()));
    return pf_gemm_prepare_one<8, WT>();
}
hipError_t pf_prepare_type(int wt) {
    switch (wt) {
        case LLMK_TYPE_Q4_0: HIPRET(pf_gemm_prepare<WT_Q4_0>()); return pf_gemm_h_prepare<WT_Q4_0>();
        case LLMK_TYPE_F16: HIPRET(pf_gemm_prepare<WT_F16>()); return pf_gemm_h_prepare<WT_F16>();
        case LLMK_TYPE_Q6_K: return pf_gemm_h_prepare<WT_Q6_K>();      // (classifier rows; no form on the f32 instruction: sc_plan)
        default: HIPRET(pf_gemm_prepare<WT_F32>()); return pf_gemm_h_prepare<WT_F32>();
    }
}
hipError_t pf_prepare(const llmk_ctx* c) {
    HIPRET(pf_prepare_type(c->cfg.weight_type));
    // the classifier's own GEMM kernels (llmk_score, llmk_batch_*, llmk_time_kernel 12), where its type differs; llmk_set_tensor_type
    // tears the workspaces down when that type changes, so the next setup comes through here again
    const int ct = c->t[LLMK_WCLS].type;
    if (ct != c->cfg.weight_type) HIPRET(pf_prepare_type(ct));
    return with_head_size(c->hs, [](auto hs) {
        constexpr int HS = decltype(hs)::value;
        return hipFuncSetAttribute((const void*)pf_attn_kernel<HS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attn_smem(PF_ATT_WAVES, HS));
    });
}
template <int NG, int NR>
hipError_t pf_gemm_launch(llmk_ctx* c, const PfLane& w, const PfGemmArgs& a, const PfPlan& p, int wt) {
    constexpr size_t smem = pf_gemm_smem<NG, NR>();
    const dim3 grid(p.grid), block(PF_WAVES * WAVE);
    if (c->pf_hm) {
        constexpr size_t smem_h = pf_gemm_h_smem<NG, NR>();
        if constexpr (NG == 8 && NR == 2) {
            // q4_0, whole batches: the same 128-row strips on EIGHT waves of one row group each -- two waves per SIMD, one wave's nibble
            // arithmetic under the other's matrix instructions (round 5, profiles/r05_prefill_eight_waves.txt: w1|w3 GEMM 33.0 -> 30.9 us on
            // TinyLlama q4_0, 96.2 -> 88.8 at 7B; f16 and f32 weights, which have no such arithmetic, lose 4-6 % to the doubled LDS reads)
            if (wt == LLMK_TYPE_Q4_0) {
                hipLaunchKernelGGL((pf_gemm_h_kernel<8, 1, WT_Q4_0, 8>), grid, dim3(8 * WAVE), smem_h, w.stream, a, c->pf->flag, w.lowcnt);
                return hipGetLastError();
            }
        }
        if (wt == LLMK_TYPE_Q4_0) hipLaunchKernelGGL((pf_gemm_h_kernel<NG, NR, WT_Q4_0>), grid, block, smem_h, w.stream, a, c->pf->flag, w.lowcnt);
        else if (wt == LLMK_TYPE_Q6_K) hipLaunchKernelGGL((pf_gemm_h_kernel<NG, NR, WT_Q6_K>), grid, block, smem_h, w.stream, a, c->pf->flag, w.lowcnt);
        else if (wt == LLMK_TYPE_F16) hipLaunchKernelGGL((pf_gemm_h_kernel<NG, NR, WT_F16>), grid, block, smem_h, w.stream, a, c->pf->flag, w.lowcnt);
        else hipLaunchKernelGGL((pf_gemm_h_kernel<NG, NR, WT_F32>), grid, block, smem_h, w.stream, a, c->pf->flag, w.lowcnt);
        return hipGetLastError();
    }
    if (wt == LLMK_TYPE_Q6_K) return hipErrorInvalidValue;      // (sc_plan keeps q6_K rows off the f32 instruction)
    if (wt == LLMK_TYPE_Q4_0) hipLaunchKernelGGL((pf_gemm_kernel<NG, WT_Q4_0, NR>), grid, block, smem, w.stream, a);
    else if (wt == LLMK_TYPE_F16) hipLaunchKernelGGL((pf_gemm_kernel<NG, WT_F16, NR>), grid, block, smem, w.stream, a);
    else hipLaunchKernelGGL((pf_gemm_kernel<NG, WT_F32, NR>), grid, block, smem, w.stream, a);
    return hipGetLastError();
}
hipError_t pf_gemm(llmk_ctx* c, const PfLane& w, const void* W, int row_stride, const float* X, int rows, int K, int T, PfEpiArgs* e, int wt = -1) {
    if (wt < 0) wt = c->cfg.weight_type;
    const PfPlan p = pf_plan(c, rows, K, T, wt);
    PfGemmArgs a;
    a.W = W; a.X = X; a.P = w.P; a.rows = rows; a.K = K; a.T = T; a.RS = row_stride;
    a.nk = p.nk; a.U = p.U; a.total = p.total;
#ifdef LLMK_PF_TRACE
    a.trace = (unsigned long long*)(X == w.HB ? w.Q : w.HB).get();   // debug build: stamps land in the SwiGLU buffer (llmk_peek 7); the w2 GEMM reads that one: its stamps go to the (dead) q buffer
#endif
    e->U = p.U; e->nk = p.nk; e->sh = p.nr == 2 ? 7 : 6;
    e->lowcnt = c->pf_hm ? w.lowcnt : nullptr; e->flag = c->pf->flag; e->gemm_blocks = p.grid;
#define PF_CASE(NG_)                                                                         \
    case NG_: return p.nr == 2 ? pf_gemm_launch<NG_, 2>(c, w, a, p, wt) : pf_gemm_launch<NG_, 1>(c, w, a, p, wt)
    switch ((T + 15) / 16) {
        PF_CASE(1); PF_CASE(2); PF_CASE(3); PF_CASE(4); PF_CASE(5); PF_CASE(6); PF_CASE(7);
        default: return p.nr == 2 ? pf_gemm_launch<8, 2>(c, w, a, p, wt) : pf_gemm_launch<8, 1>(c, w, a, p, wt);
    }
#undef PF_CASE
}
// ---- llmk_score: classifier + log-softmax for every position of a batch (prefill.h pf_score_kernel) ----
// What a scoring call asks of its batches: the call's targets are in sc_targets, its results go to sc_out (log-probs, then ids)
struct ScPlan { int R, nchunks, nparts; };
struct ScoreJob {
    bool want_lp, want_logits;
    int n;                   // positions of the call
    ScPlan sp;               // the classifier's row chunks: sc_plan, once per call (it depends on the context and its matrix instruction; q6_K rows: and on the batch's rows, sc_batch)
    float* out = nullptr;    // where the log-probs and ids go instead of sc_out, and the logits instead of sc_logits (a batch's own: llmk_batch_*)
    float* logits = nullptr;
};
// The classifier GEMM runs in chunks of R rows (a multiple of 128, or all V rows) whose partial tiles fit the workspace the layers'
// GEMMs already have: V is 2.8x the largest row count that one is sized for (2H; Llama-3: 9x), and a context that scores allocates
// no partial-tile workspace beyond what a prefill needs.  R = 0: no chunk fits (or V is not whole 4-row vectors): the call
// goes token by token -- or, with a q6_K classifier, the pass runs the decode classifier once per row (sc_batch), which is also what
// a q6_K classifier does on the f32 matrix instruction (no GEMM there) and in a pass of fewer than SC_Q6K_GEMM_MIN_ROWS rows.
// SC_Q6K_GEMM_MIN_ROWS: the row count from which a pass over q6_K classifier rows takes the GEMM.  One memory-bound launch per row
// against a GEMM whose weight arithmetic does not shrink with the rows: profiles/q6k_gemm.txt has the table behind the number.
#ifndef LLMK_Q6K_GEMM_MIN_ROWS
#define LLMK_Q6K_GEMM_MIN_ROWS 3
#endif
constexpr int SC_Q6K_GEMM_MIN_ROWS = LLMK_Q6K_GEMM_MIN_ROWS;
// rows: the rows of the pass (a q6_K classifier's answer depends on them; the chunks do not)
ScPlan sc_plan(const llmk_ctx* c, int rows = PF_TMAX) {
    const int V = c->V, wt = c->t[LLMK_WCLS].type;
    ScPlan sp{0, 0, (V + PF_SC_ROWS - 1) / PF_SC_ROWS};
    if (wt == LLMK_TYPE_Q6_K && (!c->pf_hm || rows < SC_Q6K_GEMM_MIN_ROWS)) return sp;      // (one chunk of partials)
    if (V % 4) return sp;
    auto need = [&](int rows) {
        size_t m = 0;
        for (int t : {(int)PF_TMAX, 96}) m = std::max(m, (size_t)pf_max_slots(pf_plan(c, rows, c->E, t, wt)) * PF_TMAX * rows);
        return m;
    };
    for (int nch = 1; nch <= V / 128 + 1; ++nch) {
        int R = ((V + nch - 1) / nch + 127) / 128 * 128;
        if (R >= V) R = V;
        const int n = (V + R - 1) / R, lastr = V - (n - 1) * R;
        if (need(R) <= c->pf_pcap && need(lastr) <= c->pf_pcap) {
            sp.R = R; sp.nchunks = n;
            sp.nparts = (n - 1) * ((R + PF_SC_ROWS - 1) / PF_SC_ROWS) + (lastr + PF_SC_ROWS - 1) / PF_SC_ROWS;
            return sp;
        }
        if (R == V && V <= 128) break;
    }
    return sp;
}
// built aside, as pf_setup builds the prefill's
int sc_setup(llmk_ctx* c) {
    if (c->sc) return LLMK_OK;
    auto sc = std::make_unique<llmk_ctx::Score>();
    // partial slots per position: at most one more than V / PF_SC_ROWS per chunk, and a chunk has at least 128 rows
    const size_t slots = (size_t)(c->V + PF_SC_ROWS - 1) / PF_SC_ROWS + (size_t)c->V / 128 + 2;
    for (int i = 0; i < 2; ++i) {
        HIPCHK(sc->part[i].alloc((size_t)PF_TMAX * slots));
        HIPCHK(sc->tgt[i].alloc((size_t)PF_TMAX));
    }
    HIPCHK(sc->targets.alloc((size_t)c->S));
    HIPCHK(sc->out.alloc((size_t)2 * c->S));
    HIPCHK(sc->h_out.alloc((size_t)2 * c->S));
    if (c->t[LLMK_WCLS].type == LLMK_TYPE_Q6_K)
        for (int i = 0; i < 2; ++i) HIPCHK(sc->z[i].alloc((size_t)PF_TMAX * c->V));
    c->sc = std::move(sc);
    return LLMK_OK;
}
// the merge of a batch's partials: log-probs and ids of positions i0 .. i0+T-1 of the call
hipError_t sc_merge(llmk_ctx* c, int lane, hipStream_t st, const ScoreJob& sj, int nparts, int T, int i0) {
    hipLaunchKernelGGL(pf_score_merge_kernel, dim3(T), dim3(64), 0, st, c->sc->part[lane], nparts, sj.want_lp ? c->sc->targets + i0 : nullptr,
                       c->sc->tgt[lane], (sj.out ? sj.out : c->sc->out) + i0, reinterpret_cast<int*>((sj.out ? sj.out : c->sc->out) + sj.n) + i0);
    return hipGetLastError();
}
// after the last layer of a batch (w.Xs = x * final gains, w.xn: pf_epi_resid_norm_kernel): positions i0 .. i0+T-1 of the call
hipError_t sc_batch(llmk_ctx* c, const PfLane& w, int lane, PfEpiArgs& e, const ScoreJob& sj, int T, int i0) {
    const DevTensor& ct = c->t[LLMK_WCLS];
    const int V = c->V, E = c->E;
    // (a q6_K classifier: the call's plan is that of a whole batch; a batch below the crossover -- the last one of a call -- has its own)
    const ScPlan sp = ct.type == LLMK_TYPE_Q6_K && sj.sp.R > 0 && T < SC_Q6K_GEMM_MIN_ROWS ? sc_plan(c, T) : sj.sp;
    float* const logits = sj.logits ? sj.logits : c->sc->logits;
    PfScoreArgs s;
    memset(&s, 0, sizeof(s));
    s.zp = (size_t)V; s.V = V; s.nparts = sp.nparts; s.part = c->sc->part[lane];
    s.targets = sj.want_lp ? c->sc->targets + i0 : nullptr; s.tgt = c->sc->tgt[lane];
    if (ct.type == LLMK_TYPE_Q6_K && sp.R == 0) {
        // q6_K rows without the GEMM (sc_plan): the decode classifier (final rmsnorm inside, q6k.h) on each of the batch's rows
        float* Z = sj.want_logits ? logits + (size_t)i0 * V : c->sc->z[lane];
        const size_t smem = 16 + (size_t)E * sizeof(float);
        const int blocks = (V + GEMV_WAVES * Q6K_RPW - 1) / (GEMV_WAVES * Q6K_RPW);
        for (int t = 0; t < T; ++t) {
            const GemvArgs a = base_args(c, LLMK_WCLS, 0, w.X + (size_t)t * E, (const float*)c->t[LLMK_RMS_FINAL_WEIGHT].data, Z + (size_t)t * V);
            hipLaunchKernelGGL((gemv_q6k_kernel<true>), dim3(blocks), dim3(GEMV_THREADS), smem, w.stream, a);
        }
        HIPRET(hipGetLastError());
        s.Z = Z;
        hipLaunchKernelGGL((pf_score_kernel<false>), dim3(sp.nparts, T), dim3(256), 0, w.stream, e, s);
        HIPRET(hipGetLastError());
        return sc_merge(c, lane, w.stream, sj, sp.nparts, T, i0);
    }
    for (int k = 0; k < sp.nchunks; ++k) {
        const int r0 = k * sp.R, rows = std::min(sp.R, V - r0);
#ifdef LLMK_PF_TRACE
        if (getenv("LLMK_PF_SHOW_PLAN")) {          // debug build: the plan each classifier chunk is launched with (tests/test_q6k_gemm_gpu.py quotes it)
            const PfPlan p = pf_plan(c, rows, E, T, ct.type);
            fprintf(stderr, "llmk: classifier chunk %d of %d: T %d rows %d nr %d U %d nk %d grid %d\n", k + 1, sp.nchunks, T, rows, p.nr, p.U, p.nk, p.grid);
        }
#endif
        HIPRET(pf_gemm(c, w, (const char*)ct.data + (size_t)r0 * ct.row_bytes, (int)ct.row_bytes, w.Xs, rows, E, T, &e, ct.type));
        e.rows = rows; e.out = nullptr;
        s.r0 = r0; s.part0 = k * ((sp.R + PF_SC_ROWS - 1) / PF_SC_ROWS);
        s.zout = sj.want_logits ? logits + (size_t)i0 * V + r0 : nullptr;
        hipLaunchKernelGGL((pf_score_kernel<true>), dim3((rows + PF_SC_ROWS - 1) / PF_SC_ROWS, T), dim3(256), 0, w.stream, e, s);
        HIPRET(hipGetLastError());
    }
    return sc_merge(c, lane, w.stream, sj, sp.nparts, T, i0);
}

// The layers of one pass, shared by the prefill (pf_batch) and the batched decode (bd_pass): T <= PF_TMAX rows, the ids in `tok` (0-based,
// device memory), through the embedding and every layer on the lane's stream; X ends up in w.X.  What a row's POSITION touches is the
// caller's: qkv_attn(l, e) follows layer l's QKV GEMM (e.rows / e.out are set for its epilogue) and enqueues RoPE, the K/V write and
// the attention into w.XB.  final_gains: the gains the last residual's kernel normalises w.Xs with (null: none).  `e` is left as the
// classifier's epilogue needs it.
template <class QkvAttn>
hipError_t pf_layers(llmk_ctx* c, PfLane& w, const int* tok, int T, int pos0, const float* final_gains, PfEpiArgs& e, QkvAttn&& qkv_attn) {
    const int E = c->E, H = c->H, KV = c->KV, QKV = E + 2 * KV, Tp = (T + 15) / 16 * 16;
    const float* emb = (const float*)c->t[LLMK_TOKEN_EMBEDDING_TABLE].data;
    hipLaunchKernelGGL(pf_embed_kernel, dim3((E + 255) / 256, T), dim3(256), 0, w.stream, emb, tok, w.X, E);
    HIPRET(hipGetLastError());
    memset(&e, 0, sizeof(e));
    e.P = w.P; e.xn = w.xn; e.rope = c->d_rope; e.Tp = Tp; e.T = T; e.pos0 = pos0;
    e.E = E; e.KV = KV; e.hs = c->hs; e.H = H;
    for (int l = 0; l < c->L; ++l) {
        // layer l of tensor tid: data plane (and the q4_0 scale plane), rows_per_layer rows
        auto gemm = [&](int tid, int rows_per_layer, const float* X, int K) -> hipError_t {
            const DevTensor& dt = c->t[tid];
            const char* wt = (const char*)dt.data + (size_t)l * rows_per_layer * dt.row_bytes;
            return pf_gemm(c, w, wt, (int)dt.row_bytes, X, rows_per_layer, K, T, &e);
        };
        // rmsnorm (layer 0 here, later layers in the previous residual's kernel) + QKV + RoPE + KV write   llama2.f90:527-565
        if (l == 0) {
            hipLaunchKernelGGL(pf_norm_kernel, dim3(T), dim3(256), 0, w.stream, w.X,
                               (const float*)c->t[LLMK_RMS_ATT_WEIGHT].data, w.Xs, w.xn, E, c->eps);
            HIPRET(hipGetLastError());
        }
        HIPRET(gemm(LLMK_WQKV, QKV, w.Xs, E));
        e.rows = QKV; e.out = w.Q;
        HIPRET(qkv_attn(l, e));                                                         // :572-598
        // x += wo . xb                                                                    :603-605
        HIPRET(gemm(LLMK_WO, E, w.XB, E));
        e.rows = E; e.out = w.X;
        hipLaunchKernelGGL(pf_epi_resid_norm_kernel, dim3(T), dim3(1024), 0, w.stream, e,
                           (const float*)c->t[LLMK_RMS_FFN_WEIGHT].data + (size_t)l * E, w.Xs, w.xn, c->eps);
        HIPRET(hipGetLastError());
        // (rmsnorm above) + w1|w3 + SwiGLU                                                :608-616
        HIPRET(gemm(LLMK_W13, 2 * H, w.Xs, E));
        e.rows = 2 * H; e.out = w.HB;
        hipLaunchKernelGGL(pf_epi_swiglu_kernel, dim3((H / 4 + 255) / 256, T), dim3(256), 0, w.stream, e);
        HIPRET(hipGetLastError());
        // x += w2 . hb                                                                    :618-620
        HIPRET(gemm(LLMK_W2, E, w.HB, H));
        e.rows = E; e.out = w.X;
        hipLaunchKernelGGL(pf_epi_resid_norm_kernel, dim3(T), dim3(1024), 0, w.stream, e,
                           l + 1 < c->L ? (const float*)c->t[LLMK_RMS_ATT_WEIGHT].data + (size_t)(l + 1) * E : final_gains, w.Xs, w.xn, c->eps);
        HIPRET(hipGetLastError());
    }
    return hipSuccess;
}

// one batch of T <= PF_TMAX prompt positions pos0 .. pos0+T-1 (1-based) through all layers; X[T-1] ends up in d_x
// `prev`: the lane of the batch before this one (null for the first batch of a call); `last`: this batch ends the prompt
// `sj` (llmk_score): the final rmsnorm, the classifier and the log-softmax of all T positions follow; i0 = the batch's first position in the call
hipError_t pf_batch(llmk_ctx* c, PfLane& w, const PfLane* prev, const int* tok, int T, int pos0, bool last, const ScoreJob* sj = nullptr, int i0 = 0) {
    const int E = c->E, KV = c->KV, QKV = E + 2 * KV;
    PfEpiArgs e;
    // (scoring: the FINAL rmsnorm of every row)
    HIPRET(pf_layers(c, w, tok, T, pos0, sj ? (const float*)c->t[LLMK_RMS_FINAL_WEIGHT].data : nullptr, e, [&](int l, PfEpiArgs& a) -> hipError_t {
        float* kc = c->d_kc + (size_t)l * c->S * KV;
        float* vc = c->d_vc + (size_t)l * c->S * KV;
        a.kc = kc; a.vc = vc;
        hipLaunchKernelGGL(pf_epi_qkv_kernel, dim3((QKV / 4 + 255) / 256, T), dim3(256), 0, w.stream, a);
        HIPRET(hipGetLastError());
        if (!last) HIPRET(hipEventRecord(w.kv[l], w.stream));             // the next batch's attention reads these rows
        if (prev) HIPRET(hipStreamWaitEvent(w.stream, prev->kv[l], 0));   // ... as this one reads the previous batch's
        // causal attention: position pos0+t sees cache rows 0 .. pos0+t-1
        return with_head_size(c->hs, [&](auto hs) {
            constexpr int HS = decltype(hs)::value;
            hipLaunchKernelGGL((pf_attn_kernel<HS>), dim3(c->nh, (T + 15) / 16), dim3(PF_ATT_WAVES * WAVE), attn_smem(PF_ATT_WAVES, HS), w.stream,
                               w.Q, kc, vc, w.XB, KV, c->kv_mul, pos0, T, E);
            return hipGetLastError();
        });
    }));
    if (sj) HIPRET(sc_batch(c, w, &w == &c->pf->lane[1] ? 1 : 0, e, *sj, T, i0));
    if (last) HIPRET(hipMemcpyAsync(c->d_x, w.X + (size_t)(T - 1) * E, (size_t)E * sizeof(float), hipMemcpyDeviceToDevice, w.stream));
    return hipEventRecord(w.done, w.stream);
}

// Can this context's shape take the batched pass at all?  Single GPU, shapes on the GEMMs' 64-column step
bool pf_shape_ok(const llmk_ctx* c) {
    const int pf_step = PF_KSTEP;
    return c->tp_size == 1 && !c->comm && c->E % pf_step == 0 && c->H % pf_step == 0 && c->KV % 16 == 0;
}
// May this context take the batched pass (llmk_prefill, llmk_score)?  A shape that can, and not switched off (the batched decode has
// no token-by-token form to be switched to: it asks pf_shape_ok)
bool pf_eligible(const llmk_ctx* c) {
    return pf_shape_ok(c) && !(getenv("LLMK_PREFILL") && getenv("LLMK_PREFILL")[0] == '0');
}
// the f16-range flag of the passes enqueued so far, on its way to TkHostWords::pf_flag (ENQUEUED on the ctx stream)
hipError_t pf_fetch_flag(llmk_ctx* c) {
    unsigned* h_flag = &c->host_words()->pf_flag;
    *h_flag = 0;
    return c->pf_hm ? hipMemcpyAsync(h_flag, c->pf->flag, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream) : hipSuccess;
}
// The batched pass of llmk_prefill and (sj: with the classifier and log-softmax of every position) llmk_score, ENQUEUED: tokens[0..n)
// (1-based ids) at positions pos0 .. pos0+n-1 in batches of PF_TMAX that alternate between the two lanes, then the f16-range flag on
// its way to TkHostWords::pf_flag.  The caller adds its own tail to the ctx stream and synchronises that stream once: everything
// lane 1 was given is ordered in front of it.
int pf_run(llmk_ctx* c, const int* tokens, int n, int pos0, const ScoreJob* sj) {
    c->pf_tok0.assign(tokens, tokens + n);
    for (int& t : c->pf_tok0) --t;
    HIPCHK(hipMemcpyAsync(c->pf->tok, c->pf_tok0.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    // these positions are being rewritten by other kernels: whatever an earlier sequence's decode left in the q4_0 persistent kernel's
    // scale records (token_kernel.h tk_qsc; tagged by position only) must not pass for "the position before" of the decode that follows
    HIPCHK(tk_qsc_clear(c, c->stream));
    HIPCHK(hipEventRecord(c->pf->start, c->stream));
    HIPCHK(hipStreamWaitEvent(c->pf->lane[1].stream, c->pf->start, 0));
    int k = 0;
    for (int i = 0; i < n; i += PF_TMAX, ++k) {
        // batch k runs on lane k % 2; its lane's previous batch (k - 2) is ordered by the stream, batch k - 1 by the KV events
        const bool last = i + PF_TMAX >= n;
        const hipError_t pe = pf_batch(c, c->pf->lane[k & 1], k > 0 ? &c->pf->lane[(k - 1) & 1] : nullptr, c->pf->tok + i, std::min(PF_TMAX, n - i), pos0 + i, last, sj, i);
        if (pe != hipSuccess) {   // nothing of this call may still be running (on either lane) when it returns
            hipStreamSynchronize(c->pf->lane[1].stream);
            hipStreamSynchronize(c->stream);
            return LLMK_E_HIP + (int)pe;
        }
    }
    // what follows runs on the ctx stream (= lane 0's): after everything lane 1 was given, too
    if (k >= 2) HIPCHK(hipStreamWaitEvent(c->stream, c->pf->lane[1].done, 0));
    HIPCHK(pf_fetch_flag(c));
    return LLMK_OK;
}
// ---- batched decode (batch.h) -----------------------------------------------------------------------------------
static_assert(LLMK_MAX_BATCH == PF_TMAX, "a batch's rows are the rows of one prefill pass");

// A batch's caches and prefix rows by element type (llmk_cache_create: float, _Float16 or KvQ8, one type per batch), and f(T()) for the
// type a batch has.  What differs between the types on the host: the buffers, the kernels' instantiation, and a converting kernel in
// the place of the device-to-device copy from the context's f32 rows.  A buffer of n ELEMENTS is units(n) units of its DevBuf; view(buf,
// n) is what the kernels take for it -- the pointer, or for q8_0 the quants and the scales behind them (attn_tiles.h Q8Rows; nothing is
// padded: n is a multiple of 32, so the scales start 32-byte aligned) -- and attn_at(view, e) moves it on by e elements.
template <class T> struct BdKvPlain {
    static size_t units(size_t n) { return n; }
    static T* view(DevBuf<T>& buf, size_t) { return buf.get(); }
};
template <class T> struct BdKv;
template <> struct BdKv<KvQ8> {
    static DevBuf<int8_t>& kc(llmk_batch* b) { return b->d_kc8; }
    static DevBuf<int8_t>& vc(llmk_batch* b) { return b->d_vc8; }
    static DevBuf<int8_t>& pk(llmk_batch::Prefix& p) { return p.d_pk8; }
    static DevBuf<int8_t>& pv(llmk_batch::Prefix& p) { return p.d_pv8; }
    static size_t units(size_t n) { return n + n / 32 * sizeof(_Float16); }      // bytes: 34 per 32 elements
    static Q8Rows view(DevBuf<int8_t>& buf, size_t n) { return Q8Rows{buf.get(), reinterpret_cast<_Float16*>(buf.get() + n)}; }
};
template <> struct BdKv<float> : BdKvPlain<float> {
    static DevBuf<float>& kc(llmk_batch* b) { return b->d_kc; }
    static DevBuf<float>& vc(llmk_batch* b) { return b->d_vc; }
    static DevBuf<float>& pk(llmk_batch::Prefix& p) { return p.d_pk; }
    static DevBuf<float>& pv(llmk_batch::Prefix& p) { return p.d_pv; }
};
template <> struct BdKv<_Float16> : BdKvPlain<_Float16> {
    static DevBuf<_Float16>& kc(llmk_batch* b) { return b->d_kc16; }
    static DevBuf<_Float16>& vc(llmk_batch* b) { return b->d_vc16; }
    static DevBuf<_Float16>& pk(llmk_batch::Prefix& p) { return p.d_pk16; }
    static DevBuf<_Float16>& pv(llmk_batch::Prefix& p) { return p.d_pv16; }
};
template <class F>
static auto with_kv_type(const llmk_batch* b, F f) {
    return b->kv_type == LLMK_TYPE_Q8_0 ? f(KvQ8()) : b->kv_type == LLMK_TYPE_F16 ? f(_Float16()) : f(float());
}
// rows [n][KV] of every layer of the context's f32 caches into a batch's K and V buffers (dk, dv; layers dst_layer elements apart),
// ENQUEUED: the copy an f32 batch always made, the converting kernel for an f16 one (batch.h bd_to_half_kernel) or a q8_0 one (bd_to_q8_kernel)
static hipError_t bd_copy_ctx_rows(llmk_ctx* c, float* dk, float* dv, size_t n, size_t dst_layer) {
    float* caches[2][2] = {{dk, c->d_kc}, {dv, c->d_vc}};
    for (auto& p : caches)
        for (int l = 0; l < c->L; ++l)
            HIPRET(hipMemcpyAsync(p[0] + (size_t)l * dst_layer, p[1] + (size_t)l * c->S * c->KV, n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    return hipSuccess;
}
static hipError_t bd_copy_ctx_rows(llmk_ctx* c, _Float16* dk, _Float16* dv, size_t n, size_t dst_layer) {
    const unsigned blocks = (unsigned)std::min<size_t>((n / 4 + 255) / 256, 1024);
    hipLaunchKernelGGL(bd_to_half_kernel, dim3(blocks, c->L, 2), dim3(256), 0, c->stream, c->d_kc.get(), c->d_vc.get(), dk, dv, n, (size_t)c->S * c->KV, dst_layer);
    return hipGetLastError();
}

static hipError_t bd_copy_ctx_rows(llmk_ctx* c, Q8Rows dk, Q8Rows dv, size_t n, size_t dst_layer) {
    const unsigned blocks = (unsigned)std::min<size_t>((n / 4 + 255) / 256, 1024);
    hipLaunchKernelGGL(bd_to_q8_kernel, dim3(blocks, c->L, 2), dim3(256), 0, c->stream, c->d_kc.get(), c->d_vc.get(), dk, dv, n, (size_t)c->S * c->KV, dst_layer);
    return hipGetLastError();
}

// One pass, ENQUEUED on the context's stream: the n rows in d_rows / d_tok through every layer, the classifier and the per-row first
// maximum (into d_out + n); the logits of every row into d_logits when asked for.  max_pos: the longest row (the attention's split rule).
// With attached rows among them (pass_att > 0, llmk_prefix_*) the attention is the three kernels of batch.h's prefix section; `step`:
// the rows stand `step` positions behind the uploaded ones (a decode's later passes).
template <class TC>      // TC: the caches' element type
static hipError_t bd_pass_of(llmk_batch* b, int n, int max_pos, bool want_logits, const ScPlan& sp, int step) {
    llmk_ctx* c = b->ctx;
    PfLane& w = c->pf->lane[0];
    const int E = c->E, KV = c->KV, QKV = E + 2 * KV, T = n;
    const BdCaches bc{b->d_rows, (size_t)b->seq_len * KV, b->n_slots, b->seq_len};
    int parts = bd_parts(n, c->nkv, max_pos, c->n_cu), tpp = bd_tiles_per_part(max_pos, parts);
    const bool shared = b->pass_att > 0;
    int groups = 0, pparts = 0, ptpp = 0;
    if (shared) {
        // the own parts' split rule is bd_parts on the longest OWN range, counted in whole tiles from the one that holds row `first`
        int own = 0;
        for (int i = 0; i < n; ++i) {
            const int pos = b->h_rows[i].pos + step;
            own = std::max(own, (pos + BD_TILE - 1) / BD_TILE - b->px->h_first[b->h_rows[i].slot] / BD_TILE);
        }
        parts = bd_parts(n, c->nkv, own * BD_TILE, c->n_cu);
        tpp = bd_tiles_per_part(own * BD_TILE, parts);
        groups = bd_prefix_groups(b->pass_att, c->kv_mul);
        pparts = bd_prefix_parts(b->pass_att, c->nkv, c->kv_mul, b->P, c->n_cu);
        ptpp = bd_tiles_per_part(b->P, pparts);
    }
    const int ngroups = b->pass_groups;
    if (ngroups > 0) {
        // a span pass (llmk_span_*): the split rule counts column groups, the longest group's tiles from the one that holds row `first`
        int own = 0;
        for (int k = 0; k < ngroups; ++k) {
            const BdRow& r = b->h_rows[b->sn->h_groups[k].first + b->sn->h_groups[k].rows - 1];
            own = std::max(own, (r.pos + step + BD_TILE - 1) / BD_TILE - (shared ? b->px->h_first[r.slot] : 0) / BD_TILE);
        }
        parts = bd_span_parts(ngroups, c->nkv, own, c->n_cu);
        tpp = bd_tiles_per_part(own * BD_TILE, parts);
    }
    PfEpiArgs e;
    // (every pass ends in the classifier: the FINAL rmsnorm of every row; pos0 = 0: a row's position is in its row words)
    HIPRET(pf_layers(c, w, b->d_tok, T, 0, (const float*)c->t[LLMK_RMS_FINAL_WEIGHT].data, e, [&](int l, PfEpiArgs& a) -> hipError_t {
        const size_t cache = (size_t)c->L * b->n_slots * bc.slot_stride;
        const auto kc = attn_at(BdKv<TC>::view(BdKv<TC>::kc(b), cache), (size_t)l * b->n_slots * bc.slot_stride);
        const auto vc = attn_at(BdKv<TC>::view(BdKv<TC>::vc(b), cache), (size_t)l * b->n_slots * bc.slot_stride);
        if constexpr (std::is_same_v<TC, float>) {
            a.kc = kc; a.vc = vc;
            hipLaunchKernelGGL(bd_epi_qkv_kernel, dim3((QKV / 4 + 255) / 256, T), dim3(256), 0, w.stream, a, bc);
        } else if constexpr (std::is_same_v<TC, KvQ8>) {
            a.kc = a.vc = nullptr;
            hipLaunchKernelGGL(bd_epi_qkv_q8_kernel, dim3((QKV / 4 + 255) / 256, T), dim3(256), 0, w.stream, a, bc, kc, vc);
        } else {
            a.kc = a.vc = nullptr;      // (the context's caches are not this pass's)
            hipLaunchKernelGGL(bd_epi_qkv_h_kernel, dim3((QKV / 4 + 255) / 256, T), dim3(256), 0, w.stream, a, bc, kc, vc);
        }
        HIPRET(hipGetLastError());
        // (the prefix rows of this layer: [L][P][KV] with the layers P rows apart, whatever the blocks' room)
        auto pk = kc, pv = vc;
        if (shared) {
            pk = attn_at(BdKv<TC>::view(BdKv<TC>::pk(*b->px), (size_t)c->L * b->P * KV), (size_t)l * b->P * KV);
            pv = attn_at(BdKv<TC>::view(BdKv<TC>::pv(*b->px), (size_t)c->L * b->P * KV), (size_t)l * b->P * KV);
        }
        return with_head_size(c->hs, [&](auto hs) {
            constexpr int HS = decltype(hs)::value;
            if (ngroups > 0) {
                // prefix (a pass with attached rows) + the groups' own rows + fold; one part and no attached row: straight to XB
                const int np = pparts + parts, direct = !shared && parts == 1;
                if (shared) {
                    hipLaunchKernelGGL((BdAttn<HS, TC>::prefix), dim3(c->nkv, groups, pparts), dim3(BD_WAVES * WAVE), attn_smem(BD_WAVES, HS), w.stream,
                                       w.Q, pk, pv, b->sn->d_spo, b->sn->d_spml, b->px->d_colmap, T, b->P, KV, c->kv_mul, E, ptpp, np);
                    HIPRET(hipGetLastError());
                }
                const int* first = shared ? b->px->d_first.get() : nullptr;
                hipLaunchKernelGGL((BdAttn<HS, TC>::span), dim3(c->nkv, ngroups, parts), dim3(BD_WAVES * WAVE), attn_smem(BD_WAVES, HS), w.stream,
                                   w.Q, kc, vc, w.XB, b->sn->d_spo, b->sn->d_spml, bc, b->sn->d_groups, first, T, KV, c->kv_mul, E, tpp, np, pparts, direct);
                HIPRET(hipGetLastError());
                if (!direct) hipLaunchKernelGGL((bd_attn_fold_kernel<HS>), dim3(c->nkv, T), dim3(256), 0, w.stream, b->sn->d_spo, b->sn->d_spml, w.XB, bc, first,
                                                c->kv_mul, E, c->kv_mul, np, pparts);
                return hipGetLastError();
            }
            if (shared) {
                const int np = pparts + parts;
                hipLaunchKernelGGL((BdAttn<HS, TC>::prefix), dim3(c->nkv, groups, pparts), dim3(BD_WAVES * WAVE), attn_smem(BD_WAVES, HS), w.stream,
                                   w.Q, pk, pv, b->px->d_xpo, b->px->d_xpml, b->px->d_colmap, T, b->P, KV, c->kv_mul, E, ptpp, np);
                HIPRET(hipGetLastError());
                hipLaunchKernelGGL((BdAttn<HS, TC>::own), dim3(c->nkv, T, parts), dim3(BD_WAVES * WAVE), attn_smem(BD_WAVES, HS), w.stream,
                                   w.Q, kc, vc, b->px->d_xpo, b->px->d_xpml, bc, b->px->d_first, KV, c->kv_mul, E, tpp, np, pparts);
                HIPRET(hipGetLastError());
                hipLaunchKernelGGL((bd_attn_fold_kernel<HS>), dim3(c->nkv, T), dim3(256), 0, w.stream, b->px->d_xpo, b->px->d_xpml, w.XB, bc, b->px->d_first,
                                   c->kv_mul, E, c->kv_mul, np, pparts);
                return hipGetLastError();
            }
            hipLaunchKernelGGL((BdAttn<HS, TC>::row), dim3(c->nkv, T, parts), dim3(BD_WAVES * WAVE), attn_smem(BD_WAVES, HS), w.stream,
                               w.Q, kc, vc, w.XB, b->d_po, b->d_pml, bc, KV, c->kv_mul, E, tpp);
            HIPRET(hipGetLastError());
            if (parts > 1) hipLaunchKernelGGL((bd_attn_fold_kernel<HS>), dim3(c->nkv, T), dim3(256), 0, w.stream, b->d_po, b->d_pml, w.XB, bc, (const int*)nullptr,
                                           c->kv_mul, E, BD_MAX_GROUP, parts, 0);
            return hipGetLastError();
        });
    }));
    ScoreJob sj{false, want_logits, n, sp};
    sj.out = b->d_out;
    sj.logits = b->d_logits;
    return sc_batch(c, w, 0, e, sj, T, 0);
}
static hipError_t bd_pass(llmk_batch* b, int n, int max_pos, bool want_logits, const ScPlan& sp, int step = 0) {
    return with_kv_type(b, [&](auto t) { return bd_pass_of<decltype(t)>(b, n, max_pos, want_logits, sp, step); });
}

// did the synchronised call's batched pass raise the f16-range flag?
bool pf_flagged(const llmk_ctx* c) { return c->pf_hm && c->host_words()->pf_flag != 0; }

// The f16-range flag of a batched call (prefill.h pf_gemm_h_kernel, pf_low_check) came back raised.
// bit 0: an activation of this prompt does not fit an f16 (|x| >= 65504, or not finite): this context's GEMMs go back to
// the f32 matrix instruction for good.  Bit 1 alone: a position whose whole row is below 2^-7 (the lo piece of the split
// is an f16 subnormal there): THIS call is redone on the f32 instruction, the next one tries the f16 one again (advisor,
// round 4: a BOS or early-layer row with genuinely small values must not cost the context the fast path).
// Either way the call is redone (again(): the K/V rows it wrote are rewritten) and the first event says so once.
template <class F>
int pf_redo(llmk_ctx* c, const char* who, bool* told, F again) {
    const bool for_good = (c->host_words()->pf_flag & 1u) != 0;
    if (!*told) {
        *told = true;
        fprintf(stderr, "llmk: %s met %s; %s\n", who, for_good ? "an activation beyond the f16 range" : "a position whose activations are all below 2^-7",
                for_good ? "this context's prompt GEMMs run on the f32 matrix instruction from now on" : "this call is redone on the f32 matrix instruction");
    }
    HIPCHK(hipMemsetAsync(c->pf->flag, 0, sizeof(unsigned), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->pf.reset();
    c->pf_hm = false;
    int rc = pf_setup(c);
    if (rc) return rc;
    rc = again();
    if (!for_good) c->pf.reset();          // (the next call sets the f16 instruction up again)
    return rc;
}

}  // namespace

extern "C" {

int llmk_version(void) { return 409; }

const char* llmk_strerror(int code) {
    switch (code) {
        case LLMK_OK: return "ok";
        case LLMK_E_ARG: return "llmk: bad argument";
        case LLMK_E_SHAPE: return "llmk: unsupported model shape";
        case LLMK_E_SIZE: return "llmk: byte count does not match tensor size";
        case LLMK_E_TYPE: return "llmk: unsupported ggml tensor type";
        case LLMK_E_STATE: return "llmk: forward called before all weights were uploaded";
        case LLMK_E_NODEVICE: return "llmk: no usable HIP device (there is no CPU fallback)";
        case LLMK_E_NOMEM: return "llmk: out of memory";
        case LLMK_E_TIMEOUT: return "llmk: device-side exchange timed out (persistent kernel not fully resident?)";
        case LLMK_E_COMM: return "llmk: tensor-parallel communicator missing or RCCL error";
        case LLMK_E_VERIFY: return "llmk: uploaded weights did not arrive intact on the device (three attempts)";
        case LLMK_E_NONFINITE: return "llmk: no finite logit at this position (the greedy or sampled pick has no answer)";
    }
    if (code >= LLMK_E_HIP) return hipGetErrorString((hipError_t)(code - LLMK_E_HIP));
    return "llmk: unknown error";
}

int llmk_create(const llmk_config* cfg, llmk_ctx** out) { return llmk_create_tp(cfg, 0, 1, out); }

int llmk_create_tp(const llmk_config* cfg, int tp_rank, int tp_size, llmk_ctx** out) {
    if (!cfg || !out) return LLMK_E_ARG;
    *out = nullptr;
    if (tp_size < 1 || tp_rank < 0 || tp_rank >= tp_size) return LLMK_E_ARG;
    const int E = cfg->emb_dim, H = cfg->hidden_dim, L = cfg->n_layers, nh = cfg->n_heads, nkv = cfg->n_kv_heads;
    const int V = cfg->vocab_size, S = cfg->seq_len;
    if (E <= 0 || H <= 0 || L <= 0 || nh <= 0 || nkv <= 0 || V <= 0 || S <= 0) return LLMK_E_SHAPE;
    if (E % nh || nh % nkv) return LLMK_E_SHAPE;
    const int hs = E / nh;
    if (hs != 16 && hs != 32 && hs != 64 && hs != 128) return LLMK_E_SHAPE;
    if (E % 32 || H % 32 || (V & 1)) return LLMK_E_SHAPE;  // 16-byte vectors, q4_0 blocks, row pairs
    // tensor parallelism splits by kv head (each rank: nkv/P kv heads + their nh/P query heads), hidden
    // rows and vocab rows; every local extent must keep the alignment rules above
    const int kalign = cfg->weight_type == LLMK_TYPE_Q4_0 ? 32 : cfg->weight_type == LLMK_TYPE_F16 ? 8 : 4;
    if (nkv % tp_size || H % tp_size || V % tp_size || (H / tp_size) % kalign || ((V / tp_size) & 1)) return LLMK_E_SHAPE;
    // the contraction slices of wo (the local heads' columns) and of w2 must start and end on the weight type's
    // column granule (q4_0: a 32-weight block), and the local K/V rows must keep their RoPE pairs
    if (((nh / tp_size) * hs) % kalign || (((nkv / tp_size) * hs) & 1)) return LLMK_E_SHAPE;
    if (cfg->weight_type != LLMK_TYPE_F32 && cfg->weight_type != LLMK_TYPE_F16 && cfg->weight_type != LLMK_TYPE_Q4_0)
        return LLMK_E_TYPE;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return LLMK_E_NODEVICE;
    if (cfg->device < 0 || cfg->device >= ndev) return LLMK_E_NODEVICE;
    HIPCHK(hipSetDevice(cfg->device));

    llmk_ctx* c = new (std::nothrow) llmk_ctx();
    if (!c) return LLMK_E_NOMEM;
    c->cfg = *cfg;
    c->E = E; c->H = H; c->L = L; c->nh = nh; c->nkv = nkv; c->V = V; c->S = S;
    c->hs = hs; c->KV = nkv * hs; c->kv_mul = nh / nkv;
    c->tp_rank = tp_rank; c->tp_size = tp_size;
    c->nhl = nh / tp_size; c->Eq = c->nhl * hs; c->KVl = (nkv / tp_size) * hs; c->Hl = H / tp_size; c->Vl = V / tp_size;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0)
        c->n_cu = prop.multiProcessorCount;

    const int KV = c->KV;
    c->gdesc[LLMK_TOKEN_EMBEDDING_TABLE] = {false, V, E, false};
    c->gdesc[LLMK_RMS_ATT_WEIGHT] = {true, 1, E, false};
    c->gdesc[LLMK_RMS_FFN_WEIGHT] = {true, 1, E, false};
    c->gdesc[LLMK_WQKV] = {true, E + 2 * KV, E, true};
    c->gdesc[LLMK_WO] = {true, E, E, true};
    c->gdesc[LLMK_W13] = {true, 2 * H, E, true};
    c->gdesc[LLMK_W2] = {true, E, H, true};
    c->gdesc[LLMK_RMS_FINAL_WEIGHT] = {false, 1, E, false};
    c->gdesc[LLMK_WCLS] = {false, V, E, true};
    for (int i = 0; i < LLMK_N_TENSORS; ++i) c->desc[i] = c->gdesc[i];
    // what THIS rank keeps: column-parallel qkv / w1|w3 / classifier (rows), row-parallel wo / w2 (input slice)
    c->desc[LLMK_WQKV] = {true, c->Eq + 2 * c->KVl, E, true};
    c->desc[LLMK_WO] = {true, E, c->Eq, true};
    c->desc[LLMK_W13] = {true, 2 * c->Hl, E, true};
    c->desc[LLMK_W2] = {true, E, c->Hl, true};
    c->desc[LLMK_WCLS] = {false, c->Vl, E, true};

    int rc = LLMK_OK;
#define CK(expr)                                                        \
    do {                                                                \
        hipError_t e_ = (expr);                                         \
        if (e_ != hipSuccess && rc == LLMK_OK) rc = LLMK_E_HIP + (int)e_; \
    } while (0)
    for (int i = 0; i < LLMK_N_TENSORS && rc == LLMK_OK; ++i) {
        const TensorDesc& d = c->desc[i];
        DevTensor& t = c->t[i];
        t.type = d.matrix ? cfg->weight_type : LLMK_TYPE_F32;
        const size_t rows = (size_t)d.rows * (d.layered ? L : 1);
        // TENSOR_SLACK bytes past the last row: the persistent kernel's last tile of a CU's row range may cover a few rows
        // beyond it (token_kernel.h, NT_Q / NG_A), which for the last rows of the last layer lie past the tensor
        // q4_0 device row: K/2 nibble bytes (16-byte vectors, one per 32-weight block), then the K/32 f16 block scales,
        // zero-padded to whole groups of 64 (a wave-wide scale load past a ragged row end must read finite zeros)
        t.row_bytes = dev_row_bytes(t.type, d.K);
        // the three rmsnorm gain tensors share ONE allocation, att [L][E] | ffn [L][E] | final [E]: the persistent kernel
        // addresses them from one pointer (token_kernel.h TokenArgs::rms)
        if (i == LLMK_RMS_FFN_WEIGHT || i == LLMK_RMS_FINAL_WEIGHT) {      // (views: `own` stays empty)
            t.data = (char*)c->t[LLMK_RMS_ATT_WEIGHT].data + (size_t)(i == LLMK_RMS_FFN_WEIGHT ? L : 2 * L) * E * sizeof(float);
            continue;
        }
        const size_t extra = i == LLMK_RMS_ATT_WEIGHT ? ((size_t)L + 1) * E * sizeof(float) : 0;
        CK(t.own.alloc(rows * t.row_bytes + extra + TENSOR_SLACK));
        t.data = t.own;
        if (rc == LLMK_OK) {
            if (t.type == LLMK_TYPE_Q4_0) CK(hipMemset(t.data, 0, rows * t.row_bytes + TENSOR_SLACK));
            else CK(hipMemset((char*)t.data + rows * t.row_bytes + extra, 0, TENSOR_SLACK));
        }
    }
    const size_t kvn = (size_t)L * S * c->KVl;
    CK(c->d_kc.alloc(kvn));
    CK(c->d_vc.alloc(kvn));
    CK(c->d_x.alloc((size_t)E));
    CK(c->d_q.alloc((size_t)E));
    CK(c->d_xb.alloc((size_t)E));
    CK(c->d_hb.alloc((size_t)H));
    CK(c->d_part.alloc((size_t)E));
    // the logits, then the device's scratch words (scratch_layout.h TkDevWords: the sticky error word first)
    static_assert(sizeof(TkDevWords) % sizeof(float) == 0 && sizeof(TkHostWords) % sizeof(float) == 0, "the scratch words are whole floats' worth");
    const size_t logits_bytes = (size_t)V * sizeof(float) + sizeof(TkDevWords);
    CK(c->d_logits.alloc(logits_bytes / sizeof(float)));
    CK(c->d_rope.alloc((size_t)(hs / 2)));
    CK(c->d_tokpos.alloc(4));
    CK(c->d_next.alloc(2));
    CK(c->h_tokpos.alloc(4));
    // the logits, then the host's scratch words (TkHostWords) and the S ids of the pipelined decode
    CK(c->h_logits.alloc_mapped((size_t)V + sizeof(TkHostWords) / sizeof(float) + (size_t)S));
    c->tk_direct = !(getenv("LLMK_TK_DIRECT") && getenv("LLMK_TK_DIRECT")[0] == '0');
    // llmk_forward's second logits buffer (forward_ahead.h); LLMK_FORWARD_AHEAD=0: one launch and one stream sync per call, as before
    c->fa_on = !(getenv("LLMK_FORWARD_AHEAD") && getenv("LLMK_FORWARD_AHEAD")[0] == '0');
    CK(c->fa_second.alloc_mapped((size_t)V));
    c->fa_buf[0] = c->h_logits;
    c->fa_buf_dev[0] = c->h_logits.dev();
    c->fa_buf[1] = c->fa_second;
    c->fa_buf_dev[1] = c->fa_second.dev();
    for (Event& e : c->fa_ev) CK(e.create(hipEventDisableTiming));
    CK(c->h_next.alloc(1));
    CK(c->h_samp.alloc(1));
    CK(c->h_filt.alloc(1));
    CK(c->stream.create(hipStreamNonBlocking));
    for (Event& e : c->ev) CK(e.create());
    // The whole-token persistent kernel serves the shapes it is instantiated for, on a full 256-CU part
    if (rc == LLMK_OK) rc = tk_setup_all(c);
    if (rc == LLMK_OK) {   // raise the dynamic-LDS limits the token pass needs, or reject the shape here (see g_prepare)
        g_prepare = true;
        hipError_t pe = launch_qkv(c, 0);
        if (pe == hipSuccess) pe = launch_attn(c, 0);
        if (pe == hipSuccess) pe = launch_wo(c, 0);
        if (pe == hipSuccess) pe = launch_w13(c, 0);
        if (pe == hipSuccess) pe = launch_w2(c, 0);
        if (pe == hipSuccess) pe = launch_cls(c);
        g_prepare = false;
        if (pe == hipErrorInvalidValue) rc = LLMK_E_SHAPE;   // context or contraction width needs more than 160 KB of LDS
        else CK(pe);
    }
    if (rc == LLMK_OK) {
        CK(hipMemset(c->d_logits, 0, logits_bytes));
        c->h_tokpos[0] = 0; c->h_tokpos[1] = 0; c->h_tokpos[2] = 0; c->h_tokpos[3] = 0;
        CK(hipMemset(c->d_kc, 0, kvn * sizeof(float)));  // s%key_cache(:,:,:) = 0   llama2.f90:317
        CK(hipMemset(c->d_vc, 0, kvn * sizeof(float)));
        CK(hipMemset(c->d_x, 0, (size_t)E * sizeof(float)));
        CK(hipMemset(c->d_q, 0, (size_t)E * sizeof(float)));
        CK(hipMemset(c->d_xb, 0, (size_t)E * sizeof(float)));
        CK(hipMemset(c->d_hb, 0, (size_t)H * sizeof(float)));
        // default RoPE table: freq_j = 1/10000**((2j+1)/hs)   (llama2.f90:544-545)
        float fr[64];
        for (int j = 0; j < hs / 2; ++j) fr[j] = 1.0f / powf(10000.0f, (float)(2 * j + 1) / (float)hs);
        CK(hipMemcpy(c->d_rope, fr, (size_t)(hs / 2) * sizeof(float), hipMemcpyHostToDevice));
        CK(hipDeviceSynchronize());
    }
#undef CK
    if (rc != LLMK_OK) {
        llmk_destroy(c);
        return rc;
    }
    *out = c;
    return LLMK_OK;
}

// ---- every upload is staged through the shim's own pinned memory, and verified ------------------------------------------------
// Round 4, found by checksums: twice in ~40 runs of the 8-rank 70B tests ONE block of ONE rank reached the device with
// other bytes than the host held -- once from a read-only mmap of a /dev/shm file (logits 3.6e-3 off on every rank), once from
// an anonymous numpy temporary, and that time THREE successive hipMemcpy2D calls from the same pointer delivered the same wrong
// bytes (profiles/r04_tp70_upload_damage.txt): the address had just been freed and mapped again by the allocator (one 264 MB
// temporary per layer), and a copy engine that reads pageable memory through a cached registration of the virtual range reads
// the pages that USED to be there.  Weights are copied once and read for the life of the ctx, so the shim no longer lets
// the device read caller memory at all: the CPU copies each chunk into one of two pinned staging buffers (8 MB, allocated with
// the first upload), summing its 16-bit words on the way.  THAT was not it either: the third event came with the staging in
// place, and all three have the same signature -- the device's sum is 7/8 of the host's to four digits, on every retry: an
// eighth of a freshly copied 16.5 MB scratch buffer reads as zeros to the kernel that follows the copy (one of the chip's
// eight XCDs, each with its own L2, seeing the buffer as it was before a copy ENGINE wrote it).  So now no kernel ever reads what
// a copy engine wrote: a kernel moves each chunk out of the (device-mapped) staging buffer into the tensor (q4_0: via a scratch
// the shim keeps, re-packed on the way), and the 64-bit sum of the tensor's rows AS THEY THEN ARE is compared with the host's.
// A mismatch is printed and the block staged again (three attempts, then LLMK_E_VERIFY).  ~0.15 s per GB on one host core;
// LLMK_VERIFY_UPLOAD=0 skips the comparison, never the staging.
constexpr size_t UP_STAGE_BYTES = (size_t)8 << 20;
__global__ void sum16_kernel(const unsigned* __restrict__ w, size_t nbytes, unsigned long long* out) {
    const size_t nwords = nbytes / 4;
    unsigned long long t = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned v = w[i];
        t += (v & 0xffffu) + (v >> 16);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (nbytes & 2)) t += reinterpret_cast<const unsigned short*>(w)[nbytes / 2 - 1];
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, t);
}
// rows [0, nrows) x col_bytes at pitch spitch -> dst (contiguous); returns the 64-bit sum of the 16-bit words copied
static unsigned long long stage_rows(uint8_t* dst, const uint8_t* src, size_t spitch, size_t col_bytes, size_t nrows) {
    unsigned long long t = 0;
    for (size_t r = 0; r < nrows; ++r) {
        const uint16_t* p = reinterpret_cast<const uint16_t*>(src + r * spitch);    // rows of every encoding start 2-byte aligned
        uint16_t* q = reinterpret_cast<uint16_t*>(dst + r * col_bytes);
        unsigned long long a = 0;
        for (size_t i = 0; i < col_bytes / 2; ++i) { const uint16_t v = p[i]; q[i] = v; a += v; }
        t += a;
    }
    return t;
}
// staging buffer (host memory, device-mapped) -> tensor rows: f32 / f16 rows are contiguous on both sides
__global__ void stage_copy_kernel(const unsigned* __restrict__ src, unsigned* __restrict__ dst, size_t nwords) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
static bool verify_uploads() {
    static const bool on = !(getenv("LLMK_VERIFY_UPLOAD") && getenv("LLMK_VERIFY_UPLOAD")[0] == '0');
    return on;
}
// device sum of `nbytes` contiguous bytes (null stream, like the copies before it); 0 + error code on failure
static hipError_t device_sum16(const void* dev, size_t nbytes, unsigned long long* d_acc, unsigned long long* out) {
    hipError_t e = hipMemsetAsync(d_acc, 0, sizeof(*d_acc), 0);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sum16_kernel, dim3(512), dim3(256), 0, 0, (const unsigned*)dev, nbytes, d_acc);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out, d_acc, sizeof(*out), hipMemcpyDeviceToHost);
    return e;
}

// q4_0 + persistent kernel: (re)build the unit layout of the five matrices from their rows; with the upload verification on,
// the 16-bit word sum of every unit image must equal that of the rows it was built from (the padding blocks are zeros)
static int q16_build(llmk_ctx* c) {
    static const int mats[5] = {LLMK_WQKV, LLMK_WO, LLMK_W13, LLMK_W2, LLMK_WCLS};
    for (int i = 0; i < 5; ++i) {
        const int tid = mats[i];
        const TensorDesc& d = c->desc[tid];
        const DevTensor& t = c->t[tid];
        if (tid == LLMK_WCLS && t.type == LLMK_TYPE_Q6_K) continue;      // q6_K classifier rows are dotted as rows (q6k.h)
        if (t.type != LLMK_TYPE_Q4_0 || d.rows % Q16_ROWS) return LLMK_E_SHAPE;
        const size_t rows = (size_t)d.rows * (d.layered ? c->L : 1), bytes = q16_bytes(rows, d.K);
        if (!c->q16[tid]) {
            HIPCHK(c->q16[tid].alloc(bytes + TENSOR_SLACK));
            HIPCHK(hipMemset(c->q16[tid] + bytes, 0, TENSOR_SLACK));
        }
        hipLaunchKernelGGL(q16_units_kernel, dim3((unsigned)(bytes / Q16_UNIT_BYTES)), dim3(64), 0, c->stream, (const char*)t.data, t.row_bytes, d.K,
                           q16_ncs(d.K), c->q16[tid].get());
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    if (verify_uploads()) {
        DevBuf<unsigned long long> d_acc;
        HIPCHK(d_acc.alloc(1));
        int rc = LLMK_OK;
        for (int i = 0; i < 5 && rc == LLMK_OK; ++i) {
            const int tid = mats[i];
            if (!c->q16[tid] || c->t[tid].type != LLMK_TYPE_Q4_0) continue;
            const TensorDesc& d = c->desc[tid];
            const size_t rows = (size_t)d.rows * (d.layered ? c->L : 1);
            unsigned long long a = 0, b = 0;
            hipError_t e = device_sum16(c->t[tid].data, rows * c->t[tid].row_bytes, d_acc, &a);
            if (e == hipSuccess) e = device_sum16(c->q16[tid], q16_bytes(rows, d.K), d_acc, &b);
            if (e != hipSuccess) rc = LLMK_E_HIP + (int)e;
            else if (a != b) {
                fprintf(stderr, "llmk: the unit layout of tensor %d differs from its rows (16-bit word sums 0x%llx / 0x%llx)\n", tid, b, a);
                rc = LLMK_E_VERIFY;
            }
        }
        if (rc) return rc;
    }
    c->q16_dirty = false;
    return LLMK_OK;
}

// Copy `nrows` rows of a HOST tensor (row pitch `spitch` bytes in `type` encoding; for each row only the
// bytes [col_off, col_off + col_bytes) -- a contraction slice for the row-parallel wo / w2) into local rows
// dst_row0.. of layer `layer` of tensor `tid`.  q4_0 is re-packed (nibble plane + scale plane) on the way.
static int upload_block(llmk_ctx* c, int tid, int layer, int dst_row0, int nrows, const uint8_t* src, size_t spitch,
                        size_t col_off, size_t col_bytes) {
    const TensorDesc& d = c->desc[tid];
    DevTensor& t = c->t[tid];
    const size_t first_row = (size_t)layer * d.rows + dst_row0;
    const bool verify = verify_uploads();
    int rc = LLMK_OK;
    if (!c->up) {
        // the staging objects live as long as the ctx; built aside, so the ctx has all of them or none (advisor, round 4: a failure
        // half-way must not leave something missing to be dereferenced)
        auto up = std::make_unique<llmk_ctx::Upload>();
        for (int b = 0; b < 2; ++b) {
            HIPCHK(up->stage[b].alloc_mapped(UP_STAGE_BYTES));
            HIPCHK(up->done[b].create(hipEventDisableTiming));
            HIPCHK(up->tmp[b].alloc(UP_STAGE_BYTES));
        }
        HIPCHK(up->acc.alloc(1));
        c->up = std::move(up);
    }
    unsigned long long* const d_acc = c->up->acc;
    const bool q6 = t.type == LLMK_TYPE_Q6_K;
    const bool q4 = t.type == LLMK_TYPE_Q4_0 || q6;      // re-packed on the way (q6_K: its own kernel, q6k.h)
    // whole 16-bit words on the host side; the non-q4_0 path moves 32-bit words into rows row_bytes apart (advisor, round 4)
    if (col_bytes > UP_STAGE_BYTES || col_bytes % 2 || (!q4 && (col_bytes % 4 || t.row_bytes % 4))) return LLMK_E_ARG;
    if (q6 && (col_off != 0 || col_bytes != row_bytes_for(LLMK_TYPE_Q6_K, d.K))) return LLMK_E_ARG;      // whole rows only (never a contraction slice)
    c->q16_dirty = true;
    const size_t blocks_per_row = col_bytes / 18;                       // (q4_0)
    const size_t rows_per_chunk = UP_STAGE_BYTES / col_bytes;
    char* dst0 = (char*)t.data + first_row * t.row_bytes;              // the block's rows in the tensor (contiguous: row_bytes apart)
    for (int attempt = 1; rc == LLMK_OK; ++attempt) {
        unsigned long long want = 0;
        int b = 0;
        for (size_t r = 0; r < (size_t)nrows && rc == LLMK_OK; r += rows_per_chunk, b ^= 1) {
            const size_t n = (size_t)nrows - r < rows_per_chunk ? (size_t)nrows - r : rows_per_chunk;
            hipError_t e = hipEventSynchronize(c->up->done[b]);             // the kernel that read this buffer's previous chunk has finished
            if (e != hipSuccess) { rc = LLMK_E_HIP + (int)e; break; }
            want += stage_rows((uint8_t*)c->up->stage[b].get(), src + r * spitch + col_off, spitch, col_bytes, n);
            // a KERNEL moves the chunk from the (device-mapped) staging buffer into the tensor -- re-packing q4_0 blocks on the
            // way -- so nothing a copy engine wrote is ever read by a kernel
            if (q4) {   // (wide loads over PCIe into a device scratch first: the re-packing reads 2 bytes at a time)
                hipLaunchKernelGGL(stage_copy_kernel, dim3(1024), dim3(256), 0, 0, (const unsigned*)c->up->stage[b].dev(), (unsigned*)c->up->tmp[b].get(),
                                   (n * col_bytes + 3) / 4);
                if (q6) hipLaunchKernelGGL(q6k_repack_kernel, dim3(1024), dim3(256), 0, 0, (const uint8_t*)c->up->tmp[b].get(), dst0 + r * t.row_bytes,
                                           n * (size_t)(d.K / Q6K_WEIGHTS), d.K / Q6K_WEIGHTS, t.row_bytes);
                else
                hipLaunchKernelGGL(q4_repack_kernel, dim3(1024), dim3(256), 0, 0, (const uint8_t*)c->up->tmp[b].get(), dst0 + r * t.row_bytes,
                                   n * blocks_per_row, (int)blocks_per_row, t.row_bytes);
            }
            else hipLaunchKernelGGL(stage_copy_kernel, dim3(1024), dim3(256), 0, 0, (const unsigned*)c->up->stage[b].dev(), (unsigned*)(dst0 + r * t.row_bytes),
                                    n * col_bytes / 4);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipEventRecord(c->up->done[b], 0);
            if (e != hipSuccess) rc = LLMK_E_HIP + (int)e;
        }
        if (rc != LLMK_OK || !verify) break;
#ifdef LLMK_TK_DEBUG
        {   // test aid of the debug library (tests/test_upload_verify_gpu.py): damage the first block the process uploads on its first
            // LLMK_UPLOAD_INJECT attempts -- what the verification below exists to catch
            static const int inject = getenv("LLMK_UPLOAD_INJECT") ? atoi(getenv("LLMK_UPLOAD_INJECT")) : 0;
            static bool first_block = true;
            if (first_block && attempt <= inject) (void)hipMemsetAsync(dst0, 0xA5, 64, 0);
            if (attempt >= inject) first_block = false;
        }
#endif
        // the tensor's rows as they now are: a q4_0 row's 16-bit words are its blocks' words in another order (8 nibble words and
        // the scale per block, zero padding behind), so the sum of the re-packed image equals the sum of the bytes handed over
        unsigned long long got = 0;
        const hipError_t e = device_sum16(dst0, (size_t)nrows * t.row_bytes, d_acc, &got);
        if (e != hipSuccess) { rc = LLMK_E_HIP + (int)e; break; }
        if (got == want) break;
        fprintf(stderr, "llmk: upload of tensor %d, layer %d, local rows %zu..%zu (%zu bytes) did not arrive intact: 16-bit word sum 0x%llx on the "
                        "device, 0x%llx on the host (attempt %d of 3)%s\n", tid, layer, first_row, first_row + (size_t)nrows - 1, (size_t)nrows * col_bytes,
                got, want, attempt, attempt < 3 ? " -- staging it again" : "");
        if (attempt == 3) rc = LLMK_E_VERIFY;
    }
    if (rc == LLMK_OK) { const hipError_t e = hipDeviceSynchronize(); if (e != hipSuccess) rc = LLMK_E_HIP + (int)e; }
    if (rc) return rc;
    t.rows_uploaded += (size_t)nrows;
    if (t.rows_uploaded >= (size_t)d.rows * (d.layered ? c->L : 1)) t.uploaded = true;
    return LLMK_OK;
}

// Rows [row0, row0 + nrows) of one layer of a full (unsharded) host tensor -> the part of them this rank's shard holds.
// The shard is a few runs of global rows (its query heads / K rows / V rows; its gate / up rows; its vocabulary rows) or,
// for the row-parallel wo / w2, every row but only the input columns of the local heads / hidden slice: each run is
// intersected with the rows handed over, so a loader may stream any row range -- in particular ONLY the rows of its own
// shard (host/gguf_loader.f90 stream_ggml_matrices) -- and whole layers keep working.
static int upload_rows_sharded(llmk_ctx* c, int tid, int layer, int row0, int nrows, const uint8_t* src, int type) {
    const TensorDesc& g = c->gdesc[tid];
    const size_t pitch = row_bytes_for(type, g.K);
    const int r = c->tp_rank, E = c->E, KV = c->KV, H = c->H;
    struct Run { int gfirst, n, lfirst; };            // global first row, count, local first row
    Run runs[3];
    int nruns = 0;
    size_t col_off = 0, col_bytes = pitch;
    switch (tid) {
        case LLMK_WQKV:  // rows: this rank's query heads, then its kv heads' K rows, then their V rows
            runs[nruns++] = {r * c->Eq, c->Eq, 0};
            runs[nruns++] = {E + r * c->KVl, c->KVl, c->Eq};
            runs[nruns++] = {E + KV + r * c->KVl, c->KVl, c->Eq + c->KVl};
            break;
        case LLMK_WO:    // all E rows, the input columns of this rank's heads
            runs[nruns++] = {0, E, 0};
            col_off = row_bytes_for(type, r * c->Eq); col_bytes = row_bytes_for(type, c->Eq);
            break;
        case LLMK_W13:   // gate rows then up rows of this rank's hidden slice
            runs[nruns++] = {r * c->Hl, c->Hl, 0};
            runs[nruns++] = {H + r * c->Hl, c->Hl, c->Hl};
            break;
        case LLMK_W2:    // all E rows, the input columns of this rank's hidden slice
            runs[nruns++] = {0, E, 0};
            col_off = row_bytes_for(type, r * c->Hl); col_bytes = row_bytes_for(type, c->Hl);
            break;
        case LLMK_WCLS:
            runs[nruns++] = {r * c->Vl, c->Vl, 0};
            break;
        default:         // replicated: embedding table and norm gains
            runs[nruns++] = {0, g.rows, 0};
            break;
    }
    for (int i = 0; i < nruns; ++i) {
        const int a = std::max(runs[i].gfirst, row0), b = std::min(runs[i].gfirst + runs[i].n, row0 + nrows);
        if (a >= b) continue;
        const int rc = upload_block(c, tid, layer, runs[i].lfirst + (a - runs[i].gfirst), b - a, src + (size_t)(a - row0) * pitch, pitch,
                                    col_off, col_bytes);
        if (rc) return rc;
    }
    return LLMK_OK;
}

int llmk_upload_rows(llmk_ctx* c, int tid, int layer, int row_offset, int rows, const void* host, size_t nbytes,
                     int ggml_type) {
    if (!c || !host || tid < 0 || tid >= LLMK_N_TENSORS) return LLMK_E_ARG;
    const TensorDesc& g = c->gdesc[tid];
    DevTensor& t = c->t[tid];
    const int nl = g.layered ? c->L : 1;
    if (layer < 0 || layer >= nl || row_offset < 0 || rows <= 0 || row_offset + rows > g.rows) return LLMK_E_ARG;
    if (ggml_type != t.type) return LLMK_E_TYPE;
    if (nbytes != (size_t)rows * row_bytes_for(ggml_type, g.K)) return LLMK_E_SIZE;
    HIPCHK(hipSetDevice(c->cfg.device));
    { const int rc = spec_settle(c); if (rc) return rc; }
    if (c->tp_size > 1) return upload_rows_sharded(c, tid, layer, row_offset, rows, (const uint8_t*)host, ggml_type);
    const size_t pitch = row_bytes_for(ggml_type, g.K);
    return upload_block(c, tid, layer, row_offset, rows, (const uint8_t*)host, pitch, 0, pitch);
}

int llmk_upload(llmk_ctx* c, int tid, const void* host, size_t nbytes, int ggml_type) {
    if (!c || !host || tid < 0 || tid >= LLMK_N_TENSORS) return LLMK_E_ARG;
    const TensorDesc& g = c->gdesc[tid];
    const int nl = g.layered ? c->L : 1;
    if (ggml_type != c->t[tid].type) return LLMK_E_TYPE;
    const size_t per_layer = (size_t)g.rows * row_bytes_for(ggml_type, g.K);
    if (nbytes != per_layer * nl) return LLMK_E_SIZE;
    c->t[tid].rows_uploaded = 0;
    c->t[tid].uploaded = false;
    for (int l = 0; l < nl; ++l) {
        int rc = llmk_upload_rows(c, tid, l, 0, g.rows, (const char*)host + (size_t)l * per_layer, per_layer, ggml_type);
        if (rc) return rc;
    }
    return LLMK_OK;
}

// The classifier's encoding may differ from the other matrices' (stock llama.cpp q4_0 files keep output.weight in
// q6_K; the host loader hands it over dequantised): re-type the tensor BEFORE uploading it.  Such a ctx runs the
// multi-kernel path (the persistent kernel is instantiated for one weight type).
int llmk_set_tensor_type(llmk_ctx* c, int tid, int ggml_type) {
    if (!c || tid != LLMK_WCLS) return LLMK_E_ARG;
    if (ggml_type != LLMK_TYPE_F32 && ggml_type != LLMK_TYPE_F16 && ggml_type != LLMK_TYPE_Q4_0 && ggml_type != LLMK_TYPE_Q6_K) return LLMK_E_TYPE;
    DevTensor& t = c->t[tid];
    if (t.type == ggml_type) return LLMK_OK;
    const TensorDesc& d = c->desc[tid];
    const int kalign = ggml_type == LLMK_TYPE_Q6_K ? Q6K_WEIGHTS : ggml_type == LLMK_TYPE_Q4_0 ? 32 : ggml_type == LLMK_TYPE_F16 ? 8 : 4;
    if (d.K % kalign) return LLMK_E_SHAPE;
    HIPCHK(hipSetDevice(c->cfg.device));
    { const int rc = spec_settle(c); if (rc) return rc; }
    HIPCHK(hipStreamSynchronize(c->stream));
    // the new rows, allocated and zeroed BEFORE the old ones go: a call that fails here leaves the tensor as it was, and no state has
    // a typed, un-uploaded classifier without memory behind it
    const size_t bytes = (size_t)d.rows * (d.layered ? c->L : 1) * dev_row_bytes(ggml_type, d.K) + TENSOR_SLACK;
    DevBuf<char> fresh;
    HIPCHK(fresh.alloc(bytes));
    HIPCHK(hipMemset(fresh, 0, bytes));
    c->pf.reset();      // (the next setup prepares the new type's GEMM kernels: pf_prepare)
    t.own = std::move(fresh);
    t.data = t.own;
    t.type = ggml_type;
    t.uploaded = false;
    t.rows_uploaded = 0;
    t.row_bytes = dev_row_bytes(ggml_type, d.K);
    c->q16[tid].reset();      // the classifier's unit copy, if one was built
    c->q16_dirty = true;
    if (c->use_tk) {
        c->use_tk = false;
        drop_graphs(c);
    }
    // the persistent kernel again, if one is instantiated for this shape with a classifier of this type (round 6: q6_K rows beside
    // q4_0 matrices -- a stock llama.cpp q4_0 file keeps the fast path); otherwise the multi-kernel path
    { const int rc = tk_setup_all(c); if (rc) return rc; }
    g_prepare = true;                      // the classifier GEMV may need a larger dynamic-LDS limit in its new type
    const hipError_t pe = launch_cls(c);
    g_prepare = false;
    if (pe == hipErrorInvalidValue) return LLMK_E_SHAPE;
    HIPCHK(pe);
    return LLMK_OK;
}

// rmsnorm epsilon.  The reference hard-codes 1e-5 (llama2.f90:454) and ignores the file's
// llama.attention.layer_norm_rms_epsilon; a host that opts into the file's value (llm --gguf-eps) sets it here.
int llmk_set_rms_eps(llmk_ctx* c, float eps) {
    if (!c || !(eps > 0.f) || !(eps < 1.f)) return LLMK_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    { const int rc = spec_settle(c); if (rc) return rc; }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->eps = eps;
    drop_graphs(c);   // kernel arguments are baked in
    return LLMK_OK;
}

int llmk_set_rope_freqs(llmk_ctx* c, const float* freqs, int n) {
    if (!c || !freqs || n != c->hs / 2) return LLMK_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    { const int rc = spec_settle(c); if (rc) return rc; }
    HIPCHK(hipMemcpy(c->d_rope, freqs, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    return LLMK_OK;
}

// ---- llmk_forward with the next greedy position in flight (forward_ahead.h has the policy, DESIGN.md section 3b the figures) ----
// Only the direct-mode persistent kernel of a whole-model f32 / f16 context: a q4_0 shape's range-event redo, the timed and the
// graph-less passes and the tensor-parallel ranks keep the one-launch-one-sync pass; so does the debug library's injected timeout.
static bool fa_eligible(const llmk_ctx* c) {
    if (!c->fa_on || !c->use_tk || !c->tk_direct || c->tp_size != 1 || c->comm || c->p2p) return false;
    if ((c->cfg.flags & (LLMK_FLAG_TIMINGS | LLMK_FLAG_NO_GRAPH)) || tk_table[c->tk_shape - 1].q4) return false;
    return !(TK_DEBUG && getenv("LLMK_TK_INJECT_TIMEOUT"));
}
// Position pos in the greedy instantiation, logits straight into pinned buffer pos & 1, candidates into cand[pos & 1].
// spec: the token is the fold of position pos - 1's candidates (the launch before this one on the stream), and workgroup 0
// publishes it, 1-based, in ids()[pos - 2] as it starts.  An event behind every launch: see fa_deliver.
static int fa_launch(llmk_ctx* c, int token, int pos, bool spec) {
    if (!spec) c->h_tokpos[0] = token - 1;
    c->h_tokpos[1] = pos;
    c->h_tokpos[2] += 1;
    TkGreedy g;
    g.gflags = TKG_GREEDY | (spec ? TKG_CAND_IN | TKG_ID : 0);
    g.id_index = pos - 2;
    g.logits = c->fa_buf_dev[pos & 1];
    if (spec) {
        c->host_words()->ids()[pos - 2] = 0;
        c->fa_inflight = true;
    }
    c->tk_short_grid = false;
    HIPCHK(launch_token_kernel(c, true, g));
    HIPCHK(hipEventRecord(c->fa_ev[pos & 1], c->stream));
    return LLMK_OK;
}
// The id (1-based) that a launch on the stream publishes in ids()[slot] as it starts: the one it took for the position before its own.
// 0: the stream drained without one (the sticky word was raised)
static int tk_published_id(llmk_ctx* c, int slot, int* id) {
    volatile int* ids = c->host_words()->ids();
    while ((*id = ids[slot]) == 0) {
        const hipError_t q = hipStreamQuery(c->stream);
        if (q == hipSuccess) { *id = ids[slot]; break; }
        if (q != hipErrorNotReady) return LLMK_E_HIP + (int)q;
    }
    return LLMK_OK;
}
// Wait for position pos, whose launch is on the stream, and hand its logits over.
// Completion, with a launch for pos + 1 behind it (`more`): the event recorded between the two.  hipEventSynchronize on an event
// without hipEventReleaseToDevice returns when the work in front of the event has completed AND its writes to host memory are
// visible to this thread -- the same guarantee hipStreamSynchronize gives the direct-mode pass, for position pos alone.  (The other
// candidate, polling the id the launch for pos + 1 publishes as it starts, costs no barrier packet but orders pos's plain stores to
// pinned memory by nothing HIP documents: a relaxed system-scope store from another kernel.)  Without a launch behind: the stream.
static int fa_deliver(llmk_ctx* c, int token, int pos, bool more, float* logits_out) {
    HIPCHK(more ? hipEventSynchronize(c->fa_ev[pos & 1]) : hipStreamSynchronize(c->stream));
    if (!more) c->fa_inflight = false;
    const TkVerdict v = TkRecovery::settled(c->host_words()->err);
    if (v != TkVerdict::CLEAN) {
        // NO_FINITE is the launch BEHIND this one finding no finite candidate (this position's logits hold none; they are delivered as
        // they are); anything else is this launch's timed-out exchange: the position is redone on the multi-kernel path
        c->fa_inflight = true;      // (whatever is on the stream: spec_settle drains it and reads the device's word)
        const int rc = spec_settle(c);
        if (rc) return rc;
        if (v != TkVerdict::NO_FINITE) {
            const int rc2 = token_pass(c, token, pos, TAIL_LOGITS);
            if (rc2) return rc2;
            memcpy(logits_out, c->h_logits, (size_t)c->V * sizeof(float));
            return LLMK_OK;
        }
    }
    c->tk.clean();
    memcpy(logits_out, c->fa_buf[pos & 1], (size_t)c->V * sizeof(float));
    if (v == TkVerdict::CLEAN) {
        c->fa_logits = c->fa_buf[pos & 1];
        c->fa.ran(pos);
    }
    c->fa_tok0 = token - 1;
    c->fa_pos = pos;
    return LLMK_OK;
}

int llmk_forward(llmk_ctx* c, int token, int pos, float* logits_out) {
    if (!c || !logits_out) return LLMK_E_ARG;
    if (!fa_eligible(c)) {
        int rc = run_token(c, token, pos, TAIL_LOGITS);
        if (rc) return rc;
        memcpy(logits_out, c->h_logits, (size_t)c->V * sizeof(float));
        return LLMK_OK;
    }
    int rc = tensors_ready(c);
    if (rc == LLMK_OK && (token < 1 || token > c->V || pos < 1 || pos > c->S)) rc = LLMK_E_ARG;
    if (rc == LLMK_OK && hipSetDevice(c->cfg.device) != hipSuccess) rc = LLMK_E_HIP;
    if (rc) { spec_settle(c); return rc; }
    ForwardAhead& fa = c->fa;
    if (fa.armed) {
        int id = 0;
        if (fa.expects(pos) && (rc = tk_published_id(c, pos - 2, &id)) != LLMK_OK) { spec_settle(c); return rc; }
        if (id == token) {      // (ids are 1-based: never 0)
            const bool more = fa.hit(c->S);
            if (more && (rc = fa_launch(c, 0, pos + 1, true)) != LLMK_OK) { spec_settle(c); return rc; }
            if ((rc = fa_deliver(c, token, pos, more, logits_out)) != LLMK_OK) spec_settle(c);
            return rc;
        }
        fa.miss();      // drain, then the call as it would have run with nothing in flight; it rewrites KV row pos
        if ((rc = spec_settle(c)) != LLMK_OK) return rc;      // (the backoff that miss() started outlives the settling)
    } else if (fa.scan_due(pos) && fa.scanned(fa_first_max(c->fa_logits, c->V) + 1 == token, pos, c->S)) {
        // the arming call: the greedy instantiation scores its candidates with the device's sampling words, which must hold zeros
        // (invT == 0) as in decode_run
        TkDevWords* dw = c->dev_words();
        hipError_t e = c->samp_dev.push(llmk_sample_params{}, [&] { return hipMemsetAsync(&dw->samp, 0, sizeof(llmk_sample_params), c->stream); });
        if (e != hipSuccess) { spec_settle(c); return LLMK_E_HIP + (int)e; }
        c->host_words()->err = 0;
        if ((rc = fa_launch(c, token, pos, false)) == LLMK_OK) rc = fa_launch(c, 0, pos + 1, true);
        if (rc == LLMK_OK) rc = fa_deliver(c, token, pos, true, logits_out);
        if (rc) spec_settle(c);
        return rc;
    }
    rc = token_pass(c, token, pos, TAIL_LOGITS);
    if (rc) { fa.interrupt(); return rc; }
    memcpy(logits_out, c->h_logits, (size_t)c->V * sizeof(float));
    c->fa_logits = c->h_logits;
    c->fa_tok0 = token - 1;
    c->fa_pos = pos;
    if (fa_eligible(c)) fa.ran(pos);      // (the pass may have retired the kernel)
    return LLMK_OK;
}

int llmk_forward_ahead_stats(llmk_ctx* c, int out[4]) {
    if (!c || !out) return LLMK_E_ARG;
    out[0] = c->fa.launches;
    out[1] = c->fa.hits;
    out[2] = c->fa.misses;
    out[3] = c->fa.armed ? 1 : 0;
    return LLMK_OK;
}

// The prompt loop of llama2.f90:376-402 as ONE call: tokens[0..n) (1-based ids) sit at positions pos0 .. pos0+n-1,
// the KV cache rows of those positions are written, and logits_out receives the logits of the LAST position --
// exactly what n llmk_forward calls leave behind.  f32 single-GPU contexts run the batched MFMA path (prefill.h);
// every other configuration falls back to the token-by-token pass.
int llmk_prefill(llmk_ctx* c, const int* tokens, int n, int pos0, float* logits_out) {
    if (!c || !tokens || !logits_out || n < 1 || pos0 < 1 || pos0 + n - 1 > c->S) return LLMK_E_ARG;
    int rc = check_ready(c);
    if (rc) return rc;
    for (int i = 0; i < n; ++i)
        if (tokens[i] < 1 || tokens[i] > c->V) return LLMK_E_ARG;
    if (!pf_eligible(c)) {
        for (int i = 0; i < n; ++i) {
            rc = run_token(c, tokens[i], pos0 + i, TAIL_LOGITS);
            if (rc) return rc;
        }
        memcpy(logits_out, c->h_logits, (size_t)c->V * sizeof(float));
        return LLMK_OK;
    }
    HIPCHK(hipSetDevice(c->cfg.device));
    rc = pf_setup(c, true);
    if (rc) return rc;
    rc = pf_run(c, tokens, n, pos0, nullptr);
    if (rc) return rc;
    HIPCHK(launch_cls(c));                          // final rmsnorm + classifier of the last position   :627-636
    HIPCHK(hipMemcpyAsync(c->h_logits, c->d_logits, (size_t)c->V * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (pf_flagged(c)) {
        static bool told = false;           // (each entry point reports its own first event)
        return pf_redo(c, "llmk_prefill", &told, [&] { return llmk_prefill(c, tokens, n, pos0, logits_out); });
    }
    memcpy(logits_out, c->h_logits, (size_t)c->V * sizeof(float));
    return LLMK_OK;
}

// llmk_prefill's pass with the classifier and a log-softmax for EVERY position: per position the
// log-probability of a given target, the first maximum's id and, when asked for, the logits.  Same argument checks, same KV rows,
// decode may continue behind it.
int llmk_score(llmk_ctx* c, const int* tokens, int n, int pos0, const int* targets, float* logprob_out, int* argmax_out, float* logits_out) {
    if (!c || !tokens || n < 1 || pos0 < 1 || pos0 + n - 1 > c->S) return LLMK_E_ARG;
    if ((!logprob_out && !argmax_out && !logits_out) || (logprob_out && !targets)) return LLMK_E_ARG;
    int rc = check_ready(c);
    if (rc) return rc;
    for (int i = 0; i < n; ++i)
        if (tokens[i] < 1 || tokens[i] > c->V || (targets && (targets[i] < 0 || targets[i] > c->V))) return LLMK_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    rc = sc_setup(c);
    if (rc) return rc;
    const int V = c->V;
    ScoreJob sj{logprob_out != nullptr, logits_out != nullptr, n, ScPlan{0, 0, 0}};
    bool batched = pf_eligible(c);
    if (batched) {
        rc = pf_setup(c, true);
        if (rc) return rc;
        const int ct = c->t[LLMK_WCLS].type;      // (the classifier's own GEMM kernels were prepared with the workspaces: pf_prepare)
        sj.sp = sc_plan(c, std::min(n, (int)PF_TMAX));      // (R = 0 with a q6_K classifier: the decode classifier per row, not token by token)
        if (ct != LLMK_TYPE_Q6_K && sj.sp.R == 0) {
            batched = false;
            static bool told_slow = false;          // (a call some 30x slower than its neighbours must not be silent)
            if (!told_slow) {
                told_slow = true;
                fprintf(stderr, "llmk: llmk_score runs token by token on this context: %s\n",
                        V % 4 ? "vocab_size is not a multiple of 4 (the classifier GEMM's partial tiles are read as 4-row vectors)"
                              : "no 128-row chunk of the classifier fits the prefill's partial-tile workspace");
            }
        }
    }
    if (batched && sj.want_logits) HIPCHK(c->sc->logits.reserve((size_t)n * V, c->stream));
    std::vector<int> tg0;
    if (sj.want_lp) {
        tg0.assign(targets, targets + n);
        for (int& t : tg0) --t;                                  // 0-based; -1 = no target here
        HIPCHK(hipMemcpyAsync(c->sc->targets, tg0.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    }
    if (!batched) {
        // tensor-parallel ranks, shapes off the 64-column step, LLMK_PREFILL=0: token by token; the pass leaves the position's logits in
        // the pinned vector (as for llmk_forward), one workgroup row of pf_score_kernel reads them from there
        const int np = (V + PF_SC_ROWS - 1) / PF_SC_ROWS;
        PfEpiArgs e;
        memset(&e, 0, sizeof(e));
        for (int i = 0; i < n; ++i) {
            rc = run_token(c, tokens[i], pos0 + i, TAIL_LOGITS);
            if (rc) return rc;
            if (logits_out) memcpy(logits_out + (size_t)i * V, c->h_logits, (size_t)V * sizeof(float));
            PfScoreArgs s;
            memset(&s, 0, sizeof(s));
            s.Z = c->h_logits.dev(); s.zp = (size_t)V; s.V = V; s.nparts = np; s.part = c->sc->part[0];
            s.targets = sj.want_lp ? c->sc->targets + i : nullptr; s.tgt = c->sc->tgt[0];
            hipLaunchKernelGGL((pf_score_kernel<false>), dim3(np, 1), dim3(256), 0, c->stream, e, s);
            HIPCHK(hipGetLastError());
            HIPCHK(sc_merge(c, 0, c->stream, sj, np, 1, i));
            HIPCHK(hipStreamSynchronize(c->stream));             // (the next pass overwrites the pinned vector)
        }
    } else {
        rc = pf_run(c, tokens, n, pos0, &sj);
        if (rc) return rc;
    }
    // the results: one copy, n floats and n ints
    HIPCHK(hipMemcpyAsync(c->sc->h_out, c->sc->out, (size_t)2 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (batched && pf_flagged(c)) {
        static bool told = false;
        return pf_redo(c, "llmk_score", &told, [&] { return llmk_score(c, tokens, n, pos0, targets, logprob_out, argmax_out, logits_out); });
    }
    const int* ids = reinterpret_cast<const int*>(c->sc->h_out + n);
    for (int i = 0; i < n; ++i)
        if (ids[i] < 1 || ids[i] > V) return LLMK_E_NONFINITE;      // no logit of the position is finite (pf_score_merge_kernel answers id 0)
    if (logprob_out) memcpy(logprob_out, c->sc->h_out, (size_t)n * sizeof(float));
    if (argmax_out) memcpy(argmax_out, ids, (size_t)n * sizeof(int));
    if (batched && logits_out) HIPCHK(hipMemcpy(logits_out, c->sc->logits, (size_t)n * V * sizeof(float), hipMemcpyDeviceToHost));
    return LLMK_OK;
}

// the id a pass with any tail but TAIL_LOGITS left in h_next
int token_out(llmk_ctx* c, int token, int pos, TailMode tail, int* next_token) {
    int rc = run_token(c, token, pos, tail);
    if (rc) return rc;
    // the device argmax answers 0 ("no token") when no logit is finite (a damaged upload, an overflow): an error, not an id --
    // a host that indexes its vocabulary with it reads out of bounds (advisor, round 4)
    if (c->h_next->id < 1 || c->h_next->id > c->V) return LLMK_E_NONFINITE;
    *next_token = c->h_next->id;
    return LLMK_OK;
}

// ---- the device sampler (sample.h, sample_filter.h, sample_penalty.h): one request, three bodies ------------------------------------
static_assert(LLMK_PENALTY_MAX_BIAS == LLMK_MAX_LOGIT_BIAS, "sample_penalty.h and llmk.h agree on the length of the bias list");
// the token records of `seqs` sequences of `positions` each, their counts over V ids and the parameter words of `rows` rows: built
// aside (and zeroed) by the first call that needs them
static int pen_setup(PenaltyState& pen, int device, hipStream_t st, size_t seqs, size_t positions, size_t V, size_t rows) {
    if (pen.h_pen) return LLMK_OK;
    HIPCHK(hipSetDevice(device));
    PenaltyState p;
    HIPCHK(p.hist.alloc(seqs * positions));
    HIPCHK(p.hist.zero(st));
    HIPCHK(p.cnt.alloc(seqs * V));
    HIPCHK(p.cnt.zero(st));
    HIPCHK(p.d_pen.alloc(rows));
    HIPCHK(p.d_pen.zero(st));
    HIPCHK(p.h_pen.alloc(rows));
    memset(p.h_pen, 0, rows * sizeof(llmk_penalty_params));
    HIPCHK(hipStreamSynchronize(st));
    pen = std::move(p);
    return LLMK_OK;
}
static int pen_setup(llmk_ctx* c) { return pen_setup(c->pen, c->cfg.device, c->stream, 1, (size_t)c->S, (size_t)c->V, 1); }
// ---- decode log-probs (logprob.h) ----
static_assert(LLMK_LOGPROB_MAX_TOP == LLMK_MAX_TOP_LOGPROBS, "logprob.h and llmk.h agree on the length of the list");
// the checks of a log-prob request: nothing runs and nothing is allocated here
static bool logprob_args_ok(const llmk_ctx* c, const llmk_logprobs* lp) {
    if (!c || !lp || lp->top_n < 0 || lp->top_n > LLMK_MAX_TOP_LOGPROBS) return false;
    if (lp->top_n == 0 && !lp->token_logprob) return false;
    if (lp->top_n > 0 && (!lp->top_tokens || !lp->top_logprobs)) return false;
    return c->tp_size == 1 && !c->comm && !c->p2p;
}
// Room for nrec records on the device and in pinned memory (zeroed; a request for more than there is drains `st` and replaces both),
// the pinned top_n word -- dev_top: and a device copy of it -- and, under penalties, nraw raw logits (0: none): each allocated by the
// first call that needs it
static int lp_setup(LogprobState& lp, int device, hipStream_t st, size_t nrec, size_t nraw, bool dev_top) {
    HIPCHK(hipSetDevice(device));
    if (lp.h.size() < nrec) {
        HIPCHK(lp.d.reserve(nrec, st));
        HIPCHK(lp.d.zero(st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(lp.h.alloc(nrec));
        memset(lp.h, 0, nrec * sizeof(llmk_logprob_record));
    }
    if (!lp.h_top) {
        HIPCHK(lp.h_top.alloc(1));
        *lp.h_top = 0u;
    }
    if (dev_top && !lp.d_top) HIPCHK(lp.d_top.alloc(1));
    if (nraw && !lp.raw) HIPCHK(lp.raw.alloc(nraw));
    return LLMK_OK;
}
static int lp_setup(llmk_ctx* c, bool raw) { return lp_setup(c->lp, c->cfg.device, c->stream, (size_t)c->S + 1, raw ? (size_t)c->V : 0, false); }
// a checked request becomes the running call's (every site reads c->lp_top_n); LpScope ends it
static int logprob_request(llmk_ctx* c, const llmk_logprobs* lp, bool raw) {
    const int rc = lp_setup(c, raw);
    if (rc) return rc;
    *c->lp.h_top = (unsigned)lp->top_n;
    c->lp_top_n = lp->top_n;
    return LLMK_OK;
}
struct LpScope {
    llmk_ctx* c;
    ~LpScope() { c->lp_top_n = -1; }
};
// n pinned records into entries 0 .. n-1 of the caller's arrays
static void logprob_deliver(const llmk_logprob_record* rec, size_t n, const llmk_logprobs* lp) {
    for (size_t k = 0; k < n; ++k) {
        const llmk_logprob_record& r = rec[k];
        if (lp->token_logprob) lp->token_logprob[k] = r.token_logprob;
        for (int j = 0; j < lp->top_n; ++j) {
            lp->top_tokens[k * lp->top_n + j] = r.top_tokens[j];
            lp->top_logprobs[k * lp->top_n + j] = r.top_logprobs[j];
        }
    }
}

// What a sampling call asks for: checked, then put into the pinned words that the passes copy to the device -- h_samp (invT = f32(1 / T),
// rounded once), h_filt and, with a penalty or a bias on, h_pen (inv_r = f32(1 / r), as invT is).  pn == null: an entry point WITHOUT a
// penalties argument (the _pen functions reject a null one themselves).  *tail: TAIL_PENALTY with a penalty or a bias on, else
// TAIL_FILTER with a filter on, else TAIL_SAMPLE -- so with nothing on the _pen functions ARE the _ex ones, and those the plain ones.
// Nothing is allocated (pen_setup) before every check has passed, and nothing at all for a request that needs no record.
// lp: the log-prob request of the _lp functions (null: none), checked first and granted last (logprob_request).
// The checks come first, in two functions that touch no context and no device: a context's request, llmk_batch_decode and the rows
// functions (a sampler and a penalties entry per row) all ask them.
// a public sampler, checked, as the filter kernel's words (invT = f32(1 / T)); false: out of range
static bool sampler_words(const llmk_sampler* sp, llmk_filter_params* out) {
    if (!sp) return false;
    if (sp->top_k < 0 || !(sp->top_p > 0.f && sp->top_p <= 1.f) || !(sp->min_p >= 0.f && sp->min_p <= 1.f)) return false;      // (NaN fails)
    if (!(sp->temperature > 0.f) || !isfinite(sp->temperature)) return false;      // (NaN fails the first test)
    const float invT = 1.0f / sp->temperature;
    if (!isfinite(invT) || !(invT >= FLT_MIN)) return false;              // 1/T beyond the normal f32 range
    *out = llmk_filter_params{invT, (uint32_t)sp->seed, (uint32_t)(sp->seed >> 32), sp->top_k, sp->top_p, sp->min_p, {0, 0}};
    return true;
}
// public penalties, checked against a vocabulary of V rows and a record of S positions, as the penalty kernel's words (inv_r = f32(1 / r);
// last_n = 0 unless a penalty is on); *active: a penalty or a bias is on.  false: out of range
static bool penalty_words(const llmk_penalties* pn, int V, int S, llmk_penalty_params* out, bool* active) {
    if (!pn || pn->last_n < 0 || pn->last_n > S) return false;
    if (!(pn->repeat > 0.f) || !isfinite(pn->repeat) || !isfinite(pn->frequency) || !isfinite(pn->presence)) return false;      // (NaN fails)
    const float inv_r = 1.0f / pn->repeat;
    if (!isfinite(inv_r) || !(inv_r >= FLT_MIN)) return false;
    if (pn->n_bias < 0 || pn->n_bias > LLMK_MAX_LOGIT_BIAS || (pn->n_bias > 0 && !pn->bias)) return false;
    for (int j = 0; j < pn->n_bias; ++j) {
        const llmk_logit_bias& b = pn->bias[j];
        if (b.token < 1 || b.token > V || !(isfinite(b.bias) || b.bias == -INFINITY)) return false;      // (NaN and +inf fail)
        for (int k = 0; k < j; ++k)
            if (pn->bias[k].token == b.token) return false;
    }
    const bool pen_on = pn->last_n > 0 && (pn->repeat != 1.f || pn->frequency != 0.f || pn->presence != 0.f);
    *active = pen_on || pn->n_bias > 0;
    *out = llmk_penalty_params{pn->repeat, inv_r, pn->frequency, pn->presence, pen_on ? pn->last_n : 0, pn->n_bias, {0, 0}, {}};
    for (int j = 0; j < pn->n_bias; ++j) out->bias[j] = llmk_penalty_bias{pn->bias[j].token, pn->bias[j].bias};
    return true;
}
static int sampler_request(llmk_ctx* c, const llmk_sampler* sp, const llmk_penalties* pn, TailMode* tail, const llmk_logprobs* lp = nullptr) {
    if (lp && !logprob_args_ok(c, lp)) return LLMK_E_ARG;
    llmk_filter_params filt;
    llmk_penalty_params pen;
    bool active = false;
    if (!sampler_words(sp, &filt) || (pn && !penalty_words(pn, c->V, c->S, &pen, &active))) return LLMK_E_ARG;
    *c->h_samp = llmk_sample_params{filt.invT, filt.seed_lo, filt.seed_hi, 0};
    *c->h_filt = filt;
    *tail = sp->top_k != 0 || sp->top_p != 1.f || sp->min_p != 0.f ? TAIL_FILTER : TAIL_SAMPLE;
    if (!active) return lp ? logprob_request(c, lp, false) : LLMK_OK;
    int rc = pen_setup(c);
    if (rc) return rc;
    if (lp && (rc = logprob_request(c, lp, true)) != LLMK_OK) return rc;
    *c->pen.h_pen = pen;
    *tail = TAIL_PENALTY;
    return LLMK_OK;
}

// One position, the next token drawn on the device
static int sample_forward(llmk_ctx* c, int token, int pos, const llmk_sampler* sp, const llmk_penalties* pn, int* next_token) {
    TailMode tail;
    const int rc = sampler_request(c, sp, pn, &tail);
    return rc ? rc : token_out(c, token, pos, tail, next_token);
}

static bool decode_args_ok(const llmk_ctx* c, int token, int pos0, int n, const int* ids_out) {
    return c && ids_out && n >= 1 && pos0 >= 1 && pos0 + n - 1 <= c->S && token >= 1 && token <= c->V;
}
// The generation loop of llama2.f90:379-396 for n positions with no host round trip between them: at temperature 0
// (TAIL_GREEDY, the argmax) or by the request in the pinned words (sampler_request)
// lp: where the log-prob records of a running request (c->lp_top_n >= 0) are delivered once every id is there
int decode_run(llmk_ctx* c, int token, int pos0, int n, TailMode tail, int* ids_out, llmk_token_fn on_token, void* user,
               const llmk_logprobs* lp = nullptr) {
    int rc = check_ready(c);
    if (rc) return rc;
    const bool timed = (c->cfg.flags & (LLMK_FLAG_TIMINGS | LLMK_FLAG_NO_GRAPH)) != 0;
    int done = 0;
    if (c->use_tk && !timed && !c->p2p && !c->comm && c->tp_size == 1) {
        // n launches enqueued back to back: launch i takes its token from launch i-1's candidates (device memory) and leaves
        // its own; ids reach the host through mapped memory as CU 0 of the NEXT launch resolves them
        HIPCHK(hipSetDevice(c->cfg.device));
        int* h_ids = c->host_words()->ids();
        int* h_ids_dev = c->host_words_dev()->ids();
        TkDevWords* dw = c->dev_words();
        memset(h_ids, 0, (size_t)n * sizeof(int));
        c->host_words()->err = 0;
        HIPCHK(tk_qsc_before_launch(c, pos0));
        // the GR launches score their classifier rows with the sampling words (token_kernel.h tk_sample_params): the request's, or
        // zeros -- invT = 0 is greedy, which is also what the sampler kernels run behind (enqueue_sampler).  Those words and the
        // filter's are written only where the device holds others
        const bool filter_tail = tail == TAIL_FILTER || tail == TAIL_PENALTY;
        const llmk_sample_params want = tail == TAIL_SAMPLE ? *c->h_samp : llmk_sample_params{};
        if (filter_tail)
            HIPCHK(c->filt_dev.push(*c->h_filt, [&] { return hipMemcpyAsync(&dw->filt, c->h_filt, sizeof(llmk_filter_params), hipMemcpyHostToDevice, c->stream); }));
        HIPCHK(c->samp_dev.push(want, [&] {
            return tail == TAIL_SAMPLE ? hipMemcpyAsync(&dw->samp, c->h_samp, sizeof(llmk_sample_params), hipMemcpyHostToDevice, c->stream)
                                       : hipMemsetAsync(&dw->samp, 0, sizeof(llmk_sample_params), c->stream);
        }));
        if (lp) HIPCHK(copy_logprob_top(c));
        for (int i = 0; i < n; ++i) {
            c->h_tokpos[0] = token - 1;
            c->h_tokpos[1] = pos0 + i;
            c->h_tokpos[2] += 1;
            TkGreedy g;
            g.gflags = TKG_GREEDY | (i ? TKG_CAND_IN | TKG_ID : 0);
            g.id_index = i - 1;
            c->tk_short_grid = tk_inject_timeout(pos0 + i);      // (INSIDE the pipeline)
            HIPCHK(launch_token_kernel(c, false, g));
            // the fed token: the host's at the first position, afterwards the id the filter kernel of the position before left in d_next
            if (filter_tail)
                HIPCHK(enqueue_sampler(c, tail == TAIL_PENALTY, {nullptr, pos0 + i, token, i ? c->d_next : nullptr, c->pen.hist,
                                                                 dw->cand[(pos0 + i) & 1], TK_NCU, i == 0, false,
                                                                 lp ? c->lp.d + (pos0 + i - 1) : nullptr}));
            else if (lp)      // the id: the fold of this launch's candidates, as the next launch (or cand_resolve_kernel) takes it
                HIPCHK(enqueue_logprob(c, c->d_logits, nullptr, dw->cand[(pos0 + i) & 1], TK_NCU, 0, c->lp.d + (pos0 + i - 1)));
        }
        if (lp)      // the records of the whole call, in one copy
            HIPCHK(hipMemcpyAsync(c->lp.h + (pos0 - 1), c->lp.d + (pos0 - 1), (size_t)n * sizeof(llmk_logprob_record), hipMemcpyDeviceToHost, c->stream));
        hipLaunchKernelGGL(cand_resolve_kernel, dim3(1), dim3(64), 0, c->stream, dw->cand[(pos0 + n - 1) & 1], h_ids_dev + (n - 1), c->d_next, &dw->err, c->V);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&c->h_next->err, &dw->err, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        // drain: ids are 1-based, 0 = the stream drained without this one: an error below
        for (int id; done < n; ++done) {
            if ((rc = tk_published_id(c, done, &id)) != LLMK_OK) return rc;
            if (id == 0) break;
            ids_out[done] = id;
            if (on_token) on_token(done, id, user);
        }
        HIPCHK(hipStreamSynchronize(c->stream));
        volatile int* ids = h_ids;
        for (; done < n && ids[done] != 0; ++done) {
            ids_out[done] = ids[done];
            if (on_token) on_token(done, ids_out[done], user);
        }
        const unsigned err = c->h_next->err;
        const TkRecovery::Pipelined end = c->tk.pipelined_end(pos0, n, done, err);
        if (end.what == TkVerdict::CLEAN) {
            if (lp) logprob_deliver(c->lp.h + (pos0 - 1), (size_t)n, lp);
            return LLMK_OK;
        }
        // every launch behind the trouble drained on the sticky word: the rest of the call, from the first position whose id never
        // arrived, goes position by position through run_token -- on the multi-kernel path after a retirement (it rewrites those KV
        // rows), else on the kernel, which redoes just the positions that need it (token_pass) -- once the records that the launches
        // behind a range event left of its debris are dropped
        rc = tk_perform(c, end.what, err, end.resume);
        if (rc) return rc;
        HIPCHK(tk_qsc_keep(c, end.keep));
        if (done > 0) token = ids_out[done - 1];
        c->tk_short_grid = false;
    }
    for (int i = done; i < n; ++i) {
        rc = run_token(c, token, pos0 + i, tail);
        if (rc) return rc;
        if (c->h_next->id < 1 || c->h_next->id > c->V) return LLMK_E_NONFINITE;      // (before the callback sees it)
        token = ids_out[i] = c->h_next->id;
        if (lp) c->lp.h[pos0 + i - 1] = c->lp.h[c->S];      // (a redone position rewrites its record)
        if (on_token) on_token(i, token, user);
    }
    if (lp) logprob_deliver(c->lp.h + (pos0 - 1), (size_t)n, lp);
    return LLMK_OK;
}

static int sample_decode(llmk_ctx* c, int token, int pos0, int n, const llmk_sampler* sp, const llmk_penalties* pn, int* ids_out,
                         llmk_token_fn on_token, void* user) {
    TailMode tail;
    const int rc = sampler_request(c, sp, pn, &tail);
    return rc ? rc : decode_run(c, token, pos0, n, tail, ids_out, on_token, user);
}

// Verification hook: the rule on the caller's logits as if they were those of position `pos`, by the kernels every path runs (no
// token pass; the ctx's own logits buffer is overwritten, nothing else -- the sticky error word behind it included).  The filter
// kernel runs with all filters off too; the penalty kernel's window is read from the record, which is not written.
static int sample_logits(llmk_ctx* c, const float* logits, int pos, const llmk_sampler* sp, const llmk_penalties* pn, int* token_out_,
                         int* kept_out, float* tau_out, float* adjusted_out) {
    TailMode tail;
    int rc = sampler_request(c, sp, pn, &tail);
    if (rc) return rc;
    if ((rc = check_ready(c)) != LLMK_OK) return rc;
    HIPCHK(hipSetDevice(c->cfg.device));
    c->filt_dev.invalidate();
    HIPCHK(hipMemcpyAsync(c->d_logits, logits, (size_t)c->V * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(enqueue_sampler(c, tail == TAIL_PENALTY, {nullptr, pos, 0, nullptr, nullptr, nullptr, 0, true, true}));
    HIPCHK(hipMemcpyAsync(&c->h_next->id, c->d_next, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&c->h_next->kept, c->dev_words()->filter_out, sizeof(TkDevWords::filter_out), hipMemcpyDeviceToHost, c->stream));      // kept, tau
    if (adjusted_out) HIPCHK(hipMemcpyAsync(adjusted_out, c->d_logits, (size_t)c->V * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->filt_dev.confirm(*c->h_filt);
    if (kept_out) *kept_out = c->h_next->kept;
    if (tau_out) *tau_out = c->h_next->tau;
    if (c->h_next->id < 1 || c->h_next->id > c->V) return LLMK_E_NONFINITE;
    *token_out_ = c->h_next->id;
    return LLMK_OK;
}

// The entry points: their own pointer and range checks, then one of the bodies above
int llmk_forward_greedy(llmk_ctx* c, int token, int pos, int* next_token) {
    if (!c || !next_token) return LLMK_E_ARG;
    return token_out(c, token, pos, TAIL_GREEDY, next_token);
}
int llmk_forward_sample(llmk_ctx* c, int token, int pos, float temperature, uint64_t seed, int* next_token) {
    if (!c || !next_token) return LLMK_E_ARG;
    const llmk_sampler sp = {temperature, 0, 1.f, 0.f, seed};      // (no filter)
    return sample_forward(c, token, pos, &sp, nullptr, next_token);
}
int llmk_forward_sample_ex(llmk_ctx* c, int token, int pos, const llmk_sampler* sp, int* next_token) {
    if (!c || !next_token) return LLMK_E_ARG;
    return sample_forward(c, token, pos, sp, nullptr, next_token);
}
int llmk_forward_sample_pen(llmk_ctx* c, int token, int pos, const llmk_sampler* sp, const llmk_penalties* pn, int* next_token) {
    if (!c || !next_token || !pn || token < 1 || token > c->V || pos < 1 || pos > c->S) return LLMK_E_ARG;      // (before pen_setup allocates)
    return sample_forward(c, token, pos, sp, pn, next_token);
}
int llmk_decode_greedy(llmk_ctx* c, int token, int pos0, int n, int* ids_out, llmk_token_fn on_token, void* user) {
    if (!decode_args_ok(c, token, pos0, n, ids_out)) return LLMK_E_ARG;
    return decode_run(c, token, pos0, n, TAIL_GREEDY, ids_out, on_token, user);
}
int llmk_decode_sample(llmk_ctx* c, int token, int pos0, int n, float temperature, uint64_t seed, int* ids_out,
                       llmk_token_fn on_token, void* user) {
    if (!decode_args_ok(c, token, pos0, n, ids_out)) return LLMK_E_ARG;
    const llmk_sampler sp = {temperature, 0, 1.f, 0.f, seed};      // (no filter)
    return sample_decode(c, token, pos0, n, &sp, nullptr, ids_out, on_token, user);
}
int llmk_decode_sample_ex(llmk_ctx* c, int token, int pos0, int n, const llmk_sampler* sp, int* ids_out, llmk_token_fn on_token, void* user) {
    if (!decode_args_ok(c, token, pos0, n, ids_out)) return LLMK_E_ARG;
    return sample_decode(c, token, pos0, n, sp, nullptr, ids_out, on_token, user);
}
int llmk_decode_sample_pen(llmk_ctx* c, int token, int pos0, int n, const llmk_sampler* sp, const llmk_penalties* pn, int* ids_out,
                           llmk_token_fn on_token, void* user) {
    if (!decode_args_ok(c, token, pos0, n, ids_out) || !pn) return LLMK_E_ARG;
    return sample_decode(c, token, pos0, n, sp, pn, ids_out, on_token, user);
}
// (whole-model contexts only: a TP rank's classifier owns a slice of the vocabulary, and its logits buffer belongs to the collective.
// The _pen hook's window ends at `pos`, so pos <= seq_len there)
int llmk_sample_logits(llmk_ctx* c, const float* logits, int pos, const llmk_sampler* sp, int* token_out_, int* kept_out, float* tau_out) {
    if (!c || !logits || !token_out_ || pos < 1 || c->tp_size != 1) return LLMK_E_ARG;
    return sample_logits(c, logits, pos, sp, nullptr, token_out_, kept_out, tau_out, nullptr);
}
int llmk_sample_logits_pen(llmk_ctx* c, const float* logits, int pos, const llmk_sampler* sp, const llmk_penalties* pn, int* token_out_,
                           int* kept_out, float* tau_out, float* adjusted_out) {
    if (!c || !logits || !token_out_ || !pn || pos < 1 || pos > c->S || c->tp_size != 1) return LLMK_E_ARG;
    return sample_logits(c, logits, pos, sp, pn, token_out_, kept_out, tau_out, adjusted_out);
}
// The _lp functions: the request of the _pen functions (penalties optional), or the greedy form (no sampler), plus the record
int llmk_forward_sample_lp(llmk_ctx* c, int token, int pos, const llmk_sampler* sp, const llmk_penalties* pn, const llmk_logprobs* lp,
                           int* next_token) {
    if (!c || !next_token || !logprob_args_ok(c, lp) || (!sp && pn) || token < 1 || token > c->V || pos < 1 || pos > c->S) return LLMK_E_ARG;
    int rc = check_ready(c);      // (before logprob_request allocates)
    if (rc) return rc;
    LpScope scope{c};
    TailMode tail = TAIL_GREEDY;
    rc = sp ? sampler_request(c, sp, pn, &tail, lp) : logprob_request(c, lp, false);
    if (rc == LLMK_OK) rc = token_out(c, token, pos, tail, next_token);
    if (rc == LLMK_OK) logprob_deliver(c->lp.h + c->S, 1, lp);
    return rc;
}
int llmk_decode_sample_lp(llmk_ctx* c, int token, int pos0, int n, const llmk_sampler* sp, const llmk_penalties* pn, const llmk_logprobs* lp,
                          int* ids_out, llmk_token_fn on_token, void* user) {
    if (!decode_args_ok(c, token, pos0, n, ids_out) || !logprob_args_ok(c, lp) || (!sp && pn)) return LLMK_E_ARG;
    int rc = check_ready(c);      // (before logprob_request allocates)
    if (rc) return rc;
    LpScope scope{c};
    TailMode tail = TAIL_GREEDY;
    rc = sp ? sampler_request(c, sp, pn, &tail, lp) : logprob_request(c, lp, false);
    return rc ? rc : decode_run(c, token, pos0, n, tail, ids_out, on_token, user, lp);
}
// (the hook: sample_logprob_kernel on the caller's logits, the id given)
int llmk_logprob_logits(llmk_ctx* c, const float* logits, int token, int top_n, float* token_logprob, int32_t* top_tokens, float* top_logprobs) {
    const llmk_logprobs lp = {top_n, token_logprob, top_tokens, top_logprobs};
    if (!c || !logits || !logprob_args_ok(c, &lp) || token < 0 || token > c->V) return LLMK_E_ARG;
    int rc = check_ready(c);
    if (rc) return rc;
    if ((rc = lp_setup(c, false)) != LLMK_OK) return rc;      // (no site reads a running request here: the kernel is enqueued below)
    *c->lp.h_top = (unsigned)top_n;
    HIPCHK(hipMemcpyAsync(c->d_logits, logits, (size_t)c->V * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(copy_logprob_top(c));
    HIPCHK(enqueue_logprob(c, c->d_logits, nullptr, nullptr, 0, token, c->lp.d + c->S));
    HIPCHK(hipMemcpyAsync(c->lp.h + c->S, c->lp.d + c->S, sizeof(llmk_logprob_record), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    logprob_deliver(c->lp.h + c->S, 1, &lp);
    return LLMK_OK;
}
int llmk_set_history(llmk_ctx* c, const int* tokens, int n, int pos0) {
    if (!c || !tokens || n < 1 || pos0 < 1 || pos0 + n - 1 > c->S) return LLMK_E_ARG;
    for (int i = 0; i < n; ++i)
        if (tokens[i] < 0 || tokens[i] > c->V) return LLMK_E_ARG;
    { const int rc_ = spec_settle(c); if (rc_) return rc_; }
    const int rc = pen_setup(c);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c->pen.hist + (pos0 - 1), tokens, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LLMK_OK;
}
int llmk_get_history(llmk_ctx* c, int* tokens_out, int n, int pos0) {
    if (!c || !tokens_out || n < 1 || pos0 < 1 || pos0 + n - 1 > c->S) return LLMK_E_ARG;
    { const int rc_ = spec_settle(c); if (rc_) return rc_; }
    const int rc = pen_setup(c);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(tokens_out, c->pen.hist + (pos0 - 1), (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LLMK_OK;
}

// ---- batched decode (batch.h): the entry points; the pass itself (bd_pass) is above, in front of pf_redo --------
// the context's side of a pass: workspaces, the classifier's kernels and its row chunks (they follow the matrix instruction in use)
static int bd_ready(llmk_batch* b, ScPlan* sp, int rows) {
    llmk_ctx* c = b->ctx;
    int rc = check_ready(c);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->cfg.device));
    if ((rc = sc_setup(c)) != LLMK_OK) return rc;
    if ((rc = pf_setup(c, true)) != LLMK_OK) return rc;
    const int ct = c->t[LLMK_WCLS].type;
    *sp = sc_plan(c, rows);
    if (ct != LLMK_TYPE_Q6_K && sp->R == 0) return LLMK_E_SHAPE;      // no chunk of the classifier fits the workspace: there is no token-by-token form
    return LLMK_OK;
}
// rows of a call: n in [1, n_slots], distinct slots, ids and positions in range (last_pos: the last position the call writes)
// (fed = false: rows that feed no token -- the hook of the rows functions; `tokens` is not read)
static bool bd_rows_ok(const llmk_batch* b, int n, const int* slots, const int* tokens, const int* pos, int span, bool fed = true) {
    if (!slots || (fed && !tokens) || !pos || n < 1 || n > b->n_slots || span < 1) return false;
    bool seen[LLMK_MAX_BATCH] = {};
    for (int i = 0; i < n; ++i) {
        if (slots[i] < 0 || slots[i] >= b->n_slots || seen[slots[i]]) return false;
        seen[slots[i]] = true;
        if (fed && (tokens[i] < 1 || tokens[i] > b->ctx->V)) return false;
        if (pos[i] < 1 || pos[i] > b->seq_len || span - 1 > b->seq_len - pos[i]) return false;
        if (b->n_attached > 0 && pos[i] <= b->px->h_first[slots[i]]) return false;      // an attached slot's positions 1..P are the prefix
    }
    return true;
}
static hipError_t bd_upload_rows(llmk_batch* b, int n, const int* slots, const int* tokens, const int* pos) {
    for (int i = 0; i < n; ++i) {
        b->h_rows[i] = BdRow{slots[i], pos[i]};
        b->h_tok[i] = tokens ? tokens[i] - 1 : 0;      // (null: rows that feed no token, bd_rows_ok)
    }
    hipStream_t st = b->ctx->stream;
    b->pass_att = 0;
    b->pass_groups = 0;
    if (b->n_attached > 0) {
        // the column map: the attached rows in row order, -1 up to the end of the last column group
        for (int i = 0; i < n; ++i)
            if (b->px->h_first[slots[i]] > 0) b->px->h_colmap[b->pass_att++] = i;
        if (b->pass_att > 0) {
            const int rg = bd_prefix_rg(b->ctx->kv_mul), cells = bd_prefix_groups(b->pass_att, b->ctx->kv_mul) * rg;
            for (int k = b->pass_att; k < cells; ++k) b->px->h_colmap[k] = -1;
            HIPRET(hipMemcpyAsync(b->px->d_colmap, b->px->h_colmap, (size_t)cells * sizeof(int), hipMemcpyHostToDevice, st));
        }
    }
    HIPRET(hipMemcpyAsync(b->d_rows, b->h_rows, (size_t)n * sizeof(BdRow), hipMemcpyHostToDevice, st));
    return hipMemcpyAsync(b->d_tok, b->h_tok, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st);
}

// an IEEE half's bits as the f32 of the same value (host side of llmk_cache_peek; subnormals, infinities and NaN included)
static float bd_half_bits_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, ex = (h >> 10) & 0x1Fu, man = h & 0x3FFu;
    uint32_t u;
    if (ex == 0x1Fu) {
        u = sign | 0x7F800000u | (man << 13);
    } else if (ex != 0) {
        u = sign | ((ex + 112u) << 23) | (man << 13);
    } else {
        // man * 2^-24, exact in f32
        float f = (float)man * 5.9604644775390625e-8f;
        memcpy(&u, &f, sizeof u);
        u |= sign;
    }
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

// an allocation the device has no room for is the caller's to handle (llmk_cache_create sizes caches by n_slots x seq_len), not a HIP fault
static int bd_alloc_rc(hipError_t e) {
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();      // (the runtime keeps the error for the next hipGetLastError: a launch check must not find it)
        return LLMK_E_NOMEM;
    }
    return e == hipSuccess ? LLMK_OK : LLMK_E_HIP + (int)e;
}

// llmk_batch_create IS this with LLMK_TYPE_F32: the caches of an f32 batch are allocated, zeroed and used as they always were
static int bd_create(llmk_ctx* c, int n_slots, int seq_len, int kv_type, llmk_batch** out) {
    if (!c || !out || n_slots < 1 || n_slots > LLMK_MAX_BATCH || seq_len < 1 || seq_len > c->S) return LLMK_E_ARG;
    *out = nullptr;
    if (kv_type != LLMK_TYPE_F32 && kv_type != LLMK_TYPE_F16 && kv_type != LLMK_TYPE_Q8_0) return LLMK_E_TYPE;
    int rc = check_ready(c);      // (an incomplete context is LLMK_E_STATE whatever its shape)
    if (rc) return rc;
    if (!pf_shape_ok(c) || c->kv_mul > BD_MAX_GROUP) return LLMK_E_SHAPE;
    if (kv_type == LLMK_TYPE_Q8_0 && c->KV % 32 != 0) return LLMK_E_SHAPE;      // a q8_0 block is 32 elements of a position's row
    HIPCHK(hipSetDevice(c->cfg.device));
    // built aside: the caller gets the batch only after every step succeeded (a failure releases what was made)
    auto b = std::make_unique<llmk_batch>();
    b->ctx = c; b->n_slots = n_slots; b->seq_len = seq_len; b->kv_type = kv_type;
    b->span_attn = !(getenv("LLMK_SPAN_ATTN") && getenv("LLMK_SPAN_ATTN")[0] == '0');
    ScPlan sp;
    if ((rc = bd_ready(b.get(), &sp, n_slots)) != LLMK_OK) return rc;
    const size_t cache = (size_t)c->L * n_slots * seq_len * c->KV, nb = LLMK_MAX_BATCH;
    rc = with_kv_type(b.get(), [&](auto t) -> int {
        using TC = decltype(t);
        int rc_;
        if ((rc_ = bd_alloc_rc(BdKv<TC>::kc(b.get()).alloc(BdKv<TC>::units(cache)))) != LLMK_OK) return rc_;
        if ((rc_ = bd_alloc_rc(BdKv<TC>::vc(b.get()).alloc(BdKv<TC>::units(cache)))) != LLMK_OK) return rc_;
        HIPCHK(BdKv<TC>::kc(b.get()).zero(c->stream));
        HIPCHK(BdKv<TC>::vc(b.get()).zero(c->stream));
        return LLMK_OK;
    });
    if (rc) return rc;
    HIPCHK(b->d_rows.alloc(nb));
    HIPCHK(b->d_tok.alloc(nb));
    HIPCHK(b->d_out.alloc(2 * nb));
    HIPCHK(b->d_logits.alloc((size_t)n_slots * c->V));
    // parts > 1 only while rows x kv heads x parts <= n_cu (bd_parts)
    HIPCHK(b->d_po.alloc((size_t)c->n_cu * BD_MAX_GROUP * c->hs));
    HIPCHK(b->d_pml.alloc((size_t)c->n_cu * BD_MAX_GROUP));
    HIPCHK(b->d_next.alloc(nb));
    HIPCHK(b->d_filt.alloc(nb));
    HIPCHK(b->d_out2.alloc(2 * nb));
    HIPCHK(b->d_err.alloc(1));
    HIPCHK(b->h_rows.alloc(nb));
    HIPCHK(b->h_tok.alloc(nb));
    HIPCHK(b->h_filt.alloc(nb));
    HIPCHK(b->h_out.alloc(2 * nb));
    HIPCHK(b->h_err.alloc(1));
    HIPCHK(with_head_size(c->hs, [&](auto hs) {
        constexpr int HS = decltype(hs)::value;
        return with_kv_type(b.get(), [](auto t) {
            return hipFuncSetAttribute((const void*)BdAttn<HS, decltype(t)>::row, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attn_smem(BD_WAVES, HS));
        });
    }));
    HIPCHK(hipStreamSynchronize(c->stream));
    ++c->n_batches;
    *out = b.release();
    return LLMK_OK;
}

int llmk_batch_create(llmk_ctx* c, int n_slots, int seq_len, llmk_batch** out) { return bd_create(c, n_slots, seq_len, LLMK_TYPE_F32, out); }
int llmk_cache_create(llmk_ctx* c, int n_slots, int seq_len, int kv_type, llmk_batch** out) { return bd_create(c, n_slots, seq_len, kv_type, out); }

int llmk_cache_type(llmk_batch* b) {
    if (!b) return -LLMK_E_ARG;
    return b->kv_type;
}

// device bytes of the K/V caches and of the prefix rows (the blocks as they are allocated: a prefix's only grow)
int llmk_cache_bytes(llmk_batch* b, unsigned long long* out) {
    if (!b || !out) return LLMK_E_ARG;
    *out = with_kv_type(b, [&](auto t) -> unsigned long long {
        using TC = decltype(t);
        size_t n = BdKv<TC>::kc(b).size() + BdKv<TC>::vc(b).size();
        if (b->px) n += BdKv<TC>::pk(*b->px).size() + BdKv<TC>::pv(*b->px).size();
        return (unsigned long long)n * sizeof(*BdKv<TC>::kc(b).get());
    });
    return LLMK_OK;
}

// The verification hook of the caches: n rows [kv_dim] of K (which 0) or V (1), positions pos0 .. pos0+n-1 of `slot` in `layer`, or of
// the prefix (slot -1, positions 1..P), as f32 -- exact for either type.
int llmk_cache_peek(llmk_batch* b, int which, int layer, int slot, int pos0, int n, float* out) {
    if (!b || !out || (which != 0 && which != 1) || layer < 0 || layer >= b->ctx->L || n < 1 || pos0 < 1) return LLMK_E_ARG;
    if (slot < -1 || slot >= b->n_slots || n > (slot < 0 ? b->P : b->seq_len) - (pos0 - 1)) return LLMK_E_ARG;
    llmk_ctx* c = b->ctx;
    HIPCHK(hipSetDevice(c->cfg.device));
    { const int rc_ = spec_settle(c); if (rc_) return rc_; }
    HIPCHK(hipStreamSynchronize(c->stream));
    const size_t row = (size_t)c->KV, cnt = (size_t)n * row;
    if (b->kv_type == LLMK_TYPE_Q8_0) {
        // value[i] = (float)q[i] * (float)d of i's block: one f32 product, exact (and never -0.0: d >= 0, or NaN)
        const size_t elems = (size_t)c->L * (slot < 0 ? (size_t)b->P : (size_t)b->n_slots * b->seq_len) * row;
        const size_t e0 = slot < 0 ? ((size_t)layer * b->P + (pos0 - 1)) * row : (((size_t)layer * b->n_slots + slot) * b->seq_len + (pos0 - 1)) * row;
        const Q8Rows src = attn_at(BdKv<KvQ8>::view(slot < 0 ? (which ? b->px->d_pv8 : b->px->d_pk8) : (which ? b->d_vc8 : b->d_kc8), elems), e0);
        std::vector<int8_t> q(cnt);
        std::vector<uint16_t> d(cnt / 32);
        HIPCHK(hipMemcpy(q.data(), src.q, cnt, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(d.data(), src.d, cnt / 32 * sizeof(uint16_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < cnt; ++i) out[i] = (float)q[i] * bd_half_bits_to_float(d[i / 32]);
        return LLMK_OK;
    }
    return with_kv_type(b, [&](auto t) -> int {
        using TC = std::conditional_t<std::is_same_v<decltype(t), KvQ8>, float, decltype(t)>;      // (q8_0 is answered above)
        const TC* src = slot < 0 ? (which ? BdKv<TC>::pv(*b->px) : BdKv<TC>::pk(*b->px)) + ((size_t)layer * b->P + (pos0 - 1)) * row
                                 : (which ? BdKv<TC>::vc(b) : BdKv<TC>::kc(b)) + (((size_t)layer * b->n_slots + slot) * b->seq_len + (pos0 - 1)) * row;
        if constexpr (std::is_same_v<TC, float>) {
            HIPCHK(hipMemcpy(out, src, cnt * sizeof(float), hipMemcpyDeviceToHost));
        } else {
            std::vector<uint16_t> h(cnt);
            HIPCHK(hipMemcpy(h.data(), src, cnt * sizeof(uint16_t), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < cnt; ++i) out[i] = bd_half_bits_to_float(h[i]);
        }
        return LLMK_OK;
    });
}

int llmk_batch_destroy(llmk_batch* b) {
    if (!b) return LLMK_E_ARG;
    llmk_ctx* c = b->ctx;
    hipSetDevice(c->cfg.device);
    { const int rc_ = spec_settle(c); if (rc_) return rc_; }
    hipStreamSynchronize(c->stream);
    --c->n_batches;
    delete b;
    return LLMK_OK;
}

// a slot joins (first = P) or leaves (0) the prefix: its `first` word, here and on the device (ENQUEUED)
static hipError_t prefix_first(llmk_batch* b, int slot, int first) {
    b->n_attached += (first > 0) - (b->px->h_first[slot] > 0);
    b->px->h_first[slot] = first;
    return hipMemcpyAsync(b->px->d_first + slot, b->px->h_first + slot, sizeof(int), hipMemcpyHostToDevice, b->ctx->stream);
}

// rows n_pos .. seq_len-1 of `slot` in every layer of a q8_0 batch's caches: quants and scales zeroed, ENQUEUED
static hipError_t bd_q8_zero(llmk_batch* b, int slot, int n_pos) {
    llmk_ctx* c = b->ctx;
    const size_t row = (size_t)c->KV, slot_rows = (size_t)b->seq_len * row, cache = (size_t)c->L * b->n_slots * slot_rows;
    if (n_pos >= b->seq_len) return hipSuccess;
    for (DevBuf<int8_t>* buf : {&b->d_kc8, &b->d_vc8})
        for (int l = 0; l < c->L; ++l) {
            const Q8Rows at = attn_at(BdKv<KvQ8>::view(*buf, cache), ((size_t)l * b->n_slots + slot) * slot_rows + (size_t)n_pos * row);
            HIPRET(hipMemsetAsync(at.q, 0, slot_rows - (size_t)n_pos * row, c->stream));
            HIPRET(hipMemsetAsync(at.d, 0, (slot_rows - (size_t)n_pos * row) / 32 * sizeof(_Float16), c->stream));
        }
    return hipSuccess;
}

int llmk_batch_fork(llmk_batch* b, int slot, int n_pos) {
    if (!b || slot < 0 || slot >= b->n_slots || n_pos < 0 || n_pos > std::min(b->seq_len, b->ctx->S)) return LLMK_E_ARG;
    llmk_ctx* c = b->ctx;
    HIPCHK(hipSetDevice(c->cfg.device));
    { const int rc_ = spec_settle(c); if (rc_) return rc_; }
    const size_t row = (size_t)c->KV, slot_rows = (size_t)b->seq_len * row;
    if (b->kv_type == LLMK_TYPE_F32) {
        float* caches[2][2] = {{b->d_kc, c->d_kc}, {b->d_vc, c->d_vc}};
        for (auto& p : caches)
            for (int l = 0; l < c->L; ++l) {
                float* dst = p[0] + ((size_t)l * b->n_slots + slot) * slot_rows;
                if ((size_t)n_pos < (size_t)b->seq_len)      // rows beyond n_pos: as in a fresh slot
                    HIPCHK(hipMemsetAsync(dst + (size_t)n_pos * row, 0, (slot_rows - (size_t)n_pos * row) * sizeof(float), c->stream));
                if (n_pos > 0)
                    HIPCHK(hipMemcpyAsync(dst, p[1] + (size_t)l * c->S * row, (size_t)n_pos * row * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
            }
    } else if (b->kv_type == LLMK_TYPE_F16) {
        // the same on the f16 caches: zero halves behind n_pos, the context's f32 rows converted (pf_kv_half) in the place of the copy
        for (_Float16* base : {b->d_kc16.get(), b->d_vc16.get()})
            for (int l = 0; l < c->L && (size_t)n_pos < (size_t)b->seq_len; ++l)
                HIPCHK(hipMemsetAsync(base + ((size_t)l * b->n_slots + slot) * slot_rows + (size_t)n_pos * row, 0,
                                      (slot_rows - (size_t)n_pos * row) * sizeof(_Float16), c->stream));
        if (n_pos > 0)
            HIPCHK(bd_copy_ctx_rows(c, b->d_kc16 + (size_t)slot * slot_rows, b->d_vc16 + (size_t)slot * slot_rows, (size_t)n_pos * row, (size_t)b->n_slots * slot_rows));
    } else {
        // ... and on the q8_0 caches: q = 0, d = 0 behind n_pos (which reads back +0.0), the context's rows quantised (bd_to_q8_kernel)
        const size_t cache = (size_t)c->L * b->n_slots * slot_rows;
        HIPCHK(bd_q8_zero(b, slot, n_pos));
        if (n_pos > 0)
            HIPCHK(bd_copy_ctx_rows(c, attn_at(BdKv<KvQ8>::view(b->d_kc8, cache), (size_t)slot * slot_rows),
                                    attn_at(BdKv<KvQ8>::view(b->d_vc8, cache), (size_t)slot * slot_rows), (size_t)n_pos * row, (size_t)b->n_slots * slot_rows));
    }
    // a forked or emptied slot is a new sequence: no token fed yet (the caller records the prompt with llmk_rows_set_history)
    if (b->pen.hist) HIPCHK(hipMemsetAsync(b->pen.hist + (size_t)slot * b->seq_len, 0, (size_t)b->seq_len * sizeof(int), c->stream));
    if (b->px && b->px->h_first[slot] > 0) HIPCHK(prefix_first(b, slot, 0));      // a forked slot is self-contained: it leaves the prefix
    HIPCHK(hipStreamSynchronize(c->stream));
    return LLMK_OK;
}

// ---- a shared prefix (batch.h): one copy of the K/V rows of positions 1..P, the slots attached to it keep their own rows behind it ----
int llmk_prefix_set(llmk_batch* b, int n_pos) {
    if (!b || n_pos < 0 || n_pos > std::min(b->seq_len, b->ctx->S) - 1) return LLMK_E_ARG;
    if (b->n_attached > 0) return LLMK_E_STATE;
    llmk_ctx* c = b->ctx;
    if (n_pos == 0) { b->P = 0; return LLMK_OK; }      // (the buffers stay for the next prefix)
    int rc = check_ready(c);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->cfg.device));
    const size_t row = (size_t)c->KV, nb = LLMK_MAX_BATCH;
    if (!b->px) {
        // what a pass with attached rows needs beyond the prefix rows, built aside by the first call that sets a prefix
        auto px = std::make_unique<llmk_batch::Prefix>();
        const size_t states = nb * c->nkv * 2 * BD_MAX_PARTS * c->kv_mul, words = (size_t)b->n_slots;
        HIPCHK(px->d_first.alloc(words));
        HIPCHK(px->d_first.zero(c->stream));
        HIPCHK(px->h_first.alloc(words));
        memset(px->h_first, 0, words * sizeof(int));
        HIPCHK(px->d_colmap.alloc(nb + BD_MAX_GROUP));
        HIPCHK(px->h_colmap.alloc(nb + BD_MAX_GROUP));
        HIPCHK(px->d_xpo.alloc(states * c->hs));
        HIPCHK(px->d_xpml.alloc(states));
        HIPCHK(with_head_size(c->hs, [&](auto hs) -> hipError_t {
            constexpr int HS = decltype(hs)::value;
            return with_kv_type(b, [](auto t) -> hipError_t {
                using TC = decltype(t);
                HIPRET(hipFuncSetAttribute((const void*)BdAttn<HS, TC>::prefix, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attn_smem(BD_WAVES, HS)));
                return hipFuncSetAttribute((const void*)BdAttn<HS, TC>::own, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attn_smem(BD_WAVES, HS));
            });
        }));
        b->px = std::move(px);
    }
    // the prefix rows: room for n_pos positions (a longer prefix than any before drains the stream and replaces both blocks)
    const size_t px_rows = (size_t)c->L * n_pos * row;
    rc = with_kv_type(b, [&](auto t) -> int {
        using TC = decltype(t);
        auto &pk = BdKv<TC>::pk(*b->px), &pv = BdKv<TC>::pv(*b->px);
        if (pv.size() < BdKv<TC>::units(px_rows)) b->P = 0;
        int rc_;
        if ((rc_ = bd_alloc_rc(pk.reserve(BdKv<TC>::units(px_rows), c->stream))) != LLMK_OK) return rc_;
        if ((rc_ = bd_alloc_rc(pv.reserve(BdKv<TC>::units(px_rows), c->stream))) != LLMK_OK) return rc_;
        HIPCHK(bd_copy_ctx_rows(c, BdKv<TC>::view(pk, px_rows), BdKv<TC>::view(pv, px_rows), (size_t)n_pos * row, (size_t)n_pos * row));
        return LLMK_OK;
    });
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    b->P = n_pos;
    return LLMK_OK;
}

int llmk_prefix_attach(llmk_batch* b, int slot) {
    if (!b || slot < 0 || slot >= b->n_slots) return LLMK_E_ARG;
    if (b->P < 1) return LLMK_E_STATE;
    llmk_ctx* c = b->ctx;
    HIPCHK(hipSetDevice(c->cfg.device));
    { const int rc_ = spec_settle(c); if (rc_) return rc_; }
    // a new sequence behind the prefix: own rows and token record as llmk_batch_fork(b, slot, 0) leaves them
    const size_t slot_rows = (size_t)b->seq_len * c->KV;
    HIPCHK(with_kv_type(b, [&](auto t) -> hipError_t {
        using TC = decltype(t);
        if constexpr (std::is_same_v<TC, KvQ8>) {
            return bd_q8_zero(b, slot, 0);
        } else {
            for (TC* base : {BdKv<TC>::kc(b).get(), BdKv<TC>::vc(b).get()})
                for (int l = 0; l < c->L; ++l)
                    HIPRET(hipMemsetAsync(base + ((size_t)l * b->n_slots + slot) * slot_rows, 0, slot_rows * sizeof(TC), c->stream));
            return hipSuccess;
        }
    }));
    if (b->pen.hist) HIPCHK(hipMemsetAsync(b->pen.hist + (size_t)slot * b->seq_len, 0, (size_t)b->seq_len * sizeof(int), c->stream));
    HIPCHK(prefix_first(b, slot, b->P));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LLMK_OK;
}

int llmk_prefix_len(llmk_batch* b) {
    if (!b) return -LLMK_E_ARG;
    return b->P;
}

int llmk_batch_forward(llmk_batch* b, int n, const int* slots, const int* tokens, const int* pos, float* logits_out, int* argmax_out) {
    if (!b || (!logits_out && !argmax_out) || !bd_rows_ok(b, n, slots, tokens, pos, 1)) return LLMK_E_ARG;
    llmk_ctx* c = b->ctx;
    ScPlan sp;
    int rc = bd_ready(b, &sp, n);
    if (rc) return rc;
    HIPCHK(bd_upload_rows(b, n, slots, tokens, pos));
    HIPCHK(bd_pass(b, n, *std::max_element(pos, pos + n), logits_out != nullptr, sp));
    HIPCHK(hipMemcpyAsync(b->h_out, b->d_out, (size_t)2 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(pf_fetch_flag(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (pf_flagged(c)) {
        static bool told = false;
        return pf_redo(c, "llmk_batch_forward", &told, [&] { return llmk_batch_forward(b, n, slots, tokens, pos, logits_out, argmax_out); });
    }
    const int* ids = reinterpret_cast<const int*>(b->h_out + n);
    for (int i = 0; i < n; ++i)
        if (ids[i] < 1 || ids[i] > c->V) return LLMK_E_NONFINITE;
    if (argmax_out) memcpy(argmax_out, ids, (size_t)n * sizeof(int));
    if (logits_out) HIPCHK(hipMemcpy(logits_out, b->d_logits, (size_t)n * c->V * sizeof(float), hipMemcpyDeviceToHost));
    return LLMK_OK;
}

// ---- the rows functions: a batch's samplers, penalties, bias and log-prob records, one workgroup per row of the pass ----
// the slots' token records, their counts and the rows' penalty words (pen_setup)
static int rows_pen_setup(llmk_batch* b) {
    llmk_ctx* c = b->ctx;
    return pen_setup(b->pen, c->cfg.device, c->stream, (size_t)b->n_slots, (size_t)b->seq_len, (size_t)c->V, LLMK_MAX_BATCH);
}
// What the rows of a call ask for: every entry checked (sampler_words, penalty_words; the window against the BATCH's seq_len), nothing
// allocated before every check has passed and nothing at all by a call that needs no record.  The samplers' words go to h_filt; with a
// penalty or a bias on in ANY row (*pen_on), every row's words go to h_pen -- a row with nothing on gets words that adjust nothing.
// nrec: the records the call writes (lp not null).
static int rows_request(llmk_batch* b, int n, const llmk_sampler* samplers, const llmk_penalties* penalties, const llmk_logprobs* lp, size_t nrec,
                        bool* pen_on) {
    llmk_ctx* c = b->ctx;
    *pen_on = false;
    if ((!samplers && penalties) || (lp && !logprob_args_ok(c, lp))) return LLMK_E_ARG;
    for (int i = 0; samplers && i < n; ++i)
        if (!sampler_words(samplers + i, b->h_filt + i)) return LLMK_E_ARG;
    std::vector<llmk_penalty_params> pen(penalties ? (size_t)n : 0);
    for (int i = 0; penalties && i < n; ++i) {
        bool active = false;
        if (!penalty_words(penalties + i, c->V, b->seq_len, &pen[i], &active)) return LLMK_E_ARG;
        *pen_on = *pen_on || active;
    }
    int rc;
    if (*pen_on) {
        if ((rc = rows_pen_setup(b)) != LLMK_OK) return rc;
        memcpy(b->pen.h_pen, pen.data(), (size_t)n * sizeof(llmk_penalty_params));
    }
    if (lp) {
        if ((rc = lp_setup(b->lp, c->cfg.device, c->stream, nrec, *pen_on ? (size_t)b->n_slots * c->V : 0, true)) != LLMK_OK) return rc;
        *b->lp.h_top = (unsigned)lp->top_n;
    }
    return LLMK_OK;
}
// The sampler kernels of one step or one hook call, ENQUEUED: one launch of n workgroups each, workgroup i on row i's logits in d_logits
// by row i's words.  pen: the penalty kernel first (record: it writes the slots' records, else it only reads them), the raw logits
// set aside in front of it when records are asked for; then the filter kernel, which leaves the picks in d_next; greedy: none of the
// two, the picks are `picked` (the classifier's first maxima).  lp: the log-prob kernel on the raw logits and the picks, records to
// d_lp + i * stride + step.  Returns where the picks are.
static hipError_t rows_enqueue(llmk_batch* b, int n, bool sampled, bool pen, bool record, bool lp, int stride, int step, const int** picked) {
    llmk_ctx* c = b->ctx;
    const int* rows = reinterpret_cast<const int*>(b->d_rows.get());
    if (sampled) {
        if (pen) {
            if (lp) HIPRET(hipMemcpyAsync(b->lp.raw, b->d_logits, (size_t)n * c->V * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
            hipLaunchKernelGGL(sample_penalty_rows_kernel, dim3(n), dim3(SP_THREADS), 0, c->stream, b->d_logits, c->V, rows, record ? b->d_tok : nullptr,
                               b->pen.d_pen, b->pen.hist, record ? b->pen.hist : nullptr, b->pen.cnt, b->n_slots, b->seq_len);
            HIPRET(hipGetLastError());
        }
        hipLaunchKernelGGL(sample_filter_rows_kernel, dim3(n), dim3(SF_THREADS), 0, c->stream, b->d_logits, c->V, rows, b->d_filt, b->d_next, b->d_out2);
        HIPRET(hipGetLastError());
        *picked = b->d_next;
    }
    if (lp) {
        hipLaunchKernelGGL(sample_logprob_rows_kernel, dim3(n), dim3(SF_THREADS), 0, c->stream, (sampled && pen) ? b->lp.raw : b->d_logits, c->V, *picked,
                           b->lp.d_top, b->lp.d, stride, step);
        HIPRET(hipGetLastError());
    }
    return hipSuccess;
}
// the parameter words of a call on their way to the device, like rows and tokens
static hipError_t rows_upload_words(llmk_batch* b, int n, bool sampled, bool pen, bool lp) {
    hipStream_t st = b->ctx->stream;
    if (sampled) HIPRET(hipMemcpyAsync(b->d_filt, b->h_filt, (size_t)n * sizeof(llmk_filter_params), hipMemcpyHostToDevice, st));
    if (pen) HIPRET(hipMemcpyAsync(b->pen.d_pen, b->pen.h_pen, (size_t)n * sizeof(llmk_penalty_params), hipMemcpyHostToDevice, st));
    if (lp) HIPRET(hipMemcpyAsync(b->lp.d_top, b->lp.h_top, sizeof(unsigned), hipMemcpyHostToDevice, st));
    return hipSuccess;
}
// llmk_batch_decode and llmk_rows_decode (`who`): the former is the latter without penalties and records
static int rows_decode(llmk_batch* b, const char* who, int n, const int* slots, const int* tokens, const int* pos0, int steps,
                       const llmk_sampler* samplers, const llmk_penalties* penalties, const llmk_logprobs* lp, int* ids_out) {
    if (!b || !ids_out || steps < 1 || !bd_rows_ok(b, n, slots, tokens, pos0, steps)) return LLMK_E_ARG;
    llmk_ctx* c = b->ctx;
    const size_t nids = (size_t)n * steps;
    bool pen = false;
    int rc = rows_request(b, n, samplers, penalties, lp, nids, &pen);
    if (rc) return rc;
    ScPlan sp;
    if ((rc = bd_ready(b, &sp, n)) != LLMK_OK) return rc;
    HIPCHK(b->d_ids.reserve(nids, c->stream));
    HIPCHK(bd_upload_rows(b, n, slots, tokens, pos0));
    HIPCHK(rows_upload_words(b, n, samplers != nullptr, pen, lp != nullptr));
    HIPCHK(hipMemsetAsync(b->d_err, 0, sizeof(unsigned), c->stream));
    const int max_pos0 = *std::max_element(pos0, pos0 + n);
    for (int s = 0; s < steps; ++s) {
        HIPCHK(bd_pass(b, n, max_pos0 + s, samplers != nullptr || lp != nullptr, sp, s));
        // row i's draw: the kernels the verification hooks run, on the row's logits, position (the row words) and words.  The advance
        // runs behind them: the penalty kernel of the next step finds the fed token in d_tok and the new position in d_rows
        const int* picked = reinterpret_cast<const int*>(b->d_out + n);
        HIPCHK(rows_enqueue(b, n, samplers != nullptr, pen, true, lp != nullptr, steps, s, &picked));
        hipLaunchKernelGGL(bd_advance_kernel, dim3(1), dim3(LLMK_MAX_BATCH), 0, c->stream, picked, n, c->V, s, steps, b->d_ids, b->d_tok, b->d_rows, b->d_err);
        HIPCHK(hipGetLastError());
    }
    if (lp) HIPCHK(hipMemcpyAsync(b->lp.h, b->lp.d, nids * sizeof(llmk_logprob_record), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(b->h_err, b->d_err, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(pf_fetch_flag(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (pf_flagged(c)) {
        // The redone call starts from the caller's rows again and finds the state a first call finds: the token records are indexed by
        // position, so it rewrites the very entries this one wrote (as it rewrites the K/V rows), and the counts are all zero again
        // after every launch of the penalty kernel, whatever the logits were.
        static bool told = false;
        return pf_redo(c, who, &told, [&] { return rows_decode(b, who, n, slots, tokens, pos0, steps, samplers, penalties, lp, ids_out); });
    }
    HIPCHK(hipMemcpy(ids_out, b->d_ids, nids * sizeof(int), hipMemcpyDeviceToHost));
    if (*b->h_err) return LLMK_E_NONFINITE;
    if (lp) logprob_deliver(b->lp.h, nids, lp);      // [row][step]
    return LLMK_OK;
}

int llmk_batch_decode(llmk_batch* b, int n, const int* slots, const int* tokens, const int* pos0, int steps, const llmk_sampler* samplers, int* ids_out) {
    return rows_decode(b, "llmk_batch_decode", n, slots, tokens, pos0, steps, samplers, nullptr, nullptr, ids_out);
}
int llmk_rows_decode(llmk_batch* b, int n, const int* slots, const int* tokens, const int* pos0, int steps, const llmk_sampler* samplers,
                     const llmk_penalties* penalties, const llmk_logprobs* logprobs, int* ids_out) {
    return rows_decode(b, "llmk_rows_decode", n, slots, tokens, pos0, steps, samplers, penalties, logprobs, ids_out);
}

// The verification hook of the rows functions: no pass, no K/V; the caller's logits [n][V] take the place of the batch's logits rows,
// the slots' token records are read (positions up to and including pos[i]) and not written
int llmk_rows_sample_logits(llmk_batch* b, int n, const int* slots, const int* pos, const float* logits, const llmk_sampler* samplers,
                            const llmk_penalties* penalties, const llmk_logprobs* logprobs, int* tokens_out, int* kept_out, float* tau_out,
                            float* adjusted_out) {
    if (!b || !logits || !samplers || !tokens_out || !bd_rows_ok(b, n, slots, nullptr, pos, 1, false)) return LLMK_E_ARG;
    llmk_ctx* c = b->ctx;
    int rc = check_ready(c);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->cfg.device));
    bool pen = false;
    if ((rc = rows_request(b, n, samplers, penalties, logprobs, (size_t)n, &pen)) != LLMK_OK) return rc;
    const size_t nv = (size_t)n * c->V * sizeof(float);
    std::vector<unsigned> out2((size_t)2 * n);
    HIPCHK(bd_upload_rows(b, n, slots, nullptr, pos));
    HIPCHK(rows_upload_words(b, n, true, pen, logprobs != nullptr));
    HIPCHK(hipMemcpyAsync(b->d_logits, logits, nv, hipMemcpyHostToDevice, c->stream));
    const int* picked = nullptr;
    HIPCHK(rows_enqueue(b, n, true, pen, false, logprobs != nullptr, 1, 0, &picked));
    HIPCHK(hipMemcpyAsync(tokens_out, picked, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out2.data(), b->d_out2, out2.size() * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    if (adjusted_out) HIPCHK(hipMemcpyAsync(adjusted_out, b->d_logits, nv, hipMemcpyDeviceToHost, c->stream));
    if (logprobs) HIPCHK(hipMemcpyAsync(b->lp.h, b->lp.d, (size_t)n * sizeof(llmk_logprob_record), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; ++i) {
        if (kept_out) kept_out[i] = (int)out2[2 * i];
        if (tau_out) memcpy(tau_out + i, &out2[2 * i + 1], sizeof(float));
    }
    for (int i = 0; i < n; ++i)
        if (tokens_out[i] < 1 || tokens_out[i] > c->V) return LLMK_E_NONFINITE;
    if (logprobs) logprob_deliver(b->lp.h, (size_t)n, logprobs);
    return LLMK_OK;
}

// llmk_set_history / llmk_get_history for one slot of a batch
int llmk_rows_set_history(llmk_batch* b, int slot, const int* tokens, int n, int pos0) {
    if (!b || !tokens || slot < 0 || slot >= b->n_slots || n < 1 || pos0 < 1 || pos0 + n - 1 > b->seq_len) return LLMK_E_ARG;
    for (int i = 0; i < n; ++i)
        if (tokens[i] < 0 || tokens[i] > b->ctx->V) return LLMK_E_ARG;
    { const int rc_ = spec_settle(b->ctx); if (rc_) return rc_; }
    const int rc = rows_pen_setup(b);
    if (rc) return rc;
    hipStream_t st = b->ctx->stream;
    HIPCHK(hipMemcpyAsync(b->pen.hist + (size_t)slot * b->seq_len + (pos0 - 1), tokens, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return LLMK_OK;
}
int llmk_rows_get_history(llmk_batch* b, int slot, int* tokens_out, int n, int pos0) {
    if (!b || !tokens_out || slot < 0 || slot >= b->n_slots || n < 1 || pos0 < 1 || pos0 + n - 1 > b->seq_len) return LLMK_E_ARG;
    { const int rc_ = spec_settle(b->ctx); if (rc_) return rc_; }
    const int rc = rows_pen_setup(b);
    if (rc) return rc;
    hipStream_t st = b->ctx->stream;
    HIPCHK(hipMemcpyAsync(tokens_out, b->pen.hist + (size_t)slot * b->seq_len + (pos0 - 1), (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return LLMK_OK;
}

int llmk_batch_time(llmk_batch* b, int n, int pos, int iters, float* avg_ms) {
    if (!b || !avg_ms || n < 1 || n > b->n_slots || pos < 1 || pos > b->seq_len || iters < 1) return LLMK_E_ARG;
    for (int i = 0; i < n && b->n_attached > 0; ++i)
        if (pos <= b->px->h_first[i]) return LLMK_E_ARG;      // (slots 0..n-1: an attached one's positions 1..P are the prefix)
    llmk_ctx* c = b->ctx;
    ScPlan sp;
    int rc = bd_ready(b, &sp, n);
    if (rc) return rc;
    int slots[LLMK_MAX_BATCH], tokens[LLMK_MAX_BATCH], posv[LLMK_MAX_BATCH];
    for (int i = 0; i < n; ++i) { slots[i] = i; tokens[i] = 1; posv[i] = pos; }
    HIPCHK(bd_upload_rows(b, n, slots, tokens, posv));
    HIPCHK(bd_pass(b, n, pos, false, sp));      // warm-up
    HIPCHK(hipStreamSynchronize(c->stream));
    Event e0, e1;
    HIPCHK(e0.create());
    hipError_t pe = e1.create();
    if (pe == hipSuccess) pe = hipEventRecord(e0, c->stream);
    for (int k = 0; k < iters && pe == hipSuccess; ++k) pe = bd_pass(b, n, pos, false, sp);
    if (pe == hipSuccess) pe = hipEventRecord(e1, c->stream);
    if (pe == hipSuccess) pe = hipStreamSynchronize(c->stream);
    float ms = 0.f;
    if (pe == hipSuccess) pe = hipEventElapsedTime(&ms, e0, e1);
    HIPCHK(hipMemsetAsync(c->pf->flag, 0, sizeof(unsigned), c->stream));      // (token 1 at every row: whatever the range check said is not a call's)
    HIPCHK(hipStreamSynchronize(c->stream));
    if (pe != hipSuccess) return LLMK_E_HIP + (int)pe;
    *avg_ms = ms / (float)iters;
    return LLMK_OK;
}

// ---- spans (batch.h): several consecutive positions of a slot in one pass ----
// spans of a call: distinct slots, lengths and positions in range, at most LLMK_MAX_BATCH rows in all (*rows), ids in range
// (tokens null: llmk_span_time, which feeds token 1)
static bool span_ok(const llmk_batch* b, int n_spans, const llmk_span* spans, const int* tokens, bool fed, int* rows) {
    if (!spans || (fed && !tokens) || n_spans < 1 || n_spans > LLMK_MAX_BATCH) return false;
    bool seen[LLMK_MAX_BATCH] = {};
    int n = 0;
    for (int i = 0; i < n_spans; ++i) {
        const llmk_span& s = spans[i];
        if (s.slot < 0 || s.slot >= b->n_slots || seen[s.slot]) return false;
        seen[s.slot] = true;
        if (s.len < 1 || s.len > LLMK_MAX_BATCH - n) return false;
        if (s.pos0 < 1 || s.pos0 > b->seq_len || s.len - 1 > b->seq_len - s.pos0) return false;
        if (b->n_attached > 0 && s.pos0 <= b->px->h_first[s.slot]) return false;      // an attached slot's positions 1..P are the prefix
        n += s.len;
    }
    for (int i = 0; fed && i < n; ++i)
        if (tokens[i] < 1 || tokens[i] > b->ctx->V) return false;
    *rows = n;
    return true;
}
// what a span pass needs beyond a batch's own, by the first call that needs it: logits rows beyond n_slots; the group table and the
// part states of bd_attn_span_kernel (not with LLMK_SPAN_ATTN=0: the per-row kernels have theirs)
static int span_setup(llmk_batch* b, int rows) {
    llmk_ctx* c = b->ctx;
    if (rows > b->n_slots) {
        const int rc = bd_alloc_rc(b->d_logits.reserve((size_t)LLMK_MAX_BATCH * c->V, c->stream));
        if (rc) return rc;
    }
    if (!b->span_attn || b->sn) return LLMK_OK;
    auto sn = std::make_unique<llmk_batch::Spans>();
    const size_t nb = LLMK_MAX_BATCH, states = nb * c->nkv * 2 * BD_MAX_PARTS * c->kv_mul;
    HIPCHK(sn->d_groups.alloc(nb));
    HIPCHK(sn->h_groups.alloc(nb));
    int rc;
    if ((rc = bd_alloc_rc(sn->d_spo.alloc(states * c->hs))) != LLMK_OK) return rc;
    if ((rc = bd_alloc_rc(sn->d_spml.alloc(states))) != LLMK_OK) return rc;
    HIPCHK(with_head_size(c->hs, [&](auto hs) -> hipError_t {
        constexpr int HS = decltype(hs)::value;
        return with_kv_type(b, [](auto t) -> hipError_t {
            return hipFuncSetAttribute((const void*)BdAttn<HS, decltype(t)>::span, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attn_smem(BD_WAVES, HS));
        });
    }));
    b->sn = std::move(sn);
    return LLMK_OK;
}
// the rows of the spans, in span order, as bd_upload_rows uploads them; then the group table (bd_attn_span_kernel), the way the column
// map goes up.  tokens null: every row feeds token 1.
static hipError_t span_upload(llmk_batch* b, int n_spans, const llmk_span* spans, const int* tokens) {
    int slots[LLMK_MAX_BATCH], pos[LLMK_MAX_BATCH], ones[LLMK_MAX_BATCH], n = 0;
    for (int i = 0; i < n_spans; ++i)
        for (int j = 0; j < spans[i].len; ++j, ++n) { slots[n] = spans[i].slot; pos[n] = spans[i].pos0 + j; ones[n] = 1; }
    HIPRET(bd_upload_rows(b, n, slots, tokens ? tokens : ones, pos));
    if (!b->span_attn) return hipSuccess;
    const int rg = bd_prefix_rg(b->ctx->kv_mul);
    int row = 0, ng = 0;
    for (int i = 0; i < n_spans; row += spans[i++].len)
        for (int j = 0; j < spans[i].len; j += rg) b->sn->h_groups[ng++] = BdGroup{row + j, std::min(rg, spans[i].len - j)};
    b->pass_groups = ng;
    return hipMemcpyAsync(b->sn->d_groups, b->sn->h_groups, (size_t)ng * sizeof(BdGroup), hipMemcpyHostToDevice, b->ctx->stream);
}

int llmk_span_forward(llmk_batch* b, int n_spans, const llmk_span* spans, const int* tokens, int flags, float* logits_out, int* argmax_out) {
    int n = 0;
    if (!b || (!logits_out && !argmax_out) || (flags & ~LLMK_SPAN_LAST) || !span_ok(b, n_spans, spans, tokens, true, &n)) return LLMK_E_ARG;
    if (n == n_spans) {
        // one position per slot: this IS llmk_batch_forward
        int slots[LLMK_MAX_BATCH], pos[LLMK_MAX_BATCH];
        for (int i = 0; i < n; ++i) { slots[i] = spans[i].slot; pos[i] = spans[i].pos0; }
        return llmk_batch_forward(b, n, slots, tokens, pos, logits_out, argmax_out);
    }
    llmk_ctx* c = b->ctx;
    ScPlan sp;
    int rc = bd_ready(b, &sp, n);
    if (rc) return rc;
    if ((rc = span_setup(b, n)) != LLMK_OK) return rc;
    HIPCHK(span_upload(b, n_spans, spans, tokens));
    int max_pos = 0;
    for (int i = 0; i < n_spans; ++i) max_pos = std::max(max_pos, spans[i].pos0 + spans[i].len - 1);
    HIPCHK(bd_pass(b, n, max_pos, logits_out != nullptr, sp));
    HIPCHK(hipMemcpyAsync(b->h_out, b->d_out, (size_t)2 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(pf_fetch_flag(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (pf_flagged(c)) {
        static bool told = false;
        return pf_redo(c, "llmk_span_forward", &told, [&] { return llmk_span_forward(b, n_spans, spans, tokens, flags, logits_out, argmax_out); });
    }
    const int* ids = reinterpret_cast<const int*>(b->h_out + n);
    for (int i = 0; i < n; ++i)
        if (ids[i] < 1 || ids[i] > c->V) return LLMK_E_NONFINITE;
    if (!(flags & LLMK_SPAN_LAST)) {
        if (argmax_out) memcpy(argmax_out, ids, (size_t)n * sizeof(int));
        if (logits_out) HIPCHK(hipMemcpy(logits_out, b->d_logits, (size_t)n * c->V * sizeof(float), hipMemcpyDeviceToHost));
        return LLMK_OK;
    }
    for (int i = 0, last = -1; i < n_spans; ++i) {
        last += spans[i].len;
        if (argmax_out) argmax_out[i] = ids[last];
        if (logits_out) HIPCHK(hipMemcpy(logits_out + (size_t)i * c->V, b->d_logits + (size_t)last * c->V, (size_t)c->V * sizeof(float), hipMemcpyDeviceToHost));
    }
    return LLMK_OK;
}

int llmk_span_time(llmk_batch* b, int n_spans, int len, int pos0, int iters, float* avg_ms) {
    if (!b || !avg_ms || iters < 1 || n_spans < 1 || n_spans > LLMK_MAX_BATCH) return LLMK_E_ARG;
    llmk_span spans[LLMK_MAX_BATCH];
    for (int i = 0; i < n_spans; ++i) spans[i] = llmk_span{i, pos0, len};
    int n = 0;
    if (!span_ok(b, n_spans, spans, nullptr, false, &n)) return LLMK_E_ARG;
    if (len == 1) return llmk_batch_time(b, n_spans, pos0, iters, avg_ms);      // one position per slot: that pass
    llmk_ctx* c = b->ctx;
    ScPlan sp;
    int rc = bd_ready(b, &sp, n);
    if (rc) return rc;
    if ((rc = span_setup(b, n)) != LLMK_OK) return rc;
    HIPCHK(span_upload(b, n_spans, spans, nullptr));
    const int max_pos = pos0 + len - 1;
    HIPCHK(bd_pass(b, n, max_pos, false, sp));      // warm-up
    HIPCHK(hipStreamSynchronize(c->stream));
    Event e0, e1;
    HIPCHK(e0.create());
    hipError_t pe = e1.create();
    if (pe == hipSuccess) pe = hipEventRecord(e0, c->stream);
    for (int k = 0; k < iters && pe == hipSuccess; ++k) pe = bd_pass(b, n, max_pos, false, sp);
    if (pe == hipSuccess) pe = hipEventRecord(e1, c->stream);
    if (pe == hipSuccess) pe = hipStreamSynchronize(c->stream);
    float ms = 0.f;
    if (pe == hipSuccess) pe = hipEventElapsedTime(&ms, e0, e1);
    HIPCHK(hipMemsetAsync(c->pf->flag, 0, sizeof(unsigned), c->stream));      // (token 1 at every row: whatever the range check said is not a call's)
    HIPCHK(hipStreamSynchronize(c->stream));
    if (pe != hipSuccess) return LLMK_E_HIP + (int)pe;
    *avg_ms = ms / (float)iters;
    return LLMK_OK;
}

int llmk_reset(llmk_ctx* c) {
    if (!c) return LLMK_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    { const int rc = spec_settle(c); if (rc) return rc; }
    const size_t kvn = (size_t)c->L * c->S * c->KVl * sizeof(float);
    HIPCHK(hipMemsetAsync(c->d_kc, 0, kvn, c->stream));
    HIPCHK(hipMemsetAsync(c->d_vc, 0, kvn, c->stream));
    HIPCHK(hipMemsetAsync(&c->dev_words()->err, 0, sizeof(unsigned), c->stream));   // the token kernel's sticky error word
    HIPCHK(tk_qsc_clear(c, c->stream));      // a new sequence: no position before it (the q4_0 kernels' scale records, token_kernel.h tk_qsc)
    if (c->pen.hist) {                         // ... and no token fed yet (the record of the penalties; their counts are zero between launches anyway)
        HIPCHK(hipMemsetAsync(c->pen.hist, 0, (size_t)c->S * sizeof(int), c->stream));
        HIPCHK(hipMemsetAsync(c->pen.cnt, 0, (size_t)c->V * sizeof(int), c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->host_words()->err = 0;
    c->h_next->err = 0;
    for (int i = 0; i < 5; ++i) c->times[i] = 0.f;
    return LLMK_OK;
}

int llmk_timings(llmk_ctx* c, float ms[5]) {
    if (!c || !ms) return LLMK_E_ARG;
    for (int i = 0; i < 5; ++i) ms[i] = c->times[i];
    return LLMK_OK;
}

int llmk_time_kernel(llmk_ctx* c, int kernel, int iters, float* avg_ms, double* bytes_per_launch) {
    int rc = check_ready(c);
    if (rc) return rc;
    if (kernel < 0 || kernel > 12 || iters <= 0 || !avg_ms) return LLMK_E_ARG;
    if (kernel == 6 && !c->use_tk) return LLMK_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    if (kernel == 11) {
        // the five per-layer kernels of the multi-kernel path (a tensor-parallel rank's too: without its exchanges) for all L
        // layers as ONE hipGraph, replayed `iters` times: microseconds per LAYER as the token pass pays them -- a dependent
        // kernel boundary inside a graph is ~1 us cheaper than between eager launches, which is what kernels 0..4 time
        if (c->h_tokpos[1] < 1) { c->h_tokpos[0] = 0; c->h_tokpos[1] = 1; }
        HIPCHK(hipMemcpyAsync(c->d_tokpos, c->h_tokpos, 4 * sizeof(int), hipMemcpyHostToDevice, c->stream));
        hipGraph_t g = nullptr;
        hipGraphExec_t ge = nullptr;
        HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        hipError_t e = hipSuccess;
        for (int l = 0; l < c->L && e == hipSuccess; ++l) {
            e = launch_qkv(c, l);
            if (e == hipSuccess) e = launch_attn(c, l);
            if (e == hipSuccess) e = launch_wo(c, l);
            if (e == hipSuccess) e = launch_w13(c, l);
            if (e == hipSuccess) e = launch_w2(c, l);
        }
        const hipError_t e2 = hipStreamEndCapture(c->stream, &g);
        if (e != hipSuccess || e2 != hipSuccess) { if (g) hipGraphDestroy(g); return LLMK_E_HIP + (int)(e != hipSuccess ? e : e2); }
        e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
        hipGraphDestroy(g);
        HIPCHK(e);
        for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipGraphLaunch(ge, c->stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev[6], c->stream);
        for (int i = 0; i < iters && e == hipSuccess; ++i) e = hipGraphLaunch(ge, c->stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev[7], c->stream);
        if (e == hipSuccess) e = hipEventSynchronize(c->ev[7]);
        float ms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev[6], c->ev[7]);
        hipGraphExecDestroy(ge);
        HIPCHK(e);
        *avg_ms = ms / (float)iters / (float)c->L;
        if (bytes_per_launch) {
            double b = 0;
            for (int m : {LLMK_WQKV, LLMK_WO, LLMK_W13, LLMK_W2}) b += (double)c->desc[m].rows * (double)row_bytes_for(c->t[m].type, c->desc[m].K);
            *bytes_per_launch = b;
        }
        return LLMK_OK;
    }
    ScPlan sp{0, 0, 0};
    if (kernel >= 7) {   // the prefill GEMMs at PF_TMAX positions: 7 w1|w3, 8 wqkv, 9 wo, 10 w2 (whatever the workspaces hold: timing only)
        const int pf_step = PF_KSTEP;
        if (c->tp_size != 1 || c->E % pf_step || c->H % pf_step) return LLMK_E_ARG;
        rc = pf_setup(c, true);
        if (rc) return rc;
        if (kernel == 12) {   // llmk_score's classifier GEMM: all its row chunks, without the scoring epilogue (R = 0: this context has no GEMM -- V % 4,
                              // the workspace, or q6_K rows on the f32 instruction)
            sp = sc_plan(c);
            if (sp.R == 0) return LLMK_E_ARG;
        }
        // activations of ordinary size (every float 0x3c3c3c3c = 0.0115): an all-zero workspace would make every workgroup of the f16-instruction
        // GEMM cast its low-end votes (prefill.h pf_low_check: 32k atomics per launch, +16 us) -- a path real activations do not take
        HIPCHK(hipMemsetAsync(c->pf->lane[0].Xs, 0x3c, (size_t)PF_TMAX * c->E * sizeof(float), c->stream));
        HIPCHK(hipMemsetAsync(c->pf->lane[0].HB, 0x3c, (size_t)PF_TMAX * c->H * sizeof(float), c->stream));
    }
    // Successive launches walk the layers so the weight stream never re-hits the 256 MiB Infinity
    // Cache (the classifier has one matrix: its figure is cache-assisted beyond the first launch).
    // NOTE: this overwrites x / caches at h_tokpos' position; call llmk_reset afterwards.
    if (c->h_tokpos[1] < 1) { c->h_tokpos[0] = 0; c->h_tokpos[1] = 1; }
    HIPCHK(hipMemcpyAsync(c->d_tokpos, c->h_tokpos, 4 * sizeof(int), hipMemcpyHostToDevice, c->stream));
    auto one = [&](int i) -> hipError_t {
        int l = i % c->L;
#ifdef LLMK_PF_TRACE
        if (getenv("LLMK_PF_ONE_LAYER")) l = 0;      // debug build: weights from the Infinity Cache instead of HBM
#endif
        if (kernel == 6) {  // whole-token kernel: fresh exchange epochs for every launch
            hipLaunchKernelGGL(bump_serial_kernel, dim3(1), dim3(1), 0, c->stream, c->d_tokpos);
            return launch_token_kernel(c);
        }
        if (kernel == 12) {
            PfEpiArgs e;
            const DevTensor& ct = c->t[LLMK_WCLS];
            for (int k = 0; k < sp.nchunks; ++k) {
                const int r0 = k * sp.R;
                HIPRET(pf_gemm(c, c->pf->lane[0], (const char*)ct.data + (size_t)r0 * ct.row_bytes, (int)ct.row_bytes, c->pf->lane[0].Xs, std::min(sp.R, c->V - r0), c->E,
                               PF_TMAX, &e, ct.type));
            }
            return hipSuccess;
        }
        if (kernel >= 7) {
            PfEpiArgs e;
            const int tid = kernel == 7 ? LLMK_W13 : kernel == 8 ? LLMK_WQKV : kernel == 9 ? LLMK_WO : LLMK_W2;
            const int rows = kernel == 7 ? 2 * c->H : kernel == 8 ? c->E + 2 * c->KV : c->E;
            const char* w = (const char*)c->t[tid].data + (size_t)l * rows * c->t[tid].row_bytes;
            const float* X = kernel == 10 ? c->pf->lane[0].HB : c->pf->lane[0].Xs;
            const int K = kernel == 10 ? c->H : c->E;
            return pf_gemm(c, c->pf->lane[0], w, (int)c->t[tid].row_bytes, X, rows, K, PF_TMAX, &e);
        }
        switch (kernel) {
            case 0: return launch_qkv(c, l);
            case 1: return launch_attn(c, l);
            case 2: return launch_wo(c, l);
            case 3: return launch_w13(c, l);
            case 4: return launch_w2(c, l);
            default: return launch_cls(c);
        }
    };
    for (int i = 0; i < 3; ++i) HIPCHK(one(i));
    HIPCHK(hipEventRecord(c->ev[6], c->stream));
    for (int i = 0; i < iters; ++i) HIPCHK(one(i + 3));
    HIPCHK(hipEventRecord(c->ev[7], c->stream));
    HIPCHK(hipEventSynchronize(c->ev[7]));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
    *avg_ms = ms / (float)iters;
    if (kernel == 6) c->h_tokpos[2] += iters + 3;   // the device-side serial was bumped once per launch: keep the host's in step
                                                     // (exchange epochs must stay unique per serial)
    if (bytes_per_launch) {
        const int tids[13] = {LLMK_WQKV, -1, LLMK_WO, LLMK_W13, LLMK_W2, LLMK_WCLS, -1, LLMK_W13, LLMK_WQKV, LLMK_WO, LLMK_W2, -1, LLMK_WCLS};
        double b = 0;
        if (kernel == 6) {
            double w = 0;
            const int mats[5] = {LLMK_WQKV, LLMK_WO, LLMK_W13, LLMK_W2, LLMK_WCLS};
            for (int m : mats) w += (double)c->desc[m].rows * (c->desc[m].layered ? c->L : 1) * (double)row_bytes_for(c->t[m].type, c->desc[m].K);
            b = w + (2.0 * c->L + 1) * c->E * 4 + c->E * 4 + 2.0 * c->L * c->KV * 4.0 * c->h_tokpos[1] +
                2.0 * c->L * c->KV * 4 + c->V * 4.0;
        } else if (kernel == 1) {
            b = 2.0 * c->KV * 4.0 * c->h_tokpos[1];  // K and V rows 1..pos of one layer
        } else {
            const TensorDesc& d = c->desc[tids[kernel]];
            const int type = c->t[tids[kernel]].type;      // (the q6_K GEMM reads the device rows, padding included)
            b = (double)d.rows * (double)(kernel == 12 && type == LLMK_TYPE_Q6_K ? dev_row_bytes(type, d.K) : row_bytes_for(type, d.K));
        }
        *bytes_per_launch = b;
    }
    return LLMK_OK;
}

// (errors are NEGATIVE, as llmk_path's: the forms are small non-negative numbers).  The answer is that of the batched pass itself --
// pf_shape_ok, not pf_eligible: LLMK_PREFILL=0 sends llmk_score token by token and leaves llmk_batch_* batched (include/llmk.h says so)
int llmk_cls_form(llmk_ctx* c, int rows) {
    if (!c || rows < 1 || rows > LLMK_MAX_BATCH) return -LLMK_E_ARG;
    int rc = check_ready(c);
    if (rc) return -rc;
    if (!pf_shape_ok(c)) return LLMK_CLS_NONE;
    auto setup = [&]() -> int {
        HIPCHK(hipSetDevice(c->cfg.device));
        return pf_setup(c, true);
    };
    if ((rc = setup()) != LLMK_OK) return -rc;
    if (sc_plan(c, rows).R > 0) return LLMK_CLS_GEMM;
    return c->t[LLMK_WCLS].type == LLMK_TYPE_Q6_K ? LLMK_CLS_ROWS : LLMK_CLS_NONE;
}

int llmk_peek(llmk_ctx* c, int which, int layer, int pos, float* out, int n) {
    if (!c || !out || n <= 0) return LLMK_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    { const int rc = spec_settle(c); if (rc) return rc; }
    const float* src = nullptr;
    int len = 0;
    switch (which) {
        case 0: src = c->d_x; len = c->E; break;
        case 1: src = c->d_q; len = c->Eq; break;
        case 2: src = c->d_xb; len = c->Eq; break;
        case 3: src = c->d_hb; len = c->Hl; break;
        case 4:
        case 5:
            if (layer < 0 || layer >= c->L || pos < 1 || pos > c->S) return LLMK_E_ARG;
            src = (which == 4 ? c->d_kc : c->d_vc) + ((size_t)layer * c->S + (pos - 1)) * c->KVl;
            len = c->KVl;
            break;
#ifdef LLMK_PF_TRACE
        case 7:
            if (!c->pf) return LLMK_E_ARG;
            src = c->pf->lane[0].HB; len = PF_TMAX * c->H;
            break;
#endif
        case 8: {  // the q4_0 persistent kernels' per-layer scale records (token_kernel.h tk_qsc): [2 buffers][TK_QSC_LMAX] x {|xb|, |hb|, pos, pos}
            size_t ng;
            src = reinterpret_cast<const float*>(tk_qsc_records(c, &ng));
            if (!src) return LLMK_E_ARG;
            len = (int)(2 * ng);
            break;
        }
        case 6:  // debug: raw trace stamps reinterpret as floats (2 per stamp)
            if (!c->d_trace) return LLMK_E_ARG;
            src = (const float*)c->d_trace.get(); len = TK_NCU * TK_TRACE_N * 2;
            break;
        default: return LLMK_E_ARG;
    }
    if (n > len) return LLMK_E_ARG;
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, src, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return LLMK_OK;
}

int llmk_tp_unique_id(char id_out[128]) {
    if (!id_out) return LLMK_E_ARG;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return LLMK_E_COMM;
    memcpy(id_out, &id, sizeof(id));
    return LLMK_OK;
}

int llmk_tp_init_comm(llmk_ctx* c, const char id_in[128]) {
    if (!c || !id_in || c->comm) return LLMK_E_ARG;
    if (c->p2p) return LLMK_E_STATE;      // llmk_tp_p2p_disable first: a ctx runs ONE kind of collective
    HIPCHK(hipSetDevice(c->cfg.device));
    { const int rc_ = spec_settle(c); if (rc_) return rc_; }
    ncclUniqueId id;
    memcpy(&id, id_in, sizeof(id));
    if (ncclCommInitRank(&c->comm, c->tp_size, id, c->tp_rank) != ncclSuccess) { c->comm = nullptr; return LLMK_E_COMM; }
    return LLMK_OK;
}

// ---- one-shot peer-memory collectives (tp_p2p.h) ----------------------------------------------------------------------
static int tp_inbox_alloc(llmk_ctx* c) {
    if (c->d_inbox) return LLMK_OK;
    if (c->tp_size < 2 || c->tp_size > TP_MAX_RANKS) return LLMK_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    const size_t bytes = tp_inbox_granules(c->tp_size, c->E, c->V) * sizeof(unsigned long long);
    // fine-grained: peers' stores over xGMI and this device's system-scope polls meet in memory, not in a stale L2 line
    HIPCHK(c->d_inbox.alloc_finegrained(bytes / sizeof(unsigned long long)));
    HIPCHK(hipMemset(c->d_inbox, 0, bytes));      // tag 0 is never a valid epoch
    HIPCHK(c->d_tp_bad.alloc(1));
    HIPCHK(hipDeviceSynchronize());
    c->peers.inbox[c->tp_rank] = c->d_inbox;
    // bound of every spin of the exchange kernels in WALL-CLOCK ticks (tp_p2p.h): 20 s unless LLMK_TP_TIMEOUT_MS says otherwise
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->cfg.device) != hipSuccess || khz <= 0) khz = 100000;   // 100 MHz on gfx9
    const long long ms = getenv("LLMK_TP_TIMEOUT_MS") ? atoll(getenv("LLMK_TP_TIMEOUT_MS")) : 20000;
    c->peers.timeout_ticks = (unsigned long long)(ms > 0 ? ms : 20000) * (unsigned long long)khz;
    return LLMK_OK;
}

int llmk_tp_p2p_handle(llmk_ctx* c, char handle_out[64]) {
    if (!c || !handle_out) return LLMK_E_ARG;
    { const int rc_ = spec_settle(c); if (rc_) return rc_; }
    int rc = tp_inbox_alloc(c);
    if (rc) return rc;
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
    hipIpcMemHandle_t h;
    HIPCHK(hipIpcGetMemHandle(&h, c->d_inbox));
    memcpy(handle_out, &h, sizeof(h));
    return LLMK_OK;
}

int llmk_tp_p2p_connect(llmk_ctx* c, const char* handles) {
    if (!c || !handles || c->p2p) return LLMK_E_ARG;
    { const int rc_ = spec_settle(c); if (rc_) return rc_; }
    int rc = tp_inbox_alloc(c);
    if (rc) return rc;
    for (int r = 0; r < c->tp_size; ++r) {
        if (r == c->tp_rank) continue;
        hipIpcMemHandle_t h;
        memcpy(&h, handles + (size_t)r * 64, sizeof(h));
        void* p = nullptr;
        HIPCHK(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
        c->ipc_mapped[r] = p;
        c->peers.inbox[r] = (unsigned long long*)p;
    }
    c->p2p = true;
    return LLMK_OK;
}

int llmk_tp_p2p_connect_local(llmk_ctx* c, llmk_ctx* const* ranks) {
    if (!c || !ranks || c->p2p) return LLMK_E_ARG;
    { const int rc_ = spec_settle(c); if (rc_) return rc_; }
    int rc = tp_inbox_alloc(c);
    if (rc) return rc;
    for (int r = 0; r < c->tp_size; ++r) {
        if (r == c->tp_rank) continue;
        llmk_ctx* o = ranks[r];
        if (!o || o->tp_size != c->tp_size || o->tp_rank != r || o->E != c->E || o->V != c->V) return LLMK_E_ARG;
        rc = tp_inbox_alloc(o);
        if (rc) return rc;
        HIPCHK(hipSetDevice(c->cfg.device));
        if (o->cfg.device != c->cfg.device) {
            const hipError_t e = hipDeviceEnablePeerAccess(o->cfg.device, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return LLMK_E_HIP + (int)e;
            (void)hipGetLastError();
        }
        c->peers.inbox[r] = o->d_inbox;
    }
    c->p2p = true;
    return LLMK_OK;
}

// ---- self-test of the peer-memory collectives ----------------------------------------------------------------------------
// What differs between one GPU and eight is exactly what a 1-GPU box cannot show: peers' system-scope stores landing in
// this rank's fine-grained inbox over xGMI, lazy peer access through the IPC mapping, polls of memory a remote device
// writes.  So every rank proves it on the hardware it runs on BEFORE the first token: `iters` rounds of both all-reduce
// halves and the all-gather on known integers (exact in f32), with the bounded spins of the real kernels.  The host
// collects the ranks' verdicts over its side channel and keeps the peer-memory path only if ALL passed; otherwise every
// rank calls llmk_tp_p2p_disable and the token pass runs over RCCL (llmk_tp_init_comm).
__global__ void tp_selftest_fill_kernel(float* part, float* x, float* logits, int E, int V, int me, int P, int it) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < E) { part[i] = (float)((i * 7 + me * 13 + it) % 1021); x[i] = 0.f; }
    if (i < V) logits[i] = (i / (V / P) == me) ? (float)((i * 3 + it) % 4093) : -1.f;
}
__global__ void tp_selftest_check_kernel(const float* x, const float* logits, int E, int V, int P, int it, unsigned* bad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < E) {
        float want = 0.f;
        for (int r = 0; r < P; ++r) want += (float)((i * 7 + r * 13 + it) % 1021);
        if (x[i] != 2.f * want) atomicAdd(bad, 1u);      // two all-reduces were added into x
    }
    if (i < V && logits[i] != (float)((i * 3 + it) % 4093)) atomicAdd(bad, 1u);
}
static int tp_selftest_run(llmk_ctx* c, int iters, unsigned jseed) {
    if (!c || iters < 1) return LLMK_E_ARG;
    if (!c->p2p) return LLMK_E_COMM;
    HIPCHK(hipSetDevice(c->cfg.device));
    // (no allocation and no hipFree in here: with two ranks in one process a peer's kernel may already be spinning for this rank, and
    // an allocation's fill -- LLMK_POISON -- or a free's device-wide wait queues behind it: round 6's poison runs, 2 x 20 s of timeouts)
    unsigned* d_bad = c->d_tp_bad;
    if (!d_bad) return LLMK_E_COMM;
    HIPCHK(hipMemsetAsync(d_bad, 0, sizeof(unsigned), c->stream));
    const int n = std::max(c->E, c->V);
    int rc = LLMK_OK;
    // The serial that makes the epochs unique is bumped ON THE DEVICE between rounds (the host's copy is brought in step at
    // the end): an async copy out of the pinned h_tokpos per round would read whatever the host loop, running ahead, had
    // already written there -- ranks would disagree on the epochs (seen: 4 rounds pass, 64 time out).
    hipError_t e0 = hipMemcpyAsync(c->d_tokpos, c->h_tokpos, 4 * sizeof(int), hipMemcpyHostToDevice, c->stream);
    if (e0 == hipSuccess) e0 = hipStreamSynchronize(c->stream);
    if (e0 != hipSuccess) rc = LLMK_E_HIP + (int)e0;
    for (int it = 0; it < iters && rc == LLMK_OK; ++it) {
        const unsigned js = jseed ? (jseed + (unsigned)it * 2654435761u) | 1u : 0u;
        hipLaunchKernelGGL(bump_serial_kernel, dim3(1), dim3(1), 0, c->stream, c->d_tokpos);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) {
            hipLaunchKernelGGL(tp_selftest_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->d_part, c->d_x, c->d_logits, c->E,
                               c->V, c->tp_rank, c->tp_size, it);
            e = launch_tp_allreduce_add(c, 0, js);
        }
        if (e == hipSuccess) e = launch_tp_allreduce_add(c, 1, js);
        if (e == hipSuccess) e = launch_tp_allgather(c, js);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(tp_selftest_check_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->d_x, c->d_logits, c->E, c->V,
                               c->tp_size, it, d_bad);
            e = hipGetLastError();
        }
        if (e != hipSuccess) rc = LLMK_E_HIP + (int)e;
        // the jittered rounds are milliseconds each: do not queue thousands of spinning launches ahead of the device
        if (jseed && (it & 63) == 63 && rc == LLMK_OK) { e = hipStreamSynchronize(c->stream); if (e != hipSuccess) rc = LLMK_E_HIP + (int)e; }
    }
    c->h_tokpos[2] += iters;                     // every rank ran the same number of rounds: the serials stay in step
    unsigned bad = 0, err = 0;
    if (rc == LLMK_OK) {
        hipError_t e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(&err, &c->dev_words()->err, sizeof(err), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = LLMK_E_HIP + (int)e;
        else if (err) rc = LLMK_E_TIMEOUT;
        else if (bad) rc = LLMK_E_COMM;
    }
    // leave the ctx as a fresh one: x, the logits and the sticky word
    hipMemsetAsync(c->d_x, 0, (size_t)c->E * sizeof(float), c->stream);
    hipMemsetAsync(c->d_logits, 0, (size_t)c->V * sizeof(float) + offsetof(TkDevWords, cand), c->stream);
    hipStreamSynchronize(c->stream);
    if (rc != LLMK_OK) {
        char what[160];
        fprintf(stderr, "llmk: rank %d of %d: the peer-memory collectives failed their %s (%s, %u mismatches, %s)\n",
                c->tp_rank, c->tp_size, jseed ? "stress run" : "self-test",
                rc == LLMK_E_TIMEOUT ? "a peer's granules never arrived" : rc == LLMK_E_COMM ? "wrong sums" : "HIP error", bad,
                tp_describe_err(c, err, what, sizeof(what)));
    }
    return rc;
}
int llmk_tp_p2p_selftest(llmk_ctx* c, int iters) { return tp_selftest_run(c, iters, 0u); }
// The same rounds with wave-uniform pseudo-random delays before and between the sends and the reads of every exchange
// (tp_p2p.h JIT): ranks and waves drift apart by up to a whole exchange.  Verification only (tests/test_tp_gpu.py).
int llmk_tp_p2p_stress(llmk_ctx* c, int iters, unsigned seed) { return tp_selftest_run(c, iters, seed | 1u); }

// Stop using the peer-memory collectives on this ctx (after a failed self-test on ANY rank): the token pass then needs
// the RCCL communicator (llmk_tp_init_comm).  The inbox stays mapped until llmk_destroy.
int llmk_tp_p2p_disable(llmk_ctx* c) {
    if (!c) return LLMK_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    { const int rc_ = spec_settle(c); if (rc_) return rc_; }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->p2p = false;
    drop_graphs(c);
    return LLMK_OK;
}

int llmk_tp_begin(llmk_ctx* c, int token, int pos) {
    int rc = check_ready(c);
    if (rc) return rc;
    if (token < 1 || token > c->V || pos < 1 || pos > c->S) return LLMK_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    c->h_tokpos[0] = token - 1;
    c->h_tokpos[1] = pos;
    c->h_tokpos[2] += 1;
    HIPCHK(hipMemcpyAsync(c->d_tokpos, c->h_tokpos, 4 * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_embed(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LLMK_OK;
}

int llmk_tp_segment(llmk_ctx* c, int seg, int layer) {
    int rc = check_ready(c);
    if (rc) return rc;
    if (seg < 0 || seg > 2 || layer < 0 || layer >= c->L) return LLMK_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    if (seg == 0) {
        if (layer > 0) HIPCHK(launch_add_partial(c));
        HIPCHK(launch_qkv(c, layer));
        HIPCHK(launch_attn(c, layer));
        HIPCHK(launch_wo(c, layer));
    } else if (seg == 1) {
        HIPCHK(launch_add_partial(c));
        HIPCHK(launch_w13(c, layer));
        HIPCHK(launch_w2(c, layer));
    } else {
        HIPCHK(launch_add_partial(c));
        HIPCHK(launch_cls(c));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return LLMK_OK;
}

int llmk_tp_read_partial(llmk_ctx* c, float* out) {
    if (!c || !out) return LLMK_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    { const int rc_ = spec_settle(c); if (rc_) return rc_; }
    HIPCHK(hipMemcpy(out, c->d_part, (size_t)c->E * sizeof(float), hipMemcpyDeviceToHost));
    return LLMK_OK;
}
int llmk_tp_write_partial(llmk_ctx* c, const float* in) {
    if (!c || !in) return LLMK_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    { const int rc_ = spec_settle(c); if (rc_) return rc_; }
    HIPCHK(hipMemcpy(c->d_part, in, (size_t)c->E * sizeof(float), hipMemcpyHostToDevice));
    return LLMK_OK;
}
int llmk_tp_read_logits(llmk_ctx* c, float* out_slice) {
    if (!c || !out_slice) return LLMK_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    { const int rc_ = spec_settle(c); if (rc_) return rc_; }
    HIPCHK(hipMemcpy(out_slice, c->d_logits + (size_t)c->tp_rank * c->Vl, (size_t)c->Vl * sizeof(float), hipMemcpyDeviceToHost));
    return LLMK_OK;
}

// 64-bit sum of the 32-bit words of a tensor's DEVICE image (this rank's shard, in the device layout): equal images give
// equal sums, so two uploads of the same weights, two contexts, or one context before and after a run can be compared
// without reading gigabytes back (tests: upload determinism, "weights untouched by the token pass").
__global__ void checksum_kernel(const unsigned* __restrict__ w, size_t nwords, unsigned long long* out) {
    unsigned long long t = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += (size_t)gridDim.x * blockDim.x) t += w[i];
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, t);
}
int llmk_tensor_checksum(llmk_ctx* c, int tid, unsigned long long* out) {
    if (!c || !out || tid < 0 || tid >= LLMK_N_TENSORS) return LLMK_E_ARG;
    const TensorDesc& d = c->desc[tid];
    const DevTensor& t = c->t[tid];
    if (!t.data) return LLMK_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    { const int rc_ = spec_settle(c); if (rc_) return rc_; }
    const size_t nwords = (size_t)d.rows * (d.layered ? c->L : 1) * t.row_bytes / 4;
    DevBuf<unsigned long long> d_out;
    HIPCHK(d_out.alloc(1));
    hipError_t e = d_out.zero(c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(checksum_kernel, dim3(1024), dim3(256), 0, c->stream, (const unsigned*)t.data, nwords, d_out.get());
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, sizeof(*out), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? LLMK_OK : LLMK_E_HIP + (int)e;
}

// "E,H,NH,NKV,V,type[+cls];..." of every shape the persistent kernel is instantiated for in THIS build (LLMK_TK_SHAPES)
int llmk_tk_shapes(char* buf, size_t n) {
    if (!buf || n == 0) return LLMK_E_ARG;
    static const char* tn[] = {"f32", "f16", "q4_0"};
    size_t o = 0;
    buf[0] = 0;
    for (int i = 0; i < TK_NSHAPES; ++i) {
        const TkEntry& e = tk_table[i];
        char one[96];
        const int k = snprintf(one, sizeof(one), "%s%d,%d,%d,%d,%d,%s%s", i ? ";" : "", e.E, e.H, e.NH, e.NKV, e.V, tn[e.WT], e.CLS != e.WT ? "+q6_K" : "");
        if (o + (size_t)k + 1 > n) return LLMK_E_SIZE;
        memcpy(buf + o, one, (size_t)k + 1);
        o += (size_t)k;
    }
    return LLMK_OK;
}

int llmk_path(llmk_ctx* c) {
    if (!c) return -LLMK_E_ARG;
    if (c->p2p) return LLMK_PATH_TP_P2P;
    if (c->comm) return LLMK_PATH_TP_RCCL;
    if (c->tp_size > 1) return LLMK_PATH_TP_UNCONNECTED;
    return c->use_tk ? LLMK_PATH_TOKEN_KERNEL : LLMK_PATH_MULTI_KERNEL;
}

int llmk_tp_ranks_seen(llmk_ctx* c) {
    if (!c) return -LLMK_E_ARG;
    if (c->comm) {
        int n = 0;
        if (ncclCommCount(c->comm, &n) != ncclSuccess) return -LLMK_E_COMM;
        return n;                       // what the RCCL communicator itself says
    }
    if (c->p2p) {                       // peers whose inboxes are mapped here (+ this rank)
        int n = 0;
        for (int r = 0; r < c->tp_size; ++r) n += c->peers.inbox[r] != nullptr;
        return n;
    }
    return 1;
}

int llmk_destroy(llmk_ctx* c) {
    if (!c) return LLMK_E_ARG;
    if (c->n_batches > 0) return LLMK_E_STATE;      // its batches go first (llmk_batch_destroy): they run on this context's weights and stream
    hipSetDevice(c->cfg.device);
    if (c->stream) spec_settle(c);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->comm) ncclCommDestroy(c->comm);
    for (int r = 0; r < TP_MAX_RANKS; ++r)
        if (c->ipc_mapped[r]) hipIpcCloseMemHandle(c->ipc_mapped[r]);
    drop_graphs(c);
    // everything else the context holds is owned (owned.h): the buffers and events go before the stream, which is declared first
    delete c;
    return LLMK_OK;
}

}  // extern "C"
