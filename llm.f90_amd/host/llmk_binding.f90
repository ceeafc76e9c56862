! ISO_C_BINDING interface to the llmk C-ABI (include/llmk.h).  One explicit interface per
! exported symbol; constants mirror the header.  This is the whole device boundary of the host:
! the call `logits = transformer(token,pos,s,weights)` (/root/reference/llama2.f90:380) becomes
! `rc = llmk_forward(ctx, token, pos, logits)`.
module llmk_binding
  use iso_c_binding
  implicit none

  integer(c_int), parameter :: LLMK_TYPE_F32 = 0, LLMK_TYPE_F16 = 1, LLMK_TYPE_Q4_0 = 2, LLMK_TYPE_Q6_K = 14
  integer(c_int), parameter :: LLMK_TOKEN_EMBEDDING_TABLE = 0, LLMK_RMS_ATT_WEIGHT = 1, LLMK_RMS_FFN_WEIGHT = 2, &
       LLMK_WQKV = 3, LLMK_WO = 4, LLMK_W13 = 5, LLMK_W2 = 6, LLMK_RMS_FINAL_WEIGHT = 7, LLMK_WCLS = 8
  integer(c_int), parameter :: LLMK_FLAG_NO_GRAPH = 1, LLMK_FLAG_TIMINGS = 2

  type, bind(C) :: llmk_config
     integer(c_int32_t) :: emb_dim, hidden_dim, n_layers, n_heads, n_kv_heads, vocab_size, seq_len
     integer(c_int32_t) :: weight_type, device, flags
  end type llmk_config

  ! the sampler of llmk_forward_sample_ex / llmk_decode_sample_ex: top_k = 0, top_p = 1, min_p = 0 are "off"
  ! positions pos0 .. pos0+len-1 (1-based) of `slot`: a span of llmk_span_forward (include/llmk.h)
  type, bind(C) :: llmk_span
     integer(c_int32_t) :: slot, pos0, len
  end type llmk_span
  integer(c_int), parameter :: LLMK_SPAN_LAST = 1      ! the outputs hold ONE row per span, its last position

  type, bind(C) :: llmk_sampler
     real(c_float) :: temperature
     integer(c_int32_t) :: top_k
     real(c_float) :: top_p, min_p
     integer(c_int64_t) :: seed
  end type llmk_sampler

  ! penalties and logit bias of llmk_forward_sample_pen / llmk_decode_sample_pen: last_n = 0, repeat = 1, frequency = 0,
  ! presence = 0, n_bias = 0 are "off"; bias = c_loc of an array of n_bias llmk_logit_bias (token 1-based), or c_null_ptr
  integer(c_int), parameter :: LLMK_MAX_LOGIT_BIAS = 256
  type, bind(C) :: llmk_logit_bias
     integer(c_int32_t) :: token
     real(c_float) :: bias
  end type llmk_logit_bias
  type, bind(C) :: llmk_penalties
     integer(c_int32_t) :: last_n
     real(c_float) :: repeat, frequency, presence
     type(c_ptr) :: bias
     integer(c_int32_t) :: n_bias
  end type llmk_penalties

  ! the log-prob request of llmk_forward_sample_lp / llmk_decode_sample_lp: top_n in 0 .. LLMK_MAX_TOP_LOGPROBS alternatives per
  ! position; token_logprob = c_loc of n floats or c_null_ptr; top_tokens / top_logprobs = c_loc of n * top_n values (c_null_ptr
  ! at top_n = 0)
  integer(c_int), parameter :: LLMK_MAX_TOP_LOGPROBS = 20
  type, bind(C) :: llmk_logprobs
     integer(c_int32_t) :: top_n
     type(c_ptr) :: token_logprob, top_tokens, top_logprobs
  end type llmk_logprobs

  interface
     integer(c_int) function llmk_create(cfg, ctx) bind(C, name="llmk_create")
       import :: c_int, c_ptr, llmk_config
       type(llmk_config), intent(in) :: cfg
       type(c_ptr), intent(out) :: ctx
     end function
     ! tensor-parallel shard `tp_rank` of `tp_size` (the 70B configuration): llmk_upload is still handed the FULL arrays
     integer(c_int) function llmk_create_tp(cfg, tp_rank, tp_size, ctx) bind(C, name="llmk_create_tp")
       import :: c_int, c_ptr, llmk_config
       type(llmk_config), intent(in) :: cfg
       integer(c_int), value :: tp_rank, tp_size
       type(c_ptr), intent(out) :: ctx
     end function
     integer(c_int) function llmk_tp_unique_id(id_out) bind(C, name="llmk_tp_unique_id")
       import :: c_int, c_char
       character(kind=c_char), intent(out) :: id_out(128)
     end function
     integer(c_int) function llmk_tp_init_comm(ctx, id) bind(C, name="llmk_tp_init_comm")
       import :: c_int, c_ptr, c_char
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(in) :: id(128)
     end function
     integer(c_int) function llmk_tp_p2p_handle(ctx, handle_out) bind(C, name="llmk_tp_p2p_handle")
       import :: c_int, c_ptr, c_char
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(out) :: handle_out(64)
     end function
     integer(c_int) function llmk_tp_p2p_connect(ctx, handles) bind(C, name="llmk_tp_p2p_connect")
       import :: c_int, c_ptr, c_char
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(in) :: handles(*)     ! tp_size * 64 bytes, rank order
     end function
     ! all ranks together, after the connect: 0 = this rank's peer-memory exchanges gave exact sums on this hardware
     integer(c_int) function llmk_tp_p2p_selftest(ctx, iters) bind(C, name="llmk_tp_p2p_selftest")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: iters
     end function
     integer(c_int) function llmk_tp_p2p_disable(ctx) bind(C, name="llmk_tp_p2p_disable")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function
     integer(c_int) function llmk_upload(ctx, tensor_id, host, nbytes, ggml_type) bind(C, name="llmk_upload")
       import :: c_int, c_ptr, c_size_t
       type(c_ptr), value :: ctx
       integer(c_int), value :: tensor_id
       type(c_ptr), value :: host
       integer(c_size_t), value :: nbytes
       integer(c_int), value :: ggml_type
     end function
     integer(c_int) function llmk_upload_rows(ctx, tensor_id, layer, row_offset, rows, host, nbytes, ggml_type) &
          bind(C, name="llmk_upload_rows")
       import :: c_int, c_ptr, c_size_t
       type(c_ptr), value :: ctx
       integer(c_int), value :: tensor_id, layer, row_offset, rows
       type(c_ptr), value :: host
       integer(c_size_t), value :: nbytes
       integer(c_int), value :: ggml_type
     end function
     integer(c_int) function llmk_set_tensor_type(ctx, tensor_id, ggml_type) bind(C, name="llmk_set_tensor_type")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: tensor_id, ggml_type
     end function
     integer(c_int) function llmk_set_rms_eps(ctx, eps) bind(C, name="llmk_set_rms_eps")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: ctx
       real(c_float), value :: eps
     end function
     integer(c_int) function llmk_set_rope_freqs(ctx, freqs, n) bind(C, name="llmk_set_rope_freqs")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: ctx
       real(c_float), intent(in) :: freqs(*)
       integer(c_int), value :: n
     end function
     integer(c_int) function llmk_forward(ctx, token, pos, logits) bind(C, name="llmk_forward")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: ctx
       integer(c_int), value :: token, pos
       real(c_float), intent(out) :: logits(*)
     end function
     integer(c_int) function llmk_prefill(ctx, tokens, n, pos0, logits) bind(C, name="llmk_prefill")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: ctx
       integer(c_int), intent(in) :: tokens(*)
       integer(c_int), value :: n, pos0
       real(c_float), intent(out) :: logits(*)
     end function
     ! targets and the three outputs travel as C addresses (c_loc of a `target` array): each output may be c_null_ptr = not asked for
     integer(c_int) function llmk_score(ctx, tokens, n, pos0, targets, logprob_out, argmax_out, logits_out) bind(C, name="llmk_score")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), intent(in) :: tokens(*)
       integer(c_int), value :: n, pos0
       type(c_ptr), value :: targets, logprob_out, argmax_out, logits_out
     end function
     integer(c_int) function llmk_forward_greedy(ctx, token, pos, next_token) bind(C, name="llmk_forward_greedy")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: token, pos
       integer(c_int), intent(out) :: next_token
     end function
     ! n positions at temperature 0 with the argmax on the device and no host round trip per token; on_token
     ! (void(int index, int token, void* user), or c_null_funptr) is called in order as the ids arrive
     integer(c_int) function llmk_decode_greedy(ctx, token, pos0, n, ids_out, on_token, user) bind(C, name="llmk_decode_greedy")
       import :: c_int, c_ptr, c_funptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: token, pos0, n
       integer(c_int), intent(out) :: ids_out(*)
       type(c_funptr), value :: on_token
       type(c_ptr), value :: user
     end function
     ! the sampling twins of the two above (temperature > 0, the Gumbel-max rule of include/llmk.h): the same draw from the
     ! same logits on every path, keyed by (seed, pos, row)
     integer(c_int) function llmk_forward_sample(ctx, token, pos, temperature, seed, next_token) bind(C, name="llmk_forward_sample")
       import :: c_int, c_ptr, c_float, c_int64_t
       type(c_ptr), value :: ctx
       integer(c_int), value :: token, pos
       real(c_float), value :: temperature
       integer(c_int64_t), value :: seed
       integer(c_int), intent(out) :: next_token
     end function
     integer(c_int) function llmk_decode_sample(ctx, token, pos0, n, temperature, seed, ids_out, on_token, user) &
          bind(C, name="llmk_decode_sample")
       import :: c_int, c_ptr, c_funptr, c_float, c_int64_t
       type(c_ptr), value :: ctx
       integer(c_int), value :: token, pos0, n
       real(c_float), value :: temperature
       integer(c_int64_t), value :: seed
       integer(c_int), intent(out) :: ids_out(*)
       type(c_funptr), value :: on_token
       type(c_ptr), value :: user
     end function
     ! ... and with top-k / top-p / min-p truncation in front of the draw (include/llmk.h; all filters off: the two above)
     integer(c_int) function llmk_forward_sample_ex(ctx, token, pos, sampler, next_token) bind(C, name="llmk_forward_sample_ex")
       import :: c_int, c_ptr, llmk_sampler
       type(c_ptr), value :: ctx
       integer(c_int), value :: token, pos
       type(llmk_sampler), intent(in) :: sampler
       integer(c_int), intent(out) :: next_token
     end function
     integer(c_int) function llmk_decode_sample_ex(ctx, token, pos0, n, sampler, ids_out, on_token, user) &
          bind(C, name="llmk_decode_sample_ex")
       import :: c_int, c_ptr, c_funptr, llmk_sampler
       type(c_ptr), value :: ctx
       integer(c_int), value :: token, pos0, n
       type(llmk_sampler), intent(in) :: sampler
       integer(c_int), intent(out) :: ids_out(*)
       type(c_funptr), value :: on_token
       type(c_ptr), value :: user
     end function
     ! verification hook: the rule on caller-supplied logits (vocab_size floats), no token pass
     integer(c_int) function llmk_sample_logits(ctx, logits, pos, sampler, token_out, kept_out, tau_out) bind(C, name="llmk_sample_logits")
       import :: c_int, c_ptr, c_float, llmk_sampler
       type(c_ptr), value :: ctx
       real(c_float), intent(in) :: logits(*)
       integer(c_int), value :: pos
       type(llmk_sampler), intent(in) :: sampler
       integer(c_int), intent(out) :: token_out, kept_out
       real(c_float), intent(out) :: tau_out
     end function
     ! ... and behind the repetition / frequency / presence penalties and the logit bias (include/llmk.h; nothing on: the _ex two).
     ! The penalties read the context's token record: llmk_set_history records the prompt (tokens fed at pos0 .. pos0+n-1) once,
     ! the two _pen functions record what they are fed from there
     integer(c_int) function llmk_set_history(ctx, tokens, n, pos0) bind(C, name="llmk_set_history")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), intent(in) :: tokens(*)
       integer(c_int), value :: n, pos0
     end function
     integer(c_int) function llmk_get_history(ctx, tokens_out, n, pos0) bind(C, name="llmk_get_history")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), intent(out) :: tokens_out(*)
       integer(c_int), value :: n, pos0
     end function
     ! the same two with the log-prob record of every position (include/llmk.h).  sampler and penalties travel as C addresses:
     ! c_loc of a `target` llmk_sampler / llmk_penalties, or c_null_ptr -- no sampler is the greedy form, no penalties is none
     integer(c_int) function llmk_forward_sample_lp(ctx, token, pos, sampler, penalties, logprobs, next_token) &
          bind(C, name="llmk_forward_sample_lp")
       import :: c_int, c_ptr, llmk_logprobs
       type(c_ptr), value :: ctx
       integer(c_int), value :: token, pos
       type(c_ptr), value :: sampler, penalties
       type(llmk_logprobs), intent(in) :: logprobs
       integer(c_int), intent(out) :: next_token
     end function
     integer(c_int) function llmk_decode_sample_lp(ctx, token, pos0, n, sampler, penalties, logprobs, ids_out, on_token, user) &
          bind(C, name="llmk_decode_sample_lp")
       import :: c_int, c_ptr, c_funptr, llmk_logprobs
       type(c_ptr), value :: ctx
       integer(c_int), value :: token, pos0, n
       type(c_ptr), value :: sampler, penalties
       type(llmk_logprobs), intent(in) :: logprobs
       integer(c_int), intent(out) :: ids_out(*)
       type(c_funptr), value :: on_token
       type(c_ptr), value :: user
     end function
     ! verification hook: the log-prob kernel on caller-supplied logits (vocab_size floats) for `token` (0 = none), no token pass
     integer(c_int) function llmk_logprob_logits(ctx, logits, token, top_n, token_logprob, top_tokens, top_logprobs) &
          bind(C, name="llmk_logprob_logits")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: ctx
       real(c_float), intent(in) :: logits(*)
       integer(c_int), value :: token, top_n
       type(c_ptr), value :: token_logprob, top_tokens, top_logprobs
     end function
     integer(c_int) function llmk_forward_sample_pen(ctx, token, pos, sampler, penalties, next_token) bind(C, name="llmk_forward_sample_pen")
       import :: c_int, c_ptr, llmk_sampler, llmk_penalties
       type(c_ptr), value :: ctx
       integer(c_int), value :: token, pos
       type(llmk_sampler), intent(in) :: sampler
       type(llmk_penalties), intent(in) :: penalties
       integer(c_int), intent(out) :: next_token
     end function
     integer(c_int) function llmk_decode_sample_pen(ctx, token, pos0, n, sampler, penalties, ids_out, on_token, user) &
          bind(C, name="llmk_decode_sample_pen")
       import :: c_int, c_ptr, c_funptr, llmk_sampler, llmk_penalties
       type(c_ptr), value :: ctx
       integer(c_int), value :: token, pos0, n
       type(llmk_sampler), intent(in) :: sampler
       type(llmk_penalties), intent(in) :: penalties
       integer(c_int), intent(out) :: ids_out(*)
       type(c_funptr), value :: on_token
       type(c_ptr), value :: user
     end function
     ! verification hook: the two sampler kernels on caller-supplied logits; adjusted_out = c_loc of vocab_size floats, or c_null_ptr
     integer(c_int) function llmk_sample_logits_pen(ctx, logits, pos, sampler, penalties, token_out, kept_out, tau_out, adjusted_out) &
          bind(C, name="llmk_sample_logits_pen")
       import :: c_int, c_ptr, c_float, llmk_sampler, llmk_penalties
       type(c_ptr), value :: ctx
       real(c_float), intent(in) :: logits(*)
       integer(c_int), value :: pos
       type(llmk_sampler), intent(in) :: sampler
       type(llmk_penalties), intent(in) :: penalties
       integer(c_int), intent(out) :: token_out, kept_out
       real(c_float), intent(out) :: tau_out
       type(c_ptr), value :: adjusted_out
     end function
     ! batched decode (include/llmk.h, DESIGN.md section 3i): `--parallel N`.  samplers = c_loc of a `target` array of n
     ! llmk_sampler, or c_null_ptr = greedy
     integer(c_int) function llmk_batch_create(ctx, n_slots, seq_len, batch) bind(C, name="llmk_batch_create")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: n_slots, seq_len
       type(c_ptr), intent(out) :: batch
     end function
     integer(c_int) function llmk_batch_destroy(batch) bind(C, name="llmk_batch_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: batch
     end function
     integer(c_int) function llmk_batch_fork(batch, slot, n_pos) bind(C, name="llmk_batch_fork")
       import :: c_int, c_ptr
       type(c_ptr), value :: batch
       integer(c_int), value :: slot, n_pos
     end function
     integer(c_int) function llmk_batch_decode(batch, n, slots, tokens, pos0, steps, samplers, ids_out) bind(C, name="llmk_batch_decode")
       import :: c_int, c_ptr
       type(c_ptr), value :: batch
       integer(c_int), value :: n, steps
       integer(c_int), intent(in) :: slots(*), tokens(*), pos0(*)
       type(c_ptr), value :: samplers
       integer(c_int), intent(out) :: ids_out(*)
     end function
     ! a shared prefix (include/llmk.h): `--parallel N --share-prefix`
     integer(c_int) function llmk_prefix_set(batch, n_pos) bind(C, name="llmk_prefix_set")
       import :: c_int, c_ptr
       type(c_ptr), value :: batch
       integer(c_int), value :: n_pos
     end function
     integer(c_int) function llmk_prefix_attach(batch, slot) bind(C, name="llmk_prefix_attach")
       import :: c_int, c_ptr
       type(c_ptr), value :: batch
       integer(c_int), value :: slot
     end function
     integer(c_int) function llmk_prefix_len(batch) bind(C, name="llmk_prefix_len")
       import :: c_int, c_ptr
       type(c_ptr), value :: batch
     end function
     ! a batch whose K/V caches (and shared prefix) have the element type kv_type: 0 = f32 (llmk_batch_create itself), 1 = f16,
     ! 8 = q8_0 (ggml's blocks of 32 int8 quants and an f16 scale; kv_dim a multiple of 32)
     integer(c_int) function llmk_cache_create(ctx, n_slots, seq_len, kv_type, batch) bind(C, name="llmk_cache_create")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: n_slots, seq_len, kv_type
       type(c_ptr), intent(out) :: batch
     end function
     integer(c_int) function llmk_cache_type(batch) bind(C, name="llmk_cache_type")
       import :: c_int, c_ptr
       type(c_ptr), value :: batch
     end function
     integer(c_int) function llmk_cache_bytes(batch, nbytes) bind(C, name="llmk_cache_bytes")
       import :: c_int, c_ptr, c_long_long
       type(c_ptr), value :: batch
       integer(c_long_long), intent(out) :: nbytes
     end function
     integer(c_int) function llmk_cache_peek(batch, which, layer, slot, pos0, n, out) bind(C, name="llmk_cache_peek")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: batch
       integer(c_int), value :: which, layer, slot, pos0, n
       real(c_float), intent(out) :: out(*)
     end function
     ! spans (include/llmk.h): several consecutive positions of a slot in one pass -- `--parallel N --prompts FILE`.  The outputs
     ! travel as C addresses (c_loc of a `target` array, or c_null_ptr: not asked for)
     integer(c_int) function llmk_span_forward(batch, n_spans, spans, tokens, flags, logits_out, argmax_out) &
          bind(C, name="llmk_span_forward")
       import :: c_int, c_ptr, llmk_span
       type(c_ptr), value :: batch
       integer(c_int), value :: n_spans, flags
       type(llmk_span), intent(in) :: spans(*)
       integer(c_int), intent(in) :: tokens(*)
       type(c_ptr), value :: logits_out, argmax_out
     end function
     integer(c_int) function llmk_span_time(batch, n_spans, len, pos0, iters, avg_ms) bind(C, name="llmk_span_time")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: batch
       integer(c_int), value :: n_spans, len, pos0, iters
       real(c_float), intent(out) :: avg_ms
     end function
     ! the rows functions (include/llmk.h): a batch's per-row penalties, bias and log-prob records.  samplers / penalties travel as C
     ! addresses of arrays of n entries (c_loc of a `target` array, or c_null_ptr: greedy / none); logprobs likewise (c_loc of a
     ! `target` llmk_logprobs, or c_null_ptr: no records); the optional outputs of the hook are c_loc or c_null_ptr too
     integer(c_int) function llmk_rows_set_history(batch, slot, tokens, n, pos0) bind(C, name="llmk_rows_set_history")
       import :: c_int, c_ptr
       type(c_ptr), value :: batch
       integer(c_int), value :: slot, n, pos0
       integer(c_int), intent(in) :: tokens(*)
     end function
     integer(c_int) function llmk_rows_get_history(batch, slot, tokens_out, n, pos0) bind(C, name="llmk_rows_get_history")
       import :: c_int, c_ptr
       type(c_ptr), value :: batch
       integer(c_int), value :: slot, n, pos0
       integer(c_int), intent(out) :: tokens_out(*)
     end function
     integer(c_int) function llmk_rows_decode(batch, n, slots, tokens, pos0, steps, samplers, penalties, logprobs, ids_out) &
          bind(C, name="llmk_rows_decode")
       import :: c_int, c_ptr
       type(c_ptr), value :: batch
       integer(c_int), value :: n, steps
       integer(c_int), intent(in) :: slots(*), tokens(*), pos0(*)
       type(c_ptr), value :: samplers, penalties, logprobs
       integer(c_int), intent(out) :: ids_out(*)
     end function
     integer(c_int) function llmk_rows_sample_logits(batch, n, slots, pos, logits, samplers, penalties, logprobs, tokens_out, &
          kept_out, tau_out, adjusted_out) bind(C, name="llmk_rows_sample_logits")
       import :: c_int, c_float, c_ptr
       type(c_ptr), value :: batch
       integer(c_int), value :: n
       integer(c_int), intent(in) :: slots(*), pos(*)
       real(c_float), intent(in) :: logits(*)
       type(c_ptr), value :: samplers, penalties, logprobs
       integer(c_int), intent(out) :: tokens_out(*)
       type(c_ptr), value :: kept_out, tau_out, adjusted_out
     end function
     integer(c_int) function llmk_path(ctx) bind(C, name="llmk_path")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function
     integer(c_int) function llmk_cls_form(ctx, rows) bind(C, name="llmk_cls_form")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: rows
     end function
     integer(c_int) function llmk_tk_shapes(buf, n) bind(C, name="llmk_tk_shapes")
       import :: c_int, c_char, c_size_t
       character(kind=c_char), intent(out) :: buf(*)
       integer(c_size_t), value :: n
     end function
     integer(c_int) function llmk_reset(ctx) bind(C, name="llmk_reset")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function
     integer(c_int) function llmk_timings(ctx, ms) bind(C, name="llmk_timings")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: ctx
       real(c_float), intent(out) :: ms(5)
     end function
     integer(c_int) function llmk_destroy(ctx) bind(C, name="llmk_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function
     type(c_ptr) function llmk_strerror(code) bind(C, name="llmk_strerror")
       import :: c_int, c_ptr
       integer(c_int), value :: code
     end function
     integer(c_int) function llmk_version() bind(C, name="llmk_version")
       import :: c_int
     end function
     ! libc, for the multi-process rendezvous of `llm --ngpu N`
     integer(c_int) function c_getpid() bind(C, name="getpid")
       import :: c_int
     end function
     type(c_ptr) function c_mkdtemp(template) bind(C, name="mkdtemp")       ! creates the directory, mode 0700
       import :: c_ptr, c_char
       character(kind=c_char), intent(inout) :: template(*)
     end function
     integer(c_int) function c_usleep(us) bind(C, name="usleep")
       import :: c_int
       integer(c_int), value :: us
     end function
  end interface

contains

  ! print + stop, the reference's own error convention (read_ggml.f90:122-125)
  subroutine llmk_check(rc, what)
    integer(c_int), intent(in) :: rc
    character(len=*), intent(in) :: what
    character(kind=c_char), pointer :: msg(:)
    integer :: n
    if (rc == 0) return
    call c_f_pointer(llmk_strerror(rc), msg, [256])
    n = 0
    do while (n < 256)
       if (msg(n+1) == c_null_char) exit
       n = n + 1
    end do
    print *, what, ": ", msg(1:n), " (code", rc, ")"
    stop 1
  end subroutine

end module llmk_binding
