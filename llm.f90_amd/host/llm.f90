! `llm` -- the reference's command line (/root/reference/llama2.f90:4-83, :87-411) on top of the
! MI355X decode path.  Same flags and defaults, same console output; the one call that did all the
! work, `logits = transformer(token,pos,s,weights)` (llama2.f90:380), is now
! `llmk_forward(ctx, token, pos, logits)` into hand-written gfx950 kernels (include/llmk.h).
! Model dims come from the GGUF metadata at run time (the reference hard-codes TinyLlama's,
! llama2.f90:102-108).  There is no CPU forward pass in this program.
!
!   ./llm -m model.gguf [-p prompt] [-n tokens] [-t temperature] [-s tokenizer.bin] [-v]
!         [--ak] [-d device] [--device-argmax] [--device-sample] [--prefill] [--timings] [--seed N] [--stream-load] [--ngpu N]
!         [--top-k N] [--top-p P] [--min-p M]
!         [--repeat-penalty R] [--repeat-last-n N] [--presence-penalty P] [--frequency-penalty F] [--logit-bias ID:B]...
!         [--ngpu N [--tp-rccl]] [--gguf-eps] [--gguf-rope-base] [--encode] [--score] [--logprobs N] [--parallel N [--share-prefix] [--kv-f16 | --kv-q8] [--prompts FILE]]
!
! --parallel N (1 .. 128, one GPU): N completions of the prompt decoded TOGETHER (llmk_batch_*, DESIGN.md section 3i) -- the prompt is
! prefilled once and forked into N slots, every pass over the weights serves all N; seeds seed, seed+1, ... at -t > 0 (the filter
! flags apply), greedy at -t 0 (N equal texts).  The completions are printed after generation, each under a line [k], k = 0 .. N-1.
! --share-prefix: the N slots are ATTACHED to one copy of the prompt's K/V rows (llmk_prefix_*) instead of holding a copy each: the
! attention reads the prompt rows once per group of rows, not once per row.
! --kv-f16: the N slots' K/V caches -- and the shared prefix -- hold IEEE halves (llmk_cache_create): half the bytes per pass and per
! slot, the stored values rounded to nearest even and saturated at +-65504.  Refused without --parallel: the context's own cache is f32.
! --kv-q8: they hold ggml's q8_0 blocks instead (32 int8 quants and an f16 scale: 17/64 of the f32 bytes).  About 25 times coarser than
! f16 -- the logits move by about 1e-2 of their largest (include/llmk.h) -- so it is the caller's opt-in; kv_dim must be a multiple of 32.
! Refused without --parallel and together with --kv-f16 (a batch has one cache type).
! --prompts FILE: line j (0-based) of FILE is slot j's OWN prompt (fewer than N lines is an error).  The prompts are ingested through
! the batch itself -- llmk_span_forward, the slots' chunks packed into passes of at most 128 rows -- and the N completions then run
! together from their own positions.  Refused with -p and with --share-prefix (there is no common prompt).
!
! --ngpu N (the 70B configuration, SURVEY.md section 8e): this process becomes rank 0 of N, starts N-1 copies of itself
! (one process per GPU, devices d..d+N-1), every rank loads the file and keeps its shard, the ranks meet through a
! scratch directory (64-byte inbox handles for the one-shot peer-memory collectives, or the RCCL unique id with
! --tp-rccl) and run the same generation loop in lock step; only rank 0 prints.
module arg_parse
  implicit none

  type args
     real :: temperature
     character(:), allocatable :: model_file
     character(:), allocatable :: prompt
     character(:), allocatable :: tokenizer
     logical :: verbose, ak
     logical :: verbose_ext       ! extension: --vx adds this loader's own lines to -v (the matrices' ggml type, streaming)
     integer :: n
     integer :: device            ! extension: HIP device ordinal
     logical :: device_argmax     ! extension: greedy pick on the GPU (SURVEY.md 8f rank 1)
     logical :: device_sample     ! extension: temperature sampling on the GPU (-t > 0; the Gumbel-max rule of include/llmk.h)
     integer :: top_k             ! extension: truncated sampling on the GPU (llmk_decode_sample_ex); any of the three with -t > 0
     real :: top_p, min_p         !   selects the device sampler.  0, 1, 0 = off
     real :: repeat_penalty       ! extension: llama.cpp's penalties over the last repeat_last_n tokens (-1 = the whole context) and
     integer :: repeat_last_n     !   --logit-bias ID:B (repeatable; ID 1-based as --encode prints it, B may be -inf), all in the device
     real :: presence_penalty, frequency_penalty   ! sampler (llmk_decode_sample_pen); any of them with -t > 0 selects it.  1, 64, 0, 0 = off
     integer :: n_bias
     integer :: bias_id(256)      ! (LLMK_MAX_LOGIT_BIAS entries)
     real :: bias_val(256)
     logical :: prefill           ! extension: the prompt goes through the model as ONE batched pass (llmk_prefill)
     logical :: stream_load       ! extension: matrices go from the file to the device tensor by tensor (always with --ngpu)
     logical :: timings           ! extension: fill the five "Timings" lines from hipEvent section timers (slow path)
     integer :: seed              ! extension: >= 0 seeds the sampler (the reference's is unseeded, llama2.f90:433)
     integer :: ngpu              ! extension: tensor-parallel ranks, one process per GPU
     integer :: tp_rank           ! (internal) rank of a worker started by `--ngpu`
     character(:), allocatable :: tp_dir   ! (internal) rendezvous directory
     logical :: tp_rccl           ! extension: RCCL ring collectives instead of the one-shot peer-memory ones
     logical :: gguf_eps, gguf_rope_base   ! extension: honour the file's rms epsilon / RoPE base (the reference hard-codes
                                           ! 1e-5 and 10000, llama2.f90:454,545)
     logical :: encode_only       ! extension: print the prompt's 1-based token ids (bpe_encode) and stop -- no device needed
     logical :: share_prefix      ! extension: --share-prefix: the --parallel slots share ONE copy of the prompt's K/V rows (llmk_prefix_*)
     logical :: kv_q8             ! extension: --kv-q8: they are q8_0 blocks (llmk_cache_create with LLMK_TYPE_Q8_0)
     logical :: kv_f16            ! extension: --kv-f16: the --parallel slots' K/V caches and the shared prefix are f16 (llmk_cache_create)
     character(:), allocatable :: prompts_file   ! extension: --prompts FILE: one prompt per --parallel slot, a line each (llmk_span_*)
     integer :: parallel          ! extension: --parallel N (0 = off): N completions decoded together on one GPU (llmk_batch_*)
     integer :: logprobs          ! extension: --logprobs N (0 .. 20): the log-prob of every generated token and its N most likely
                                  ! alternatives, from the device (llmk_*_sample_lp); -1 = off
     logical :: score             ! extension: score the prompt instead of continuing it (llmk_score): log-prob per token, perplexity
  end type args

contains

  subroutine parse_args(a)
    type(args), intent(out) :: a
    integer :: i, nargs
    character(len=1024) :: opt, val

    a%temperature = 0               ! defaults: llama2.f90:26-32
    a%model_file = "stories15M.bin"
    a%prompt = ""
    a%tokenizer = ""
    a%verbose = .false.
    a%verbose_ext = .false.
    a%ak = .false.
    a%n = 256
    a%device = 0
    a%device_argmax = .false.
    a%device_sample = .false.
    a%top_k = 0
    a%top_p = 1
    a%min_p = 0
    a%repeat_penalty = 1
    a%repeat_last_n = 64
    a%presence_penalty = 0
    a%frequency_penalty = 0
    a%n_bias = 0
    a%prefill = .false.
    a%stream_load = .false.
    a%timings = .false.
    a%seed = -1
    a%ngpu = 1
    a%tp_rank = 0
    a%tp_dir = ""
    a%tp_rccl = .false.
    a%gguf_eps = .false.
    a%gguf_rope_base = .false.
    a%encode_only = .false.
    a%score = .false.
    a%logprobs = -1
    a%parallel = 0
    a%share_prefix = .false.
    a%kv_f16 = .false.
    a%kv_q8 = .false.
    a%prompts_file = ""

    nargs = command_argument_count()
    i = 1
    do while (i <= nargs)
       call get_command_argument(i, opt)
       val = ""
       if (i < nargs) call get_command_argument(i + 1, val)
       select case (trim(opt))
       case ("-m", "--model");       a%model_file = trim(val); i = i + 2
       case ("-p", "--prompt");      a%prompt = trim(val);     i = i + 2
       case ("-s", "--tokenizer");   a%tokenizer = trim(val);  i = i + 2
       case ("-t", "--temperature"); read (val, *) a%temperature; i = i + 2
       case ("-n", "--num_tokens");  read (val, *) a%n;           i = i + 2
       case ("-d", "--device");      read (val, *) a%device;      i = i + 2
       case ("-v", "--verbose");     a%verbose = .true.;       i = i + 1
       case ("--vx");                a%verbose = .true.; a%verbose_ext = .true.; i = i + 1
       case ("--ak");                a%ak = .true.;            i = i + 1
       case ("--device-argmax");     a%device_argmax = .true.; i = i + 1
       case ("--device-sample");     a%device_sample = .true.; i = i + 1
       case ("--top-k");             read (val, *) a%top_k;       i = i + 2
       case ("--top-p");             read (val, *) a%top_p;       i = i + 2
       case ("--min-p");             read (val, *) a%min_p;       i = i + 2
       case ("--repeat-penalty");    read (val, *) a%repeat_penalty;    i = i + 2
       case ("--repeat-last-n");     read (val, *) a%repeat_last_n;     i = i + 2
       case ("--presence-penalty");  read (val, *) a%presence_penalty;  i = i + 2
       case ("--frequency-penalty"); read (val, *) a%frequency_penalty; i = i + 2
       case ("--logit-bias");        call parse_bias(a, trim(val));     i = i + 2
       case ("--prefill");           a%prefill = .true.;       i = i + 1
       case ("--stream-load");       a%stream_load = .true.;   i = i + 1
       case ("--timings");           a%timings = .true.;       i = i + 1
       case ("--seed");              read (val, *) a%seed;        i = i + 2
       case ("--ngpu");              read (val, *) a%ngpu;        i = i + 2
       case ("--tp-rank");           read (val, *) a%tp_rank;     i = i + 2
       case ("--tp-dir");            a%tp_dir = trim(val);     i = i + 2
       case ("--tp-rccl");           a%tp_rccl = .true.;       i = i + 1
       case ("--gguf-eps");          a%gguf_eps = .true.;      i = i + 1
       case ("--gguf-rope-base");    a%gguf_rope_base = .true.; i = i + 1
       case ("--encode");            a%encode_only = .true.;   i = i + 1
       case ("--score");             a%score = .true.;         i = i + 1
       case ("--share-prefix");      a%share_prefix = .true.;  i = i + 1
       case ("--kv-f16");            a%kv_f16 = .true.;        i = i + 1
       case ("--kv-q8");             a%kv_q8 = .true.;         i = i + 1
       case ("--prompts");           a%prompts_file = trim(val); i = i + 2
       case ("--parallel")
          read (val, *) a%parallel
          if (a%parallel < 1 .or. a%parallel > 128) then
             print *, "--parallel takes N in 1 .. 128"
             stop 1
          end if
          i = i + 2
       case ("--logprobs")
          read (val, *) a%logprobs
          if (a%logprobs < 0 .or. a%logprobs > 20) then
             print *, "--logprobs takes N in 0 .. 20"
             stop 1
          end if
          i = i + 2
       case default
          print *, "Unrecognized option:", trim(opt)
          stop
       end select
    end do
  end subroutine parse_args

  ! --logit-bias ID:B -- B a number, or -inf (also -infinity) to ban the token
  subroutine parse_bias(a, val)
    use, intrinsic :: ieee_arithmetic, only: ieee_value, ieee_negative_inf
    type(args), intent(inout) :: a
    character(len=*), intent(in) :: val
    integer :: k, ios
    k = index(val, ":")
    ios = 1
    if (k > 1 .and. k < len(val) .and. a%n_bias < size(a%bias_id)) then
       a%n_bias = a%n_bias + 1
       read (val(1:k - 1), *, iostat=ios) a%bias_id(a%n_bias)
       if (ios == 0) then
          select case (val(k + 1:))
          case ("-inf", "-Inf", "-INF", "-infinity", "-Infinity")
             a%bias_val(a%n_bias) = ieee_value(1.0, ieee_negative_inf)
          case default
             read (val(k + 1:), *, iostat=ios) a%bias_val(a%n_bias)
          end select
       end if
    end if
    if (ios /= 0) then
       print *, "--logit-bias takes ID:B (at most 256 of them; B a number or -inf):", val
       stop 1
    end if
  end subroutine parse_bias

end module arg_parse


! The sink stream_ggml_weights hands its tensors to (read_ggml's tensor_sink): straight to the device context.
module device_sink
  use iso_c_binding
  use llmk_binding
  implicit none
  type(c_ptr) :: sink_ctx = c_null_ptr
contains
  subroutine upload_sink(tensor_id, layer, row_offset, rows, host, nbytes, ggml_type)
    integer, intent(in) :: tensor_id, layer, row_offset, rows, ggml_type
    type(c_ptr), intent(in) :: host
    integer(c_size_t), intent(in) :: nbytes
    call llmk_check(llmk_upload_rows(sink_ctx, int(tensor_id, c_int), int(layer, c_int), int(row_offset, c_int), int(rows, c_int), &
         host, nbytes, int(ggml_type, c_int)), "llmk_upload_rows")
  end subroutine
end module device_sink


! Tokens of llmk_decode_greedy reach the terminal as they are resolved, like the reference's own loop prints them
! (llama2.f90:396): the C-ABI calls ts_on_token from the calling thread, in order.
module token_stream
  use iso_c_binding
  implicit none
  character(:), dimension(:), allocatable :: ts_vocab
  integer(4), allocatable :: ts_len(:)
  logical :: ts_print = .true.
  integer(8) :: ts_first = 0            ! the host's clock_ticks() at the first streamed token (0: none yet)
contains
  subroutine ts_on_token(idx, tok, user) bind(C)
    integer(c_int), value :: idx, tok
    type(c_ptr), value :: user
    if (ts_print) write (*, fmt="(A)", advance="no") ts_vocab(tok)(1:ts_len(tok))
    if (ts_first == 0) call system_clock(ts_first)        ! the same clock as clock_ticks()
  end subroutine
end module token_stream


program llm
  use iso_c_binding
  use token_stream
  use device_sink
  use precision_module
  use weight_module
  use arg_parse
  use read_ggml, only: load_ggml, stream_ggml_weights, verbose_ext
  use ak_loader, only: load_ak
  use llmk_binding
  implicit none

  type(args) :: opts
  type(TransformerWeights), target :: weights
  type(Config) :: conf
  type(RunState) :: s
  type(llmk_config) :: kcfg
  type(c_ptr) :: ctx
  real(kind=wp), allocatable, target :: logits(:)
  real(kind=wp), allocatable :: scores(:), freqs(:), probs(:)
  character(:), dimension(:), allocatable :: vocab
  integer(4), allocatable :: vocab_len(:)
  integer, allocatable :: prompt_tokens(:)
  integer(c_int), allocatable :: batch(:)
  integer(c_int), allocatable :: stream_ids(:)
  integer :: pos0, k, loop_end
  integer :: seq_len, pos, token, next_tok, l, hs, j, max_len
  integer(c_int) :: flags, rc
  integer(8) :: t_start, t_end                      ! clock_ticks(): see elapsed_ms
  real(kind=wp) :: dt_ms
  real(c_float) :: ktimes(5)
  logical :: lead                                   ! this rank prints (rank 0, or the only process)
  integer, allocatable :: hash_tab(:)               ! open-addressing index over vocab (lookup)
  integer :: hash_mask
  real(kind=wp) :: rope_base
  logical :: dsample                                ! --device-sample in its case: -t > 0 on one GPU
  integer(c_int64_t) :: dseed                       ! its seed: --seed N, or the clock's
  logical :: filtered                               ! --top-k / --top-p / --min-p given
  logical :: penalised                              ! a penalty or a --logit-bias given: llmk_*_sample_pen
  type(llmk_penalties) :: pens
  type(llmk_logit_bias), allocatable, target :: bias_list(:)
  integer(c_int), allocatable :: hist_tokens(:)
  type(llmk_sampler) :: sampler
  integer(c_int) :: dnext
  integer(c_int), allocatable, target :: sc_targets(:)   ! --score: the prompt's tokens, each the target of the position before it
  real(c_float), allocatable, target :: sc_logprob(:)
  real(kind=wp) :: sc_sum
  logical :: lp_on                                  ! --logprobs N on one GPU: the device consumer with the log-prob record
  type(llmk_sampler), target :: lp_sampler
  type(llmk_penalties), target :: lp_pens
  type(c_ptr) :: lp_sp, lp_pn                       ! their addresses, or c_null_ptr (greedy form; no penalties)
  integer(c_int), allocatable :: lp_ids(:)          ! the generated tokens, in order
  real(c_float), allocatable, target :: lp_token(:), lp_top(:)
  integer(c_int32_t), allocatable, target :: lp_top_ids(:)
  integer :: lp_n, lp_w
  integer(c_long_long) :: kv_bytes                   ! --vx with --parallel: the device bytes of the batch's K/V caches
  type(c_ptr) :: pbatch                             ! --parallel N: the batch, its rows and samplers, the ids [row][step]
  integer(c_int), allocatable :: par_slots(:), par_tokens(:), par_pos(:), par_ids(:)
  type(llmk_sampler), allocatable, target :: par_samplers(:)
  type(c_ptr) :: par_sp
  integer :: par_steps
  integer, allocatable :: par_k(:), par_fed(:)      ! --prompts: positions slot j's prompt fills (BOS + its first k-1 tokens); ingested so far
  integer(c_int), allocatable :: par_first(:)       ! ... and the token each slot feeds at position k_j + 1
  type(llmk_span), allocatable :: par_spans(:)
  integer(c_int), allocatable :: par_feed(:)        ! the tokens of one ingest pass, [row]
  integer(c_int), allocatable :: par_seq(:)         ! what the slots feed at their positions 1 .. k_j, slot after slot ...
  integer, allocatable :: par_off(:)                ! ... slot j's at par_seq(par_off(j) + 1 : par_off(j) + par_k(j))
  integer(c_int), allocatable, target :: par_am(:)  ! an ingest pass's first maxima, one per span (not used: the decode feeds the prompt's last token)
  integer :: par_passes, n_sp, n_rows, take

  call parse_args(opts)
  ! --parallel N: what a batch does not do is said and stops here (include/llmk.h: penalties, logit bias and log-prob records are out
  ! of scope for a batch; a batch lives on one GPU; --score continues nothing)
  if (opts%parallel > 0) then
     if (opts%ngpu > 1) then
        print *, "--parallel: the completions are decoded together on one GPU (no tensor-parallel batches): drop --ngpu"
        stop 1
     end if
     if (opts%score) then
        print *, "--parallel: --score scores the prompt and continues nothing: drop one of the two"
        stop 1
     end if
     if (opts%logprobs >= 0) then
        print *, "--parallel: --logprobs is not available for completions decoded together (llmk_batch_decode keeps no log-prob records)"
        stop 1
     end if
     if (opts%n_bias > 0) then
        print *, "--parallel: --logit-bias is not available for completions decoded together (llmk_batch_decode applies no logit bias)"
        stop 1
     end if
     if (opts%repeat_penalty /= 1 .or. opts%presence_penalty /= 0 .or. opts%frequency_penalty /= 0) then
        print *, "--parallel: the penalties are not available for completions decoded together (llmk_batch_decode applies none)"
        stop 1
     end if
  end if
  if (opts%share_prefix .and. opts%parallel == 0) then
     print *, "--share-prefix: nothing to share without --parallel N"
     stop 1
  end if
  if (opts%kv_f16 .and. opts%parallel == 0) then
     print *, "--kv-f16: only the K/V caches of --parallel N can be f16 (the context's own cache stays f32)"
     stop 1
  end if
  if (opts%kv_q8 .and. opts%parallel == 0) then
     print *, "--kv-q8: only the K/V caches of --parallel N can be q8_0 (the context's own cache stays f32)"
     stop 1
  end if
  if (opts%kv_q8 .and. opts%kv_f16) then
     print *, "--kv-q8: a batch's K/V caches have one type: drop --kv-f16 or --kv-q8"
     stop 1
  end if
  if (opts%prompts_file /= "") then
     if (opts%parallel == 0) then
        print *, "--prompts: one prompt per slot needs the slots: add --parallel N"
        stop 1
     end if
     if (opts%prompt /= "") then
        print *, "--prompts: every slot takes its own prompt from the file: drop -p"
        stop 1
     end if
     if (opts%share_prefix) then
        print *, "--prompts: own prompts leave no common prefix to share: drop --share-prefix"
        stop 1
     end if
  end if
  lead = opts%tp_rank == 0
  if (opts%ngpu > 1) call tp_launch_workers()
  if (opts%ak) then
     ! llama2.c flat format: no tokenizer inside, `-s tokenizer.bin` is required (llama2.f90:160-356)
     call load_ak(opts%model_file, weights, conf, opts%verbose)
     if (opts%tokenizer == "") then
        print *, "--ak needs a tokenizer file: -s tokenizer.bin"
        stop 1
     end if
  else
     ! --ngpu N (and --stream-load): the matrices stay in the file until the device context exists, then each rank streams
     ! the rows of its own shard to its GPU -- no rank ever holds the model, or even a layer, in host memory
     if (opts%ngpu > 1) opts%stream_load = .true.
     verbose_ext = opts%verbose_ext
     call load_ggml(opts%model_file, weights, conf, vocab, scores, vocab_len, opts%verbose .and. lead, defer=opts%stream_load)
  end if
  if (opts%verbose .and. lead) print *, "Loaded weights"
  if (opts%tokenizer /= "") call read_tokenizer_bin(opts%tokenizer)
  max_len = maxval(vocab_len)
  call build_lookup()
  if (opts%encode_only) then                        ! the tokenizer alone (llama2.f90:372): ids on one line, no device
     prompt_tokens = bpe_encode(opts%prompt)
     print '(*(I0,1X))', prompt_tokens
     stop
  end if
  if (opts%seed >= 0) call seed_sampler(opts%seed)

  ! ---- device context + one-time weight upload (the host arrays are not needed afterwards) -----
  ! The reference's five section timers (llama2.f90:538-638) need an event pair and a sync per section, which rules out
  ! the persistent token kernel and the hipGraph: they are opt-in (--timings) so that `-v`, like the reference's, only
  ! adds prints and the tokens/second line always describes the fast path.  Without --timings the five lines print 0.
  flags = 0
  if (opts%timings) flags = LLMK_FLAG_TIMINGS
  kcfg = llmk_config(conf%emb_dim, conf%hidden_dim, conf%n_layers, conf%n_heads, conf%n_kv_heads, &
                     conf%vocab_size, conf%seq_len, weights%wtype, tp_device(), flags)
  if (opts%ngpu > 1) then
     call llmk_check(llmk_create_tp(kcfg, int(opts%tp_rank, c_int), int(opts%ngpu, c_int), ctx), "llmk_create_tp")
  else
     call llmk_check(llmk_create(kcfg, ctx), "llmk_create")
  end if
  if (weights%wcls_type /= weights%wtype) &
       call llmk_check(llmk_set_tensor_type(ctx, LLMK_WCLS, int(weights%wcls_type, c_int)), "llmk_set_tensor_type")
  if (opts%stream_load .and. .not. opts%ak) then
     sink_ctx = ctx
     call stream_ggml_weights(upload_sink, weights, conf, opts%tp_rank, max(opts%ngpu, 1), opts%verbose .and. lead)
  else
     call upload_weights()
  end if
  if (opts%ngpu > 1) call tp_connect()
  if (opts%gguf_eps .and. conf%rms_eps > 0) call llmk_check(llmk_set_rms_eps(ctx, conf%rms_eps), "llmk_set_rms_eps")

  ! RoPE frequencies with the reference's own expression (llama2.f90:544-545): for 1-based odd i,
  ! head_dim = mod(i,head_size) = 1,3,5,...; freq = 1/10000**(head_dim/head_size)
  hs = conf%emb_dim / conf%n_heads
  allocate(freqs(hs / 2))
  rope_base = 10000.0
  if (opts%gguf_rope_base .and. conf%rope_freq_base > 0) rope_base = conf%rope_freq_base
  do j = 1, hs / 2
     freqs(j) = 1.0 / (rope_base ** (real(2*j - 1, kind=wp) / hs))
  end do
  call llmk_check(llmk_set_rope_freqs(ctx, freqs, int(hs / 2, c_int)), "llmk_set_rope_freqs")
  ! which of the two implementations of the pass this shape and weight type get (include/llmk.h llmk_path): the persistent
  ! whole-token kernel exists for the compiled-in shapes only (the reference's dims are compile-time too, llama2.f90:102-108);
  ! every other model runs -- correctly, at roughly two thirds of the rate -- on five launches per layer.  Said under --vx.
  if (opts%verbose_ext .and. lead) then
     select case (llmk_path(ctx))
     case (1); print *, "device path: persistent whole-token kernel"
     case (2); print *, "device path: tensor-parallel, one-shot peer-memory collectives"
     case (3); print *, "device path: tensor-parallel, RCCL collectives"
     case default; print *, "device path: five kernels per layer (no persistent kernel is instantiated for this shape and weight type)"
     end select
     ! ... and for which shapes this build of libllmk.so has one (make TK_SHAPES="E,H,NH,NKV,V,WT ..." adds more; the reference's
     ! own dims are seven compile-time parameters, llama2.f90:102-108)
     block
       character(kind=c_char) :: sbuf(4096)
       character(len=4096) :: stxt
       integer :: k
       if (llmk_tk_shapes(sbuf, int(size(sbuf), c_size_t)) == 0) then
          stxt = ""
          do k = 1, size(sbuf)
             if (sbuf(k) == c_null_char) exit
             stxt(k:k) = sbuf(k)
          end do
          print *, "persistent kernel built for (E,H,heads,kv heads,V,type): ", trim(stxt)
       end if
     end block
  end if

  allocate(logits(conf%vocab_size), probs(conf%vocab_size))
  s%times = 0

  seq_len = conf%seq_len
  if (opts%n <= seq_len) then                        ! llama2.f90:363-368
     seq_len = opts%n
  else if (lead) then
     print *, opts%n, "greater than maxinum squence length"
     print *, "set to", seq_len
  end if

  prompt_tokens = bpe_encode(opts%prompt)

  ! --score: the prompt is scored, not continued -- positions 1 .. k hold BOS and the first k-1 prompt tokens, the target of
  ! position i is prompt token i; classifier and log-softmax of all k positions run on the device in the one call (llmk_score)
  if (opts%score) then
     k = size(prompt_tokens)
     if (k < 1) then
        print *, "--score needs a prompt of at least one token (-p)"
        stop 1
     end if
     if (k > conf%seq_len .or. opts%ngpu > 1) then
        print *, "--score: the prompt must fit the context (", conf%seq_len, "positions ) on one GPU"
        stop 1
     end if
     allocate(batch(k), sc_targets(k), sc_logprob(k))
     batch(1) = 2
     batch(2:) = int(prompt_tokens(1:k - 1), c_int)
     sc_targets = int(prompt_tokens, c_int)
     t_start = clock_ticks()
     call llmk_check(llmk_score(ctx, batch, int(k, c_int), 1_c_int, c_loc(sc_targets), c_loc(sc_logprob), c_null_ptr, c_null_ptr), &
          "llmk_score")
     t_end = clock_ticks()
     dt_ms = elapsed_ms(t_start, t_end)
     sc_sum = 0
     do pos = 1, k
        print '(I0,1X,I0,1X,ES15.8)', pos, prompt_tokens(pos), sc_logprob(pos)
        sc_sum = sc_sum + sc_logprob(pos)
     end do
     print '(A,1X,I0)', "tokens", k
     print '(A,1X,ES15.8)', "sum logprob", sc_sum
     print '(A,1X,ES15.8)', "perplexity", exp(-sc_sum / k)
     print *, 1000 * k / dt_ms, "positions/second"
     rc = llmk_destroy(ctx)
     stop
  end if

  ! --parallel N: positions 1 .. k (BOS and the first k-1 prompt tokens) are prefilled ONCE on the context and forked into N slots;
  ! the last prompt token (BOS without a prompt) is fed to all N rows at position k+1 and llmk_batch_decode runs positions
  ! k+1 .. seq_len for all of them, every id drawn on the device: row i by the sampler (temperature, filters, seed + i), or the first
  ! maximum at -t 0.  Nothing is printed before the call returns; then the completions, one after another
  if (opts%parallel > 0) then
     k = size(prompt_tokens)
     if (opts%prompts_file /= "") call read_prompts()      ! (k becomes the longest prompt's)
     if (k >= seq_len) then
        print *, "--parallel: the prompt (", k, "tokens ) leaves no position to generate within -n", seq_len
        stop 1
     end if
     if (opts%kv_f16) then
        rc = llmk_cache_create(ctx, int(opts%parallel, c_int), int(seq_len, c_int), 1_c_int, pbatch)      ! LLMK_TYPE_F16
     else if (opts%kv_q8) then
        rc = llmk_cache_create(ctx, int(opts%parallel, c_int), int(seq_len, c_int), 8_c_int, pbatch)      ! LLMK_TYPE_Q8_0
     else
        rc = llmk_batch_create(ctx, int(opts%parallel, c_int), int(seq_len, c_int), pbatch)
     end if
     if (rc == 2) then                               ! LLMK_E_SHAPE
        print *, "--parallel: this model's shape has no batched pass (emb_dim and hidden_dim must be multiples of 64, kv_dim of 16, " // &
             "at most 16 query heads per kv head; with --kv-q8 kv_dim must be a multiple of 32)"
        stop 1
     end if
     call llmk_check(rc, "llmk_batch_create")
     if (opts%verbose_ext) then
        call llmk_check(llmk_cache_bytes(pbatch, kv_bytes), "llmk_cache_bytes")
        print '(A,A,A,I0,A,I0,A)', " batch K/V caches: ", trim(merge("q8_0", merge("f16 ", "f32 ", llmk_cache_type(pbatch) == 1), llmk_cache_type(pbatch) == 8)), ", ", opts%parallel, &
             " slots, ", kv_bytes, " bytes"
     end if
     t_start = clock_ticks()
     token = 2
     if (opts%prompts_file /= "") then
        call ingest_prompts()
        if (opts%verbose_ext) print '(A,I0,A)', " prompts ingested in ", par_passes, " span passes"
     else if (k > 0) then
        allocate(batch(k))
        batch(1) = 2
        batch(2:) = int(prompt_tokens(1:k - 1), c_int)
        call llmk_check(llmk_prefill(ctx, batch, int(k, c_int), 1_c_int, logits), "llmk_prefill")
        token = prompt_tokens(k)
     end if
     par_steps = seq_len - k
     allocate(par_slots(opts%parallel), par_tokens(opts%parallel), par_pos(opts%parallel), par_ids(opts%parallel * par_steps))
     allocate(par_samplers(opts%parallel))
     par_sp = c_null_ptr
     dseed = 0
     if (opts%temperature > 0) then
        if (opts%seed >= 0) then
           dseed = int(opts%seed, c_int64_t)
        else
           call system_clock(dseed)
        end if
        if (opts%verbose) print *, "device sampler seed:", dseed
        par_sp = c_loc(par_samplers)
     end if
     ! --share-prefix: one copy of the prompt's rows for all N slots (without a prompt there is nothing to share)
     if (opts%share_prefix .and. k > 0) call llmk_check(llmk_prefix_set(pbatch, int(k, c_int)), "llmk_prefix_set")
     do j = 1, opts%parallel
        if (opts%prompts_file /= "") then
           continue                                   ! (the slot holds its own prompt's rows: ingest_prompts)
        else if (opts%share_prefix .and. k > 0) then
           call llmk_check(llmk_prefix_attach(pbatch, int(j - 1, c_int)), "llmk_prefix_attach")
        else
           call llmk_check(llmk_batch_fork(pbatch, int(j - 1, c_int), int(k, c_int)), "llmk_batch_fork")
        end if
        par_slots(j) = int(j - 1, c_int)
        par_tokens(j) = int(token, c_int)
        par_pos(j) = int(k + 1, c_int)
        if (opts%prompts_file /= "") then
           par_tokens(j) = par_first(j)
           par_pos(j) = int(par_k(j) + 1, c_int)
        end if
        par_samplers(j)%temperature = real(opts%temperature, c_float)
        par_samplers(j)%top_k = int(opts%top_k, c_int32_t)
        par_samplers(j)%top_p = real(opts%top_p, c_float)
        par_samplers(j)%min_p = real(opts%min_p, c_float)
        par_samplers(j)%seed = dseed + int(j - 1, c_int64_t)
     end do
     call llmk_check(llmk_batch_decode(pbatch, int(opts%parallel, c_int), par_slots, par_tokens, par_pos, int(par_steps, c_int), &
          par_sp, par_ids), "llmk_batch_decode")
     t_end = clock_ticks()
     dt_ms = elapsed_ms(t_start, t_end)
     do j = 1, opts%parallel
        print '(A,I0,A)', "[", j - 1, "]"
        do pos = 1, par_steps
           l = par_ids((j - 1) * par_steps + pos)
           write (*, fmt="(A)", advance="no") vocab(l)(1:vocab_len(l))
        end do
        print '(A)', ""
     end do
     print *, "Inference time: ", dt_ms / 1000, " seconds"
     print *, 1000 * real(opts%parallel, wp) * par_steps / dt_ms, "tokens/second (", opts%parallel, "completions together )"
     rc = llmk_batch_destroy(pbatch)
     rc = llmk_destroy(ctx)
     stop
  end if

  ! --device-sample: EVERY id after the prompt is drawn on the device (llmk_forward_sample / llmk_decode_sample), the first one
  ! and the one after a --prefill prompt included, so the transcript is a function of (model, prompt, T, seed) alone
  ! --top-k / --top-p / --min-p: the truncations live in the device sampler only, so with -t > 0 they select it
  filtered = opts%top_k /= 0 .or. opts%top_p /= 1 .or. opts%min_p /= 0
  if (filtered .and. opts%temperature == 0 .and. lead) &
       write (0, '(A)') "llm: --top-k / --top-p / --min-p are ignored at temperature 0 (the greedy pick needs no truncation)"
  if (filtered .and. opts%temperature > 0 .and. opts%ngpu /= 1 .and. lead) &
       write (0, '(A)') "llm: --top-k / --top-p / --min-p are ignored with --ngpu > 1 (the device sampler runs on one GPU, " // &
       "the host sampler does not truncate)"
  ! --repeat-penalty / --presence-penalty / --frequency-penalty / --logit-bias: likewise (they need the tokens chosen so far, which
  ! stay on the device)
  if (opts%repeat_last_n < 0) opts%repeat_last_n = conf%seq_len
  opts%repeat_last_n = min(opts%repeat_last_n, conf%seq_len)
  penalised = opts%n_bias > 0 .or. (opts%repeat_last_n > 0 .and. &
       (opts%repeat_penalty /= 1 .or. opts%presence_penalty /= 0 .or. opts%frequency_penalty /= 0))
  if (penalised .and. opts%temperature == 0 .and. lead) &
       write (0, '(A)') "llm: the penalties and --logit-bias are ignored at temperature 0 (they live in the device sampler; " // &
       "-t with --top-k 1 is its greedy form)"
  if (penalised .and. opts%temperature > 0 .and. opts%ngpu /= 1 .and. lead) &
       write (0, '(A)') "llm: the penalties and --logit-bias are ignored with --ngpu > 1 (the device sampler runs on one GPU)"
  ! --logprobs N: the records come from the device consumer, so the flag selects it as the filter flags do -- the sampler at -t > 0,
  ! the greedy form (llmk_decode_greedy's rule) at -t 0
  lp_on = opts%logprobs >= 0 .and. opts%ngpu == 1
  if (opts%logprobs >= 0 .and. opts%ngpu /= 1 .and. lead) &
       write (0, '(A)') "llm: --logprobs is ignored with --ngpu > 1 (the log-prob kernel runs on one GPU)"
  dsample = (opts%device_sample .or. filtered .or. penalised .or. lp_on) .and. opts%temperature > 0 .and. opts%ngpu == 1
  penalised = penalised .and. dsample
  if (dsample) then
     if (opts%seed >= 0) then
        dseed = int(opts%seed, c_int64_t)
     else
        call system_clock(dseed)
     end if
     if (opts%verbose .and. lead) print *, "device sampler seed:", dseed
     sampler%temperature = real(opts%temperature, c_float)
     sampler%top_k = int(opts%top_k, c_int32_t)
     sampler%top_p = real(opts%top_p, c_float)
     sampler%min_p = real(opts%min_p, c_float)
     sampler%seed = dseed
     if (opts%verbose_ext .and. lead) print '(A,F8.4,A,I0,A,F8.5,A,F8.5)', " device sampler: temperature", opts%temperature, &
          " top_k ", opts%top_k, " top_p", opts%top_p, " min_p", opts%min_p
     allocate(bias_list(max(1, opts%n_bias)))
     do k = 1, opts%n_bias
        bias_list(k)%token = int(opts%bias_id(k), c_int32_t)
        bias_list(k)%bias = real(opts%bias_val(k), c_float)
     end do
     pens%last_n = int(opts%repeat_last_n, c_int32_t)
     pens%repeat = real(opts%repeat_penalty, c_float)
     pens%frequency = real(opts%frequency_penalty, c_float)
     pens%presence = real(opts%presence_penalty, c_float)
     pens%bias = c_loc(bias_list)
     pens%n_bias = int(opts%n_bias, c_int32_t)
     if (penalised .and. opts%verbose_ext .and. lead) then
        print '(A,F8.4,A,I0,A,F8.4,A,F8.4,A,I0,A)', " device sampler: repeat penalty", opts%repeat_penalty, " over the last ", &
             opts%repeat_last_n, " tokens, frequency", opts%frequency_penalty, " presence", opts%presence_penalty, ", ", opts%n_bias, &
             " logit bias entries"
        do k = 1, opts%n_bias
           print '(A,I0,A,ES12.4)', "   logit bias: token ", opts%bias_id(k), " ", opts%bias_val(k)
        end do
     end if
  end if

  if (lp_on) then
     lp_w = opts%logprobs
     allocate(lp_ids(conf%seq_len), lp_token(conf%seq_len), lp_top(max(1, lp_w * conf%seq_len)), lp_top_ids(max(1, lp_w * conf%seq_len)))
     lp_n = 0
     lp_sp = c_null_ptr
     lp_pn = c_null_ptr
     if (dsample) then
        lp_sampler = sampler
        lp_sp = c_loc(lp_sampler)
        if (penalised) then
           lp_pens = pens
           lp_pn = c_loc(lp_pens)
        end if
     end if
  end if

  ! ---- generation loop (llama2.f90:376-402) -------------------------------------------------------
  t_start = 0
  token = 2                                          ! BOS: 1-based index of <s>
  pos0 = 1
  if ((dsample .or. lp_on) .and. opts%prefill .and. size(prompt_tokens) > 0 .and. size(prompt_tokens) < seq_len) then
     ! positions 1 .. k (BOS, then the first k-1 prompt tokens) in one call; the last prompt token goes through the loop below,
     ! whose llmk_forward_sample draws the first id on the device (--logprobs at -t 0 too: the first generated token gets its record)
     k = size(prompt_tokens)
     allocate(batch(k))
     batch(1) = 2
     batch(2:) = int(prompt_tokens(1:k - 1), c_int)
     t_start = clock_ticks()
     call llmk_check(llmk_prefill(ctx, batch, int(k, c_int), 1_c_int, logits), "llmk_prefill")
     if (lead) then
        do pos = 1, k
           write (*, fmt="(A)", advance="no") vocab(prompt_tokens(pos))(1:vocab_len(prompt_tokens(pos)))
        end do
     end if
     token = prompt_tokens(k)
     pos0 = k + 1
  else if (opts%prefill .and. size(prompt_tokens) > 0 .and. size(prompt_tokens) < seq_len) then
     ! positions 1 .. k+1 of the loop below (BOS, then the k prompt tokens) in one call: same cache, same logits
     ! at position k+1, same text on stdout
     k = size(prompt_tokens)
     allocate(batch(k + 1))
     batch(1) = 2
     batch(2:) = int(prompt_tokens, c_int)
     t_start = clock_ticks()   ! the clock covers the prompt pass: tokens/second counts those positions too (llama2.f90:405)
     call llmk_check(llmk_prefill(ctx, batch, int(k + 1, c_int), 1_c_int, logits), "llmk_prefill")
     if (lead) then
        do pos = 1, k
           write (*, fmt="(A)", advance="no") vocab(prompt_tokens(pos))(1:vocab_len(prompt_tokens(pos)))
        end do
     end if
     if (opts%temperature == 0) then
        token = argmax1(logits)
     else
        probs = softmax_t(logits / opts%temperature)
        token = sample(probs)
     end if
     if (lead) write (*, fmt="(A)", advance="no") vocab(token)(1:vocab_len(token))
     pos0 = k + 2
  end if
  ! --device-argmax at temperature 0: every position after the prompt is one call (llmk_decode_greedy: the argmax stays on
  ! the device, the launches are enqueued back to back, the ids stream back through mapped memory and are printed as they
  ! arrive).  The positions whose next token is a PROMPT token still go through the loop below -- and so does the FIRST
  ! position in any case: the reference starts its clock after the first token (llama2.f90:398-399) and divides seq_len - 1
  ! tokens by what follows, so that token is produced, and the clock started, before the pipelined launches are enqueued
  ! (started at the first streamed id instead, several tokens had already completed: the printed rate was slightly high).
  loop_end = seq_len
  ! the penalties read the context's token record: BOS and the prompt (the tokens fed at positions 1 .. k+1; the last of them is
  ! recorded again by the first sampled position, which is fed it) go in once, before the first sampled position
  if (penalised) then
     k = min(size(prompt_tokens), conf%seq_len - 1)
     allocate(hist_tokens(k + 1))
     hist_tokens(1) = 2
     hist_tokens(2:) = int(prompt_tokens(1:k), c_int)
     call llmk_check(llmk_set_history(ctx, hist_tokens, int(k + 1, c_int), 1_c_int), "llmk_set_history")
  end if
  ! --device-sample likewise, with llmk_forward_sample_pen / llmk_decode_sample_pen (no penalty and no bias: llmk_forward_sample_ex /
  ! llmk_decode_sample_ex; all filters off as well: llmk_forward_sample / llmk_decode_sample)
  if ((opts%device_argmax .and. opts%temperature == 0 .and. opts%ngpu == 1) .or. dsample .or. lp_on) &
       loop_end = min(seq_len, max(size(prompt_tokens), pos0))
  do pos = pos0, loop_end
     if (lp_on .and. pos > size(prompt_tokens)) then
        call llmk_check(llmk_forward_sample_lp(ctx, int(token, c_int), int(pos, c_int), lp_sp, lp_pn, lp_request(lp_n, 1), dnext), &
             "llmk_forward_sample_lp")
        lp_n = lp_n + 1
        lp_ids(lp_n) = dnext
        token = dnext
        if (lead) write (*, fmt="(A)", advance="no") vocab(token)(1:vocab_len(token))
        if (t_start == 0) t_start = clock_ticks()
        cycle
     end if
     if (dsample .and. pos > size(prompt_tokens)) then
        call llmk_check(llmk_forward_sample_pen(ctx, int(token, c_int), int(pos, c_int), sampler, pens, dnext), "llmk_forward_sample_pen")
        next_tok = dnext
        token = next_tok
        if (lead) write (*, fmt="(A)", advance="no") vocab(token)(1:vocab_len(token))
        if (t_start == 0) t_start = clock_ticks()
        cycle
     end if
     call llmk_check(llmk_forward(ctx, int(token, c_int), int(pos, c_int), logits), "llmk_forward")
     if (pos <= size(prompt_tokens)) then
        next_tok = prompt_tokens(pos)
     else if (opts%temperature == 0) then
        next_tok = argmax1(logits)
     else
        probs = softmax_t(logits / opts%temperature)
        next_tok = sample(probs)
     end if
     token = next_tok
     if (lead) write (*, fmt="(A)", advance="no") vocab(token)(1:vocab_len(token))
     if (t_start == 0) t_start = clock_ticks()       ! clock starts after the first token
  end do
  if (loop_end < seq_len) then
     allocate(stream_ids(seq_len - loop_end))
     ts_vocab = vocab
     ts_len = vocab_len
     ts_print = lead
     if (lp_on) then
        call llmk_check(llmk_decode_sample_lp(ctx, int(token, c_int), int(loop_end + 1, c_int), int(seq_len - loop_end, c_int), &
             lp_sp, lp_pn, lp_request(lp_n, seq_len - loop_end), stream_ids, c_funloc(ts_on_token), c_null_ptr), "llmk_decode_sample_lp")
        lp_ids(lp_n + 1:lp_n + size(stream_ids)) = stream_ids
        lp_n = lp_n + size(stream_ids)
     else if (dsample) then
        call llmk_check(llmk_decode_sample_pen(ctx, int(token, c_int), int(loop_end + 1, c_int), int(seq_len - loop_end, c_int), &
             sampler, pens, stream_ids, c_funloc(ts_on_token), c_null_ptr), "llmk_decode_sample_pen")
     else
        call llmk_check(llmk_decode_greedy(ctx, int(token, c_int), int(loop_end + 1, c_int), int(seq_len - loop_end, c_int), &
             stream_ids, c_funloc(ts_on_token), c_null_ptr), "llmk_decode_greedy")
     end if
     token = stream_ids(size(stream_ids))
     if (t_start == 0) t_start = ts_first
  end if
  t_end = clock_ticks()
  dt_ms = elapsed_ms(t_start, t_end)

  call llmk_check(llmk_timings(ctx, ktimes), "llmk_timings")
  s%times = ktimes
  ! --logprobs: after the generated text and a newline, in the formats of --score: one line per generated token -- index, id,
  ! log-prob, then the N alternatives as id:log-prob -- and the three totals
  if (lp_on .and. lead) then
     print '(A)', ""
     sc_sum = 0
     do pos = 1, lp_n
        write (*, '(I0,1X,I0,1X,ES15.8)', advance="no") pos, lp_ids(pos), lp_token(pos)
        do j = 1, lp_w
           write (*, '(1X,I0,A,ES15.8)', advance="no") lp_top_ids((pos - 1) * lp_w + j), ":", lp_top((pos - 1) * lp_w + j)
        end do
        print '(A)', ""
        sc_sum = sc_sum + lp_token(pos)
     end do
     print '(A,1X,I0)', "tokens", lp_n
     print '(A,1X,ES15.8)', "sum logprob", sc_sum
     if (lp_n > 0) print '(A,1X,ES15.8)', "perplexity", exp(-sc_sum / lp_n)
  end if
  if (lead) then
     print *, ""
     print *, "Inference time: ", dt_ms / 1000, " seconds"
     print *, 1000 * (seq_len - 1) / dt_ms, "tokens/second"
     print *, "Timings"
     do l = 1, 5
        print *, l, s%times(l) / seq_len
     end do
  end if
  if (opts%ngpu > 1) call tp_finish()
  rc = llmk_destroy(ctx)

contains

  ! --prompts FILE: line j of the file is slot j's prompt.  Slot j's positions 1 .. k_j hold BOS and the first k_j - 1 tokens of its
  ! prompt, and its last token (BOS for an empty line) is what the slot feeds at k_j + 1 -- `-p` for every slot.  k: the longest k_j.
  subroutine read_prompts()
    character(len=65536) :: line
    integer, allocatable :: toks(:)
    integer :: u, ios, jj
    allocate(par_k(opts%parallel), par_fed(opts%parallel), par_first(opts%parallel), par_off(opts%parallel), par_seq(0))
    open (newunit=u, file=opts%prompts_file, status="old", action="read", iostat=ios)
    if (ios /= 0) then
       print *, "--prompts: cannot open ", opts%prompts_file
       stop 1
    end if
    do jj = 1, opts%parallel
       read (u, '(A)', iostat=ios) line
       if (ios /= 0) then
          print '(A,A,A,I0,A,I0,A)', " --prompts: ", opts%prompts_file, " has ", jj - 1, " lines; --parallel ", opts%parallel, &
               " needs one prompt per slot"
          stop 1
       end if
       toks = bpe_encode(trim(line))
       par_k(jj) = size(toks)
       par_off(jj) = size(par_seq)
       par_first(jj) = 2
       if (par_k(jj) > 0) then
          par_first(jj) = int(toks(par_k(jj)), c_int)
          par_seq = [par_seq, 2_c_int, int(toks(1:par_k(jj) - 1), c_int)]
       end if
    end do
    close (u)
    k = maxval(par_k)
  end subroutine read_prompts

  ! the slots' prompts through the batch itself: every pass takes the next chunk of every slot that still has one, in slot order, up to
  ! 128 rows in all (llmk_span_forward; LLMK_SPAN_LAST: one first maximum per span comes back)
  subroutine ingest_prompts()
    integer :: jj
    allocate(par_spans(opts%parallel), par_feed(128), par_am(opts%parallel))
    par_fed = 0
    par_passes = 0
    do while (any(par_fed < par_k))
       n_sp = 0
       n_rows = 0
       do jj = 1, opts%parallel
          take = min(par_k(jj) - par_fed(jj), 128 - n_rows)
          if (take < 1) cycle
          n_sp = n_sp + 1
          par_spans(n_sp) = llmk_span(int(jj - 1, c_int32_t), int(par_fed(jj) + 1, c_int32_t), int(take, c_int32_t))
          par_feed(n_rows + 1:n_rows + take) = par_seq(par_off(jj) + par_fed(jj) + 1:par_off(jj) + par_fed(jj) + take)
          n_rows = n_rows + take
          par_fed(jj) = par_fed(jj) + take
       end do
       call llmk_check(llmk_span_forward(pbatch, int(n_sp, c_int), par_spans, par_feed, LLMK_SPAN_LAST, c_null_ptr, c_loc(par_am)), &
            "llmk_span_forward")
       par_passes = par_passes + 1
    end do
  end subroutine ingest_prompts

  ! the request for the next n positions: the records go behind the `done` already there
  function lp_request(done, n) result(r)
    integer, intent(in) :: done, n
    type(llmk_logprobs) :: r
    r%top_n = int(lp_w, c_int32_t)
    r%token_logprob = c_loc(lp_token(done + 1))
    r%top_tokens = c_null_ptr
    r%top_logprobs = c_null_ptr
    if (lp_w > 0 .and. n > 0) then
       r%top_tokens = c_loc(lp_top_ids(done * lp_w + 1))
       r%top_logprobs = c_loc(lp_top(done * lp_w + 1))
    end if
  end function lp_request

  subroutine upload_weights()
    integer(c_size_t) :: f4
    f4 = 4
    call llmk_check(llmk_upload(ctx, LLMK_TOKEN_EMBEDDING_TABLE, c_loc(weights%token_embedding_table), &
         f4 * size(weights%token_embedding_table, kind=c_size_t), LLMK_TYPE_F32), "upload token_embedding_table")
    call llmk_check(llmk_upload(ctx, LLMK_RMS_ATT_WEIGHT, c_loc(weights%rms_att_weight), &
         f4 * size(weights%rms_att_weight, kind=c_size_t), LLMK_TYPE_F32), "upload rms_att_weight")
    call llmk_check(llmk_upload(ctx, LLMK_RMS_FFN_WEIGHT, c_loc(weights%rms_ffn_weight), &
         f4 * size(weights%rms_ffn_weight, kind=c_size_t), LLMK_TYPE_F32), "upload rms_ffn_weight")
    call llmk_check(llmk_upload(ctx, LLMK_RMS_FINAL_WEIGHT, c_loc(weights%rms_final_weight), &
         f4 * size(weights%rms_final_weight, kind=c_size_t), LLMK_TYPE_F32), "upload rms_final_weight")
    if (weights%wtype == LLMK_TYPE_F32) then
       call llmk_check(llmk_upload(ctx, LLMK_WQKV, c_loc(weights%wqkv), f4 * size(weights%wqkv, kind=c_size_t), &
            LLMK_TYPE_F32), "upload wqkv")
       call llmk_check(llmk_upload(ctx, LLMK_WO, c_loc(weights%wo), f4 * size(weights%wo, kind=c_size_t), &
            LLMK_TYPE_F32), "upload wo")
       call llmk_check(llmk_upload(ctx, LLMK_W13, c_loc(weights%w13), f4 * size(weights%w13, kind=c_size_t), &
            LLMK_TYPE_F32), "upload w13")
       call llmk_check(llmk_upload(ctx, LLMK_W2, c_loc(weights%w2), f4 * size(weights%w2, kind=c_size_t), &
            LLMK_TYPE_F32), "upload w2")
       call llmk_check(llmk_upload(ctx, LLMK_WCLS, c_loc(weights%wcls), f4 * size(weights%wcls, kind=c_size_t), &
            LLMK_TYPE_F32), "upload wcls")
       deallocate(weights%wqkv, weights%wo, weights%w13, weights%w2, weights%wcls)
    else
       call llmk_check(llmk_upload(ctx, LLMK_WQKV, c_loc(weights%wqkv_raw), size(weights%wqkv_raw, kind=c_size_t), &
            int(weights%wtype, c_int)), "upload wqkv")
       call llmk_check(llmk_upload(ctx, LLMK_WO, c_loc(weights%wo_raw), size(weights%wo_raw, kind=c_size_t), &
            int(weights%wtype, c_int)), "upload wo")
       call llmk_check(llmk_upload(ctx, LLMK_W13, c_loc(weights%w13_raw), size(weights%w13_raw, kind=c_size_t), &
            int(weights%wtype, c_int)), "upload w13")
       call llmk_check(llmk_upload(ctx, LLMK_W2, c_loc(weights%w2_raw), size(weights%w2_raw, kind=c_size_t), &
            int(weights%wtype, c_int)), "upload w2")
       if (weights%wcls_type == LLMK_TYPE_F32) then      ! classifier dequantised by the loader (q6_K output.weight)
          call llmk_check(llmk_upload(ctx, LLMK_WCLS, c_loc(weights%wcls), f4 * size(weights%wcls, kind=c_size_t), &
               LLMK_TYPE_F32), "upload wcls")
          deallocate(weights%wcls)
       else
          call llmk_check(llmk_upload(ctx, LLMK_WCLS, c_loc(weights%wcls_raw), size(weights%wcls_raw, kind=c_size_t), &
               int(weights%wcls_type, c_int)), "upload wcls")
          deallocate(weights%wcls_raw)
       end if
       deallocate(weights%wqkv_raw, weights%wo_raw, weights%w13_raw, weights%w2_raw)
    end if
    deallocate(weights%token_embedding_table)
  end subroutine upload_weights

  ! maxloc(v, dim=1) (llama2.f90:388: the first maximum, 1-based) in two vectorisable passes: eight running maxima, then the first
  ! element equal to the largest.  flang's maxloc is a scalar compare-and-branch loop: 20-45 us for the 32,000 logits, 3-6 % of a
  ! 0.68 ms token -- the one piece of host arithmetic on the path (measured: bench.py fortran_host, profiles/r05_*fortran_cli*).
  function argmax1(v) result(idx)
    real(kind=wp), intent(in) :: v(:)
    integer :: idx, i, n8
    real(kind=wp) :: m(8), mm
    n8 = size(v) / 8 * 8
    m = v(1)
    do i = 1, n8, 8
       m = max(m, v(i:i + 7))
    end do
    mm = maxval(m)
    do i = n8 + 1, size(v)
       mm = max(mm, v(i))
    end do
    do idx = 1, size(v)
       if (v(idx) == mm) return
    end do
    idx = maxloc(v, dim=1)                    ! (a NaN among the logits: whatever the intrinsic answers)
  end function argmax1

  ! Wall clock.  The reference converts a 4-byte millisecond count to real(4) BEFORE subtracting (llama2.f90:417-423):
  ! a count of ~1e9 has a 64-128 ms quantum as a float, which is nothing against its 60 s runs and everything against a
  ! 0.17 s run of 256 tokens on the GPU.  Same two printed lines, same real(4) list-directed format; the difference is taken
  ! in 8-byte ticks first (microseconds or finer with amdflang).
  function clock_ticks() result(t)
    integer(8) :: t
    call system_clock(t)
    if (t == 0) t = 1                    ! 0 means "clock not started yet" in the generation loop
  end function clock_ticks
  function elapsed_ms(t0, t1) result(ms)
    integer(8), intent(in) :: t0, t1
    real(kind=wp) :: ms
    integer(8) :: rate
    call system_clock(count_rate=rate)
    ms = real(1000.0d0 * real(t1 - t0, 8) / real(rate, 8), kind=wp)
  end function elapsed_ms

  ! llama2.c tokenizer.bin: max_len, then (f32 score, i32 len, bytes) per token (llama2.f90:321-356)
  subroutine read_tokenizer_bin(path)
    character(len=*), intent(in) :: path
    integer :: tu, n, tl, width
    real(kind=wp) :: sc
    character(len=:), allocatable :: buf
    open(newunit=tu, file=path, form="unformatted", access="stream", status="old", action="read")
    read(tu) width
    if (allocated(vocab)) deallocate(vocab, scores, vocab_len)
    allocate(character(len=width) :: vocab(conf%vocab_size))
    allocate(scores(conf%vocab_size), vocab_len(conf%vocab_size))
    do n = 1, conf%vocab_size
       read(tu) sc
       read(tu) tl
       allocate(character(len=tl) :: buf)
       read(tu) buf
       vocab(n) = buf
       scores(n) = sc
       vocab_len(n) = tl
       deallocate(buf)
    end do
    close(tu)
  end subroutine read_tokenizer_bin

  ! ---- vocabulary index: exact-match lookup honouring the true token length (trailing blanks are data).  The reference
  ! scans all V strings per lookup (llama2.f90:643-655), O(V) per candidate pair of every merge round; this is an
  ! open-addressing hash (FNV-1a over the bytes) built once.  Same answer: the FIRST index holding the string.
  function hash_bytes(str, n) result(h)
    character(len=*), intent(in) :: str
    integer, intent(in) :: n
    integer :: h, i
    integer(8) :: acc
    acc = 2166136261_8
    do i = 1, n
       acc = iand(ieor(acc, int(ichar(str(i:i)), 8)) * 16777619_8, 4294967295_8)
    end do
    h = int(iand(acc, int(hash_mask, 8)))
  end function hash_bytes

  subroutine build_lookup()
    integer :: i, h, cap
    cap = 1
    do while (cap < 2 * size(vocab) + 2)
       cap = cap * 2
    end do
    hash_mask = cap - 1
    if (allocated(hash_tab)) deallocate(hash_tab)
    allocate(hash_tab(0:cap - 1))
    hash_tab = 0
    do i = 1, size(vocab)
       h = hash_bytes(vocab(i), int(vocab_len(i)))
       do
          if (hash_tab(h) == 0) then
             hash_tab(h) = i
             exit
          end if
          if (vocab_len(hash_tab(h)) == vocab_len(i)) then
             if (vocab(hash_tab(h))(1:vocab_len(i)) == vocab(i)(1:vocab_len(i))) exit    ! duplicate: the first index wins
          end if
          h = iand(h + 1, hash_mask)
       end do
    end do
  end subroutine build_lookup

  function lookup(str, n) result(idx)
    character(len=*), intent(in) :: str
    integer, intent(in) :: n
    integer :: idx, h
    h = hash_bytes(str, n)
    do
       idx = hash_tab(h)
       if (idx == 0) exit
       if (vocab_len(idx) == n) then
          if (vocab(idx)(1:n) == str(1:n)) return
       end if
       h = iand(h + 1, hash_mask)
    end do
    idx = -1
  end function lookup

  ! a byte with no single-character token: llama's byte-fallback token "<0xXX>", else <unk> (the reference indexes
  ! vocab_len(-1) here, llama2.f90:666-668 + :683)
  function byte_token(ch) result(idx)
    character(len=1), intent(in) :: ch
    integer :: idx
    character(len=6) :: name
    character(len=16), parameter :: hex = "0123456789ABCDEF"
    integer :: b
    idx = lookup(ch, 1)
    if (idx > 0) return
    b = ichar(ch)
    name = "<0x" // hex(b / 16 + 1:b / 16 + 1) // hex(mod(b, 16) + 1:mod(b, 16) + 1) // ">"
    idx = lookup(name, 6)
    if (idx < 0) idx = 1                                   ! <unk>
  end function byte_token

  ! llama2.c-style BPE (behaviour of llama2.f90:658-724): start from one token per byte, then
  ! repeatedly fuse the adjacent pair whose concatenation is the best-scoring vocabulary entry.
  function bpe_encode(text) result(tokens)
    character(len=*), intent(in) :: text
    integer, allocatable :: tokens(:)
    integer :: n, i, best_i, best_tok, cand, la, lb
    real(kind=wp) :: best_score
    character(len=:), allocatable :: pair

    n = len(text)
    allocate(tokens(n))
    do i = 1, n
       tokens(i) = byte_token(text(i:i))
    end do
    do
       best_score = -1e10
       best_i = -1
       best_tok = -1
       do i = 1, n - 1
          la = vocab_len(tokens(i))
          lb = vocab_len(tokens(i + 1))
          pair = vocab(tokens(i))(1:la) // vocab(tokens(i + 1))(1:lb)
          cand = lookup(pair, la + lb)
          if (cand > 0) then
             if (scores(cand) > best_score) then
                best_score = scores(cand)
                best_i = i
                best_tok = cand
             end if
          end if
       end do
       if (best_i < 0) exit
       tokens(best_i) = best_tok
       tokens(best_i + 1:n - 1) = tokens(best_i + 2:n)
       n = n - 1
    end do
    tokens = tokens(1:n)
  end function bpe_encode

  ! softmax over the whole vocabulary for temperature sampling (llama2.f90:390, :468-478)
  function softmax_t(x) result(p)
    real(kind=wp), intent(in) :: x(:)
    real(kind=wp) :: p(size(x))
    p = exp(x - maxval(x))
    p = p / sum(p)
  end function softmax_t

  ! inverse-CDF draw (llama2.f90:428-447)
  function sample(p) result(idx)
    real(kind=wp), intent(in) :: p(:)
    integer :: idx
    real(kind=wp) :: r, cdf
    call random_number(r)
    cdf = 0
    do idx = 1, size(p)
       cdf = cdf + p(idx)
       if (r < cdf) return
    end do
    idx = size(p)
  end function sample

  ! `--seed N`: a reproducible sampler (and identical draws on every tensor-parallel rank)
  subroutine seed_sampler(seed)
    integer, intent(in) :: seed
    integer :: n, i
    integer, allocatable :: put(:)
    call random_seed(size=n)
    allocate(put(n))
    do i = 1, n
       put(i) = ieor(seed * 1664525 + 1013904223, i * 668265263)
    end do
    call random_seed(put=put)
  end subroutine seed_sampler

  ! ---- `--ngpu N`: one process per GPU ------------------------------------------------------------------------------
  integer(c_int) function tp_device()
    character(len=8) :: env
    integer :: st
    tp_device = int(opts%device + opts%tp_rank, c_int)
    call get_environment_variable("LLMK_TP_SAME_DEVICE", env, status=st)      ! test aid: all ranks on one GPU
    if (st == 0) tp_device = int(opts%device, c_int)
  end function tp_device

  function shell_quote(a) result(q)
    character(len=*), intent(in) :: a
    character(len=:), allocatable :: q
    integer :: i
    q = "'"
    do i = 1, len(a)
       if (a(i:i) == "'") then
          q = q // "'\''"
       else
          q = q // a(i:i)
       end if
    end do
    q = q // "'"
  end function shell_quote

  ! rank 0: make the rendezvous directory and start ranks 1..N-1 as copies of this command line
  subroutine tp_launch_workers()
    character(kind=c_char) :: tmpl(32)
    character(len=4096) :: arg
    character(len=:), allocatable :: cmd, base
    character(len=32) :: num
    integer :: i, r, seed, ticks
    if (opts%tp_rank > 0) return                       ! a worker: everything was handed down
    ! a fresh private directory (mkdtemp: unpredictable name, mode 0700, fails rather than reuse): nothing stale from a
    ! crashed run with the same pid, nothing another local user could have planted
    tmpl(1:22) = transfer("/tmp/llmk_tp_XXXXXX" // c_null_char // "  ", tmpl(1:22))
    if (.not. c_associated(c_mkdtemp(tmpl))) then
       print *, "cannot create the tensor-parallel rendezvous directory under /tmp"
       stop 1
    end if
    opts%tp_dir = transfer(tmpl(1:19), repeat(" ", 19))
    call execute_command_line("touch " // opts%tp_dir // "/alive")
    call get_command_argument(0, arg)
    base = shell_quote(trim(arg))
    do i = 1, command_argument_count()
       call get_command_argument(i, arg)
       base = base // " " // shell_quote(trim(arg))
    end do
    if (opts%temperature /= 0 .and. opts%seed < 0) then   ! sampling: every rank must draw the same numbers
       call system_clock(ticks)
       seed = iand(ticks, 1073741823)
       opts%seed = seed
       write (num, "(I0)") seed
       base = base // " --seed " // trim(num)
    end if
    do r = 1, opts%ngpu - 1
       write (num, "(I0)") r
       cmd = base // " --tp-rank " // trim(num) // " --tp-dir " // opts%tp_dir // " > /dev/null 2> " // opts%tp_dir // &
             "/rank" // trim(num) // ".err &"
       call execute_command_line(cmd, wait=.false.)
    end do
  end subroutine tp_launch_workers

  subroutine tp_put(name, bytes)
    character(len=*), intent(in) :: name
    character(kind=c_char), intent(in) :: bytes(:)
    integer :: fu
    open(newunit=fu, file=opts%tp_dir // "/" // name // ".tmp", form="unformatted", access="stream", status="replace")
    write (fu) bytes
    close(fu)
    call execute_command_line("mv " // opts%tp_dir // "/" // name // ".tmp " // opts%tp_dir // "/" // name)   ! atomic
  end subroutine tp_put

  subroutine tp_get(name, bytes)
    character(len=*), intent(in) :: name
    character(kind=c_char), intent(out) :: bytes(:)
    integer :: fu, waited
    logical :: there
    waited = 0
    do
       inquire(file=opts%tp_dir // "/" // name, exist=there)
       if (there) exit
       inquire(file=opts%tp_dir // "/alive", exist=there)
       if (.not. there .and. opts%tp_rank > 0) stop 1   ! rank 0 is gone (it removes the directory on every exit path it controls)
       rc = c_usleep(20000_c_int)
       waited = waited + 1
       if (waited > 15000) then                        ! 5 minutes: a peer died while loading
          print *, "tensor-parallel rendezvous timed out waiting for ", name
          if (opts%tp_rank == 0) then                  ! what the workers said, then nothing left behind
             call execute_command_line("cat " // opts%tp_dir // "/rank*.err 1>&2; rm -rf " // opts%tp_dir)
          end if
          stop 1
       end if
    end do
    open(newunit=fu, file=opts%tp_dir // "/" // name, form="unformatted", access="stream", status="old", action="read")
    read (fu) bytes
    close(fu)
  end subroutine tp_get

  ! exchange the inbox handles (or the RCCL id) through the rendezvous directory
  subroutine tp_connect()
    character(kind=c_char) :: h(64), uid(128), verdict(1)
    character(kind=c_char), allocatable :: all(:)
    character(len=32) :: num
    integer :: r
    logical :: all_ok
    if (opts%tp_rccl) then
       if (opts%tp_rank == 0) then
          call llmk_check(llmk_tp_unique_id(uid), "llmk_tp_unique_id")
          call tp_put("uid", uid)
       else
          call tp_get("uid", uid)
       end if
       call llmk_check(llmk_tp_init_comm(ctx, uid), "llmk_tp_init_comm")
       return
    end if
    call llmk_check(llmk_tp_p2p_handle(ctx, h), "llmk_tp_p2p_handle")
    write (num, "(I0)") opts%tp_rank
    call tp_put("inbox" // trim(num), h)
    allocate(all(64 * opts%ngpu))
    do r = 0, opts%ngpu - 1
       write (num, "(I0)") r
       call tp_get("inbox" // trim(num), all(64 * r + 1:64 * r + 64))
    end do
    call llmk_check(llmk_tp_p2p_connect(ctx, all), "llmk_tp_p2p_connect")
    ! The peer-memory path proves itself on THIS hardware before the first token (64 rounds of every collective on known
    ! integers).  Unless every rank passes, all ranks drop it together and the token pass runs over RCCL.
    verdict(1) = "y"
    if (llmk_tp_p2p_selftest(ctx, 64_c_int) /= 0) verdict(1) = "n"
    write (num, "(I0)") opts%tp_rank
    call tp_put("p2p" // trim(num), verdict)
    all_ok = .true.
    do r = 0, opts%ngpu - 1
       write (num, "(I0)") r
       call tp_get("p2p" // trim(num), verdict)
       if (verdict(1) /= "y") all_ok = .false.
    end do
    if (.not. all_ok) then
       if (lead) write (0, *) "llmk: the peer-memory collectives failed their self-test on this node: using RCCL"
       call llmk_check(llmk_tp_p2p_disable(ctx), "llmk_tp_p2p_disable")
       if (opts%tp_rank == 0) then
          call llmk_check(llmk_tp_unique_id(uid), "llmk_tp_unique_id")
          call tp_put("uid", uid)
       else
          call tp_get("uid", uid)
       end if
       call llmk_check(llmk_tp_init_comm(ctx, uid), "llmk_tp_init_comm")
    end if
  end subroutine tp_connect

  ! rank 0 leaves last and removes the directory
  subroutine tp_finish()
    character(kind=c_char) :: one(1)
    character(len=32) :: num
    integer :: r
    one(1) = "x"
    write (num, "(I0)") opts%tp_rank
    if (opts%tp_rank > 0) then
       call tp_put("done" // trim(num), one)
       return
    end if
    do r = 1, opts%ngpu - 1
       write (num, "(I0)") r
       call tp_get("done" // trim(num), one)
    end do
    call execute_command_line("rm -rf " // opts%tp_dir)
  end subroutine tp_finish

end program llm
