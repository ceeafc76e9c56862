"""The split decode attention of the context's own sequence (csrc/attn_split.h) against the float64 pass (tests/ref_pass.py), on needle
models (tests/attn_needle.py): layer 0's softmax mass sits on cache rows 0, 15 | 16 | 17, on both sides of tile P -- the first row
that makes a part take two tiles -- and on the last row, so a dropped, doubled or misplaced timestep moves the logits far above the bar.
Every position is fed, so every position is a query: 1, 15, 16, 17, the trailing parts empty (fewer tiles than parts), tiles = P - 1,
P, P + 1, and each later change of the tiles per part.  The bar is the project's: 1e-4 of the position's max |logit|.

Behind that, launch_attn's other callers under the split form -- the tensor-parallel ranks' pass, LLMK_FLAG_TIMINGS, llmk_time_kernel,
token-by-token llmk_prefill / llmk_score, the sampling decode's graph -- a shallower position behind a deeper one (the part states
persist between launches), and kv_mul beyond the 16 MFMA columns.  The operator alone: tests/test_attn_split_op_gpu.py."""
import numpy as np
import pytest

import attn_needle as an
from conftest import REL_TOL, rel_err
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf
from ref_pass import RefPass

pytestmark = pytest.mark.gpu

# (head size, kv_mul, kv heads, weight type, seq_len, positions fed); parts: attn_split.h ats_parts on 256 CUs (attn_needle.ats_parts)
GRID = [(hs, kv_mul, 2, "f32", 424, 424) for hs in (16, 64, 128) for kv_mul in (1, 3, 8)]
TYPES = [(64, 3, 2, wt, 424, 424) for wt in ("f16", "q4_0")]
DEEP = (16, 1, 128, "f32", 560, 560)        # 2 parts: from position 497 on every wave of both parts has two tiles
LONG = (16, 4, 2, "f32", 65536, 1040)       # 64 parts; tiles = 64 | 65 at positions 1024 | 1025


@pytest.fixture(scope="module")
def case(request):
    """(weights, tokens, float64 logits [n][V], parts) of a 2-layer needle model; shared, read-only"""
    hs, kv_mul, nkv, wtype, S, n = request.param
    s = gguf.LlamaShape(hs * kv_mul * nkv, 64, 2, kv_mul * nkv, nkv, 320, S)
    P = an.ats_parts(nkv, S)
    layout = {0: [0, 15, 16 * P, n - 1], 1: [16, 17, 16 * P - 1]}
    if nkv == 1:
        layout = {0: sorted(layout[0] + layout[1])}
    tokens, needle_tokens = an.needle_sequence(s, layout, 20261127)
    fw32 = an.shape_needles(gguf.synth_fused(s, 4242), needle_tokens, an.BETA)
    fw = an.encode_fused(fw32, an.WTYPES[wtype])
    ref = RefPass(fw32 if wtype == "f32" else fw.as_f32()).feed(tokens[:n])
    ref.setflags(write=False)
    return fw, tokens[:n], ref, P


@pytest.mark.parametrize("case", GRID + TYPES + [DEEP], indirect=True, ids=lambda p: "hs%d-kvmul%d-nkv%d-%s-S%d" % p[:5])
def test_split_attention_matches_the_float64_pass_at_every_position(case, monkeypatch):
    fw, tokens, ref, P = case
    monkeypatch.setenv("LLMK_ATTN_SPLIT", "1")
    m = llmk.Llmk(fw, flags=llmk.FLAG_MULTI_KERNEL)
    logits = np.array([m.forward(int(tok), pos) for pos, tok in enumerate(tokens, 1)])
    m.close()
    err = rel_err(logits, ref)
    print(f"P = {P}: rel_err max {err.max():.2e} at position {int(np.argmax(err)) + 1}; at 1, 15, 16, 17: {err[[0, 14, 15, 16]]}; "
          f"tiles P-1, P, P+1: {err[[16 * P - 17, 16 * P - 1, 16 * P]]}")
    assert err.max() <= REL_TOL, (err.max(), int(np.argmax(err)) + 1)


@pytest.mark.parametrize("case", [LONG], indirect=True, ids=["S65536"])
@pytest.mark.parametrize("flags", [0, llmk.FLAG_MULTI_KERNEL])
def test_a_context_beyond_the_lds_score_row_is_created_on_the_multi_kernel_path(case, flags, monkeypatch):
    fw, tokens, ref, _ = case
    monkeypatch.delenv("LLMK_ATTN_SPLIT", raising=False)
    m = llmk.Llmk(fw, flags=flags)
    assert m.path() == 0, m.path_name()
    logits = np.array([m.forward(int(tok), pos) for pos, tok in enumerate(tokens[:40], 1)])
    m.close()
    assert rel_err(logits, ref[:40]).max() <= REL_TOL


@pytest.mark.parametrize("case", [LONG], indirect=True, ids=["S65536"])
def test_graph_replay_across_a_part_boundary_is_the_eager_pass_and_deterministic(case):
    fw, tokens, ref, P = case
    runs = []
    for flags in (llmk.FLAG_NO_GRAPH, 0, 0):
        m = llmk.Llmk(fw, flags=flags)
        m.prefill(tokens[:16 * P - 24], 1)
        pos0 = 16 * P - 23                      # 40 positions: 1001 .. 1040, tiles 63 -> 65
        ids = m.decode_greedy(int(tokens[pos0 - 1]), pos0, 40)
        m.reset()
        m.prefill(tokens[:pos0 - 1], 1)
        fed = [int(tokens[pos0 - 1])] + [int(i) for i in ids[:-1]]
        runs.append((ids, np.array([m.forward(tok, pos0 + i) for i, tok in enumerate(fed)])))
        m.close()
    (eager_ids, eager), (ids_a, a), (ids_b, b) = runs
    assert np.array_equal(ids_a, eager_ids) and np.array_equal(ids_b, eager_ids)
    assert np.array_equal(a, b) and np.array_equal(np.argmax(a, axis=1) + 1, ids_a)
    assert rel_err(a[:1], ref[pos0 - 1:pos0]).max() <= REL_TOL


@pytest.mark.parametrize("case", [(16, 4, 2, "f32", 424, 80)], indirect=True, ids=["tiny-gqa"])
def test_without_the_switch_the_old_kernel_runs_bit_for_bit(case, monkeypatch):
    fw, tokens, ref, _ = case
    out = {}
    for value in (None, "0", "1"):
        monkeypatch.delenv("LLMK_ATTN_SPLIT", raising=False) if value is None else monkeypatch.setenv("LLMK_ATTN_SPLIT", value)
        m = llmk.Llmk(fw, flags=llmk.FLAG_MULTI_KERNEL)
        out[value] = np.array([m.forward(int(tok), pos) for pos, tok in enumerate(tokens, 1)])
        m.close()
    assert np.array_equal(out[None], out["0"])
    assert not np.array_equal(out[None], out["1"]) and rel_err(out["1"], ref).max() <= REL_TOL


# ---- launch_attn's other callers under the split form: the ranks' pass, the timed pass, the token-by-token prefill, the sampler's graph ----
def feed(m, tokens, pos0=1):
    return np.array([m.forward(int(tok), pos) for pos, tok in enumerate(tokens, pos0)])


@pytest.mark.parametrize("case", [(16, 4, 4, "f32", 424, 90)], indirect=True, ids=["nkv4"])
@pytest.mark.parametrize("tp", [2, 4])
def test_virtual_ranks_under_the_split_form_match_the_float64_pass(case, tp, monkeypatch):
    """n_kv_local = 2 | 1: the grid is KVl / HS kv heads by ats_parts(nkv / tp_size, ..) parts.  tests/test_tp_gpu.tp_generate's
    exchange, teacher-forced over 90 positions (past tile P + 1)."""
    fw, tokens, ref, P = case
    monkeypatch.setenv("LLMK_ATTN_SPLIT", "1")
    assert an.ats_parts(4 // tp, 424) == P and len(tokens) > 16 * (P + 1)
    ranks = [llmk.Llmk(fw, tp_rank=r, tp_size=tp) for r in range(tp)]

    def exchange():
        total = ranks[0].tp_read_partial()
        for m in ranks[1:]:
            total = total + m.tp_read_partial()       # fixed rank order, f32
        for m in ranks:
            m.tp_write_partial(total)

    logits = np.empty((len(tokens), fw.shape.vocab_size), np.float32)
    for pos, tok in enumerate(tokens, 1):
        for m in ranks:
            m.tp_begin(int(tok), pos)
        for layer in range(fw.shape.n_layers):
            for seg in (0, 1):
                for m in ranks:
                    m.tp_segment(seg, layer)
                exchange()
        for m in ranks:
            m.tp_segment(2)
        logits[pos - 1] = np.concatenate([m.tp_read_logits() for m in ranks])
    for m in ranks:
        m.close()
    one = llmk.Llmk(fw, flags=llmk.FLAG_MULTI_KERNEL)
    single = feed(one, tokens)
    one.close()
    err, err1 = rel_err(logits, ref), rel_err(single, logits.astype(np.float64))
    print(f"tp {tp}: rel_err vs float64 max {err.max():.2e} at {int(np.argmax(err)) + 1}; one rank vs the ranks {err1.max():.2e}")
    assert err.max() <= REL_TOL, (err.max(), int(np.argmax(err)) + 1)
    assert err1.max() <= REL_TOL


TINY = (16, 4, 2, "f32", 424, 80)


@pytest.fixture()
def split_base(case, monkeypatch):
    """the case under LLMK_ATTN_SPLIT=1 and its per-position llmk_forward logits on the multi-kernel path"""
    fw, tokens, ref, P = case
    monkeypatch.setenv("LLMK_ATTN_SPLIT", "1")
    m = llmk.Llmk(fw, flags=llmk.FLAG_MULTI_KERNEL)
    base = feed(m, tokens)
    m.close()
    assert rel_err(base, ref).max() <= REL_TOL
    return fw, tokens, base, P


@pytest.mark.parametrize("case", [TINY], indirect=True, ids=["tiny-gqa"])
def test_the_timed_pass_and_the_token_by_token_prefill_are_the_forward_pass_bit_for_bit(split_base, monkeypatch):
    fw, tokens, base, _ = split_base
    m = llmk.Llmk(fw, flags=llmk.FLAG_TIMINGS | llmk.FLAG_MULTI_KERNEL)
    timed = feed(m, tokens)
    m.close()
    assert np.array_equal(timed, base), "LLMK_FLAG_TIMINGS"
    monkeypatch.setenv("LLMK_PREFILL", "0")
    m = llmk.Llmk(fw, flags=llmk.FLAG_MULTI_KERNEL)
    assert np.array_equal(m.prefill(tokens, 1), base[-1]), "llmk_prefill, token by token"
    m.reset()
    assert np.array_equal(m.score(tokens, want_logits=True, want_logprob=False), base), "llmk_score, token by token"
    m.close()


@pytest.mark.parametrize("case", [TINY], indirect=True, ids=["tiny-gqa"])
def test_time_kernel_runs_the_split_pair_and_a_reset_context_feeds_as_before(split_base):
    fw, tokens, base, _ = split_base
    m = llmk.Llmk(fw, flags=llmk.FLAG_MULTI_KERNEL)
    feed(m, tokens)
    ms1, _ = m.time_kernel(1, 8)
    ms11, _ = m.time_kernel(11, 2)
    assert ms1 > 0 and ms11 > 0, (ms1, ms11)
    m.reset()
    assert np.array_equal(feed(m, tokens), base)
    m.close()


@pytest.mark.parametrize("case", [TINY], indirect=True, ids=["tiny-gqa"])
def test_the_sampling_decodes_graph_draws_the_forward_sample_chain_across_tile_P(split_base):
    fw, tokens, _, P = split_base
    pos0, n, T, seed = 16 * P - 19, 40, 0.9, 20261127              # positions 45 .. 84: tiles 3 -> 6 at P = 4
    assert pos0 < 16 * P < pos0 + n - 1
    m = llmk.Llmk(fw, flags=llmk.FLAG_MULTI_KERNEL)
    feed(m, tokens[:pos0 - 1])
    ids = m.decode_sample(int(tokens[pos0 - 1]), pos0, n, T, seed)
    m.reset()
    feed(m, tokens[:pos0 - 1])
    chain, tok = [], int(tokens[pos0 - 1])
    for pos in range(pos0, pos0 + n):
        tok = m.forward_sample(tok, pos, T, seed)
        chain.append(tok)
    m.close()
    assert chain == ids.tolist()


@pytest.mark.parametrize("case", [(16, 4, 2, "f32", 424, 200)], indirect=True, ids=["tiny-gqa-200"])
def test_going_back_to_a_shallower_position_finds_no_state_of_the_deeper_one(split_base):
    """Position 200 has 13 tiles in 4 parts (4, 4, 4, 1); position 30 has two, and parts 2 and 3 -- which held tiles -- are empty
    there: their states must have been rewritten neutral by that launch, with or without llmk_reset."""
    fw, tokens, base, P = split_base
    assert P == 4
    m = llmk.Llmk(fw, flags=llmk.FLAG_MULTI_KERNEL)
    assert np.array_equal(feed(m, tokens), base)
    assert np.array_equal(m.forward(int(tokens[29]), 30), base[29]), "position 30 again, behind position 200"
    m.reset()
    assert np.array_equal(feed(m, tokens[:40]), base[:40]), "positions 1 .. 40 behind a reset"
    m.close()


# ---- more than ATS_MAX_GROUP query heads per kv head: no split form, attn_kernel and its limit stand ----
E_SHAPE = 2             # include/llmk.h LLMK_E_SHAPE: what llmk_create answers where attn_kernel's score row does not fit the LDS
S_BEYOND = 40448        # attn_kernel's score row ends at 40,444 positions


@pytest.mark.parametrize("case", [(16, 32, 1, "f32", 200, 200)], indirect=True, ids=["kvmul32"])
def test_kv_mul_beyond_the_mfma_columns_keeps_attn_kernel_and_its_limit(case, monkeypatch):
    fw, tokens, ref, _ = case
    assert fw.shape.n_heads // fw.shape.n_kv_heads > an.ATS_MAX_GROUP
    out = {}
    for value in (None, "1"):
        monkeypatch.delenv("LLMK_ATTN_SPLIT", raising=False) if value is None else monkeypatch.setenv("LLMK_ATTN_SPLIT", value)
        m = llmk.Llmk(fw, flags=llmk.FLAG_MULTI_KERNEL)
        out[value] = feed(m, tokens)
        m.close()
    assert np.array_equal(out["1"], out[None]) and rel_err(out[None], ref).max() <= REL_TOL
    with pytest.raises(llmk.LlmkError) as e:
        llmk.Llmk(fw, flags=llmk.FLAG_MULTI_KERNEL, seq_len=S_BEYOND)
    assert e.value.code == E_SHAPE


@pytest.mark.parametrize("case", [(16, 16, 1, "f32", S_BEYOND, 20)], indirect=True, ids=["kvmul16"])
def test_kv_mul_16_is_created_beyond_attn_kernels_limit(case, monkeypatch):
    fw, tokens, ref, _ = case
    monkeypatch.delenv("LLMK_ATTN_SPLIT", raising=False)
    m = llmk.Llmk(fw, flags=llmk.FLAG_MULTI_KERNEL)
    logits = feed(m, tokens)
    m.close()
    assert rel_err(logits, ref).max() <= REL_TOL
