"""The split decode attention of the context's own sequence (csrc/attn_split.h) against the float64 pass (tests/ref_pass.py), on needle
models (tests/attn_needle.py): layer 0's softmax mass sits on cache rows 0, 15 | 16 | 17, on both sides of tile P -- the first row
that makes a part take two tiles -- and on the last row, so a dropped, doubled or misplaced timestep moves the logits far above the bar.
Every position is fed, so every position is a query: 1, 15, 16, 17, the trailing parts empty (fewer tiles than parts), tiles = P - 1,
P, P + 1, and each later change of the tiles per part.  The bar is the project's: 1e-4 of the position's max |logit|."""
import numpy as np
import pytest

import attn_needle as an
from conftest import REL_TOL, rel_err
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf
from ref_pass import RefPass

pytestmark = pytest.mark.gpu

# (head size, kv_mul, kv heads, weight type, seq_len, positions fed); parts: attn_split.h ats_parts on 256 CUs
GRID = [(hs, kv_mul, 2, "f32", 424, 424) for hs in (16, 64, 128) for kv_mul in (1, 3, 8)]
TYPES = [(64, 3, 2, wt, 424, 424) for wt in ("f16", "q4_0")]
DEEP = (16, 1, 128, "f32", 560, 560)        # 2 parts: from position 497 on every wave of both parts has two tiles
LONG = (16, 4, 2, "f32", 65536, 1040)       # 64 parts; tiles = 64 | 65 at positions 1024 | 1025


@pytest.fixture(scope="module")
def case(request):
    """(weights, tokens, float64 logits [n][V], parts) of a 2-layer needle model; shared, read-only"""
    hs, kv_mul, nkv, wtype, S, n = request.param
    s = gguf.LlamaShape(hs * kv_mul * nkv, 64, 2, kv_mul * nkv, nkv, 320, S)
    P = max(1, min(256 // nkv, -(-(-(-S // 16)) // 8), 64))
    layout = {0: [0, 15, 16 * P, n - 1], 1: [16, 17, 16 * P - 1]}
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
