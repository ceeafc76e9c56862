"""Trees for the batched decode (llmk_tree_*): drafted continuations that share a stem, in one pass.  New on the
device: the QKV epilogues with a RoPE position apart from the place, bd_attn_tree_kernel's ancestor predicate, bd_tree_move_kernel.
Every test reaches them through the public entry points."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import kv16_ref as kr
import span_tiles as st
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf
from ref_pass import RefPass
from test_batch_span_gpu import ROW_CASES, bits, first_max, model, random_seq, within_the_bar

pytestmark = pytest.mark.gpu

# nodes 0 and 1 hang under the root; 2 | 3 and 5 | 6 are siblings; 0 -> 2 -> 5 -> 8 has depth 3; the places 2 and 3 lie between node 4
# and its parent 1 without being its ancestors
TREE = [-1, -1, 0, 0, 1, 2, 2, 4, 5, 5, 7, 8]
HEAP = [(j - 1) // 2 for j in range(100)]      # (node 0: -1, the root) all four mask words, ancestors in earlier column groups
POS0 = 12                                      # places 11 .. straddle the first tile boundary; pos0 - 1 is no tile multiple


def path_to(parent, j):
    return path_to(parent, parent[j]) + [j] if j >= 0 else []


def fed(fw32, tokens):
    """the float64 pass that has fed `tokens`"""
    p = RefPass(fw32)
    p.feed(tokens)
    return p


def ref_tree(stem, pos0, tokens, parent):
    """node j: the float64 pass that fed the slot's first pos0 - 1 tokens (stem), then the tokens along root -> j -- its parent's pass
    forked and fed one token more"""
    at, out = [], []
    for j, p in enumerate(parent):
        at.append(stem.fork(pos0 - 1) if p < 0 else at[p].fork(at[p].n))
        out.append(at[j].feed([tokens[j]])[0])
    return np.stack(out)


@pytest.mark.parametrize("cid", list(ROW_CASES))
def test_every_node_matches_the_float64_pass_on_its_own_sequence(cid):
    shape, wtype, q6k = ROW_CASES[cid]
    fw, fw32 = model(dataclasses.replace(gguf.SHAPES[shape], seq_len=128), wtype, q6k)      # places 12 .. 111
    rng, V = np.random.default_rng(21), fw.shape.vocab_size
    stems = [random_seq(rng, V, POS0 - 1) for _ in range(2)]
    toks = [random_seq(rng, V, len(TREE) + 1)[1:], random_seq(rng, V, len(HEAP) + 1)[1:]]
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 2)
    b.forward_spans([(0, 1, POS0 - 1), (1, 1, POS0 - 1)], stems[0] + stems[1], want_argmax=False)
    lg, am = b.forward_tree([(1, POS0, len(HEAP)), (0, POS0, len(TREE))], toks[1] + toks[0], HEAP + TREE)
    b.close()
    m.close()
    assert np.array_equal(am, first_max(lg))
    within_the_bar(f"{cid} heap", lg[:len(HEAP)], ref_tree(fed(fw32, stems[1]), POS0, toks[1], HEAP))
    within_the_bar(f"{cid} tree", lg[len(HEAP):], ref_tree(fed(fw32, stems[0]), POS0, toks[0], TREE))


def test_a_tree_behind_four_hundred_positions_runs_several_parts():
    fw, fw32 = model("tk-small-long")
    s, pos0 = fw.shape, 400
    rng = np.random.default_rng(22)
    stem, toks = random_seq(rng, s.vocab_size, pos0 - 1), random_seq(rng, s.vocab_size, len(TREE) + 1)[1:]
    assert st.span_parts([(0, pos0, len(TREE))], s.n_kv_heads, s.n_heads // s.n_kv_heads)[0] > 1
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 1)
    b.ingest(0, stem)
    lg = b.forward_tree([(0, pos0, len(TREE))], toks, TREE, want_argmax=False)
    b.close()
    m.close()
    within_the_bar("behind 399 positions", lg, ref_tree(fed(fw32, stem), pos0, toks, TREE))


@pytest.mark.parametrize("shape", ["tiny-hs64", "tiny-kvmul3"])
def test_a_tree_in_a_slot_attached_to_a_prefix(shape):
    """P = 9: slot 0 has two own rows in front of the tree; slot 1 none (pos0 - 1 == P: a child of the root sees the prefix and itself alone)"""
    fw, fw32 = model(shape)
    rng = np.random.default_rng(23)
    stem, toks = random_seq(rng, fw.shape.vocab_size, POS0 - 1), random_seq(rng, fw.shape.vocab_size, len(TREE) + 1)[1:]
    P = 9
    m = llmk.Llmk(fw)
    m.prefill(stem[:P], 1)
    b = llmk.Batch(m, 2)
    b.set_prefix(P)
    b.attach(0)
    b.attach(1)
    b.forward_spans([(0, P + 1, POS0 - 1 - P)], stem[P:], want_argmax=False)
    lg = b.forward_tree([(0, POS0, len(TREE)), (1, P + 1, len(TREE))], toks * 2, TREE * 2, want_argmax=False)
    b.close()
    m.close()
    within_the_bar(f"{shape} attached, own rows", lg[:len(TREE)], ref_tree(fed(fw32, stem), POS0, toks, TREE))
    within_the_bar(f"{shape} attached, none", lg[len(TREE):], ref_tree(fed(fw32, stem[:P]), P + 1, toks, TREE))


def test_a_node_s_bits_depend_on_its_ancestors_alone():
    fw, _ = model("tiny-hs64")
    toks = list(range(30, 30 + len(TREE)))
    other = toks[:2] + [99] + toks[3:]                    # node 2 differs: 2, 5, 6, 8 and 9 hang under it
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 2)
    one = b.forward_tree([(0, 1, len(TREE))], toks, TREE, want_argmax=False)
    two = b.forward_tree([(1, 1, len(TREE))], other, TREE, want_argmax=False)
    b.close()
    m.close()
    for j in range(len(TREE)):
        assert np.array_equal(bits(one[j]), bits(two[j])) == (2 not in path_to(TREE, j)), j


def stored(b, n_layers, slot, rows):      # (K, V) [L][len(rows)][kv_dim] of the cache rows `rows` (0-based) of `slot`
    K, V = kr.peek_all(b, n_layers, slot, max(rows) + 1)
    return K[:, rows], V[:, rows]


@pytest.mark.parametrize("kv", ["f32", "f16", "q8_0"])
def test_each_path_matches_the_pass_fed_its_stored_rows_and_a_chain_is_a_span(kv):
    fw, fw32 = model("tk-small")
    L, V = fw.shape.n_layers, fw.shape.vocab_size
    rng = np.random.default_rng(24)
    stem, toks, chain = random_seq(rng, V, POS0 - 1), random_seq(rng, V, len(TREE) + 1)[1:], random_seq(rng, V, 6)[1:]
    m = llmk.Llmk(fw)
    b, twin = llmk.Batch(m, 2, kv_type=kv), llmk.Batch(m, 2, kv_type=kv)
    for x in (b, twin):
        x.forward_spans([(0, 1, POS0 - 1), (1, 1, POS0 - 1)], stem * 2, want_argmax=False)
    spans = [(1, POS0, 5), (0, POS0, len(TREE))]
    lg = b.forward_tree(spans, chain + toks, list(range(-1, 4)) + TREE, want_argmax=False)
    lg2 = twin.forward_spans(spans, chain + toks, want_argmax=False)
    for leaf in (3, 6, 9, 10, 11):
        path = path_to(TREE, leaf)
        K, Vr = stored(b, L, 0, list(range(POS0 - 1)) + [POS0 - 1 + j for j in path])
        ref = kr.forward_fed(fw32, stem + [toks[j] for j in path], K, Vr)[POS0 - 1:]
        within_the_bar(f"{kv} path {path}", lg[[5 + j for j in path]], ref)
    assert np.array_equal(bits(lg[:5]), bits(lg2[:5]))
    for x, y in zip(stored(b, L, 1, list(range(POS0 + 4))), stored(twin, L, 1, list(range(POS0 + 4)))):
        assert np.array_equal(bits(x), bits(y))
    twin.close()
    b.close()
    m.close()


@pytest.mark.parametrize("kv", ["f32", "f16", "q8_0"])
def test_accept_moves_the_path_down_in_place_and_the_slot_continues(kv):
    fw, fw32 = model("tk-small")
    L, V = fw.shape.n_layers, fw.shape.vocab_size
    rng = np.random.default_rng(25)
    stem, toks = random_seq(rng, V, POS0 - 1), random_seq(rng, V, len(TREE) + 1)[1:]
    path = [0, 2, 5, 8]                                   # row 2 is step 1's source and step 2's destination
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 1, kv_type=kv)
    b.forward_spans([(0, 1, POS0 - 1)], stem, want_argmax=False)
    b.forward_tree([(0, POS0, len(TREE))], toks, TREE, want_argmax=False)
    before = stored(b, L, 0, list(range(POS0 - 1)) + [POS0 - 1 + j for j in path])
    b.accept(0, POS0, path)
    n = POS0 - 1 + len(path)
    for x, y in zip(before, stored(b, L, 0, list(range(n)))):
        assert np.array_equal(bits(x), bits(y))
    seq = stem + [toks[j] for j in path] + [77]
    lg = b.forward([0], [77], [n + 1], want_argmax=False)
    b.accept(0, POS0, [])
    ref = RefPass(fw32).feed(seq) if kv == "f32" else kr.forward_fed(fw32, seq, *stored(b, L, 0, list(range(n + 1))))
    b.close()
    m.close()
    within_the_bar(f"{kv} behind the accepted path", lg, ref[-1:])


def test_code_path_claims_and_refusals():
    fw, _ = model("tk-small", seed=1)
    E_ARG, V, P = 1, fw.shape.vocab_size, 9
    m = llmk.Llmk(fw)
    m.prefill([2] + list(range(40, 40 + P - 1)), 1)
    b, twin = llmk.Batch(m, 3), llmk.Batch(m, 3)                 # seq_len 64
    fresh = b.cache_bytes()
    spans, toks = [(0, 1, 9), (1, 1, 3)], list(range(5, 17))
    lg, am = b.forward_tree(spans, toks, list(range(-1, 8)) + [-1, 0, 1])      # chains: llmk_span_forward, before any tree state
    lg2, am2 = twin.forward_spans(spans, toks)
    assert np.array_equal(bits(lg), bits(lg2)) and np.array_equal(am, am2)
    b.accept(0, 1, [0, 1, 2])
    assert b.cache_bytes() == twin.cache_bytes() == fresh
    b.set_prefix(P)
    b.attach(2)
    ip = C.POINTER(C.c_int)
    out = np.zeros((129, V), np.float32).ctypes.data_as(C.POINTER(C.c_float))

    def fwd(trees, tokens, parent, n=None, null=(), outputs=True):
        a = [(llmk.Span * len(trees))(*[llmk.Span(*x) for x in trees]), (C.c_int * len(tokens))(*tokens), (C.c_int * len(parent))(*parent)]
        a = [None if i in null else C.cast(x, ip if i else C.POINTER(llmk.Span)) for i, x in enumerate(a)]
        return llmk.lib().llmk_tree_forward(b._h, len(trees) if n is None else n, *a, out if outputs else None, None)

    def acc(slot, pos0, path, n=None, null=False):
        return llmk.lib().llmk_tree_accept(b._h, slot, pos0, len(path) if n is None else n, None if null else (C.c_int * max(1, len(path)))(*path))
    ms = C.c_float()
    tm = lambda *a: llmk.lib().llmk_tree_time(b._h, *a, C.byref(ms))
    ok, t3, p3 = [(0, 9, 3)], [5, 5, 5], [-1, -1, 0]
    cases = {
        "null trees": lambda: fwd(ok, t3, p3, null=(0,)), "null tokens": lambda: fwd(ok, t3, p3, null=(1,)),
        "null parent": lambda: fwd(ok, t3, p3, null=(2,)), "no tree": lambda: fwd(ok, t3, p3, n=0), "len 0": lambda: fwd([(0, 9, 0), (1, 9, 3)], t3, p3),
        "129 rows": lambda: fwd([(0, 1, 64), (1, 1, 64), (2, P + 1, 1)], [5] * 129, [-1] * 129), "slot 3": lambda: fwd([(3, 9, 3)], t3, p3),
        "slot -1": lambda: fwd([(-1, 9, 3)], t3, p3), "a slot twice": lambda: fwd(ok * 2, t3 * 2, p3 * 2), "pos0 0": lambda: fwd([(0, 0, 3)], t3, p3),
        "places past seq_len": lambda: fwd([(0, 63, 3)], t3, p3), "attached at P": lambda: fwd([(2, P, 3)], t3, p3), "token 0": lambda: fwd(ok, [5, 0, 5], p3),
        "token V+1": lambda: fwd(ok, [5, 5, V + 1], p3), "parent -2": lambda: fwd(ok, t3, [-1, -2, 0]), "its own parent": lambda: fwd(ok, t3, [-1, -1, 2]),
        "a later parent": lambda: fwd(ok, t3, [1, -1, 0]), "no output": lambda: fwd(ok, t3, p3, outputs=False),
        "accept slot 3": lambda: acc(3, 9, [0, 2]), "accept n -1": lambda: acc(0, 9, [0, 2], n=-1), "accept null path": lambda: acc(0, 9, [0, 2], null=True),
        "accept not increasing": lambda: acc(0, 9, [0, 2, 2]), "accept path -1": lambda: acc(0, 9, [-1, 2]), "accept pos0 0": lambda: acc(0, 0, [0, 2]),
        "accept past seq_len": lambda: acc(0, 9, [0, 56]), "accept attached at P": lambda: acc(2, P, [0, 2]), "time 4 slots": lambda: tm(4, 3, 9, 1),
        "time past seq_len": lambda: tm(1, 3, 63, 1), "time attached": lambda: tm(3, 3, P, 1), "time no iteration": lambda: tm(1, 3, 9, 0),
    }

    def snapshot():
        return [bits(b.peek_kv(w, l, j, 1, 64)) for w in (0, 1) for l in range(fw.shape.n_layers) for j in range(3)]
    before = snapshot()
    for what, call in cases.items():
        assert call() == E_ARG, what
        assert all(np.array_equal(x, y) for x, y in zip(before, snapshot())), what
    assert fwd(ok, t3, p3) == 0 and acc(0, 9, [0, 2]) == 0 and acc(0, 9, []) == 0 and tm(2, 7, 9, 1) == 0 and ms.value > 0.0      # the batch stays usable
    twin.close()
    b.close()
    m.close()
