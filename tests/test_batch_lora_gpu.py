"""A LoRA adapter per slot of a batch (llmk_lora_*; csrc/lora.h).  The reference is the float64 pass over
W + scale B A, each slot's sequence alone (lora_ref.py, which also asserts that every adapter moves the logits by more than 100 x the bar:
an ignored or swapped adapter fails).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lora_ref as lr
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf
from test_batch_span_gpu import bits, first_max, model, random_seq, within_the_bar
from test_batch_tree_gpu import ref_tree

pytestmark = pytest.mark.gpu
F32, F16, Q4_0 = gguf.GGML_F32, gguf.GGML_F16, gguf.GGML_Q4_0

CASES = {      # shape, matrices, q6_K classifier, [(rank, targets)], rows.  lora_chunk: E 128 | 256 one chunk, H 768 three, 1408 six (ragged)
    "f32-1row-rank4": ("tiny-gqa", F32, False, [(4, lr.ALL)], 1),
    "f16-16rows-rank16-qv": ("tk-small", F16, False, [(16, lr.QV)], 16),
    "q4_0-q6k-17rows-rank64": ("tk-small", Q4_0, True, [(64, lr.ALL)], 17),            # two groups, the second with one column
    "q4_0-17rows-mixed": ("tk-small", Q4_0, False, [(24, lr.ALL), (24, lr.QV), (8, lr.REST)], 17),
    "f32-hs128w-17rows-mixed": ("tiny-hs128w", F32, False, [(24, lr.ALL), (16, lr.QV), (8, lr.REST)], 17),
    "f32-16rows-16adapters": ("tk-small", F32, False, [(4 + 4 * (i % 4), lr.ALL) for i in range(16)], 16),
    "f32-128rows-mixed": ("tiny-gqa", F32, False, [(16, lr.ALL), (24, lr.QV), (4, lr.REST)], 128),
}


def assignment(n_adapters, n):
    """row j on adapter j mod n_adapters; with several adapters every (n_adapters + 1)-th row on the base model"""
    return [None if n_adapters > 1 and j % (n_adapters + 1) == n_adapters else j % (n_adapters + 1) % n_adapters for j in range(n)]


def assigned(fw, specs, assign, seed):
    """(rng, adapters, context, Lora handles, a batch with slot j on assign[j])"""
    rng = np.random.default_rng(seed)
    adapters = [lr.draw(rng, fw.shape, r, t) for r, t in specs]
    m = llmk.Llmk(fw)
    ads = lr.upload(llmk, m, adapters)
    b = llmk.Batch(m, len(assign))
    for j, a in enumerate(assign):
        b.set_lora(j, None if a is None else ads[a])
    return rng, adapters, m, ads, b


def close(*handles):
    for h in handles:
        h.close()


def run_case(cid):
    shape, wtype, q6k, specs, n = CASES[cid]
    fw, fw32 = model(shape, wtype, q6k)
    assign = assignment(len(specs), n)
    rng, adapters, m, ads, b = assigned(fw, specs, assign, 31)
    seqs = [random_seq(rng, fw.shape.vocab_size, 2) for _ in range(n)]
    ref = lr.references(lr.models(fw32, adapters), assign, seqs)
    for p in (1, 2):
        order = rng.permutation(n)
        lg, am = b.forward(order, [seqs[j][p - 1] for j in order], [p] * n)
        assert np.array_equal(am, first_max(lg))
        within_the_bar(f"{cid} position {p}", lg, np.stack([ref[j][p - 1] for j in order]))
    close(b, *ads, m)


@pytest.mark.parametrize("cid", list(CASES))
def test_rows_on_adapters_match_the_float64_pass_over_the_merged_weights(cid):
    run_case(cid)


def test_the_f32_instruction_s_partial_tiles_take_the_correction_in_a_child_process():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "f32-hs128w-17rows-mixed"], env=dict(os.environ, LLMK_PF_F32_MFMA="1"),
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]


TREE = [-1, -1, 0, 0, 1, 2]
SPECS = [(16, lr.ALL), (24, lr.QV), (4, lr.REST)]
ASSIGN = [0, 1, 2, None, 0, 1]
POS0 = 4


@pytest.mark.parametrize("kind", ["forward", "decode", "spans", "tree"])
def test_every_call_kind_with_mixed_adapters(kind):
    fw, fw32 = model("tk-small")
    n, V = len(ASSIGN), fw.shape.vocab_size
    rng, adapters, m, ads, b = assigned(fw, SPECS, ASSIGN, 32)
    ms = lr.models(fw32, adapters)
    lens = {"forward": [1] * n, "decode": [4] * n, "spans": [20, 3, 17, 3, 1, 2], "tree": [len(TREE)] * n}[kind]      # slots 0 and 2: more than one group
    seqs = [random_seq(rng, V, POS0 - 1 + k) for k in lens]
    slots = list(range(n))
    b.forward_spans([(j, 1, POS0 - 1) for j in slots], [t for s in seqs for t in s[:POS0 - 1]], want_argmax=False)      # under the adapters
    if kind == "decode":
        ids = b.decode(slots, [s[POS0 - 1] for s in seqs], [POS0] * n, 4)
        seqs = [s[:POS0] + ids[j, :3].tolist() for j, s in enumerate(seqs)]
        got = [b.forward(slots, [s[POS0 - 1 + k] for s in seqs], [POS0 + k] * n, want_argmax=False) for k in range(4)]      # the replay rewrites the same rows
        assert np.array_equal(first_max(np.stack(got, axis=1)), ids)
        got = np.concatenate(np.stack(got, axis=1))
    elif kind == "tree":
        got = b.forward_tree([(j, POS0, len(TREE)) for j in slots], [t for s in seqs for t in s[POS0 - 1:]], TREE * n, want_argmax=False)
    else:
        got = b.forward_spans([(j, POS0, k) for j, k in zip(slots, lens)], [t for s in seqs for t in s[POS0 - 1:]], want_argmax=False)
    if kind == "tree":
        def nodes(k, s):
            stem = ms[k].fork(0)
            stem.feed(s[:POS0 - 1])
            return ref_tree(stem, POS0, s[POS0 - 1:], TREE)
        ref = [nodes(0 if a is None else a + 1, s) for a, s in zip(ASSIGN, seqs)]
        assert all(a is None or lr.far(r, nodes(0, s)) for a, r, s in zip(ASSIGN, ref, seqs))
    else:
        ref = [r[POS0 - 1:] for r in lr.references(ms, ASSIGN, seqs)]
    within_the_bar(kind, got, np.concatenate(ref))
    close(b, *ads, m)


def test_base_rows_keep_their_bits_and_the_interface_does_what_it_says(tmp_path):
    fw, fw32 = model("tk-small")
    rng, adapters, m, ads, b = assigned(fw, [(16, lr.ALL)], [None, None, None, 0], 33)
    plain = llmk.Batch(m, 4)
    rows = ([0, 1, 2], [2, 77, 300], [1, 1, 1])
    base = plain.forward(*rows, want_argmax=False)
    assert np.array_equal(bits(base), bits(b.forward(*rows, want_argmax=False)))      # adapters exist, slot 3 has one, the pass has none
    b.set_lora(0, ads[0])
    one = b.forward(*rows, want_argmax=False)
    assert np.array_equal(bits(one), bits(b.forward(*rows, want_argmax=False)))       # the same call twice
    assert np.array_equal(bits(one[1:]), bits(base[1:])) and lr.far(one[:1], base[:1].astype(np.float64))
    path = str(tmp_path / "adapter.gguf")
    gguf.write_lora_gguf(path, lr.SCALE * 16, adapters[0][2])
    filed = llmk.Lora.from_gguf(m, path)
    b.set_lora(0, filed)
    assert (filed.rank, filed.scale) == (16, np.float32(lr.SCALE * 16) / 16)
    assert np.array_equal(bits(one), bits(b.forward(*rows, want_argmax=False)))
    b.set_lora(0, None)
    assert np.array_equal(bits(base), bits(b.forward(*rows, want_argmax=False)))
    # a piece uploaded again replaces the one it names
    A, B = lr.draw(rng, fw.shape, 16, ("attn_q",))[2]["attn_q", 0]
    ads[0].upload("wqkv", 0, 0, A, B)
    adapters[0][2]["attn_q", 0] = (A, B)
    b.set_lora(0, ads[0])
    ref = lr.references(lr.models(fw32, adapters), [0], [[2]])
    within_the_bar("a replaced piece", b.forward(*rows, want_argmax=False)[:1], ref[0])
    close(plain, b, filed, *ads, m)


def test_refusals_leave_the_pass_as_it_was():
    fw, _ = model("tk-small")
    s, L, h = fw.shape, llmk.lib(), C.c_void_p()
    rng, adapters, m, ads, b = assigned(fw, [(8, lr.QV)], [0, None], 34)
    other = llmk.Llmk(fw)
    foreign = llmk.Lora(other, 8, 0.5)
    buf = np.zeros((2 * s.hidden_dim, s.hidden_dim), np.float32).ctypes.data
    create = lambda rank, scale, ctx=m._h: L.llmk_lora_create(ctx, rank, scale, C.byref(h))
    up = lambda tid, layer, row0, rows, t=0, a=buf: L.llmk_lora_upload(ads[0]._h, tid, layer, row0, rows, a, buf, t)
    assign = lambda slot, ad: L.llmk_lora_assign(b._h, slot, ad)
    cases = {      # LLMK_E_ARG (1) unless a code stands beside the call
        "rank 0": lambda: create(0, 0.5), "rank 65": lambda: create(65, 0.5), "scale inf": lambda: create(8, float("inf")),
        "scale nan": lambda: create(8, float("nan")), "null context": lambda: create(8, 0.5, None),
        "overlaps q": lambda: up(3, 0, s.emb_dim - 4, 8), "inside q": lambda: up(3, 0, 4, 8), "rows past the tensor": lambda: up(4, 0, s.emb_dim - 4, 8),
        "rows % 4": lambda: up(4, 0, 0, 6), "row0 % 4": lambda: up(4, 0, 2, 8), "no rows": lambda: up(4, 0, 0, 0), "layer": lambda: up(4, s.n_layers, 0, 8),
        "the embedding table": lambda: up(0, 0, 0, 8), "null A": lambda: up(4, 0, 0, 8, a=None), "q4_0 pieces": (lambda: up(4, 0, 0, 8, t=2), 4),
        "slot 2": lambda: assign(2, ads[0]._h), "slot -1": lambda: assign(-1, None), "another context's": lambda: assign(1, foreign._h),
        "destroy while assigned": (lambda: L.llmk_lora_destroy(ads[0]._h), 5),
    }
    rows = ([1, 0], [2, 2], [1, 1])
    before = b.forward(*rows, want_argmax=False)
    for what, case in cases.items():
        call, code = case if isinstance(case, tuple) else (case, 1)
        assert call() == code, what
        assert np.array_equal(bits(before), bits(b.forward(*rows, want_argmax=False))), what
    b.close()                                          # ... which releases the adapter
    assert L.llmk_destroy(m._h) == 5                   # LLMK_E_STATE: no batch is left: the live adapter alone refuses
    close(*ads, m, foreign, other)


if __name__ == "__main__":
    run_case(sys.argv[1])
