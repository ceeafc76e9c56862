"""The committed traces of tests/serve_trace.py without a device: does every trace hold every kind of op, do
the traces between them go through every transition tests/test_batch_serve_gpu.py is there for, and is every op legal in the host
model's state?  The coverage is read from the op lists -- World.events, collected while the ops are replayed with made-up answers in
the place of the device's -- so a change to the generator that loses a transition fails here, before the GPU test silently stops
covering it."""
import json

import numpy as np
import pytest

import serve_trace as st
from llm_f90_amd.tools import gguf
from ref_pass import RefPass

S, V = 64, 400            # tk-small and tiny-kvmul3: seq_len 64; the smaller vocabulary
TYPES = {"span-first": ["f32"], "prefix-first": ["q8_0"], "two": ["f16", "q8_0"]}


def events(name):
    ops = st.generate(name)
    return ops, st.replay(st.World(S, V, TYPES[name]), ops, np.random.default_rng(1))


@pytest.mark.parametrize("name", list(st.TRACES))
def test_every_trace_holds_every_kind_of_op_and_at_least_60_ops(name):
    ops, ev = events(name)
    assert len(ops) >= 60, len(ops)
    missing = [k for k in st.OP_KINDS if k not in ev]
    assert not missing, missing
    for step in range(1, 7):
        assert any(op["op"] in ("decode", "decode_rows") and op["steps"] == step for op in ops), step
    assert any(op["op"] == "fork" and op["n_pos"] == 0 for op in ops) and any(op["op"] == "set_prefix" and op["n_pos"] == 0 for op in ops)
    assert {op["what"] for op in ops if op["op"] == "refuse"} == set(st.REFUSALS)


def test_the_traces_go_through_every_transition_between_them():
    seen = {name: events(name)[1] for name in st.TRACES}
    for t in st.TRANSITIONS:
        assert any(t in ev for ev in seen.values()), t
    # a: the two orders are two traces; k: the trace of two batches
    assert "a_span_first" in seen["span-first"] and "a_prefix_first" not in seen["span-first"]
    assert "a_prefix_first" in seen["prefix-first"] and "a_span_first" not in seen["prefix-first"]
    assert "k_two_types" in seen["two"] and {op["b"] for op in st.generate("two")} == {0, 1}
    for name in ("span-first", "prefix-first"):                  # one batch alone goes through everything else
        assert set(st.TRANSITIONS) - seen[name] <= {"a_span_first", "a_prefix_first", "k_two_types"}, (name, set(st.TRANSITIONS) - seen[name])


@pytest.mark.parametrize("name", list(st.TRACES))
def test_every_op_is_legal_at_most_128_rows_wide_and_within_seq_len(name):
    """World.begin asserts legality against the state; restated here on the ops alone: rows, positions, tokens, slots"""
    ops = st.generate(name)
    assert json.dumps(ops) == json.dumps(st.generate(name))                       # seeded: the same trace in every process
    st.replay(st.World(S, V, TYPES[name]), ops, np.random.default_rng(2))          # (other answers: the ops stay legal)
    for op in ops:
        if op["op"] == "refuse":
            continue
        rows = pos = toks = slots = ()
        if op["op"] == "forward":
            rows, pos, toks, slots = op["slots"], op["pos"], op["tokens"], op["slots"]
        elif op["op"] == "spans":
            pos = [p + n - 1 for _, p, n in op["spans"]] + [p for _, p, _ in op["spans"]]
            rows, toks, slots = op["tokens"], op["tokens"], [sl for sl, _, _ in op["spans"]]
        elif op["op"] in ("decode", "decode_rows"):
            rows, toks, slots = op["slots"], op["tokens"], op["slots"]
            pos = list(op["pos0"]) + [p + op["steps"] - 1 for p in op["pos0"]]
        elif op["op"] in ("prefill", "set_history"):
            toks = [t for t in op["tokens"] if t]
        assert len(rows) <= st.MAX_ROWS and all(1 <= p <= S for p in pos), op
        assert all(1 <= t <= V for t in toks) and all(0 <= sl < st.N_SLOTS for sl in slots) and len(set(slots)) == len(slots), op


def test_the_model_refuses_what_is_not_legal():
    w = st.World(S, V)
    w.begin(dict(op="prefill", tokens=[2, 3, 4, 5]))
    for bad in (dict(op="fork", slot=0, n_pos=5), dict(op="attach", slot=0), dict(op="forward", slots=[0], tokens=[3], pos=[2]),
                dict(op="forward", slots=[1, 1], tokens=[3, 3], pos=[1, 1]), dict(op="spans", spans=[(0, 1, 65)], tokens=[3] * 65),
                dict(op="set_prefix", n_pos=5)):
        with pytest.raises(AssertionError):
            w.begin(bad)
    w.begin(dict(op="time", n=2, pos=1, iters=1))
    with pytest.raises(AssertionError):                                            # a slot a time hook overwrote
        w.begin(dict(op="forward", slots=[1], tokens=[3], pos=[1]))
    w.begin(dict(op="fork", slot=1, n_pos=0))
    w.begin(dict(op="forward", slots=[1], tokens=[3], pos=[1]))
    w.begin(dict(op="set_prefix", n_pos=3))
    w.begin(dict(op="attach", slot=2))
    with pytest.raises(AssertionError):
        w.begin(dict(op="set_prefix", n_pos=0))
    with pytest.raises(AssertionError):
        w.begin(dict(op="forward", slots=[2], tokens=[3], pos=[3]))


def test_a_slot_s_reference_is_the_pass_over_its_logical_sequence_alone():
    """the model's references on a trace prefix, with numbers: a slot's logits after forks, attaches, rejected drafts and a replaced
    prefix are what a fresh RefPass gives on the slot's logical sequence (prefix tokens + own tokens) alone"""
    fw = gguf.synth_fused(gguf.SHAPES["tiny-kvmul3"], 777)
    w = st.World(S, V, ["f32"], RefPass(fw))
    rng = np.random.default_rng(3)
    checked = 0
    for op in st.generate("prefix-first")[:70]:
        out = w.begin(op)
        if op["op"] in ("greedy", "decode", "decode_rows"):
            w.finish(op, st.made_up(w, op, rng))
        if op["op"] == "forward":
            for i, sl in enumerate(op["slots"]):
                seq = w.b[0].slots[sl].seq
                assert len(seq) == op["pos"][i] and seq[-1] == op["tokens"][i]
                want = RefPass(fw).feed(seq)[-1]
                assert np.abs(out["logits"][i] - want).max() <= 1e-9 * np.abs(want).max(), (op, sl)
                checked += 1
    assert checked >= 20
