"""llmk_forward with the next greedy position in flight (csrc/forward_ahead.h) against a second context
created with LLMK_FORWARD_AHEAD=0, which runs one launch and one stream sync per call: the logits of every call are the same BITS
(the greedy instantiation of the token kernel stores the same quotient as the plain one), the K/V rows up to the last position are
the same, and every other entry point finds the context as it would have been with nothing in flight.  llmk_forward_ahead_stats
says that the launches really happened: without it these tests would pass with the feature never arming.

tk-small (f32) and tk-small16 (f16): the shapes the persistent kernel is instantiated for at test size, seq_len 64."""
import numpy as np
import pytest

from llm_f90_amd import llmk

pytestmark = pytest.mark.gpu

SHAPES = [("tk-small", 0), ("tk-small16", 1)]
IDS = ["f32", "f16"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(params=SHAPES, ids=IDS)
def pair(request, gguf, monkeypatch):
    """(shape, ahead, plain): two contexts on the same weights, the second with the feature switched off at create"""
    name, wtype = request.param
    s = gguf.SHAPES[name]
    fw = gguf.synth_fused(s, 20261020, wtype)
    monkeypatch.delenv("LLMK_FORWARD_AHEAD", raising=False)
    a = llmk.Llmk(fw)
    monkeypatch.setenv("LLMK_FORWARD_AHEAD", "0")
    b = llmk.Llmk(fw)
    monkeypatch.delenv("LLMK_FORWARD_AHEAD")
    assert a.path() == 1 and b.path() == 1, (a.path_name(), b.path_name())
    yield s, a, b
    assert b.forward_ahead_stats() == {"launches": 0, "hits": 0, "misses": 0, "armed": False}
    a.close()
    b.close()


def greedy(a, b, pos0, pos1, token, wrong=()):
    """positions pos0..pos1 on both contexts, each fed the first maximum of the logits before (at a position in `wrong`: that id
    + 1, wrapped); every call's logits bit-identical.  Returns the next token."""
    for pos in range(pos0, pos1 + 1):
        if pos in wrong:
            token = token % a.V + 1
        la, lb = a.forward(token, pos), b.forward(token, pos)
        assert same_bits(la, lb), pos
        token = int(np.argmax(la)) + 1
    return token


def same_kv(s, a, b, upto):
    for layer in range(s.n_layers):
        for which in (4, 5):
            for pos in range(1, upto + 1):
                if not np.array_equal(a.peek(which, s.kv_dim, layer, pos), b.peek(which, s.kv_dim, layer, pos)):
                    return False
    return True


def test_greedy_run_hits_from_the_fourth_position_to_the_last(pair):
    s, a, b = pair
    S = s.seq_len
    greedy(a, b, 1, S, 2)
    st = a.forward_ahead_stats()
    # armed by the third call; positions 4..S are hits; launched ahead: positions 4..S and nothing for S + 1
    assert st["hits"] >= 60 and st["hits"] == S - 3 and st["misses"] == 0, st
    assert st["launches"] == S - 3 and not st["armed"], st
    with pytest.raises(llmk.LlmkError):
        a.forward(2, S + 1)
    assert same_kv(s, a, b, S)


def test_wrong_tokens_miss_and_the_machine_comes_back(pair):
    s, a, b = pair
    S = s.seq_len
    greedy(a, b, 1, S, 2, wrong=(5, 6, 20))
    st = a.forward_ahead_stats()
    # position 5 finds position 5 in flight on another token: a miss.  6 and 20 fall into the 16 calls without a comparison that
    # follow it; 22 and 23 agree again, 24..S are hits (and 4 was one)
    assert st["misses"] == 1, st
    assert st["hits"] == 1 + (S - 23), st
    assert not st["armed"]
    assert same_kv(s, a, b, S)


def test_every_other_entry_point_settles_the_launch_in_flight(pair):
    s, a, b = pair
    V = s.vocab_size
    rng = np.random.default_rng(5)
    toks = (rng.integers(1, V, 7) + 1).tolist()

    def in_flight():
        """both contexts reset and five greedy positions on: position 6 is in flight on `a`.  Returns the token for position 6."""
        a.reset(), b.reset()
        tok = greedy(a, b, 1, 5, 2)
        assert a.forward_ahead_stats()["armed"]
        return tok

    def settled(upto):
        assert not a.forward_ahead_stats()["armed"]
        assert same_kv(s, a, b, upto)

    in_flight()                                            # llmk_reset
    a.reset(), b.reset()
    settled(6)
    greedy(a, b, 1, 6, 2)

    in_flight()                                            # llmk_prefill, over the row the launch wrote
    assert same_bits(a.prefill(toks, 6), b.prefill(toks, 6))
    settled(12)
    greedy(a, b, 13, 18, toks[-1])

    in_flight()                                            # llmk_score
    for x, y in zip(a.score(toks, 6, want_argmax=True, want_logits=True), b.score(toks, 6, want_argmax=True, want_logits=True)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    settled(12)

    tok = in_flight()                                      # llmk_forward somewhere else: a miss
    before = a.forward_ahead_stats()["misses"]
    assert same_bits(a.forward(tok, 1), b.forward(tok, 1))
    assert a.forward_ahead_stats()["misses"] == before + 1
    settled(5)
    greedy(a, b, 2, 20, tok)                               # (through the 16 calls without a comparison that a miss starts)
    assert a.forward_ahead_stats()["armed"]

    tok = in_flight()                                      # llmk_forward_greedy
    assert a.forward_greedy(tok, 6) == b.forward_greedy(tok, 6)
    settled(6)

    tok = in_flight()                                      # llmk_decode_greedy
    assert np.array_equal(a.decode_greedy(tok, 6, 10), b.decode_greedy(tok, 6, 10))
    settled(15)

    in_flight()                                            # llmk_peek: rows up to the last position the caller asked for
    for which in (4, 5):
        assert np.array_equal(a.peek(which, s.kv_dim, 1, 5), b.peek(which, s.kv_dim, 1, 5))
    settled(5)

    in_flight()                                            # llmk_time_kernel, and the reset it asks for
    assert a.time_kernel(6, 3)[0] > 0 and b.time_kernel(6, 3)[0] > 0
    assert not a.forward_ahead_stats()["armed"]
    a.reset(), b.reset()
    greedy(a, b, 1, 8, 2)
    assert a.forward_ahead_stats()["armed"]
    # llmk_close with position 9 in flight: the fixture's teardown


def test_two_runs_with_a_reset_between_are_bit_identical(pair):
    s, a, _ = pair
    runs = []
    for _r in range(2):
        a.reset()
        tok, out = 2, []
        for pos in range(1, s.seq_len + 1):
            out.append(a.forward(tok, pos))
            tok = int(np.argmax(out[-1])) + 1
        runs.append(np.stack(out))
    assert same_bits(runs[0], runs[1])
    assert a.forward_ahead_stats()["hits"] == 2 * (s.seq_len - 3)
