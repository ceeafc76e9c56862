"""Lifecycle of what the shim owns (csrc/owned.h): buffers that a later call grows, lazily built state that is dropped and built
again, whole create .. close cycles.  tk-small f32, the smallest case of the batch tests; every comparison is BIT-EXACT against a fresh
context or batch that is given the same calls, so a stale pointer, a buffer that kept its old size or state that survived a rebuild
shows as a difference."""
import numpy as np
import pytest

from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf

pytestmark = pytest.mark.gpu

TOKENS = [2] + list(range(40, 48))          # 9 positions
ROWS = dict(slots=[1, 0], tokens=[50, 70], pos0=[1, 1])


@pytest.fixture(scope="module")
def fw():
    return gguf.synth_fused(gguf.SHAPES["tk-small"], 4242)


@pytest.fixture(scope="module")
def fresh_score(fw):
    """(log-probs, argmax, logits) of the 9 positions on a context that did nothing else"""
    m = llmk.Llmk(fw)
    out = m.score(TOKENS, want_argmax=True, want_logits=True)
    m.close()
    return out


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def head(score, n):
    """the first n positions of a longer call's (log-probs, argmax, logits) as a call of n positions answers them: its last
    position has no next token, hence no target"""
    lp, am, lg = score
    return [np.append(lp[:n - 1], np.float32(0)), am[:n], lg[:n]]


def upload_classifier(m, rows, ggml_type):
    a = np.ascontiguousarray(rows)
    llmk._ck(llmk.lib().llmk_upload(m._h, llmk.TENSOR_IDS["wcls"], a.ctypes.data, a.nbytes, ggml_type))


def test_a_longer_score_regrows_the_logits_buffer(fw, fresh_score):
    m = llmk.Llmk(fw)
    short = m.score(TOKENS[:3], want_argmax=True, want_logits=True)
    assert same(short, head(fresh_score, 3))
    assert same(m.score(TOKENS, want_argmax=True, want_logits=True), fresh_score)
    assert same(m.score(TOKENS[:3], want_argmax=True, want_logits=True), short)      # (and the larger buffer serves the shorter call)
    m.close()


def test_a_longer_rows_decode_regrows_the_ids_and_the_records(fw):
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 2)
    short = b.decode_rows(**ROWS, steps=2, top_n=3, want_token_logprob=True)
    grown = b.decode_rows(**ROWS, steps=5, top_n=3, want_token_logprob=True)
    b.close()
    b = llmk.Batch(m, 2)
    fresh = b.decode_rows(**ROWS, steps=5, top_n=3, want_token_logprob=True)
    b.close()
    m.close()
    assert fresh[0].shape == (2, 5) and fresh[0].min() >= 1 and fresh[2].shape == (2, 5, 3)
    assert same(grown, fresh)
    assert same(short, [a[:, :2] for a in fresh])


def test_a_longer_prefix_regrows_the_prefix_rows(fw):
    m = llmk.Llmk(fw)
    m.prefill(TOKENS, 1)

    def behind(b, P):
        b.set_prefix(P)
        b.attach(0)
        return b.forward([0], [50], [P + 1])
    b = llmk.Batch(m, 2)
    behind(b, 3)
    b.fork(0, 0)                      # (detached: the prefix may be replaced)
    grown = behind(b, 9)
    b.close()
    b = llmk.Batch(m, 2)
    fresh = behind(b, 9)
    b.close()
    m.close()
    assert same(grown, fresh)


def test_prefill_workspaces_are_rebuilt_around_a_retyped_classifier(fw, fresh_score):
    m = llmk.Llmk(fw)
    want = m.prefill(TOKENS, 1)
    m.set_tensor_type("wcls", gguf.GGML_F16)
    upload_classifier(m, gguf.encode(fw.wcls, gguf.GGML_F16), gguf.GGML_F16)
    half = m.prefill(TOKENS, 1)                        # (workspaces built for an f16 classifier, then dropped again)
    assert half.shape == want.shape and np.isfinite(half).all()
    m.set_tensor_type("wcls", gguf.GGML_F32)
    upload_classifier(m, fw.wcls, gguf.GGML_F32)
    again = m.prefill(TOKENS, 1)
    scored = m.score(TOKENS, want_argmax=True, want_logits=True)
    m.close()
    m = llmk.Llmk(fw)
    fresh = m.prefill(TOKENS, 1)
    m.close()
    assert same([want], [fresh]) and same([again], [fresh])
    assert same(scored, fresh_score)


def test_two_whole_cycles_in_one_process_agree(fw, fresh_score):
    def cycle():
        m = llmk.Llmk(fw)
        out = [m.prefill(TOKENS, 1)]
        b = llmk.Batch(m, 2)
        b.fork(1, len(TOKENS))
        out.append(b.decode([1, 0], [50, 2], [len(TOKENS) + 1, 1], 3))
        out += list(m.score(TOKENS, want_argmax=True, want_logits=True))
        out.append(m.decode_greedy(50, len(TOKENS) + 1, 4))
        b.close()
        m.close()
        return out
    first, second = cycle(), cycle()
    assert same(first, second)
    assert same(first[2:5], fresh_score)
