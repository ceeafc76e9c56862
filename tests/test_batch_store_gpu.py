"""The K/V store of a batch (llmk_cache_create): every call that writes, zeroes, copies or reads the cache
blocks and the prefix rows, driven through ONE script for each of the three element types.  The types' own test files check what a
type stores; this one checks that the store calls do the same thing whatever the type is: after every step, every position of every
slot (and of the prefix) is the context's row converted by the type's rule, or +0.0, and the byte count is the closed form.

3 slots of 20 positions -- two attention tiles, the second ragged -- on a context filled to 20 positions:
fork(0, 20) (no tail to zero), fork(1, 7), fork(2, 0), set_prefix(5), attach(2), fork(2, 3) (a fork over an attached slot: it detaches).
"""
import numpy as np
import pytest

import kv16_ref as kr
import kvq8_ref as kq
from llm_f90_amd import llmk
from test_batch_kv16_gpu import bits, model

pytestmark = pytest.mark.gpu

N_SLOTS, SEQ, P = 3, 20, 5
# the type's conversion of an f32 row, and the bytes of n elements
RULES = {"f32": (lambda x: np.asarray(x, np.float32), lambda n: 4 * n),
         "f16": (kr.stored_half, lambda n: 2 * n),
         "q8_0": (kq.stored_q8, lambda n: n + n // 32 * 2)}


@pytest.fixture(scope="module")
def filled():
    """(the context, its K/V rows [which][layer][SEQ][kv_dim] of positions 1..SEQ), shared by the three cases and never changed"""
    fw, _ = model("tk-small", seed=31)
    s = fw.shape
    rng = np.random.default_rng(9)
    prompt = [2] + (rng.integers(3, s.vocab_size, SEQ - 1) + 1).tolist()
    m = llmk.Llmk(fw)
    m.prefill(prompt, 1)
    rows = np.stack([np.stack([np.stack([m.peek(4 + which, s.kv_dim, l, p) for p in range(1, SEQ + 1)]) for l in range(s.n_layers)])
                     for which in (0, 1)])
    rows.setflags(write=False)
    yield m, rows
    m.close()


@pytest.mark.parametrize("kv_type", list(RULES))
def test_every_store_call_of_a_type_through_one_script(filled, kv_type):
    m, ctx = filled
    s = m.shape
    convert, nbytes = RULES[kv_type]
    stored = convert(ctx)
    if kv_type != "f32":
        assert not np.array_equal(bits(stored), bits(ctx))      # (the conversion is visible on these rows)
    b = llmk.Batch(m, N_SLOTS, seq_len=SEQ, kv_type=kv_type)
    assert b.kv_type == kv_type
    want = np.zeros((N_SLOTS,) + ctx.shape, np.float32)          # [slot][which][layer][SEQ][kv_dim], +0.0: a fresh slot
    prefix = 0

    def check(step):
        for which in (0, 1):
            for l in range(s.n_layers):
                for slot in range(N_SLOTS):
                    got = b.peek_kv(which, l, slot, 1, SEQ)
                    assert np.array_equal(bits(got), bits(want[slot, which, l])), (kv_type, step, which, l, slot)
                if prefix:
                    assert np.array_equal(bits(b.peek_kv(which, l, -1, 1, prefix)), bits(stored[which, l, :prefix])), (kv_type, step, which, l)
        assert b.prefix_len == prefix
        elems = 2 * s.n_layers * s.kv_dim * (N_SLOTS * SEQ + prefix)
        assert b.cache_bytes() == nbytes(elems), (kv_type, step, b.cache_bytes())

    def fork(slot, n_pos):
        b.fork(slot, n_pos)
        want[slot] = 0
        want[slot, :, :, :n_pos] = stored[:, :, :n_pos]

    check("create")
    for slot, n_pos in ((0, SEQ), (1, 7), (2, 0)):
        fork(slot, n_pos)
        check(f"fork({slot}, {n_pos})")
    b.set_prefix(P)
    prefix = P
    check(f"set_prefix({P})")
    b.attach(2)
    want[2] = 0
    check("attach(2)")
    fork(2, 3)
    check("fork(2, 3)")
    # the fork detached slot 2: its positions 1..P are its own again, and the prefix can be replaced
    b.forward([2], [77], [4], want_argmax=False)
    b.set_prefix(0)
    assert b.prefix_len == 0
    b.close()
