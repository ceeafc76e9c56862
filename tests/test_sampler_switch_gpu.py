"""Changing the sampler on one context in mid-sequence, with no reset() in between: greedy, temperature sampling, the filters and
the penalties take turns over one sequence of 40 positions (include/llmk.h: the three tiers of llmk_forward_* / llmk_decode_*).
Every tier leaves parameter words on the device that the next call must not mistake for its own (the sampling words of the
pipelined launches, the filter's words, which the verification hook overwrites too), so the bars are: one llmk_decode_* call per
segment and a chain of per-position llmk_forward_* calls give one transcript and one token record; every id is the numpy
reference's pick (tests/sample_ref.py, filter_ref.py, penalty_ref.py) from the logits of its position; the record holds the fed
token wherever a _pen call was fed one and nothing anywhere else (the other tiers do not maintain it)."""
import numpy as np
import pytest

import filter_ref
import penalty_ref
import sample_ref
from llm_f90_amd import llmk

pytestmark = pytest.mark.gpu
T = 0.9
NINF = float("-inf")
FILTERS = dict(top_k=40, top_p=0.9)
# (tier, positions, arguments).  Segments 3 and 4 ask for the SAME filter words, and the hook runs between them with others: the
# fourth must notice that the device no longer holds what the third left there.
SEGMENTS = [
    ("greedy", 4, {}),
    ("sample", 5, dict(seed=11)),
    ("ex", 4, dict(seed=7, **FILTERS)),
    ("pen", 5, dict(seed=7, **FILTERS, last_n=16, repeat=1.1, frequency=0.2, presence=0.1, bias=[(5, NINF), (9, 1.5)])),
    ("greedy", 3, {}),
    ("ex", 5, dict(seed=7, top_k=5, min_p=0.05)),
    ("sample", 4, dict(seed=12)),
    ("pen", 5, dict(seed=7, **FILTERS, last_n=8, repeat=1.3, presence=0.5, bias=[(9, -2.0), (17, NINF), (30, 0.75)])),
    ("ex", 5, dict(seed=7)),
]
N = sum(n for _, n, _ in SEGMENTS)
HOOK_AFTER = 3                      # llmk_sample_logits between the third and the fourth segment
BOS = 2


def _decode(m, tier, tok, pos0, n, kw):
    if tier == "greedy":
        return m.decode_greedy(tok, pos0, n)
    return {"sample": m.decode_sample, "ex": m.decode_sample_ex, "pen": m.decode_sample_pen}[tier](tok, pos0, n, T, **kw)


def _forward(m, tier, tok, pos, kw):
    if tier == "greedy":
        return m.forward_greedy(tok, pos)
    return {"sample": m.forward_sample, "ex": m.forward_sample_ex, "pen": m.forward_sample_pen}[tier](tok, pos, T, **kw)


def _reference(tier, kw, lg, record, pos):
    """-> (the reference's 1-based pick from the logits of `pos`, whether it is safe to compare, the kept rows or None)"""
    if tier == "greedy":
        top2 = np.sort(lg.astype(np.float64))[-2:]
        return int(np.argmax(lg)) + 1, (top2[1] - top2[0]) / max(abs(top2[1]), 1.0) > 1e-5, None
    if tier == "sample" or (tier == "ex" and set(kw) == {"seed"}):      # all filters off: llmk_decode_sample itself
        want, margin = sample_ref.sample(lg, T, kw["seed"], pos)
        return want, margin > 1e-5, None
    if tier == "ex":
        f = {k: v for k, v in kw.items() if k != "seed"}
        want, margin, r = filter_ref.sample(lg, T, kw["seed"], pos, **f)
    else:
        p = {k: v for k, v in kw.items() if k != "seed"}
        want, margin, r, _ = penalty_ref.sample(lg, record[:pos], pos, T, kw["seed"], **p)
    return want, r.safe and margin > 1e-5, r.mask if r.safe else None


@pytest.mark.parametrize("flags", [0, llmk.FLAG_MULTI_KERNEL], ids=["persistent", "multikernel"])
def test_the_tail_changes_in_mid_sequence(flags, gguf):
    """tk-small (V = 1,024, seq_len 64).  The uncompared positions are capped like those of the transcripts of
    test_decode_sample_gpu.py and its neighbours: max(1, n // 50)."""
    fw = gguf.synth_fused(gguf.SHAPES["tk-small"], 3)
    V, S = fw.shape.vocab_size, fw.shape.seq_len
    assert N == 40 and N <= S
    path = 0 if flags else 1
    # one decode call per segment
    a = llmk.Llmk(fw, flags=flags)
    assert a.path() == path
    a.set_history([BOS], 1)
    ids, tok, pos = [], BOS, 1
    for k, (tier, n, kw) in enumerate(SEGMENTS, 1):
        ids += _decode(a, tier, tok, pos, n, kw).tolist()
        tok, pos = ids[-1], pos + n
        if k == HOOK_AFTER:
            z = np.linspace(-3.0, 3.0, V).astype(np.float32)
            r = filter_ref.sample(z, 0.5, 99, 3, top_k=3)[2]
            htok, kept, _ = a.sample_logits(z, 3, 0.5, 99, top_k=3)
            assert kept == r.kept == 3 and r.mask[htok - 1]
    assert a.path() == path
    rec_a = a.get_history(S, 1).tolist()
    a.close()
    fed = [BOS] + ids[:-1]                                            # the tokens fed at positions 1 .. N
    # the same sequence position by position
    b = llmk.Llmk(fw, flags=flags)
    b.set_history([BOS], 1)
    chain, tok, pos = [], BOS, 1
    for tier, n, kw in SEGMENTS:
        for _ in range(n):
            tok = _forward(b, tier, tok, pos, kw)
            chain.append(tok)
            pos += 1
    assert b.path() == path
    rec_b = b.get_history(S, 1).tolist()
    b.close()
    assert chain == ids
    # the record: the fed token wherever a _pen call was fed one (and what set_history put there), nothing anywhere else
    record, pos = np.zeros(S, np.int64), 1
    record[0] = BOS
    for tier, n, kw in SEGMENTS:
        if tier == "pen":
            record[pos - 1:pos - 1 + n] = fed[pos - 1:pos - 1 + n]
        pos += n
    assert rec_a == record.tolist()
    assert rec_b == record.tolist()
    # every id is the rule of its segment applied to the logits of its position
    c = llmk.Llmk(fw, flags=flags)
    pos, uncompared = 1, 0
    for tier, n, kw in SEGMENTS:
        for _ in range(n):
            lg = c.forward(fed[pos - 1], pos)
            want, safe, mask = _reference(tier, kw, lg, record, pos)
            print(f"pos {pos} {tier}: id {ids[pos - 1]} want {want} safe {safe}")
            if safe:
                assert ids[pos - 1] == want, (pos, tier, ids[pos - 1], want)
            if mask is not None:
                assert mask[ids[pos - 1] - 1], (pos, tier)
            uncompared += not safe
            pos += 1
    c.close()
    assert uncompared <= max(1, N // 50), uncompared
    assert 5 not in ids[13:18] and 17 not in ids[30:35]              # the bans of the two _pen segments
