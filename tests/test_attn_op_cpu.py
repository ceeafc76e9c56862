"""tests/attn_op_ref.py without a GPU: attn_op is the float64 pass's layer attention, classify names the five classes of the
non-finite rule and attn_op's NaN pattern follows the rule for each, and the poison construction reaches every class in float32."""
import numpy as np
import pytest

import attn_op_ref as ao
from llm_f90_amd.tools import gguf
from ref_pass import RefPass


def test_attn_op_is_the_float64_passes_layer_attention():
    s = gguf.LlamaShape(96, 64, 1, 6, 2, 300, 40)      # hs 16, kv_mul 3
    fw = gguf.synth_fused(s, 77)
    tokens = np.random.default_rng(5).integers(1, s.vocab_size + 1, 40)
    kept = {}
    RefPass(fw).feed(tokens, tap=lambda l, name, a: kept.__setitem__(name, a))
    worst = 0.0
    for i in range(len(tokens)):
        out = ao.attn_op(kept["q"][i], kept["k"][:i + 1], kept["v"][:i + 1], 3)
        assert out.dtype == np.float64 and out.shape == (6, 16)
        worst = max(worst, float(np.abs(out.reshape(-1) - kept["xb"][i]).max()))
    print(f"max |attn_op - RefPass xb| = {worst:.2e}")
    assert worst <= 1e-12


def _hand(s0, s1):
    """q, K of one head of size 4 whose two visible scores are s0 and s1 (times 2 = sqrt(hs)): q = e0, K rows (2 s, 0, 0, 0)"""
    q = np.array([[1, 0, 0, 0]], np.float32)
    K = np.zeros((2, 1, 4), np.float32)
    K[:, 0, 0] = [2 * s0, 2 * s1]
    return q, K


V2 = np.array([[[1, 2, 3, 4]], [[5, 6, 7, 8]]], np.float32)


@pytest.mark.parametrize("s0,s1,cls,out", [
    (np.nan, 1.0, "nan", [np.nan] * 4),
    (np.inf, 1.0, "+inf", [np.nan] * 4),
    (np.inf, -np.inf, "+inf", [np.nan] * 4),
    (-np.inf, -np.inf, "all-inf", [np.nan] * 4),
    (-np.inf, 1.0, "some-inf", [5, 6, 7, 8]),
    (0.0, 0.0, "finite", [3, 4, 5, 6]),
])
def test_classify_names_the_class_and_attn_op_follows_the_rule(s0, s1, cls, out):
    q, K = _hand(np.float32(s0), np.float32(s1))
    assert ao.classify(q, K, 1) == [cls]
    got = ao.attn_op(q, K, V2, 1)[0]
    assert np.array_equal(np.isnan(got), np.isnan(out))
    assert np.array_equal(got[~np.isnan(got)], np.array(out, np.float64)[~np.isnan(out)])


def test_a_weight_of_zero_times_a_non_finite_v_element_is_nan_in_that_element_only():
    q, K = _hand(np.float32(-np.inf), np.float32(1.0))
    V = V2.copy()
    V[0, 0, 2] = np.inf
    got = ao.attn_op(q, K, V, 1)[0]
    assert np.array_equal(np.isnan(got), [False, False, True, False]) and np.array_equal(got[[0, 1, 3]], [5, 6, 8])
    V[0, 0, 2], V[1, 0, 2] = 3, -np.inf         # a positive weight: the infinity itself
    assert ao.attn_op(q, K, V, 1)[0][2] == -np.inf


def test_assert_modest_refuses_a_large_finite_element():
    ao.assert_modest(np.array([1.0, -np.inf, np.nan, 999.0], np.float32))
    with pytest.raises(AssertionError):
        ao.assert_modest(np.array([2e3], np.float32))


@pytest.mark.parametrize("layout", list(ao.POISON_LAYOUTS))
@pytest.mark.parametrize("hs", [16, 64])
def test_the_poison_construction_reaches_every_class_in_float32(hs, layout):
    fw, tokens = ao.build_poison(hs, layout)
    kept = {}
    with np.errstate(all="ignore"):
        RefPass(fw, np.float32).feed(tokens, tap=lambda l, name, a: kept.__setitem__(name, a))
    q, k, v = kept["q"], kept["k"], kept["v"]
    assert q.dtype == np.float32
    ao.assert_modest(q, k, v)
    seen, by_head = set(), {}
    for i in range(len(tokens)):
        cls = ao.classify(q[i], k[:i + 1], 4)
        out = ao.attn_op(q[i], k[:i + 1], v[:i + 1], 4)
        for h, c in enumerate(cls):
            seen.add((c, bool(np.isfinite(out[h]).all())))
            by_head.setdefault(h, set()).add(c)
            assert np.isnan(out[h]).all() == (c in ("nan", "+inf", "all-inf")), (i + 1, h, c)
    print({h: sorted(c) for h, c in by_head.items()})
    ao.coverage(seen)
    # the heads the construction aims: 0 meets +inf, 1 a -inf beside finite scores, 2 a NaN, 4 nothing but -inf; kv group 1 has finite K
    assert "+inf" in by_head[0] and "some-inf" in by_head[1] and "nan" in by_head[2] and "all-inf" in by_head[4]
    assert all(by_head[h] == {"finite"} for h in (5, 6, 7)) and by_head[4] == {"finite", "all-inf"}
    assert np.isfinite(k[:, 1]).all()
    # position 79: the newest row's V element D1 of kv head 1 is +inf and every head of the group has finite scores -- the plain
    # softmax gives +inf there and finite values elsewhere
    last = ao.attn_op(q[-1], k, v, 4)
    assert v[-1, 1, ao.POISON_D1] == np.inf and np.isfinite(np.delete(v[:, 1], ao.POISON_D1, axis=1)).all()
    for h in range(4, 8):
        assert last[h, ao.POISON_D1] == np.inf and np.isfinite(np.delete(last[h], ao.POISON_D1)).all()
    if layout == "late":        # position 17: head 2's only NaN score is alone in tile 1, every score of tile 0 is finite
        s17 = ao.scores(q[16], k[:17], 4)[2]
        assert np.isnan(s17[16]) and np.isfinite(s17[:16]).all()
