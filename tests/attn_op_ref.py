"""TEST INFRASTRUCTURE -- decode attention as an operator: the float64 softmax of ONE layer's q, K and V, for checks that cost O(rows)
per query where the float64 pass (tests/ref_pass.py) costs a whole model, and that still mean something when scores are not finite.

On the multi-kernel path d_xb is written only by the attention launch, so after llmk_forward(tok, pos) llmk_peek 1 and 2 hold the
LAST layer's rotated q and its attention output, and llmk_peek 4 and 5 that layer's K / V rows: a test compares the device's output
with attn_op of the device's own inputs.  One-layer models (the needles of attn_needle.shape_needles sit in layer 0) make that layer
the one under test.

The non-finite rule of csrc/attn_split.h is the plain softmax's, so attn_op special-cases nothing: the max of a row with a NaN is NaN,
inf - inf is NaN, all -inf gives -inf - -inf, exp(-inf) is exactly 0, and 0 * inf in e V is NaN in that element only.  (Products are
taken element by element and summed, not handed to a BLAS, whose treatment of a zero factor is its own.)

shape_poison / poison_sequence build the model and the sequence that put every class of classify() in front of a kernel at once.
Used by tests/test_attn_op_cpu.py (is the helper right, does the construction reach every class?) and tests/test_attn_split_op_gpu.py."""
from __future__ import annotations

import numpy as np

from llm_f90_amd.tools import gguf

CLASSES = ("nan", "+inf", "all-inf", "some-inf", "finite")
MODEST = 1e3        # every finite element of q, K and V is below this, so no finite f32 dot product overflows where float64 does not


def scores(q, K, kv_mul: int):
    """float64 scores [nh][n] of q [nh][hs] against K [n][nkv][hs] (or [n][kv_dim]): s = K_g q / sqrt(hs), g = h / kv_mul"""
    q = np.asarray(q, np.float64)
    nh, hs = q.shape
    K = np.asarray(K, np.float64).reshape(len(K), -1, hs)
    with np.errstate(all="ignore"):
        return np.stack([(K[:, h // kv_mul] * q[h]).sum(axis=1) / np.sqrt(np.float64(hs)) for h in range(nh)])


def attn_op(q, K, V, kv_mul: int):
    """q [nh][hs], K and V [n][nkv][hs] as peeked -> the attention output [nh][hs] in float64: per head e = exp(s - max s),
    out = e V / sum e"""
    q = np.asarray(q, np.float64)
    nh, hs = q.shape
    V = np.asarray(V, np.float64).reshape(len(V), -1, hs)
    s = scores(q, K, kv_mul)
    out = np.empty((nh, hs), np.float64)
    with np.errstate(all="ignore"):
        for h in range(nh):
            e = np.exp(s[h] - s[h].max())
            out[h] = (e[:, None] * V[:, h // kv_mul]).sum(axis=0) / e.sum()
    return out


def classify(q, K, kv_mul: int):
    """per head, what its visible float64 scores hold: "nan" (some score is NaN), "+inf" (none is NaN, one is +inf), "all-inf"
    (every score is -inf), "some-inf" (a -inf beside finite ones) or "finite".  The first three give a NaN output."""
    out = []
    for s in scores(q, K, kv_mul):
        if np.isnan(s).any():
            out.append("nan")
        elif (s == np.inf).any():
            out.append("+inf")
        elif (s == -np.inf).all():
            out.append("all-inf")
        elif (s == -np.inf).any():
            out.append("some-inf")
        else:
            out.append("finite")
    return out


def assert_modest(*arrays):
    """every element is modest or exactly +-inf / NaN: f32 and float64 scores fall into the same class"""
    for a in arrays:
        a = np.asarray(a)
        fin = np.isfinite(a)
        assert (np.abs(a[fin]) < MODEST).all(), float(np.abs(a[fin]).max())


def peek_rows(m, layer: int, n: int, kv_dim: int, first: int = 1):
    """K and V rows first .. n (positions, 1-based) of `layer` as two f32 arrays [n - first + 1][kv_dim]"""
    K = np.stack([m.peek(4, kv_dim, layer, pos) for pos in range(first, n + 1)])
    V = np.stack([m.peek(5, kv_dim, layer, pos) for pos in range(first, n + 1)])
    return K, V


# ------------------------------------------------------------------------------------------------
# the poison model: every class at once
# ------------------------------------------------------------------------------------------------
BIG = np.float32(3e38)      # times 1 / rms(token) ~ 1.7 it overflows f32: +-inf in q, K or V for a token whose feature is 1, exactly 0 else
POISON_A = np.float32(4.0)
POISON_S = 80               # seq_len of the poison contexts
POISON_N = 79               # positions fed: the last one is no multiple of the 16-row tile
# cache row (0-based) -> kind.  "k": the token's K row of kv head 0 is +inf in the lowest-frequency RoPE pair (and, as a query, head 4's
# pair is -inf); "kv": that, and element POISON_D0 of its V row of kv head 0 is +inf; "v1": element POISON_D1 of its V row of kv head 1
# is +inf and nothing else -- the newest row of the last position, with finite scores in every head of that group.
# Rows 5 and 70 are the last row of a ragged tile when they are the query; 15 | 16 and 31 | 47 end and begin tiles; rows 48 .. 69 are
# fillers: tile 3 (rows 48 .. 63) is finite as a whole.  Positions 6 .. 16 see K poison only: head 1's output is finite throughout there.
POISON_ROWS = {5: "k", 15: "k", 16: "kv", 31: "kv", 47: "k", 70: "k", POISON_N - 1: "v1"}
# The same with the FIRST poison in row 16: at position 17 head 2's NaN score stands alone in its tile -- the wave that meets it has
# seen nothing finite (attn_tiles' STRICT) -- while the wave of tile 0 has finite scores only; row 32 likewise behind a finite tile 1.
POISON_ROWS_LATE = {16: "k", 32: "kv", POISON_N - 1: "v1"}
POISON_LAYOUTS = {"rows": POISON_ROWS, "late": POISON_ROWS_LATE}
POISON_D0, POISON_D1 = 3, 5
POISON_FEATURE = {"k": (1,), "kv": (1, 2), "v1": (3,)}
NRES = 4                    # reserved embedding dims: 0 is 1 for every token, 1 .. 3 are the kinds' features


def poison_shape(hs: int, kv_mul: int = 4, nkv: int = 2):
    return gguf.LlamaShape(hs * kv_mul * nkv, 64, 1, kv_mul * nkv, nkv, 320, POISON_S)


def poison_sequence(shape, seed: int, rows=None):
    """tokens (1-based ids) of POISON_N positions: a token of its own at every row of `rows` (POISON_ROWS; ids 3, 4, ..), fillers from
    the ids behind them elsewhere; and {kind: [ids]}"""
    rows = POISON_ROWS if rows is None else rows
    rng = np.random.default_rng(seed)
    tokens = rng.integers(3 + len(rows), shape.vocab_size + 1, POISON_N).astype(np.int32)
    kinds = {k: [] for k in POISON_FEATURE}
    for i, (row, kind) in enumerate(sorted(rows.items())):
        tokens[row] = 3 + i
        kinds[kind].append(3 + i)
    return tokens, kinds


def shape_poison(fw, kinds):
    """Edit one-layer f32 FusedWeights (kv_mul 4, two kv heads) so that at one position the query heads of kv group 0 fall into
    different classes; returns fw.  Nothing but the rows named here reads the reserved dims.  pr = hs - 2, the first row of the
    lowest-frequency RoPE pair (it turns by < 0.02 rad over the context, so both elements of a rotated (x, 0) have the sign of x and
    both of a rotated (a, a) stay positive):
      K of kv head 0: row pr reads dim 1 with gain BIG and nothing else, row pr + 1 is zero -> (+inf, +inf) at "k" / "kv" rows, (0, 0) else;
      q head 0 pair (+a, 0) of dim 0 -> +inf at those rows: NaN output;  head 1 (-a, 0) -> -inf beside finite scores: weight exactly 0;
      head 2 (0, 0) -> 0 * inf: a NaN score;  head 3 keeps its weights (a random pair: +-inf or NaN);
      K of kv head 1: the pair reads dim 0 as (a, a) for every token; q head 4 row pr reads dim 1 with gain -BIG -> (-inf, -inf) when the
      query is a "k" / "kv" token: every visible score is -inf; heads 5 .. 7 keep their weights and kv head 1 has finite K throughout;
      V of kv head 0, element D0, reads dim 2 with gain BIG (on top of its weights): +inf at "kv" rows -- 0 * inf = NaN in that element
      only for head 1; V of kv head 1, element D1, reads dim 3 likewise: +inf in the "v1" row."""
    assert fw.ggml_type == gguf.GGML_F32
    s = fw.shape
    E, KV, hs, nh, nkv = s.emb_dim, s.kv_dim, s.head_size, s.n_heads, s.n_kv_heads
    assert s.n_layers == 1 and nkv == 2 and nh == 8
    emb = np.array(fw.token_embedding_table, np.float32, copy=True)
    emb[:, :NRES] = 0
    emb[:, 0] = 1.0
    for kind, ids in kinds.items():
        for tk in ids:
            emb[tk - 1, list(POISON_FEATURE[kind])] = 1.0
    fw.token_embedding_table = emb
    w = np.array(fw.wqkv, np.float32, copy=True)
    w[0, :, :NRES] = 0
    pr, a = hs - 2, POISON_A
    for row in (0 * hs + pr, 1 * hs + pr, 2 * hs + pr, 4 * hs + pr, E + pr, E + hs + pr):
        w[0, row:row + 2] = 0
    w[0, 0 * hs + pr, 0] = a
    w[0, 1 * hs + pr, 0] = -a
    w[0, 4 * hs + pr, 1] = -BIG
    w[0, E + pr, 1] = BIG
    w[0, E + hs + pr, 0] = a
    w[0, E + hs + pr + 1, 0] = a
    w[0, E + KV + POISON_D0, 2] = BIG
    w[0, E + KV + hs + POISON_D1, 3] = BIG
    fw.wqkv = w
    fw.rms_att_weight = np.array(fw.rms_att_weight, np.float32, copy=True)
    fw.rms_att_weight[0, :NRES] = 1.0
    return fw


def build_poison(hs: int, layout: str = "rows"):
    """(weights, tokens) of the poison case of head size hs with the poison rows POISON_LAYOUTS[layout]"""
    s = poison_shape(hs)
    tokens, kinds = poison_sequence(s, 20261127, POISON_LAYOUTS[layout])
    return shape_poison(gguf.synth_fused(s, 4242), kinds), tokens


def coverage(seen):
    """the guard of the non-finite tests: `seen` = {(class, output wholly finite?)} over all (head, position); every class must occur,
    "some-inf" with a finite output at least once"""
    missing = [c for c in CLASSES if not any(k == c for k, _ in seen)]
    assert not missing, f"the construction never reaches {missing}"
    assert ("some-inf", True) in seen, "no head with a -inf score beside finite ones has a wholly finite output"
