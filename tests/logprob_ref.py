"""numpy restatement of the decode log-probs rule (llm.f90_amd/csrc/logprob.h, include/llmk.h llmk_decode_sample_lp), in float64:

    L              = score_ref.lse(z)                       z: the V raw logits of the position
    token_logprob  = z[id - 1] - L                          0.0 for id == 0
    alternatives   : the rows with z > -inf that are not NaN, by z descending then index ascending (np.lexsort on (index, -z); -0.0
                     and +0.0 tie); entry j < top_n is the j-th of them, {1-based id, z - L}; {0, -inf} past the last one

A NaN (or +inf) logit makes L, and with it every value, NaN here; the header's L is then whatever score.h's steps and merges give in
the kernel's order (NaN, except where the NaN is the first thing an empty state meets: that state stays empty and drops it).  Only
the ids are defined for such a vector, and only they are compared."""
import numpy as np

import filter_ref
import score_ref

MAX_TOP = 20
BAR = 2.0 ** -20      # |value - ref| <= BAR * max(1, |L|, max finite |z|): the bar for hook and host comparisons against float64


def rule(logits, token: int, top_n: int):
    """-> (token_logprob float64, top_tokens [top_n] int32, top_logprobs [top_n] float64, L float64)"""
    z32 = np.asarray(logits, np.float32)
    z = z32.astype(np.float64)
    with np.errstate(invalid="ignore"):
        L = float(score_ref.lse(z)[0])
        rows = np.flatnonzero(z > -np.inf)                       # (False for NaN)
        order = rows[np.lexsort((rows, -z[rows]))][:top_n]
        toks = np.zeros(top_n, np.int32)
        vals = np.full(top_n, -np.inf, np.float64)
        toks[:len(order)] = order + 1
        vals[:len(order)] = z[order] - L
        tlp = float(z[token - 1] - L) if token > 0 else 0.0
    return tlp, toks, vals, L


def scale(logits, L: float) -> float:
    """what the bar is relative to: max(1, |L|, the largest finite |z|)"""
    z = np.asarray(logits, np.float64)
    fin = np.abs(z[np.isfinite(z)])
    return max(1.0, abs(L) if np.isfinite(L) else 0.0, float(fin.max()) if fin.size else 0.0)


def check(name, logits, token, top_n, got_tlp, got_toks, got_vals, host=None):
    """ids and padding exact, values within the bar; returns the largest error in units of the bar.  Where the float64 reference is
    NaN (a NaN / +inf logit) the value is what score.h's arithmetic gives in the kernel's order: with `host` = (token_logprob,
    top_logprobs) of llmk_logprob_rule on the same vector, a value must be NaN exactly where the host rule's is, and within twice the
    bar of it where it is not (both sides within the bar of the same real number; the scale from |L| <= |z| + |z - L|)"""
    tlp, toks, vals, L = rule(logits, token, top_n)
    assert np.array_equal(np.asarray(got_toks)[:top_n], toks), (name, np.asarray(got_toks)[:top_n].tolist(), toks.tolist())
    bar = BAR * scale(logits, L)
    got = np.concatenate([[got_tlp], np.asarray(got_vals, np.float64)[:top_n]])
    ref = np.concatenate([[tlp], vals])
    worst = 0.0
    hv = None if host is None else np.concatenate([[host[0]], np.asarray(host[1], np.float64)[:top_n]])
    for j, (g, r) in enumerate(zip(got, ref)):
        if np.isnan(r):
            if hv is not None:
                assert np.isnan(g) == np.isnan(hv[j]), (name, g, hv[j])
                if not np.isnan(g):
                    fin = np.abs(np.asarray(logits, np.float64)[np.isfinite(logits)])
                    assert g == hv[j] or abs(g - hv[j]) <= 2 * BAR * max(1.0, float(fin.max()) + abs(hv[j])), (name, g, hv[j])
        elif np.isinf(r):
            assert g == r, (name, g, r)
        else:
            assert abs(g - r) <= bar, (name, g, r, bar)
            worst = max(worst, abs(g - r) / bar)
    return worst


# ---- the logit vectors both test files run (CPU: the header on the host; GPU: llmk_logprob_logits)
def vectors(V: int):
    """[(name, logits, token)]: filter_ref's families, all rows equal, 30 rows tied at the maximum (straddles top_n = 20), +-0.0 ties,
    all but 5 rows at -inf (padding), no row above -inf"""
    rng = np.random.default_rng([20261101, V])
    out = []
    for sd in (0, 1):
        for name, z in filter_ref.vectors(V, sd):
            ok = np.flatnonzero(np.isfinite(z))
            out.append((f"{name}-s{sd}", z, int(ok[rng.integers(len(ok))]) + 1))
    out.append(("all-equal", np.full(V, 1.5, np.float32), V))
    base = (2.5 * rng.standard_normal(V)).astype(np.float32)
    tied = base.copy()
    tied[rng.permutation(V)[:30]] = np.float32(base.max() + 1)
    out.append(("30-tied-at-max", tied, int(np.argmax(tied)) + 1))
    zeros = (-np.abs(base) - np.float32(0.5)).astype(np.float32)      # every other row below zero: the zeros are the top of the list
    idx = np.sort(rng.permutation(V)[:12])
    zeros[idx[0::2]] = np.float32(-0.0)
    zeros[idx[1::2]] = np.float32(0.0)
    out.append(("signed-zero-ties", zeros, int(idx[3]) + 1))
    few = np.full(V, -np.inf, np.float32)
    keep = rng.permutation(V)[:5]
    few[keep] = base[keep]
    out.append(("all-but-5-minus-inf", few, int(keep[2]) + 1))
    out.append(("no-token", base, 0))
    out.append(("nothing-listable", np.full(V, -np.inf, np.float32), 0))
    return out
