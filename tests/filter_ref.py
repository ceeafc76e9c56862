"""numpy restatement of the truncated sampler's rule (llm.f90_amd/csrc/sample_filter.h, include/llmk.h llmk_decode_sample_ex),
by sort and cumulative sum in float64:

    s = z * invT (f32),  m = max s,  e = exp(s - m)
    top-k : tau_k = the k-th largest logit counting duplicates (ties all kept); off at k = 0 or k >= the number of non-NaN rows
    top-p : row kept iff G(z) < top_p * S,  S = sum of e over z >= tau_k,  G(t) = sum of e over z > t;  off at exactly 1
    min-p : row kept iff e >= min_p;  off at 0
    kept  = { i : z[i] >= tau },  tau = max of the three;  token = 1 + first argmax of sample_ref's score over the kept rows

The header floors e * 2^32 to integers and compares those; here the masses stay real numbers, so a vector is SAFE to compare only
if no row's nucleus mass G / S lies within 1e-5 of top_p and no e[i] within 1e-5 * min_p of min_p (the floors move G / S by at most
V * 2^-32 < 1e-5 for V <= 32,000, expf's rounding by ~1e-7).

An unsafe vector still bounds the kept set: every threshold the two margins admit lies between a lowest and a highest one, so the
kept set lies between rule().lo (the widest) and rule().hi (the narrowest), lo >= mask >= hi, all three equal on a safe vector.
Kept sets are nested threshold sets, so a first-maximum pick over lo that lies in hi is the pick of every set in between:
sample_window() says whether the pick is decided in that sense.  At V = 32,000 a model's flat logits put a thousand rows near
min_p and one vector in 25 is unsafe, yet the pick is decided on nearly all of them."""
from types import SimpleNamespace

import numpy as np

import sample_ref

MARGIN = 1e-5


def rule(logits, T: float, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0):
    """-> mask (kept rows), kept, tau (f32; +inf when there is no token), safe"""
    z = np.array(logits, np.float32)
    z[z == 0] = np.float32(0.0)                               # -0.0 counts as +0.0
    V = z.size
    valid = ~np.isnan(z)
    out = SimpleNamespace(mask=np.zeros(V, bool), kept=0, tau=np.float32(np.inf), safe=True)
    out.lo = out.hi = out.mask
    if not valid.any() or z[valid].max() == -np.inf:
        return out
    zmax = z[valid].max()
    invT = sample_ref.inv_temperature(T)
    top_p, min_p = np.float32(top_p), np.float32(min_p)
    with np.errstate(over="ignore", invalid="ignore"):
        s = (z * invT).astype(np.float32)
        m = np.float32(zmax * invT)
        if not np.isfinite(m):
            tau = zmax
        else:
            e = np.exp((s - m).astype(np.float32).astype(np.float64))
            e[~valid] = 0.0
            tau = np.float32(-np.inf)
            zs = np.sort(z[valid])[::-1]
            k_on = 1 <= top_k < zs.size
            tau_k = zs[top_k - 1] if k_on else np.float32(-np.inf)
            tau = tau_lo = tau_hi = max(tau, tau_k)
            if top_p < 1:
                order = np.argsort(-z[valid], kind="stable")
                zd, ed = z[valid][order], e[valid][order]
                S = ed[zd >= tau_k].sum()
                before = np.concatenate([[0.0], np.cumsum(ed)[:-1]])
                first = np.concatenate([[True], zd[1:] != zd[:-1]])       # the first row of each distinct value: G = the mass before it
                vals, G = zd[first], before[first]
                keep = G < float(top_p) * S
                tau = max(tau, vals[keep].min())
                tau_lo = max(tau_lo, vals[G < (float(top_p) + MARGIN) * S].min())
                tau_hi = max(tau_hi, vals[(G < (float(top_p) - MARGIN) * S) | (vals == zmax)].min())
                inset = vals >= tau_k
                out.safe &= bool((np.abs(G[inset] / S - float(top_p)) > MARGIN).all())
            if min_p > 0:
                tau = max(tau, z[valid & (e >= float(min_p))].min())
                tau_lo = max(tau_lo, z[valid & (e >= float(min_p) * (1 - MARGIN))].min())
                tau_hi = max(tau_hi, z[valid & ((e > float(min_p) * (1 + MARGIN)) | (z == zmax))].min())
                out.safe &= bool((np.abs(e[valid] - float(min_p)) > MARGIN * float(min_p)).all())
    out.tau = np.float32(tau)
    out.mask = valid & (z >= tau) & (z > -np.inf)
    out.kept = int(out.mask.sum())
    if np.isfinite(m):
        out.lo, out.hi = valid & (z >= tau_lo) & (z > -np.inf), valid & (z >= tau_hi) & (z > -np.inf)
    else:
        out.lo = out.hi = out.mask
    return out


def _pick(logits, T, seed, pos, mask):
    """-> (0-based first argmax of sample_ref's score over mask, relative margin between the top two scores there)"""
    with np.errstate(over="ignore", invalid="ignore"):
        sc = sample_ref.scores(logits, T, seed, pos).astype(np.float64)
    sc[~mask] = -np.inf
    j = int(np.argmax(sc))
    if int(mask.sum()) == 1:
        return j, np.inf
    top2 = np.partition(sc, -2)[-2:]
    return j, (top2[1] - top2[0]) / max(abs(top2[1]), 1.0)


def sample(logits, T: float, seed: int, pos: int, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0):
    """-> (1-based token or 0, relative margin between the top two scores among the kept rows, the rule() result)"""
    r = rule(logits, T, top_k, top_p, min_p)
    if r.kept == 0:
        return 0, np.inf, r
    j, margin = _pick(logits, T, seed, pos, r.mask)
    return j + 1, margin, r


def sample_window(logits, T: float, seed: int, pos: int, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0):
    """-> (1-based token or 0, margin, decided, the rule() result): the pick and the margin over the widest kept set the margins
    admit (r.lo); decided when that row is also in the narrowest (r.hi), so that every admissible kept set has this pick and at
    least this margin.  On a safe vector this is sample() with decided = True."""
    r = rule(logits, T, top_k, top_p, min_p)
    if r.kept == 0:
        return 0, np.inf, True, r
    j, margin = _pick(logits, T, seed, pos, r.lo)
    return j + 1, margin, bool(r.hi[j]), r


# ---- the seeded logit vectors and sampler settings both test files run (CPU: the header on the host; GPU: llmk_sample_logits)
def vectors(V: int, seed: int):
    """[(name, logits)]: flat, peaked (one row +20), two-level with exact ties, -inf / NaN rows, a tie at the maximum for top_p to land in"""
    rng = np.random.default_rng([20261018, V, seed])
    smooth = (2.5 * rng.standard_normal(V)).astype(np.float32)
    # Above a few dozen rows a continuous vector has rows of mass below 1e-5 wherever a large top_p lands, and no such vector is safe to
    # compare: there the flat family sits on a grid of 0.137 (a few hundred distinct values with many ties each; the step is no power
    # of two, so every byte of the keys still varies).  The peaked family stays continuous at every size.
    flat = smooth if V < 100 else (np.round(smooth / np.float32(0.137)) * np.float32(0.137)).astype(np.float32)
    peaked = smooth.copy()
    peaked[rng.integers(V)] += np.float32(20)
    two = np.zeros(V, np.float32)
    idx = rng.permutation(V)
    two[idx[:5]] = 2.0
    two[idx[5:15]] = 1.0
    two[idx[15]] = -0.0
    nonfin = flat.copy()
    hole = rng.permutation(V)
    nonfin[hole[:V // 10]] = -np.inf
    nonfin[hole[V // 10:V // 5]] = np.nan
    tied = (flat - np.float32(3)).astype(np.float32)
    tied[idx[:2]] = 6.0                                        # two rows share the maximum: a small top_p lands between them
    return [("flat", flat), ("peaked", peaked), ("two-level", two), ("nonfinite", nonfin), ("tied-max", tied)]


def settings(V: int):
    """[(top_k, top_p, min_p)]: each filter alone over its values, then combinations"""
    s = [(0, 1.0, 0.0)]
    s += [(k, 1.0, 0.0) for k in (1, 2, 40, V, V + 5)]
    s += [(0, p, 0.0) for p in (0.1, 0.9, 0.999)]
    s += [(0, 1.0, m) for m in (0.05, 0.5)]
    s += [(40, 0.9, 0.0), (40, 0.95, 0.05), (5, 0.5, 0.1), (0, 0.9, 0.1), (10, 0.1, 0.0), (2, 0.999, 0.5)]
    return s


def cases(Vs, seeds=(0, 1)):
    """every vector x every setting: dicts with name, z, T, seed, pos, top_k, top_p, min_p"""
    out = []
    for V in Vs:
        for sd in seeds:
            for vi, (name, z) in enumerate(vectors(V, sd)):
                for si, (k, p, m) in enumerate(settings(V)):
                    T = (0.9, 1.0, 0.5)[(vi + si + sd) % 3]
                    out.append(dict(name=f"{name}-V{V}-s{sd}-k{k}-p{p}-m{m}-T{T}", z=z, T=T, seed=1000 * sd + 17 * si + vi, pos=1 + (si * 7 + vi) % 97,
                                    top_k=k, top_p=p, min_p=m))
    return out
