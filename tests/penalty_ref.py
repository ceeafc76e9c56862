"""numpy float32 restatement of steps 1 and 2 of the penalty rule (llm.f90_amd/csrc/sample_penalty.h, include/llmk.h
llmk_decode_sample_pen), one rounded operation per line:

    bias       z[t] <- z[t] + b                                   for every entry (t, b) of the bias list (t 1-based)
    penalties  z[t] <- z[t] * inv_r  if z[t] > 0  else  z[t] * r   for every t that occurs c[t] > 0 times in the window
               z[t] <- z[t] - (f32(c[t]) * f + p)
    window     the tokens fed at positions max(1, pos - last_n + 1) .. pos according to hist (hist[q - 1] = the token fed at
               position q, 0 = none);  inv_r = f32(1 / r)

Every operation is a correctly rounded IEEE float32 operation on both sides, so the adjusted vector is compared bit for bit.  Step 3
is filter_ref.sample on the adjusted vector (sample())."""
import numpy as np

import filter_ref

MAX_LOGIT_BIAS = 256
THREADS = 256                     # sample_penalty_kernel's workgroup (kernels.h SP_THREADS): one case has a longer window


def inv_repeat(repeat: float):
    return np.float32(1.0) / np.float32(repeat)


def window(hist, pos: int, last_n: int):
    """the recorded tokens of the window of `pos`, "none" entries dropped"""
    if last_n <= 0:
        return np.zeros(0, np.int64)
    lo = max(1, pos - last_n + 1)
    w = np.asarray(hist, np.int64)[lo - 1:pos]
    return w[w != 0]


def adjust(z, hist, pos: int, last_n: int = 0, repeat: float = 1.0, frequency: float = 0.0, presence: float = 0.0, bias=()):
    """-> the adjusted logits (float32)"""
    z = np.array(z, np.float32)
    r, inv_r = np.float32(repeat), inv_repeat(repeat)
    f, p = np.float32(frequency), np.float32(presence)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for t, b in bias:
            z[t - 1] = np.float32(z[t - 1] + np.float32(b))
        toks, cnt = np.unique(window(hist, pos, last_n), return_counts=True)
        for t, c in zip(toks.tolist(), cnt.tolist()):
            v = z[t - 1]
            s = np.float32(v * inv_r) if v > 0 else np.float32(v * r)
            cf = np.float32(np.float32(c) * f)
            d = np.float32(cf + p)
            z[t - 1] = np.float32(s - d)
    return z


def sample(z, hist, pos, T, seed, top_k=0, top_p=1.0, min_p=0.0, **pen):
    """-> (1-based token or 0, margin, the filter_ref.rule() result, the adjusted logits)"""
    adj = adjust(z, hist, pos, **pen)
    tok, margin, r = filter_ref.sample(adj, T, seed, pos, top_k, top_p, min_p)
    return tok, margin, r, adj


def same_bits(a, b) -> bool:
    """bit for bit, NaN positions matching as NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# ---- the cases both test files run (CPU: the header on the host; GPU: llmk_set_history + llmk_sample_logits_pen) ------------------
SAMPLERS = [(40, 0.9, 0.0), (0, 1.0, 0.0), (1, 1.0, 0.0), (0, 0.9, 0.05), (5, 0.5, 0.0)]
PENALTIES = [dict(repeat=1.1, frequency=0.2, presence=0.1), dict(repeat=1.3, frequency=0.0, presence=0.0),
             dict(repeat=1.0, frequency=0.5, presence=0.0), dict(repeat=1.0, frequency=0.0, presence=0.7),
             dict(repeat=0.8, frequency=-0.1, presence=-0.2)]


def _special_rows(z):
    """one row each, where the vector has one: +0.0, -0.0, negative, positive, -inf, NaN (0-based)"""
    sign = np.signbit(z)
    picks = [np.flatnonzero((z == 0) & ~sign), np.flatnonzero((z == 0) & sign), np.flatnonzero(z < 0), np.flatnonzero(z > 0),
             np.flatnonzero(np.isneginf(z)), np.flatnonzero(np.isnan(z))]
    return [int(p[0]) for p in picks if p.size]


def windows(V: int, z, rng, long_S: int):
    """[(name, hist, pos, last_n)]: hist holds `pos` entries (1-based ids, 0 = none)"""
    out = []
    d = rng.permutation(V)[:40] + 1                                    # distinct tokens
    out.append(("empty", np.zeros(12, np.int64), 12, 8))
    h = np.zeros(12, np.int64)
    h[9] = d[0]
    out.append(("one", h, 12, 8))
    out.append(("identical", np.full(20, d[1], np.int64), 20, 16))     # c = last_n
    h = d[:16].copy()
    h[[2, 7, 13]] = d[20]
    out.append(("thrice", np.concatenate([d[24:30], h]), 22, 16))      # the six tokens in front lie outside the window
    h = d[:16].copy()
    h[[0, 5, 6, 15]] = 0
    h[9] = h[3]
    out.append(("with-none", h, 16, 16))
    out.append(("pos-below-last_n", d[:5].copy(), 5, 16))
    sp = np.array(_special_rows(z), np.int64) + 1
    out.append(("special-rows", np.concatenate([sp, sp[:2], d[:3]]), len(sp) + min(2, len(sp)) + 3, 64))
    h = rng.integers(1, V + 1, long_S).astype(np.int64)                # longer than the kernel's workgroup, repeats throughout
    h[rng.integers(0, long_S, long_S // 10)] = 0
    out.append(("long", h, long_S, long_S))
    return out


def bias_lists(V: int, z, hist, rng):
    """[(name, [(token, bias)])]"""
    inwin = [int(t) for t in hist if t != 0][:1]
    valid = np.where(np.isnan(z), -np.inf, z)
    top = int(np.argmax(valid)) + 1
    many = (rng.permutation(V)[:MAX_LOGIT_BIAS] + 1).tolist()
    vals = (3.0 * rng.standard_normal(MAX_LOGIT_BIAS)).astype(np.float32).tolist()
    return [("none", []),
            ("in-window", [(t, 1.5) for t in inwin] + [(top, -2.0)] if inwin and inwin[0] != top else [(top, -2.0)]),
            ("ban-max", [(top, -np.inf)]),
            ("full", list(zip(many, vals)))]


def cases(Vs, long_S: int = 300, seeds=(0,)):
    """every vector of filter_ref.vectors x every window x every bias list, penalties and samplers cycling:
    dicts with name, z, hist, pos, last_n, repeat, frequency, presence, bias, T, seed, top_k, top_p, min_p, banned"""
    out = []
    for V in Vs:
        for sd in seeds:
            rng = np.random.default_rng([20261018, V, sd, 7])
            for vi, (vname, z) in enumerate(filter_ref.vectors(V, sd)):
                for wi, (wname, hist, pos, last_n) in enumerate(windows(V, z, rng, long_S)):
                    for bi, (bname, bias) in enumerate(bias_lists(V, z, hist, rng)):
                        i = vi + wi + bi
                        k, p, m = SAMPLERS[i % len(SAMPLERS)]
                        pen = PENALTIES[(vi + 2 * wi + bi) % len(PENALTIES)]
                        out.append(dict(name=f"{vname}-V{V}-s{sd}-{wname}-{bname}", z=z, hist=hist, pos=pos, last_n=last_n, bias=bias,
                                        T=(0.9, 1.0, 0.5)[i % 3], seed=1000 * sd + 31 * wi + 7 * bi + vi, top_k=k, top_p=p, min_p=m,
                                        banned=[t for t, b in bias if b == -np.inf], **pen))
    return out


def pen_args(c):
    return dict(last_n=c["last_n"], repeat=c["repeat"], frequency=c["frequency"], presence=c["presence"], bias=c["bias"])
