"""llmk_forward_sample_ex / llmk_decode_sample_ex / llmk_sample_logits: top-k, top-p and min-p truncation in the device sampler
(include/llmk.h; the rule: llm.f90_amd/csrc/sample_filter.h, restated in float64 by tests/filter_ref.py).  Bars: the kernel's kept
set (count and threshold) and pick are the reference's on every vector that is safe to compare; every id of a transcript is the
reference's pick from the logits of its position; the pipelined launches and a chain of per-position calls give one transcript;
with all filters off the functions are llmk_forward_sample / llmk_decode_sample; the draws follow the softmax renormalised over the
kept rows; the CLI's --top-k / --top-p / --min-p print what the C-ABI returns."""
import os
import subprocess

import numpy as np
import pytest
from scipy.stats import chi2

import filter_ref
import sample_ref
from conftest import ROOT
from llm_f90_amd import llmk

pytestmark = pytest.mark.gpu
LLM = os.path.join(ROOT, "llm.f90_amd", "host", "llm")
T = 0.9
E_ARG, E_NONFINITE = 1, 11


def _case(name, gguf):
    """(weights, flags, whether the persistent kernel serves the ctx): the shapes of test_decode_sample_gpu.py"""
    S = gguf.SHAPES
    if name == "tk-small":
        return gguf.synth_fused(S["tk-small"], 3), 0, True
    if name == "tk-small-multikernel":
        return gguf.synth_fused(S["tk-small"], 3), llmk.FLAG_MULTI_KERNEL, False
    if name == "tiny-gqa":
        return gguf.synth_fused(S["tiny-gqa"], 1), 0, False
    if name == "tinyllama-q4_0-q6k":
        return gguf.with_q6k_classifier(gguf.synth_fused(S["tinyllama"], 20260928, 2)), 0, True
    raise KeyError(name)


# ---- the kernel on caller-supplied logits -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny-gqa", "tk-small"])
def test_sample_logits_is_the_reference_rule(name, gguf):
    """tiny-gqa: V = 300, below the workgroup's 1,024 threads; tk-small: V = 1,024"""
    fw, flags, tk = _case(name, gguf)
    m = llmk.Llmk(fw, flags=flags)
    V = fw.shape.vocab_size
    cases = filter_ref.cases((V,))
    unsafe = 0
    for c in cases:
        want, margin, r = filter_ref.sample(c["z"], c["T"], c["seed"], c["pos"], c["top_k"], c["top_p"], c["min_p"])
        tok, kept, tau = m.sample_logits(c["z"], c["pos"], c["T"], c["seed"], c["top_k"], c["top_p"], c["min_p"])
        if not r.safe:
            unsafe += 1
            continue
        assert kept == r.kept, (c["name"], kept, r.kept)
        assert np.float32(tau) == r.tau, (c["name"], tau, r.tau)
        assert r.mask[tok - 1], c["name"]
        if margin > 1e-5:
            assert tok == want, (c["name"], tok, want, margin)
        if (c["top_k"], c["top_p"], c["min_p"]) == (0, 1.0, 0.0) and not np.isnan(c["z"]).any():      # filters off: sample_ref's rule
            w0, m0 = sample_ref.sample(c["z"], c["T"], c["seed"], c["pos"])
            assert tok == w0 or m0 <= 1e-5, c["name"]
    assert unsafe <= len(cases) // 50, (unsafe, len(cases))
    # top_k = 1 is the first-maximum argmax, whatever the seed
    for vname, z in filter_ref.vectors(V, 2):
        first = int(np.flatnonzero(z == np.nanmax(z))[0]) + 1
        ties = int((z == np.nanmax(z)).sum())
        for seed in range(12):
            tok, kept, tau = m.sample_logits(z, 5, T, seed, top_k=1)
            assert kept == ties and tau == np.nanmax(z), vname
            assert (tok == first) if ties == 1 else (z[tok - 1] == np.nanmax(z)), (vname, seed)
    m.close()


def test_nonfinite_logits_and_invalid_arguments(gguf):
    fw, flags, _ = _case("tk-small", gguf)
    m = llmk.Llmk(fw, flags=flags)
    V = fw.shape.vocab_size
    for z in (np.full(V, np.nan, np.float32), np.full(V, -np.inf, np.float32)):
        with pytest.raises(llmk.LlmkError) as e:
            m.sample_logits(z, 1, T, 1, top_k=40, top_p=0.9)
        assert e.value.code == E_NONFINITE
    z = np.zeros(V, np.float32)
    z[[3, 9]] = np.inf                                          # a maximum of +inf keeps the rows equal to it
    tok, kept, tau = m.sample_logits(z, 1, T, 1, top_k=40, top_p=0.9, min_p=0.05)
    assert tok in (4, 10) and kept == 2 and tau == np.inf
    nan = float("nan")
    bad = [dict(top_k=-1), dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.5), dict(top_p=nan), dict(min_p=-0.1), dict(min_p=1.5),
           dict(min_p=nan), dict(temperature=0.0), dict(temperature=nan), dict(temperature=-1.0), dict(temperature=float("inf"))]
    ok = np.zeros(V, np.float32)
    for kw in bad:
        a = dict(temperature=T, seed=1, top_k=40, top_p=0.9, min_p=0.05)
        a.update(kw)
        for call in (lambda: m.forward_sample_ex(2, 1, **a), lambda: m.decode_sample_ex(2, 1, 2, **a), lambda: m.sample_logits(ok, 1, **a)):
            with pytest.raises(llmk.LlmkError) as e:
                call()
            assert e.value.code == E_ARG, kw
    assert m.forward_greedy(2, 1) >= 1                          # nothing ran: position 1 is still free
    m.close()


# ---- transcripts --------------------------------------------------------------------------------------------------------------
SETTINGS = [dict(top_k=40, top_p=0.9, min_p=0.0), dict(top_k=0, top_p=1.0, min_p=0.1)]
WINDOW_CASE = ("tinyllama-q4_0-q6k", 0.1)       # the one (model, min_p) whose flat logits put a row inside the min-p margin too often
DENSE_FACTOR = 1000                             # the rows near min_p are counted in a window this many margins wide


@pytest.mark.parametrize("name", ["tk-small", "tk-small-multikernel", "tiny-gqa", "tinyllama-q4_0-q6k"])
def test_decode_sample_ex_ids_are_the_rule_applied_to_the_logits(name, gguf):
    """decode_sample_ex over 64 positions; the ids teacher-forced through llmk_forward on a second context; each id must be the
    reference's pick from that position's logits wherever the position is safe (nucleus / min-p margins of filter_ref, score margin
    among the kept rows > 1e-5), and lie in the reference's kept set; at most max(1, n // 50) positions may go uncompared.

    One case cannot meet that cap by its input, whatever the sampler does: the 32,000 logits of tinyllama-q4_0-q6k are flat, so
    min_p = 0.1 keeps over a thousand rows and some row's e falls within 1e-5 * min_p of min_p at about one position in 25.  The
    test shows this from the logits themselves (DENSE_FACTOR below), and for that case alone compares more positions, not fewer:
    every safe one as everywhere, and every unsafe one whose pick is the same over each kept set the margin admits
    (filter_ref.sample_window); the cap then bounds the positions still uncompared, the unsafe ones have a bound of their own, and
    every id lies in the widest admissible set."""
    fw, flags, tk = _case(name, gguf)
    n, seed = 64, 20261018
    m = llmk.Llmk(fw, flags=flags)
    assert m.path() == (1 if tk else 0)
    runs = []
    for s in SETTINGS:
        m.reset()
        runs.append(m.decode_sample_ex(2, 1, n, T, seed, **s))
    m.reset()
    top5 = m.decode_sample_ex(2, 1, n, T, seed, top_k=5)
    m.reset()
    plain = m.decode_sample(2, 1, n, T, seed)
    assert m.path() == (1 if tk else 0)
    m.close()
    assert not np.array_equal(top5, plain)                      # the truncation changes the transcript of the same seed
    m = llmk.Llmk(fw, flags=flags)
    cap = max(1, n // 50)
    for s, ids in zip(SETTINGS, runs):
        window = (name, s["min_p"]) == WINDOW_CASE
        m.reset()
        tok, skipped, unsafe, undecided, near = 2, 0, 0, 0, 0
        for pos in range(1, n + 1):
            lg = m.forward(tok, pos)
            want, margin, decided, r = filter_ref.sample_window(lg, T, seed, pos, **s)
            if r.safe:                                              # (sample_window is sample() here: lo == hi == mask)
                if margin > 1e-5:
                    assert ids[pos - 1] == want, (s, pos, ids[pos - 1], want, margin)
                assert r.mask[ids[pos - 1] - 1], (s, pos)
            elif window:
                if decided and margin > 1e-5:
                    assert ids[pos - 1] == want, (s, pos, ids[pos - 1], want, margin)
                assert r.lo[ids[pos - 1] - 1], (s, pos)
            unsafe += not r.safe
            skipped += not (r.safe and margin > 1e-5)
            undecided += not (decided and margin > 1e-5)
            if window:                                              # rows within DENSE_FACTOR margins of min_p
                e = np.exp((lg.astype(np.float64) - lg.max()) / T)
                near += int((np.abs(e - s["min_p"]) <= DENSE_FACTOR * filter_ref.MARGIN * s["min_p"]).sum())
            tok = int(ids[pos - 1])
        print(f"{name} {s}: {skipped} of {n} unsafe or near-tied, {unsafe} unsafe, {undecided} uncompared, {near} rows near min_p")
        if window:
            # the rows within 1,000 margins of min_p number `near` over the transcript, so a margin's own width holds near / 1,000
            # of them on average: above the cap, the issue's count cannot hold (if this fails the model is no longer flat: drop
            # the window case); the unsafe positions stay within four Poisson deviations of that mean
            expect = near / DENSE_FACTOR
            assert expect > cap, (s, near)
            assert unsafe <= expect + 4 * np.sqrt(expect) + 1, (s, unsafe, expect)
            assert undecided <= cap, (s, undecided)
        else:
            assert skipped <= cap, (s, skipped)
        assert len(set(ids.tolist())) > 8, s                    # not a greedy transcript in disguise
    m.close()


@pytest.mark.parametrize("flags", [0, llmk.FLAG_MULTI_KERNEL], ids=["persistent", "multikernel"])
def test_pipelined_decode_equals_the_per_position_chain(flags, gguf):
    fw = gguf.synth_fused(gguf.SHAPES["tk-small"], 3)
    n, seed = 64, 7
    s = dict(top_k=40, top_p=0.9, min_p=0.02)
    m = llmk.Llmk(fw, flags=flags)
    path = 0 if flags else 1
    assert m.path() == path
    seen = []
    ids = m.decode_sample_ex(2, 1, n, T, seed, on_token=lambda i, t, u: seen.append((i, t)), **s)
    assert seen == list(enumerate(ids.tolist()))                  # streamed in order, each id once
    m.reset()
    chain, tok = [], 2
    for pos in range(1, n + 1):
        tok = m.forward_sample_ex(tok, pos, T, seed, **s)
        chain.append(tok)
    assert chain == ids.tolist()
    m.reset()
    assert np.array_equal(m.decode_sample_ex(2, 1, n, T, seed, **s), ids)
    m.reset()
    assert not np.array_equal(m.decode_sample_ex(2, 1, n, T, seed + 1, **s), ids)
    m.reset()                                                     # all filters off: llmk_decode_sample itself
    plain = m.decode_sample(2, 1, n, T, seed)
    m.reset()
    assert np.array_equal(m.decode_sample_ex(2, 1, n, T, seed), plain)
    m.reset()
    assert [m.forward_sample_ex(t, p, T, seed) for p, t in enumerate([2] + plain[:7].tolist(), 1)] == plain[:8].tolist()
    m.reset()
    m.decode_sample_ex(2, 1, n, T, seed, **s)
    m.reset()                                                     # greedy afterwards is still greedy, sampling still unfiltered
    g = m.decode_greedy(2, 1, n)
    m.reset()
    toks, _ = m.generate(n, want_logits=False)
    assert np.array_equal(g, toks)
    m.reset()
    assert np.array_equal(m.decode_sample(2, 1, n, T, seed), plain)
    assert m.path() == path
    m.close()


def test_decode_sample_ex_resumes_after_forward_and_prefill(gguf):
    fw = gguf.synth_fused(gguf.SHAPES["tk-small-long"], 11)
    n, seed = 160, 99
    s = dict(top_k=40, top_p=0.9, min_p=0.02)
    m = llmk.Llmk(fw)
    assert m.path() == 1
    ref = m.decode_sample_ex(2, 1, n, T, seed, **s)
    for k in (1, 7, 129):
        m.reset()
        tok = 2
        for pos in range(1, k + 1):
            m.forward(tok, pos)
            tok = int(ref[pos - 1])
        assert np.array_equal(m.decode_sample_ex(tok, k + 1, n - k, T, seed, **s), ref[k:n]), k
        m.reset()
        m.prefill([2] + ref[:k - 1].tolist(), 1)
        assert np.array_equal(m.decode_sample_ex(int(ref[k - 1]), k + 1, n - k, T, seed, **s), ref[k:n]), k
    assert m.path() == 1
    m.close()


# ---- distribution -------------------------------------------------------------------------------------------------------------
def _chi2(obs, exp):
    stat = float(((obs - exp) ** 2 / exp).sum())
    return stat, float(chi2.sf(stat, len(obs) - 1))


def test_draws_follow_the_softmax_renormalised_over_the_top_k_rows(gguf):
    fw = gguf.synth_fused(gguf.SHAPES["tk-small"], 3)
    m = llmk.Llmk(fw)
    assert m.path() == 1
    N, pos, k = 12000, 3, 8
    for p in (1, 2):
        m.forward(2 + p, p)
    lg = m.forward(7, pos).astype(np.float64)
    rows = np.argsort(-lg, kind="stable")[:k]
    assert lg[rows[-1]] > np.partition(lg, -k - 1)[-k - 1]        # no tie at the k-th place: exactly 8 rows
    # the smallest temperature of the list at which each of the 8 rows expects >= 20 draws
    for temp in (0.25, 0.5, 1.0, 2.0, 4.0, 8.0):
        pr = np.exp((lg - lg.max()) / temp)
        pr /= pr.sum()
        sub = pr[rows] / pr[rows].sum()
        if (sub * N >= 20).all():
            break
    assert (sub * N >= 20).all()
    counts = np.zeros(lg.size)
    for seed in range(N):
        counts[m.forward_sample_ex(7, pos, temp, seed, top_k=k) - 1] += 1
    m.close()
    assert counts[rows].sum() == N                                 # every draw lies in the reference's 8 rows
    stat, p = _chi2(counts[rows], sub * N)
    assert p > 1e-6, (temp, stat, p)
    rest = 1.0 - pr[rows].sum()                                    # the same counts against the unrestricted softmax: rejected
    stat_w, p_w = _chi2(np.append(counts[rows], 0.0), np.append(pr[rows], rest) * N)
    assert p_w < 1e-6, (temp, stat_w, p_w, rest)


# ---- CLI ----------------------------------------------------------------------------------------------------------------------
def _cli(args, cwd):
    r = subprocess.run([LLM] + args, capture_output=True, cwd=cwd, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split(b"\n")[1], r.stderr


def test_cli_filters_print_the_decode_sample_ex_transcript(gguf, tmp_path):
    s = gguf.SHAPES["tk-small"]
    seed_w = 3
    path = str(tmp_path / "synth.gguf")
    gguf.write_synth_gguf(path, s, seed_w)
    vocab = gguf.vocab_strings(s.vocab_size)
    m = llmk.Llmk(gguf.synth_fused(s, seed_w))
    assert m.path() == 1
    n = 64
    want = b"".join(vocab[t - 1] for t in m.decode_sample_ex(2, 1, n, T, 1, top_k=40, top_p=0.9))
    m.reset()
    want_minp = b"".join(vocab[t - 1] for t in m.decode_sample_ex(2, 1, n, T, 1, min_p=0.1))
    m.reset()
    greedy = b"".join(vocab[t - 1] for t in m.decode_greedy(2, 1, n))
    m.close()
    base = ["-m", path, "-n", str(n)]
    got, err = _cli(base + ["-t", "0.9", "--seed", "1", "--top-k", "40", "--top-p", "0.9"], str(tmp_path))
    assert got == want
    assert b"ignored" not in err
    got, _ = _cli(base + ["-t", "0.9", "--seed", "1", "--min-p", "0.1", "--device-sample"], str(tmp_path))
    assert got == want_minp
    got, err = _cli(base + ["-t", "0", "--top-k", "40"], str(tmp_path))
    assert got == greedy
    assert err.count(b"are ignored at temperature 0") == 1
