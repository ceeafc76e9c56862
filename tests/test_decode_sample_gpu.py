"""llmk_forward_sample / llmk_decode_sample: temperature sampling on the device by the Gumbel-max rule of include/llmk.h.
Bars: every id is the rule (tests/sample_ref.py) applied to the logits of its position; the pipelined launches and a chain of
per-position calls give the same transcript id for id; the draws follow softmax(logits / T); the CLI's --device-sample prints
what the C-ABI returns."""
import os
import subprocess

import numpy as np
import pytest
from scipy.stats import chi2

import sample_ref
from conftest import ROOT, load_golden, safe_positions
from llm_f90_amd import llmk

pytestmark = pytest.mark.gpu
LLM = os.path.join(ROOT, "llm.f90_amd", "host", "llm")
T = 0.9


def _case(name, gguf):
    """(weights, flags, whether the persistent kernel serves the ctx)"""
    S = gguf.SHAPES
    if name == "tk-small":
        return gguf.synth_fused(S["tk-small"], 3), 0, True
    if name == "tk-small-multikernel":
        return gguf.synth_fused(S["tk-small"], 3), llmk.FLAG_MULTI_KERNEL, False
    if name == "tiny-gqa":
        return gguf.synth_fused(S["tiny-gqa"], 1), 0, False
    if name == "tk-small16":
        return gguf.synth_fused(S["tk-small16"], 4242, 1), 0, True
    if name == "tinyllama-q4_0":
        return gguf.synth_fused(S["tinyllama"], 20260928, 2), 0, True
    if name == "tinyllama-q4_0-q6k":
        return gguf.with_q6k_classifier(gguf.synth_fused(S["tinyllama"], 20260928, 2)), 0, True
    raise KeyError(name)


@pytest.mark.parametrize("name", ["tk-small", "tk-small-multikernel", "tiny-gqa", "tk-small16", "tinyllama-q4_0", "tinyllama-q4_0-q6k"])
def test_decode_sample_ids_are_the_rule_applied_to_the_logits(name, gguf):
    """decode_sample over 64 positions; the ids teacher-forced through llmk_forward on a second context; each id must be the
    numpy rule's pick from that position's logits wherever the top two scores are not a near-tie."""
    fw, flags, tk = _case(name, gguf)
    n, seed = 64, 20261016
    m = llmk.Llmk(fw, flags=flags)
    assert m.path() == (1 if tk else 0)
    ids = m.decode_sample(2, 1, n, T, seed)
    m.close()
    m = llmk.Llmk(fw, flags=flags)
    tok, skipped = 2, 0
    for pos in range(1, n + 1):
        want, margin = sample_ref.sample(m.forward(tok, pos), T, seed, pos)
        if margin > 1e-5:
            assert ids[pos - 1] == want, (pos, ids[pos - 1], want, margin)
        else:
            skipped += 1
        tok = int(ids[pos - 1])
    m.close()
    assert skipped <= max(1, n // 50), skipped
    assert len(set(ids.tolist())) > 8                   # not a greedy transcript in disguise


@pytest.mark.parametrize("flags", [0, llmk.FLAG_MULTI_KERNEL], ids=["persistent", "multikernel"])
def test_pipelined_decode_equals_the_per_position_chain(flags, gguf):
    fw = gguf.synth_fused(gguf.SHAPES["tk-small"], 3)
    n, seed = 64, 7
    m = llmk.Llmk(fw, flags=flags)
    assert m.path() == (0 if flags else 1)
    seen = []
    ids = m.decode_sample(2, 1, n, T, seed, on_token=lambda i, t, u: seen.append((i, t)))
    assert seen == list(enumerate(ids.tolist()))                  # streamed in order, each id once
    m.reset()
    chain, tok = [], 2
    for pos in range(1, n + 1):
        tok = m.forward_sample(tok, pos, T, seed)
        chain.append(tok)
    assert chain == ids.tolist()
    m.reset()
    assert np.array_equal(m.decode_sample(2, 1, n, T, seed), ids)
    m.reset()
    assert not np.array_equal(m.decode_sample(2, 1, n, T, seed + 1), ids)
    m.reset()                                                     # greedy afterwards is still greedy (invT back to 0)
    g = m.decode_greedy(2, 1, n)
    m.reset()
    toks, _ = m.generate(n, want_logits=False)
    assert np.array_equal(g, toks)
    m.close()


def test_decode_sample_resumes_after_forward_and_prefill(gguf):
    fw = gguf.synth_fused(gguf.SHAPES["tk-small-long"], 11)
    n, seed = 200, 99
    m = llmk.Llmk(fw)
    assert m.path() == 1
    ref = m.decode_sample(2, 1, n, T, seed)
    for k in (1, 7, 130):
        m.reset()
        tok = 2
        for pos in range(1, k + 1):
            m.forward(tok, pos)
            tok = int(ref[pos - 1])
        assert np.array_equal(m.decode_sample(tok, k + 1, n - k, T, seed), ref[k:n]), k
    m.reset()
    k = 129
    m.prefill([2] + ref[:k - 1].tolist(), 1)
    assert np.array_equal(m.decode_sample(int(ref[k - 1]), k + 1, n - k, T, seed), ref[k:n])
    with pytest.raises(llmk.LlmkError):
        m.decode_sample(2, fw.shape.seq_len, 2, T, seed)          # runs past the context
    m.close()


def _chi2(counts, probs, keep):
    """chi-square statistic and p-value over the bins `keep` plus one pooled bin of the rest"""
    N = counts.sum()
    obs = np.append(counts[keep], counts.sum() - counts[keep].sum())
    exp = np.append(probs[keep], 1.0 - probs[keep].sum()) * N
    stat = float(((obs - exp) ** 2 / exp).sum())
    return stat, float(chi2.sf(stat, len(obs) - 1))


def test_draws_follow_softmax_of_logits_over_temperature(gguf):
    fw = gguf.synth_fused(gguf.SHAPES["tk-small"], 3)
    m = llmk.Llmk(fw)
    assert m.path() == 1
    N, pos = 12000, 3
    for p in (1, 2):
        m.forward(2 + p, p)
    lg = m.forward(7, pos).astype(np.float64)
    # the smallest temperature of the list at which >= 10 tokens expect >= 20 draws (and the pooled rest, too)
    for temp in (0.25, 0.5, 1.0, 2.0, 4.0, 8.0):
        pr = np.exp((lg - lg.max()) / temp)
        pr /= pr.sum()
        keep = np.flatnonzero(pr * N >= 20)
        if len(keep) >= 10 and (1 - pr[keep].sum()) * N >= 20:
            break
    assert len(keep) >= 10
    counts = np.zeros(lg.size)
    for seed in range(N):
        counts[m.forward_sample(7, pos, temp, seed) - 1] += 1
    m.close()
    stat, p = _chi2(counts, pr, keep)
    assert p > 1e-6, (temp, stat, p, len(keep))
    wrong = np.exp((lg - lg.max()) / (0.5 * temp))                # the same draws against half the temperature: rejected
    wrong /= wrong.sum()
    stat_w, p_w = _chi2(counts, wrong, keep)
    assert p_w < 1e-6, (temp, stat_w, p_w)


def test_temperature_limits_and_the_greedy_limit(gguf):
    fw = gguf.synth_fused(gguf.SHAPES["tk-small"], 3)
    m = llmk.Llmk(fw)
    for bad in (0.0, -0.5, float("nan"), float("inf"), -float("inf"), 1e-45):
        with pytest.raises(llmk.LlmkError) as e:
            m.forward_sample(2, 1, bad, 1)
        assert e.value.code == 1
        with pytest.raises(llmk.LlmkError) as e:
            m.decode_sample(2, 1, 2, bad, 1)
        assert e.value.code == 1
    m.close()
    # T = 1e-6: the draw is the argmax wherever the reference's own top-1 margin is safe (teacher-forced on its goldens)
    for tag, flags in (("tk-small", 0), ("tk-small", llmk.FLAG_MULTI_KERNEL), ("tiny-gqa", 0)):
        g = load_golden(tag)
        fw = gguf.synth_fused(gguf.SHAPES[str(g["shape"])], int(g["seed"]))
        m = llmk.Llmk(fw, flags=flags)
        n = int(g["n"])
        safe = safe_positions(g, n)
        tok = 2
        for pos in range(1, n + 1):
            got = m.forward_sample(tok, pos, 1e-6, pos * 31 + 5)
            if safe[pos - 1]:
                assert got == g["tokens"][pos - 1], (tag, flags, pos)
            tok = int(g["tokens"][pos - 1])
        m.reset()
        ids = m.decode_sample(2, 1, n, 1e-6, 12345)
        first_bad = int(np.argmin(safe)) if not safe.all() else n
        assert np.array_equal(ids[:first_bad], g["tokens"][:first_bad]), (tag, flags)
        m.close()


def _cli(args, cwd):
    r = subprocess.run([LLM] + args, capture_output=True, cwd=cwd, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split(b"\n")[1]


def test_cli_device_sample_prints_the_decode_sample_transcript(gguf, tmp_path):
    s = gguf.SHAPES["tk-small"]
    seed_w = 3
    path = str(tmp_path / "synth.gguf")
    gguf.write_synth_gguf(path, s, seed_w)
    vocab = gguf.vocab_strings(s.vocab_size)
    fw = gguf.synth_fused(s, seed_w)
    m = llmk.Llmk(fw)
    assert m.path() == 1
    n = 64
    prompt = "Once upon"
    enc = subprocess.run([LLM, "-m", path, "-p", prompt, "--encode"], capture_output=True, cwd=str(tmp_path), timeout=120)
    assert enc.returncode == 0, enc.stdout + enc.stderr
    ptoks = [int(t) for t in enc.stdout.strip().split(b"\n")[-1].split()]      # (after the " data offset" line)
    assert 1 < len(ptoks) < n
    base = ["-m", path, "-n", str(n), "-t", "0.9", "--device-sample"]
    for seed in (7, 8):
        m.reset()
        want = b"".join(vocab[t - 1] for t in m.decode_sample(2, 1, n, T, seed))
        got = _cli(base + ["--seed", str(seed)], str(tmp_path))
        assert got == want, seed
        assert _cli(base + ["--seed", str(seed)], str(tmp_path)) == got
        if seed == 7:
            first = got
    assert first != got                                           # --seed 8 draws another transcript
    m.reset()
    k = len(ptoks)
    tok = 2
    for pos in range(1, k + 1):
        m.forward(tok, pos)
        tok = ptoks[pos - 1]
    want = b"".join(vocab[t - 1] for t in ptoks + m.decode_sample(tok, k + 1, n - k, T, 7).tolist())
    m.close()
    assert _cli(base + ["--seed", "7", "-p", prompt], str(tmp_path)) == want
    assert _cli(base + ["--seed", "7", "-p", prompt, "--prefill"], str(tmp_path)) == want
