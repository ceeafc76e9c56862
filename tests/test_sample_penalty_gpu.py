"""llmk_forward_sample_pen / llmk_decode_sample_pen / llmk_sample_logits_pen / llmk_set_history: repetition, frequency and presence
penalties and the logit bias in the device sampler (include/llmk.h; the rule: llm.f90_amd/csrc/sample_penalty.h, restated in numpy
float32 by tests/penalty_ref.py).  Bars: the kernel's adjusted logits are the reference's bit for bit; kept set and pick are the
reference's on every vector that is safe to compare; every id of a transcript is the reference's pick from the logits of its
position and the transcript's own window; the pipelined launches, a chain of per-position calls and the multi-kernel path give one
transcript and one token record; with everything neutral the functions are the _ex ones; the CLI prints what the C-ABI returns."""
import os
import subprocess

import numpy as np
import pytest

import filter_ref
import penalty_ref
from conftest import ROOT
from llm_f90_amd import llmk

pytestmark = pytest.mark.gpu
LLM = os.path.join(ROOT, "llm.f90_amd", "host", "llm")
T = 0.9
E_ARG, E_NONFINITE = 1, 11
NINF = float("-inf")


def _case(name, gguf):
    """(weights, flags, whether the persistent kernel serves the ctx): the small shapes of test_sample_filter_gpu.py"""
    S = gguf.SHAPES
    if name == "tk-small":
        return gguf.synth_fused(S["tk-small"], 3), 0, True
    if name == "tk-small-multikernel":
        return gguf.synth_fused(S["tk-small"], 3), llmk.FLAG_MULTI_KERNEL, False
    if name == "tiny-gqa":
        return gguf.synth_fused(S["tiny-gqa"], 1), 0, False
    raise KeyError(name)


# ---- 1. the kernel on caller-supplied logits and a caller-supplied record ---------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny-gqa", "tk-small", "tk-small-multikernel"])
def test_sample_logits_pen_is_the_reference_rule(name, gguf):
    """tiny-gqa: V = 300; tk-small: V = 1,024.  The shapes' own seq_len is 64, below the kernel's 256 threads, so the contexts are
    created with seq_len = 320 (the record is seq_len ints) and the "long" case's window of 300 positions makes every thread loop."""
    fw, flags, tk = _case(name, gguf)
    long_S = 300
    assert long_S > penalty_ref.THREADS
    m = llmk.Llmk(fw, flags=flags, seq_len=320)
    V = fw.shape.vocab_size
    cases = penalty_ref.cases((V,), long_S=long_S)
    uncompared = 0
    for c in cases:
        pen = penalty_ref.pen_args(c)
        want, margin, r, adj_ref = penalty_ref.sample(c["z"], c["hist"], c["pos"], c["T"], c["seed"], c["top_k"], c["top_p"], c["min_p"], **pen)
        m.set_history(c["hist"], 1)
        assert np.array_equal(m.get_history(c["pos"], 1), c["hist"])
        tok, kept, tau, adj = m.sample_logits_pen(c["z"], c["pos"], c["T"], c["seed"], c["top_k"], c["top_p"], c["min_p"], **pen)
        assert np.array_equal(m.get_history(c["pos"], 1), c["hist"]), c["name"]         # read, not written
        bad = np.flatnonzero(~((adj.view(np.uint32) == adj_ref.view(np.uint32)) | (np.isnan(adj) & np.isnan(adj_ref))))
        assert penalty_ref.same_bits(adj, adj_ref), (c["name"], bad[:8], adj[bad[:8]], adj_ref[bad[:8]])
        for t in c["banned"]:
            assert tok != t, c["name"]
        if not r.safe:
            uncompared += 1
            continue
        assert kept == r.kept, (c["name"], kept, r.kept)
        assert np.float32(tau) == r.tau, (c["name"], tau, r.tau)
        assert r.mask[tok - 1], c["name"]
        if margin > 1e-5:
            assert tok == want, (c["name"], tok, want, margin)
        else:
            uncompared += 1
    print(f"{name}: {uncompared} of {len(cases)} uncompared")
    assert uncompared <= len(cases) // 50, (uncompared, len(cases))
    m.close()


# ---- 2. transcripts -----------------------------------------------------------------------------------------------------------------
PROMPT = [2, 11, 23, 11, 40, 7]
SAMPLER = dict(top_k=40, top_p=0.9)
PEN = dict(last_n=16, repeat=1.1, frequency=0.2, presence=0.1, bias=[(5, NINF), (9, 1.5)])
N, SEQ = 64, 96


def _feed_prompt(m, prompt):
    """positions 1 .. k-1 through the model, the whole prompt into the record; the last prompt token is what the decode is fed"""
    for pos, tok in enumerate(prompt[:-1], 1):
        m.forward(tok, pos)
    m.set_history(prompt, 1)
    return prompt[-1], len(prompt)


@pytest.mark.parametrize("name", ["tk-small", "tk-small-multikernel", "tiny-gqa"])
def test_decode_sample_pen_ids_are_the_rule_applied_to_the_logits(name, gguf):
    """decode_sample_pen over 64 positions behind a recorded prompt; the ids teacher-forced through llmk_forward on a second context;
    each id must be the reference's pick from that position's logits and the transcript's own window wherever the position is safe
    (filter_ref's margins, score margin > 1e-5), and lie in the reference's kept set; at most max(1, n // 50) positions may go
    uncompared.  (seq_len = 96 holds prompt and transcript; the shapes' dims are unchanged.)"""
    fw, flags, tk = _case(name, gguf)
    seed = 20261018
    m = llmk.Llmk(fw, flags=flags, seq_len=SEQ)
    assert m.path() == (1 if tk else 0)
    tok, k = _feed_prompt(m, PROMPT)
    ids = m.decode_sample_pen(tok, k, N, T, seed, **SAMPLER, **PEN)
    assert m.path() == (1 if tk else 0)
    fed = PROMPT + ids[:-1].tolist()                              # the tokens fed at positions 1 .. k + N - 1
    assert m.get_history(len(fed), 1).tolist() == fed
    assert m.get_history(SEQ - len(fed), len(fed) + 1).tolist() == [0] * (SEQ - len(fed))
    m.close()
    assert 5 not in ids.tolist()
    m = llmk.Llmk(fw, flags=flags, seq_len=SEQ)
    for pos, t in enumerate(PROMPT[:-1], 1):
        m.forward(t, pos)
    skipped = 0
    for i in range(N):
        pos = k + i
        lg = m.forward(fed[pos - 1], pos)
        want, margin, r, _ = penalty_ref.sample(lg, np.array(fed[:pos]), pos, T, seed, **SAMPLER, **PEN)
        print(f"{name} pos {pos}: id {ids[i]} want {want} margin {margin:.3g} safe {r.safe} kept {r.kept}")
        if r.safe:
            if margin > 1e-5:
                assert ids[i] == want, (pos, ids[i], want, margin)
            assert r.mask[ids[i] - 1], pos
        skipped += not (r.safe and margin > 1e-5)
    assert skipped <= max(1, N // 50), skipped
    assert len(set(ids.tolist())) > 8                            # not a greedy transcript in disguise
    m.close()


# ---- 3. one transcript on every path ------------------------------------------------------------------------------------------------
def test_one_transcript_and_one_record_on_every_path(gguf):
    fw = gguf.synth_fused(gguf.SHAPES["tk-small"], 3)
    seed = 7
    runs = []
    for flags in (0, llmk.FLAG_MULTI_KERNEL):
        m = llmk.Llmk(fw, flags=flags, seq_len=SEQ)
        assert m.path() == (0 if flags else 1)
        tok, k = _feed_prompt(m, PROMPT)
        seen = []
        ids = m.decode_sample_pen(tok, k, N, T, seed, on_token=lambda i, t, u: seen.append((i, t)), **SAMPLER, **PEN)
        assert seen == list(enumerate(ids.tolist()))              # streamed in order, each id once
        runs.append((ids.tolist(), m.get_history(SEQ, 1).tolist()))
        m.close()
        m = llmk.Llmk(fw, flags=flags, seq_len=SEQ)               # a fresh context: the chain of per-position calls
        tok, k = _feed_prompt(m, PROMPT)
        chain = []
        for pos in range(k, k + N):
            tok = m.forward_sample_pen(tok, pos, T, seed, **SAMPLER, **PEN)
            chain.append(tok)
        runs.append((chain, m.get_history(SEQ, 1).tolist()))
        assert m.path() == (0 if flags else 1)
        m.close()
    for ids, hist in runs[1:]:
        assert ids == runs[0][0]
        assert hist == runs[0][1]
    assert runs[0][1][:len(PROMPT) + N - 1] == PROMPT + runs[0][0][:-1]


# ---- 4. off is off ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, llmk.FLAG_MULTI_KERNEL], ids=["persistent", "multikernel"])
def test_neutral_penalties_are_decode_sample_ex(flags, gguf):
    fw = gguf.synth_fused(gguf.SHAPES["tk-small"], 3)
    seed = 7
    m = llmk.Llmk(fw, flags=flags)
    want = m.decode_sample_ex(2, 1, N, T, seed, **SAMPLER)
    m.reset()
    plain = m.decode_sample(2, 1, N, T, seed)
    for pen in (dict(), dict(last_n=16), dict(last_n=0, repeat=1.3, frequency=0.5, presence=0.5), dict(last_n=64, repeat=1.0, frequency=0.0, presence=-0.0)):
        m.reset()
        assert np.array_equal(m.decode_sample_pen(2, 1, N, T, seed, **SAMPLER, **pen), want), pen
        m.reset()
        assert [m.forward_sample_pen(t, p, T, seed, **SAMPLER, **pen) for p, t in enumerate([2] + want[:7].tolist(), 1)] == want[:8].tolist()
        assert not m.get_history(N, 1).any()                      # the record is not maintained
    m.reset()                                                     # ... and with the filters off as well: llmk_decode_sample itself
    assert np.array_equal(m.decode_sample_pen(2, 1, N, T, seed), plain)
    m.reset()                                                     # the penalties change the transcript of the same seed; _ex afterwards is still _ex
    assert not np.array_equal(m.decode_sample_pen(2, 1, N, T, seed, **SAMPLER, last_n=16, repeat=1.5, frequency=1.0), want)
    m.reset()
    assert np.array_equal(m.decode_sample_ex(2, 1, N, T, seed, **SAMPLER), want)
    m.close()


# ---- 5. behaviour without a reference -----------------------------------------------------------------------------------------------
def test_a_huge_frequency_penalty_never_repeats_and_a_ban_holds(gguf):
    fw, flags, _ = _case("tiny-gqa", gguf)
    S = 72
    prompt = [2, 50, 60, 70]
    m = llmk.Llmk(fw, flags=flags, seq_len=S)
    tok, k = _feed_prompt(m, prompt)
    ids = m.decode_sample_pen(tok, k, N, T, 3, last_n=S, frequency=1e6).tolist()
    assert len(set(ids)) == N and not set(ids) & set(prompt)
    m.reset()
    assert not m.get_history(S, 1).any()                          # llmk_reset clears the record
    tok, k = _feed_prompt(m, prompt)
    banned = ids[0]                                               # what the same draw picks first when nothing forbids it
    ids2 = m.decode_sample_pen(tok, k, N, T, 3, last_n=S, frequency=1e6, bias=[(banned, NINF)]).tolist()
    assert banned not in ids2 and len(set(ids2)) == N and not set(ids2) & set(prompt)
    m.reset()
    tok, k = _feed_prompt(m, prompt)
    free = m.decode_sample_pen(tok, k, N, T, 3, bias=[(banned, 0.0)]).tolist()      # a bias of 0 changes no logit: the plain sampler's ids
    m.reset()
    for pos, t in enumerate(prompt[:-1], 1):
        m.forward(t, pos)
    assert free == m.decode_sample(tok, k, N, T, 3).tolist()
    assert len(set(free)) < N                                     # (it does repeat when nothing forbids it)
    m.close()


# ---- 6. arguments -------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_and_nonfinite_adjusted_logits(gguf):
    fw, flags, _ = _case("tk-small", gguf)
    m = llmk.Llmk(fw, flags=flags)
    V, S = fw.shape.vocab_size, fw.shape.seq_len
    nan, inf = float("nan"), float("inf")
    bad = [dict(last_n=-1), dict(last_n=S + 1), dict(repeat=0.0), dict(repeat=-1.0), dict(repeat=nan), dict(repeat=inf), dict(repeat=1e-39),
           dict(repeat=3e38), dict(frequency=nan), dict(frequency=inf), dict(presence=nan), dict(presence=-inf), dict(bias=[(3, nan)]),
           dict(bias=[(3, inf)]), dict(bias=[(0, 1.0)]), dict(bias=[(V + 1, 1.0)]), dict(bias=[(3, 1.0), (4, 1.0), (3, -1.0)]),
           dict(bias=[(t, 0.5) for t in range(1, llmk.MAX_LOGIT_BIAS + 2)]), dict(temperature=0.0), dict(temperature=nan), dict(top_k=-1),
           dict(top_p=0.0), dict(min_p=1.5)]
    ok = np.zeros(V, np.float32)
    for kw in bad:
        a = dict(temperature=T, seed=1, top_k=40, top_p=0.9, min_p=0.05, last_n=16, repeat=1.1, frequency=0.2, presence=0.1, bias=[(7, -1.0)])
        a.update(kw)
        for call in (lambda: m.forward_sample_pen(2, 1, **a), lambda: m.decode_sample_pen(2, 1, 2, **a), lambda: m.sample_logits_pen(ok, 1, **a)):
            with pytest.raises(llmk.LlmkError) as e:
                call()
            assert e.value.code == E_ARG, kw
    for call in (lambda: m.set_history([2, V + 1], 1), lambda: m.set_history([2, -1], 1), lambda: m.set_history([2, 3], S), lambda: m.set_history([2], 0),
                 lambda: m.get_history(2, S), lambda: m.sample_logits_pen(ok, S + 1, T, 1, last_n=4, repeat=1.1)):
        with pytest.raises(llmk.LlmkError) as e:
            call()
        assert e.value.code == E_ARG
    assert m.forward_greedy(2, 1) >= 1                          # nothing ran: position 1 is still free
    # the limits themselves are inside
    m.set_history([300, 0, V], S - 2)                          # (rows beyond the bias list's; a zero logit stays zero under repeat alone)
    assert m.get_history(3, S - 2).tolist() == [300, 0, V]
    tok, kept, tau, adj = m.sample_logits_pen(ok, S, T, 1, last_n=S, repeat=1.1, bias=[(t, 0.5) for t in range(1, llmk.MAX_LOGIT_BIAS + 1)])
    assert (adj[:llmk.MAX_LOGIT_BIAS] == 0.5).all() and not adj[llmk.MAX_LOGIT_BIAS:].any()
    # no adjusted logit above -inf: no token
    with pytest.raises(llmk.LlmkError) as e:
        m.sample_logits_pen(np.full(V, nan, np.float32), 1, T, 1, top_k=40, last_n=4, repeat=1.1, bias=[(7, -1.0)])
    assert e.value.code == E_NONFINITE
    z = np.full(V, -np.inf, np.float32)
    z[3] = 1.0
    assert m.sample_logits_pen(z, 1, T, 1, bias=[(5, 1.0)])[0] == 4
    with pytest.raises(llmk.LlmkError) as e:
        m.sample_logits_pen(z, 1, T, 1, bias=[(4, NINF)])
    assert e.value.code == E_NONFINITE
    m.close()


# ---- 7. CLI -------------------------------------------------------------------------------------------------------------------------
def _cli(args, cwd):
    r = subprocess.run([LLM] + args, capture_output=True, cwd=cwd, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split(b"\n")[1], r.stderr


def test_cli_penalties_print_the_decode_sample_pen_transcript(gguf, tmp_path):
    s = gguf.SHAPES["tk-small"]
    seed_w = 3
    path = str(tmp_path / "synth.gguf")
    gguf.write_synth_gguf(path, s, seed_w)
    vocab = gguf.vocab_strings(s.vocab_size)
    m = llmk.Llmk(gguf.synth_fused(s, seed_w))
    assert m.path() == 1
    n = 64
    m.set_history([2], 1)
    ids = m.decode_sample_pen(2, 1, n, T, 1, top_k=40, last_n=16, repeat=1.1, bias=[(5, NINF)])
    want = b"".join(vocab[t - 1] for t in ids)
    m.reset()
    plain = b"".join(vocab[t - 1] for t in m.decode_sample_ex(2, 1, n, T, 1, top_k=40))
    m.reset()
    greedy = b"".join(vocab[t - 1] for t in m.decode_greedy(2, 1, n))
    m.close()
    assert want != plain
    base = ["-m", path, "-n", str(n)]
    got, err = _cli(base + ["-t", "0.9", "--seed", "1", "--top-k", "40", "--repeat-penalty", "1.1", "--repeat-last-n", "16", "--logit-bias", "5:-inf"],
                    str(tmp_path))
    assert got == want
    assert b"ignored" not in err
    got, err = _cli(base + ["-t", "0", "--repeat-penalty", "1.1"], str(tmp_path))
    assert got == greedy
    assert err.count(b"ignored at temperature 0") == 1


def test_cli_records_bos_and_the_prompt_before_the_first_sampled_position(gguf, tmp_path):
    """With a prompt of k tokens the CLI feeds BOS and the prompt at positions 1 .. k+1 and records them there.  A window of two
    positions, a bias of +30 on the prompt's last-but-one token P and a presence penalty of 30 make the transcript say where P was
    recorded: at the first sampled position (k+1) the window is positions k and k+1, P sits at k and the penalty cancels its bias;
    recorded one position early, or not at all, P is all but certain to be drawn there.  The CLI's text must be the C-ABI's for
    set_history([BOS] + prompt, 1) + decode_sample_pen from position k+1, token by token and through --prefill."""
    s = gguf.SHAPES["tk-small"]
    seed_w = 3
    path = str(tmp_path / "synth.gguf")
    gguf.write_synth_gguf(path, s, seed_w)
    vocab = gguf.vocab_strings(s.vocab_size)
    prompt = "Once upon"
    enc = subprocess.run([LLM, "-m", path, "-p", prompt, "--encode"], capture_output=True, cwd=str(tmp_path), timeout=120)
    assert enc.returncode == 0, enc.stdout + enc.stderr
    ptoks = [int(t) for t in enc.stdout.strip().split(b"\n")[-1].split()]      # (after the " data offset" line)
    n, k = 64, len(ptoks)
    assert 2 <= k < n
    P = ptoks[-2]
    assert P != ptoks[-1] and P != 2
    pen = dict(top_k=40, last_n=2, presence=30.0, bias=[(P, 30.0)])
    m = llmk.Llmk(gguf.synth_fused(s, seed_w))
    assert m.path() == 1

    def transcript(record, at):
        m.reset()
        tok = 2
        for pos in range(1, k + 1):
            m.forward(tok, pos)
            tok = ptoks[pos - 1]
        m.set_history(record, at)
        return ptoks + m.decode_sample_pen(tok, k + 1, n - k, T, 1, **pen).tolist()

    ids = transcript([2] + ptoks, 1)
    assert m.get_history(n, 1).tolist() == ([2] + ids)[:n]        # the tokens fed at positions 1 .. n
    early = transcript(ptoks, 1)                                  # the prompt one position early (no BOS): P has left the window
    none = transcript([2], 1)                                     # the prompt not recorded
    m.close()
    assert early[k] == P and none[k] == P                         # (30 / 0.9 nats above its logit: the test can tell)
    assert ids != early and ids != none
    want = b"".join(vocab[t - 1] for t in ids)
    args = ["-m", path, "-n", str(n), "-t", "0.9", "--seed", "1", "--top-k", "40", "--repeat-last-n", "2", "--presence-penalty", "30",
            "--logit-bias", f"{P}:30", "-p", prompt]
    got, err = _cli(args, str(tmp_path))
    assert got == want
    got, err = _cli(args + ["--prefill"], str(tmp_path))
    assert got == want


# ---- 8. a redone position -----------------------------------------------------------------------------------------------------------
def test_a_timeout_inside_the_pipeline_leaves_the_same_transcript_and_record():
    """A launch of the pipelined decode that times out (the debug library launches position 20 one workgroup short:
    LLMK_TK_INJECT_TIMEOUT, as test_decode_greedy_gpu.py does) drains the launches behind it, whose penalty kernels have already
    written what they found in d_next into the record.  The redo on the multi-kernel path feeds every position the host's token
    and rewrites its entry before any window reads it: ids and record are those of an undisturbed multi-kernel context."""
    import sys
    dbg = os.path.join(ROOT, "llm.f90_amd", "csrc", "libllmk_debug.so")
    assert os.path.exists(dbg), "libllmk_debug.so not built (make -C llm.f90_amd debug)"
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "import llm_f90_amd\n"
        "from llm_f90_amd import llmk\n"
        "from llm_f90_amd.tools import gguf\n"
        f"PROMPT, N, SEQ, T = {PROMPT!r}, {N}, {SEQ}, {T}\n"
        "SAMPLER = dict(top_k=40, top_p=0.9)\n"
        "PEN = dict(last_n=16, repeat=1.1, frequency=0.2, presence=0.1, bias=[(5, float('-inf')), (9, 1.5)])\n"
        "fw = gguf.synth_fused(gguf.SHAPES['tk-small'], 3)\n"
        "runs = []\n"
        "for flags in (llmk.FLAG_MULTI_KERNEL, 0):\n"
        "    m = llmk.Llmk(fw, flags=flags, seq_len=SEQ)\n"
        "    assert m.path() == (0 if flags else 1)\n"
        "    for pos, tok in enumerate(PROMPT[:-1], 1):\n"
        "        m.forward(tok, pos)\n"
        "    m.set_history(PROMPT, 1)\n"
        "    seen = []\n"
        "    ids = m.decode_sample_pen(PROMPT[-1], len(PROMPT), N, T, 7, on_token=lambda i, t, u: seen.append((i, t)), **SAMPLER, **PEN)\n"
        "    assert seen == list(enumerate(ids.tolist())), seen\n"
        "    assert m.path() == 0\n"                                  # the persistent kernel was retired
        "    runs.append((ids.tolist(), m.get_history(SEQ, 1).tolist()))\n"
        "    m.close()\n"
        "assert runs[0][0] == runs[1][0], runs\n"
        "assert runs[0][1] == runs[1][1], runs\n"
        "assert runs[0][1][:len(PROMPT) + N - 1] == PROMPT + runs[0][0][:-1]\n"
        "print('PENALTY-REDO-OK')\n")
    env = dict(os.environ, LLMK_LIB=dbg, LLMK_TK_INJECT_TIMEOUT="20")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, env=env, timeout=300)
    assert r.returncode == 0 and b"PENALTY-REDO-OK" in r.stdout, r.stdout + r.stderr
    assert b"timed out" in r.stderr and b"multi-kernel path" in r.stderr
