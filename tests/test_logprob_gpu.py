"""llmk_forward_sample_lp / llmk_decode_sample_lp / llmk_logprob_logits: the log-prob of every generated token and its top-N
alternatives, computed on the device behind the kernel that picked the token (include/llmk.h; the rule: llm.f90_amd/csrc/logprob.h,
restated in float64 by tests/logprob_ref.py).  Bars: on caller-supplied logits the kernel's ids and padding are the reference's
exactly and its values lie within 2^-20 * max(1, |L|, max finite |z|) of float64; a transcript's ids are those of decode_greedy /
decode_sample_ex, its log-probs those of llmk_score and of score_ref on teacher-forced logits within test_score_gpu.py's bound
(2 * 1e-4 * max|logit|); the pipelined launches and a chain of per-position calls give one record; the figures describe the RAW
logits under a logit bias; the CLI's --logprobs prints what the C-ABI returns."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import logprob_ref
import score_ref
from conftest import REL_TOL, ROOT, load_golden
from llm_f90_amd import llmk
from test_logprob_cpu import _run as host_rule, host_prog      # noqa: F401  (the header on the host: llmk_logprob_rule)
from test_score_gpu import _host_rope_table

pytestmark = pytest.mark.gpu
LLM = os.path.join(ROOT, "llm.f90_amd", "host", "llm")
T = 0.9
E_ARG = 1
SHAPES = ["tk-small", "tk-small-multikernel", "tiny-gqa", "tinyllama-q4_0-q6k"]
SAMPLERS = {"greedy": None, "temperature": dict(), "top_k40-top_p0.9": dict(top_k=40, top_p=0.9)}


@functools.lru_cache(maxsize=None)
def _weights(name):
    """(weights, flags, whether the persistent kernel serves the ctx): the shapes of the sampler tests"""
    from llm_f90_amd.tools import gguf
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


def _lp_kwargs(s, seed):
    return dict() if s is None else dict(temperature=T, seed=seed, **s)


# ---- the kernel on caller-supplied logits -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny-gqa", "tk-small", "tinyllama-q4_0-q6k"])
def test_logprob_logits_is_the_reference_rule(name, host_prog):      # noqa: F811
    """tiny-gqa: V = 300, fewer rows than threads; tk-small: V = 1,024, one row per thread; tinyllama: V = 32,000 = 31.25 x 1,024, a
    ragged last round"""
    fw, flags, _ = _weights(name)
    m = llmk.Llmk(fw, flags=flags)
    V = fw.shape.vocab_size
    vectors = logprob_ref.vectors(V)
    if name == "tinyllama-q4_0-q6k":                               # (no full-width golden at this size: the model's own logits)
        rows = [m.forward(2 + p, p) for p in (1, 2, 3)]
        m.reset()
    else:
        rows = list(load_golden(name)["logits"][:6])
    vectors += [(f"logits-{i}", z, int(np.argmax(z)) + 1) for i, z in enumerate(rows)]
    cases = [(z, tok, n) for _, z, tok in vectors for n in (0, 1, 20)]
    names = [f"{vn}-n{n}" for vn, _, _ in vectors for n in (0, 1, 20)]
    host = host_rule(host_prog, cases)
    worst, same_bits = 0.0, 0
    for cname, (z, tok, n), (_, h_tlp, h_toks, h_vals) in zip(names, cases, host):
        tlp, toks, vals = m.logprob_logits(z, tok, n)
        worst = max(worst, logprob_ref.check(cname, z, tok, n, tlp, toks, vals, host=(h_tlp, h_vals)))
        assert np.array_equal(toks, h_toks), cname               # the ids the host rule picks
        assert np.array_equal(np.isnan(vals), np.isnan(h_vals)) and np.isnan(tlp) == np.isnan(h_tlp), cname      # ... and its NaNs
        same_bits += np.array_equal(np.float32(tlp).view(np.uint32), np.float32(h_tlp).view(np.uint32)) and \
            np.array_equal(vals.view(np.uint32), h_vals.view(np.uint32))
    print(f"{name}: largest error {worst:.4f} of the bar (2^-20 of the scale) over {len(cases)} calls; "
          f"{same_bits} of them bit-identical to the host's expf / logf")
    assert m.forward_greedy(2, 1) >= 1                           # the hook ran no token pass: position 1 is still free
    m.close()


# ---- transcripts --------------------------------------------------------------------------------------------------------------
def _check_records(tag, ids, tlp, toks, vals, logits, score_lp):
    """ids [n], token_logprob [n], top lists [n][top_n], teacher-forced logits [n][V], llmk_score's log-probs [n]"""
    z = logits.astype(np.float64)
    bound = 2 * REL_TOL * np.abs(z).max(axis=1)
    L = score_ref.lse(z)
    ref = z - L[:, None]
    rows = np.arange(len(ids))
    d_ref = np.abs(tlp - ref[rows, ids - 1])
    d_score = np.abs(tlp.astype(np.float64) - score_lp)
    print(f"{tag}: max |token_logprob - score_ref| {d_ref.max():.3e}, - llmk_score {d_score.max():.3e} (bound {bound.min():.3e} ..)")
    assert (d_ref <= bound).all(), (tag, int(np.argmax(d_ref / bound)), d_ref.max())
    assert (d_score <= bound).all(), (tag, int(np.argmax(d_score / bound)), d_score.max())
    top_n = toks.shape[1]
    assert (toks >= 1).all() and (toks <= z.shape[1]).all()
    assert (np.diff(vals, axis=1) <= 0).all(), tag                # values do not increase from entry to entry
    listed_ref = np.take_along_axis(ref, toks.astype(np.int64) - 1, axis=1)
    assert (np.abs(vals - listed_ref) <= bound[:, None]).all(), tag
    for i in rows:
        assert len(set(toks[i].tolist())) == top_n, (tag, i)
        rest = z[i].copy()
        rest[toks[i] - 1] = -np.inf                               # no unlisted row above the last listed one
        assert rest.max() - z[i, toks[i, -1] - 1] <= bound[i], (tag, i)


@pytest.mark.parametrize("sampler", list(SAMPLERS))
@pytest.mark.parametrize("name", SHAPES)
def test_decode_sample_lp_transcript(name, sampler):
    fw, flags, tk = _weights(name)
    s = SAMPLERS[sampler]
    n, seed, top_n = 64, 20261101, 20
    m = llmk.Llmk(fw, flags=flags)
    assert m.path() == (1 if tk else 0)
    ids, tlp, toks, vals = m.decode_sample_lp(2, 1, n, top_n, **_lp_kwargs(s, seed))
    assert m.path() == (1 if tk else 0)
    m.close()
    m = llmk.Llmk(fw, flags=flags)                                # a second context: the same ids without the records
    want = m.decode_greedy(2, 1, n) if s is None else m.decode_sample_ex(2, 1, n, T, seed, **s)
    assert np.array_equal(ids, want)
    fed = [2] + ids[:-1].tolist()
    m.reset()
    logits = np.array([m.forward(t, p) for p, t in enumerate(fed, 1)])
    m.reset()
    score_lp = m.score(fed, 1, targets=ids)
    m.close()
    _check_records(f"{name} {sampler}", ids, tlp, toks, vals, logits, score_lp)
    if s is None:                                                 # greedy: the token is the first alternative wherever the top-1 margin is safe
        top2 = np.sort(logits, axis=1)[:, -2:]
        safe = (top2[:, 1] - top2[:, 0]) > 4 * REL_TOL * np.abs(logits).max(axis=1)
        assert np.array_equal(toks[safe, 0], ids[safe]) and np.array_equal(vals[safe, 0], tlp[safe])
    else:
        assert len(set(ids.tolist())) > 8                         # not a greedy transcript in disguise


@pytest.mark.parametrize("sampler", list(SAMPLERS))
def test_pipelined_decode_equals_the_per_position_chain(sampler):
    fw, flags, _ = _weights("tk-small")
    s = SAMPLERS[sampler]
    n, seed, top_n = 64, 7, 5
    m = llmk.Llmk(fw, flags=flags)
    assert m.path() == 1
    seen = []
    ids, tlp, toks, vals = m.decode_sample_lp(2, 1, n, top_n, on_token=lambda i, t, u: seen.append((i, t)), **_lp_kwargs(s, seed))
    assert seen == list(enumerate(ids.tolist()))                  # on_token keeps its timing: in order, each id once
    m.reset()
    tok, chain = 2, []
    for pos in range(1, n + 1):
        tok, c_tlp, c_toks, c_vals = m.forward_sample_lp(tok, pos, top_n, **_lp_kwargs(s, seed))
        chain.append((tok, c_tlp, c_toks.copy(), c_vals.copy()))
    assert m.path() == 1
    assert [c[0] for c in chain] == ids.tolist()
    c_tlp = np.array([c[1] for c in chain], np.float32)
    c_toks, c_vals = np.array([c[2] for c in chain]), np.array([c[3] for c in chain])
    m.reset()
    fed = [2] + ids[:-1].tolist()
    bound = 2 * REL_TOL * np.array([np.abs(m.forward(t, p)).max() for p, t in enumerate(fed, 1)])
    assert np.array_equal(c_toks, toks)
    assert (np.abs(c_tlp - tlp) <= bound).all() and (np.abs(c_vals - vals) <= bound[:, None]).all()
    print(f"{sampler}: pipelined and per-position values bit-identical: "
          f"{np.array_equal(c_tlp.view(np.uint32), tlp.view(np.uint32)) and np.array_equal(c_vals.view(np.uint32), vals.view(np.uint32))}")
    # with no request the entry points give what they gave: the same ids again, and a request for the log-prob alone
    m.reset()
    ids0, tlp0, toks0, _ = m.decode_sample_lp(2, 1, n, 0, **_lp_kwargs(s, seed))
    assert np.array_equal(ids0, ids) and toks0.shape == (n, 0) and np.array_equal(tlp0.view(np.uint32), tlp.view(np.uint32))
    m.close()


def test_logprobs_describe_the_raw_logits_under_a_bias():
    fw, flags, _ = _weights("tk-small")
    n, seed, top_n = 64, 11, 5
    four = [17, 300, 555, 1024]
    m = llmk.Llmk(fw, flags=flags)
    ids, tlp, toks, vals = m.decode_sample_lp(2, 1, n, top_n, temperature=T, seed=seed, bias=[(t, 40.0) for t in four])
    want = m.get_history(n)                                       # the record is kept by the _pen rule: the tokens fed
    assert want.tolist() == [2] + ids[:-1].tolist()
    m.close()
    m = llmk.Llmk(fw, flags=flags)
    assert np.array_equal(m.decode_sample_pen(2, 1, n, T, seed, bias=[(t, 40.0) for t in four]), ids)
    m.reset()
    fed = [2] + ids[:-1].tolist()
    z = np.array([m.forward(t, p) for p, t in enumerate(fed, 1)]).astype(np.float64)
    m.close()
    assert np.abs(z).max() < 10                                   # (so +40 puts the four above every other row)
    assert set(ids.tolist()) <= set(four)
    bound = 2 * REL_TOL * np.abs(z).max(axis=1)
    rows = np.arange(n)
    raw = z[rows, ids - 1] - score_ref.lse(z)
    adj = z.copy()
    adj[:, np.array(four) - 1] += 40.0
    adjusted = adj[rows, ids - 1] - score_ref.lse(adj)
    print(f"raw {raw.mean():.3f} (-log V = {-np.log(z.shape[1]):.3f}), adjusted {adjusted.mean():.3f} (-log 4 = {-np.log(4):.3f}), "
          f"got {tlp.mean():.3f}")
    assert (np.abs(tlp - raw) <= bound).all()
    assert (np.abs(tlp - adjusted) > 1.0).all()
    # ... and so do the alternatives: the raw top rows, not the four
    order = np.argsort(-z, axis=1, kind="stable")[:, :top_n]
    safe = np.diff(-np.take_along_axis(z, np.argsort(-z, axis=1, kind="stable")[:, :top_n + 1], axis=1), axis=1).min(axis=1) > 2 * bound
    assert safe.sum() > n // 2 and np.array_equal(toks[safe] - 1, order[safe])


# ---- arguments ----------------------------------------------------------------------------------------------------------------
def test_invalid_requests_are_rejected_before_anything_runs():
    from llm_f90_amd.tools import gguf
    fw, flags, _ = _weights("tk-small")
    m = llmk.Llmk(fw, flags=flags)
    L, h, V = llmk.lib(), m._h, fw.shape.vocab_size
    nxt, ids = C.c_int(0), (C.c_int * 4)()
    sp = C.byref(llmk.sampler(T, 1, 40, 0.9))
    pn = C.byref(llmk.penalties(bias=[(5, 1.0)]))
    ok = llmk.logprobs(4, 3)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)

    def req(top_n, token=True, tokens=True, values=True):
        r = llmk.logprobs(4, max(top_n, 1))
        r.top_n = top_n
        if not token:
            r.token_logprob = fp()
        if not tokens:
            r.top_tokens = ip()
        if not values:
            r.top_logprobs = fp()
        return r

    bad = [None, req(-1), req(21), req(0, token=False), req(3, tokens=False), req(3, values=False)]
    for r in bad:
        lp = C.byref(r) if r is not None else None
        for s_, p_ in ((sp, None), (sp, pn), (None, None)):
            assert L.llmk_forward_sample_lp(h, 2, 1, s_, p_, lp, C.byref(nxt)) == E_ARG
            assert L.llmk_decode_sample_lp(h, 2, 1, 4, s_, p_, lp, ids, None, None) == E_ARG
    # the greedy form takes no penalties; the sampler is checked as in the _pen functions
    assert L.llmk_forward_sample_lp(h, 2, 1, None, pn, C.byref(ok), C.byref(nxt)) == E_ARG
    assert L.llmk_decode_sample_lp(h, 2, 1, 4, None, pn, C.byref(ok), ids, None, None) == E_ARG
    assert L.llmk_decode_sample_lp(h, 2, 1, 4, C.byref(llmk.sampler(0.0, 1)), None, C.byref(ok), ids, None, None) == E_ARG
    assert L.llmk_forward_sample_lp(h, 2, 1, sp, None, C.byref(ok), None) == E_ARG
    assert L.llmk_forward_sample_lp(h, V + 1, 1, sp, None, C.byref(ok), C.byref(nxt)) == E_ARG
    # the hook
    z = np.zeros(V, np.float32)
    zp = z.ctypes.data_as(fp)
    assert L.llmk_logprob_logits(h, None, 1, 3, ok.token_logprob, ok.top_tokens, ok.top_logprobs) == E_ARG
    assert L.llmk_logprob_logits(h, zp, -1, 3, ok.token_logprob, ok.top_tokens, ok.top_logprobs) == E_ARG
    assert L.llmk_logprob_logits(h, zp, V + 1, 3, ok.token_logprob, ok.top_tokens, ok.top_logprobs) == E_ARG
    assert L.llmk_logprob_logits(h, zp, 1, 21, ok.token_logprob, ok.top_tokens, ok.top_logprobs) == E_ARG
    assert L.llmk_logprob_logits(h, zp, 1, -1, ok.token_logprob, ok.top_tokens, ok.top_logprobs) == E_ARG
    assert L.llmk_logprob_logits(h, zp, 1, 0, None, None, None) == E_ARG
    assert L.llmk_logprob_logits(h, zp, 1, 3, ok.token_logprob, None, ok.top_logprobs) == E_ARG
    assert L.llmk_logprob_logits(h, zp, 1, 3, None, ok.top_tokens, ok.top_logprobs) == 0      # the list alone
    assert ok.tokens[0].tolist() == [1, 2, 3] and np.allclose(ok.values[0], -np.log(V), atol=1e-5)
    assert L.llmk_logprob_logits(h, zp, 0, 0, ok.token_logprob, None, None) == 0 and ok.token[0] == 0.0
    assert m.forward_greedy(2, 1) >= 1                            # nothing ran: position 1 is still free
    m.close()
    # a tensor-parallel context
    tp = llmk.Llmk.create_empty(gguf.SHAPES["tk-small"], 0, tp_rank=0, tp_size=2)
    assert L.llmk_forward_sample_lp(tp._h, 2, 1, sp, None, C.byref(ok), C.byref(nxt)) == E_ARG
    assert L.llmk_decode_sample_lp(tp._h, 2, 1, 4, None, None, C.byref(ok), ids, None, None) == E_ARG
    assert L.llmk_logprob_logits(tp._h, zp, 1, 3, ok.token_logprob, ok.top_tokens, ok.top_logprobs) == E_ARG
    tp.close()


# ---- CLI ----------------------------------------------------------------------------------------------------------------------
def _cli(args, cwd):
    r = subprocess.run([LLM] + args, capture_output=True, cwd=cwd, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout, r.stderr


def _records(stdout, top_n):
    """the --logprobs block: [(index, id, logprob text, [(id, logprob text)])] and the named totals"""
    rows, named = [], {}
    for line in stdout.decode(errors="replace").split("\n")[2:]:
        f = line.split()
        if len(f) >= 3 and f[0].isdigit() and f[1].isdigit() and "E" in f[2]:
            pairs = re.findall(r"(\d+):\s*(\S+)", line)
            assert len(pairs) == top_n, line
            rows.append((int(f[0]), int(f[1]), f[2], [(int(a), b) for a, b in pairs]))
        elif len(f) >= 2 and f[0] in ("tokens", "sum", "perplexity"):
            named[" ".join(f[:-1])] = f[-1]
    return rows, named


@pytest.mark.parametrize("temperature", [0.9, 0.0])
def test_cli_logprobs_prints_what_the_c_abi_returns(temperature, gguf, tmp_path):
    s = gguf.SHAPES["tk-small"]
    seed_w, n, top_n = 3, 64, 3
    path = str(tmp_path / "synth.gguf")
    gguf.write_synth_gguf(path, s, seed_w)
    vocab = gguf.vocab_strings(s.vocab_size)
    m = llmk.Llmk(gguf.synth_fused(s, seed_w))
    m.set_rope_freqs(_host_rope_table(s.head_size))
    kw = dict(temperature=temperature, seed=1) if temperature else dict()
    # the CLI's first position is one call, the rest one pipelined call
    t1, l1, k1, v1 = m.forward_sample_lp(2, 1, top_n, **kw)
    ids, tlp, toks, vals = m.decode_sample_lp(t1, 2, n - 1, top_n, **kw)
    m.close()
    ids, tlp = np.append(t1, ids), np.append(np.float32(l1), tlp)
    toks, vals = np.vstack([k1[None], toks]), np.vstack([v1[None], vals])
    base = ["-m", path, "-n", str(n), "-t", str(temperature), "--seed", "1"]
    out, err = _cli(base + ["--logprobs", str(top_n)], str(tmp_path))
    assert b"ignored" not in err
    assert out.split(b"\n")[1] == b"".join(vocab[t - 1] for t in ids)
    rows, named = _records(out, top_n)
    assert [r[0] for r in rows] == list(range(1, n + 1)) and [r[1] for r in rows] == ids.tolist()
    for r, want, wt, wv in zip(rows, tlp, toks, vals):
        assert r[2] == f"{float(want):.8E}", (r, want)
        assert [a for a, _ in r[3]] == wt.tolist() and [b for _, b in r[3]] == [f"{float(v):.8E}" for v in wv], (r, wt, wv)
    printed = np.array([float(r[2]) for r in rows])
    assert int(named["tokens"]) == n
    assert abs(float(named["sum logprob"]) - printed.sum()) <= 1e-6 * abs(printed.sum())
    assert abs(float(named["perplexity"]) - np.exp(-printed.mean())) <= 2e-6 * np.exp(-printed.mean())
    # without the flag the device consumer prints the same transcript, and nothing of the block
    plain, _ = _cli(base + (["--device-sample"] if temperature else ["--device-argmax"]), str(tmp_path))
    assert plain.split(b"\n")[1] == out.split(b"\n")[1]
    assert _records(plain, 0) == ([], {})
    zero, _ = _cli(base + ["--logprobs", "0"], str(tmp_path))
    assert zero.split(b"\n")[1] == out.split(b"\n")[1]
    assert [(r[0], r[1], r[2]) for r in _records(zero, 0)[0]] == [(r[0], r[1], r[2]) for r in rows]


def test_cli_logprobs_with_a_prefilled_prompt_and_a_bad_count(gguf, tmp_path):
    """`--logprobs N --prefill` at temperature 0: the first generated token has its record too (it is picked by the device consumer,
    not by the host's argmax), so the block is that of the run without --prefill; N outside 0..20 is rejected"""
    s = gguf.SHAPES["tk-small"]
    path = str(tmp_path / "synth.gguf")
    gguf.write_synth_gguf(path, s, 3)
    base = ["-m", path, "-n", "48", "-t", "0", "-p", "Once upon a time", "--logprobs", "2"]
    enc = subprocess.run([LLM, "-m", path, "-p", "Once upon a time", "--encode"], capture_output=True, cwd=str(tmp_path), timeout=120)
    k = len(enc.stdout.strip().split(b"\n")[-1].split())
    assert 1 < k < 40
    out, _ = _cli(base, str(tmp_path))
    pre, _ = _cli(base + ["--prefill"], str(tmp_path))
    rows, named = _records(out, 2)
    prows, pnamed = _records(pre, 2)
    assert len(rows) == 48 - k and int(named["tokens"]) == 48 - k == int(pnamed["tokens"])
    assert [(r[0], r[1]) for r in prows] == [(r[0], r[1]) for r in rows]
    assert pre.split(b"\n")[1] == out.split(b"\n")[1]
    for bad in ("-3", "21"):
        r = subprocess.run([LLM, "-m", path, "-n", "8", "--logprobs", bad], capture_output=True, cwd=str(tmp_path), timeout=120)
        assert r.returncode != 0 and b"--logprobs takes N in 0 .. 20" in r.stdout
