"""`llm --parallel N --kv-f16`: the N slots' K/V caches -- and with --share-prefix the prompt's one copy -- hold IEEE halves
(llmk_cache_create).  The CLI and llmk.Batch(kv_type="f16") run the same library calls, so the texts are
compared id for id, as tests/test_host_batch_gpu.py and tests/test_host_batch_prefix_gpu.py do for f32 caches."""
import os
import subprocess

import pytest

from conftest import ROOT
from llm_f90_amd import llmk

pytestmark = pytest.mark.gpu
LLM = os.path.join(ROOT, "llm.f90_amd", "host", "llm")
SEED, N, PROMPT, ROWS = 20260928, 24, "hi there", 4


def completions(out, n):
    """the text under each line [k], k = 0 .. n-1"""
    lines = out.split(b"\n")
    return [lines[lines.index(b"[%d]" % k) + 1] for k in range(n)]


@pytest.fixture(scope="module")
def model(gguf, tmp_path_factory):
    d = tmp_path_factory.mktemp("kv_f16")
    path = str(d / "m.gguf")
    s = gguf.SHAPES["tk-small"]
    gguf.write_synth_gguf(path, s, SEED)
    return path, str(d), s


def run(model, *flags):
    path, cwd, _ = model
    return subprocess.run([LLM, "-m", path, "-n", str(N), "-p", PROMPT, "-t", "0", *flags], capture_output=True, cwd=cwd, timeout=120)


def through_the_binding(gguf, s, kv_type, share):
    """greedy texts of ROWS slots behind the prompt: positions 1 .. k = BOS and the first k-1 prompt tokens, the last one fed at k+1"""
    pids = [3 + ord(c) - 32 + 1 for c in PROMPT]
    k = len(pids)
    vocab = gguf.vocab_strings(s.vocab_size)
    m = llmk.Llmk(gguf.synth_fused(s, SEED))
    m.prefill([2] + pids[:-1], 1)
    b = llmk.Batch(m, ROWS, N, kv_type=kv_type)
    if share:
        b.set_prefix(k)
    for j in range(ROWS):
        b.attach(j) if share else b.fork(j, k)
    ids = b.decode(list(range(ROWS)), [pids[-1]] * ROWS, [k + 1] * ROWS, N - k)
    b.close()
    m.close()
    return [b"".join(vocab[t - 1] for t in row) for row in ids]


@pytest.mark.parametrize("share", [False, True], ids=["forked", "share-prefix"])
def test_kv_f16_completions_are_batch_decode_s_on_an_f16_batch(model, gguf, share):
    assert os.path.exists(LLM), "host/llm not built (amdflang) -- the drop-in CLI is part of the product"
    r = run(model, "--parallel", str(ROWS), "--kv-f16", "--vx", *(["--share-prefix"] if share else []))
    assert r.returncode == 0, r.stdout + r.stderr
    assert completions(r.stdout, ROWS) == through_the_binding(gguf, model[2], "f16", share)
    assert b"batch K/V caches: f16" in r.stdout, r.stdout
    assert b"tokens/second" in r.stdout


def test_a_run_without_the_flag_prints_what_the_f32_batch_gives(model, gguf):
    r = run(model, "--parallel", str(ROWS))
    assert r.returncode == 0, r.stdout + r.stderr
    assert completions(r.stdout, ROWS) == through_the_binding(gguf, model[2], "f32", False)
    assert b"K/V caches" not in r.stdout                 # (--vx alone names the type)
    x = run(model, "--parallel", str(ROWS), "--vx")
    assert x.returncode == 0 and b"batch K/V caches: f32" in x.stdout, x.stdout
    assert completions(x.stdout, ROWS) == completions(r.stdout, ROWS)


def test_kv_f16_without_parallel_says_so_and_stops(model):
    r = run(model, "--kv-f16")
    assert r.returncode != 0, r.stdout
    assert b"--kv-f16" in r.stdout and b"--parallel" in r.stdout, r.stdout
    assert b"tokens/second" not in r.stdout
