"""`llm --parallel N`: N completions of one prompt decoded together (llmk_batch_*) through the Fortran host --
the prompt prefilled once, forked into N slots, every id drawn on the device.  The CLI and llmk.Batch.decode run the same library
path, so the texts are compared id for id."""
import os
import subprocess

import pytest

from conftest import ROOT
from llm_f90_amd import llmk

pytestmark = pytest.mark.gpu
LLM = os.path.join(ROOT, "llm.f90_amd", "host", "llm")
SEED, N, PROMPT = 20260928, 24, "hi there"


def run(args, cwd, ok=True):
    r = subprocess.run([LLM] + args, capture_output=True, cwd=cwd, timeout=120)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r.stdout


def completions(out, n):
    """the text under each line [k], k = 0 .. n-1"""
    lines = out.split(b"\n")
    got = []
    for k in range(n):
        i = lines.index(b"[%d]" % k)
        got.append(lines[i + 1])
    return got


@pytest.fixture(scope="module")
def model(gguf, tmp_path_factory):
    d = tmp_path_factory.mktemp("parallel")
    path = str(d / "m.gguf")
    s = gguf.SHAPES["tk-small"]
    gguf.write_synth_gguf(path, s, SEED)
    return path, str(d), s


def test_parallel_completions_are_batch_decode_s(model, gguf):
    assert os.path.exists(LLM), "host/llm not built (amdflang) -- the drop-in CLI is part of the product"
    path, cwd, s = model
    out = run(["-m", path, "-n", str(N), "-p", PROMPT, "--parallel", "3", "-t", "0.9", "--seed", "7", "--top-k", "40"], cwd)
    got = completions(out, 3)
    # the same through the binding: positions 1 .. k = BOS and the first k-1 prompt tokens, the last one fed at k+1 to every row
    pids = [3 + ord(c) - 32 + 1 for c in PROMPT]
    k = len(pids)
    vocab = gguf.vocab_strings(s.vocab_size)
    m = llmk.Llmk(gguf.synth_fused(s, SEED))
    m.prefill([2] + pids[:-1], 1)
    b = llmk.Batch(m, 3, N)
    for j in range(3):
        b.fork(j, k)
    ids = b.decode([0, 1, 2], [pids[-1]] * 3, [k + 1] * 3, N - k, [llmk.sampler(0.9, 7 + j, top_k=40) for j in range(3)])
    b.close()
    m.close()
    want = [b"".join(vocab[t - 1] for t in row) for row in ids]
    assert got == want
    assert len(set(got)) == 3                      # three seeds, three texts
    assert b"tokens/second" in out


def test_parallel_at_temperature_zero_prints_equal_texts(model):
    path, cwd, _ = model
    got = completions(run(["-m", path, "-n", str(N), "-p", PROMPT, "--parallel", "3", "-t", "0"], cwd), 3)
    assert got[0] == got[1] == got[2] and len(got[0]) > 0


@pytest.mark.parametrize("extra,word", [(["--logprobs", "3"], b"--logprobs"), (["--logit-bias", "5:-1"], b"--logit-bias"),
                                        (["--repeat-penalty", "1.1"], b"penalties"), (["--score"], b"--score"), (["--ngpu", "2"], b"--ngpu")])
def test_parallel_says_what_it_does_not_combine_with_and_stops(model, extra, word):
    path, cwd, _ = model
    r = subprocess.run([LLM, "-m", path, "-n", str(N), "-p", PROMPT, "--parallel", "2", "-t", "0.9"] + extra, capture_output=True, cwd=cwd,
                       timeout=120)
    assert r.returncode != 0, r.stdout
    assert b"--parallel" in r.stdout and word in r.stdout, r.stdout
    assert b"[0]" not in r.stdout


def test_parallel_refuses_a_shape_without_a_batched_pass(gguf, tmp_path):
    path = str(tmp_path / "m.gguf")
    gguf.write_synth_gguf(path, gguf.SHAPES["tiny-mha"], SEED)          # H = 352
    r = subprocess.run([LLM, "-m", path, "-n", "8", "--parallel", "2", "-t", "0"], capture_output=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode != 0 and b"--parallel" in r.stdout and b"multiples of 64" in r.stdout, r.stdout
