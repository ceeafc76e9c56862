"""`llm --parallel N --prompts FILE`: a prompt of its own per slot (llmk_span_*) through the Fortran host -- the
prompts ingested through the batch in span passes, the completions decoded together from their own positions.  The CLI and
llmk.Batch.ingest + llmk.Batch.decode run the same library path, so the texts are compared id for id."""
import os
import subprocess

import pytest

from conftest import ROOT
from llm_f90_amd import llmk

pytestmark = pytest.mark.gpu
LLM = os.path.join(ROOT, "llm.f90_amd", "host", "llm")
SEED, N = 20260928, 40
PROMPTS = ["hi there", "a", "the quick brown fox jumps"]      # 8, 1 and 25 byte tokens (the synthetic vocabulary has no merges)


def completions(out, n):
    """the text under each line [k], k = 0 .. n-1"""
    lines = out.split(b"\n")
    return [lines[lines.index(b"[%d]" % k) + 1] for k in range(n)]


@pytest.fixture(scope="module")
def model(gguf, tmp_path_factory):
    d = tmp_path_factory.mktemp("prompts")
    path = str(d / "m.gguf")
    s = gguf.SHAPES["tk-small"]
    gguf.write_synth_gguf(path, s, SEED)
    with open(d / "prompts.txt", "w") as f:
        f.write("\n".join(PROMPTS) + "\n")
    return path, str(d), s


def test_per_slot_prompts_are_ingest_and_batch_decode_s(model, gguf):
    assert os.path.exists(LLM), "host/llm not built (amdflang) -- the drop-in CLI is part of the product"
    path, cwd, s = model
    r = subprocess.run([LLM, "-m", path, "-n", str(N), "--parallel", "3", "--prompts", "prompts.txt", "-t", "0", "--vx"], capture_output=True,
                       cwd=cwd, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = completions(r.stdout, 3)
    assert b"prompts ingested in 1 span passes" in r.stdout          # 8 + 1 + 25 rows: one pass
    # the same through the binding: slot j's positions 1 .. k_j = BOS and the first k_j - 1 prompt tokens, the last one fed at k_j + 1
    pids = [[3 + ord(c) - 32 + 1 for c in p] for p in PROMPTS]
    ks = [len(p) for p in pids]
    vocab = gguf.vocab_strings(s.vocab_size)
    m = llmk.Llmk(gguf.synth_fused(s, SEED))
    b = llmk.Batch(m, 3, N)
    for j in range(3):
        b.ingest(j, [2] + pids[j][:-1])
    ids = b.decode([0, 1, 2], [p[-1] for p in pids], [k + 1 for k in ks], N - max(ks))
    b.close()
    m.close()
    want = [b"".join(vocab[t - 1] for t in row) for row in ids]
    assert got == want
    assert len(set(got)) == 3 and all(len(g) > 0 for g in got)      # three prompts, three texts
    assert b"tokens/second" in r.stdout


def test_too_few_prompts_is_an_error(model):
    path, cwd, _ = model
    r = subprocess.run([LLM, "-m", path, "-n", str(N), "--parallel", "4", "--prompts", "prompts.txt", "-t", "0"], capture_output=True, cwd=cwd,
                       timeout=120)
    assert r.returncode == 1, r.stdout
    assert b"--prompts" in r.stdout and b"one prompt per slot" in r.stdout and b"[0]" not in r.stdout


@pytest.mark.parametrize("args,word", [(["--prompts", "prompts.txt"], b"--parallel"),
                                       (["--parallel", "3", "--prompts", "prompts.txt", "-p", "hi"], b"-p"),
                                       (["--parallel", "3", "--prompts", "prompts.txt", "--share-prefix"], b"--share-prefix")])
def test_prompts_says_what_it_does_not_combine_with_and_stops(model, args, word):
    path, cwd, _ = model
    r = subprocess.run([LLM, "-m", path, "-n", str(N), "-t", "0"] + args, capture_output=True, cwd=cwd, timeout=120)
    assert r.returncode != 0, r.stdout
    assert b"--prompts" in r.stdout and word in r.stdout, r.stdout
    assert b"[0]" not in r.stdout
