"""`llm --parallel N --share-prefix`: the N slots attached to ONE copy of the prompt's K/V rows (llmk_prefix_*)
instead of holding a copy each.  The CLI and llmk.Batch with set_prefix / attach run the same library calls, so the texts are compared
id for id (tests/test_host_batch_gpu.py does this for the forked slots)."""
import os
import subprocess

import pytest

from conftest import ROOT
from llm_f90_amd import llmk

pytestmark = pytest.mark.gpu
LLM = os.path.join(ROOT, "llm.f90_amd", "host", "llm")
SEED, N, PROMPT = 20260928, 24, "hi there"


def completions(out, n):
    """the text under each line [k], k = 0 .. n-1"""
    lines = out.split(b"\n")
    return [lines[lines.index(b"[%d]" % k) + 1] for k in range(n)]


@pytest.fixture(scope="module")
def model(gguf, tmp_path_factory):
    d = tmp_path_factory.mktemp("share_prefix")
    path = str(d / "m.gguf")
    s = gguf.SHAPES["tk-small"]
    gguf.write_synth_gguf(path, s, SEED)
    return path, str(d), s


def test_shared_prefix_completions_are_batch_decode_s_on_attached_slots(model, gguf):
    assert os.path.exists(LLM), "host/llm not built (amdflang) -- the drop-in CLI is part of the product"
    path, cwd, s = model
    r = subprocess.run([LLM, "-m", path, "-n", str(N), "-p", PROMPT, "--parallel", "3", "-t", "0.9", "--seed", "7", "--top-k", "40",
                        "--share-prefix"], capture_output=True, cwd=cwd, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = completions(r.stdout, 3)
    # the same through the binding: positions 1 .. k = BOS and the first k-1 prompt tokens, the last one fed at k+1 to every row
    pids = [3 + ord(c) - 32 + 1 for c in PROMPT]
    k = len(pids)
    vocab = gguf.vocab_strings(s.vocab_size)
    m = llmk.Llmk(gguf.synth_fused(s, SEED))
    m.prefill([2] + pids[:-1], 1)
    b = llmk.Batch(m, 3, N)
    b.set_prefix(k)
    for j in range(3):
        b.attach(j)
    ids = b.decode([0, 1, 2], [pids[-1]] * 3, [k + 1] * 3, N - k, [llmk.sampler(0.9, 7 + j, top_k=40) for j in range(3)])
    b.close()
    m.close()
    want = [b"".join(vocab[t - 1] for t in row) for row in ids]
    assert got == want
    assert len(set(got)) == 3                      # three seeds, three texts
    assert b"tokens/second" in r.stdout


def test_share_prefix_without_parallel_says_so_and_stops(model):
    path, cwd, _ = model
    r = subprocess.run([LLM, "-m", path, "-n", str(N), "-p", PROMPT, "-t", "0.9", "--share-prefix"], capture_output=True, cwd=cwd, timeout=120)
    assert r.returncode != 0, r.stdout
    assert b"--share-prefix" in r.stdout and b"--parallel" in r.stdout, r.stdout
    assert b"tokens/second" not in r.stdout
