"""`llm --parallel N --kv-q8`: the N slots' K/V caches -- and with --share-prefix the prompt's one copy -- hold q8_0 blocks
(llmk_cache_create with LLMK_TYPE_Q8_0).  The CLI and llmk.Batch(kv_type="q8_0") run the same library calls,
so the texts are compared id for id, as tests/test_host_batch_kv16_gpu.py does for f16 caches; the flag is refused without --parallel
and together with --kv-f16."""
import os

import pytest

from llm_f90_amd import llmk      # noqa: F401
from test_host_batch_kv16_gpu import LLM, ROWS, SEED, completions, run, through_the_binding

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(gguf, tmp_path_factory):
    d = tmp_path_factory.mktemp("kv_q8")
    path = str(d / "m.gguf")
    s = gguf.SHAPES["tk-small"]
    gguf.write_synth_gguf(path, s, SEED)
    return path, str(d), s


@pytest.mark.parametrize("share", [False, True], ids=["forked", "share-prefix"])
def test_kv_q8_completions_are_batch_decode_s_on_a_q8_0_batch(model, gguf, share):
    assert os.path.exists(LLM), "host/llm not built (amdflang) -- the drop-in CLI is part of the product"
    r = run(model, "--parallel", str(ROWS), "--kv-q8", "--vx", *(["--share-prefix"] if share else []))
    assert r.returncode == 0, r.stdout + r.stderr
    assert completions(r.stdout, ROWS) == through_the_binding(gguf, model[2], "q8_0", share)
    assert b"batch K/V caches: q8_0" in r.stdout, r.stdout
    assert b"tokens/second" in r.stdout


def test_kv_q8_without_parallel_says_so_and_stops(model):
    r = run(model, "--kv-q8")
    assert r.returncode != 0, r.stdout
    assert b"--kv-q8" in r.stdout and b"--parallel" in r.stdout, r.stdout
    assert b"tokens/second" not in r.stdout


def test_kv_q8_together_with_kv_f16_says_so_and_stops(model):
    r = run(model, "--parallel", str(ROWS), "--kv-q8", "--kv-f16")
    assert r.returncode != 0, r.stdout
    assert b"--kv-q8" in r.stdout and b"--kv-f16" in r.stdout and b"one type" in r.stdout, r.stdout
    assert b"tokens/second" not in r.stdout
