"""tk_attention and the service wave's fold keep their bits: logits of the persistent kernel against a fixture recorded with the
library as it was before that code was rewritten for latency (tests/attn_hop_bits.py, tests/host_tools/attn_hop_bits_record.py).
Teacher-forced with a fixed token sequence, compared at every position where the attention code changes branch: the first
timesteps, one and two batches of 32, the live-batch variants, the tile of 256 with the second part, the third part, the last."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from llm_f90_amd import llmk
import attn_hop_bits as ahb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(GOLDEN, "attn_hop_bits.npz"))
    assert int(z["seed"]) == ahb.SEED
    return z


@pytest.mark.parametrize("key,tag,wtype", ahb.CASES, ids=[c[0] for c in ahb.CASES])
def test_attention_hop_logits_are_bit_identical(key, tag, wtype, fixture, gguf):
    pos, lg = ahb.run_case(gguf, llmk, tag, wtype)
    ref_pos, ref = fixture[key + "/pos"], fixture[key + "/logits"]
    assert np.array_equal(pos, ref_pos)
    assert np.array_equal(pos, ahb.positions(gguf.SHAPES[tag].seq_len))
    for i, p in enumerate(pos.tolist()):
        same = np.array_equal(lg[i].view(np.uint32), ref[i].view(np.uint32))
        assert same, f"{key} position {p}: {np.count_nonzero(lg[i].view(np.uint32) != ref[i].view(np.uint32))} of {lg.shape[1]} logits differ, max |diff| {np.abs(lg[i] - ref[i]).max():.3e}"
