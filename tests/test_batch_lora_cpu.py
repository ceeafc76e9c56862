"""The condition on the inputs of tests/test_batch_lora_gpu.py, on the reference alone: every drawn adapter moves the float64 logits
by more than 100 x the bar, and any two differ by as much (lora_ref.references asserts it)."""
import numpy as np
import pytest

import lora_ref as lr
from llm_f90_amd.tools import gguf


@pytest.mark.parametrize("shape", ["tiny-gqa", "tk-small", "tiny-hs128w"])
def test_the_drawn_adapters_move_the_reference_far_beyond_the_bar(shape):
    fw = gguf.synth_fused(gguf.SHAPES[shape], 777)
    rng = np.random.default_rng(31)
    adapters = [lr.draw(rng, fw.shape, r, t) for r, t in [(4, lr.ALL), (24, lr.QV), (4, lr.REST), (64, lr.ALL)]]
    lr.references(lr.models(fw, adapters), [0, 1, 2, 3, None], [[2, 9, 40]] * 5)
