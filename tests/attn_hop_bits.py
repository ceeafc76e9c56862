"""The persistent kernel's attention arithmetic, bit for bit: the cases, the positions and the teacher-forced drive that
tests/test_attn_hop_bits_gpu.py and tests/host_tools/attn_hop_bits_record.py share.

The fixture tests/golden/attn_hop_bits.npz holds logits of the library as it was BEFORE tk_attention was rewritten for latency
(one-tile softmax in registers, straight-line score batches, the fold's reads issued together).  That rewrite may change the
schedule, where values live and control flow, never a value: every later change of that code is held to the same bits."""
import numpy as np

SEED = 20261021
# (fixture key, shape, weight type): the small shapes the persistent kernel is built for -- head size 64, kv_mul 2 over 704
# positions (one, two and three parts), and the f16 kernel
CASES = [("tk-small-long-f32", "tk-small-long", 0), ("tk-small16-f16", "tk-small16", 1)]
# where tk_attention changes branch: first timesteps | one batch of 32 | the second | the live-batch variants (1, 2, 4, 8) |
# the tile of 256 and the second part | the third part
BRANCH_POSITIONS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)


def positions(seq_len):
    """the branch positions inside the context, and its last position"""
    return sorted({p for p in BRANCH_POSITIONS if p <= seq_len} | {seq_len})


def tokens(shape):
    """the fixed token of every position, 1-based ids"""
    return np.random.default_rng(SEED).integers(1, shape.vocab_size + 1, size=shape.seq_len)


def run_case(gguf, llmk, tag, wtype):
    """positions 1 .. seq_len through llmk_forward with the fixed tokens; returns (stored positions, their logits [n][V])"""
    s = gguf.SHAPES[tag]
    m = llmk.Llmk(gguf.synth_fused(s, SEED, wtype))
    assert m.path() == 1, m.path_name()
    tok = tokens(s)
    keep = positions(s.seq_len)
    out = np.empty((len(keep), s.vocab_size), np.float32)
    for pos in range(1, s.seq_len + 1):
        lg = m.forward(int(tok[pos - 1]), pos)
        if pos in keep:
            out[keep.index(pos)] = lg
    assert m.path() == 1, m.path_name()            # no position was redone elsewhere
    m.close()
    return np.asarray(keep, np.int32), out
