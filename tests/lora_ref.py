"""TEST INFRASTRUCTURE -- adapters for the batched decode (llmk_lora_*): seeded draws, the merged float64 reference, and the
condition on the inputs without which a pass that ignored an adapter, or swapped two, would pass."""
import dataclasses

import numpy as np

from conftest import REL_TOL, rel_err
from llm_f90_amd.tools import gguf
from ref_pass import RefPass

ALL = gguf.LORA_TARGETS
QV = ("attn_q", "attn_v")
REST = ("attn_k", "attn_output", "ffn_gate", "ffn_up", "ffn_down")
SCALE = 0.3


def draw(rng, s, rank, targets, scale=SCALE):
    """(rank, scale, {(target, layer): (A, B)}) on every layer: A ~ N(0, 1/K), B ~ N(0, 1) / sqrt(rank), float32"""
    pieces = {}
    for l in range(s.n_layers):
        for t in targets:
            name, _, rows = gguf.lora_piece(s, t)
            K = s.hidden_dim if name == "w2" else s.emb_dim
            pieces[t, l] = ((rng.normal(size=(rank, K)) / np.sqrt(K)).astype(np.float32), (rng.normal(size=(rows, rank)) / np.sqrt(rank)).astype(np.float32))
    return rank, scale, pieces


def merged(fw32, adapter):
    """W' = W + scale B A per piece, formed in float64 and cast to f32 (6e-8 relative: far inside the bar)"""
    _, scale, pieces = adapter
    w = {n: getattr(fw32, n).copy() for n in ("wqkv", "wo", "w13", "w2")}
    for (t, l), (A, B) in pieces.items():
        name, r0, rows = gguf.lora_piece(fw32.shape, t)
        w[name][l, r0:r0 + rows] = (w[name][l, r0:r0 + rows].astype(np.float64) + scale * (B.astype(np.float64) @ A.astype(np.float64))).astype(np.float32)
    return dataclasses.replace(fw32, **w)


def far(x, y):
    return rel_err(x, y).min() > 100 * REL_TOL


def models(fw32, adapters):
    """the float64 passes, never fed themselves: [0] the base model, [k + 1] the model merged with adapters[k]"""
    return [RefPass(fw32)] + [RefPass(merged(fw32, a)) for a in adapters]


def references(ms, assign, seqs):
    """slot j's sequence alone through the model of its adapter assign[j] (None: the base): logits [len][V] per slot.  Asserted first:
    a slot's logits with and without its adapter, and slot 0's sequence under any two adapters of the pass, differ by more than
    100 x REL_TOL at every position."""
    out = []
    for a, seq in zip(assign, seqs):
        out.append(ms[0 if a is None else a + 1].fork(0).feed(seq))
        assert a is None or far(out[-1], ms[0].fork(0).feed(seq)), ("an adapter too close to the base model", a)
    probe = [ms[a + 1].fork(0).feed(seqs[0]) for a in sorted({a for a in assign if a is not None})]
    assert all(far(x, y) for i, x in enumerate(probe) for y in probe[:i]), "two adapters too close to each other"
    return out


def upload(llmk, m, adapters):
    out = []
    for rank, scale, pieces in adapters:
        out.append(llmk.Lora(m, rank, scale))
        for (t, l), (A, B) in pieces.items():
            out[-1].upload(gguf.lora_piece(m.shape, t)[0], l, gguf.lora_piece(m.shape, t)[1], A, B)
    return out
