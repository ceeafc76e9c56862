"""Attention needle tests: every attention kernel on models whose layer-0 softmax mass sits on a few chosen timesteps, placed on the
kernels' tile, batch and part boundaries (tests/attn_needle.py builds the models and names the boundaries from mirrors of the
headers; tests/test_attn_needle_cpu.py shows that the f32 oracle is a sound reference on these inputs and that ONE needle dropped
or read from the wrong kv head moves every later position's logits by > 0.1 of max |logit| -- a thousand times the bar).

With synth_fused's flat softmax a dropped, duplicated or misread boundary row moves the logits by ~ 1/pos of a V row and hides
under the 1e-4 bar exactly at the long contexts whose tests exist for the boundaries; and the running-softmax rescales
(pf_attn_kernel's alpha, tk_service's expf(M - Mn) part merge) only ever see factors near 1.  Here every position is a query, so
each needle is seen as the token's own key (LDS on the persistent kernel), as the last cached row (the clamp target), and across
the moving part boundaries; tiles and parts without a needle are rescaled by ~ e^-30 (e^-190: exactly 0, in the sharp case).

Every case: teacher-forced on the case's tokens, against the f32 C oracle on the (host-decoded) weights, at EVERY position:
rel_err <= REL_TOL, the top-8 element-wise <= REL_TOL, argmax equal where the oracle's top-1 margin is safe.

  attn_kernel<HS>  (multi-kernel decode, f32): head sizes 16 / 32 / 64 / 128, contexts of TILE + 40
  tk_attention + the part merge (persistent kernel): tk-small f32 and tk-small16 f16 over 2,100 positions (1..8 parts), and the
                   sharp case (tk-small f32, 700 positions, beta 64)
  pf_attn_kernel   (llmk_score / llmk_prefill): f32 / f16 / q4_0 at head sizes 64 / 128 / 16, in one call and in two calls
                   with needles on both sides of the split, and decode continuing on the rows prefill wrote

Left out on purpose: the device-side greedy and sample loops (they feed their own tokens and cannot be teacher-forced onto
needles), and the tensor-parallel ranks (they launch these same attention kernels)."""
import numpy as np
import pytest

import attn_needle as an
from conftest import REL_TOL, rel_err, top8_elementwise
from llm_f90_amd import llmk

pytestmark = pytest.mark.gpu

DECODE = [c for c in an.CASES if c.startswith("decode-")]
TK = [c for c in an.CASES if c.startswith("tk-")]
PREFILL = [c for c in an.CASES if c.startswith("prefill-")]


def check(cid, logits, ref, what=""):
    logits = np.asarray(logits).reshape(-1, ref.shape[-1])
    err = rel_err(logits, ref)
    e8 = top8_elementwise(logits, ref=ref)
    safe = an.safe_argmax_positions(ref)
    print(f"{cid} {what}: rel_err max {err.max():.2e} at {int(np.argmax(err))}, top-8 max {e8.max():.2e} at {int(np.argmax(e8))}, "
          f"{int(safe.sum())} of {len(safe)} positions safe for argmax")
    assert err.max() <= REL_TOL, (what, err.max(), int(np.argmax(err)))
    assert e8.max() <= REL_TOL, (what, e8.max(), int(np.argmax(e8)))
    assert len(safe) < 16 or safe.sum() > len(safe) // 2
    assert np.array_equal(np.argmax(logits, axis=1)[safe], np.argmax(ref, axis=1)[safe]), what


def decode_all(m, tokens):
    return np.array([m.forward(int(tok), pos) for pos, tok in enumerate(tokens, 1)])


@pytest.mark.parametrize("cid", DECODE)
def test_multi_kernel_decode_attention_on_needles(cid):
    """attn_kernel<HS>: needles at 0, TPB-1 | TPB, TILE-1 | TILE and the last timestep; rows clamped to pos-1, the second batch"""
    b = an.build_case(cid)
    m = llmk.Llmk(b.fw, flags=llmk.FLAG_MULTI_KERNEL)
    assert m.path() == 0
    logits = decode_all(m, b.tokens)
    m.close()
    check(cid, logits, an.oracle_logits(cid))


@pytest.mark.parametrize("cid", TK)
def test_persistent_kernel_attention_in_parts_on_needles(cid):
    """tk_attention and tk_service's merge: needles at 0, TPB-1 | TPB, TILE-1 | TILE, on both sides of part boundaries at P = 2, 6
    and 8 (attn_needle.TK_PLANS) and on the last timestep.  The sharp case: parts without a needle contribute exactly 0."""
    b = an.build_case(cid)
    m = llmk.Llmk(b.fw)
    assert m.path() == 1, m.path_name()
    logits = decode_all(m, b.tokens)
    assert m.path() == 1, m.path_name()            # no position was redone elsewhere
    m.close()
    check(cid, logits, an.oracle_logits(cid))


@pytest.mark.parametrize("cid", PREFILL)
def test_score_attention_on_needles_in_one_call_and_in_two(cid):
    """pf_attn_kernel behind llmk_score: needles at rows 0, 15 | 16, 127 | 128, split-1 | split, split+15 and the last row"""
    b = an.build_case(cid)
    ref = an.oracle_logits(cid)
    split = an.PF_SPLIT[b.case.shape]
    m = llmk.Llmk(b.fw)
    whole = m.score(b.tokens, 1, want_logits=True, want_logprob=False)
    check(cid, whole, ref, "one call")
    m.reset()
    first = m.score(b.tokens[:split], 1, want_logits=True, want_logprob=False)
    second = m.score(b.tokens[split:], split + 1, want_logits=True, want_logprob=False)
    m.close()
    check(cid, np.concatenate([first, second]), ref, f"two calls, split at {split}")


@pytest.mark.parametrize("cid", PREFILL)
def test_decode_reads_the_needle_rows_prefill_wrote(cid):
    """llmk_prefill of the first k tokens leaves position k's logits, and llmk_forward at k + 1 attends over the rows it wrote:
    k = the split (the next token is a needle) and k = S - 1 (the last timestep is a needle and the token's own key)"""
    b = an.build_case(cid)
    ref = an.oracle_logits(cid)
    m = llmk.Llmk(b.fw)
    for k in (an.PF_SPLIT[b.case.shape], b.case.S - 1):
        m.reset()
        lk = m.prefill(b.tokens[:k], 1)
        nxt = m.forward(int(b.tokens[k]), k + 1)
        check(cid, np.stack([lk, nxt]), ref[k - 1:k + 1], f"prefill {k} + forward")
    m.close()
