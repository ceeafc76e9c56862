"""Is the needle construction (tests/attn_needle.py) sound?  For every case tests/test_attn_needle_gpu.py runs -- shape, weight
type (f16 / q4_0: on the host-decoded weights), needle layout -- three things are checked here, without a GPU:

1. Reference agreement: the f32 C oracle (oracle/llm_oracle.c), teacher-forced on the case's tokens, is within REL_TOL / 2 of
   forward_all(float64) at every position (rel_err: relative to the position's max |logit|).  Peaked softmaxes amplify f32
   rounding of the scores; the cap keeps the project's 1e-4 bar against the oracle meaningful on these inputs.
2. Sensitivity: masking ONE needle timestep in layer 0 moves the f64 logits of EVERY later position by at least
   10 * REL_TOL * max |logit|; for GQA shapes so does reading the neighbouring kv head.  (The needle on the last timestep of a
   context has no later position: it is only ever read as the token's own key.)
3. The mirrors of the kernels' tile and part arithmetic reproduce the headers.

Measured (x86-64, strict f32 oracle), beta = 10 unless noted; "drop" = the smallest change over all needles and later positions,
"shift" = the smallest change over all positions with kv_head_shift = 1, both relative to max |logit|; every needle group holds
> 0.999999 of its heads' layer-0 mass from its first needle on:

    case                              oracle vs f64   drop      shift
    decode-tiny-gqa-f32-1064          4.1e-06         2.6e-01   6.7e-01
    decode-tiny-mha-f32-552           2.9e-06         9.7e-02   --
    decode-tk-small-f32-296           2.8e-06         2.0e-01   8.7e-01
    decode-tiny-hs128-f32-168         3.5e-06         2.1e-01   --
    tk-tk-small-f32-2100              7.6e-06         1.2e-01   7.9e-01
    tk-tk-small16-f16-2100            7.9e-06         1.2e-01   7.3e-01
    tk-tk-small-f32-700-sharp         3.2e-05         1.6e-01   7.9e-01
    prefill-tk-small-long-f32-704     4.3e-06         1.2e-01   7.4e-01
    prefill-tk-small-long-f16-704     5.4e-06         1.2e-01   7.4e-01
    prefill-tk-small-long-q4_0-704    5.4e-06         1.0e-01   7.8e-01
    prefill-tiny-hs128-long-f32-320   6.0e-06         1.1e-01   --
    prefill-tiny-hs128-long-f16-320   5.3e-06         1.1e-01   --
    prefill-tiny-hs128-long-q4_0-320  5.2e-06         9.7e-02   --
    prefill-tiny-gqa-f32-300          4.9e-06         1.3e-01   8.3e-01
    prefill-tiny-gqa-f16-300          6.1e-06         1.3e-01   8.3e-01
    prefill-tiny-gqa-q4_0-300         5.7e-06         1.3e-01   8.2e-01

(The flat softmax of the unshaped weights gives 5.7e-3 * 600 / pos for one dropped timestep: below the 1e-4 bar past pos ~ 3,400
and 20 to 100 times smaller than the figures above wherever the boundary code runs.)

The sharp case: beta is doubled from 16 while the cap of check 1 holds, on tk-small at 700 positions.  oracle vs f64:
beta 16: 7.7e-06, 32: 1.4e-05, 64: 3.2e-05, 128: 5.5e-05 (over the cap of 5e-05) -> BETA_SHARP = 64: needle scores of ~ 190, every
filler's weight below 2^-149 (expf underflows to exactly 0 in f32) and attention parts without a needle contribute nothing to the merge."""
import os
import re
import functools

import numpy as np
import pytest

import attn_needle as an
from conftest import REL_TOL, ROOT, rel_err
from llm_f90_amd.tools import gguf

CSRC = os.path.join(ROOT, "llm.f90_amd", "csrc")


@functools.lru_cache(maxsize=None)
def f64_ref(cid):
    """(f64 logits, forward_all's cache, per kv head: smallest mass of the needle group over the queries from its first needle
    on and the heads that read it, largest single filler weight there).  Shared by the tests of a case; not modified."""
    b = an.build_case(cid)
    cache = {}
    logits, att = an.forward_all(b.fw32, b.tokens, cache=cache)
    s = b.fw32.shape
    kv_mul = s.n_heads // s.n_kv_heads
    mass = {}
    for g, ts in b.layout.items():
        filler = np.ones(len(b.tokens), bool)
        filler[ts] = False
        a = att[g * kv_mul:(g + 1) * kv_mul, min(ts):]
        mass[g] = (float(a[:, :, ts].sum(axis=2).min()), float(a[:, :, filler].max()))
    logits.setflags(write=False)
    return logits, cache, mass


@pytest.mark.parametrize("cid", list(an.CASES))
def test_c_oracle_is_within_half_the_parity_bar_of_the_f64_reference(cid):
    l64, _, _ = f64_ref(cid)
    e = rel_err(an.oracle_logits(cid), l64)
    print(f"{cid}: oracle vs f64 {e.max():.2e} at position {int(np.argmax(e)) + 1}")
    assert e.max() <= REL_TOL / 2, (e.max(), int(np.argmax(e)))


@pytest.mark.parametrize("cid", list(an.CASES))
def test_needles_hold_the_mass_and_dropping_one_moves_every_later_position(cid):
    b = an.build_case(cid)
    l64, cache, mass = f64_ref(cid)
    scale = np.abs(l64).max(axis=1)
    for g, (group, filler) in mass.items():
        print(f"{cid}: kv head {g}: needle group mass >= {group:.9f}, largest filler weight {filler:.2e}")
        assert group > 0.999
    needles = [(g, t) for g, ts in b.layout.items() for t in ts if t + 1 < len(b.tokens)]

    def change(gt):
        ld, _ = an.forward_all(b.fw32, b.tokens, drop=(0, gt[1]), cache=cache)
        return (np.abs(ld - l64).max(axis=1) / scale)[gt[1] + 1:]
    changes = [change(gt) for gt in needles]
    for (g, t), d in zip(needles, changes):
        print(f"{cid}: drop timestep {t} of kv head {g}: change min {d.min():.2e} median {np.median(d):.2e} over {len(d)} later positions")
    for (g, t), d in zip(needles, changes):
        assert d.min() >= 10 * REL_TOL, (g, t, d.min(), t + 1 + int(np.argmin(d)))
    s = b.fw32.shape
    if s.n_heads > s.n_kv_heads > 1:
        ls, _ = an.forward_all(b.fw32, b.tokens, kv_head_shift=1)
        d = np.abs(ls - l64).max(axis=1) / scale
        print(f"{cid}: kv_head_shift=1: change min {d.min():.2e}")
        assert d.min() >= 10 * REL_TOL, (d.min(), int(np.argmin(d)))


def test_sharp_case_filler_weights_underflow_in_f32_and_whole_parts_contribute_nothing():
    cid = "tk-tk-small-f32-700-sharp"
    b = an.build_case(cid)
    _, _, mass = f64_ref(cid)
    for g, (group, filler) in mass.items():
        assert filler < 2.0 ** -149, (g, filler)           # below the smallest f32 subnormal: expf(score - max) is exactly 0
    s = b.fw32.shape
    plan = an.TkAttPlan.of(s.n_heads, s.head_size, b.case.S)
    assert plan.P >= 3
    empty = [p for p in range(plan.P) if not any(plan.t0(p) <= t < plan.t1(p) and t + 1 < b.case.S for t in b.layout[1])]
    assert empty, "at the last position some part of kv head 1's heads must hold no needle"


def test_sharp_beta_is_the_last_doubling_under_the_cap():
    """BETA_SHARP holds the cap (the parametrised test above); twice that does not"""
    import dataclasses
    c = dataclasses.replace(an.CASES["tk-tk-small-f32-700-sharp"], beta=2 * an.BETA_SHARP)
    cid = c.id + "-x2"
    an.CASES[cid] = c
    try:
        b = an.build_case(cid)
        e = rel_err(an.oracle_logits(cid), an.forward_all(b.fw32, b.tokens)[0])
    finally:
        del an.CASES[cid]
    print(f"beta {c.beta}: oracle vs f64 {e.max():.2e}")
    assert e.max() > REL_TOL / 2


def test_forward_all_suffix_run_equals_the_full_run():
    """the drop runs recompute only the rows behind the dropped timestep: same logits as a run without the cache"""
    b = an.build_case("decode-tiny-hs128-f32-168")
    _, cache, _ = f64_ref("decode-tiny-hs128-f32-168")
    a, _ = an.forward_all(b.fw32, b.tokens, drop=(0, 7), cache=cache)
    f, _ = an.forward_all(b.fw32, b.tokens, drop=(0, 7))
    assert np.abs(a - f).max() <= 1e-12 * np.abs(f).max()


def test_forward_all_float32_follows_the_oracle_on_unshaped_weights():
    """forward_all states the reference's conventions (RoPE pairing and exponent, 1-based pos, eps, SwiGLU, GQA): on plain
    synth_fused weights its f32 and f64 passes agree with the C oracle far inside the bar"""
    s = gguf.SHAPES["tiny-gqa"]
    fw = gguf.synth_fused(s, 7)
    from oracle.oracle import Oracle
    toks = np.random.default_rng(3).integers(1, s.vocab_size + 1, s.seq_len)
    o = Oracle(fw, "strict")
    ol = np.array([o.forward(int(t), p) for p, t in enumerate(toks, 1)])
    assert rel_err(ol, an.forward_all(fw, toks)[0]).max() <= REL_TOL / 10
    assert rel_err(an.forward_all(fw, toks, np.float32)[0], ol).max() <= REL_TOL / 10


def test_tile_mirrors_match_the_headers():
    kernels = open(os.path.join(CSRC, "kernels.h")).read()
    tk = open(os.path.join(CSRC, "token_kernel.h")).read()
    pf = open(os.path.join(CSRC, "prefill.h")).read()
    const = lambda text, name: int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))
    assert const(kernels, "ATT_U") == an.ATT_U
    assert "constexpr int TPB = 4 * TPW;" in kernels and "constexpr int TILE = TPB * ATT_U;" in kernels
    assert const(tk, "TK_NCU") == an.TK_NCU and const(tk, "TK_WAVES") == an.TK_WAVES
    assert "TPB = TK_WAVES * TPW, U = 8, TILE = TPB * U;" in tk
    assert "PMAX = HPC < 8 ? HPC : 8;" in tk and "STEP = TILE;" in tk
    assert const(pf, "PF_TMAX") == an.PF_TMAX and const(pf, "PF_ATT_WAVES") == an.PF_ATT_WAVES
    # attn_kernel<HS>: HS/4 lanes per timestep, 4 waves of 64, 16 block-instructions per batch
    assert [an.attn_kernel_tiles(hs) for hs in (16, 32, 64, 128)] == [(64, 1024), (32, 512), (16, 256), (8, 128)]
    # TkAtt: 8 waves, 8 block-instructions per batch
    assert [an.tk_tiles(hs) for hs in (64, 128)] == [(32, 256), (16, 128)]
    assert an.PF_STRIDE == 128


# (n_heads, head size, pos) -> (P, chunk), by hand from token_kernel.h:1141-1146:
#   P = min(PMAX, ceil(pos / TILE)), chunk = ceil(ceil(pos / P) / TPB) * TPB; PMAX = min(256 / n_heads, 8)
PLAN_TABLE = [
    ((4, 64, 1), (1, 32)),            # one part up to TILE = 256 timesteps
    ((4, 64, 256), (1, 256)),
    ((4, 64, 257), (2, 160)),         # ceil(257 / 2) = 129 -> 5 * 32
    ((4, 64, 300), (2, 160)),         # 150 -> 160
    ((4, 64, 513), (3, 192)),         # 171 -> 192
    ((4, 64, 1300), (6, 224)),        # ceil(1300 / 256) = 6; 217 -> 224
    ((4, 64, 2048), (8, 256)),
    ((4, 64, 2100), (8, 288)),        # ceil(2100 / 256) = 9 -> PMAX; 263 -> 288
    ((8, 64, 2100), (8, 288)),        # tk-small16: 32 CUs per head, PMAX still 8
    ((32, 128, 300), (3, 112)),       # head size 128: TPB 16, TILE 128; 100 -> 112
    ((64, 128, 2100), (4, 528)),      # 4 CUs per head: PMAX 4; 525 -> 528
]


@pytest.mark.parametrize("key,want", PLAN_TABLE)
def test_part_plan_mirror_matches_the_headers_formula(key, want):
    plan = an.TkAttPlan.of(*key)
    assert (plan.P, plan.chunk) == want
    pos = key[2]
    assert plan.t0(0) == 0 and plan.t1(plan.P - 1) == pos
    assert all(plan.t1(p) == plan.t0(p + 1) for p in range(plan.P - 1))
    assert all(plan.t0(p) < plan.t1(p) for p in range(plan.P))


def test_layouts_sit_on_the_boundaries_they_name():
    b = an.build_case("tk-tk-small-f32-2100")
    both = sorted(b.layout[0] + b.layout[1])
    assert both == [0, 31, 32, 159, 160, 255, 256, 671, 672, 2015, 2016, 2099]
    assert {an.TkAttPlan.of(4, 64, pos).P for pos, _ in an.TK_PLANS} == {2, 6, 8}
    assert {an.TkAttPlan.of(4, 64, pos).P for pos in range(1, 2101)} == set(range(1, 9))
    for cid, bb in ((c, an.build_case(c)) for c in an.CASES):
        assert not set(bb.layout[0]) & set(bb.layout[1]), cid
        toks = bb.tokens[sorted(bb.layout[0] + bb.layout[1])]
        assert len(set(toks.tolist())) == len(toks), cid              # a token of its own per needle
