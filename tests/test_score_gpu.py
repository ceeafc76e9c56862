"""Batched scoring (llmk_score): per-position log-probs, argmax and logits of a whole prompt in one
call -- the classifier as a GEMM over each batch of the prefill, the log-softmax on the device -- against the real reference's
goldens at EVERY position, against the oracle on host-decoded weights for the f16 / q4_0 / q6_K variants, and for what the call
leaves behind (KV rows, decode continues)."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import score_ref
from conftest import REL_TOL, ROOT, load_golden, rel_err, safe_positions
from llm_f90_amd import llmk
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu


def check(lp, am, lg, ref_logits, targets, safe=None, ref_tokens=None):
    """the three bounds of the issue: logits within REL_TOL at every position; log-probs within 2 * REL_TOL * max|ref logits| of
    score_ref on the reference's logits (the log-sum-exp moves by at most the largest logit error, the target's logit by the
    same); argmax equal wherever the reference's top-1 margin is safe"""
    ref_logits = np.asarray(ref_logits)
    e = rel_err(lg, ref_logits)
    rlp, ram = score_ref.score(ref_logits, targets)
    scale = np.abs(ref_logits).max(axis=1)
    dlp = np.abs(lp.astype(np.float64) - rlp)
    print(f"max rel err logits {e.max():.3e}; max |logprob diff| {dlp.max():.3e} (bound {2 * REL_TOL * scale.min():.3e} ..); "
          f"max |logprob diff| / (max|logit|) {np.max(dlp / scale):.3e}")
    assert e.max() <= REL_TOL, (int(np.argmax(e)), e.max())
    assert (dlp <= 2 * REL_TOL * scale).all(), (int(np.argmax(dlp / scale)), dlp.max())
    if safe is None:
        top2 = np.sort(ref_logits, axis=1)[:, -2:]
        safe = (top2[:, 1] - top2[:, 0]) > 4 * REL_TOL * scale
    else:
        assert safe.mean() >= 0.99, safe.mean()               # (the goldens: at most 1 % of a case's positions may be unsafe)
    want = ram if ref_tokens is None else np.asarray(ref_tokens)
    assert np.array_equal(am[safe], want[safe])


@pytest.mark.parametrize("tag", ["tiny-gqa", "tiny-mha", "tiny-hs64", "tiny-hs128", "tiny-70bish", "tk-small", "tk-small-long",
                                 "tiny-hs128-long"])
def test_score_matches_the_real_reference_at_every_position(tag, gguf):
    g = load_golden(tag)
    fw = gguf.synth_fused(gguf.SHAPES[str(g["shape"])], int(g["seed"]))
    n = len(g["tokens"])
    fed = ([2] + g["tokens"].tolist())[:n]
    m = llmk.Llmk(fw)
    tg = score_ref.default_targets(fed)
    lp, am, lg = m.score(fed, 1, want_argmax=True, want_logits=True)
    assert lp[-1] == 0.0
    check(lp, am, lg, g["logits"][:n], tg, safe_positions(g, n), g["tokens"][:n])
    m.close()


def _variant(gguf, fw, variant):
    if variant == "q4_0+q6_K":
        return gguf.with_q6k_classifier(fw)
    if variant == "q4_0+f32cls":
        return dataclasses.replace(fw, wcls=gguf.decode(fw.wcls, fw.cls_type, fw.shape.emb_dim), wcls_type=0)
    return fw


def _oracle_logits(fw32, seq):
    o = Oracle(fw32, "omp")
    return np.array([o.forward(tok, pos) for pos, tok in enumerate(seq, 1)])


@pytest.mark.parametrize("variant", ["f16", "q4_0", "q4_0+q6_K", "q4_0+f32cls"])
@pytest.mark.parametrize("shape,n", [("tk-small-long", 1), ("tk-small-long", 17), ("tk-small-long", 129), ("tiny-hs64", 17), ("tiny-hs64", 90)])
def test_score_variants_match_oracle_on_decoded_weights(variant, shape, n, gguf):
    s = gguf.SHAPES[shape]
    fw = _variant(gguf, gguf.synth_fused(s, 4242, 1 if variant == "f16" else 2), variant)
    rng = np.random.default_rng(6)
    seq = [2] + (rng.integers(3, s.vocab_size, n - 1) + 1).tolist()
    tg = rng.integers(1, s.vocab_size + 1, n).astype(np.int32)
    ref = _oracle_logits(fw.as_f32(), seq)
    m = llmk.Llmk(fw)
    lp, am, lg = m.score(seq, 1, targets=tg, want_argmax=True, want_logits=True)
    check(lp, am, lg, ref, tg)
    m.close()


def test_score_tinyllama_150_positions_vs_oracle(gguf):
    """BASELINE.json's shape, two batches (128 + 22), V = 32,000 in three row chunks"""
    s = gguf.SHAPES["tinyllama"]
    fw = gguf.synth_fused(s, 20260928)
    rng = np.random.default_rng(1)
    seq = [2] + (rng.integers(3, s.vocab_size, 149) + 1).tolist()
    ref = _oracle_logits(fw, seq)
    m = llmk.Llmk(fw)
    tg = score_ref.default_targets(seq)
    lp, am, lg = m.score(seq, 1, want_argmax=True, want_logits=True)
    check(lp, am, lg, ref, tg)
    ms, b = m.time_kernel(12, 5)
    assert ms > 0 and b == s.vocab_size * s.emb_dim * 4
    m.close()


@pytest.mark.parametrize("shape", ["tk-small-long", "tiny-mha"])
def test_score_outputs_are_independent_and_repeatable(shape, gguf):
    """every subset of the three outputs gives the bits all three give; so does a second call; targets == 0 gives 0.0"""
    s = gguf.SHAPES[shape]
    m = llmk.Llmk(gguf.synth_fused(s, 99))
    rng = np.random.default_rng(2)
    n = min(150, s.seq_len)
    seq = [2] + (rng.integers(3, s.vocab_size, n - 1) + 1).tolist()
    tg = rng.integers(0, s.vocab_size + 1, n).astype(np.int32)
    tg[[0, 5, n - 1]] = 0
    lp, am, lg = m.score(seq, 1, targets=tg, want_argmax=True, want_logits=True)
    assert (lp[tg == 0] == 0.0).all() and (lp[tg > 0] < 0.0).all()
    for wl, wa, wg in [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]:
        m.reset()
        out = m.score(seq, 1, targets=tg, want_logprob=bool(wl), want_argmax=bool(wa), want_logits=bool(wg))
        out = list(out) if isinstance(out, tuple) else [out]
        if wl:
            assert np.array_equal(out.pop(0).view(np.uint32), lp.view(np.uint32))
        if wa:
            assert np.array_equal(out.pop(0), am)
        if wg:
            assert np.array_equal(out.pop(0).view(np.uint32), lg.view(np.uint32))
    m.close()


def test_score_leaves_what_prefill_leaves_and_decode_continues(gguf):
    s = gguf.SHAPES["tk-small-long"]
    fw = gguf.synth_fused(s, 31)
    rng = np.random.default_rng(9)
    n = 140
    seq = [2] + (rng.integers(3, s.vocab_size, n - 1) + 1).tolist()
    a, b = llmk.Llmk(fw), llmk.Llmk(fw)
    la = a.prefill(seq, 1)
    lp, am, lg = b.score(seq, 1, want_argmax=True, want_logits=True)
    for layer in range(s.n_layers):
        for pos in (1, 17, 128, 129, n):
            for which in (4, 5):
                assert np.array_equal(a.peek(which, s.kv_dim, layer, pos), b.peek(which, s.kv_dim, layer, pos))
    assert rel_err(lg[-1][None], la[None]).max() <= REL_TOL
    first = int(np.argmax(la)) + 1
    assert am[-1] == first
    assert np.array_equal(a.decode_greedy(first, n + 1, 12), b.decode_greedy(first, n + 1, 12))
    a.close(); b.close()


def test_score_in_two_calls_and_after_decode(gguf):
    s = gguf.SHAPES["tiny-gqa"]
    fw = gguf.synth_fused(s, 31)
    rng = np.random.default_rng(9)
    seq = [2] + (rng.integers(3, s.vocab_size, 39) + 1).tolist()
    tg = score_ref.default_targets(seq)
    a, b = llmk.Llmk(fw), llmk.Llmk(fw)
    lp, am, lg = a.score(seq, 1, want_argmax=True, want_logits=True)
    for pos in range(1, 6):
        b.forward(seq[pos - 1], pos)
    lp1, am1, lg1 = b.score(seq[5:18], 6, targets=tg[5:18], want_argmax=True, want_logits=True)
    lp2, am2, lg2 = b.score(seq[18:], 19, targets=tg[18:], want_argmax=True, want_logits=True)
    check(np.concatenate([lp1, lp2]), np.concatenate([am1, am2]), np.concatenate([lg1, lg2]), lg[5:], tg[5:])
    a.close(); b.close()


def test_score_on_the_multi_kernel_flag(gguf):
    g = load_golden("tk-small")
    fw = gguf.synth_fused(gguf.SHAPES[str(g["shape"])], int(g["seed"]))
    n = len(g["tokens"])
    fed = ([2] + g["tokens"].tolist())[:n]
    m = llmk.Llmk(fw, flags=llmk.FLAG_MULTI_KERNEL)
    lp, am, lg = m.score(fed, 1, want_argmax=True, want_logits=True)
    check(lp, am, lg, g["logits"][:n], score_ref.default_targets(fed), safe_positions(g, n), g["tokens"][:n])
    m.close()


CHILD = r'''
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import llm_f90_amd
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf
import score_ref
z = np.load(sys.argv[1] + "/tests/golden/" + sys.argv[2] + ".npz")
fw = gguf.synth_fused(gguf.SHAPES[str(z["shape"])], int(z["seed"]))
n = len(z["tokens"])
fed = ([2] + z["tokens"].tolist())[:n]
m = llmk.Llmk(fw)
lp, am, lg = m.score(fed, 1, want_argmax=True, want_logits=True)
ref = z["logits"][:n].astype(np.float64)
scale = np.abs(ref).max(axis=1)
rlp, ram = score_ref.score(ref, score_ref.default_targets(fed))
print(json.dumps({"rel": float((np.abs(lg - ref).max(axis=1) / scale).max()), "lp": float((np.abs(lp - rlp) / scale).max()),
                  "am_diff": np.nonzero(am != z["tokens"][:n])[0].tolist()}))
m.close()
'''


@pytest.mark.parametrize("env", [{"LLMK_PF_F32_MFMA": "1"}, {"LLMK_PREFILL": "0"}], ids=["f32-mfma", "prefill-off"])
def test_score_on_the_other_paths_in_a_child_process(env, gguf):
    tag = "tk-small-long"
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, tag], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    g = load_golden(tag)
    assert out["rel"] <= REL_TOL and out["lp"] <= 2 * REL_TOL
    unsafe = np.nonzero(~safe_positions(g))[0].tolist()
    assert set(out["am_diff"]) <= set(unsafe)


def test_score_argument_errors(gguf):
    s = gguf.SHAPES["tiny-gqa"]
    m = llmk.Llmk(gguf.synth_fused(s, 1))
    L, h = llmk.lib(), m._h
    import ctypes as C
    tok = (C.c_int * 4)(2, 5, 6, 7)
    lp, am = (C.c_float * 4)(), (C.c_int * 4)()
    bad = (C.c_int * 4)(5, s.vocab_size + 1, 0, 0)
    neg = (C.c_int * 4)(5, -1, 0, 0)
    ok = (C.c_int * 4)(5, 6, 7, 0)
    assert L.llmk_score(h, tok, 4, 1, bad, lp, am, None) == 1               # target out of range
    assert L.llmk_score(h, tok, 4, 1, neg, lp, am, None) == 1
    assert L.llmk_score(h, tok, 4, 1, ok, None, None, None) == 1            # nothing asked for
    assert L.llmk_score(h, tok, 4, 1, None, lp, am, None) == 1              # log-probs without targets
    assert L.llmk_score(h, tok, 4, s.seq_len - 2, ok, lp, am, None) == 1    # runs past the context
    assert L.llmk_score(h, tok, 0, 1, ok, lp, am, None) == 1
    zero = (C.c_int * 4)(2, 0, 6, 7)
    assert L.llmk_score(h, zero, 4, 1, ok, lp, am, None) == 1               # token id out of range
    assert L.llmk_score(h, tok, 4, 1, None, None, am, None) == 0            # argmax alone needs no targets
    out = m.score([2, 5, 6, 7], 1)
    assert out.shape == (4,) and out[-1] == 0.0 and (out[:3] < 0).all()
    m.close()


LLM = os.path.join(ROOT, "llm.f90_amd", "host", "llm")


def _host_rope_table(hs):
    """The RoPE frequencies as the Fortran host computes them (host/llm.f90: 1 / 10000 ** ((2j-1) / hs) in f32, the power through
    libm's powf).  numpy's float32 power differs from powf by one ulp in 7 of the 32 frequencies at head size 64, which moves a
    log-prob by an f32 ulp here and there: both programs must start from the same table to agree to the printed digits."""
    import ctypes
    libm = ctypes.CDLL("libm.so.6")
    libm.powf.restype, libm.powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    return np.array([np.float32(1.0) / np.float32(libm.powf(10000.0, float(np.float32(2 * j - 1) / np.float32(hs)))) for j in range(1, hs // 2 + 1)],
                    np.float32)


def test_cli_score_prints_the_bindings_logprobs_and_the_perplexity(gguf, tmp_path):
    """`llm --score -p ...` on a small synthetic GGUF whose vocabulary encodes the prompt: one `index id logprob` line per scored
    token, equal to Llmk.score's to the printed digits; then tokens, sum logprob, perplexity = exp(-sum / count), the rate"""
    s = gguf.SHAPES["tk-small"]
    path = str(tmp_path / "synth.gguf")
    gguf.write_synth_gguf(path, s, 3)
    prompt = "Once upon a time"
    enc = subprocess.run([LLM, "-m", path, "-p", prompt, "--encode"], capture_output=True, cwd=str(tmp_path), timeout=120)
    assert enc.returncode == 0, enc.stdout + enc.stderr
    ptoks = [int(t) for t in enc.stdout.strip().split(b"\n")[-1].split()]
    k = len(ptoks)
    assert k > 1
    m = llmk.Llmk(gguf.synth_fused(s, 3))
    m.set_rope_freqs(_host_rope_table(s.head_size))
    lp = m.score([2] + ptoks[:-1], 1, targets=ptoks)
    m.close()
    r = subprocess.run([LLM, "-m", path, "-p", prompt, "--score"], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.split("\n") if l.strip()]
    rows = [l for l in lines if len(l) == 3 and l[0].isdigit() and l[1].isdigit()]
    assert [int(l[0]) for l in rows] == list(range(1, k + 1)) and [int(l[1]) for l in rows] == ptoks
    for l, want in zip(rows, lp):
        assert l[2] == f"{float(want):.8E}", (l, want)
    printed = np.array([float(l[2]) for l in rows])
    named = {" ".join(l[:-1]): l[-1] for l in lines if len(l) >= 2 and not l[0][0].isdigit() and l[0][0] != "-"}
    assert int(named["tokens"]) == k
    assert abs(float(named["sum logprob"]) - printed.sum()) <= 1e-6 * abs(printed.sum())
    assert abs(float(named["perplexity"]) - np.exp(-printed.mean())) <= 2e-6 * np.exp(-printed.mean())
    rate = [l for l in lines if l[-1] == "positions/second"]
    assert len(rate) == 1 and float(rate[0][0]) > 0
    bad = subprocess.run([LLM, "-m", path, "-p", "", "--score"], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert bad.returncode != 0 and "at least one token" in bad.stdout


@pytest.mark.parametrize("case", ["large", "small"])
def test_score_range_flag_redoes_the_call_on_the_f32_instruction(case, gguf):
    """The f16-range flag covers a scoring call as it covers llmk_prefill (tests/test_prefill_gpu.py has the two constructions):
    FFN gains of 1e5 put activations beyond 65504 (bit 0: the context stays on the f32 instruction), attention gains of 2^-10
    with wo * 2^10 put whole rows below 2^-7 (bit 1: this call alone is redone).  Either way the call returns the redone
    values: every position within the bounds of the oracle, and a second call gives the same bits."""
    s = gguf.SHAPES["tk-small16"]
    fw = gguf.synth_fused(s, 77 if case == "large" else 78, 0)
    if case == "large":
        fw.rms_ffn_weight = (fw.rms_ffn_weight * np.float32(1e5)).astype(np.float32)
    else:
        fw.rms_att_weight = (fw.rms_att_weight * np.float32(2.0 ** -10)).astype(np.float32)
        fw.wo = (fw.wo * fw.wo.dtype.type(1024)).astype(fw.wo.dtype)
    rng = np.random.default_rng(11)
    n = 41
    seq = [2] + (rng.integers(3, s.vocab_size, n - 1) + 1).tolist()
    tg = score_ref.default_targets(seq)
    ref = _oracle_logits(fw, seq)
    assert np.all(np.isfinite(ref))
    m = llmk.Llmk(fw)
    lp, am, lg = m.score(seq, 1, want_argmax=True, want_logits=True)
    check(lp, am, lg, ref, tg)
    m.reset()
    lp2, am2, lg2 = m.score(seq, 1, want_argmax=True, want_logits=True)
    assert np.array_equal(lp.view(np.uint32), lp2.view(np.uint32)) and np.array_equal(am, am2) and np.array_equal(lg.view(np.uint32), lg2.view(np.uint32))
    m.close()


def test_score_a_position_without_a_finite_logit_is_an_error(gguf):
    """final gains of +inf make every logit of every position +-inf or NaN: LLMK_E_NONFINITE (11), not an id"""
    s = gguf.SHAPES["tiny-gqa"]
    fw = gguf.synth_fused(s, 5)
    fw.rms_final_weight = np.full_like(fw.rms_final_weight, np.inf)
    m = llmk.Llmk(fw)
    with pytest.raises(llmk.LlmkError) as ei:
        m.score([2, 5, 6], 1, want_argmax=True)
    assert ei.value.code == 11
    m.close()


FLAG_CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import llm_f90_amd
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf
case = sys.argv[2]
s = gguf.SHAPES["tk-small16"]
fw = gguf.synth_fused(s, 77 if case == "large" else 78, 0)
if case == "large":
    fw.rms_ffn_weight = (fw.rms_ffn_weight * np.float32(1e5)).astype(np.float32)
elif case == "small":
    fw.rms_att_weight = (fw.rms_att_weight * np.float32(2.0 ** -10)).astype(np.float32)
    fw.wo = (fw.wo * fw.wo.dtype.type(1024)).astype(fw.wo.dtype)
rng = np.random.default_rng(11)
seq = [2] + (rng.integers(3, s.vocab_size, 40) + 1).tolist()
m = llmk.Llmk(fw)
lp = m.score(seq, 1)
assert np.isfinite(lp).all()
m.close()
'''


@pytest.mark.parametrize("case,note", [("large", "llmk_score met an activation beyond the f16 range"),
                                       ("small", "llmk_score met a position whose activations are all below 2^-7"), ("plain", None)])
def test_score_range_flag_really_rises(case, note):
    """the inputs of the test above, in a process of their own (the note is printed once per process): the redo branch of
    llmk_score says on stderr which bit of the flag it met; ordinary weights raise nothing"""
    r = subprocess.run([sys.executable, "-c", FLAG_CHILD, ROOT, case], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    if note:
        assert note in r.stderr, r.stderr[-2000:]
    else:
        assert "llmk_score met" not in r.stderr, r.stderr[-2000:]
