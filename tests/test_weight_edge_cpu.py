"""Weight-format edge inputs without a GPU (tests/weight_edge.py): the scalar decoders against the vectorised ones and against the
Fortran loader on every crafted family, forward64 against the f32 oracle class by class, and a list of deliberately wrong
decoders, each of which the inputs and the bar of the GPU tests (test_weight_edge_gpu.py) must catch."""
import os
import subprocess

import numpy as np
import pytest

import weight_edge as we
from conftest import REL_TOL, rel_err
from oracle.oracle import Oracle
from test_host_cpu import FC, _read_dump, tools  # noqa: F401  (the loader_dump build of the host tests)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_class_err_is_rel_err_within_a_class_and_falls_back_to_the_position_for_a_zero_class():
    ref = np.array([[4.0, 0.0, 1e-3, -2.0, 0.0, 2e-3]])
    got = ref + np.array([[4e-4, 1e-6, 1e-7, 0.0, 0.0, 0.0]])
    e = we.class_err(got, ref, np.array([0, 1, 2, 0, 1, 2]))
    assert np.allclose(e[0], [4e-4 / 4.0, 1e-6 / 4.0, 1e-7 / 2e-3])
    assert rel_err(got, ref)[0] == pytest.approx(1e-4)                   # the whole-position figure: class 2's 5e-5 is invisible in it
    assert np.isnan(we.class_err(got, ref, np.array([0, 0, 0, 3, 3, 3]))[0, 1])          # no row of class 1: not a figure
    got[0, 2] = np.nan                                                     # a NaN in the output of class 2 is NOT "within the bar":
    e = we.class_err(got, ref, np.array([0, 1, 2, 0, 1, 2]))[0]            # callers assert `err <= REL_TOL`, which a NaN fails
    assert np.isnan(e[2]) and not e[2] <= REL_TOL and e[0] <= 4 * REL_TOL and not rel_err(got, ref)[0] <= REL_TOL
    got[0, 1] = np.inf                                                     # ... and so does an infinity in a zero class
    assert not we.class_err(got, ref, np.array([0, 1, 2, 0, 1, 2]))[0, 1] <= REL_TOL


def test_report_turns_red_on_a_nan_or_an_infinity_in_one_class():
    """the per-class and the whole-position checks are `not (err <= REL_TOL)`: a NaN cannot pass as "not larger than the bar"."""
    ref, classes = np.array([4.0, 0.0, 1e-3, -2.0, 0.0, 2e-3]), np.array([0, 1, 2, 0, 1, 2])
    for bad in (np.nan, np.inf):
        r = we.Report("self-check")
        got = ref.copy()
        got[2] = bad
        r.add("logits", 1, got, ref, classes)
        r.whole(1, got, ref)
        assert [(w, c) for w, _, c, _ in r.red] == [("logits", "2"), ("whole position", "-")]
        with pytest.raises(AssertionError):
            r.finish()
    r = we.Report("self-check")
    r.add("logits", 1, ref, ref, classes)
    r.whole(1, ref, ref)
    r.finish()


def test_scalar_decoders_equal_the_vectorised_ones_bit_for_bit_on_every_crafted_family(gguf):
    """Every class, every sub-variant the row index cycles through (sign of d and of zero, scale values, live sub-block and
    super-block, code patterns), row-wise and pair-wise classes: the plain loops of weight_edge against tools/gguf.py."""
    K = 512
    for pair in (False, True):
        raw, cls = we.craft_q6k(9 * 14, K, 3, pair)
        assert set(cls) == set(range(9))
        ref = gguf.dequantize_q6_K(raw, K)
        assert np.abs(ref).max() <= 8 and np.all(np.isfinite(ref))
        assert np.all(ref[np.isin(cls, we.Q6K_ZERO)] == 0) and np.all(np.any(ref[~np.isin(cls, we.Q6K_ZERO)] != 0, axis=1))
        for r in range(len(raw)):
            assert np.array_equal(_bits(we.q6k_scalar(raw[r], K)), _bits(ref[r])), (pair, r, cls[r])
        raw, cls = we.craft_q4_0(7 * 16, K, 4, True, pair)
        assert set(cls) == set(range(7))
        ref = gguf.dequantize_q4_0(raw, K)
        assert np.abs(ref).max() <= 8 and np.all(ref[cls == 0] == 0)
        for r in range(len(raw)):
            assert np.array_equal(_bits(we.q4_0_scalar(raw[r], K)), _bits(ref[r])), (pair, r, cls[r])
        assert set(we.craft_q4_0(70, K, 4, False)[1]) == {3, 4, 5, 6}      # no tiny class where a row cannot be read out alone
        h, cls = we.craft_f16(5 * 8, K, 5, True, pair)
        ref = gguf.decode(h, 1, K)
        for r in range(len(h)):
            assert np.array_equal(_bits(we.f16_row_scalar(h[r].view(np.uint16))), _bits(ref[r])), (pair, r, cls[r])
        sub = h[cls == 0].view(np.uint16)
        assert np.all((sub & 0x7C00) == 0) and np.all((sub & 0x3FF) != 0)   # all subnormal, none zero
        assert np.any(h.view(np.uint16) == 0x8000) and np.any(h.view(np.uint16) == 0)


def test_crafted_q6k_rows_cover_what_the_quantiser_never_emits(gguf):
    """the facts of the issue, turned round: negative, zero and -128 scales, scales below 61, d of both signs, normal and subnormal d"""
    raw, cls = we.craft_q6k(9 * 32, 1024, 20261019)
    b = raw.reshape(-1, 210)
    sc = b[:, 192:208].view(np.int8)
    d = b[:, 208:210].copy().view(np.float16).reshape(-1)
    assert {-128, -127, -64, -1, 0, 1, 63, 127} <= set(np.unique(sc).tolist())
    assert np.any(d < 0) and np.any(d > 0) and np.any(np.abs(d) >= 2.0 ** -14) and np.any((d != 0) & (np.abs(d) < 2.0 ** -14))
    a = raw[cls == 0].reshape(-1, 210)
    da = a[:, 208:210].copy().view(np.float16).reshape(-1)
    assert np.all(da <= -2.0 ** -14) and np.all(a[:, 192:208].view(np.int8) < 0)
    live = (raw[cls == 3].reshape(-1, 4, 210)[:, :, 192:208] != 0)
    assert np.all(live.reshape(len(live), -1).sum(axis=1) == 1)
    assert len({tuple(np.argwhere(x)[0]) for x in live}) == len(live)      # 32 rows: 32 different (super-block, sub-block) places


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not installed")
@pytest.mark.parametrize("mat_type", [1, 2], ids=["f16", "q4_0"])
def test_fortran_loader_decodes_every_crafted_family_like_the_scalar_decoders(tools, gguf, mat_type):  # noqa: F811
    """The crafted rows through a GGUF file and host/gguf_loader.f90 (LLM_DEQUANT_CLS=1: q6k_weight decodes the classifier): the
    decoded q6_K classifier equals q6k_scalar bit for bit on every row; the f16 / q4_0 matrices are handed over as bytes -- the
    same bytes, and the scalar decoders read them like the vectorised ones; without LLM_DEQUANT_CLS the classifier's bytes."""
    d = tools["dir"]
    s = gguf.LlamaShape(512, 512, 1, 8, 2, 288, 32)                        # two super-blocks per classifier row
    fw, _ = we.craft_model(gguf, s, mat_type, 14, 77)
    path, out = str(d / f"edge-{mat_type}.gguf"), str(d / f"edge-{mat_type}.bin")
    gguf.write_gguf(path, fw)                                              # (wcls_type 14: the writer stores the raw super-blocks)
    subprocess.run([tools["dump"], path, out], capture_output=True, check=True, env=dict(os.environ, LLM_DEQUANT_CLS="1"))
    got = _read_dump(out, gguf)
    assert got["wtype"] == mat_type and got["wcls_type"] == 0
    cls = got["wcls"].reshape(-1).view("<f4").reshape(s.vocab_size, s.emb_dim)
    for r in range(s.vocab_size):
        assert np.array_equal(_bits(cls[r]), _bits(we.q6k_scalar(fw.wcls[r], s.emb_dim))), r
    for name, K in (("wqkv", 512), ("wo", 512), ("w13", 512), ("w2", 512)):
        mine = np.ascontiguousarray(getattr(fw, name)[0])
        assert np.array_equal(got[name].reshape(-1), mine.view(np.uint8).reshape(-1)), name
        dumped = got[name].reshape(mine.shape[0], -1)
        full = gguf.decode(dumped if mat_type == 2 else dumped.view("<f2"), mat_type, K)
        for r in range(0, mine.shape[0], 9):                               # (9 is coprime to the 5 and 7 classes: every class, many rows)
            row = we.q4_0_scalar(dumped[r], K) if mat_type == 2 else we.f16_row_scalar(dumped[r].view("<u2"))
            assert np.array_equal(_bits(row), _bits(full[r])), (name, r)
    env = {k: v for k, v in os.environ.items() if k != "LLM_DEQUANT_CLS"}
    subprocess.run([tools["dump"], path, out], capture_output=True, check=True, env=env)
    got = _read_dump(out, gguf)
    assert got["wcls_type"] == 14 and np.array_equal(got["wcls"].reshape(-1), fw.wcls.reshape(-1))


# what the GPU tests assert, per position: (quantity, the classes of its rows)
ASSERTED = ("logits", "k", "v")


def _worst(got, ref, rc):
    """{quantity: worst class_err over positions and classes}, plus the whole position's rel_err of the logits"""
    out = {q: we.worst(we.class_err(got[q], ref[q].reshape(-1, ref[q].shape[-1]), rc[q])) for q in got if q != "whole"}
    out["whole"] = float(rel_err(got["logits"], ref["logits"]).max())
    return out


@pytest.mark.parametrize("name", list(we.MODELS))
def test_forward64_agrees_with_the_f32_oracle_within_a_quarter_of_the_bar_in_every_class(name, gguf):
    """The reference of the GPU tests against the project's own: oracle/llm_oracle.c (f32, sequential sums) on the same decoded
    weights, teacher-forced over the 5 positions.  Per class, logits, K rows, V rows and the residual stream x: the oracle alone
    stays at or below REL_TOL / 4 = 2.5e-5 (the factor safe_positions uses), so the bar of the GPU tests is a bar on the kernels.
    Measured (worst class over the 5 positions; x86-64; `whole` is rel_err of the logits):
        model               logits    k         v         x         whole
        q6k-E256-f16        8.1e-07   7.6e-07   6.9e-07   1.2e-06   8.0e-07
        q6k-E1024-q4        1.8e-06   1.3e-06   1.2e-06   1.4e-06   1.3e-06
        tinyllama-q4-q6k    2.5e-06   3.2e-06   2.4e-06   2.2e-06   2.1e-06
        llama7b-q4-q6k      3.2e-06   3.7e-06   3.0e-06   3.6e-06   2.8e-06
        tinyllama-q4        2.5e-06   3.2e-06   2.4e-06   2.2e-06   2.2e-06
        tk-small-q4         7.7e-07   7.7e-07   5.7e-07   1.2e-06   7.6e-07
        tiny-70bish-q4      2.1e-06   1.3e-06   1.2e-06   1.9e-06   1.7e-06
        tk-small16-f16      8.5e-06   9.4e-07   1.3e-06   2.1e-06   3.9e-06
    (tk-small16-f16: the class of one non-zero weight per row -- a logit that is one activation; the largest figure is still about
    a third of REL_TOL / 4.)
    """
    fw, rc, ref = we.model(gguf, name)
    s = fw.shape
    o = Oracle(we.decoded(gguf, fw), "omp" if s.emb_dim >= 2048 else "strict")
    n = len(we.TOKENS)
    got = {"logits": np.empty((n, s.vocab_size)), "x": np.empty((n, s.emb_dim))}
    for pos, tok in enumerate(we.TOKENS, start=1):
        got["logits"][pos - 1], tr = o.forward(tok, pos, trace=True)
        got["x"][pos - 1] = tr[s.n_layers - 1]
    got["k"], got["v"] = o.key_cache[0, :n], o.value_cache[0, :n]
    w = _worst(got, {q: (ref[q][0] if q in ("k", "v") else ref[q]) for q in ("logits", "k", "v", "x")}, rc)
    print("oracle vs forward64 %-18s" % name, " ".join("%s %.1e" % kv for kv in w.items()))
    assert max(w.values()) <= REL_TOL / 4, w


# ---- deliberately wrong decoders, one fault each ---------------------------------------------------------------------
def _f16(b2):
    return b2.copy().view(np.float16).astype(np.float32)


def q6k_np(raw, K, fault=None):
    """ggml's dequantize_row_q6_K in numpy, with one fault"""
    rows = raw.shape[0]
    b = raw.reshape(-1, 210)
    ql = b[:, 0:128].reshape(-1, 2, 64).astype(np.int32)
    qh = b[:, 128:192].reshape(-1, 2, 32).astype(np.int32)
    sc = (b[:, 192:208] if fault == "scale unsigned" else b[:, 192:208].view(np.int8)).reshape(-1, 2, 8).astype(np.float32)
    d = _f16(b[:, 208:210]).reshape(-1)
    if fault == "|d|":
        d = np.abs(d)
    if fault == "d of super-block 0":
        d = np.repeat(d.reshape(rows, -1)[:, :1], K // 256, axis=1).reshape(-1)
    if fault == "subnormal flushed":
        d = np.where(np.abs(d) < 2.0 ** -14, np.float32(0), d)
    sh = (0, 4, 2, 6) if fault == "qh fields of k = 1, 2 swapped" else (0, 2, 4, 6)
    q = np.empty((b.shape[0], 2, 4, 32), np.int32)
    q[:, :, 0] = (ql[:, :, 0:32] & 15) | (((qh >> sh[0]) & 3) << 4)
    q[:, :, 1] = (ql[:, :, 32:64] & 15) | (((qh >> sh[1]) & 3) << 4)
    q[:, :, 2] = (ql[:, :, 0:32] >> 4) | (((qh >> sh[2]) & 3) << 4)
    q[:, :, 3] = (ql[:, :, 32:64] >> 4) | (((qh >> sh[3]) & 3) << 4)
    q -= 31 if fault == "offset 31" else 32
    lsub = np.zeros(32, np.int64) if fault == "l / 16 dropped" else np.arange(32) // 16
    idx = lsub[None, :] + 2 * np.arange(4)[:, None]                                   # scales[8 n + 2 k + l / 16]
    scq = (np.broadcast_to(sc[:, :1], sc.shape) if fault == "half n dropped" else sc)[:, :, idx]
    return ((d[:, None, None, None] * scq) * q.astype(np.float32)).reshape(rows, K)


def q4_np(raw, K, fault=None):
    rows = raw.shape[0]
    b = raw.reshape(rows, K // 32, 18)
    d = _f16(np.ascontiguousarray(b[:, :, 0:2])).reshape(rows, -1)
    if fault == "|d|":
        d = np.abs(d)
    if fault == "block scale index + 1":
        d = np.roll(d, -1, axis=1)
    if fault == "subnormal flushed":
        d = np.where(np.abs(d) < 2.0 ** -14, np.float32(0), d)
    lo, hi = (b[:, :, 2:] & 15).astype(np.int32), (b[:, :, 2:] >> 4).astype(np.int32)
    if fault == "halves swapped":
        lo, hi = hi, lo
    nib = np.concatenate([lo, hi], axis=2)
    if fault == "signed nibble":
        v = np.where(nib >= 8, nib - 16, nib)
    else:
        v = nib - (7 if fault == "offset 7" else 8)
    return (v.astype(np.float32) * d[:, :, None]).reshape(rows, K)


def f16_np(h, K, fault=None):
    w = h.astype(np.float32)
    return np.where(np.abs(w) < 2.0 ** -14, np.float32(0), w) if fault == "subnormal flushed" else w


MUTANTS = [("q6k-E1024-q4", 14, f) for f in ("scale unsigned", "|d|", "l / 16 dropped", "half n dropped", "qh fields of k = 1, 2 swapped",
                                            "d of super-block 0", "offset 31", "subnormal flushed")] + \
          [(m, 2, f) for m in ("tk-small-q4",) for f in ("halves swapped", "block scale index + 1", "offset 7", "signed nibble", "|d|",
                                                                             "subnormal flushed")] + \
          [("tk-small16-f16", 1, "subnormal flushed")]
DECODERS = {14: q6k_np, 2: q4_np, 1: f16_np}


def _decode_with(gguf, fw, wtype, fault):
    """fw.as_f32() with every tensor of type `wtype` read by the numpy decoder with `fault`"""
    d = fw.as_f32()
    E, H = fw.shape.emb_dim, fw.shape.hidden_dim
    dec = DECODERS[wtype]
    if fw.cls_type == wtype:
        d.wcls = dec(fw.wcls, E, fault)
    if fw.ggml_type == wtype:
        for name, K in (("wqkv", E), ("wo", E), ("w13", E), ("w2", H)):
            setattr(d, name, dec(getattr(fw, name)[0], K, fault)[None])
    return d


def test_the_unfaulted_numpy_decoders_are_the_decoders(gguf):
    for name, wtype in (("q6k-E1024-q4", 14), ("tk-small-q4", 2), ("tk-small16-f16", 1)):
        fw = we.model(gguf, name)[0]
        a, b = _decode_with(gguf, fw, wtype, None), fw.as_f32()
        for f in ("wqkv", "wo", "w13", "w2", "wcls"):
            assert np.array_equal(_bits(getattr(a, f)), _bits(getattr(b, f))), (name, f)


@pytest.mark.parametrize("name,wtype,fault", MUTANTS, ids=["%s-%s" % ({14: "q6_K", 2: "q4_0", 1: "f16"}[t], f.replace(" ", "_")) for _, t, f in MUTANTS])
def test_a_decoder_with_one_fault_is_caught_by_the_inputs_and_the_bar_of_the_gpu_tests(name, wtype, fault, gguf):
    """Sensitivity without a GPU: forward64 on the weights a WRONG decoder would read, against forward64 on the right ones, through
    the quantities and the function the GPU tests assert with (logits, K rows, V rows by class; the whole position).  Every fault
    must exceed REL_TOL somewhere.  Factors (worst class_err / REL_TOL, over the 3 decode positions; `whole`: what the
    whole-position bar alone sees):
        q6_K scale read as unsigned          2.3e+06 (whole 6.8e+05)    q4_0 low / high halves swapped   2.6e+04 (whole 1.7e+04)
        q6_K |d|                             2.2e+04 (whole 2.0e+04)    q4_0 block scale index + 1       3.1e+04 (whole 1.8e+04)
        q6_K l / 16 dropped                  1.8e+04 (whole 8.1e+03)    q4_0 offset 7                    1.8e+04 (whole 8.6e+03)
        q6_K half n dropped                  1.9e+04 (whole 8.5e+03)    q4_0 nibble as signed 4-bit      1.2e+05 (whole 5.7e+04)
        q6_K qh fields of k = 1, 2 swapped   1.3e+04 (whole 1.1e+04)    q4_0 |d|                         3.0e+04 (whole 2.0e+04)
        q6_K d of super-block 0              1.3e+06 (whole 3.9e+05)    q4_0 subnormal d flushed         1.0e+04 (whole 3.3e+01)
        q6_K offset 31                       1.1e+05 (whole 1.1e+05)    f16  subnormal weight flushed    1.0e+04 (whole 4.4e+00)
        q6_K subnormal d flushed             1.0e+04 (whole 5.5e+03)
    (q6_K on q6k-E1024-q4, q4_0 on tk-small-q4, f16 on tk-small16-f16.  The flushes show what the classes are for: the whole-position
    bar alone sees the f16 one at 4.4 times the bar, a class of its own sees it at 10,000 times.)
    """
    fw, rc, ref = we.model(gguf, name)
    bad = we.forward64(_decode_with(gguf, fw, wtype, fault), we.TOKENS[:3])
    got = {"logits": bad["logits"], "k": bad["k"][0], "v": bad["v"][0]}
    w = _worst(got, {"logits": ref["logits"][:3], "k": ref["k"][0, :3], "v": ref["v"][0, :3]}, rc)
    factor = max(w[q] for q in ASSERTED) / REL_TOL
    print("mutant %-5s %-30s factor %.1e (whole position %.1e)  " % ({14: "q6_K", 2: "q4_0", 1: "f16"}[wtype], fault, factor, w["whole"] / REL_TOL),
          " ".join("%s %.1e" % (q, w[q]) for q in ASSERTED))
    assert factor > 1, w
