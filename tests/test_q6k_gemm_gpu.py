"""The q6_K classifier as a GEMM (prefill.h pf_gemm_h_kernel, WT_Q6_K): llmk_score's batches and the batched decode read a stock
q4_0 file's output.weight once per pass.  Crafted rows (tests/weight_edge.py: one class of q6_K encodings per row, nine classes,
so every row slot of every strip meets every class), the float64 reference on the decoded weights, conftest.REL_TOL on the whole
position and WITHIN every class of rows (weight_edge.Report) -- the bars test_weight_edge_gpu.py holds the per-row classifier to.

Shapes (one layer, seq_len 136).  The classifier runs in sc_plan's row chunks, and a chunk is as large as the partial-tile workspace
that the LAYERS' matrices size (pf_setup_inner) admits; each chunk has pf_plan's plan for its own rows.  What is written here is what
sc_batch launched on an MI355X (256 CUs), printed chunk by chunk by the debug build under LLMK_PF_SHOW_PLAN=1, the same at 128 and at
17 positions: (R, U, nk, grid) = rows of the chunk, units per block, 64-column steps per strip, blocks.
  E256-f16    E 256, H 512, V 1000, f16 matrices: one super-block = four steps (both halves, both nibble positions, all four bit
              pairs of the high-bit plane); V is a multiple of 4 but not of 64: a ragged last strip, one row group per wave.  One
              chunk, (1000, 2, 4, 32).
  E1024-q4    E 1024, H 2048, V 1024, q4_0 matrices: four super-blocks (the super-block index of the scales and of d).  One chunk,
              (1024, 2, 16, 128), one row group per wave.
  E512-q4     E 512, H 5120, V 8260, q4_0 matrices.  The issue's E 512 / V 640 gives (640, 2, 8, 40): U divides nk, no block crosses
              a strip.  With nk = 8 and 256 CUs the first U that is not a multiple of 4 and does not divide nk is 6, which takes more
              than 1024 units = 8192 rows IN ONE CHUNK; 8260 = 129 strips of 64 rows + 4 rows is the nearest vocabulary, and
              H = 5120 the nearest hidden size (in steps of 1024) whose workspace, 3 x 128 x 2H floats, admits that chunk's
              3 x 128 x 8260 (at H = 1024 the classifier runs as three chunks of (2816 | 2628, 2, 8, 176 | 168): no block crosses
              a strip).  One chunk, (8260, 6, 8, 174): blocks start on steps 0, 6, 4, 2 of a strip (6 and 2: the middle of a
              super-block) and every second block crosses a strip boundary.
              test_the_plans_this_file_states_are_the_plans_that_run holds these figures to the code.
  tinyllama   weight_edge's tinyllama-q4-q6k (E 2048, H 5632, V 32000): TWO row groups per wave, in three chunks of 10752, 10752
              and 10496 rows, (10752, 12, 32, 224) twice and (10496, 12, 32, 219): blocks start on steps 0, 12, 24, 4, 16, 28, 8, 20
              of a strip (whole super-blocks) and cross strip boundaries; at 128 positions this is the largest instantiation (eight
              position groups x two row groups).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import score_ref
import weight_edge as we
from conftest import REL_TOL, ROOT, rel_err
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf

pytestmark = pytest.mark.gpu

GEMM_MIN_ROWS = 3      # csrc/llmk.hip SC_Q6K_GEMM_MIN_ROWS (test_q6k_gemm_cpu.py holds the two together)
SEQ_LEN = 136
SHAPES = {"E256-f16": ((256, 512, 4, 2, 1000), 1), "E1024-q4": ((1024, 2048, 8, 2, 1024), 2), "E512-q4": ((512, 5120, 4, 4, 8260), 2)}
SEED = 20261101
NS = [1, 16, 17, 128, 129]
_models = {}


def tokens(V, n, seed=3):
    return [2] + (np.random.default_rng(seed).integers(3, V, n - 1) + 1).tolist()


def build(name):
    """(FusedWeights, classes of the classifier rows) -- the same bytes in every process"""
    (E, H, nh, nkv, V), mt = SHAPES[name]
    fw, classes = we.craft_model(gguf, gguf.LlamaShape(E, H, 1, nh, nkv, V, SEQ_LEN), mt, 14, SEED)
    return fw, classes["wcls"]


def model(name):
    """(fw, classes, the 129 tokens, forward64's logits of them): once per process, read only"""
    if name not in _models:
        fw, cls = build(name)
        seq = tokens(fw.shape.vocab_size, 129)
        _models[name] = (fw, cls, seq, we.forward64(we.decoded(gguf, fw), seq)["logits"])
    return _models[name]


def check_score(label, lp, am, lg, ref, tg, cls):
    """test_score_gpu.py's three bounds (logits within REL_TOL per position, log-probs within 2 REL_TOL max|logit| of score_ref on
    the reference's logits, argmax where the reference's margin is safe) and the per-class bars"""
    r = we.Report(label)
    for i in range(len(ref)):
        r.add("logits", i + 1, lg[i], ref[i], cls, we.Q6K_CLASSES)
        r.whole(i + 1, lg[i], ref[i])
    r.finish()
    rlp, ram = score_ref.score(ref, tg)
    scale = np.abs(ref).max(axis=1)
    dlp = np.abs(lp.astype(np.float64) - rlp)
    print(f"{label}: max |logprob diff| / max|logit| {np.max(dlp / scale):.3e}")
    assert (dlp <= 2 * REL_TOL * scale).all(), (int(np.argmax(dlp / scale)), dlp.max())
    top2 = np.sort(ref, axis=1)[:, -2:]
    safe = (top2[:, 1] - top2[:, 0]) > 4 * REL_TOL * scale
    assert np.array_equal(am[safe], ram[safe])


# ---- 1: llmk_score ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_score_on_the_q6k_gemm_matches_forward64_in_every_class(name, n):
    fw, cls, seq, ref = model(name)
    tg = score_ref.default_targets(seq[:n])
    m = llmk.Llmk(fw)
    for rows in sorted({min(n, 128), n - 128 if n > 128 else 128, GEMM_MIN_ROWS, max(GEMM_MIN_ROWS - 1, 1)}):      # (the call's batch sizes)
        assert m.cls_form(rows) == (llmk.CLS_GEMM if rows >= GEMM_MIN_ROWS else llmk.CLS_ROWS), rows
    lp, am, lg = m.score(seq[:n], 1, want_argmax=True, want_logits=True)
    check_score("q6k gemm score %s n=%d" % (name, n), lp, am, lg, ref[:n], tg, cls)
    m.reset()
    lp2, am2, lg2 = m.score(seq[:n], 1, want_argmax=True, want_logits=True)
    assert np.array_equal(lp.view(np.uint32), lp2.view(np.uint32)) and np.array_equal(am, am2)
    assert np.array_equal(lg.view(np.uint32), lg2.view(np.uint32))
    assert m.cls_form(128) == llmk.CLS_GEMM          # no range flag moved the context
    m.close()


def test_score_with_two_row_groups_per_wave_at_a_full_batch():
    """weight_edge's tinyllama-q4-q6k: 250 strips of 128 rows; 128 positions and 17 (eight and two position groups)"""
    import dataclasses
    fw, rc, _ = we.model(gguf, "tinyllama-q4-q6k")
    fw = dataclasses.replace(fw, shape=dataclasses.replace(fw.shape, seq_len=128))      # (weight_edge's has 64)
    seq = tokens(fw.shape.vocab_size, 128, seed=8)
    ref = we.forward64(we.decoded(gguf, fw), seq)["logits"]
    m = llmk.Llmk(fw)
    assert m.cls_form(128) == llmk.CLS_GEMM
    for n in (128, 17):
        m.reset()
        tg = score_ref.default_targets(seq[:n])
        lp, am, lg = m.score(seq[:n], 1, want_argmax=True, want_logits=True)
        check_score("q6k gemm score tinyllama n=%d" % n, lp, am, lg, ref[:n], tg, rc["logits"])
    m.close()


# ---- 2: batched decode --------------------------------------------------------------------------------------------------------------
_rows = {}


def ragged_rows():
    """33 sequences of 1..7 tokens on E1024-q4 and forward64 of each alone"""
    if not _rows:
        fw, cls, _, _ = model("E1024-q4")
        d = we.decoded(gguf, fw)
        lens = [1 + (3 * j) % 7 for j in range(33)]
        seqs = [tokens(fw.shape.vocab_size, n, seed=100 + j) for j, n in enumerate(lens)]
        _rows.update(seqs=seqs, ref=[we.forward64(d, s)["logits"] for s in seqs])
    return _rows["seqs"], _rows["ref"]


@pytest.mark.parametrize("R", [1, 5, 16, 33])
def test_batch_forward_rows_at_ragged_positions_match_forward64_on_each_sequence_alone(R):
    """slot j's sequence starts so that every slot reaches its LAST position in the last pass: that pass has R rows at positions
    1..7, the passes before it fewer; every row of every pass is checked"""
    fw, cls, _, _ = model("E1024-q4")
    seqs, ref = ragged_rows()
    seqs, ref = seqs[:R], ref[:R]
    last = max(len(s) for s in seqs)
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, R)
    r = we.Report("q6k gemm batch forward R=%d" % R)
    for t in range(last):
        slots = [j for j in reversed(range(R)) if t >= last - len(seqs[j])]
        pos = [t - (last - len(seqs[j])) + 1 for j in slots]
        want = llmk.CLS_GEMM if len(slots) >= GEMM_MIN_ROWS else llmk.CLS_ROWS
        assert m.cls_form(len(slots)) == want
        lg, am = b.forward(slots, [seqs[j][p - 1] for j, p in zip(slots, pos)], pos)
        assert np.array_equal(am, np.argmax(lg, axis=1) + 1)
        for i, (j, p) in enumerate(zip(slots, pos)):
            r.add("logits", p, lg[i], ref[j][p - 1], cls, we.Q6K_CLASSES)
            r.whole(p, lg[i], ref[j][p - 1])
    assert len(slots) == R
    b.close()
    m.close()
    r.finish()


def test_batch_decode_picks_what_sample_logits_picks_from_the_same_logits():
    fw, cls, _, _ = model("E1024-q4")
    sps = [dict(temperature=1.0, seed=11, top_k=1), dict(temperature=0.9, seed=12), dict(temperature=0.8, seed=13, top_k=5),
           dict(temperature=1.1, seed=14, top_p=0.9, min_p=0.05), dict(temperature=0.7, seed=15)]
    slots, toks, pos0, steps = [4, 2, 0, 1, 3], [2, 50, 7, 60, 9], [1] * 5, 4
    m = llmk.Llmk(fw)
    b = llmk.Batch(m, 5)
    ids = b.decode(slots, toks, pos0, steps, [llmk.sampler(**sp) for sp in sps])
    b.close()
    b = llmk.Batch(m, 5)
    for st in range(steps):
        lg = b.forward(slots, toks if st == 0 else ids[:, st - 1].tolist(), [p + st for p in pos0], want_argmax=False)
        for i, sp in enumerate(sps):
            want = m.sample_logits(lg[i], pos0[i] + st, **sp)[0]
            assert ids[i, st] == want, (i, st, ids[i, st], want)
    b.close()
    b = llmk.Batch(m, 5)
    greedy = b.decode(slots, toks, pos0, steps)
    b.close()
    b = llmk.Batch(m, 5)
    for st in range(steps):
        am = b.forward(slots, toks if st == 0 else greedy[:, st - 1].tolist(), [p + st for p in pos0], want_logits=False)
        assert np.array_equal(greedy[:, st], am)
    b.close()
    m.close()


# ---- 3, 4: the other form, in processes of their own ------------------------------------------------------------------------------------
CHILD = r'''
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import llm_f90_amd
from llm_f90_amd import llmk
import test_q6k_gemm_gpu as t
out, arrays = {}, {}
for case in sys.argv[3].split(","):
    name, n, edit = case.split(":")
    fw, cls = t.build(name)
    if edit != "plain":
        t.plant(fw, edit)
    seq = t.tokens(fw.shape.vocab_size, 129)[:int(n)]
    m = llmk.Llmk(fw)
    out[case + ":before"] = m.cls_form(128)
    lp, am, lg = m.score(seq, 1, want_argmax=True, want_logits=True)
    out[case + ":after"] = m.cls_form(128)
    arrays[case + ":lp"], arrays[case + ":am"], arrays[case + ":lg"] = lp, am, lg
    m.close()
np.savez(sys.argv[2], **arrays)
print(json.dumps(out))
'''
BIG_ROW, BIG_SB = 515, 2


def plant(fw, what):
    """super-block BIG_SB of classifier row BIG_ROW: d = f16 4096 ("big") or an f16 NaN ("nan"), every scale 127, every q 63"""
    blk = np.empty(we.Q6K_BYTES, np.uint8)
    blk[0:192] = 0xFF
    blk[192:208] = 127
    blk[208], blk[209] = (0x00, 0x6C) if what == "big" else (0x00, 0x7E)
    fw.wcls = fw.wcls.copy()
    fw.wcls[BIG_ROW, BIG_SB * we.Q6K_BYTES:(BIG_SB + 1) * we.Q6K_BYTES] = blk


def run_child(tmp_path, tag, cases, env):
    path = str(tmp_path / (tag + ".npz"))
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, path, ",".join(cases)], env=dict(os.environ, **env), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(path)
    return json.loads(r.stdout.strip().splitlines()[-1]), {k: z[k] for k in z.files}, r.stderr


def test_both_forms_agree(tmp_path):
    """the same calls on a context created under LLMK_PF_F32_MFMA=1: the per-row form, within REL_TOL of the GEMM form's logits"""
    cases = ["%s:129:plain" % name for name in SHAPES]
    out, rows, _ = run_child(tmp_path, "rows", cases, {"LLMK_PF_F32_MFMA": "1"})
    for name, case in zip(SHAPES, cases):
        assert out[case + ":before"] == llmk.CLS_ROWS and out[case + ":after"] == llmk.CLS_ROWS
        fw, cls, seq, ref = model(name)
        m = llmk.Llmk(fw)
        assert m.cls_form(128) == llmk.CLS_GEMM
        lg = m.score(seq, 1, want_logprob=False, want_logits=True)
        m.close()
        e = rel_err(rows[case + ":lg"], lg)
        print(f"{name}: per-row form against the GEMM form, max rel err {e.max():.3e}")
        assert e.max() <= REL_TOL, (name, int(np.argmax(e)), e.max())


PLANS = {"E256-f16": "rows 1000 nr 1 U 2 nk 4 grid 32", "E1024-q4": "rows 1024 nr 1 U 2 nk 16 grid 128",
         "E512-q4": "rows 8260 nr 1 U 6 nk 8 grid 174"}


def test_the_plans_this_file_states_are_the_plans_that_run(tmp_path):
    """the debug build (same ABI) says on stderr what sc_batch launches for each classifier chunk: the E512-q4 shape is in this file
    for its plan -- U = 6 on nk = 8 -- and a change of pf_plan, of the workspace or of the shape that loses it must not pass
    silently.  The figures are those of 256 compute units"""
    cases = ["%s:17:plain" % name for name in SHAPES]
    out, got, err = run_child(tmp_path, "plan", cases, {"LLMK_LIB": os.path.join(ROOT, "llm.f90_amd", "csrc", "libllmk_debug.so"),
                                                        "LLMK_PF_SHOW_PLAN": "1"})
    lines = [ln for ln in err.splitlines() if ln.startswith("llmk: classifier chunk")]
    print("\n".join(lines))
    want = ["llmk: classifier chunk 1 of 1: T 17 " + PLANS[name] for name in SHAPES]
    assert lines == want, ("the plans in this file's docstring are an MI355X's (256 compute units)", lines, want)
    for name, case in zip(SHAPES, cases):              # ... and the debug build computes what the release build does
        fw, cls, seq, ref = model(name)
        assert rel_err(got[case + ":lg"], ref[:17]).max() <= REL_TOL


def test_a_weight_beyond_the_f16_range_sends_the_call_through_the_redo(tmp_path):
    """d = 4096, scale 127, q = 63: a weight of 1.6e7 in one super-block of one row raises bit 0 of the range flag; the call
    returns the redone values and the context's classifier runs per row from then on.  The twin with a NaN d: only that row's
    logit is NaN; argmax and log-probs are the per-row form's (a context that started on the f32 instruction), bit for bit"""
    n = 17
    cases = ["E1024-q4:%d:big" % n, "E1024-q4:%d:nan" % n]
    out, got, err = run_child(tmp_path, "flag", cases, {})
    assert "llmk_score met an activation beyond the f16 range" in err, err[-2000:]
    rout, rows, rerr = run_child(tmp_path, "flag_rows", cases, {"LLMK_PF_F32_MFMA": "1"})
    assert "llmk_score met" not in rerr, rerr[-2000:]
    for case in cases:
        assert out[case + ":before"] == llmk.CLS_GEMM and out[case + ":after"] == llmk.CLS_ROWS, (case, out)
        assert rout[case + ":before"] == llmk.CLS_ROWS
    fw, cls = build("E1024-q4")
    plant(fw, "big")
    seq = tokens(fw.shape.vocab_size, 129)[:n]
    ref = we.forward64(we.decoded(gguf, fw), seq)["logits"]
    lg = got[cases[0] + ":lg"].astype(np.float64)
    ordinary = np.arange(fw.shape.vocab_size) != BIG_ROW
    big = np.abs(lg[:, BIG_ROW] - ref[:, BIG_ROW]) / np.abs(ref[:, BIG_ROW])
    rest = np.max(np.abs(lg[:, ordinary] - ref[:, ordinary]), axis=1) / np.max(np.abs(ref[:, ordinary]), axis=1)
    print(f"big row: max rel err {big.max():.3e} (|ref| {np.abs(ref[:, BIG_ROW]).min():.3e} ..); ordinary rows {rest.max():.3e}")
    assert big.max() <= 1e-4 and rest.max() <= REL_TOL
    lg = got[cases[1] + ":lg"]
    assert np.isnan(lg[:, BIG_ROW]).all() and np.isfinite(lg[:, ordinary]).all()
    for k in ("lp", "am"):
        assert np.array_equal(got[cases[1] + ":" + k], rows[cases[1] + ":" + k], equal_nan=True), k


# ---- 5, 6 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_time_kernel_12_times_the_q6k_gemm(name):
    fw, _, _, _ = model(name)
    (E, _, _, _, V), _ = SHAPES[name]
    m = llmk.Llmk(fw)
    ms, b = m.time_kernel(12, 5)
    assert ms > 0 and b == V * ((E // 256 * 210 + 15) // 16 * 16)
    m.close()


def test_a_vocabulary_off_the_four_row_vectors_stays_on_the_per_row_form():
    fw, rc, ref = we.model(gguf, "q6k-E256-f16")          # V = 1002
    m = llmk.Llmk(fw)
    assert m.cls_form(5) == llmk.CLS_ROWS and m.cls_form(128) == llmk.CLS_ROWS
    with pytest.raises(llmk.LlmkError):
        m.time_kernel(12, 2)
    tg = score_ref.default_targets(we.TOKENS)
    lp, am, lg = m.score(we.TOKENS, 1, want_argmax=True, want_logits=True)
    check_score("q6k per-row score V=1002", lp, am, lg, ref["logits"], tg, rc["logits"])
    m.close()
