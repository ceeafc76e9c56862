"""Is the yardstick of tests/test_tk_qsc_gpu.py sound?  No device: the float64 pass of tests/qsc_ref.py against the C oracle and
against itself in float32, the mirror of the kernel's scale rule on the sequences of the tests (events where they are meant to be,
with room on both sides), the preconditions on every id a GPU test compares, and the drivers themselves on a context made of the
reference and the mirror -- and on one that breaks the contract."""
import numpy as np
import pytest

import qsc_ref as Q
from conftest import REL_TOL, rel_err
from oracle.oracle import Oracle


@pytest.fixture(scope="module")
def built():
    return Q.build()


def run_on_fake(b, driver, *args, fake=Q.Fake):
    m, worst = fake(b), Q.Worst()
    if driver in (Q.g6, Q.g8):
        fakes = [m]
        def fresh():
            fakes.append(fake(b))
            return fakes[-1]
        driver(m, b, worst, fresh)
        return [l for f in fakes for l in f.launches]
    driver(m, b, worst, *args)
    return m.launches


SCENARIOS = {"g1": (Q.g1,), "g2": (Q.g2,), "g3": (Q.g3,), "g4-reset": (Q.g4, "reset"), "g4-prefill": (Q.g4, "prefill"),
             "g4-score": (Q.g4, "score"), "g5": (Q.g5,), "g6": (Q.g6,), "g7": (Q.g7,), "g8": (Q.g8,)}


def test_the_tolerance_is_the_suites():
    assert Q.REL_TOL == REL_TOL


def test_float64_pass_matches_the_c_oracle(built):
    """logits of the ten positions of G3 (three of them spikes) within REL_TOL of oracle/llm_oracle.c on the decoded weights"""
    ref = built.refs["g3"]
    o = Oracle(built.fw32, "omp")
    ol = np.array([o.forward(int(t), pos) for pos, t in enumerate(ref.tokens, 1)])
    err = rel_err(ol, ref.logits)
    print("float64 pass against the C oracle, per position:", err)
    assert np.all(np.isfinite(ref.logits)) and err.max() <= REL_TOL, err


def test_float32_restatement_gives_the_same_maxima(built):
    """the noise floor of invariant R, reference against reference: the same pass in float32 moves no maximum by REL_TOL / 10"""
    ref = built.refs["g3"]
    _, xb, hb = Q.forward_maxima(built.fw32, ref.tokens, np.float32)
    e = max(np.abs(xb / ref.xb - 1).max(), np.abs(hb / ref.hb - 1).max())
    print(f"float32 against float64 maxima: worst relative difference {e:.3g}")
    assert e <= REL_TOL / 10, e
    # and forward_maxima from position 1 is what the incremental greedy loops computed
    lg, xb, hb = Q.forward_maxima(built.fw32, built.refs["g6"].tokens)
    g6 = built.refs["g6"]
    assert rel_err(lg, g6.logits).max() < 1e-12 and np.abs(xb / g6.xb - 1).max() < 1e-12 and np.abs(hb / g6.hb - 1).max() < 1e-12


def test_the_numbers_the_sequences_were_designed_on(built):
    r = built.refs["g3"]
    spikes = [4, 7, 8]
    others = [i for i in range(10) if i not in spikes]
    assert np.all(r.hb[spikes, 1] > 4.0e4) and np.all(r.hb[spikes, 1] < 5.0e4)
    assert r.hb[others, 1].max() < 32 and r.hb[:, [0, 2]].max() < 10 and r.hb[:, [0, 2]].min() > 3
    assert r.xb.max() < 4 and r.xb.min() > 1.5
    assert np.abs(r.logits).max(axis=1).min() > 4 and np.abs(r.logits).max() < 5
    assert int(r.ids[4]) == 2734


def test_mirror_arithmetic():
    for x, want in ((1.0, 1.0), (1.5, 1.0), (2.0, 0.5), (0.75, 2.0), (4.0e-3, 256.0), (4.4e4, 2.0 ** -15)):
        assert Q.tk_pow2_inv(x) == np.float32(want), (x, Q.tk_pow2_inv(x))
    for amax in (1.0, 1.99, 2.0, 5.6, 63.9, 64.0, 4.4e4, 3.0e-3):
        assert 64 <= amax * float(Q.tk_scale_for(amax, 1.0)) < 128
    assert Q.tk_scale_for(0.0, 7.0) == 7 and Q.tk_scale_for(np.inf, 7.0) == 7 and Q.tk_scale_for(np.nan, 7.0) == 7
    assert Q.tk_predict(4.0, 0.0) == 4 and Q.tk_predict(4.0, 9.0) == 6
    val, tag = np.zeros((128, 2), np.float32), np.zeros((128, 2), np.int32)
    val[1], tag[1] = (3.0, 5.0), (6, 7)
    assert Q.tk_hist_amax(val, tag, 1, 3, Q.XB, 7) == 3 and Q.tk_hist_amax(val, tag, 1, 3, Q.XB, 8) == 0
    assert Q.tk_hist_amax(val, tag, 1, 3, Q.HB, 8) == 5 and Q.tk_hist_amax(val, tag, 3, 3, Q.HB, 8) == 0
    # the fit rule on whole vectors: a block's sum / 32 never exceeds its largest element, so the largest element decides
    rng = np.random.default_rng(3)
    for v in (rng.standard_normal(5632), np.full(2048, 3.0), np.r_[np.zeros(31), 4.4e4, rng.standard_normal(64)]):
        assert Q.image_load(v, 4.0) == np.abs(v).max() * 4.0


def test_records_round_trip_through_the_peek_layout():
    mi = Q.Mirror(3)
    mi.launch(1, [2.0, 3.0, 4.0], [5.0, 6.0, 7.0])

    class M:
        def peek(self, which, n):
            assert (which, n) == (8, 8 * 128)
            return mi.rec.raw()
    rec = Q.read_records(M())
    assert np.array_equal(rec.val, mi.rec.val) and np.array_equal(rec.tag, mi.rec.tag)
    assert rec.tag[1, :3].tolist() == [[1, 1]] * 3 and rec.val[1, 1].tolist() == [3.0, 6.0] and not rec.tag[0].any()


@pytest.mark.parametrize("name", SCENARIOS)
def test_events_fall_where_they_are_meant_to_with_room_on_both_sides(name, built):
    """Every launch of the scenario, with the history it actually has (the driver on Fake): at an event the vector is at least 4
    times what fits (65504), every other image written is at most a quarter of what the kernel lets pass (60000).  The drivers
    assert the positions of the events themselves."""
    launches = run_on_fake(built, *SCENARIOS[name])
    assert launches
    hi = [ld / Q.F16_MAX for w in launches for (l, k, ld) in w.loads if (l, k) == w.event]
    lo = [ld / Q.TK_FIT for w in launches for (l, k, ld) in w.loads if (l, k) != w.event]
    print(name, "events", [(w.pos, w.event) for w in launches if w.event], "least event", min(hi, default=None), "largest other", max(lo))
    assert all(h >= 4 for h in hi) and max(lo) <= 0.25, (hi, max(lo))
    for w in launches:      # a spike is an event of layer 1's hb image and of nothing else
        assert w.event in (None, (1, Q.HB))


def test_a_normal_token_behind_a_spike_sits_at_the_edge_of_the_full_precision_band(built):
    """G2's position 6 is the precision of an image predicted too high: layer 1's hb is predicted sqrt(now * hist) with now = layer
    0's hb in [3.5, 9.2] and hist = the spike's 4.3e4 .. 4.6e4, i.e. 388 .. 650, and scaled so that the prediction lies in [64, 128);
    the vector's largest element is 5 .. 30, so it is written at 0.49 .. 9.9: 2^3 .. 2^7 below the target"""
    w = Q.expected(built, "g3", 7)[5]
    ld = [x for (l, k, x) in w.loads if (l, k) == (1, Q.HB)][0]
    assert 0.49 <= ld <= 9.9, ld


def test_compared_ids_have_a_margin(built):
    """every position whose greedy id a GPU test compares: top-1 margin above 4 * REL_TOL * max |logit| in the reference"""
    g6, g7 = built.refs["g6"], built.refs["g7"]
    assert g6.margin_ok()[4:11].all(), g6.margin_ok()
    assert g7.margin_ok()[len(Q.G7_HEAD):].all(), g7.margin_ok()
    assert len(g7.tokens) == len(Q.G7_HEAD) + Q.G7_ROUNDS * (1 + Q.G7_CLEAN) <= built.fw.shape.seq_len


def test_g6_construction(built):
    g6 = built.refs["g6"]
    assert g6.tokens[:5].tolist() == Q.G6_HEAD + [Q.SPIKE]
    assert np.array_equal(g6.tokens[5:], g6.ids[4:11])                       # a greedy chain from position 5 on
    assert int(g6.tokens[6]) == built.spike2 != Q.SPIKE
    assert built.spike2 not in g6.tokens[:6] and list(g6.tokens).count(built.spike2) == 1
    assert built.fw.token_embedding_table[built.spike2 - 1, 5] == np.float32(Q.SPIKE_X)
    for name in ("g1", "g3", "g4b", "g5", "g7"):
        assert built.spike2 not in built.refs[name].tokens
    s = built.fw.shape
    assert np.array_equal(built.fw.w13[1, 0], Q.spike_row(s.emb_dim)) and np.array_equal(built.fw.w13[1, s.hidden_dim], Q.spike_row(s.emb_dim))
    row = built.fw32.w13[1, 0]
    assert row[5] == np.float32(np.float16(0.9)) * np.float32(7) and np.count_nonzero(row) == 1


def test_g8_can_tell_a_kernel_that_ignores_the_tags(built):
    """The precondition of G8: in the state G3 leaves behind position 8, a kernel that took layer 2's record of position 6 for
    history would write position 9's layer-2 hb image at another power of two (2^6 apart: the lo pieces of the image round
    elsewhere, the logits differ in their last bits); with position 8 fed twice there is nothing for it to take."""
    r, L = built.refs["g3"], built.fw.shape.n_layers

    def at9(tagless, twice):
        mi = Q.Mirror(L, tagless)
        for p in list(range(1, 9)) + ([8] if twice else []):
            mi.launch(p, r.xb[p - 1], r.hb[p - 1])
        return {(l, k): ld for (l, k, ld) in mi.launch(9, r.xb[8], r.hb[8]).loads}
    good, bad = at9(False, False), at9(True, False)
    assert good == at9(False, True) == at9(True, True)
    assert {k for k in good if good[k] != bad[k]} == {(2, Q.HB)} and bad[(2, Q.HB)] / good[(2, Q.HB)] >= 32


class StaleFake(Q.Fake):
    """a context that keeps what an earlier sequence left when a position is fed again (no drop in front of a rewind)"""
    def __init__(self, b):
        super().__init__(b)
        self.mirror.keep_only = lambda pos: None


class DebrisFake(Q.Fake):
    """a context whose pipelined calls leave, behind an event, whole records of the positions queued behind it"""
    def decode_greedy(self, token, pos0, n):
        ids = super().decode_greedy(token, pos0, n)
        if n > 1 and any(l.event for l in self.launches[-n:]):
            p = pos0 + n - 1
            self.mirror.rec.val[p & 1, :3] = 1.0
            self.mirror.rec.tag[p & 1, :3] = p
        return ids


def test_the_drivers_notice_a_broken_contract(built):
    with pytest.raises(AssertionError):
        run_on_fake(built, Q.g5, fake=StaleFake)
    with pytest.raises(AssertionError):
        run_on_fake(built, Q.g6, fake=DebrisFake)
