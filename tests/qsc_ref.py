"""TEST INFRASTRUCTURE -- the q4_0 persistent kernel's per-layer scale records (csrc/token_kernel.h tk_qsc) as a tested contract.

Each launch of the q4_0 token kernel leaves, per layer, the largest |element| of its xb (attention output) and hb (SwiGLU output)
vectors, tagged with its position, in the buffer of its position's parity; the next position scales its f16 hi | lo images from
them.  This module holds
  * Pass / forward_maxima: the float64 forward pass of tests/ref_pass.py, to which they add those maxima, collected through its tap;
  * a mirror in plain Python of the kernel's scale rule (tk_pow2_inv .. tk_hist_amax, the fit test of tk_coop_part) and of the host's
    part of the protocol (who clears the records, what a redo leaves): Mirror says where a fed sequence raises a range event and
    which records each launch leaves;
  * the model and the sequences of the tests, and the drivers g1 .. g7 that tests/test_tk_qsc_gpu.py runs on the device and
    tests/test_tk_qsc_cpu.py runs on Fake, a context made of the reference and the mirror (is the yardstick itself sound?).
DESIGN.md section 3d2 states the contract in words."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from llm_f90_amd.tools import gguf
from ref_pass import RefPass

REL_TOL = 1e-4          # conftest.REL_TOL (a test asserts that they are the same number)

# ------------------------------------------------------------------------------------------------
# float64 reference with the maxima
# ------------------------------------------------------------------------------------------------
class Pass(RefPass):
    """ref_pass.RefPass whose feed also returns the maxima the kernel records"""

    def feed(self, tokens):
        """tokens (1-based ids) at the next len(tokens) positions.  Returns (logits [m][V], xb [m][L], hb [m][L]): per position and
        layer the largest |element| of the attention output (all heads, in front of wo) and of silu(gate) * up."""
        m = np.size(tokens)
        amax = {"xb": np.empty((m, self.s.n_layers)), "hb": np.empty((m, self.s.n_layers))}

        def tap(l, name, a):
            if name in amax:
                amax[name][:, l] = np.abs(a).max(axis=1)
        return super().feed(tokens, tap=tap), amax["xb"], amax["hb"]


def forward_maxima(fw_f32, tokens, dtype=np.float64):
    """the whole sequence from position 1: (logits [n][V], xb [n][L], hb [n][L]) -- see Pass.feed"""
    return Pass(fw_f32, dtype).feed(tokens)


# ------------------------------------------------------------------------------------------------
# mirror of the kernel's scale rule (csrc/token_kernel.h:532-605) in f32
# ------------------------------------------------------------------------------------------------
TK_QSC_LMAX = 128                       # :556
TK_IMG_TARGET = np.float32(64.0)        # :557
TK_FIT = 60000.0                        # :663  tk_coop_part: an image whose largest |scaled element| is not below this raises 0x4000
F16_MAX = 65504.0                       # the end of the format the hi pieces are written in
Q16_SUM_DIV = 32.0                      # q4_units.h:53  a block's sum is held as sum / 32
XB, HB = 0, 1                           # field of a record: .x / .z and .y / .w
f32 = np.float32


def tk_pow2_inv(x) -> np.float32:
    """2^-floor(log2 x), by the biased exponent of x: x times it lies in [1, 2) (:535)"""
    e = int(f32(x).view(np.uint32) >> np.uint32(23)) & 0xff
    return np.uint32(min(max(254 - e, 1), 254) << 23).view(np.float32)


def tk_scale_for(amax, fallback) -> np.float32:
    """the scale that puts a vector whose largest |element| is amax into [64, 128) (:563)"""
    amax = f32(amax)
    return tk_pow2_inv(amax * f32(1.0 / 64.0)) if (amax > 0 and amax < f32(3.0e38)) else f32(fallback)


def tk_predict(now, hist) -> np.float32:
    """this token's vector of the layer before and the same layer's of the position before: their geometric mean (:587)"""
    return np.sqrt(f32(now) * f32(hist)) if hist > 0 else f32(now)


def tk_hist_amax(val, tag, l: int, L: int, kind: int, pos: int) -> np.float32:
    """what layer l's record in the buffer (val [128][2], tag [128][2]) says of the position before pos; 0: nothing (:599)"""
    if l >= L or l >= TK_QSC_LMAX:
        return f32(0)
    v = f32(val[l, kind])
    return v if (int(tag[l, kind]) == pos - 1 and v > 0 and v < f32(3.0e38)) else f32(0)


def image_load(vec, scale) -> float:
    """The fit rule of an xb / hb image, on a whole vector: what has to stay below TK_FIT is the largest |scaled element| (the hi
    piece of an element under a high nibble is written at 1/16 of it, q16_pair_scale) -- and the largest |block sum| / 32, which is
    never above the block's largest |element| (q16_put_sum, Q16_SUM_DIV), so the elements decide.  Returns the larger of the two."""
    y = np.asarray(vec, np.float64) * float(scale)
    sums = np.abs(y[:len(y) // 32 * 32].reshape(-1, 32).sum(axis=1)) / Q16_SUM_DIV
    return float(max(np.abs(y).max(), sums.max() if len(sums) else 0.0))


@dataclasses.dataclass
class Launch:
    """what one launch of the token kernel does at position pos"""
    pos: int
    event: tuple            # (layer, kind) of the vector that did not fit, or None
    written: list           # the (layer, kind) fields that carry tag pos afterwards, in the order they are written
    loads: list             # (layer, kind, largest |scaled element|) of every image written, the event's included


class Records:
    """[2 buffers][128 layers] x {|xb|, |hb|, pos, pos}: val[b][l][kind] f32, tag[b][l][kind] int32"""

    def __init__(self, val=None, tag=None):
        self.val = np.zeros((2, TK_QSC_LMAX, 2), np.float32) if val is None else val
        self.tag = np.zeros((2, TK_QSC_LMAX, 2), np.int32) if tag is None else tag

    def copy(self):
        return Records(self.val.copy(), self.tag.copy())

    def raw(self) -> np.ndarray:
        """as llmk_peek(8) returns them: 8 * 128 floats"""
        out = np.empty((2, TK_QSC_LMAX, 4), np.float32)
        out[:, :, :2] = self.val
        out[:, :, 2:] = self.tag.view(np.float32)
        return out.reshape(-1)


def read_records(m) -> Records:
    r = np.asarray(m.peek(8, 8 * TK_QSC_LMAX), np.float32).reshape(2, TK_QSC_LMAX, 4)
    return Records(r[:, :, :2].copy(), r[:, :, 2:].copy().view(np.int32))


class Mirror:
    """The records of one context: the kernel's rule per launch, and the host's part --
      * llmk_reset, llmk_prefill and llmk_score zero both buffers (clear);
      * a launch that does not continue the position before it (a rewind, a jump) first drops every field whose tag is not pos - 1;
      * the redo of a position on the multi-kernel path writes nothing: what the launch with the event left stays."""

    def __init__(self, L: int, tagless: bool = False):
        """tagless: a kernel that takes whatever a record holds for history, whichever position wrote it -- what G8 must notice"""
        self.L, self.rec, self.last, self.tagless = L, Records(), 0, tagless

    def clear(self):
        self.rec, self.last = Records(), 0

    def keep_only(self, pos: int):
        drop = self.rec.tag != pos
        self.rec.val[drop] = 0
        self.rec.tag[drop] = 0

    def launch(self, pos: int, xb, hb) -> Launch:
        """xb, hb [L]: the largest |element| of this position's vectors"""
        if pos != self.last + 1:
            self.keep_only(pos - 1)
        self.last = pos
        hv, ht = self.rec.val[(pos - 1) & 1].copy(), self.rec.tag[(pos - 1) & 1].copy()      # (read at entry: token_kernel.h:2053)
        ov, ot = self.rec.val[pos & 1], self.rec.tag[pos & 1]
        # layer 0: its own record of the position before, else the largest element assumed in [1, 2) (:2058-2062)
        sc = [tk_scale_for(hv[0, k], TK_IMG_TARGET) if int(ht[0, k]) == pos - 1 else TK_IMG_TARGET for k in (XB, HB)]
        out = Launch(pos, None, [], [])
        for l in range(self.L):
            for kind, amax in ((XB, xb[l]), (HB, hb[l])):
                am = f32(amax)
                load = float(am) * float(sc[kind])
                out.loads.append((l, kind, load))
                if l < TK_QSC_LMAX:         # (the vector that raises the event is recorded too: :1655)
                    ov[l, kind], ot[l, kind] = am, pos
                    out.written.append((l, kind))
                if not load < TK_FIT:
                    out.event = (l, kind)
                    return out
                sc[kind] = tk_scale_for(tk_predict(am, tk_hist_amax(hv, np.full_like(ht, pos - 1) if self.tagless else ht, l + 1, self.L, kind, pos)), sc[kind])
        return out


# ------------------------------------------------------------------------------------------------
# the model and the sequences
# ------------------------------------------------------------------------------------------------
SPIKE = 777                                     # 1-based id: embedding row 776 has SPIKE_X in column 5
SPIKE_X, SPIKE_W = 60.0, 6.3                    # layer 1's first gate and up rows read column 5 alone with weight 6.3 (q4_0: 0.9 * 7)
CLEAN = [5, 9, 12, 31, 44, 8, 60, 23]           # G1
G3 = [5, 9, 12, 31, 777, 8, 44, 777, 777, 60]   # G2 is its first seven positions
SEQ_B = [7, 19, 3, 101, 250, 66, 90]            # G4
G5 = CLEAN[:6] + [SPIKE, 8]                     # seven positions of CLEAN, position 7 again with the spike, then position 8
G6_HEAD = CLEAN[:4]                             # then decode_greedy(777, 5, 3), decode_greedy(id, 8, 4), forward(id, 12)
# G7: the head through forward(), then five rounds of decode_greedy(777, p, 1), decode_greedy(id, p + 1, 5).  (Head [5] makes one
# spike follow a pick whose layer-1 hb is 93: that event is 3.0 times the range where test_tk_qsc_cpu.py asks for 4.)
G7_HEAD = [9]
G7_ROUNDS, G7_CLEAN = 5, 5


@dataclasses.dataclass
class Ref:
    """a fed sequence and what the float64 pass says of it (shared by the tests: read-only)"""
    tokens: np.ndarray      # [n] 1-based ids
    logits: np.ndarray      # [n][V]
    xb: np.ndarray          # [n][L]
    hb: np.ndarray          # [n][L]

    @property
    def ids(self):
        """the greedy pick behind every position, 1-based"""
        return np.argmax(self.logits, axis=1) + 1

    def margin_ok(self):
        """positions whose top-1 margin is above 4 * REL_TOL * max |logit|"""
        top2 = np.sort(self.logits, axis=1)[:, -2:]
        return (top2[:, 1] - top2[:, 0]) > 4 * REL_TOL * np.abs(self.logits).max(axis=1)


def _ref(tokens, parts) -> Ref:
    r = Ref(np.asarray(tokens, np.int32), *(np.concatenate([q[i] for q in parts]) for i in range(3)))
    for a in (r.tokens, r.logits, r.xb, r.hb):
        a.setflags(write=False)
    return r


def _greedy(p: Pass, tokens, token: int, n: int, parts):
    """n more positions, the first fed `token`, each further one the pick of the one before; appends to tokens / parts"""
    for _ in range(n):
        tokens.append(int(token))
        parts.append(p.feed([token]))
        token = int(np.argmax(parts[-1][0][0])) + 1
    return token


@dataclasses.dataclass
class Built:
    fw: object              # the q4_0 weights the device gets
    fw32: object            # the same, host-decoded
    spike2: int             # G6's second spike token (1-based)
    refs: dict              # name -> Ref


def spike_row(E: int) -> np.ndarray:
    """the q4_0 row that reads column 5 alone with weight 6.3: block 0 has d = 0.9 and nibble 0xF at element 5, every other nibble
    is 8 (= 0) and every other scale 0"""
    row = np.zeros((E // 32, 18), np.uint8)
    row[:, 2:] = 0x88
    row[0, 0:2] = np.array([0.9], np.float16).view(np.uint8)
    row[0, 2 + 5] = 0x8F
    return row.reshape(-1)


@functools.lru_cache(maxsize=None)
def build() -> Built:
    """TkTinyLlamaQ4's columns with 3 layers; the direction event of test_llama2_7b_q4_0_one_position_beyond_f16... in LAYER 1, so
    that there are layers in front of and behind it"""
    s = gguf.LlamaShape(2048, 5632, 3, 32, 4, 32000, 64)
    fw = gguf.synth_fused(s, 7, gguf.GGML_Q4_0)
    emb = fw.token_embedding_table = fw.token_embedding_table.copy()
    emb[SPIKE - 1, 5] = np.float32(SPIKE_X)
    fw.w13 = fw.w13.copy()
    fw.w13[1, 0] = fw.w13[1, s.hidden_dim] = spike_row(s.emb_dim)
    fw32 = fw.as_f32()
    assert fw32.token_embedding_table is emb
    base = Pass(fw32)
    refs = {}
    for name, toks in (("g1", CLEAN), ("g4b", SEQ_B), ("g5", G5)):
        refs[name] = _ref(toks, [base.fork(0).feed(toks)])
    # G6: the second spike token is the greedy pick two positions behind 777 -- found on the model as it is, then given the spike's
    # embedding column; it is fed nowhere in front of that position, so nothing the loop has computed changes
    p, toks, parts = base.fork(0), list(G6_HEAD), []
    parts.append(p.feed(G6_HEAD))
    nxt = _greedy(p, toks, SPIKE, 2, parts)             # positions 5 and 6
    spike2 = nxt
    assert spike2 != SPIKE and spike2 not in toks and spike2 not in CLEAN + G3 + SEQ_B + G5
    emb[spike2 - 1, 5] = np.float32(SPIKE_X)
    nxt = _greedy(p, toks, spike2, 1 + 4, parts)        # position 7, then 8 .. 11
    _greedy(p, toks, nxt, 1, parts)                     # position 12 (a forward)
    refs["g6"] = _ref(toks, parts)
    refs["g3"] = _ref(G3, [base.fork(0).feed(G3)])        # (after the edit, like everything the device computes)
    # G7
    p, toks, parts = base.fork(0), list(G7_HEAD), []
    parts.append(p.feed(toks))
    for _ in range(G7_ROUNDS):
        nxt = _greedy(p, toks, SPIKE, 1, parts)
        _greedy(p, toks, nxt, G7_CLEAN, parts)
    refs["g7"] = _ref(toks, parts)
    for name in ("g1", "g4b", "g5"):
        assert spike2 not in refs[name].tokens
    return Built(fw, fw32, spike2, refs)


# ------------------------------------------------------------------------------------------------
# a context made of the reference and the mirror: what the drivers see on a device that keeps the contract
# ------------------------------------------------------------------------------------------------
class Fake:
    """llmk.Llmk as far as the drivers use it.  Every fed prefix must be a prefix of one of the built sequences."""

    def __init__(self, b: Built):
        self.b, self.mirror, self.fed, self.launches = b, Mirror(b.fw.shape.n_layers), [], []

    def _at(self, token: int, pos: int) -> tuple:
        self.fed = self.fed[:pos - 1] + [int(token)]
        assert len(self.fed) == pos
        for r in self.b.refs.values():
            if len(r.tokens) >= pos and np.array_equal(r.tokens[:pos], self.fed):
                return r, pos - 1
        raise AssertionError(("no reference for", self.fed))

    def forward(self, token, pos):
        r, i = self._at(token, pos)
        self.launches.append(self.mirror.launch(pos, r.xb[i], r.hb[i]))
        return r.logits[i].astype(np.float32)

    def decode_greedy(self, token, pos0, n):
        ids = []
        for i in range(n):
            token = int(np.argmax(self.forward(token, pos0 + i))) + 1
            ids.append(token)
        return np.array(ids, np.int32)

    def prefill(self, tokens, pos0=1):
        for i, t in enumerate(tokens):
            r, j = self._at(t, pos0 + i)
        self.mirror.clear()
        return r.logits[j].astype(np.float32)

    def score(self, tokens, pos0=1, **kw):
        self.prefill(tokens, pos0)

    def reset(self):
        self.fed = []
        self.mirror.clear()

    def peek(self, which, n, layer=0, pos=1):
        assert which == 8 and n == 8 * TK_QSC_LMAX
        return self.mirror.rec.raw()

    def path(self):
        return 1

    def close(self):
        pass


# ------------------------------------------------------------------------------------------------
# the drivers
# ------------------------------------------------------------------------------------------------
class Worst:
    """the largest errors a run of the drivers met (printed, and quoted in DESIGN.md)"""

    def __init__(self):
        self.record = self.logit = self.top8 = 0.0

    def __repr__(self):
        return f"worst record error {self.record:.3g}, worst logit error {self.logit:.3g} (top-8 element-wise {self.top8:.3g})"


def check_R(m, fed: Ref, npos: int, worst: Worst, L: int) -> Records:
    """Invariant R: a record field whose tag is p holds the reference maximum of position p of the sequence actually fed (its first
    npos positions), relative error at most REL_TOL; nothing is tagged beyond npos or behind layer L.  Returns the records read."""
    rec = read_records(m)
    assert not rec.tag[:, L:].any() and not rec.val[:, L:].any(), "records behind the last layer"
    for b in range(2):
        for l in range(L):
            for kind, ref in ((XB, fed.xb), (HB, fed.hb)):
                p = int(rec.tag[b, l, kind])
                if p == 0:
                    continue
                assert 1 <= p <= npos and (p & 1) == b, ("tag", p, "buffer", b, "layer", l, "kind", kind, "fed", npos)
                err = abs(float(rec.val[b, l, kind]) / ref[p - 1, l] - 1.0)
                worst.record = max(worst.record, err)
                assert err <= REL_TOL, ("R", "tag", p, "layer", l, "kind", kind, float(rec.val[b, l, kind]), ref[p - 1, l], err)
    return rec


def tagged(rec: Records, pos: int, L: int) -> list:
    """the (layer, kind) fields of buffer pos & 1 that carry tag pos"""
    return [(l, k) for l in range(L) for k in (XB, HB) if int(rec.tag[pos & 1, l, k]) == pos]


def check_logits(got, fed: Ref, pos: int, worst: Worst):
    """position pos's logits within REL_TOL of the reference's: of max |logit|, and element-wise on its eight largest"""
    ref = fed.logits[pos - 1]
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    idx = np.argsort(-ref, kind="stable")[:8]
    e8 = (np.abs(got[idx] - ref[idx]) / np.abs(ref[idx])).max()
    worst.logit, worst.top8 = max(worst.logit, err), max(worst.top8, e8)
    assert err <= REL_TOL and e8 <= REL_TOL, ("logits of position", pos, err, e8)


def expected(b: Built, name: str, npos: int = None) -> list:
    """the launches of refs[name]'s positions 1 .. npos fed one after the other on a fresh context, by the mirror"""
    r = b.refs[name]
    mi = Mirror(b.fw.shape.n_layers)
    return [mi.launch(p, r.xb[p - 1], r.hb[p - 1]) for p in range(1, (len(r.tokens) if npos is None else npos) + 1)]


ALL = lambda L: [(l, k) for l in range(L) for k in (XB, HB)]


def feed(m, fed: Ref, positions, worst: Worst, L: int, want: list):
    """forward() at each of `positions` of the sequence, with R, the tags the mirror's launch `want[pos - 1]` leaves, and the logits"""
    for pos in positions:
        lg = m.forward(int(fed.tokens[pos - 1]), pos)
        rec = check_R(m, fed, pos, worst, L)
        assert tagged(rec, pos, L) == want[pos - 1].written, (pos, tagged(rec, pos, L), want[pos - 1].written)
        assert m.path() == 1, "the kernel was retired"
        check_logits(lg, fed, pos, worst)


def g1(m, b: Built, worst: Worst):
    """clean run"""
    fed, L = b.refs["g1"], b.fw.shape.n_layers
    want = expected(b, "g1")
    assert all(w.event is None for w in want)
    before = read_records(m)
    assert not before.val.any() and not before.tag.any()
    for pos in range(1, len(fed.tokens) + 1):
        feed(m, fed, [pos], worst, L, want)
        rec = read_records(m)
        assert tagged(rec, pos, L) == ALL(L)
        o = (pos - 1) & 1
        assert np.array_equal(rec.val[o].view(np.uint32), before.val[o].view(np.uint32)) and np.array_equal(rec.tag[o], before.tag[o]), \
            ("the other buffer changed at position", pos)
        before = rec


def g2(m, b: Built, worst: Worst):
    """event and the positions after it"""
    fed, L = b.refs["g3"], b.fw.shape.n_layers
    want = expected(b, "g3", 7)
    assert [w.event for w in want] == [None] * 4 + [(1, HB)] + [None] * 2
    assert want[4].written == [(0, XB), (0, HB), (1, XB), (1, HB)] and want[5].written == want[6].written == ALL(L)
    feed(m, fed, range(1, 8), worst, L, want)


def g3(m, b: Built, worst: Worst):
    """spike after spike"""
    fed, L = b.refs["g3"], b.fw.shape.n_layers
    want = expected(b, "g3")
    assert [w.event for w in want] == [None] * 4 + [(1, HB)] + [None] * 2 + [(1, HB)] + [None] * 2
    feed(m, fed, range(1, 11), worst, L, want)


def g4(m, b: Built, worst: Worst, how: str):
    """clearing: how = reset | prefill | score"""
    A, B, L = b.refs["g1"], b.refs["g4b"], b.fw.shape.n_layers
    feed(m, A, range(1, 7), worst, L, expected(b, "g1"))
    if how == "reset":
        m.reset()
    elif how == "prefill":
        m.prefill(B.tokens[:6], 1)
    else:
        m.score(B.tokens[:6], 1)
    rec = read_records(m)
    assert not rec.val.any() and not rec.tag.any(), "records left behind " + how
    if how != "reset":
        mi = Mirror(L)
        mi.clear()
        w7 = mi.launch(7, B.xb[6], B.hb[6])          # no position before it: the layer-before rule
        assert w7.event is None
        feed(m, B, [7], worst, L, [None] * 6 + [w7])


def g5(m, b: Built, worst: Worst):
    """rewind over an event"""
    A, F, L = b.refs["g1"], b.refs["g5"], b.fw.shape.n_layers
    feed(m, A, range(1, 8), worst, L, expected(b, "g1"))
    mi = Mirror(L)
    for p in range(1, 8):
        mi.launch(p, A.xb[p - 1], A.hb[p - 1])
    w7 = mi.launch(7, F.xb[6], F.hb[6])
    w8 = mi.launch(8, F.xb[7], F.hb[7])
    assert w7.event == (1, HB) and w8.event is None
    assert (2, XB) not in w7.written and (2, HB) not in w7.written
    feed(m, F, [7, 8], worst, L, [None] * 6 + [w7, w8])


def g6(m, b: Built, worst: Worst, fresh):
    """pipelined loop over two events; fresh() makes a second context"""
    F, L = b.refs["g6"], b.fw.shape.n_layers
    want = expected(b, "g6")
    assert [p for p, w in enumerate(want, 1) if w.event] == [5, 7] and int(F.tokens[6]) == b.spike2
    feed(m, F, range(1, 5), worst, L, want)
    ids = m.decode_greedy(SPIKE, 5, 3)
    assert np.array_equal(ids, F.ids[4:7]), (ids, F.ids[4:7])
    assert m.path() == 1, "the kernel was retired"
    rec = check_R(m, F, 7, worst, L)
    assert tagged(rec, 7, L) == want[6].written == [(0, XB), (0, HB), (1, XB), (1, HB)], tagged(rec, 7, L)
    ids2 = m.decode_greedy(int(ids[-1]), 8, 4)
    assert np.array_equal(ids2, F.ids[7:11]), (ids2, F.ids[7:11])
    check_R(m, F, 11, worst, L)
    feed(m, F, [12], worst, L, want)
    m2 = fresh()
    try:
        for pos in range(1, 5):
            m2.forward(int(F.tokens[pos - 1]), pos)
        ids7 = m2.decode_greedy(SPIKE, 5, 7)
        assert np.array_equal(ids7, F.ids[4:11]), (ids7, F.ids[4:11])
        assert m2.path() == 1
        check_R(m2, F, 11, worst, L)
    finally:
        m2.close()


def g7(m, b: Built, worst: Worst):
    """the counter of events in a row"""
    F, L = b.refs["g7"], b.fw.shape.n_layers
    want = expected(b, "g7")
    spikes = [len(G7_HEAD) + 1 + (1 + G7_CLEAN) * r for r in range(G7_ROUNDS)]
    assert [p for p, w in enumerate(want, 1) if w.event] == spikes
    feed(m, F, range(1, len(G7_HEAD) + 1), worst, L, want)
    for p in spikes:
        ids = m.decode_greedy(SPIKE, p, 1)
        assert np.array_equal(ids, F.ids[p - 1:p]), (p, ids, F.ids[p - 1:p])
        assert m.path() == 1, f"the kernel was retired at position {p}"
        rec = check_R(m, F, p, worst, L)
        assert tagged(rec, p, L) == want[p - 1].written
        ids = m.decode_greedy(int(ids[0]), p + 1, G7_CLEAN)
        assert np.array_equal(ids, F.ids[p:p + G7_CLEAN]), (p, ids, F.ids[p:p + G7_CLEAN])
        assert m.path() == 1, f"the kernel was retired behind position {p}"
        rec = check_R(m, F, p + G7_CLEAN, worst, L)
        assert tagged(rec, p + G7_CLEAN, L) == ALL(L)


def g8(m, b: Built, worst: Worst, fresh):
    """A record with another position's tag is not history.  G3 straight through leaves, behind the event of position 8, layer 2's
    record of position 6 in the buffer position 9 reads; a second context feeds position 8 twice, which drops it (and changes
    nothing else: the same launch, the same redo).  Positions 9 and 10 must not be able to tell: bit-identical logits."""
    F, L = b.refs["g3"], b.fw.shape.n_layers
    want = expected(b, "g3")
    feed(m, F, range(1, 9), worst, L, want)
    assert int(read_records(m).tag[0, 2, HB]) == 6
    m2 = fresh()
    feed(m2, F, range(1, 9), worst, L, want)
    feed(m2, F, [8], worst, L, want)
    assert not read_records(m2).tag[0, 2].any()
    for pos in (9, 10):
        a = m.forward(int(F.tokens[pos - 1]), pos)
        c = m2.forward(int(F.tokens[pos - 1]), pos)
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32)), ("position", pos, np.abs(a - c).max())
        check_logits(a, F, pos, worst)
        ra, rc = check_R(m, F, pos, worst, L), check_R(m2, F, pos, worst, L)
        assert tagged(ra, pos, L) == tagged(rc, pos, L) == ALL(L)
        assert np.array_equal(ra.val[pos & 1].view(np.uint32), rc.val[pos & 1].view(np.uint32))
