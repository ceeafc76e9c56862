"""TEST INFRASTRUCTURE -- a host model of a context and the batches that live on it, and seeded traces of a batch as it is served
(DESIGN.md section 3i): one batch through every kind of call, in orders the per-feature files never use.

World is the model: the context's fed tokens, per batch the slots (fed tokens by position, attached flag, token record, the highest
cache row written since the slot was last zeroed, whether a time hook overwrote its rows), the prefix and P.  An op is a dict
{"op": kind, "b": batch index, ...}.  World.begin(op) asserts that the op is legal in the current state, applies it and returns what
the device must answer: reference logits (a RefPass per slot, rolled back with RefPass.fork(n); None without weights), the error code
of a refusal.  Ops whose fed tokens are the device's own answers (a context greedy run, a decode) are completed with World.finish.
World.events collects the op kinds and the transitions (a .. j of tests/test_batch_serve_cpu.py) that the ops went through, from the
op list alone: tests/test_batch_serve_cpu.py replays every committed trace with made-up answers and asserts the coverage.

generate(name) is the generator: numpy.random.default_rng(seed) chooses tokens, lengths, slots and row orders; the order of the
phases is scripted, because every transition has to occur.  It emits only ops that are legal in a World it keeps alongside, plus
deliberate refusals.  Two scripts that take turns on one context give the trace of two batches of different cache types."""
from __future__ import annotations

import re

import numpy as np

E_ARG, E_STATE = 1, 5
MAX_ROWS = 128
RUN = 5                 # forward calls of a context greedy run: forward-ahead is armed by the third
N_SLOTS = 8
REFUSALS = ("twice", "attached_pos", "beyond", "token0", "rows129", "set_prefix_attached", "attach_no_prefix")
OP_KINDS = ("prefill", "greedy", "reset", "fork", "fork0", "set_prefix", "set_prefix0", "attach", "forward_mixed", "spans_mixed", "spans_wide",
            "spans_ones", "spans_last", "draft_spans", "draft_forward", "draft_decode", "decode_greedy", "decode_sampled", "rows_pen", "rows_bias",
            "rows_top_n", "set_history", "get_history", "sample_rows", "time", "time_spans", "peek") + tuple("refuse_" + r for r in REFUSALS)
TRANSITIONS = ("a_span_first", "a_prefix_first", "b_alloc_after_attach", "b_fork_recorded", "b_attach_recorded", "c_lp_plain_first",
               "c_lp_pen_later", "d_forward", "d_decode", "d_sample", "e_chain", "e_reattach", "f_fork", "f_attach", "f_span", "g_order", "h_more_ids",
               "i_refusal_then_pass", "j_fork", "j_set_prefix", "j_forward", "j_continues", "k_two_types")


def active(pen) -> bool:
    """llmk_rows_decode's rule: a bias, or a window with a penalty that is not neutral"""
    return bool(pen.get("bias")) or (pen.get("last_n", 0) > 0 and (pen.get("repeat", 1.0) != 1.0 or pen.get("frequency", 0.0) != 0.0
                                                                    or pen.get("presence", 0.0) != 0.0))


class Slot:
    def __init__(self, S, ref):
        self.seq, self.attached, self.dirty, self.hi, self.rec, self.ref = [], False, False, 0, np.zeros(S, np.int32), ref
        self.long, self.emptied_long, self.forked_away, self.draft = False, False, False, None


class BatchModel:
    def __init__(self, world, n_slots, S, kv_type, refs):
        self.w, self.n_slots, self.S, self.kv_type, self.refs = world, n_slots, S, kv_type, refs
        self.slots = [Slot(S, world.ref0.fork(0) if refs else None) for _ in range(n_slots)]
        self.P, self.prefix, self.prefix_ref, self.cap = 0, [], None, 0
        self.has_records = self.seen_span = self.seen_prefix = self.seen_lp = self.wide = False
        self.max_ids, self.chain, self.P1, self.P2, self.classes = 0, 0, 0, 0, ""

    @property
    def n_attached(self):
        return sum(s.attached for s in self.slots)

    def cache_bytes(self, shape):
        u = 2 * shape.n_layers * shape.kv_dim * (self.n_slots * self.S + self.cap)
        return {"f32": 4 * u, "f16": 2 * u, "q8_0": u // 32 * 34}[self.kv_type]


class World:
    """refs: a RefPass on the f32 weights (None: no numbers, the states and events alone).  batches: the cache type per batch; a batch
    keeps slot references only if it is an f32 batch (the others are judged against the rows they stored)."""

    def __init__(self, S, V, kv_types=("f32",), ref=None, n_slots=N_SLOTS):
        self.S, self.V, self.ref0 = S, V, ref
        self.tokens, self.ref = [], (ref.fork(0) if ref is not None else None)
        self.b = [BatchModel(self, n_slots, S, t, ref is not None and t == "f32") for t in kv_types]
        self.events, self.prev, self.armed_gap = set(), None, False
        if len(set(kv_types)) > 1:
            self.events.add("k_two_types")

    @property
    def n(self):
        return len(self.tokens)

    # ---- the context ----
    def feed_ctx(self, toks):
        assert toks and self.n + len(toks) <= self.S and all(1 <= t <= self.V for t in toks)
        self.tokens = self.tokens + list(toks)
        return self.ref.feed(toks) if self.ref is not None else None

    # ---- a row of a slot ----
    def _row_ok(self, bm, slot, pos, n=1):
        s = bm.slots[slot]
        assert 0 <= slot < bm.n_slots and not s.dirty, ("a slot a time hook overwrote", slot)
        assert 1 <= pos and pos + n - 1 <= bm.S and pos <= len(s.seq) + 1, (slot, pos, len(s.seq))
        assert not s.attached or pos > bm.P, (slot, pos, bm.P)

    def _feed(self, bm, slot, toks, pos):
        """tokens at positions pos .. of `slot`: the rows behind them are dead.  The reference logits [len][V], or None."""
        s = bm.slots[slot]
        s.seq = s.seq[:pos - 1] + list(toks)
        s.hi = max(s.hi, pos + len(toks) - 1)
        s.long = s.long or len(s.seq) >= bm.S - 2
        s.emptied_long = False
        if not bm.refs:
            return None
        s.ref = s.ref.fork(pos - 1)
        return s.ref.feed(toks)

    def _zero(self, bm, slot, how):
        s = bm.slots[slot]
        if bm.has_records and s.rec.any():
            self.events.add(f"b_{how}_recorded")
        s.rec[:] = 0
        s.dirty, s.draft = False, None

    def _records(self, bm):
        if not bm.has_records and bm.n_attached > 0:
            self.events.add("b_alloc_after_attach")
        bm.has_records = True

    def _draft(self, bm, slot, pos, kind):
        d = bm.slots[slot].draft
        if d is not None and d[0] < pos < d[0] + d[1]:
            self.events.add("draft_" + kind)
        bm.slots[slot].draft = None

    def _forward(self, bm, slots, toks, pos):
        out = [self._feed(bm, sl, [t], p) for sl, t, p in zip(slots, toks, pos)]
        return np.concatenate(out) if bm.refs else None

    # ---- an op ----
    def begin(self, op):
        kind = op["op"]
        ev = self.events
        bm = self.b[op.get("b", 0)]
        out = {}
        cls = "x"
        if kind == "prefill":
            out["logits"] = self.feed_ctx(op["tokens"])
            ev.add("prefill")
        elif kind == "greedy":
            assert self.n + RUN <= self.S and 1 <= op["token"] <= self.V
            ev.add("greedy")
        elif kind == "reset":
            self.tokens, self.ref = [], (self.ref0.fork(0) if self.ref0 is not None else None)
            ev.add("reset")
        elif kind == "fork":
            slot, n = op["slot"], op["n_pos"]
            assert 0 <= slot < bm.n_slots and 0 <= n <= min(self.n, bm.S)
            s = bm.slots[slot]
            ev.add("fork" if n else "fork0")
            if s.long and 0 < n < len(s.seq):
                ev.add("f_fork")
            s.emptied_long = s.long and n == 0
            s.long = False
            if s.attached:
                s.attached, s.forked_away = False, True
                if bm.chain == 2 and bm.n_attached == 0:
                    bm.chain = 3
            self._zero(bm, slot, "fork")
            s.seq, s.hi = self.tokens[:n], n
            if bm.refs:
                s.ref = self.ref.fork(n)
            cls = "F"
        elif kind == "set_prefix":
            n = op["n_pos"]
            assert bm.n_attached == 0 and 0 <= n <= min(self.n, bm.S - 1)
            ev.add("set_prefix" if n else "set_prefix0")
            if n and not bm.seen_prefix:
                bm.seen_prefix = True
                if not bm.seen_span:
                    ev.add("a_prefix_first")
            if n and bm.chain == 0:
                bm.chain, bm.P1 = 1, n
            elif n == 0 and bm.chain == 3:
                bm.chain = 4
            elif bm.chain == 4 and n > bm.P1:
                bm.chain, bm.P2 = 5, n
            elif bm.chain == 5 and 0 < n < bm.P2:
                ev.add("e_chain")
            bm.P, bm.prefix, bm.cap = n, self.tokens[:n], max(bm.cap, n)
            if bm.refs:
                bm.prefix_ref = self.ref.fork(n)
        elif kind == "attach":
            slot = op["slot"]
            assert 0 <= slot < bm.n_slots and bm.P > 0
            s = bm.slots[slot]
            ev.add("attach")
            if s.long:
                ev.add("f_attach")
            if s.forked_away:
                ev.add("e_reattach")
            s.long = s.emptied_long = False
            self._zero(bm, slot, "attach")
            s.attached, s.seq, s.hi = True, list(bm.prefix), 0
            if bm.refs:
                s.ref = bm.prefix_ref.fork(bm.P)
            if bm.chain == 1:
                bm.chain = 2
        elif kind == "forward":
            slots, toks, pos = op["slots"], op["tokens"], op["pos"]
            assert 1 <= len(slots) <= bm.n_slots and len(set(slots)) == len(slots) == len(toks) == len(pos)
            assert all(1 <= t <= self.V for t in toks)
            for sl, p in zip(slots, pos):
                self._row_ok(bm, sl, p)
                self._draft(bm, sl, p, "forward")
            att = {bm.slots[sl].attached for sl in slots}
            if att == {True, False}:
                ev.add("forward_mixed")
            cls = "A" if True in att else "P"
            if bm.wide:
                ev.add("d_forward")
            out["logits"] = self._forward(bm, slots, toks, pos)
        elif kind == "spans":
            spans, toks = op["spans"], op["tokens"]
            rows = sum(n for _, _, n in spans)
            assert 1 <= rows <= MAX_ROWS and rows == len(toks) and len({sl for sl, _, _ in spans}) == len(spans)
            assert all(1 <= t <= self.V for t in toks)
            lens = {n for _, _, n in spans}
            refs, r = [], 0
            for sl, p, n in spans:
                assert n >= 1
                self._row_ok(bm, sl, p, n)
                self._draft(bm, sl, p, "spans")
                if p == 1 and bm.slots[sl].emptied_long:
                    ev.add("f_span")
                lg = self._feed(bm, sl, toks[r:r + n], p)
                refs.append(lg[-1:] if (lg is not None and op.get("last_only")) else lg)
                if n > 1:
                    bm.slots[sl].draft = (p, n)
                r += n
            out["logits"] = np.concatenate(refs) if bm.refs else None
            if lens == {1}:
                ev.add("spans_ones")
                cls = "P"
            else:
                cls = "S"
                if not bm.seen_span:
                    bm.seen_span = True
                    if not bm.seen_prefix:
                        ev.add("a_span_first")
                if len(lens) > 1:
                    ev.add("spans_mixed")
                if rows > bm.n_slots:
                    ev.add("spans_wide")
                    bm.wide = True
                if op.get("last_only"):
                    ev.add("spans_last")
        elif kind in ("decode", "decode_rows"):
            slots, toks, pos0, steps = op["slots"], op["tokens"], op["pos0"], op["steps"]
            assert 1 <= len(slots) <= bm.n_slots and len(set(slots)) == len(slots) and 1 <= steps <= 6
            for sl, p in zip(slots, pos0):
                self._row_ok(bm, sl, p, steps)
                self._draft(bm, sl, p, "decode")
            pens = op.get("penalties")
            assert pens is None or op.get("samplers") is not None
            if kind == "decode":
                ev.add("decode_sampled" if op.get("samplers") else "decode_greedy")
            lp = op.get("top_n") is not None or op.get("want_lp")
            pen = pens is not None and any(active(p) for p in pens)
            if pens is not None and any(p.get("bias") for p in pens):
                ev.add("rows_bias")
            if pens is not None and any(p.get("last_n", 0) > 0 and active(p) for p in pens):
                ev.add("rows_pen")
            if op.get("top_n"):
                ev.add("rows_top_n")
            if pen:
                self._records(bm)
            self._lp(bm, lp, pen)
            if bm.max_ids and len(slots) * steps > bm.max_ids:
                ev.add("h_more_ids")
            bm.max_ids = max(bm.max_ids, len(slots) * steps)
            if bm.wide:
                ev.add("d_decode")
            cls = "D"
        elif kind == "set_history":
            slot, toks, pos0 = op["slot"], op["tokens"], op["pos0"]
            assert 0 <= slot < bm.n_slots and len(toks) >= 1 and pos0 >= 1 and pos0 + len(toks) - 1 <= bm.S and all(0 <= t <= self.V for t in toks)
            self._records(bm)
            bm.slots[slot].rec[pos0 - 1:pos0 - 1 + len(toks)] = toks
            ev.add("set_history")
        elif kind == "get_history":
            assert 0 <= op["slot"] < bm.n_slots
            self._records(bm)
            out["record"] = bm.slots[op["slot"]].rec.copy()
            ev.add("get_history")
        elif kind == "sample_rows":
            slots, pos = op["slots"], op["pos"]
            assert 1 <= len(slots) <= bm.n_slots and len(set(slots)) == len(slots) and len(op["samplers"]) == len(slots)
            for sl, p in zip(slots, pos):
                assert 1 <= p <= bm.S and (not bm.slots[sl].attached or p > bm.P)
            pens = op.get("penalties")
            pen = pens is not None and any(active(p) for p in pens)
            if pen:
                self._records(bm)
            self._lp(bm, op.get("top_n") is not None or op.get("want_lp"), pen)
            if bm.wide:
                ev.add("d_sample")
            out["records"] = [bm.slots[sl].rec.copy() for sl in slots]
            ev.add("sample_rows")
        elif kind == "time":
            n, pos = op["n"], op["pos"]
            assert 1 <= n <= bm.n_slots and 1 <= pos <= bm.S
            for s in bm.slots[:n]:
                assert not s.attached or pos > bm.P
                s.dirty, s.hi = True, max(s.hi, pos)
            ev.add("time")
            cls = "T"
        elif kind == "time_spans":
            n, length, pos0 = op["n_spans"], op["len"], op["pos0"]
            assert 1 <= n <= bm.n_slots and length >= 2 and n * length <= MAX_ROWS and 1 <= pos0 and pos0 + length - 1 <= bm.S
            for s in bm.slots[:n]:
                assert not s.attached or pos0 > bm.P
                s.dirty, s.hi = True, max(s.hi, pos0 + length - 1)
            ev.add("time_spans")
            cls = "T"
        elif kind == "peek":
            assert -1 <= op["slot"] < bm.n_slots and (op["slot"] >= 0 or bm.P > 0)
            ev.add("peek")
        elif kind == "refuse":
            what = op["what"]
            out["code"] = self._refusal(bm, what, op)
            ev.add("refuse_" + what)
        else:
            raise AssertionError(kind)
        # ---- what follows what ----
        prev = self.prev
        if prev is not None and prev["op"] == "refuse" and kind in ("forward", "spans"):
            ev.add("i_refusal_then_pass")
        if prev is not None and prev["op"] == "greedy":
            if kind == "fork" and op["n_pos"] > 0:
                ev.add("j_fork")
            if kind == "set_prefix" and op["n_pos"] > 0:
                ev.add("j_set_prefix")
            if kind == "forward":
                ev.add("j_forward")
            if kind in ("fork", "set_prefix", "forward"):
                self.armed_gap = True
        if kind in ("prefill", "greedy") and self.armed_gap and self.n > len(op.get("tokens", ())):
            ev.add("j_continues")
        if kind in ("prefill", "greedy", "reset"):
            self.armed_gap = False
        else:
            bm.classes += cls
            if re.search("SPADTF+P$", bm.classes):
                ev.add("g_order")
        self.prev = op
        return out

    def _lp(self, bm, lp, pen):
        if not lp:
            return
        if not bm.seen_lp and not pen:
            self.events.add("c_lp_plain_first")
        elif pen and "c_lp_plain_first" in self.events:
            self.events.add("c_lp_pen_later")
        bm.seen_lp = True

    def _refusal(self, bm, what, op):
        """a refusal must be one for the reason it names, in the state the model is in: everything else about the call is legal"""
        if what == "twice":
            assert len(op["slots"]) == 2 and op["slots"][0] == op["slots"][1]
            self._row_ok(bm, op["slots"][0], op["pos"][0])
        elif what == "attached_pos":
            (sl,), (p,) = op["slots"], op["pos"]
            assert bm.slots[sl].attached and 1 <= p <= bm.P
        elif what == "beyond":
            assert op["pos"] == [bm.S + 1] and not bm.slots[op["slots"][0]].dirty
        elif what == "token0":
            assert op["tokens"] == [0]
            self._row_ok(bm, op["slots"][0], op["pos"][0])
        elif what == "rows129":
            assert sum(n for _, _, n in op["spans"]) == MAX_ROWS + 1 and len(op["tokens"]) == MAX_ROWS + 1
            assert all(p == 1 and n <= bm.S and not bm.slots[sl].attached for sl, p, n in op["spans"])
        elif what == "set_prefix_attached":
            assert bm.n_attached > 0 and 0 <= op["n_pos"] <= min(self.n, bm.S - 1)
            return E_STATE
        elif what == "attach_no_prefix":
            assert bm.P == 0 and 0 <= op["slot"] < bm.n_slots
            return E_STATE
        else:
            raise AssertionError(what)
        return E_ARG

    def finish(self, op, answer):
        """a greedy run: `answer` the RUN tokens fed (the first is op["token"]); a decode: the ids [n][steps].  Returns the reference
        logits, per call of the run [RUN][V] or per step of the decode [steps][n][V] (None without weights)."""
        if op["op"] == "greedy":
            assert len(answer) == RUN and answer[0] == op["token"]
            out = [self.feed_ctx([int(t)]) for t in answer]
            return np.concatenate(out) if self.ref is not None else None
        bm = self.b[op.get("b", 0)]
        ids = np.asarray(answer)
        slots, steps = op["slots"], op["steps"]
        assert ids.shape == (len(slots), steps) and ids.min() >= 1 and ids.max() <= self.V
        pens = op.get("penalties")
        record = pens is not None and any(active(p) for p in pens)
        out = []
        for st in range(steps):
            toks = list(op["tokens"]) if st == 0 else ids[:, st - 1].tolist()
            pos = [p + st for p in op["pos0"]]
            out.append(self._forward(bm, slots, toks, pos))
            if record:
                for sl, t, p in zip(slots, toks, pos):
                    bm.slots[sl].rec[p - 1] = t
        return np.stack(out) if bm.refs else None

    def fed(self, op, ids):
        """the tokens a decode fed at step st, the way a replay feeds them again: [steps][n]"""
        ids = np.asarray(ids)
        return [list(op["tokens"]) if st == 0 else ids[:, st - 1].tolist() for st in range(op["steps"])]


def made_up(world, op, rng):
    """an answer where the device's is not at hand: ids drawn from the seeded rng"""
    if op["op"] == "greedy":
        return [op["token"]] + (rng.integers(1, world.V, RUN - 1) + 1).tolist()
    return rng.integers(1, world.V, (len(op["slots"]), op["steps"])) + 1


def replay(world, ops, rng):
    """every op through the model with made-up answers: the events"""
    for op in ops:
        world.begin(op)
        if op["op"] in ("greedy", "decode", "decode_rows"):
            world.finish(op, made_up(world, op, rng))
    return world.events


# ---- the generator ------------------------------------------------------------------------------------------------------------------------
SAMPLERS = [dict(temperature=1.0, seed=11, top_k=1), dict(temperature=0.9, seed=12), dict(temperature=0.8, seed=13, top_k=5),
            dict(temperature=1.1, seed=14, top_p=0.9, min_p=0.05)]


class Script:
    """one batch's life, in groups of ops that stay together; between two groups the other script of a two-batch trace may have used
    the context, so a group asks for the context it needs (need) before it forks or sets a prefix"""

    def __init__(self, world, b, rng, ops, prefix_first):
        self.w, self.bi, self.bm, self.rng, self.ops, self.prefix_first = world, b, world.b[b], rng, ops, prefix_first

    def do(self, op, **kw):
        op = dict(op=op, b=self.bi, **kw)
        self.w.begin(op)
        if op["op"] in ("greedy", "decode", "decode_rows"):
            self.w.finish(op, made_up(self.w, op, self.rng))
        self.ops.append(op)

    def tok(self, n=None):
        t = self.rng.integers(1, self.w.V, n or 1) + 1
        return t.tolist() if n else int(t[0])

    def nxt(self, slot):
        return len(self.bm.slots[slot].seq) + 1

    def need(self, n, room=0):
        """the context holds at least n positions and has room for `room` more"""
        w = self.w
        if max(n, w.n) + room > w.S:
            self.do("reset")
        if w.n < n:
            self.do("prefill", tokens=[2] + self.tok(n - w.n - 1) if w.n == 0 and n > 1 else self.tok(n - w.n))

    def fork(self, slot, n):
        self.need(n)
        self.do("fork", slot=slot, n_pos=n)

    def forward(self, slots):
        slots = [int(s) for s in self.rng.permutation(slots)]
        self.do("forward", slots=slots, tokens=self.tok(len(slots)), pos=[self.nxt(s) for s in slots])

    def spans(self, spans, **kw):
        self.do("spans", spans=spans, tokens=self.tok(sum(n for _, _, n in spans)), **kw)

    def samplers(self, n):
        k = int(self.rng.integers(0, 4))
        return [dict(SAMPLERS[(k + i) % 4], seed=int(self.rng.integers(1, 1 << 30))) for i in range(n)]

    def refuse(self, what, **kw):
        self.do("refuse", what=what, **kw)

    def run(self):
        rng, bm, S = self.rng, self.bm, self.w.S
        r = lambda lo, hi: int(rng.integers(lo, hi + 1))      # noqa: E731
        # -- a: the first span pass and the first prefix, in either order
        if self.prefix_first:
            self.need(12)
            self.do("set_prefix", n_pos=7)
            self.do("attach", slot=5)
            self.spans([(0, 1, 3), (5, 8, 2), (1, 1, 1)])
        else:
            self.spans([(0, 1, 3), (1, 1, 1), (2, 1, 2)])
        yield
        # -- forks (0 included), a ragged plain pass, a refusal in front of it
        n3, n4 = r(18, 22), r(8, 11)
        self.fork(3, n3)
        self.fork(4, n4)
        self.do("fork", slot=7, n_pos=0)
        self.refuse("twice", slots=[3, 3], tokens=self.tok(2), pos=[n3 + 1] * 2)
        self.forward([3, 4, 0, 7])
        self.do("peek", slot=4)
        yield
        # -- the prefix and attached rows; b: the records come after the attaching
        if not self.prefix_first:
            self.need(12)
            self.do("set_prefix", n_pos=7)
        self.do("attach", slot=5)
        self.do("attach", slot=6)
        self.refuse("attached_pos", slots=[5], tokens=[self.tok()], pos=[r(1, 7)])
        self.forward([5, 3, 6])
        self.do("peek", slot=-1)
        self.do("set_history", slot=5, tokens=bm.slots[5].seq[:], pos0=1)
        self.do("set_history", slot=3, tokens=self.tok(6), pos0=r(1, 9))
        self.do("get_history", slot=5)
        yield
        # -- c: records without penalties, then with; a bias; h's base line of 4 ids
        rows = dict(slots=[3, 5], tokens=self.tok(2), pos0=[self.nxt(3), self.nxt(5)])
        self.do("decode_rows", **rows, steps=2, samplers=self.samplers(2), penalties=None, top_n=3, want_lp=True)
        rows = dict(slots=[5, 3], tokens=self.tok(2), pos0=[self.nxt(5), self.nxt(3)])
        self.do("decode_rows", **rows, steps=3, samplers=self.samplers(2), penalties=[dict(last_n=8, repeat=1.3, presence=0.2), dict()], top_n=2,
                want_lp=True)
        rows = dict(slots=[3, 4], tokens=self.tok(2), pos0=[self.nxt(3), self.nxt(4)])
        banned = self.tok()
        self.do("decode_rows", **rows, steps=2, samplers=self.samplers(2), penalties=[dict(bias=[(banned, 2.5), (banned % 399 + 2, -1.0)]),
                                                                                      dict(last_n=4, frequency=0.3)], top_n=None, want_lp=False)
        self.do("get_history", slot=3)
        # ... and a fork and an attach of slots that hold records
        self.fork(3, r(12, 16))
        self.do("attach", slot=5)
        self.do("get_history", slot=5)
        self.forward([3, 5])
        yield
        # -- d: a pass wider than the slots, then a plain pass, a decode and the sampling hook
        self.spans([(0, self.nxt(0), 6), (1, self.nxt(1), 5)])
        self.forward([0, 1, 2])
        self.do("decode", slots=[1, 0], tokens=self.tok(2), pos0=[self.nxt(1), self.nxt(0)], steps=4, samplers=None)
        self.do("sample_rows", slots=[0, 1], pos=[self.nxt(0) - 1, self.nxt(1) - 1], seed=r(1, 1 << 20), samplers=self.samplers(2),
                penalties=[dict(last_n=6, repeat=1.2), dict()], top_n=2, want_lp=True)
        yield
        # -- e: every attached slot forked away, the prefix dropped, a longer one, a shorter one; a slot attached again
        self.refuse("set_prefix_attached", n_pos=min(3, self.w.n))
        self.forward([6])
        self.fork(5, r(3, 6))
        self.do("fork", slot=6, n_pos=0)
        self.do("set_prefix", n_pos=0)
        self.refuse("attach_no_prefix", slot=2)
        self.forward([5, 6])
        self.need(30)
        self.do("set_prefix", n_pos=r(15, 17))
        self.do("attach", slot=5)
        self.forward([5, 2])
        self.do("fork", slot=5, n_pos=0)
        self.do("set_prefix", n_pos=r(8, 10))
        self.do("attach", slot=6)
        self.forward([6, 3])
        yield
        # -- f: a slot that held a sequence near seq_len, emptied and refilled shorter: by fork, by attach, from position 1 by a span
        for slot, how in ((1, "fork"), (2, "attach"), (0, "span")):
            self.fork(slot, S - 2)
            self.forward([slot])
            if how == "fork":
                self.fork(slot, r(5, 12))
            elif how == "attach":
                self.do("attach", slot=slot)
            else:
                self.do("fork", slot=slot, n_pos=0)
                self.spans([(slot, 1, 4)])
            self.forward([slot, 3])
        yield
        # -- g: span pass, plain pass, attached pass, decode, time hook, re-fork, plain pass
        self.spans([(0, self.nxt(0), 3), (1, self.nxt(1), 2)])
        self.forward([3, 0])
        self.forward([6, 3, 2])
        self.do("decode", slots=[3, 6], tokens=self.tok(2), pos0=[self.nxt(3), self.nxt(6)], steps=5, samplers=self.samplers(2))
        self.do("time", n=2, pos=r(3, 9), iters=1)
        self.fork(0, r(6, 9))
        self.fork(1, r(6, 9))
        self.forward([0, 1])
        yield
        # -- refusals, each in front of a pass
        self.refuse("beyond", slots=[0], tokens=[self.tok()], pos=[S + 1])
        self.forward([0])
        self.refuse("token0", slots=[1], tokens=[0], pos=[self.nxt(1)])
        self.spans([(1, self.nxt(1), 2), (0, self.nxt(0), 1)], last_only=True)
        self.refuse("rows129", spans=[(0, 1, 43), (1, 1, 43), (3, 1, 43)], tokens=self.tok(129))
        self.spans([(0, self.nxt(0), 1), (1, self.nxt(1), 1), (3, self.nxt(3), 1)])
        yield
        # -- a rejected draft: j of a span's rows accepted, the slot goes on at pos0 + j with other tokens: by a span, a pass, a decode
        for slot, how in ((0, "spans"), (1, "forward"), (3, "decode")):
            p = self.nxt(slot)
            self.spans([(slot, p, 4)])
            at = p + r(1, 3)
            if how == "spans":
                self.spans([(slot, at, 3)])
            elif how == "forward":
                self.do("forward", slots=[slot], tokens=[self.tok()], pos=[at])
            else:
                self.do("decode", slots=[slot], tokens=[self.tok()], pos0=[at], steps=1, samplers=None)
        yield
        # -- h: more ids than any decode before: every slot, 6 steps (the slots a time hook or a long sequence left unusable are refilled)
        for slot in range(bm.n_slots):
            if bm.slots[slot].dirty or self.nxt(slot) + 5 > S:
                self.fork(slot, r(2, 9))
        slots = [int(s) for s in rng.permutation(bm.n_slots)]
        self.do("decode", slots=slots, tokens=self.tok(len(slots)), pos0=[self.nxt(s) for s in slots], steps=6, samplers=self.samplers(len(slots)))
        self.do("time_spans", n_spans=2, len=3, pos0=r(2, 6), iters=1)
        self.fork(0, r(2, 6))
        self.fork(1, 0)
        self.forward([1, 0, 4])
        yield
        # -- j: a context greedy run directly in front of fork, of set_prefix and of a pass; the context goes on behind each
        for slot in range(bm.n_slots):             # (nothing stays attached: set_prefix is legal)
            if bm.slots[slot].attached:
                self.fork(slot, r(0, 4))
        self.need(6, room=3 * RUN + 6)
        self.do("greedy", token=self.tok())
        self.do("fork", slot=2, n_pos=self.w.n)
        self.do("prefill", tokens=self.tok(3))
        self.do("greedy", token=self.tok())
        self.do("set_prefix", n_pos=self.w.n - 1)
        self.do("greedy", token=self.tok())
        self.forward([2, 6])
        self.do("prefill", tokens=self.tok(2))
        self.do("attach", slot=7)
        self.forward([7, 2])
        self.do("get_history", slot=7)


def generate(name):
    """the ops of the committed trace `name`: (cache types of its batches, ops)"""
    seed, firsts = TRACES[name]
    rng = np.random.default_rng(seed)
    w, ops = World(64, 400, ["f32", "q8_0"][:len(firsts)]), []
    runs = [Script(w, i, rng, ops, pf).run() for i, pf in enumerate(firsts)]
    while runs:
        for g in list(runs):
            try:
                next(g)
            except StopIteration:
                runs.remove(g)
    return ops


# name: (seed, per batch: whether the first prefix comes before the first span pass).  Tokens are drawn below 400, the smaller of the
# two vocabularies the traces run on; "two": two batches of different cache types that take turns on one context.
TRACES = {"span-first": (20261021, (False,)), "prefix-first": (20261022, (True,)), "two": (20261023, (False, True))}
