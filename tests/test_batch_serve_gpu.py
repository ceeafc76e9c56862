"""A batch as it is served: ONE long-lived batch through every kind of call, in the orders of the seeded traces
of tests/serve_trace.py, checked against the host model after every op -- where the per-feature files start from a fresh batch, make
one or two calls and close it.  What the library keeps between calls (the column map and `first` words, the part states, prefix
blocks that only grow, token records and record buffers grown by reserve, the logits rows a wide span pass reserved, "the rows
uploaded last", P and the attached count, llmk_forward's launch in flight) meets here in orders no other file uses;
tests/test_batch_serve_cpu.py names the transitions and asserts that the traces go through them.

   1  the traces "span-first" and "prefix-first" on tk-small and tiny-kvmul3, f32 weights, f32 | f16 | q8_0 caches; tk-small with q4_0
      weights and a q6_K classifier; tk-small under LLMK_PF_F32_MFMA=1
   2  the trace "two": two batches of different cache types that take turns on one context
   3  size: the converting copies' second grid-stride sweep and its ragged end (1,331,200 elements)
   4  size: cache offsets beyond 2^31 elements (128 slots x 2,048 positions x 9 layers of kv_dim 1,024)

After every op: logits (forward, forward_spans, and the replay of every decode) within REL_TOL by rel_err and the top-8 element-wise
error -- an f32 batch against the float64 pass over the slot's logical sequence alone, an f16 / q8_0 batch against forward_fed on the
rows it stored (the prefix rows from slot -1, then the slot's own), those rows being halves / idempotent q8_0 rows and layer 0's
bit for bit stored_half / stored_q8 of a lockstep f32 batch's; argmax_out the first maximum; decode ids what llmk_rows_sample_logits
answers on the replay's logits, log-prob records what llmk_logprob_logits answers; token records; zero rows behind a forked or attached
slot's sequence; the refusals' codes; prefix_len, cache type and cache_bytes."""
import functools
import os

import numpy as np
import pytest

import kv16_ref as kr
import kvq8_ref as kq
import serve_trace as st
from conftest import REL_TOL, rel_err, top8_elementwise
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf
from ref_pass import Given, RefPass
from test_batch_kv16_gpu import bits, code_of, first_max, representable

pytestmark = pytest.mark.gpu

E_NOMEM = 7
# the shapes of the size cases: kv_dim 1,024 (Llama-2-7B's is 4,096; the sweeps are counted in elements, the offsets too)
SIZE_SHAPES = {"sweep": gguf.LlamaShape(1024, 1024, 1, 8, 8, 512, 1536), "big": gguf.LlamaShape(1024, 1024, 9, 8, 8, 512, 2048)}
STORED = {"f32": lambda x: np.asarray(x, np.float32), "f16": kr.stored_half, "q8_0": kq.stored_q8}
IS_STORED = {"f32": lambda x: bool(np.isfinite(x).all()), "f16": representable, "q8_0": kq.idempotent}


@functools.lru_cache(maxsize=None)
def weights(shape, wtype=gguf.GGML_F32, q6k=False, seed=777):
    """(weights for the device, the same decoded to f32, a RefPass on them whose converted matrices every fork shares)"""
    s = gguf.SHAPES.get(shape) or SIZE_SHAPES[shape]
    fw = gguf.synth_fused(s, seed, wtype)
    if q6k:
        fw = gguf.with_q6k_classifier(fw)
    fw32 = fw.as_f32() if (wtype or q6k) else fw
    return fw, fw32, RefPass(fw32)


class Worst:
    """the worst rel_err and top-8 figure of a case; every comparison is asserted at REL_TOL where it is made"""

    def __init__(self, label):
        self.label, self.rel, self.top8, self.rows = label, 0.0, 0.0, 0

    def check(self, what, got, ref):
        got, ref = np.asarray(got, np.float32).reshape(-1, ref.shape[-1]), np.asarray(ref, np.float64).reshape(-1, ref.shape[-1])
        assert not np.isnan(got).any(), (self.label, what)
        err, e8 = rel_err(got, ref).max(), top8_elementwise(got, ref=ref).max()
        self.rel, self.top8, self.rows = max(self.rel, err), max(self.top8, e8), self.rows + len(got)
        assert err <= REL_TOL and e8 <= REL_TOL, (self.label, what, err, e8)

    def report(self):
        print(f"{self.label}: {self.rows} rows, worst rel_err {self.rel:.2e}, worst top-8 {self.top8:.2e}")


def ctx_rows(m, n):
    """the context's K | V rows of positions 1..n: [2][L][n][KV]"""
    s = m.shape
    return np.stack([np.stack([np.stack([m.peek(4 + which, s.kv_dim, l, p) for p in range(1, n + 1)]) for l in range(s.n_layers)]) for which in (0, 1)])


def forward_fed(ref0, tokens, K, V, pos):
    """kv16_ref.forward_fed -- the float64 pass whose attention reads the GIVEN rows K[l], V[l] -- on a RefPass that has its matrices
    converted already (a fork shares them)"""
    return ref0.fork(0).feed(tokens, np.asarray(pos), Given(K, V))


def is_zero(rows):
    return not bits(rows).any()                                               # +0.0, bit for bit


class Served:
    """one batch of a trace on the device next to its model (serve_trace.BatchModel); an f16 / q8_0 batch has an f32 batch in lockstep"""

    def __init__(self, m, ref0, bm, worst):
        self.m, self.ref0, self.bm, self.worst, self.s = m, ref0, bm, worst, m.shape
        self.t = bm.kv_type
        self.b = llmk.Batch(m, bm.n_slots, kv_type=self.t)
        self.lock = llmk.Batch(m, bm.n_slots) if self.t != "f32" else None
        self.prefix_rows = None

    def close(self):
        for b in (self.b, self.lock):
            if b is not None:
                b.close()

    def both(self):
        return [b for b in (self.b, self.lock) if b is not None]

    # ---- rows ----
    def slot_rows(self, slot, upto):
        """(K, V) [L][upto][KV] of the slot's positions 1..upto as an attention pass reads them: the prefix rows, then its own"""
        P = self.bm.P if self.bm.slots[slot].attached else 0
        out = []
        for which in (0, 1):
            per = []
            for l in range(self.s.n_layers):
                own = self.b.peek_kv(which, l, slot, P + 1, upto - P)
                per.append(np.concatenate([self.b.peek_kv(which, l, -1, 1, P), own]) if P else own)
            out.append(np.stack(per))
            assert IS_STORED[self.t](out[-1]), (slot, which)
        return out

    def layer0(self, slot, pos, n):
        """layer 0's rows depend on token and position alone: exactly what the type stores for the lockstep f32 batch's rows"""
        if self.lock is None:
            return
        for which in (0, 1):
            x, h = self.lock.peek_kv(which, 0, slot, pos, n), self.b.peek_kv(which, 0, slot, pos, n)
            assert x.any() and np.array_equal(bits(h), bits(STORED[self.t](x))), (self.t, slot, pos, n, which)

    def zero_behind(self, slot):
        hi = self.bm.slots[slot].hi
        for b in self.both():
            for which in (0, 1):
                for l in range(self.s.n_layers):
                    if hi < self.bm.S:
                        assert is_zero(b.peek_kv(which, l, slot, hi + 1, self.bm.S - hi)), (slot, hi, which, l)

    def accounting(self):
        assert self.b.prefix_len == self.bm.P and self.b.kv_type == self.t and self.b.cache_bytes() == self.bm.cache_bytes(self.s)

    def records(self, slots):
        if self.bm.has_records:
            for slot in slots:
                assert np.array_equal(self.b.get_history(slot, self.bm.S), self.bm.slots[slot].rec), slot

    # ---- passes ----
    def reference(self, ref, spans, toks):
        """an f32 batch: the model's; else forward_fed on the stored rows, per span (slot, pos0, len) of the pass"""
        if self.t == "f32":
            return ref
        out, r = [], 0
        for slot, p, n in spans:
            K, V = self.slot_rows(slot, p + n - 1)
            out.append(forward_fed(self.ref0, toks[r:r + n], K, V, np.arange(p, p + n)))
            r += n
        return np.concatenate(out)

    def forward(self, what, slots, toks, pos, ref, twice=False):
        lg, am = self.b.forward(slots, toks, pos)
        assert np.array_equal(am, first_max(lg)), what
        if twice:
            lg2, am2 = self.b.forward(slots, toks, pos)
            assert np.array_equal(bits(lg), bits(lg2)) and np.array_equal(am, am2), what
        self.worst.check(what, lg, self.reference(ref, [(sl, p, 1) for sl, p in zip(slots, pos)], toks))
        if self.lock is not None:
            self.lock.forward(slots, toks, pos)
            for sl, p in zip(slots, pos):
                self.layer0(sl, p, 1)
        return lg

    def spans(self, what, op, ref):
        spans, toks, last = op["spans"], op["tokens"], bool(op.get("last_only"))
        lg, am = self.b.forward_spans(spans, toks, last_only=last)
        assert np.array_equal(am, first_max(lg)), what
        want = self.reference(None, spans, toks) if self.t != "f32" else ref
        if last and self.t != "f32":
            want = want[np.cumsum([n for _, _, n in spans]) - 1]
        self.worst.check(what, lg, want)
        if self.lock is not None:
            self.lock.forward_spans(spans, toks, want_argmax=False)
            for sl, p, n in spans:
                self.layer0(sl, p, n)

    def decode(self, what, w, op):
        slots, toks, pos0, steps = op["slots"], op["tokens"], op["pos0"], op["steps"]
        sps = [llmk.sampler(**sp) for sp in op["samplers"]] if op.get("samplers") else None
        pns = [llmk.penalties(**pn) for pn in op["penalties"]] if op.get("penalties") else None
        top_n, want_lp = op.get("top_n"), bool(op.get("want_lp"))
        tlp = tt = tv = None
        if op["op"] == "decode":
            ids = self.b.decode(slots, toks, pos0, steps, sps)
        else:
            out = self.b.decode_rows(slots, toks, pos0, steps, sps, pns, top_n=top_n, want_token_logprob=want_lp)
            out = list(out) if isinstance(out, tuple) else [out]
            ids = out.pop(0)
            tlp = out.pop(0) if want_lp else None
            tt, tv = out if top_n else (None, None)
        assert ids.shape == (len(slots), steps) and ids.min() >= 1 and ids.max() <= self.m.V, what
        refs = w.finish(op, ids)
        self.records(slots)
        # the header's definition, replayed on this very batch: a row is a function of its token and the earlier rows, so the rewrite
        # leaves the same bits, and every id is what the hooks answer on the replay's logits
        for stp, fed in enumerate(w.fed(op, ids)):
            pos = [p + stp for p in pos0]
            lg = self.forward(f"{what} replay {stp}", slots, fed, pos, refs[stp] if refs is not None else None)
            if sps is None:
                assert np.array_equal(ids[:, stp], first_max(lg)), (what, stp)
            else:
                got = self.b.sample_logits_rows(slots, pos, lg, sps, pns)[0]
                assert np.array_equal(ids[:, stp], got), (what, stp, ids[:, stp], got)
            for i in range(len(slots) if (want_lp or top_n) else 0):
                tl, wt, wv = self.m.logprob_logits(lg[i], int(ids[i, stp]), top_n or 0)
                if want_lp:
                    assert bits(tlp[i, stp]) == bits(np.float32(tl)), (what, stp, i)
                if top_n:
                    assert np.array_equal(tt[i, stp], wt) and np.array_equal(bits(tv[i, stp]), bits(wv)), (what, stp, i)
        self.records(slots)

    def sample_rows(self, what, op, expect):
        slots, pos, top_n, want_lp = op["slots"], op["pos"], op.get("top_n"), bool(op.get("want_lp"))
        z = (np.random.default_rng(op["seed"]).standard_normal((len(slots), self.m.V)) * 3).astype(np.float32)
        pens = op.get("penalties") or [{}] * len(slots)
        out = list(self.b.sample_logits_rows(slots, pos, z, [llmk.sampler(**sp) for sp in op["samplers"]],
                                             [llmk.penalties(**pn) for pn in pens] if op.get("penalties") else None, top_n=top_n,
                                             want_token_logprob=want_lp))
        tok, kept, tau, adj = out[:4]
        for i, (sp, pn) in enumerate(zip(op["samplers"], pens)):
            self.m.set_history(expect["records"][i])
            wtok, wkept, wtau, wadj = self.m.sample_logits_pen(z[i], pos[i], **sp, **pn)
            assert (tok[i], kept[i]) == (wtok, wkept) and bits(tau[i]) == bits(np.float32(wtau)) and np.array_equal(bits(adj[i]), bits(wadj)), (what, i)
            if want_lp or top_n:
                tl, wt, wv = self.m.logprob_logits(z[i], int(tok[i]), top_n or 0)
                rest = out[4:]
                if want_lp:
                    assert bits(rest.pop(0)[i]) == bits(np.float32(tl)), (what, i)
                if top_n:
                    assert np.array_equal(rest[0][i], wt) and np.array_equal(bits(rest[1][i]), bits(wv)), (what, i)

    # ---- an op of this batch ----
    def step(self, what, w, op, expect, twice):
        kind, bm, b = op["op"], self.bm, self.b
        if kind == "fork":
            slot, n = op["slot"], op["n_pos"]
            for bb in self.both():
                bb.fork(slot, n)
            if n:
                rows = ctx_rows(self.m, n)
                for which in (0, 1):
                    for l in range(self.s.n_layers):
                        assert np.array_equal(bits(b.peek_kv(which, l, slot, 1, n)), bits(STORED[self.t](rows[which, l]))), (what, which, l)
            self.zero_behind(slot)
            self.records([slot])
        elif kind == "set_prefix":
            n = op["n_pos"]
            for bb in self.both():
                bb.set_prefix(n)
            if n:
                rows = ctx_rows(self.m, n)
                self.prefix_rows = np.stack([np.stack([b.peek_kv(which, l, -1, 1, n) for l in range(self.s.n_layers)]) for which in (0, 1)])
                assert np.array_equal(bits(self.prefix_rows), bits(STORED[self.t](rows))), what
        elif kind == "attach":
            for bb in self.both():
                bb.attach(op["slot"])
            self.zero_behind(op["slot"])
            self.records([op["slot"]])
        elif kind == "forward":
            self.forward(what, op["slots"], op["tokens"], op["pos"], expect["logits"], twice)
        elif kind == "spans":
            self.spans(what, op, expect["logits"])
        elif kind in ("decode", "decode_rows"):
            self.decode(what, w, op)
        elif kind == "set_history":
            b.set_history(op["slot"], op["tokens"], op["pos0"])
            self.records([op["slot"]])
        elif kind == "get_history":
            assert np.array_equal(b.get_history(op["slot"], bm.S), expect["record"]), what
        elif kind == "sample_rows":
            self.sample_rows(what, op, expect)
        elif kind == "time":
            assert b.time(op["n"], op["pos"], op["iters"]) > 0.0
        elif kind == "time_spans":
            assert b.time_spans(op["n_spans"], op["len"], op["pos0"], op["iters"]) > 0.0
        elif kind == "peek":
            slot = op["slot"]
            if slot < 0:                                                      # a snapshot: nothing the context did since has moved it
                now = np.stack([np.stack([b.peek_kv(which, l, -1, 1, bm.P) for l in range(self.s.n_layers)]) for which in (0, 1)])
                assert np.array_equal(bits(now), bits(self.prefix_rows)), what
            else:
                self.zero_behind(slot)
                for which in (0, 1):
                    assert IS_STORED[self.t](b.peek_kv(which, self.s.n_layers - 1, slot, 1, bm.S)), (what, which)
        elif kind == "refuse":
            r = op["what"]
            if r == "rows129":
                code = code_of(b.forward_spans, op["spans"], op["tokens"])
            elif r == "set_prefix_attached":
                code = code_of(b.set_prefix, op["n_pos"])
            elif r == "attach_no_prefix":
                code = code_of(b.attach, op["slot"])
            else:
                code = code_of(b.forward, op["slots"], op["tokens"], op["pos"])
            assert code == expect["code"], (what, code)
        else:
            raise AssertionError(kind)
        self.accounting()


def run_trace(m, ref, name, kv_types, label):
    """the ops of trace `name` on context m and one batch per cache type, the model's answer checked after every op"""
    ops = st.generate(name)
    s = m.shape
    w = st.World(s.seq_len, s.vocab_size, kv_types, ref)
    worst = Worst(label)
    served = [Served(m, ref, bm, worst) for bm in w.b]
    last = {bi: max(k for k, op in enumerate(ops) if op["op"] == "forward" and op["b"] == bi) for bi in range(len(kv_types))}
    m.reset()
    try:
        for k, op in enumerate(ops):
            kind, what = op["op"], f"{label} op {k} {op['op']}"
            pos0 = w.n + 1
            expect = w.begin(op)
            if kind == "prefill":
                worst.check(what, m.prefill(op["tokens"], pos0), expect["logits"][-1:])
            elif kind == "greedy":
                tok, fed, lgs = op["token"], [], []
                for i in range(st.RUN):
                    lgs.append(m.forward(tok, pos0 + i))
                    fed.append(tok)
                    tok = int(first_max(lgs[-1]))
                if m.path() == 1:                                             # the persistent kernel: position pos0 + RUN is in flight
                    assert m.forward_ahead_stats()["armed"], what
                worst.check(what, np.stack(lgs), w.finish(op, fed))
            elif kind == "reset":
                m.reset()
            else:
                served[op["b"]].step(what, w, op, expect, twice=(k == last[op["b"]]))
    finally:
        for sv in served:
            sv.close()
    worst.report()
    return worst


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
CASES = {f"{shape}-{t}": (shape, gguf.GGML_F32, False, t, False) for shape in ("tk-small", "tiny-kvmul3") for t in ("f32", "f16", "q8_0")}
CASES["tk-small-q4_0-q6k-f32"] = ("tk-small", gguf.GGML_Q4_0, True, "f32", False)
CASES.update({f"tk-small-{t}-f32-mfma": ("tk-small", gguf.GGML_F32, False, t, True) for t in ("f32", "f16", "q8_0")})


def context(fw, f32_mfma):
    """a context; f32_mfma: created, and taken through its first batched call, under LLMK_PF_F32_MFMA=1 -- the instruction a context
    that once saw an outlier stays on for good"""
    if not f32_mfma:
        return llmk.Llmk(fw)
    os.environ["LLMK_PF_F32_MFMA"] = "1"
    try:
        m = llmk.Llmk(fw)
        b = llmk.Batch(m, 1)
        b.forward([0], [2], [1], want_argmax=False)
        b.close()
    finally:
        del os.environ["LLMK_PF_F32_MFMA"]
    return m


@pytest.mark.parametrize("name", ["span-first", "prefix-first"])
@pytest.mark.parametrize("cid", list(CASES))
def test_one_batch_through_every_call_kind_answers_what_the_model_expects(cid, name):
    """Measured worst rel_err / top-8 per case: DESIGN.md section 3i (printed here)."""
    shape, wtype, q6k, t, f32_mfma = CASES[cid]
    fw, _, ref = weights(shape, wtype, q6k)
    m = context(fw, f32_mfma)
    try:
        assert shape != "tk-small" or wtype != gguf.GGML_F32 or m.path() == 1, m.path_name()      # transition j really arms
        run_trace(m, ref, name, [t], f"{cid}, {name}")
    finally:
        m.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("types", [("f16", "q8_0"), ("q8_0", "f32")], ids=["f16+q8_0", "q8_0+f32"])
def test_two_batches_of_different_cache_types_take_turns_on_one_context(types):
    fw, _, ref = weights("tk-small")
    m = llmk.Llmk(fw)
    try:
        run_trace(m, ref, "two", list(types), f"tk-small {'+'.join(types)}, two")
    finally:
        m.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
SWEEP = SIZE_SHAPES["sweep"]
SWEEP_N = 1300
BIG = SIZE_SHAPES["big"]
BIG_SLOTS, BIG_N = 128, 40


def prompt(shape, n, seed):
    return [2] + (np.random.default_rng(seed).integers(3, shape.vocab_size, n - 1) + 1).tolist()


def all_rows(b, L, slot, pos0, n):
    return np.stack([np.stack([b.peek_kv(which, l, slot, pos0, n) for l in range(L)]) for which in (0, 1)])


@pytest.fixture(scope="module")
def sweep():
    """the context of the two-sweeps cases, prefilled once: (context, its rows [2][1][1300][1024], the prompt)"""
    fw, _, _ = weights("sweep", seed=20261021)
    m = llmk.Llmk(fw)
    toks = prompt(SWEEP, SWEEP_N, 7)
    m.prefill(toks, 1)
    yield m, ctx_rows(m, SWEEP_N), toks
    m.close()


@pytest.mark.parametrize("t", ["f32", "f16", "q8_0"])
def test_the_converting_copies_second_sweep_and_its_ragged_end(sweep, t):
    """bd_to_half_kernel and bd_to_q8_kernel cover 1,048,576 elements per sweep of their grid (1,024 blocks x 256 threads x 4);
    fork(1, 1300) at kv_dim 1,024 is 1,331,200 elements: one full sweep and a ragged second one.  Every stored row is the context's
    through the type's rule, bit for bit; then a row at 1,301 on the forked slot and one behind the prefix of 1,299, against
    forward_fed on the stored rows."""
    m, rows, toks = sweep
    s, n, P = m.shape, SWEEP_N, SWEEP_N - 1
    assert 2 * 1024 * 256 * 4 > n * s.kv_dim == 1331200 > 1024 * 256 * 4
    ref0 = weights("sweep", seed=20261021)[2]
    worst = Worst(f"two sweeps, {t}")
    b = llmk.Batch(m, 2, kv_type=t)
    try:
        b.fork(1, n)
        b.set_prefix(P)
        assert b.prefix_len == P and b.kv_type == t
        want = STORED[t](rows)
        assert np.array_equal(bits(all_rows(b, 1, 1, 1, n)), bits(want))
        assert np.array_equal(bits(all_rows(b, 1, -1, 1, P)), bits(want[:, :, :P]))
        assert is_zero(all_rows(b, 1, 1, n + 1, s.seq_len - n)) and is_zero(all_rows(b, 1, 0, 1, s.seq_len))
        tok = 77
        lg, am = b.forward([1], [tok], [n + 1])
        assert np.array_equal(am, first_max(lg))
        K, V = all_rows(b, 1, 1, 1, n + 1)
        assert np.array_equal(bits(K[:, :n]), bits(want[0])) and IS_STORED[t](K) and IS_STORED[t](V)
        worst.check("forked row", lg, forward_fed(ref0, [tok], K, V, [n + 1]))
        b.attach(0)
        lg, am = b.forward([0], [toks[P]], [P + 1])
        assert np.array_equal(am, first_max(lg))
        K, V = (np.concatenate([pre, own], axis=1) for pre, own in zip(all_rows(b, 1, -1, 1, P), all_rows(b, 1, 0, P + 1, 1)))
        assert is_zero(all_rows(b, 1, 0, 1, P)) and IS_STORED[t](K) and IS_STORED[t](V)
        worst.check("attached row", lg, forward_fed(ref0, [toks[P]], K, V, [P + 1]))
    finally:
        b.close()
    worst.report()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """the context of the large caches, prefilled once, with the float64 pass over its prompt: (context, rows, prompt, RefPass)"""
    fw, _, ref0 = weights("big", seed=20261022)
    m = llmk.Llmk(fw)
    toks = prompt(BIG, BIG_N, 8)
    m.prefill(toks, 1)
    ref = ref0.fork(0)
    ref.feed(toks)
    yield m, ctx_rows(m, BIG_N), toks, ref
    m.close()


@pytest.mark.parametrize("t", ["f32", "f16", "q8_0"])
def test_cache_offsets_beyond_2_31_elements(big, t):
    """128 slots of 2,048 positions, 9 layers, kv_dim 1,024: 2,415,919,104 elements per cache (19.3 GB of f32 for K and V).  Slot 127's
    rows in the last layer start beyond element 2^31 of the allocation (and, in bytes, beyond 2^32 in every type).  Forks into slots
    127 and 0, a pass with rows of slots 127, 0 and 64, a span on slot 127, and a row of slot 127 at position 2,048 over the zero rows
    in between; an f32 batch against the float64 pass over the logical sequence (zero rows where the cache holds them), the others
    against forward_fed; slots 1 and 126 still read +0.0 in every layer."""
    m, rows, toks, ref = big
    s, L, S, n, last = m.shape, BIG.n_layers, BIG.seq_len, BIG_N, BIG_SLOTS - 1
    assert (((L - 1) * BIG_SLOTS + last) * S) * s.kv_dim > 2 ** 31
    assert L * BIG_SLOTS * S * s.kv_dim == 2415919104
    ref0 = weights("big", seed=20261022)[2]
    worst = Worst(f"offsets beyond 2^31, {t}")
    try:
        b = llmk.Batch(m, BIG_SLOTS, kv_type=t)
    except llmk.LlmkError as e:
        if e.code == E_NOMEM:
            pytest.skip(f"no room on this device for the {t} caches of {BIG_SLOTS} slots x {S} positions")
        raise
    try:
        assert b.cache_bytes() == {"f32": 8, "f16": 4, "q8_0": 2}[t] * 2415919104 + (2415919104 // 8 if t == "q8_0" else 0)
        b.fork(last, n)
        b.fork(0, n)
        want = STORED[t](rows)
        for slot in (last, 0):
            assert np.array_equal(bits(all_rows(b, L, slot, 1, n)), bits(want)), slot
            assert is_zero(all_rows(b, L, slot, n + 1, 8)) and is_zero(all_rows(b, L, slot, S - 7, 8)), slot
        rng = np.random.default_rng(9)
        t3 = (rng.integers(3, s.vocab_size, 3) + 1).tolist()
        span = (rng.integers(3, s.vocab_size, 5) + 1).tolist()
        tail = int(rng.integers(3, s.vocab_size)) + 1

        def fed(slot, toks_, pos0):
            K, V = all_rows(b, L, slot, 1, pos0 + len(toks_) - 1)
            assert all(IS_STORED[t](np.concatenate([z[:, :64], z[:, 64:][:, -1:]], axis=1)) for z in (K, V))      # (the rest is zero rows)
            return forward_fed(ref0, toks_, K, V, np.arange(pos0, pos0 + len(toks_)))
        # a pass with rows of slots 127, 0 and 64 (from position 1)
        lg, am = b.forward([last, 0, 64], t3, [n + 1, n + 1, 1])
        assert np.array_equal(am, first_max(lg))
        r127 = ref.fork(n)
        if t == "f32":
            want3 = np.concatenate([r127.feed(t3[:1]), ref.fork(n).feed(t3[1:2]), ref.fork(0).feed(t3[2:])])
        else:
            want3 = np.concatenate([fed(last, t3[:1], n + 1), fed(0, t3[1:2], n + 1), fed(64, t3[2:], 1)])
        worst.check("slots 127, 0, 64", lg, want3)
        # a span (127, 42, 5)
        lg, am = b.forward_spans([(last, n + 2, 5)], span)
        assert np.array_equal(am, first_max(lg))
        worst.check("span on slot 127", lg, r127.feed(span) if t == "f32" else fed(last, span, n + 2))
        # one row of slot 127 at position 2,048, over the zero rows in between
        lg, am = b.forward([last], [tail], [S])
        assert np.array_equal(am, first_max(lg))
        if t == "f32":
            gap = S - 1 - r127.n
            r127.k = [np.concatenate([k, np.zeros((gap,) + k.shape[1:], k.dtype)]) for k in r127.k]
            r127.v = [np.concatenate([v, np.zeros((gap,) + v.shape[1:], v.dtype)]) for v in r127.v]
            wantz = r127.feed([tail])
        else:
            wantz = fed(last, [tail], S)
        worst.check("slot 127 at position 2048", lg, wantz)
        held = all_rows(b, L, last, 1, S)
        assert np.array_equal(bits(held[:, :, :n]), bits(want)) and is_zero(held[:, :, n + 6:S - 1]) and held[:, :, S - 1].any() and held[:, :, n:n + 6].any()
        assert np.array_equal(bits(all_rows(b, L, 0, 1, n)), bits(want)) and is_zero(all_rows(b, L, 0, n + 2, S - n - 1))
        assert all_rows(b, L, 64, 1, 1).any() and is_zero(all_rows(b, L, 64, 2, S - 1))
        for slot in (1, last - 1):
            assert is_zero(all_rows(b, L, slot, 1, S)), slot
    finally:
        b.close()
    worst.report()
