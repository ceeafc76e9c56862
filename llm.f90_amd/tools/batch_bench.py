"""Batched decode against the single-stream decode of the same context, in one process.

    python -m llm_f90_amd.tools.batch_bench --shape tinyllama --type f32
    python -m llm_f90_amd.tools.batch_bench --shape llama2-7b --type q4_0 --cls-q6k

For n = 1, 2, 4, ... 128 rows and positions 25 and 1024: llmk_batch_time's milliseconds per full pass (every layer, the classifier and a
greedy pick for every row) and the aggregate tokens per second n / pass; then llmk_decode_greedy's tokens per second on the same
context (one sequence on the persistent kernel, or whatever path the shape gets).  Every figure is the median of --repeats
measurements behind a warm-up, with the spread (max - min) / median beside it.  Weights are bench.py's synthetic ones (same seed).
Prints a table on stdout and, with --json, one JSON line.

    python -m llm_f90_amd.tools.batch_bench --shape tinyllama --type f32 --sampled

measures whole decode calls instead (64 steps from position 25 at 8, 32 and 128 rows): greedy, one sampler per row, and -- through
llmk_rows_decode, where the library has it -- a repeat penalty and log-prob records on top.

    python -m llm_f90_amd.tools.batch_bench --shape llama2-7b --type q4_0 --cls-q6k --shared-prefix 1000

times the pass at 8, 32 and 128 rows and position --pos (1024) with the slots ATTACHED to one P-position prefix (llmk_prefix_*) and with
the slots FORKED at P, in one process, alternating; against another build selected with LLMK_LIB that has no llmk_prefix_*, the forked
figures alone (--forked-only: the same from this build, no prefix ever set).

    python -m llm_f90_amd.tools.batch_bench --shape llama2-7b --type q4_0 --cls-q6k --kv both --shared-prefix 1000

times the pass at 8, 32 and 128 rows, at positions 25 and --pos, with f32 and with f16 K/V caches (llmk_cache_create): two batches in
ONE process, the types alternating measurement by measurement; forked slots, and -- with --shared-prefix P, at --pos -- slots attached
behind P positions.  --kv f32 | f16 | q8_0 measures one type alone, --kv all the three (q8_0: llmk_cache_create with LLMK_TYPE_Q8_0).

    python -m llm_f90_amd.tools.batch_bench --shape llama2-7b --type q4_0 --cls-q6k --spans

times span passes (llmk_span_*): (a) one span of 128 rows ending at --pos with bd_attn_span_kernel and with the per-row attention
kernels (a second batch created under LLMK_SPAN_ATTN=0), on f32 and f16 caches, llmk_span_time, alternating; (b) a prompt of
--pos - 24 tokens into one slot in spans of 128 against llmk_prefill + llmk_batch_fork, wall clock of the calls; (c) 112 decode rows
at --pos with and without one 16-row chunk of another slot in the same pass, wall clock of the calls."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import llm_f90_amd  # noqa: E402,F401
from llm_f90_amd import llmk  # noqa: E402
from llm_f90_amd.tools import gguf  # noqa: E402

ROWS = (1, 2, 4, 8, 16, 32, 64, 128)
POSITIONS = (25, 1024)


def med_spread(xs):
    m = statistics.median(xs)
    return m, (max(xs) - min(xs)) / m if m else 0.0


def build(shape_name: str, type_name: str, cls_q6k: bool):
    """the context bench.py builds for --shape / --type / --cls-q6k"""
    import bench
    shape = gguf.SHAPES[shape_name]
    wtype = {"f32": 0, "f16": 1, "q4_0": 2}[type_name]
    big = shape.matmul_params() > 3e9
    if big and wtype == 0:
        raise SystemExit("the 7B/70B shapes are benchmarked as q4_0 or f16")
    if cls_q6k and (wtype == 0 or shape.emb_dim % 256):
        raise SystemExit("--cls-q6k: a q6_K classifier beside f16 / q4_0 matrices, emb_dim a multiple of 256")
    fw = None if big else gguf.synth_fused(shape, bench.SEED, wtype)
    if cls_q6k and fw is not None:
        fw = gguf.with_q6k_classifier(fw)
    if big:
        return bench.build_streamed(shape, wtype, fw, 0, 0, 0, 1, None, cls_q6k=cls_q6k), shape
    return llmk.Llmk(fw), shape


SAMPLED_ROWS = (8, 32, 128)
SAMPLED_POS, SAMPLED_STEPS = 25, 64


def sampled(m, shape, repeats: int):
    """--sampled: the wall clock of a whole decode call of SAMPLED_STEPS steps from SAMPLED_POS -- llmk_batch_decode greedy and with one
    sampler per row, and, where the library exports the rows functions, llmk_rows_decode with a repeat penalty and with log-prob
    records on top -- as the median of `repeats` calls behind a warm-up call.  Every call starts from the same rows: it rewrites the
    K/V rows and the token records it wrote before."""
    have_rows = hasattr(llmk.lib(), "llmk_rows_decode")
    b = llmk.Batch(m, max(SAMPLED_ROWS), SAMPLED_POS + SAMPLED_STEPS - 1)
    out = []
    for n in SAMPLED_ROWS:
        rows = (list(range(n)), [2 + i for i in range(n)], [SAMPLED_POS] * n)
        sps = [llmk.sampler(0.9, 1000 + i, top_k=40) for i in range(n)]
        cases = [("greedy", lambda: b.decode(*rows, SAMPLED_STEPS)),
                 ("T0.9 top-k 40", lambda: b.decode(*rows, SAMPLED_STEPS, sps))]
        if have_rows:
            pens = [llmk.penalties(last_n=64, repeat=1.1) for _ in range(n)]
            cases += [("+ repeat 1.1 / 64", lambda: b.decode_rows(*rows, SAMPLED_STEPS, sps, pens)),
                      ("+ top_n 5", lambda: b.decode_rows(*rows, SAMPLED_STEPS, sps, pens, top_n=5, want_token_logprob=True))]
        for name, call in cases:
            call()                                              # warm-up
            ms = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                call()
                ms.append((time.perf_counter() - t0) * 1e3 / SAMPLED_STEPS)
            med, spread = med_spread(ms)
            out.append({"n": n, "sampler": name, "ms_per_step": med, "spread": spread, "tok_s": n / med * 1e3})
    b.close()
    return out


def shared_prefix(m, shape, P: int, pos: int, iters: int, repeats: int, forked_only: bool = False):
    """--shared-prefix P: llmk_batch_time at SAMPLED_ROWS rows, all at `pos`, behind a P-position prompt prefilled on the context -- the
    slots attached to one copy of its K/V rows, then the slots forked at P, `repeats` times in turn, each measurement behind a warm-up
    of the same form."""
    if not 1 <= P < pos <= shape.seq_len:
        raise SystemExit(f"--shared-prefix P --pos Q: 1 <= P < Q <= {shape.seq_len}")
    have = hasattr(llmk.lib(), "llmk_prefix_set") and not forked_only
    m.reset()
    m.prefill([2] + [3 + i % (shape.vocab_size - 3) for i in range(P - 1)], 1)
    slots, b = max(SAMPLED_ROWS), None
    while b is None:
        try:
            b = llmk.Batch(m, slots, pos)
        except llmk.LlmkError as e:
            if slots == 1:
                raise
            print(f"# pos {pos}: no room for {slots} slots ({e}); trying {slots // 2}", file=sys.stderr)
            slots //= 2
    out = []
    for n in SAMPLED_ROWS:
        if n > slots:
            continue
        ms = {"forked": [], "attached": []}
        for _ in range(repeats):
            for form in (("attached", "forked") if have else ("forked",)):
                for j in range(n):
                    b.fork(j, P)                                # (a fork detaches; the prefix is set with no slot attached)
                if form == "attached":
                    b.set_prefix(P)
                    for j in range(n):
                        b.attach(j)
                b.time(n, pos, 3)                               # warm-up in this form
                ms[form].append(b.time(n, pos, iters))
        row = {"n": n, "pos": pos, "prefix": P}
        for form, xs in ms.items():
            if xs:
                row[form + "_ms"], row[form + "_spread"] = med_spread(xs)
        out.append(row)
    b.close()
    return out


def kv_types(m, shape, kinds, P: int, pos: int, iters: int, repeats: int):
    """--kv: llmk_batch_time at SAMPLED_ROWS rows at positions 25 and `pos` on one batch per K/V type in `kinds`, all alive together,
    the types alternating `repeats` times, each measurement behind a warm-up of the same type and form.  Forms: the slots forked
    behind the prompt (position - 1 prompt positions, or P), and with P > 0 at `pos` the slots attached to a P-position prefix."""
    positions = [q for q in (SAMPLED_POS, pos) if q <= shape.seq_len]
    if P and not 1 <= P < pos <= shape.seq_len:
        raise SystemExit(f"--shared-prefix P --pos Q: 1 <= P < Q <= {shape.seq_len}")
    m.reset()
    m.prefill([2] + [3 + i % (shape.vocab_size - 3) for i in range(max(P, SAMPLED_POS) - 1)], 1)
    out = []
    for q in positions:
        slots, bs = max(SAMPLED_ROWS), None
        while bs is None:
            made = {}
            try:
                for kind in kinds:
                    made[kind] = llmk.Batch(m, slots, q, kv_type=kind)
                bs = made
            except llmk.LlmkError as e:
                for b in made.values():
                    b.close()
                if slots == 1:
                    raise
                print(f"# pos {q}: no room for {slots} slots of {' + '.join(kinds)} ({e}); trying {slots // 2}", file=sys.stderr)
                slots //= 2
        behind = min(P, q - 1) if P else min(SAMPLED_POS, q) - 1
        for form in (("forked", "attached") if P and q > P else ("forked",)):
            for n in SAMPLED_ROWS:
                if n > slots:
                    continue
                ms = {kind: [] for kind in kinds}
                for b in bs.values():
                    for j in range(n):
                        b.fork(j, behind)                        # (a fork detaches; the prefix is set with no slot attached)
                    if form == "attached":
                        b.set_prefix(P)
                        for j in range(n):
                            b.attach(j)
                for _ in range(repeats):
                    for kind, b in bs.items():
                        b.time(n, q, 3)                          # warm-up of this type
                        ms[kind].append(b.time(n, q, iters))
                row = {"n": n, "pos": q, "form": form, "behind": behind, "bytes": {kind: b.cache_bytes() for kind, b in bs.items() if hasattr(llmk.lib(), "llmk_cache_bytes")}}
                for kind, xs in ms.items():
                    row[kind + "_ms"], row[kind + "_spread"] = med_spread(xs)
                out.append(row)
        for b in bs.values():
            b.close()
    return out


def spans(m, shape, pos: int, iters: int, repeats: int):
    """--spans: the three measurements of profiles/batch_spans.txt, every figure the median of `repeats` behind a warm-up"""
    out = {"a": [], "b": {}, "c": {}}
    pos0 = pos - 127
    for kind in ("f32", "f16", "q8_0"):
        if kind == "q8_0" and shape.kv_dim % 32:      # (no q8_0 caches on this shape)
            continue
        os.environ["LLMK_SPAN_ATTN"] = "0"
        try:
            rows_b = llmk.Batch(m, 1, pos, kv_type=kind)
        finally:
            del os.environ["LLMK_SPAN_ATTN"]
        span_b = llmk.Batch(m, 1, pos, kv_type=kind)
        ms = {"span": [], "rows": []}
        for _ in range(repeats):
            for form, b in (("span", span_b), ("rows", rows_b)):
                b.time_spans(1, 128, pos0, 3)
                ms[form].append(b.time_spans(1, 128, pos0, iters))
        row = {"kv": kind, "pos0": pos0, "len": 128}
        for form, xs in ms.items():
            row[form + "_ms"], row[form + "_spread"] = med_spread(xs)
        out["a"].append(row)
        rows_b.close()
        span_b.close()
    # (b) a prompt into one slot: spans against prefill + fork
    n = pos - 24
    prompt = [2] + [3 + i % (shape.vocab_size - 3) for i in range(n - 1)]
    b = llmk.Batch(m, 1, pos)
    ms = {"spans": [], "prefill_fork": []}
    for r in range(repeats + 1):
        t0 = time.perf_counter()
        b.ingest(0, prompt)
        t1 = time.perf_counter()
        m.prefill(prompt, 1)
        b.fork(0, n)
        t2 = time.perf_counter()
        if r:
            ms["spans"].append((t1 - t0) * 1e3)
            ms["prefill_fork"].append((t2 - t1) * 1e3)
    out["b"] = {"tokens": n}
    for form, xs in ms.items():
        out["b"][form + "_ms"], out["b"][form + "_spread"] = med_spread(xs)
    b.close()
    # (c) 112 decode rows with and without a 16-row chunk of slot 112 in the same pass
    slots, b = 113, None
    for kind in ("f32", "f16"):
        try:
            b = llmk.Batch(m, slots, pos, kv_type=kind)
            break
        except llmk.LlmkError as e:
            print(f"# (c): no room for {slots} slots of {kind} caches ({e})", file=sys.stderr)
    if b is not None:
        dec = [(j, pos, 1) for j in range(112)]
        forms = {"decode": dec, "decode_chunk": dec + [(112, pos - 15, 16)]}
        ms = {k: [] for k in forms}
        for r in range(repeats + 1):
            for form, sp in forms.items():
                toks = [2] * sum(x[2] for x in sp)
                b.forward_spans(sp, toks, want_logits=False)
                t0 = time.perf_counter()
                for _ in range(iters):
                    b.forward_spans(sp, toks, want_logits=False)
                if r:
                    ms[form].append((time.perf_counter() - t0) * 1e3 / iters)
        out["c"] = {"kv": b.kv_type, "pos": pos}
        for form, xs in ms.items():
            out["c"][form + "_ms"], out["c"][form + "_spread"] = med_spread(xs)
        b.close()
    return out


def print_spans(shape_name, type_name, r, iters, repeats):
    print(f"# library {llmk.LIB_PATH} (llmk_version {llmk.lib().llmk_version()})")
    print(f"# span passes, {shape_name} {type_name}: medians of {repeats} (spread = (max - min) / median)")
    print(f"# (a) one span of 128 rows, llmk_span_time, {iters} passes per measurement, the forms alternating: bd_attn_span_kernel | LLMK_SPAN_ATTN=0")
    print(f"{'kv':>5} {'pos0':>6} {'len':>4} {'span ms':>9} {'spread':>7} {'per-row ms':>11} {'spread':>7} {'per-row / span':>15}")
    for x in r["a"]:
        print(f"{x['kv']:>5} {x['pos0']:6d} {x['len']:4d} {x['span_ms']:9.3f} {x['span_spread']:7.3f} {x['rows_ms']:11.3f} {x['rows_spread']:7.3f} {x['rows_ms'] / x['span_ms']:15.2f}")
    x = r["b"]
    print(f"# (b) a prompt of {x['tokens']} tokens into one slot, wall clock of the calls (f32 caches)")
    print(f"  spans of 128 (Batch.ingest) {x['spans_ms']:9.3f} ms (spread {x['spans_spread']:.3f})   llmk_prefill + llmk_batch_fork {x['prefill_fork_ms']:9.3f} ms (spread {x['prefill_fork_spread']:.3f})")
    x = r["c"]
    if x:
        print(f"# (c) 112 decode rows at position {x['pos']} ({x['kv']} caches), wall clock of llmk_span_forward (argmax only), {iters} calls per measurement")
        print(f"  alone {x['decode_ms']:9.3f} ms (spread {x['decode_spread']:.3f})   + one 16-row chunk of another slot {x['decode_chunk_ms']:9.3f} ms (spread {x['decode_chunk_spread']:.3f})"
              f"   difference {x['decode_chunk_ms'] - x['decode_ms']:.3f} ms")


def print_kv(shape_name, type_name, kinds, rows, iters, repeats):
    print(f"# library {llmk.LIB_PATH} (llmk_version {llmk.lib().llmk_version()})")
    print(f"# batched decode by K/V cache type, {shape_name} {type_name}: llmk_batch_time, median of {repeats} x {iters} passes per type, "
          f"the types alternating in one process (spread = (max - min) / median)")
    ratios = [(a, b) for a, b in (("f32", "f16"), ("f16", "q8_0")) if a in kinds and b in kinds]
    print(f"{'n':>5} {'pos':>6} {'form':>9} {'behind':>7} " + " ".join(f"{k + ' ms':>10} {'spread':>7}" for k in kinds) + "".join(f" {a + ' / ' + b:>11}" for a, b in ratios))
    for r in rows:
        cells = " ".join(f"{r[k + '_ms']:10.3f} {r[k + '_spread']:7.3f}" for k in kinds)
        ratio = "".join(f" {r[a + '_ms'] / r[b + '_ms']:11.2f}" for a, b in ratios)
        print(f"{r['n']:5d} {r['pos']:6d} {r['form']:>9} {r['behind']:7d} {cells}{ratio}")


def print_shared(shape_name, type_name, rows, iters, repeats):
    print(f"# library {llmk.LIB_PATH} (llmk_version {llmk.lib().llmk_version()})")
    print(f"# batched decode behind a shared prompt, {shape_name} {type_name}: llmk_batch_time, median of {repeats} x {iters} passes per form, "
          f"the forms alternating (spread = (max - min) / median)")
    print(f"{'n':>5} {'prefix':>7} {'pos':>6} {'forked ms':>10} {'spread':>7} {'attached ms':>12} {'spread':>7} {'forked / attached':>18}")
    for r in rows:
        att = f"{r['attached_ms']:12.3f} {r['attached_spread']:7.3f} {r['forked_ms'] / r['attached_ms']:18.2f}" if "attached_ms" in r else f"{'-':>12} {'-':>7} {'-':>18}"
        print(f"{r['n']:5d} {r['prefix']:7d} {r['pos']:6d} {r['forked_ms']:10.3f} {r['forked_spread']:7.3f} {att}")


def print_sampled(shape_name, type_name, rows, repeats):
    print(f"# library {llmk.LIB_PATH} (llmk_version {llmk.lib().llmk_version()})")
    print(f"# llmk_batch_decode / llmk_rows_decode, {shape_name} {type_name}, {SAMPLED_STEPS} steps from position {SAMPLED_POS}: wall clock of the call, "
          f"median of {repeats} behind a warm-up (spread = (max - min) / median; + over greedy: ms/step above the greedy call of the same n)")
    print(f"{'n':>5} {'sampler':>20} {'ms/step':>9} {'spread':>7} {'+- ms':>7} {'tok/s':>10} {'+ over greedy':>14}")
    greedy = {r["n"]: r["ms_per_step"] for r in rows if r["sampler"] == "greedy"}
    for r in rows:
        print(f"{r['n']:5d} {r['sampler']:>20} {r['ms_per_step']:9.3f} {r['spread']:7.3f} {r['spread'] * r['ms_per_step']:7.3f} {r['tok_s']:10.1f} "
              f"{r['ms_per_step'] - greedy[r['n']]:14.3f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", default="tinyllama", choices=sorted(gguf.SHAPES))
    ap.add_argument("--type", default="f32", choices=["f32", "f16", "q4_0"])
    ap.add_argument("--cls-q6k", action="store_true")
    ap.add_argument("--iters", type=int, default=20, help="passes per measurement")
    ap.add_argument("--repeats", type=int, default=5, help="measurements per figure (the median is reported)")
    ap.add_argument("--decode-steps", type=int, default=248, help="positions of one llmk_decode_greedy measurement (behind 8 warm-up positions)")
    ap.add_argument("--single-only", action="store_true",
                    help="only the llmk_decode_greedy figures: the baseline of another build of the library selected with LLMK_LIB")
    ap.add_argument("--sampled", action="store_true",
                    help="only the sampled-decode table: whole llmk_batch_decode / llmk_rows_decode calls at 8, 32 and 128 rows (also "
                         "against another build selected with LLMK_LIB: the rows functions are measured where the library has them)")
    ap.add_argument("--shared-prefix", type=int, default=0, metavar="P",
                    help="only the shared-prefix table: the pass at 8, 32 and 128 rows at --pos with the slots attached to one P-position "
                         "prefix and with the slots forked at P, alternating")
    ap.add_argument("--pos", type=int, default=1024, help="the rows' position of --shared-prefix")
    ap.add_argument("--forked-only", action="store_true",
                    help="with --shared-prefix: only the forked figures, no prefix is ever set (what another build selected with LLMK_LIB "
                         "that has no llmk_prefix_* measures: the like-for-like baseline of the unshared path)")
    ap.add_argument("--kv", choices=["f32", "f16", "q8_0", "both", "all"], default=None,
                    help="only the K/V-type table: the pass at 8, 32 and 128 rows at positions 25 and --pos on batches with f32, f16 and / or "
                         "q8_0 K/V caches (both: f32 and f16; all: the three), alternating in one process; with --shared-prefix P also "
                         "attached behind P positions at --pos")
    ap.add_argument("--spans", action="store_true",
                    help="only the span tables (llmk_span_*): a 128-row span ending at --pos with and without bd_attn_span_kernel, a prompt "
                         "in spans against prefill + fork, 112 decode rows with and without a 16-row chunk")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()

    m, shape = build(a.shape, a.type, a.cls_q6k)
    if a.spans:
        r = spans(m, shape, a.pos, a.iters, a.repeats)
        m.close()
        print_spans(a.shape, a.type + ("+q6_K" if a.cls_q6k else ""), r, a.iters, a.repeats)
        if a.json:
            print(json.dumps({"shape": a.shape, "type": a.type + ("+q6_K" if a.cls_q6k else ""), "spans": r}))
        return
    if a.sampled:
        rows = sampled(m, shape, a.repeats)
        m.close()
        print_sampled(a.shape, a.type + ("+q6_K" if a.cls_q6k else ""), rows, a.repeats)
        if a.json:
            print(json.dumps({"shape": a.shape, "type": a.type + ("+q6_K" if a.cls_q6k else ""), "sampled": rows}))
        return
    if a.kv:
        kinds = {"both": ("f32", "f16"), "all": ("f32", "f16", "q8_0")}.get(a.kv, (a.kv,))
        rows = kv_types(m, shape, kinds, a.shared_prefix, a.pos, a.iters, a.repeats)
        m.close()
        print_kv(a.shape, a.type + ("+q6_K" if a.cls_q6k else ""), kinds, rows, a.iters, a.repeats)
        if a.json:
            print(json.dumps({"shape": a.shape, "type": a.type + ("+q6_K" if a.cls_q6k else ""), "kv": rows}))
        return
    if a.shared_prefix:
        rows = shared_prefix(m, shape, a.shared_prefix, a.pos, a.iters, a.repeats, a.forked_only)
        m.close()
        print_shared(a.shape, a.type + ("+q6_K" if a.cls_q6k else ""), rows, a.iters, a.repeats)
        if a.json:
            print(json.dumps({"shape": a.shape, "type": a.type + ("+q6_K" if a.cls_q6k else ""), "shared_prefix": rows}))
        return
    positions = [p for p in POSITIONS if p <= shape.seq_len]
    out = {"shape": a.shape, "type": a.type + ("+q6_K" if a.cls_q6k else ""), "path": m.path_name(), "batch": [], "decode_greedy": {}}

    # single stream first: llmk_decode_greedy, the library's fastest decode, at the positions the batch rows sit at
    for pos in positions:
        steps = min(a.decode_steps, shape.seq_len - pos + 1)
        rates = []
        for r in range(a.repeats + 1):
            m.reset()
            m.decode_greedy(2, max(1, pos - 8), 8)              # warm-up (the first call also captures the graphs)
            t0 = time.perf_counter()
            m.decode_greedy(2, pos, steps)
            dt = time.perf_counter() - t0
            if r:
                rates.append(steps / dt)
        med, spread = med_spread(rates)
        out["decode_greedy"][str(pos)] = {"tok_s": med, "spread": spread, "steps": steps}

    if a.single_only:
        positions_b = []
    else:
        positions_b = positions
    # one batch per position, its caches no longer than the position needs (128 slots x 1,024 positions of a 7B model are 137 GB of
    # f32 K/V rows); where even that does not fit beside the weights, the row counts that do
    for pos in positions_b:
        slots, b = max(ROWS), None
        while b is None:
            try:
                b = llmk.Batch(m, slots, pos)
            except llmk.LlmkError as e:
                if slots == 1:
                    raise
                print(f"# pos {pos}: no room for {slots} slots ({e}); trying {slots // 2}", file=sys.stderr)
                slots //= 2
        for n in ROWS:
            if n > slots:
                continue
            b.time(n, pos, 3)                                   # warm-up at this row count (its GEMM instantiation, its plan)
            ms = [b.time(n, pos, a.iters) for _ in range(a.repeats)]
            med, spread = med_spread(ms)
            out["batch"].append({"n": n, "pos": pos, "ms_per_pass": med, "spread": spread, "tok_s": n / med * 1e3})
        b.close()
    m.close()

    print(f"# library {llmk.LIB_PATH} (llmk_version {llmk.lib().llmk_version()})")
    print(f"# batched decode, {a.shape} {out['type']}: llmk_batch_time, median of {a.repeats} x {a.iters} passes (spread = (max - min) / median)")
    print(f"# single stream on the same context ({out['path']}): llmk_decode_greedy, median of {a.repeats} runs")
    for pos in positions:
        d = out["decode_greedy"][str(pos)]
        print(f"pos {pos:5d}   decode_greedy {d['tok_s']:10.1f} tok/s  (spread {d['spread']:.3f}, {d['steps']} positions, {1e3 / d['tok_s']:.3f} ms/token)")
        if not a.single_only:
            print(f"{'n':>5} {'ms/pass':>10} {'spread':>8} {'tok/s':>12} {'x single':>9}")
        for row in out["batch"]:
            if row["pos"] == pos:
                print(f"{row['n']:5d} {row['ms_per_pass']:10.3f} {row['spread']:8.3f} {row['tok_s']:12.1f} {row['tok_s'] / d['tok_s']:9.2f}")
    if a.json:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
