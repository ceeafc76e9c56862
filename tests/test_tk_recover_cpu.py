"""The host's reaction to the persistent kernel's sticky error word (llm.f90_amd/csrc/tk_recover.h) on the CPU: the header is compiled
with g++ into a stand-alone program whose main plays llmk.hip's part -- it asks the policy what each scripted event means, does what
llmk.hip would do to the state (a RETIRE sets `retired`, a retired context launches no kernel) and prints the answers -- and the
transcripts are checked here.  The same program is built once more with -fsanitize=address,undefined.  No HIP, no GPU.

Script lines on stdin (W in hex):   s POS W            one launch, one sync at POS that left word W (token_pass)
                                    p POS0 N DONE W    N pipelined launches from POS0, DONE ids arrived, word W (decode_run)
                                    t W                a drained speculative launch left W (spec_settle)
                                    r | f              llmk_reset | a batched prefill or score (pf_run)
Output, one line per event (KEEP: the record tag kept in front of the launch, `-` = the records stay as they are):
    s KEEP VERDICT FIRST RUN RETIRED          FIRST: the context's first range event (the one-time message)
    p KEEP VERDICT KEEPTAG RESUME RUN RETIRED
    t VERDICT RETIRED
    s multi | p multi                         the context is retired: multi-kernel launches, no word to look at
`filter KEEP` as argv: records as 4 hex words each (x y z w bits) on stdin; prints CHANGED, then the records as they are left.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "llm.f90_amd", "csrc")

MAIN = r"""
#include "tk_recover.h"
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>
using namespace llmk;
static const char* name(TkVerdict v) {
    return v == TkVerdict::CLEAN ? "clean" : v == TkVerdict::NO_FINITE ? "nofinite" : v == TkVerdict::REDO ? "redo" : "retire";
}
static void tag(int keep) { if (keep == TK_KEEP_ALL) printf(" -"); else printf(" %d", keep); }
int main(int argc, char** argv) {
    if (argc > 2 && !strcmp(argv[1], "filter")) {
        std::vector<TkQscRecord> rec;
        unsigned w[4];
        while (scanf("%x %x %x %x", w, w + 1, w + 2, w + 3) == 4) {
            TkQscRecord r;
            memcpy(&r, w, sizeof(r));
            rec.push_back(r);
        }
        printf("%d\n", tk_qsc_filter(rec.data(), (int)rec.size(), atoi(argv[2])) ? 1 : 0);
        for (const TkQscRecord& r : rec) {
            memcpy(w, &r, sizeof(r));
            printf("%08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
        }
        return 0;
    }
    if (argc > 2 && !strcmp(argv[1], "words")) {      // words W: tk_range_only and the message's words
        const unsigned code = (unsigned)strtoul(argv[2], nullptr, 16);
        printf("%d %s\n", tk_range_only(code) ? 1 : 0, tk_err_words(code));
        return 0;
    }
    TkRecovery tk;
    char op;
    while (scanf(" %c", &op) == 1) {
        if (op == 'r' || op == 'f') { tk.cleared(); continue; }      // (llmk_reset clears the word too: nothing of the policy's)
        if (op == 't') {
            unsigned w;
            if (scanf("%x", &w) != 1) return 2;
            const TkVerdict v = TkRecovery::settled(w);
            if (v == TkVerdict::RETIRE) tk.retired = true;
            printf("t %s %d\n", name(v), tk.retired ? 1 : 0);
        } else if (op == 's') {
            int pos;
            unsigned w;
            if (scanf("%d %x", &pos, &w) != 2) return 2;
            if (tk.retired) { printf("s multi\n"); continue; }
            printf("s");
            tag(tk.before_launch(pos, true));
            const TkRecovery::Single v = tk.single(w);
            if (v.what == TkVerdict::RETIRE) tk.retired = true;
            printf(" %s %d %d %d\n", name(v.what), v.first_event ? 1 : 0, tk.range_run, tk.retired ? 1 : 0);
        } else if (op == 'p') {
            int pos0, n, done;
            unsigned w;
            if (scanf("%d %d %d %x", &pos0, &n, &done, &w) != 4) return 2;
            if (tk.retired) { printf("p multi\n"); continue; }
            printf("p");
            tag(tk.before_launch(pos0, true));
            const TkRecovery::Pipelined e = tk.pipelined_end(pos0, n, done, w);
            if (e.what == TkVerdict::RETIRE) tk.retired = true;
            printf(" %s", name(e.what));
            tag(e.keep);
            printf(" %d %d %d\n", e.resume, tk.range_run, tk.retired ? 1 : 0);
        } else {
            return 2;
        }
    }
    return 0;
}
"""

RANGE = 0x4000 | 0x1000 | 0x2b      # a range event as the host reads it: the cause with its epoch byte, drained
SPINS = (0x100 | 0x07, 0x200 | 0x03, 0x300 | 0x15, 0x400 | 0xfe)


def build(d, flags):
    src = d / "tk_main.cpp"
    src.write_text(MAIN)
    exe = d / ("tk_main" + "_san" * bool(flags))
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", HEADER_DIR, str(src), "-o", str(exe)] + flags, check=True)
    return str(exe)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return build(tmp_path_factory.mktemp("tk_recover"), [])


def script(events):
    return "\n".join(" ".join("%x" % a if i == len(e) - 1 and e[0] in "spt" else str(a) for i, a in enumerate(e)) for e in events) + "\n"


def run(prog, events):
    r = subprocess.run([prog], input=script(events), capture_output=True, text=True, check=True)
    assert r.stderr == ""
    return [x for x in r.stdout.split("\n") if x]


def rec_text(recs):
    return "\n".join("%08x %08x %08x %08x" % tuple(r) for r in recs) + "\n"


def run_filter(prog, keep, recs):
    r = subprocess.run([prog, "filter", str(keep)], input=rec_text(recs), capture_output=True, text=True, check=True)
    assert r.stderr == ""
    lines = r.stdout.split()
    out = [int(x, 16) for x in lines[1:]]
    return int(lines[0]), [tuple(out[i:i + 4]) for i in range(0, len(out), 4)]


def bits(f):
    import struct
    return struct.unpack("<I", struct.pack("<f", f))[0]


# ---- the scripts (name -> events), each with its transcript in the test of the same name; the sanitized build replays them all
SCRIPTS = {
    "clean_run": [("s", 1, 0), ("s", 2, 0), ("p", 3, 8, 8, 0), ("s", 11, 0), ("p", 12, 4, 4, 0), ("t", 0), ("s", 16, 0)],
    "four_in_a_row": [("s", p, 0) for p in (1, 2)] + [("s", p, RANGE) for p in (3, 4, 5, 6)] + [("s", 7, 0), ("p", 8, 4, 4, 0)],
    "clean_between": [("s", p, RANGE) for p in (1, 2, 3)] + [("s", 4, 0)] + [("s", p, RANGE) for p in (5, 6, 7)] + [("s", 8, 0)],
    "clean_call_between": [("s", p, RANGE) for p in (1, 2, 3)] + [("p", 4, 5, 5, 0)] + [("s", p, RANGE) for p in (9, 10, 11, 12)],
    "g7": [("s", 1, 0)] + [e for k in range(5) for e in (("p", 2 + 6 * k, 6, 3, RANGE), ("s", 5 + 6 * k, RANGE), ("s", 6 + 6 * k, 0),
                                                           ("s", 7 + 6 * k, 0))],
    "pipelined_done0": [("s", 1, 0), ("s", 2, RANGE), ("p", 3, 4, 0, RANGE), ("s", 3, RANGE), ("p", 4, 4, 0, RANGE), ("s", 4, RANGE)],
    "g5": [("s", 6, 0), ("s", 7, 0), ("s", 6, 0), ("s", 7, 0), ("s", 7, 0), ("s", 3, 0), ("s", 9, 0)],
    "after_reset": [("s", 4, 0), ("r",), ("s", 1, 0), ("s", 2, 0), ("r",), ("s", 5, 0), ("f",), ("s", 6, 0), ("p", 7, 3, 3, 0), ("s", 10, 0),
                    ("p", 11, 3, 3, 0), ("f",), ("p", 14, 2, 2, 0)],
    "reset_keeps_the_counts": [("s", 1, RANGE), ("s", 2, RANGE), ("r",), ("s", 1, RANGE), ("s", 2, RANGE)],
    "settle": [("t", 0x2000), ("t", 0x2000 | 0x1000), ("s", 1, 0), ("t", 0x300 | 0x1000), ("s", 2, 0)],
    "pipelined_timeout": [("p", 1, 8, 5, 0x100 | 0x1000 | 0x44), ("s", 6, 0), ("p", 7, 2, 2, 0)],
    "pipelined_ids_missing": [("p", 1, 8, 5, 0)],
}
SCRIPTS.update({"spin_%x" % w: [("s", 1, w | 0x1000)] for w in SPINS})
SCRIPTS.update({"spin_range_%x" % w: [("s", 1, w | 0x4000 | 0x1000)] for w in SPINS})
SCRIPTS.update({"spin_pipelined_%x" % w: [("p", 1, 4, 2, w | 0x4000)] for w in SPINS})
SCRIPTS.update({"spin_settle_%x" % w: [("t", w), ("t", w | 0x4000)] for w in SPINS})


def test_header_has_no_hip():
    """plain C++ that g++ compiles alone: the header includes nothing at all"""
    assert "#include" not in open(os.path.join(HEADER_DIR, "tk_recover.h")).read()


def test_clean_run(prog):
    """nothing is asked of the host, no record is touched, the count stays 0"""
    assert run(prog, SCRIPTS["clean_run"]) == ["s - clean 0 0 0", "s - clean 0 0 0", "p - clean - 11 0 0", "s - clean 0 0 0",
                                                "p - clean - 16 0 0", "t clean 0", "s - clean 0 0 0"]


def test_range_events_in_a_row(prog):
    """three single-pass range events in a row redo and keep the kernel, the fourth retires; the message once"""
    assert run(prog, SCRIPTS["four_in_a_row"]) == ["s - clean 0 0 0", "s - clean 0 0 0", "s - redo 1 1 0", "s - redo 0 2 0", "s - redo 0 3 0",
                                                    "s - retire 0 3 1", "s multi", "p multi"]
    # ... with a clean position between the third and the fourth: no retirement, and three more are borne
    out = run(prog, SCRIPTS["clean_between"])
    assert out == ["s - redo 1 1 0", "s - redo 0 2 0", "s - redo 0 3 0", "s - clean 0 0 0", "s - redo 0 1 0", "s - redo 0 2 0", "s - redo 0 3 0",
                   "s - clean 0 0 0"]
    # ... and so does the clean return of a pipelined call, whose positions ran clean; four in a row behind it retire
    out = run(prog, SCRIPTS["clean_call_between"])
    assert out == ["s - redo 1 1 0", "s - redo 0 2 0", "s - redo 0 3 0", "p - clean - 9 0 0", "s - redo 0 1 0", "s - redo 0 2 0", "s - redo 0 3 0",
                   "s - retire 0 3 1"]


def test_g7_pipelined_calls_that_each_end_on_an_event(prog):
    """five pipelined calls, each ending on a range event behind three clean positions, clean single positions between them: every
    call clears, keeps the last clean position's record and resumes behind it; the redone position counts 1; never retired"""
    out = run(prog, SCRIPTS["g7"])
    want = ["s - clean 0 0 0"]
    for k in range(5):
        p0 = 2 + 6 * k
        # (the single pass at p0 + 3 continues the remembered position p0 + 2: nothing more to drop)
        want += ["p - redo %d %d 0 0" % (p0 + 2, p0 + 3), "s - redo %d 1 0" % (k == 0), "s - clean 0 0 0", "s - clean 0 0 0"]
    assert out == want
    assert not any(l.endswith(" 1") for l in out)


def test_pipelined_call_with_no_id(prog):
    """done = 0: the count is NOT reset (the limit is not consulted at this site either), and nothing of the call's is worth
    keeping -- tag pos0 - 1"""
    assert run(prog, SCRIPTS["pipelined_done0"]) == ["s - clean 0 0 0", "s - redo 1 1 0", "p - redo 2 3 1 0", "s - redo 0 2 0",
                                                      "p - redo 3 4 2 0", "s - redo 0 3 0"]


def test_g5_a_launch_that_does_not_continue_the_one_before(prog):
    """p, p + 1, then p again: the second asks nothing, the third keeps only p - 1; the same position twice, a rewind, a jump"""
    assert run(prog, SCRIPTS["g5"]) == ["s 5 clean 0 0 0", "s - clean 0 0 0", "s 5 clean 0 0 0", "s - clean 0 0 0", "s 6 clean 0 0 0",
                                         "s 2 clean 0 0 0", "s 8 clean 0 0 0"]


def test_after_a_reset_or_a_prefill(prog):
    """a launch at 1 behind a reset keeps nothing; a launch at 5 behind one keeps tag 4 (the records are empty: the filter then
    changes nothing); the clean return of a pipelined call remembers its last position"""
    assert run(prog, SCRIPTS["after_reset"]) == ["s 3 clean 0 0 0", "s - clean 0 0 0", "s - clean 0 0 0", "s 4 clean 0 0 0", "s 5 clean 0 0 0",
                                                  "p - clean - 10 0 0", "s - clean 0 0 0", "p - clean - 14 0 0", "p 13 clean - 16 0 0"]


def test_reset_touches_neither_count(prog):
    """llmk_reset starts a new sequence on the same model: the run goes on (and the message is not printed again)"""
    assert run(prog, SCRIPTS["reset_keeps_the_counts"]) == ["s - redo 1 1 0", "s - redo 0 2 0", "s - redo 0 3 0", "s - retire 0 3 1"]


@pytest.mark.parametrize("w", SPINS)
def test_every_spin_timeout_class_retires(prog, w):
    """alone and together with a range event, at each of the three sites"""
    assert run(prog, SCRIPTS["spin_%x" % w]) == ["s - retire 0 0 1"]
    assert run(prog, SCRIPTS["spin_range_%x" % w]) == ["s - retire 0 0 1"]
    assert run(prog, SCRIPTS["spin_pipelined_%x" % w]) == ["p - retire - 3 0 1"]
    assert run(prog, SCRIPTS["spin_settle_%x" % w]) == ["t retire 1", "t retire 1"]


def test_settle_and_the_pipelined_retirements(prog):
    """no finite candidate at a settle clears and retires nothing; a timeout there retires; a pipelined call that ends on a timeout,
    or without its ids and without a word, retires and resumes at the first position whose id never arrived"""
    assert run(prog, SCRIPTS["settle"]) == ["t nofinite 0", "t nofinite 0", "s - clean 0 0 0", "t retire 1", "s multi"]
    assert run(prog, SCRIPTS["pipelined_timeout"]) == ["p - retire - 6 0 1", "s multi", "p multi"]
    assert run(prog, SCRIPTS["pipelined_ids_missing"]) == ["p - retire - 6 0 1"]


def test_the_words(prog):
    def words(code):
        out = subprocess.run([prog, "words", "%x" % code], capture_output=True, text=True, check=True).stdout.rstrip("\n")
        return int(out[0]), out[2:]
    timeout = "timed out waiting for its peer workgroups"
    rng = "met an activation beyond the f16 range of its matrix-core operands"
    assert words(0x4000 | 0x1000) == (1, rng) and words(0x4000 | 0x7f) == (1, rng) and words(RANGE) == (1, rng)
    assert words(0x2000) == (0, "found no finite logit among its candidates")
    assert words(0x4000 | 0x2000) == (0, "found no finite logit among its candidates")
    assert words(0x1000) == (0, timeout) and words(0) == (0, timeout)
    for w in SPINS:
        assert words(w) == (0, timeout) and words(w | 0x1000) == (0, timeout) and words(w | 0x4000 | 0x1000) == (0, rng)


# ---- the record filter
ONE, NAN, NEG0 = bits(1.0), 0x7fc12345, 0x80000000
RECORDS = [
    (bits(2.5), bits(7.25), 6, 6),          # both fields of the kept position
    (bits(2.5), bits(7.25), 5, 7),          # neither
    (bits(3.0), bits(4.0), 6, 7),           # x kept, y dropped
    (bits(3.0), bits(4.0), 9, 6),           # y kept, x dropped
    (0, 0, 0, 0),                           # empty: untouched, and no change
    (NAN, bits(float("inf")), 6, 6),        # kept bit for bit, whatever the value
    (0, bits(1e-30), 0, 0),                 # a value without a tag is not empty
    (0, 0, 8, 0),                           # nor is a tag without a value
    (NEG0, ONE, 0, 6),                      # -0.0 is a zero value: empty
]


def test_record_filter(prog):
    changed, out = run_filter(prog, 6, RECORDS)
    assert changed == 1
    assert out == [RECORDS[0], (0, 0, 0, 0), (bits(3.0), 0, 6, 0), (0, bits(4.0), 0, 6), (0, 0, 0, 0), RECORDS[5], (0, 0, 0, 0), (0, 0, 0, 0),
                   RECORDS[8]]
    # nothing but kept and empty fields: no change, so no copy back
    quiet = [RECORDS[0], RECORDS[4], RECORDS[5], RECORDS[8], (0, ONE, 0, 6), (ONE, 0, 6, 0)]
    assert run_filter(prog, 6, quiet) == (0, quiet)
    # keep = 0 (a launch at position 1 that continues nothing): untagged fields are tag 0's
    assert run_filter(prog, 0, [(ONE, ONE, 0, 3)]) == (1, [(ONE, 0, 0, 0)])
    # a record whose fields carry different tags loses exactly one of them, either one
    assert run_filter(prog, 7, [RECORDS[2]]) == (1, [(0, bits(4.0), 0, 7)])
    assert run_filter(prog, 4, []) == (0, [])


def test_sanitized_build_replays_every_script(prog, tmp_path):
    """a stand-alone host program: address and undefined-behaviour sanitizers linked in, no preloading"""
    san = build(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    for name, events in SCRIPTS.items():
        assert run(san, events) == run(prog, events), name
    assert run_filter(san, 6, RECORDS) == run_filter(prog, 6, RECORDS)
    full = [(bits(1.0 + i), bits(2.0 + i), i % 7, i % 5) for i in range(256)]      # both buffers of 128 records
    assert run_filter(san, 3, full) == run_filter(prog, 3, full)
