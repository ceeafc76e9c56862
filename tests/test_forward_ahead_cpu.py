"""The policy of llmk_forward's next-position launches (llm.f90_amd/csrc/forward_ahead.h) on the CPU: the header is compiled with
g++ into a stand-alone program whose main plays llmk.hip's part -- it asks the state machine what each scripted call does and
prints that -- and the transcripts are checked here.  No HIP, no GPU.

Script lines on stdin:   f POS AGREE DEVHIT   a call forward(tok, POS); AGREE: tok is the first maximum of the previous logits
                                              (asked for only when the machine scans), DEVHIT: tok is the id the device published
                                              (asked for only when the machine is armed for POS)
                         i                    another entry point settles the context
Output, one line per call:   plain | scan | arm N | hit N | miss      (N: the position launched behind this one, 0 = none)
and at the end:              stats LAUNCHES HITS MISSES SCANS ARMED
"""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "llm.f90_amd", "csrc")

MAIN = r"""
#include "forward_ahead.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "max")) {      // max V0 V1 ...: fa_first_max of the values
        std::vector<float> v;
        for (int i = 2; i < argc; ++i) v.push_back(strtof(argv[i], nullptr));
        printf("%d\n", llmk::fa_first_max(v.data(), (int)v.size()));
        return 0;
    }
    const int S = atoi(argv[1]);
    llmk::ForwardAhead fa;
    char op;
    while (scanf(" %c", &op) == 1) {
        if (op == 'i') { fa.interrupt(); continue; }
        int pos, agree, devhit;
        if (scanf("%d %d %d", &pos, &agree, &devhit) != 3) return 2;
        if (fa.armed) {
            if (fa.expects(pos) && devhit) {
                const bool more = fa.hit(S);
                printf("hit %d\n", more ? pos + 1 : 0);
                fa.ran(pos);
                continue;
            }
            fa.miss();
            printf("miss\n");
        } else if (fa.scan_due(pos)) {
            if (fa.scanned(agree != 0, pos, S)) {
                printf("arm %d\n", pos + 1);
                fa.ran(pos);
                continue;
            }
            printf("scan\n");
        } else {
            printf("plain\n");
        }
        fa.ran(pos);
    }
    printf("stats %d %d %d %d %d\n", fa.launches, fa.hits, fa.misses, fa.scans, fa.armed ? 1 : 0);
    return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("forward_ahead")
    src = d / "fa_main.cpp"
    src.write_text(MAIN)
    exe = d / "fa_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", HEADER_DIR, str(src), "-o", str(exe)], check=True)
    return str(exe)


def run(prog, S, calls):
    """calls: [(pos, agree, devhit) | "i"] -> (per-call lines, stats dict)"""
    text = "\n".join("i" if c == "i" else "f %d %d %d" % c for c in calls) + "\n"
    out = subprocess.run([prog, str(S)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    lines = [x for x in out if x]
    st = [int(x) for x in lines[-1].split()[1:]]
    return lines[:-1], dict(zip(("launches", "hits", "misses", "scans", "armed"), st))


def test_header_has_no_hip():
    """plain C++ that g++ compiles alone: the header includes nothing at all"""
    assert "#include" not in open(os.path.join(HEADER_DIR, "forward_ahead.h")).read()


def test_greedy_run_arms_on_third_call(prog):
    lines, st = run(prog, 64, [(p, 1, 1) for p in range(1, 11)])
    assert lines[:3] == ["plain", "scan", "arm 4"]
    assert lines[3:] == ["hit %d" % (p + 1) for p in range(4, 11)]
    assert st == {"launches": 8, "hits": 7, "misses": 0, "scans": 2, "armed": 1}


def test_position_S_launches_nothing_beyond(prog):
    S = 12
    lines, st = run(prog, S, [(p, 1, 1) for p in range(1, S + 1)])
    assert lines[-2:] == ["hit %d" % S, "hit 0"]
    launched = [int(x.split()[1]) for x in lines if x.split()[0] in ("arm", "hit")]
    assert max(launched) == S and st["armed"] == 0
    # a run whose streak completes AT position S has nothing to speculate on: it never arms
    lines, st = run(prog, 3, [(1, 1, 1), (2, 1, 1), (3, 1, 1)])
    assert lines == ["plain", "scan", "scan"] and st["launches"] == 0 and st["armed"] == 0


def test_miss_backs_off_and_doubles(prog):
    calls = [(1, 1, 1), (2, 1, 1), (3, 1, 1), (4, 1, 1), (5, 1, 0)]      # armed at 3, hit at 4, wrong token at 5
    calls += [(p, 1, 1) for p in range(6, 40)]
    lines, st = run(prog, 4096, calls)
    assert lines[:5] == ["plain", "scan", "arm 4", "hit 5", "miss"]
    assert lines[5:21] == ["plain"] * 16                                 # 16 sequential calls skip the comparison
    assert lines[21:23] == ["scan", "arm 24"]
    assert st["misses"] == 1
    # every further miss doubles the stretch without comparisons, up to 1,024
    calls, pos, expect = [], 1, []
    for k in range(9):
        n = min(16 << k, 1024)
        first = [(pos, 1, 1)] if k == 0 else []                          # (the very first call has nothing to compare with)
        calls += first + [(pos + len(first), 1, 1), (pos + len(first) + 1, 1, 1), (pos + len(first) + 2, 1, 0)]
        expect += ["plain"] * len(first) + ["scan", "arm %d" % (pos + len(first) + 2), "miss"]
        pos += len(first) + 3
        calls += [(pos + j, 1, 1) for j in range(n)]
        expect += ["plain"] * n
        pos += n
    lines, st = run(prog, 1 << 20, calls)
    assert lines == expect
    assert st["misses"] == 9


def test_non_sequential_position_is_a_miss(prog):
    lines, st = run(prog, 64, [(1, 1, 1), (2, 1, 1), (3, 1, 1), (7, 1, 1), (8, 1, 1)])
    assert lines == ["plain", "scan", "arm 4", "miss", "plain"]
    assert st["misses"] == 1 and st["armed"] == 0
    # ... and, idle, a jump breaks the streak: two agreements must be consecutive calls of one sequence
    lines, st = run(prog, 64, [(1, 1, 1), (2, 1, 1), (9, 1, 1), (10, 1, 1), (11, 1, 1)])
    assert lines == ["plain", "scan", "plain", "scan", "arm 12"]


def test_settling_goes_idle_without_a_miss(prog):
    lines, st = run(prog, 64, [(1, 1, 1), (2, 1, 1), (3, 1, 1), "i", (4, 1, 1), (5, 1, 1), (6, 1, 1)])
    assert lines == ["plain", "scan", "arm 4", "plain", "scan", "arm 7"]
    assert st["misses"] == 0


@pytest.mark.parametrize("N", [64, 1000, 1500])
def test_host_sampler_scans_a_handful_of_times(prog, N):
    """a caller that samples on the host agrees with the argmax 1 time in 1,000: at most ceil(log2(N / 16)) + 2 scans in N calls"""
    calls = [(p, 1 if p % 1000 == 19 else 0, 0) for p in range(1, N + 1)]      # (19: the second scan, so the agreement is SEEN)
    lines, st = run(prog, 1 << 20, calls)
    assert st["launches"] == 0 and st["hits"] == 0 and st["armed"] == 0
    assert st["scans"] <= math.ceil(math.log2(N / 16)) + 2
    assert lines.count("scan") == st["scans"] >= 2


def test_first_max_is_the_devices_rule(prog):
    def fm(*v):
        return int(subprocess.run([prog, "max"] + [str(x) for x in v], capture_output=True, text=True, check=True).stdout)
    assert fm(1, 3, 3, 2) == 1                      # the first maximum
    assert fm("nan", 1, "nan", 5, 5) == 3           # a NaN never wins
    assert fm("nan", "-inf") == -1                  # nothing greater than -inf: no token
    assert fm("-inf", -3.5, "inf") == 2
