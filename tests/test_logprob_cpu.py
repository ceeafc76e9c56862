"""The decode log-probs rule (llm.f90_amd/csrc/logprob.h) on the host: llmk_logprob_rule, the serial statement of what
sample_logprob_kernel computes, compiled into a host program and held against the float64 restatement of tests/logprob_ref.py --
ids and padding exactly, values within the bar 2^-20 * max(1, |L|, max finite |z|).  No device needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import logprob_ref
from conftest import ROOT, load_golden

CSRC = os.path.join(ROOT, "llm.f90_amd", "csrc")
# per case: "V token top_n" then V f32 bit patterns (hex).  Output per case: listed, the bits of token_logprob, then top_n pairs
# "id bits"
PROGRAM = r'''
#include "logprob.h"
#include <stdio.h>
#include <string.h>
#include <vector>
int main() {
    int V, token, top_n;
    while (scanf("%d %d %d", &V, &token, &top_n) == 3) {
        std::vector<float> z(V);
        for (int i = 0; i < V; ++i) { unsigned b; if (scanf("%x", &b) != 1) return 1; memcpy(&z[i], &b, 4); }
        float tlp = 0.f, vals[LLMK_LOGPROB_MAX_TOP];
        int32_t toks[LLMK_LOGPROB_MAX_TOP];
        const int listed = llmk_logprob_rule(z.data(), V, token, top_n, &tlp, toks, vals);
        uint32_t b;
        memcpy(&b, &tlp, 4);
        printf("%d %08x", listed, b);
        for (int j = 0; j < top_n; ++j) { memcpy(&b, &vals[j], 4); printf(" %d %08x", toks[j], b); }
        printf("\n");
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def host_prog(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        cxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    d = tmp_path_factory.mktemp("logprob")
    src, exe = str(d / "logprob_host.cpp"), str(d / "logprob_host")
    with open(src, "w") as f:
        f.write(PROGRAM)
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(exe, cases):
    """cases: [(logits, token, top_n)] -> [(listed, token_logprob, top_tokens, top_logprobs)]"""
    text = "".join(f"{len(z)} {tok} {n} " + " ".join(f"{int(b):x}" for b in np.asarray(z, np.float32).view(np.uint32)) + "\n" for z, tok, n in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [l.split() for l in r.stdout.split("\n") if l]
    assert len(lines) == len(cases)
    out = []
    for l, (_, _, n) in zip(lines, cases):
        f = lambda h: np.array([int(h, 16)], np.uint32).view(np.float32)[0]
        out.append((int(l[0]), f(l[1]), np.array([int(v) for v in l[2::2]], np.int32), np.array([f(v) for v in l[3::2]], np.float32)))
        assert len(out[-1][2]) == n
    return out


def test_rule_matches_float64_on_the_vectors(host_prog):
    worst = 0.0
    for V in (33, 300, 1024, 4099, 32000):
        cases, names = [], []
        for name, z, tok in logprob_ref.vectors(V):
            for n in (0, 1, 20):
                cases.append((z, tok, n))
                names.append(f"{name}-V{V}-n{n}")
        for name, (z, tok, n), (listed, tlp, toks, vals) in zip(names, cases, _run(host_prog, cases)):
            worst = max(worst, logprob_ref.check(name, z, tok, n, tlp, toks, vals))
            assert listed == int((toks > 0).sum()) == min(n, int((np.asarray(z) > -np.inf).sum())), name
    print(f"largest error: {worst:.4f} of the bar (2^-20 of the scale)")


def test_rule_on_golden_rows(host_prog):
    """rows of two real-reference goldens, the token each position's argmax"""
    worst = 0.0
    for tag in ("tiny-gqa", "tk-small"):
        lg = load_golden(tag)["logits"]
        cases = [(z, int(np.argmax(z)) + 1, 20) for z in lg[:16]]
        for i, ((z, tok, n), (listed, tlp, toks, vals)) in enumerate(zip(cases, _run(host_prog, cases))):
            worst = max(worst, logprob_ref.check(f"{tag}-{i}", z, tok, n, tlp, toks, vals))
            assert toks[0] == tok and tlp == vals[0]             # the first alternative of a greedy position IS its token
            assert np.all(np.diff(vals) <= 0)
    print(f"largest error: {worst:.4f} of the bar")


def test_order_and_padding_by_hand(host_prog):
    ninf, nan = -np.inf, np.nan
    z = np.array([1.0, nan, 3.0, -0.0, ninf, 3.0, 0.0, np.float32(1e-45)], np.float32)
    (listed, tlp, toks, vals), = _run(host_prog, [(z, 3, 8)])
    assert listed == 6 and toks.tolist() == [3, 6, 1, 8, 4, 7, 0, 0]      # 3.0 twice by index; the denormal above the zeros; -0.0 before +0.0 by index
    assert np.all(vals[6:] == ninf)      # (a NaN row never reaches the ids; what it does to L is score.h's business)
    z = np.array([ninf, 2.0, ninf, 1.0], np.float32)
    (listed, tlp, toks, vals), = _run(host_prog, [(z, 4, 3)])
    L = np.log(np.exp(2.0) + np.exp(1.0))
    assert listed == 2 and toks.tolist() == [2, 4, 0] and vals[2] == ninf
    assert abs(tlp - (1.0 - L)) < 1e-6 and abs(vals[0] - (2.0 - L)) < 1e-6 and tlp == vals[1]
    (listed, tlp, toks, vals), = _run(host_prog, [(z, 0, 0)])
    assert listed == 0 and tlp == 0.0 and len(toks) == 0


def test_what_a_nan_row_does_to_the_values(host_prog):
    """score.h's empty state drops a NaN it meets first, so in the kernel's order (thread t steps rows t, t + 1024, ...) a NaN row
    reaches L only behind another row of its thread: at V <= 1,024 never -- the values are those of the vector without its NaN rows
    -- and at V = 32,000, with a tenth of the rows NaN, always"""
    for V in (300, 1024):
        for name, z, tok in logprob_ref.vectors(V):
            if not np.isnan(z).any():
                continue
            clean = np.where(np.isnan(z), -np.inf, z).astype(np.float32)
            (listed, tlp, toks, vals), = _run(host_prog, [(z, tok, 20)])
            assert np.isfinite(tlp) and np.isfinite(vals).all(), name
            logprob_ref.check(name, clean, tok, 20, tlp, toks, vals)
    seen = 0
    for name, z, tok in logprob_ref.vectors(32000):
        if np.isnan(z).any():
            (listed, tlp, toks, vals), = _run(host_prog, [(z, tok, 20)])
            assert np.isnan(tlp) and np.isnan(vals).all() and (toks > 0).all(), name
            seen += 1
    assert seen == 2


def test_logprob_ref_restates_the_definition():
    z = np.array([0.0, 1.0, 2.0, 2.0, -np.inf], np.float32)
    tlp, toks, vals, L = logprob_ref.rule(z, 2, 6)
    assert toks.tolist() == [3, 4, 2, 1, 0, 0] and np.all(vals[4:] == -np.inf)
    assert abs(L - np.log(np.exp(0) + np.exp(1) + 2 * np.exp(2))) < 1e-12 and abs(tlp - (1.0 - L)) < 1e-12 and tlp == vals[2]
    assert abs(np.exp(vals[:4]).sum() - 1.0) < 1e-12
    assert logprob_ref.rule(z, 0, 0)[0] == 0.0
