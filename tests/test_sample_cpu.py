"""The device sampler's arithmetic (llm.f90_amd/csrc/sample.h) on the host: Philox4x32-10 against the Random123
known answers, and the tests' numpy restatement of the whole rule (tests/sample_ref.py) against the header compiled
into a host program -- w and u bit for bit, g within a few ulp.  No device needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sample_ref
from conftest import ROOT

CSRC = os.path.join(ROOT, "llm.f90_amd", "csrc")
PROGRAM = r'''
#include "sample.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "philox")) {      // ctr0..3 key0..1 per line (hex) -> the 4 output words
        unsigned c[6];
        while (scanf("%x %x %x %x %x %x", &c[0], &c[1], &c[2], &c[3], &c[4], &c[5]) == 6) {
            const llmk_u32x4 o = llmk_philox4x32_10(c[0], c[1], c[2], c[3], c[4], c[5]);
            printf("%08x %08x %08x %08x\n", o.v[0], o.v[1], o.v[2], o.v[3]);
        }
        return 0;
    }
    unsigned long long seed;                           // seed pos i per line -> w, u bits, g bits, score bits of logit 1.5, invT 1.25
    int pos, i;
    while (scanf("%llu %d %d", &seed, &pos, &i) == 3) {
        const uint32_t w = llmk_sample_bits(seed, pos, i);
        const float u = llmk_sample_u(w), g = llmk_sample_gumbel(w), s = llmk_sample_score(1.5f, 1.25f, seed, pos, i);
        uint32_t ub, gb, sb;
        memcpy(&ub, &u, 4); memcpy(&gb, &g, 4); memcpy(&sb, &s, 4);
        printf("%u %u %u %u\n", w, ub, gb, sb);
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def host_prog(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        cxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    d = tmp_path_factory.mktemp("sample")
    src, exe = str(d / "sample_host.cpp"), str(d / "sample_host")
    with open(src, "w") as f:
        f.write(PROGRAM)
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(exe, args, text):
    r = subprocess.run([exe] + args, input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return r.stdout.split("\n")


KAT = [  # Random123's kat_vectors for philox4x32_10: counter, key -> output
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def test_philox_known_answers(host_prog):
    out = _run(host_prog, ["philox"], "".join(f"{c} {k}\n" for c, k, _ in KAT))
    for (_, _, want), got in zip(KAT, out):
        assert got == want
    for c, k, want in KAT:                                 # the numpy restatement agrees
        ctr = [np.uint32(int(x, 16)) for x in c.split()]
        key = [np.uint32(int(x, 16)) for x in k.split()]
        got = " ".join(f"{int(x):08x}" for x in sample_ref.philox4x32_10(ctr, key))
        assert got == want


def test_numpy_rule_matches_the_header(host_prog):
    rng = np.random.default_rng(20261016)
    n = 4000
    seeds = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    seeds[:8] = [0, 1, 7, 0xFFFFFFFF, 1 << 32, (1 << 32) + 5, 2 ** 64 - 1, 0xDEADBEEFCAFEF00D]
    pos = rng.integers(1, 4097, n)
    idx = rng.integers(0, 128256, n)
    idx[:4] = [0, 1, 2, 3]
    out = _run(host_prog, [], "".join(f"{int(s)} {int(p)} {int(i)}\n" for s, p, i in zip(seeds, pos, idx)))
    got = np.array([[int(v) for v in l.split()] for l in out if l], np.uint64)
    assert got.shape == (n, 4)
    w = np.array([sample_ref.bits(int(s), int(p), int(i)) for s, p, i in zip(seeds, pos, idx)], np.uint32)
    assert np.array_equal(got[:, 0].astype(np.uint32), w)
    u = sample_ref.uniform(w)
    assert np.array_equal(got[:, 1].astype(np.uint32), u.view(np.uint32))
    assert (u > 0).all() and (u < 1).all()
    g = sample_ref.gumbel(w)
    g_host = got[:, 2].astype(np.uint32).view(np.float32)
    ulp = np.spacing(np.maximum(np.abs(g), np.float32(1))).astype(np.float64)   # (near g = 0 the outer log amplifies the inner one's rounding)
    assert (np.abs(g_host.astype(np.float64) - g) <= 4 * ulp).all()
    s = (np.float32(1.5) * np.float32(1.25) + g_host).astype(np.float32)   # the score: product, then sum, each rounded
    assert np.array_equal(got[:, 3].astype(np.uint32), s.view(np.uint32))


def test_numpy_rule_draws_softmax():
    """The Gumbel-max rule on the host: frequencies over many seeds follow softmax(logits / T)."""
    logits = np.array([1.0, 0.5, 0.0, -1.0, 2.0, 0.25], np.float32)
    T = 0.8
    n = 20000
    counts = np.zeros(logits.size)
    for seed in range(n):
        tok, _ = sample_ref.sample(logits, T, seed, 3)
        counts[tok - 1] += 1
    p = np.exp(logits / T - np.max(logits / T))
    p /= p.sum()
    assert np.all(np.abs(counts / n - p) < 5 * np.sqrt(p * (1 - p) / n) + 1e-3)
