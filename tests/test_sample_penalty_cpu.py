"""The penalty rule (llm.f90_amd/csrc/sample_penalty.h: logit bias, then repetition / frequency / presence penalties over a window of
the token record, in front of the truncated sampler) on the host: the header compiled into a stand-alone program against the tests'
numpy float32 restatement (tests/penalty_ref.py), bit for bit, and the rule's properties.  No device needed."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import filter_ref
import penalty_ref
import sample_ref
from conftest import ROOT

CSRC = os.path.join(ROOT, "llm.f90_amd", "csrc")
PROGRAM = r'''
#include "sample_filter.h"
#include "sample_penalty.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
// input file: cases of { int32 V, pos, last_n, n_bias, top_k; float r, inv_r, f, p, invT, top_p, min_p; uint64 seed;
//                        {int32 token; float bias}[n_bias]; int32 hist[pos]; float z[V] }
// output file: per case { int32 token, kept; uint32 tau bits; float adjusted[V] }
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    int32_t h[5];
    while (fread(h, 4, 5, f) == 5) {
        float q[7];
        uint64_t seed;
        if (fread(q, 4, 7, f) != 7 || fread(&seed, 8, 1, f) != 1) return 3;
        const int V = h[0], pos = h[1];
        if (h[3] < 0 || h[3] > LLMK_PENALTY_MAX_BIAS) return 4;
        llmk_penalty_params pp;
        memset(&pp, 0, sizeof(pp));
        pp.repeat = q[0]; pp.inv_repeat = q[1]; pp.frequency = q[2]; pp.presence = q[3];
        pp.last_n = h[2]; pp.n_bias = h[3];
        if (h[3] && fread(pp.bias, sizeof(llmk_penalty_bias), (size_t)h[3], f) != (size_t)h[3]) return 3;
        std::vector<int> hist((size_t)pos), cnt((size_t)V, 0);
        std::vector<float> z((size_t)V);
        if (fread(hist.data(), 4, hist.size(), f) != hist.size() || fread(z.data(), 4, z.size(), f) != z.size()) return 3;
        llmk_penalty_rule(z.data(), V, &pp, hist.data(), pos, cnt.data());
        for (int i = 0; i < V; ++i)
            if (cnt[(size_t)i] != 0) return 5;                 // the rule leaves its scratch counts zero
        llmk_filter_params p;
        memset(&p, 0, sizeof(p));
        p.invT = q[4]; p.top_p = q[5]; p.min_p = q[6]; p.top_k = h[4];
        p.seed_lo = (uint32_t)seed; p.seed_hi = (uint32_t)(seed >> 32);
        int32_t out[3];
        float tau;
        int kept;
        out[0] = llmk_filter_rule(z.data(), V, &p, pos, &kept, &tau);
        out[1] = kept;
        memcpy(&out[2], &tau, 4);
        if (fwrite(out, 4, 3, o) != 3 || fwrite(z.data(), 4, z.size(), o) != z.size()) return 6;
    }
    fclose(f);
    fclose(o);
    return 0;
}
'''


@pytest.fixture(scope="module")
def host_prog(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        cxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    d = tmp_path_factory.mktemp("sample_penalty")
    src, exe = str(d / "penalty_host.cpp"), str(d / "penalty_host")
    with open(src, "w") as f:
        f.write(PROGRAM)
    base = [cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, src, "-o", exe]
    # stand-alone host code: the one place a sanitizer belongs; a toolchain without its runtime builds the plain program
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe, str(d)


def run_header(host_prog, cases):
    """[(token, kept, tau, adjusted)] of llmk_penalty_rule + llmk_filter_rule for penalty_ref.cases()-style dicts"""
    exe, d = host_prog
    path, out = os.path.join(d, "cases.bin"), os.path.join(d, "out.bin")
    with open(path, "wb") as f:
        for c in cases:
            z = np.ascontiguousarray(c["z"], np.float32)
            hist = np.ascontiguousarray(c["hist"], np.int32)
            assert hist.size == c["pos"]
            f.write(struct.pack("<iiiiifffffffQ", z.size, c["pos"], c["last_n"], len(c["bias"]), c["top_k"], c["repeat"],
                                float(penalty_ref.inv_repeat(c["repeat"])), c["frequency"], c["presence"],
                                float(sample_ref.inv_temperature(c["T"])), c["top_p"], c["min_p"], c["seed"]))
            for t, b in c["bias"]:
                f.write(struct.pack("<if", t, b))
            f.write(hist.tobytes())
            f.write(z.tobytes())
    r = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(out, "rb").read()
    res, at = [], 0
    for c in cases:
        V = np.asarray(c["z"]).size
        tok, kept = struct.unpack_from("<ii", raw, at)
        tau = np.frombuffer(raw, np.float32, 1, at + 8)[0]
        res.append((tok, kept, tau, np.frombuffer(raw, np.float32, V, at + 12).copy()))
        at += 12 + 4 * V
    assert at == len(raw)
    return res


@pytest.fixture(scope="module")
def all_cases():
    return penalty_ref.cases((300, 1024))


@pytest.fixture(scope="module")
def header_out(host_prog, all_cases):
    return run_header(host_prog, all_cases)


def test_cases_cover_what_they_should(all_cases):
    names = " ".join(c["name"] for c in all_cases)
    for w in ("empty", "one", "identical", "thrice", "with-none", "pos-below-last_n", "special-rows", "long"):
        assert f"-{w}-" in names
    c = next(c for c in all_cases if "-identical-" in c["name"])
    assert len(penalty_ref.window(c["hist"], c["pos"], c["last_n"])) == c["last_n"] and len(set(c["hist"].tolist())) == 1
    c = next(c for c in all_cases if "-thrice-" in c["name"])
    assert np.unique(penalty_ref.window(c["hist"], c["pos"], c["last_n"]), return_counts=True)[1].max() == 3
    c = next(c for c in all_cases if "-with-none-" in c["name"])
    assert (c["hist"][c["pos"] - c["last_n"]:c["pos"]] == 0).any()
    assert any(c["pos"] < c["last_n"] for c in all_cases)
    assert any(len(c["bias"]) == penalty_ref.MAX_LOGIT_BIAS for c in all_cases)
    assert any(c["last_n"] > penalty_ref.THREADS and c["pos"] > penalty_ref.THREADS for c in all_cases)
    # the window rows' logits: +0.0, -0.0, negative, -inf and NaN all occur
    seen = set()
    for c in all_cases:
        rows = c["z"][penalty_ref.window(c["hist"], c["pos"], c["last_n"]) - 1]
        sign = np.signbit(rows)
        seen |= {k for k, m in (("+0", (rows == 0) & ~sign), ("-0", (rows == 0) & sign), ("neg", rows < 0), ("-inf", np.isneginf(rows)),
                                ("nan", np.isnan(rows))) if m.any()}
    assert seen == {"+0", "-0", "neg", "-inf", "nan"}
    # a bias on a row that is also in the window; -inf on the maximum
    assert any(set(t for t, _ in c["bias"]) & set(penalty_ref.window(c["hist"], c["pos"], c["last_n"]).tolist()) for c in all_cases)
    for c in all_cases:
        if c["banned"]:
            assert c["z"][c["banned"][0] - 1] == np.nanmax(c["z"])


def test_adjusted_logits_equal_the_float32_rule_bit_for_bit(all_cases, header_out):
    for c, (tok, kept, tau, adj) in zip(all_cases, header_out):
        want = penalty_ref.adjust(c["z"], c["hist"], c["pos"], **penalty_ref.pen_args(c))
        assert penalty_ref.same_bits(adj, want), (c["name"], np.flatnonzero(adj.view(np.uint32) != want.view(np.uint32))[:8])
        untouched = np.ones(adj.size, bool)
        untouched[[t - 1 for t, _ in c["bias"]]] = False
        untouched[penalty_ref.window(c["hist"], c["pos"], c["last_n"]) - 1] = False
        assert penalty_ref.same_bits(adj[untouched], np.asarray(c["z"], np.float32)[untouched]), c["name"]


def test_picks_are_the_filter_rule_on_the_adjusted_logits(all_cases, header_out):
    """step 3: kept, tau and the pick as tests/test_sample_filter_cpu.py compares them; filter_ref alone must call all but
    len(cases) // 50 of the chosen vectors safe, near-ties of the score included (the cap of the GPU test)"""
    uncompared = 0
    for c, (tok, kept, tau, adj) in zip(all_cases, header_out):
        want, margin, r, _ = penalty_ref.sample(c["z"], c["hist"], c["pos"], c["T"], c["seed"], c["top_k"], c["top_p"], c["min_p"],
                                                **penalty_ref.pen_args(c))
        if not r.safe:
            uncompared += 1
            continue
        assert kept == r.kept, (c["name"], kept, r.kept)
        assert np.float32(tau) == r.tau, (c["name"], tau, r.tau)
        if r.kept == 0:
            assert tok == 0, c["name"]
            continue
        if margin > 1e-5:
            assert tok == want, (c["name"], tok, want, margin)
        else:
            uncompared += 1
        assert r.mask[tok - 1], c["name"]
    assert uncompared <= len(all_cases) // 50, (uncompared, len(all_cases))
    for V in (300, 1024):                                       # ... and per vocabulary size, as the GPU test runs them
        sub = [c for c in all_cases if c["z"].size == V]
        n = 0
        for c in sub:
            _, margin, r, _ = penalty_ref.sample(c["z"], c["hist"], c["pos"], c["T"], c["seed"], c["top_k"], c["top_p"], c["min_p"],
                                                 **penalty_ref.pen_args(c))
            n += not (r.safe and margin > 1e-5)
        assert n <= len(sub) // 50, (V, n, len(sub))


def test_repeat_above_one_never_raises_a_windowed_row(all_cases, header_out):
    n = 0
    for c, (tok, kept, tau, adj) in zip(all_cases, header_out):
        if not (c["repeat"] > 1 and c["frequency"] >= 0 and c["presence"] >= 0):
            continue
        biased = penalty_ref.adjust(c["z"], c["hist"], c["pos"], bias=c["bias"])
        rows = np.unique(penalty_ref.window(c["hist"], c["pos"], c["last_n"])) - 1
        ok = ~np.isnan(biased[rows])
        assert (adj[rows][ok] <= biased[rows][ok]).all(), c["name"]
        n += rows.size
    assert n > 1000


def test_a_banned_row_is_never_picked(all_cases, header_out):
    n = 0
    for c, (tok, kept, tau, adj) in zip(all_cases, header_out):
        for t in c["banned"]:
            assert adj[t - 1] == -np.inf or np.isnan(adj[t - 1]), c["name"]
            assert tok != t, c["name"]
            n += 1
    assert n >= 40


def test_neutral_parameters_return_the_input_bits(host_prog, all_cases):
    neutral = [dict(c, repeat=1.0, frequency=0.0, presence=0.0, bias=[], banned=[]) for c in all_cases]
    neutral += [dict(c, last_n=0, bias=[], banned=[]) for c in all_cases[::7]]
    for c, (tok, kept, tau, adj) in zip(neutral, run_header(host_prog, neutral)):
        assert penalty_ref.same_bits(adj, c["z"]), c["name"]
        want, margin, r = filter_ref.sample(c["z"], c["T"], c["seed"], c["pos"], c["top_k"], c["top_p"], c["min_p"])
        if r.safe and margin > 1e-5:
            assert tok == want, c["name"]


def test_penalty_kernel_has_no_scratch(tmp_path):
    """sample_penalty_kernel compiled for gfx950: 0 bytes of scratch, no spills, no LDS"""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    src = tmp_path / "k.hip"
    src.write_text('#include "kernels.h"\n')
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", "-I", CSRC, str(src), "-o", str(tmp_path / "k.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = r.stderr.split("Function Name: ")
    mine = [b for b in blocks if "sample_penalty_kernel" in b.split("\n")[0]]
    assert len(mine) == 1
    get = lambda key: int(re.search(re.escape(key) + r":\s+(\d+)", mine[0]).group(1))
    assert get("ScratchSize [bytes/lane]") == 0
    assert get("SGPRs Spill") == 0 and get("VGPRs Spill") == 0
    assert get("LDS Size [bytes/block]") == 0
