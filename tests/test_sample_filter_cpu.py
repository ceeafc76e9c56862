"""The truncated sampler's rule (llm.f90_amd/csrc/sample_filter.h: top-k, top-p, min-p in front of the Gumbel-max draw) on the host:
the header compiled into a stand-alone program against the tests' numpy float64 restatement (tests/filter_ref.py: sort and
cumulative sum) on seeded logit vectors, and the rule's properties.  No device needed."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import filter_ref
import sample_ref
from conftest import ROOT

CSRC = os.path.join(ROOT, "llm.f90_amd", "csrc")
PROGRAM = r'''
#include "sample_filter.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
// input file: cases of { int32 V, pos, top_k; float invT, top_p, min_p; uint64 seed; float z[V] } -> "token kept tau-bits" per case
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[3];
    while (fread(h, 4, 3, f) == 3) {
        float q[3];
        uint64_t seed;
        if (fread(q, 4, 3, f) != 3 || fread(&seed, 8, 1, f) != 1) return 3;
        std::vector<float> z((size_t)h[0]);
        if (fread(z.data(), 4, z.size(), f) != z.size()) return 3;
        llmk_filter_params p;
        memset(&p, 0, sizeof(p));
        p.invT = q[0]; p.top_p = q[1]; p.min_p = q[2]; p.top_k = h[2];
        p.seed_lo = (uint32_t)seed; p.seed_hi = (uint32_t)(seed >> 32);
        int kept;
        float tau;
        const int tok = llmk_filter_rule(z.data(), h[0], &p, h[1], &kept, &tau);
        uint32_t tb;
        memcpy(&tb, &tau, 4);
        printf("%d %d %u\n", tok, kept, tb);
    }
    fclose(f);
    return 0;
}
'''


@pytest.fixture(scope="module")
def host_prog(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        cxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    d = tmp_path_factory.mktemp("sample_filter")
    src, exe = str(d / "filter_host.cpp"), str(d / "filter_host")
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
    """[(token, kept, tau)] of the header's llmk_filter_rule for filter_ref.cases()-style dicts"""
    exe, d = host_prog
    path = os.path.join(d, "cases.bin")
    with open(path, "wb") as f:
        for c in cases:
            z = np.ascontiguousarray(c["z"], np.float32)
            f.write(struct.pack("<iiifffQ", z.size, c["pos"], c["top_k"], float(sample_ref.inv_temperature(c["T"])), c["top_p"], c["min_p"],
                                c["seed"]))
            f.write(z.tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [l.split() for l in r.stdout.split("\n") if l]
    assert len(rows) == len(cases)
    return [(int(t), int(k), np.array([int(b)], np.uint32).view(np.float32)[0]) for t, k, b in rows]


@pytest.fixture(scope="module")
def all_cases():
    return filter_ref.cases((37, 300, 1000, 32000))


@pytest.fixture(scope="module")
def header_out(host_prog, all_cases):
    return run_header(host_prog, all_cases)


def test_header_agrees_with_the_float64_rule(all_cases, header_out):
    """kept set (= kept count and tau) on every safe vector, the pick wherever the top two scores among the kept rows are no
    near-tie; at most 1 vector in 50 may be unsafe."""
    unsafe = 0
    for c, (tok, kept, tau) in zip(all_cases, header_out):
        want, margin, r = filter_ref.sample(c["z"], c["T"], c["seed"], c["pos"], c["top_k"], c["top_p"], c["min_p"])
        if not r.safe:
            unsafe += 1
            continue
        assert kept == r.kept, (c["name"], kept, r.kept)
        assert np.float32(tau) == r.tau, (c["name"], tau, r.tau)
        if margin > 1e-5:
            assert tok == want, (c["name"], tok, want, margin)
        assert r.mask[tok - 1], c["name"]
    assert unsafe <= len(all_cases) // 50, (unsafe, len(all_cases))


def test_kept_set_lies_in_the_window_on_every_vector(all_cases, header_out):
    """safe or not: the header's kept set lies between the narrowest and the widest set the margins admit, its pick in the
    widest, and where the pick over the widest set lies in the narrowest it is the header's pick"""
    for c, (tok, kept, tau) in zip(all_cases, header_out):
        want, margin, decided, r = filter_ref.sample_window(c["z"], c["T"], c["seed"], c["pos"], c["top_k"], c["top_p"], c["min_p"])
        assert (r.hi <= r.mask).all() and (r.mask <= r.lo).all(), c["name"]
        if r.safe:
            assert decided and (r.hi == r.lo).all(), c["name"]
            assert (want, margin) == filter_ref.sample(c["z"], c["T"], c["seed"], c["pos"], c["top_k"], c["top_p"], c["min_p"])[:2]
        assert int(r.hi.sum()) <= kept <= int(r.lo.sum()), (c["name"], kept)
        assert r.lo[tok - 1], c["name"]
        if decided and margin > 1e-5:
            assert tok == want, (c["name"], tok, want, margin)


def test_a_row_on_the_min_p_bound_leaves_the_pick_decided(host_prog):
    """V = 32,000 flat logits with one row placed on e = min_p: unsafe for the kept set by construction, yet the pick is decided
    unless that one row wins the draw; the header agrees on every decided vector"""
    V, T, min_p = 32000, 0.9, 0.1
    rng = np.random.default_rng(20261018)
    cases = []
    for i in range(24):
        z = (0.8 * rng.standard_normal(V)).astype(np.float32)
        z[rng.integers(V)] = np.float32(z.max() + T * np.log(min_p))
        cases.append(dict(name=f"on-bound-{i}", z=z, T=T, seed=100 + i, pos=1 + i, top_k=0, top_p=1.0, min_p=min_p))
    out = run_header(host_prog, cases)
    unsafe = undecided = 0
    for c, (tok, kept, tau) in zip(cases, out):
        want, margin, decided, r = filter_ref.sample_window(c["z"], c["T"], c["seed"], c["pos"], c["top_k"], c["top_p"], c["min_p"])
        unsafe += not r.safe
        assert r.kept > 100, c["name"]
        assert int(r.hi.sum()) <= kept <= int(r.lo.sum()) and r.lo[tok - 1], c["name"]
        if decided and margin > 1e-5:
            assert tok == want, (c["name"], tok, want, margin)
        else:
            undecided += 1
    assert unsafe >= 20 and undecided <= 1, (unsafe, undecided)


def test_top_k_1_keeps_exactly_the_ties_of_the_maximum(all_cases, header_out):
    n = 0
    for c, (tok, kept, tau) in zip(all_cases, header_out):
        if c["top_k"] != 1:
            continue
        z = c["z"]
        zmax = np.nanmax(z)
        assert kept == int((z == zmax).sum()) and tau == zmax, c["name"]
        assert z[tok - 1] == zmax
        n += 1
    assert n >= 40
    # two-level vectors: five rows share the maximum, top_k = 1 and 2 keep all five
    for c, (tok, kept, tau) in zip(all_cases, header_out):
        if c["name"].startswith("two-level") and c["top_k"] in (1, 2) and c["top_p"] == 1.0:
            assert kept == 5, c["name"]


def test_filters_off_keeps_every_row_above_minus_infinity(all_cases, header_out):
    n = 0
    for c, (tok, kept, tau) in zip(all_cases, header_out):
        V = c["z"].size
        if c["top_p"] != 1.0 or c["min_p"] != 0.0 or 0 < c["top_k"] < V:
            continue
        z = c["z"]
        assert kept == int((z > -np.inf).sum()), c["name"]            # (NaN compares false)
        assert tau == -np.inf, c["name"]
        if not np.isnan(z).any():                                     # the unfiltered rule of sample_ref (its argmax knows no NaN rows)
            want, margin = sample_ref.sample(z, c["T"], c["seed"], c["pos"])
            assert tok == want or margin <= 1e-5, c["name"]
        n += 1
    assert n >= 100


def test_kept_set_grows_with_top_k_top_p_and_one_minus_min_p(host_prog):
    """the kept sets are threshold sets { z >= tau }: growing = tau not rising and the count not falling"""
    cases = []
    sweeps = [("top_k", [1, 2, 3, 5, 8, 15, 16, 40, 100, 299, 300, 305]), ("top_p", [0.01, 0.1, 0.3, 0.5, 0.7, 0.9, 0.99, 0.999, 1.0]),
              ("min_p", [1.0, 0.9, 0.5, 0.2, 0.05, 0.01, 1e-4, 0.0])]
    for name, z in filter_ref.vectors(300, 5):
        for field, values in sweeps:
            for base in (dict(top_k=0, top_p=1.0, min_p=0.0), dict(top_k=50, top_p=0.95, min_p=0.001)):
                for v in values:
                    c = dict(name=f"{name}-{field}", z=z, T=0.9, seed=1, pos=1, **base)
                    c[field] = v
                    cases.append(c)
    out = run_header(host_prog, cases)
    i = 0
    for name, z in filter_ref.vectors(300, 5):
        for field, values in sweeps:
            for _ in range(2):
                got = out[i:i + len(values)]
                i += len(values)
                kept = [k for _, k, _ in got]
                taus = [t for _, _, t in got]
                assert all(a <= b for a, b in zip(kept, kept[1:])), (name, field, kept)
                assert all(a >= b for a, b in zip(taus, taus[1:])), (name, field, taus)
                assert kept[0] >= 1


def test_no_row_above_minus_infinity_is_no_token(host_prog):
    V = 64
    cases = [dict(name="nan", z=np.full(V, np.nan, np.float32), T=0.9, seed=1, pos=1, top_k=40, top_p=0.9, min_p=0.0),
             dict(name="-inf", z=np.full(V, -np.inf, np.float32), T=0.9, seed=1, pos=1, top_k=0, top_p=1.0, min_p=0.1)]
    z = np.zeros(V, np.float32)
    z[[3, 9]] = np.inf
    cases.append(dict(name="+inf", z=z, T=0.9, seed=1, pos=1, top_k=40, top_p=0.9, min_p=0.05))
    out = run_header(host_prog, cases)
    assert out[0][:2] == (0, 0) and out[1][:2] == (0, 0)
    assert out[2][0] in (4, 10) and out[2][1] == 2 and out[2][2] == np.inf


def test_filter_kernel_has_no_scratch(tmp_path):
    """sample_filter_kernel compiled for gfx950: 0 bytes of scratch, no spills, and registers that admit its 1,024 threads
    (hipcc of ROCm 7.2 reports 96 VGPRs, 78 SGPRs and 55,568 bytes of LDS)"""
    import re
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    src = tmp_path / "k.hip"
    src.write_text('#include "kernels.h"\n')
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", "-I", CSRC, str(src), "-o", str(tmp_path / "k.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = r.stderr.split("Function Name: ")
    mine = [b for b in blocks if "sample_filter_kernel" in b.split("\n")[0]]
    assert len(mine) == 1
    get = lambda key: int(re.search(re.escape(key) + r":\s+(\d+)", mine[0]).group(1))
    assert get("ScratchSize [bytes/lane]") == 0
    assert get("SGPRs Spill") == 0 and get("VGPRs Spill") == 0
    assert get("VGPRs") <= 128                                  # 16 waves of one workgroup on 4 SIMDs
    assert get("LDS Size [bytes/block]") <= 64 * 1024
