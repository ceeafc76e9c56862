"""llmk_score's arithmetic (llm.f90_amd/csrc/score.h) on the host: the element step and the merge rule of the running
log-sum-exp, and the first-maximum rule, compiled into a host program and held against a float64 numpy log-sum-exp in
several groupings; the tests' numpy restatement of llmk_score's outputs (tests/score_ref.py).  No device needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import score_ref
from conftest import GOLDEN_CASES, ROOT, load_golden

CSRC = os.path.join(ROOT, "llm.f90_amd", "csrc")
# per row: "V" then V f32 bit patterns (hex).  Output per row, for each grouping g of GROUPS (0 = one chain of element steps; else
# chunks of g elements, each stepped from the empty state): the f32 bits of lse and the first maximum's index, once with the chunk
# states merged left to right and once merged pairwise as a tree
PROGRAM = r'''
#include "score.h"
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <vector>
static const int GROUPS[4] = {0, 2, 7, 128};
int main() {
    int V;
    while (scanf("%d", &V) == 1) {
        std::vector<float> z(V);
        for (int i = 0; i < V; ++i) { unsigned b; if (scanf("%x", &b) != 1) return 1; memcpy(&z[i], &b, 4); }
        for (int gi = 0; gi < 4; ++gi) {
            const int g = GROUPS[gi] ? GROUPS[gi] : V;
            std::vector<llmk_lse> st;
            std::vector<llmk_amax> am;
            for (int i0 = 0; i0 < V; i0 += g) {
                llmk_lse s = llmk_lse_empty();
                llmk_amax a = llmk_amax_empty();
                for (int i = i0; i < V && i < i0 + g; ++i) { s = llmk_lse_step(s, z[i]); a = llmk_amax_step(a, z[i], i); }
                st.push_back(s); am.push_back(a);
            }
            llmk_lse chain = llmk_lse_empty();
            llmk_amax achain = llmk_amax_empty();
            for (size_t k = 0; k < st.size(); ++k) { chain = llmk_lse_merge(chain, st[k]); achain = llmk_amax_merge(achain, am[k]); }
            while (st.size() > 1) {          // tree: neighbours pairwise, the odd one carried (and merged from the right, too)
                std::vector<llmk_lse> s2;
                std::vector<llmk_amax> a2;
                for (size_t k = 0; k + 1 < st.size(); k += 2) { s2.push_back(llmk_lse_merge(st[k + 1], st[k])); a2.push_back(llmk_amax_merge(am[k + 1], am[k])); }
                if (st.size() & 1) { s2.push_back(st.back()); a2.push_back(am.back()); }
                st.swap(s2); am.swap(a2);
            }
            const float l0 = llmk_lse_value(chain), l1 = llmk_lse_value(st[0]);
            uint32_t b0, b1;
            memcpy(&b0, &l0, 4); memcpy(&b1, &l1, 4);
            printf("%08x %d %08x %d ", b0, achain.i, b1, am[0].i);
        }
        printf("\n");
    }
    return 0;
}
'''
NGROUPINGS = 8      # 4 groupings x (chain, tree)


@pytest.fixture(scope="module")
def host_prog(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        cxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    d = tmp_path_factory.mktemp("score")
    src, exe = str(d / "score_host.cpp"), str(d / "score_host")
    with open(src, "w") as f:
        f.write(PROGRAM)
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(exe, rows):
    text = "".join(f"{len(r)} " + " ".join(f"{int(b):x}" for b in np.asarray(r, np.float32).view(np.uint32)) + "\n" for r in rows)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = [l.split() for l in r.stdout.split("\n") if l]
    assert len(out) == len(rows)
    lse = np.array([[int(v, 16) for v in l[0::2]] for l in out], np.uint32).view(np.float32)
    idx = np.array([[int(v) for v in l[1::2]] for l in out], np.int64)
    assert lse.shape == (len(rows), NGROUPINGS)
    return lse, idx


def _rows():
    rng = np.random.default_rng(20261016)
    rows = []
    for V in (1, 2, 7, 300, 1000, 1024, 32000):
        for scale in (0.5, 3.0, 30.0):
            rows.append((rng.standard_normal(V) * scale).astype(np.float32))
    for V in (300, 1024, 4099):                                 # -inf entries: scattered, whole leading chunks, all but one
        r = (rng.standard_normal(V) * 3).astype(np.float32)
        r[rng.random(V) < 0.3] = -np.inf
        rows.append(r)
        r = (rng.standard_normal(V) * 3).astype(np.float32)
        r[:256] = -np.inf
        rows.append(r)
        r = np.full(V, -np.inf, np.float32)
        r[V // 2] = 1.25
        rows.append(r)
    for V in (300, 32000):                                      # the maximum comes last (every step before it rescales or adds), and first
        r = np.sort((rng.standard_normal(V) * 3).astype(np.float32))
        rows.append(r)
        rows.append(r[::-1].copy())
    r = (rng.standard_normal(1000) * 3).astype(np.float32)      # a repeated maximum: the first one wins
    r[[17, 400, 999]] = 20.0
    rows.append(r)
    return rows


# Largest |f32 grouping - float64 lse| over the rows above, in f32 ulps of lse, per grouping in the program's output order (one
# chain: both columns; pairs, chunks of 7, chunks of 128: merged left to right / as a tree), measured with this test (g++ -O2,
# glibc expf / logf).  A state that goes through n sequential steps or merges is a sequential f32 sum of n terms and its rounding
# grows with n: one chain over 32,000 sorted logits is 77 ulp off, 16,000 pair states merged left to right 27 ulp; the groupings
# that keep every chain short (what the kernels do: four element steps per thread, then merges of equal halves) stay at 1 ulp.
# Each bound is three times its measurement.
MEASURED_ULP = np.array([77.09, 77.09, 27.09, 1.02, 3.09, 1.02, 1.02, 1.02])
BOUND_ULP = 3 * MEASURED_ULP


def test_lse_groupings_match_float64(host_prog):
    rows = _rows()
    lse, idx = _run(host_prog, rows)
    ref = np.array([score_ref.lse(r)[0] for r in rows])
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = np.abs(lse.astype(np.float64) - ref[:, None]) / ulp[:, None]
    print(f"max error {err.max():.3f} ulp; per grouping {err.max(axis=0).round(3).tolist()}")
    assert np.isfinite(lse).all()
    assert (err.max(axis=0) <= BOUND_ULP).all(), err.max(axis=0)
    first = np.array([int(np.argmax(r)) for r in rows])
    assert (idx == first[:, None]).all()


def test_empty_and_all_minus_inf_rows(host_prog):
    rows = [np.full(v, -np.inf, np.float32) for v in (1, 7, 300)]
    lse, idx = _run(host_prog, rows)
    assert np.all(lse == -np.inf) and np.all(idx == -1)          # no NaN out of -inf - -inf anywhere
    rows = [np.array([0.5, np.nan, 1.0], np.float32)]             # a NaN logit poisons the row's lse and never wins the maximum
    lse, idx = _run(host_prog, rows)
    assert np.isnan(lse).all() and np.all(idx == 2)


def test_golden_rows_through_the_header(host_prog):
    """every row of two real-reference goldens: the header's log-sum-exp (one chain and chunks of 128) against float64"""
    for tag in ("tiny-gqa", "tk-small"):
        g = load_golden(tag)
        rows = list(g["logits"])
        lse, idx = _run(host_prog, rows)
        ref = score_ref.lse(g["logits"])
        err = np.abs(lse.astype(np.float64) - ref[:, None]) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)[:, None]
        print(tag, err.max(axis=0).round(3).tolist())
        assert (err.max(axis=0) <= BOUND_ULP).all(), err.max(axis=0)
        assert (idx == np.argmax(g["logits"], axis=1)[:, None]).all()


def test_score_ref_restates_the_definition():
    z = np.array([[0.0, 1.0, 2.0, 2.0], [-1.0, -np.inf, 3.0, 0.5]], np.float64)
    lp, am = score_ref.score(z, [2, 0])
    assert am.tolist() == [3, 3]                                  # first maximum, 1-based
    assert lp[1] == 0.0
    assert abs(lp[0] - (1.0 - np.log(np.exp(0) + np.exp(1) + 2 * np.exp(2)))) < 1e-12
    assert np.allclose(np.exp(score_ref.score(z, [1, 1])[0][0]) + np.exp(lp[0]) + 2 * np.exp(score_ref.score(z, [3, 1])[0][0]), 1.0)
    assert score_ref.default_targets([2, 5, 9]).tolist() == [5, 9, 0]
    assert score_ref.lse(np.full((1, 4), -np.inf))[0] == -np.inf


def test_plain_f32_lse_over_the_goldens_is_far_inside_the_gpu_bound():
    """orientation for the GPU tests' bound on log-probs (2 * REL_TOL * max|logit|, >= 5e-4 on these goldens): a plain numpy f32
    log-sum-exp differs from float64 by < 1e-6 on every golden row"""
    worst = 0.0
    for tag in GOLDEN_CASES:
        z = load_golden(tag)["logits"]
        m = z.max(axis=1, keepdims=True)
        f32 = (m[:, 0] + np.log(np.exp(z - m, dtype=np.float32).sum(axis=1, dtype=np.float32))).astype(np.float32)
        worst = max(worst, np.abs(f32.astype(np.float64) - score_ref.lse(z)).max())
    assert worst < 1e-6, worst
