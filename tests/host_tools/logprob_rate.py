"""Rate of the pipelined decode with the log-prob record (llmk_decode_sample_lp, top_n 0 / 5 / 20) next to the same call without it
(llmk_decode_sample_ex / llmk_decode_greedy), in one process, alternated; seeded, warmed up, each figure the median of 5.
    python tests/host_tools/logprob_rate.py [model=tinyllama-f32|llama2-7b-q4_0+q6_K] [n=248] [out.txt]
    python tests/host_tools/logprob_rate.py MODEL trace      one decode of each kind and nothing else (for a kernel trace of its own:
                                                             sample_logprob_kernel beside sample_filter_kernel at top_k 40, top_p 0.95)
"""
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import llm_f90_amd  # noqa: F401
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf
import bench

MODELS = {"tinyllama-f32": ("tinyllama", 0, False), "llama2-7b-q4_0+q6_K": ("llama2-7b", 2, True)}
name = sys.argv[1] if len(sys.argv) > 1 else "tinyllama-f32"
trace = len(sys.argv) > 2 and sys.argv[2] == "trace"
n = 248 if trace or len(sys.argv) < 3 else int(sys.argv[2])
out = open(sys.argv[3], "a") if len(sys.argv) > 3 else None
shape_name, wtype, q6 = MODELS[name]
s = gguf.SHAPES[shape_name]
fw = gguf.synth_fused(s, bench.SEED, wtype) if shape_name == "tinyllama" else None
m = bench.build_streamed(s, wtype, fw, 0, 0, 0, 1, None, "none", cls_q6k=q6)
T, SEED, FILT = 0.9, 1, dict(top_k=40, top_p=0.95)


def say(line):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


variants = {
    "sample_ex (top_k 40, top_p 0.95)": lambda: m.decode_sample_ex(2, 1, n, T, SEED, **FILT),
    "sample_lp top_n 0": lambda: m.decode_sample_lp(2, 1, n, 0, temperature=T, seed=SEED, **FILT)[0],
    "sample_lp top_n 5": lambda: m.decode_sample_lp(2, 1, n, 5, temperature=T, seed=SEED, **FILT)[0],
    "sample_lp top_n 20": lambda: m.decode_sample_lp(2, 1, n, 20, temperature=T, seed=SEED, **FILT)[0],
    "greedy": lambda: m.decode_greedy(2, 1, n),
    "greedy_lp top_n 20": lambda: m.decode_sample_lp(2, 1, n, 20)[0],
}
say(f"# python tests/host_tools/logprob_rate.py {' '.join(sys.argv[1:3])}    ({name}, path: {m.path_name()}, {n} positions per call)")
if trace:
    for k in ("sample_ex (top_k 40, top_p 0.95)", "sample_lp top_n 20"):
        m.reset()
        variants[k]()
    m.close()
    sys.exit(0)
times = {k: [] for k in variants}
ids = {}
for rep in range(6):                                   # rep 0 warms up
    for k, f in variants.items():
        m.reset()
        t0 = time.perf_counter()
        r = f()
        dt = time.perf_counter() - t0
        if rep:
            times[k].append(dt)
        else:
            ids[k] = np.asarray(r)
assert all(np.array_equal(ids[k], ids["sample_ex (top_k 40, top_p 0.95)"]) for k in ids if k.startswith("sample"))
assert np.array_equal(ids["greedy"], ids["greedy_lp top_n 20"])
base = {"sample": statistics.median(times["sample_ex (top_k 40, top_p 0.95)"]), "greedy": statistics.median(times["greedy"])}
for k in variants:
    med = statistics.median(times[k])
    say(f"{k:34s} {n / med:9.1f} tok/s  (min {n / max(times[k]):8.1f} max {n / min(times[k]):8.1f})  "
        f"{(med - base[k.split('_')[0]]) / n * 1e6:+7.2f} us per token against the call without log-probs")
m.close()
