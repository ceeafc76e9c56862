"""Rate of llmk_score next to the only way to get the same numbers without it (n llmk_forward calls, log-softmax on the host),
next to llmk_prefill on the same tokens (the difference is the price of the classifier for all positions) and with the logits
copied back.  Seeded tokens, warmed up, each figure the median of 5, the variants alternated inside one process.
    python tests/host_tools/score_rate.py [model=tinyllama-f32|tinyllama-f16|llama2-7b-q4_0+q6_K] [n=512,2048] [out.txt]
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

MODELS = {"tinyllama-f32": ("tinyllama", 0, False), "tinyllama-f16": ("tinyllama", 1, False), "llama2-7b-q4_0+q6_K": ("llama2-7b", 2, True)}
name = sys.argv[1] if len(sys.argv) > 1 else "tinyllama-f32"
ns = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "512,2048").split(",")]
out = open(sys.argv[3], "a") if len(sys.argv) > 3 else None
shape_name, wtype, q6 = MODELS[name]
s = gguf.SHAPES[shape_name]
fw = gguf.synth_fused(s, bench.SEED, wtype) if shape_name == "tinyllama" else None
m = bench.build_streamed(s, wtype, fw, 0, 0, 0, 1, None, "none", cls_q6k=q6)


def say(line):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def host_logprobs(seq, tg):
    """the baseline: one llmk_forward (and its 4 V byte copy) per position, log-softmax in numpy"""
    lp = np.zeros(len(seq), np.float32)
    for pos, tok in enumerate(seq, 1):
        z = m.forward(tok, pos)
        if tg[pos - 1]:
            mx = z.max()
            lp[pos - 1] = z[tg[pos - 1] - 1] - (mx + np.log(np.exp(z - mx).sum()))
    return lp


say(f"# python tests/host_tools/score_rate.py {' '.join(sys.argv[1:3])}    ({name}, path: {m.path_name()})")
for n in ns:
    rng = np.random.default_rng(n)
    seq = [2] + (rng.integers(3, s.vocab_size, n - 1) + 1).tolist()
    tg = np.append(np.asarray(seq[1:], np.int32), 0).astype(np.int32)
    variants = {
        "score": lambda: m.score(seq, 1, targets=tg),
        "forward x n + host log-softmax": lambda: host_logprobs(seq, tg),
        "prefill": lambda: m.prefill(seq, 1),
        "score + logits": lambda: m.score(seq, 1, targets=tg, want_logits=True),
    }
    times = {k: [] for k in variants}
    ref = None
    for rep in range(6):                               # rep 0 warms up
        for k, f in variants.items():
            m.reset()
            t0 = time.perf_counter()
            r = f()
            dt = time.perf_counter() - t0
            if rep:
                times[k].append(dt)
            elif k == "score":
                ref = r
            elif k.startswith("forward"):
                say(f"n {n}: max |score - host log-softmax of llmk_forward| = {np.abs(ref - r).max():.3e}")
    med = {k: statistics.median(v) for k, v in times.items()}
    for k in variants:
        say(f"n {n:5d}  {k:32s} {med[k] * 1e3:10.2f} ms  {n / med[k]:10.0f} positions/s")
    say(f"n {n:5d}  score / baseline = {med['forward x n + host log-softmax'] / med['score']:.1f}x;  classifier share of score = "
        f"{(med['score'] - med['prefill']) / med['score'] * 100:.1f} %;  logits copy = +{(med['score + logits'] - med['score']) * 1e3:.2f} ms")
m.reset()
for k, label in [(7, "w1|w3"), (8, "wqkv"), (9, "wo"), (10, "w2"), (12, "classifier")]:
    if k == 12 and q6:
        say("time_kernel 12: no classifier GEMM on a q6_K classifier (the decode classifier runs per position)")
        continue
    ms, b = m.time_kernel(k, 20)
    say(f"time_kernel {k:2d} {label:10s} {ms * 1e3:8.1f} us  {b / 1e6:8.1f} MB")
m.close()
