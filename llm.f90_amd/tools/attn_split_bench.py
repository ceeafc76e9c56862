"""Decode attention of the context's own sequence: attn_kernel against the split pair of csrc/attn_split.h, per launch, by
llmk_time_kernel(ctx, 1, ..) -- one layer's attention at the context's current position, successive launches walking the layers.

    python -m llm_f90_amd.tools.attn_split_bench [--iters 200] [--reps 5] [--out FILE]

Two contexts per geometry on the same weights, one created with LLMK_ATTN_SPLIT unset and one with LLMK_ATTN_SPLIT=1, both with
seq_len 32,768 (attn_kernel's LDS score row still holds it).  The K/V rows are whatever the cache holds (zeros but for the fed
positions): the kernels' loads and arithmetic do not depend on the values.  Geometries: TinyLlama's attention (32 heads of 64, 4 kv
heads: kv_mul 8) over 8 layers and Llama-2-7B's (32 heads of 128, 32 kv heads: kv_mul 1) over 2 -- with few layers the K/V rows of a
short context stay in the 256 MB Infinity Cache between launches, as they do not in a real token pass (the figures below a few
thousand positions are latency figures either way).  Per position: the median of --reps alternating timings of --iters launches
(3 warm-up launches each), their range, and bytes/s against the algorithmic bytes 2 * kv_dim * 4 * pos of one layer's K and V rows."""
import argparse
import os
import statistics
import sys

from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf

GEOMETRIES = {"tinyllama (hs 64, kv_mul 8)": gguf.LlamaShape(2048, 64, 8, 32, 4, 64, 32768),
              "llama2-7b (hs 128, kv_mul 1)": gguf.LlamaShape(4096, 64, 2, 32, 32, 64, 32768)}
POSITIONS = (256, 1024, 4096, 16384, 32768)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else sys.stdout
    os.environ["LLMK_FORWARD_AHEAD"] = "0"      # llmk_forward leaves the position it was given
    print(f"# llmk_version {llmk.lib().llmk_version()}; {a.reps} x {a.iters} launches per figure; us per launch: median (min .. max); "
          f"GB/s of the median against 2 * kv_dim * 4 * pos bytes", file=out)
    for name, shape in GEOMETRIES.items():
        fw = gguf.synth_fused(shape, 20261127, gguf.GGML_F16)
        ctx = {}
        for kind, env in (("attn_kernel", None), ("split", "1")):
            os.environ.pop("LLMK_ATTN_SPLIT", None)
            if env:
                os.environ["LLMK_ATTN_SPLIT"] = env
            ctx[kind] = llmk.Llmk(fw, flags=llmk.FLAG_MULTI_KERNEL)
        os.environ.pop("LLMK_ATTN_SPLIT", None)
        print(f"{name}: {shape.n_layers} layers, kv_dim {shape.kv_dim}", file=out)
        for pos in POSITIONS:
            us = {kind: [] for kind in ctx}
            for m in ctx.values():
                m.forward(1, pos)
            for _ in range(a.reps):
                for kind, m in ctx.items():
                    ms, nbytes = m.time_kernel(1, a.iters)
                    us[kind].append(ms * 1e3)
            cells = []
            for kind in ctx:
                med = statistics.median(us[kind])
                cells.append(f"{kind} {med:9.2f} ({min(us[kind]):.2f} .. {max(us[kind]):.2f}) us {nbytes / med / 1e3:8.1f} GB/s")
            print(f"  pos {pos:6d}  {nbytes / 1e6:9.2f} MB  " + "   ".join(cells) +
                  f"   attn_kernel / split {statistics.median(us['attn_kernel']) / statistics.median(us['split']):.2f}", file=out, flush=True)
        for m in ctx.values():
            m.close()


if __name__ == "__main__":
    main()
