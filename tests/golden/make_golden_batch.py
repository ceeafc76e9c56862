#!/usr/bin/env python3
"""Golden vectors of the batched decode tests (tests/test_batch_gpu.py), by RUNNING THE REAL REFERENCE as make_golden.py does
(build container only): tiny-hs128w-long = tiny-hs128-long with hidden_dim 1408, a multiple of the batched GEMMs' 64-column step --
the batched passes refuse 1376.  oracle/build_ref.sh compiles the reference with these dims into oracle/_ref/; only DATA is kept:
the reference's logits per position and its greedy ids.

    python tests/golden/make_golden_batch.py          # rewrites tests/golden/tiny-hs128w-long.npz
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import llm_f90_amd  # noqa: E402,F401
from llm_f90_amd.tools import gguf  # noqa: E402

SEED = 20260928
CASES = [("tiny-hs128w-long", 320)]


def main():
    outdir = os.path.dirname(os.path.abspath(__file__))
    for name, n in CASES:
        s = gguf.SHAPES[name]
        dims = [s.emb_dim, s.hidden_dim, s.n_layers, s.n_heads, s.n_kv_heads, s.vocab_size, s.seq_len]
        subprocess.run([os.path.join(ROOT, "oracle", "build_ref.sh"), name] + [str(d) for d in dims], check=True)
        exe = os.path.join(ROOT, "oracle", "_ref", "llm_ref_" + name)
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, name + ".gguf")
            gguf.write_synth_gguf(path, s, SEED)
            r = subprocess.run([exe, "-m", path, "-n", str(n), "-t", "0"], cwd=td, capture_output=True, check=True)
            logits = np.fromfile(os.path.join(td, "logits.bin"), dtype="<f4").reshape(n, s.vocab_size)
        toks = [int(np.argmax(logits[i])) + 1 for i in range(n)]
        text = b"".join(gguf.vocab_strings(s.vocab_size)[t - 1] for t in toks)
        lines = r.stdout.split(b"\n")
        assert lines[0].strip().startswith(b"data offset"), lines[0]
        assert lines[1].rstrip(b" ") == text, (lines[1], text)      # the reference printed the same tokens
        srt = np.sort(logits, axis=1)
        np.savez_compressed(os.path.join(outdir, name + ".npz"), shape=name, seed=SEED, n=n, prompt="", ak=False,
                            prompt_ids=np.asarray([], np.int32), logits=logits, tokens=np.asarray(toks, np.int32),
                            stdout=np.frombuffer(r.stdout, np.uint8), top1_margin=(srt[:, -1] - srt[:, -2]))
        print(f"{name}: n={n} V={s.vocab_size} max|logit|={np.abs(logits).max():.3f} min top-1 margin={np.min(srt[:, -1] - srt[:, -2]):.4f}")


if __name__ == "__main__":
    main()
