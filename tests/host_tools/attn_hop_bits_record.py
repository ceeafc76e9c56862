#!/usr/bin/env python3
"""Records tests/golden/attn_hop_bits.npz: the logits tests/test_attn_hop_bits_gpu.py compares bit for bit.

Run it with a library built from the commit BEFORE the change under test, selected with LLMK_LIB:
    LLMK_LIB=/path/to/parent/libllmk.so python tests/host_tools/attn_hop_bits_record.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import llm_f90_amd  # noqa: E402,F401
from llm_f90_amd import llmk  # noqa: E402
from llm_f90_amd.tools import gguf  # noqa: E402
import attn_hop_bits as ahb  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "attn_hop_bits.npz")
    z = {}
    for key, tag, wtype in ahb.CASES:
        pos, lg = ahb.run_case(gguf, llmk, tag, wtype)
        z[key + "/pos"], z[key + "/logits"] = pos, lg
        print(f"{key}: {len(pos)} positions {pos.tolist()}, logits {lg.shape}, library {llmk.LIB_PATH}")
    np.savez_compressed(out, seed=np.int64(ahb.SEED), **z)
    print(f"wrote {out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
