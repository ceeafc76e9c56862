"""Every legal q6_K, q4_0 and f16 encoding through every kernel that decodes one (tests/weight_edge.py: crafted rows, one class
of encodings per row; test_weight_edge_cpu.py: what the reference and the bar are worth).  One layer, 3 decode positions and
a batch of 5, teacher-forced; the reference is forward64 on the decoded weights; the bar is conftest.REL_TOL, applied WITHIN every
class of rows (class_err) and to the whole position (rel_err).

Which llmk_peek is live where (csrc/llmk.hip llmk_peek): 4 and 5 read the context's KV cache, which every path writes (the
multi-kernel QKV epilogue, the persistent kernel, the batched pass, a rank's slice); 0..3 read d_x / d_q / d_xb / d_hb, which only
the multi-kernel launches write (launch_qkv, launch_attn, launch_w13, launch_w2 -- the persistent kernel keeps these vectors in its
own exchange buffers), so q, xb, hb and x are checked on path 0 only."""
import numpy as np
import pytest

import weight_edge as we
from llm_f90_amd import llmk

pytestmark = pytest.mark.gpu

MK = llmk.FLAG_MULTI_KERNEL
# (model, flags): the persistent kernel where the library holds the shape, and the multi-kernel path (tk-small has no q4_0
# instantiation of the persistent kernel, so its one case is the multi-kernel path; tinyllama-q4 stands in on the persistent kernel)
CASES = [("q6k-E256-f16", 0), ("q6k-E1024-q4", 0), ("tinyllama-q4-q6k", 0), ("tinyllama-q4-q6k", MK), ("llama7b-q4-q6k", 0),
         ("llama7b-q4-q6k", MK), ("tinyllama-q4", 0), ("tk-small-q4", MK), ("tiny-70bish-q4", MK),
         ("tk-small16-f16", 0), ("tk-small16-f16", MK)]
IDS = ["%s-%s" % (n, "multikernel" if f else "default") for n, f in CASES]
WT = {(1, 1): "f16", (2, 2): "q4_0", (2, 14): "q4_0+q6_K", (1, 14): "f16+q6_K"}


def expected_path(name, flags):
    """1 where this build of the library holds a persistent-kernel instantiation of the model and it was not switched off"""
    (E, H, nh, nkv, V), mt, ct = we.MODELS[name]
    return 1 if not flags and (E, H, nh, nkv, V, WT[(mt, ct)]) in llmk.tk_shapes() else 0


# these must really run the persistent kernel under the default flags
ON_THE_PERSISTENT_KERNEL = {"tinyllama-q4-q6k", "llama7b-q4-q6k", "tinyllama-q4", "tk-small16-f16"}


def _names(fw):
    return we.CLASS_NAMES[fw.cls_type], we.CLASS_NAMES[fw.ggml_type]


@pytest.mark.parametrize("name,flags", CASES, ids=IDS)
def test_decode_matches_forward64_in_every_class_of_encodings(name, flags, gguf):
    """3 decode positions: the logits by classifier class, the K and V cache rows by wqkv class, on the multi-kernel path q, xb,
    hb and x by row class, and the whole position."""
    fw, rc, ref = we.model(gguf, name)
    s = fw.shape
    cn, mn = _names(fw)
    m = llmk.Llmk(fw, flags=flags)
    path = expected_path(name, flags)
    assert m.path() == path, m.path_name()
    assert path == 1 or flags or name not in ON_THE_PERSISTENT_KERNEL
    r = we.Report("decode %s path %d" % (name, path))
    for pos, tok in enumerate(we.TOKENS[:3], start=1):
        lg = m.forward(tok, pos)
        r.add("logits", pos, lg, ref["logits"][pos - 1], rc["logits"], cn)
        r.whole(pos, lg, ref["logits"][pos - 1])
        r.add("k", pos, m.peek(4, s.kv_dim, 0, pos), ref["k"][0, pos - 1], rc["k"], mn)
        r.add("v", pos, m.peek(5, s.kv_dim, 0, pos), ref["v"][0, pos - 1], rc["v"], mn)
        if path == 0:
            for which, q, n in ((0, "x", s.emb_dim), (1, "q", s.emb_dim), (2, "xb", s.emb_dim), (3, "hb", s.hidden_dim)):
                r.add(q, pos, m.peek(which, n), ref[q][pos - 1], rc[q], mn)
    assert m.path() == path                      # nothing retired the persistent kernel on the way
    m.close()
    r.finish()


@pytest.mark.parametrize("name", list(we.MODELS))
def test_prefill_and_score_match_forward64_in_every_class_of_encodings(name, gguf):
    """The batched kernels: llmk_prefill of 5 tokens leaves the logits of position 5 and the K and V rows of all 5 (the q4_0 / f16
    GEMMs of prefill.h); llmk_score returns the logits of every position (the classifier GEMM of score.h, or gemv_q6k_kernel row by
    row for a q6_K classifier)."""
    fw, rc, ref = we.model(gguf, name)
    s = fw.shape
    cn, mn = _names(fw)
    n = len(we.TOKENS)
    m = llmk.Llmk(fw)
    r = we.Report("prefill %s" % name)
    lg = m.prefill(we.TOKENS, 1)
    r.add("logits", n, lg, ref["logits"][n - 1], rc["logits"], cn)
    r.whole(n, lg, ref["logits"][n - 1])
    for pos in range(1, n + 1):
        r.add("k", pos, m.peek(4, s.kv_dim, 0, pos), ref["k"][0, pos - 1], rc["k"], mn)
        r.add("v", pos, m.peek(5, s.kv_dim, 0, pos), ref["v"][0, pos - 1], rc["v"], mn)
    m.reset()
    sc = we.Report("score %s" % name)
    lgs = m.score(we.TOKENS, 1, want_logits=True, want_logprob=False)
    for pos in range(1, n + 1):
        sc.add("logits", pos, lgs[pos - 1], ref["logits"][pos - 1], rc["logits"], cn)
        sc.whole(pos, lgs[pos - 1], ref["logits"][pos - 1])
    m.close()
    red = r.red + sc.red
    r.red = sc.red = []
    r.finish()
    sc.finish()
    assert not red, (name, red)


def test_virtual_ranks_with_a_crafted_q6k_classifier_match_forward64(gguf):
    """test_tp_gpu.py's q6_K case on crafted rows: two tensor-parallel ranks, each with its V / 2 rows of raw super-blocks (row
    r of rank 1 is row 320 + r of the file: its classes start elsewhere in the cycle), q4_0 matrices split by rows and by columns."""
    s = gguf.LlamaShape(512, 1024, 1, 4, 4, 640, 32)
    fw, classes = we.craft_model(gguf, s, 2, 14, 99)
    ref = we.forward64(we.decoded(gguf, fw), we.TOKENS[:3])
    P = 2
    ranks = [llmk.Llmk(fw, tp_rank=k, tp_size=P) for k in range(P)]

    def exchange():
        total = ranks[0].tp_read_partial()
        for m in ranks[1:]:
            total = total + m.tp_read_partial()
        for m in ranks:
            m.tp_write_partial(total)
    r = we.Report("virtual ranks q4_0+q6_K")
    for pos, tok in enumerate(we.TOKENS[:3], start=1):
        for m in ranks:
            m.tp_begin(tok, pos)
        for seg in (0, 1):
            for m in ranks:
                m.tp_segment(seg, 0)
            exchange()
        for m in ranks:
            m.tp_segment(2)
        lg = np.concatenate([m.tp_read_logits() for m in ranks])
        r.add("logits", pos, lg, ref["logits"][pos - 1], classes["wcls"], we.Q6K_CLASSES)
        r.whole(pos, lg, ref["logits"][pos - 1])
    for m in ranks:
        m.close()
    r.finish()
