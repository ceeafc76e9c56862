"""llmk_cls_form (include/llmk.h): the entry point that tells which form the classifier of a batched pass takes -- what of it can
be checked without a GPU."""
import os
import re

from conftest import ROOT
from llm_f90_amd import llmk


def test_cls_form_is_exported_and_refuses_a_null_context():
    L = llmk.lib()
    assert "llmk_cls_form" in llmk.SYMBOLS and hasattr(L, "llmk_cls_form")
    assert L.llmk_cls_form(None, 5) == -1           # -LLMK_E_ARG: errors are negative, the forms are 0, 1, 2
    assert (llmk.CLS_NONE, llmk.CLS_GEMM, llmk.CLS_ROWS) == (0, 1, 2)


def test_version_counts_the_new_entry_point():
    assert llmk.lib().llmk_version() >= 404


def test_header_binding_and_crossover_agree():
    inc = open(os.path.join(ROOT, "include", "llmk.h")).read()
    for name, val in (("LLMK_CLS_NONE", llmk.CLS_NONE), ("LLMK_CLS_GEMM", llmk.CLS_GEMM), ("LLMK_CLS_ROWS", llmk.CLS_ROWS)):
        assert re.search(r"#define %s %d\b" % (name, val), inc), name
    assert "int llmk_cls_form(llmk_ctx *ctx, int rows);" in inc
    f90 = open(os.path.join(ROOT, "llm.f90_amd", "host", "llmk_binding.f90")).read()
    assert 'bind(C, name="llmk_cls_form")' in f90
    # the crossover the GPU tests assume is the library's
    hip = open(os.path.join(ROOT, "llm.f90_amd", "csrc", "llmk.hip")).read()
    m = re.search(r"#define LLMK_Q6K_GEMM_MIN_ROWS (\d+)", hip)
    gpu = open(os.path.join(ROOT, "tests", "test_q6k_gemm_gpu.py")).read()
    assert m and re.search(r"^GEMM_MIN_ROWS = %s\b" % m.group(1), gpu, re.M)
