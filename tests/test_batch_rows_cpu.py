"""The rows functions (llmk_rows_*) without a device: the header declares the four symbols and the binding lists
them, null handles are refused before anything touches a GPU, and the paragraph of llmk_batch_decode still says where penalties and
records went."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from llm_f90_amd import llmk

NAMES = ["llmk_rows_set_history", "llmk_rows_get_history", "llmk_rows_decode", "llmk_rows_sample_logits"]


@pytest.fixture(scope="module")
def lib():
    llmk.build_lib()
    return llmk.lib()


def header():
    return open(os.path.join(ROOT, "include", "llmk.h")).read()


def test_header_declares_the_rows_symbols_and_the_binding_lists_them(lib):
    declared = set(re.findall(r"^int (llmk_rows_[a-z_]+)\(", header(), re.M))
    assert declared == set(NAMES)
    for name in NAMES:
        assert name in llmk.SYMBOLS and hasattr(lib, name), name
    f90 = open(os.path.join(ROOT, "llm.f90_amd", "host", "llmk_binding.f90")).read()
    for name in NAMES:
        assert f'bind(C, name="{name}")' in f90, name
    for method in ("decode_rows", "sample_logits_rows", "set_history", "get_history"):
        assert callable(getattr(llmk.Batch, method)), method
    assert lib.llmk_version() >= 405


def test_null_handles_are_refused_without_a_device(lib):
    one = (C.c_int * 1)(1)
    out = (C.c_int * 1)(0)
    z = (C.c_float * 4)()
    sp = llmk.sampler(1.0, 1)
    assert lib.llmk_rows_set_history(None, 0, one, 1, 1) == 1
    assert lib.llmk_rows_get_history(None, 0, out, 1, 1) == 1
    assert lib.llmk_rows_decode(None, 1, one, one, one, 1, None, None, None, out) == 1
    assert lib.llmk_rows_decode(None, 1, one, one, one, 1, C.byref(sp), None, None, out) == 1
    assert lib.llmk_rows_sample_logits(None, 1, one, one, z, C.byref(sp), None, None, out, None, None, None) == 1


def test_the_batch_decode_paragraph_keeps_its_sentence_and_points_at_the_rows_functions():
    flat = re.sub(r"\s*\n \*\s*", " ", header())
    assert "Penalties, logit bias and log-prob records are out of scope of this function: llmk_rows_decode, below, takes them" in flat
    para = flat[flat.index(" decode: "):flat.index(" time: ")]
    assert "Penalties, logit bias and log-prob records are out of scope" in para
