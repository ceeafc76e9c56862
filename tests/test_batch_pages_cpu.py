"""Paged K/V caches (llmk_pages_*): what can be said without a device -- the header and the binding hold the five names, and a NULL
handle is refused before anything touches one."""
import ctypes as C
import os
import re

from conftest import ROOT
from llm_f90_amd import llmk

NAMES = ["llmk_pages_create", "llmk_pages_free", "llmk_pages_release", "llmk_pages_share", "llmk_pages_table"]


def test_the_header_and_the_binding_hold_the_five_names():
    hdr = open(os.path.join(ROOT, "include", "llmk.h")).read()
    assert sorted(set(re.findall(r"\b(llmk_pages_[a-z_]+)\s*\(", hdr))) == NAMES
    assert sorted(s for s in llmk.SYMBOLS if s.startswith("llmk_pages_")) == NAMES


def test_null_handles_are_refused_without_a_device():
    llmk.build_lib()
    lib, h = llmk.lib(), C.c_void_p()
    assert lib.llmk_pages_create(None, 2, 64, 0, 16, 4, C.byref(h)) == 1 and not h.value
    assert lib.llmk_pages_release(None, 0, 0) == 1 and lib.llmk_pages_share(None, 1, 0, 1) == 1
    assert lib.llmk_pages_free(None) == -1 and lib.llmk_pages_table(None, 0, None, 0) == -1
