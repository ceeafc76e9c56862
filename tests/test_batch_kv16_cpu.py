"""A batch with f16 K/V caches (llmk_cache_*) without a device: the header declares the four symbols and the
bindings list them, null handles are refused before anything touches a GPU, the stored-value contract (clamp, then round to nearest
even) written out on integers agrees with np.float16, and the yardstick of tests/test_batch_kv16_gpu.py -- kv16_ref.forward_fed, the
float64 forward pass fed GIVEN cache rows -- is sound: fed its own rows it is forward_all, fed f16-rounded rows it is far enough from
forward_all that a pass which ignored the stored rows could not meet the bar."""
import functools
import os
import re

import numpy as np
import pytest

import attn_needle as an
import kv16_ref as kr
from conftest import REL_TOL, ROOT, rel_err
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf

NAMES = ["llmk_cache_create", "llmk_cache_type", "llmk_cache_bytes", "llmk_cache_peek"]
MODELS = ("tk-small", "tiny-gqa", "tiny-hs128w", "tiny-hs64")      # the shapes of the GPU tests' logits comparisons
N_POS = 60


@pytest.fixture(scope="module")
def lib():
    llmk.build_lib()
    return llmk.lib()


def test_header_declares_the_four_cache_symbols_and_the_bindings_list_them(lib):
    hdr = open(os.path.join(ROOT, "include", "llmk.h")).read()
    assert set(re.findall(r"^int (llmk_cache_[a-z_]+)\(", hdr, re.M)) == set(NAMES)
    f90 = open(os.path.join(ROOT, "llm.f90_amd", "host", "llmk_binding.f90")).read()
    for name in NAMES:
        assert name in llmk.SYMBOLS and hasattr(lib, name), name
        assert f'bind(C, name="{name}")' in f90, name
    assert lib.llmk_version() >= 407
    for attr in ("kv_type", "cache_bytes", "peek_kv"):
        assert hasattr(llmk.Batch, attr), attr
    assert llmk.KV_TYPES == {"f32": 0, "f16": 1}
    assert re.search(r"#define LLMK_TYPE_F32 0\b", hdr) and re.search(r"#define LLMK_TYPE_F16 1\b", hdr)


def test_null_arguments_are_refused_without_a_device(lib):
    import ctypes as C
    out = C.c_void_p()
    for kv_type in (0, 1, 2):
        assert lib.llmk_cache_create(None, 2, 16, kv_type, C.byref(out)) == 1
    assert lib.llmk_cache_type(None) == -1
    n = C.c_ulonglong(7)
    assert lib.llmk_cache_bytes(None, C.byref(n)) == 1 and n.value == 7
    row = np.zeros(64, np.float32)
    assert lib.llmk_cache_peek(None, 0, 0, 0, 1, 1, row.ctypes.data_as(C.POINTER(C.c_float))) == 1
    assert lib.llmk_cache_peek(None, 1, 0, -1, 1, 1, row.ctypes.data_as(C.POINTER(C.c_float))) == 1


def test_the_device_code_converts_by_a_plain_cast_behind_a_clamp():
    src = open(os.path.join(ROOT, "llm.f90_amd", "csrc", "prefill.h")).read()
    assert "x != x ? (_Float16)x : (_Float16)fminf(fmaxf(x, -65504.f), 65504.f)" in src
    # (cvt_pkrtz rounds toward zero: the prefill's GEMM splits activations with it, nothing of the batch's caches may)
    assert "cvt_pkrtz" not in open(os.path.join(ROOT, "llm.f90_amd", "csrc", "batch.h")).read()
    assert "cvt_pkrtz" not in src[src.index("pf_kv_half(float x)"):src.index("__global__ void pf_epi_qkv_kernel")]


def test_clamp_then_round_to_nearest_even_agrees_with_numpy_on_a_grid():
    """ties between neighbouring halves (normal and subnormal), the subnormal range and what lies below it, +-65504, the values
    beyond it (65520 is the tie that np.float16 alone would round to inf), +-0, +-inf, NaN, and a random sweep of all exponents"""
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)           # every finite non-negative half
    ties = (h[:-1] + h[1:]) / 2                                                                # exact in f32: 12 significant bits
    near = np.concatenate([ties, np.nextafter(ties.astype(np.float32), np.float32(0)), np.nextafter(ties.astype(np.float32), np.float32(1e9))])
    special = [0.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -26, 3 * 2.0 ** -26, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 65504.0, 65519.0, 65520.0, 65536.0,
               1e9, 3.4e38, np.inf, 1e-45, 1e-40]
    rng = np.random.default_rng(16)
    sweep = rng.integers(0, 0x7F800000, 200_000, dtype=np.int64).astype(np.uint32).view(np.float32)
    x = np.concatenate([h, near, special, sweep]).astype(np.float32)
    x = np.concatenate([x, -x])
    assert len(x) > 500_000
    want = kr.stored_half(x).astype(np.float16).view(np.uint16)
    got = kr.half_mirror(x)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (x[bad[:5]], got[bad[:5]], want[bad[:5]])
    assert np.isfinite(kr.stored_half(x)).all() and np.abs(kr.stored_half(x)).max() == 65504.0
    with np.errstate(over="ignore"):
        assert kr.stored_half(np.float32(65520.0)) == 65504.0 and np.isinf(np.float16(np.float32(65520.0)))
    assert kr.half_mirror(np.float32(-0.0))[0] == 0x8000 and kr.half_mirror(np.float32(0.0))[0] == 0
    nan = kr.half_mirror(np.array([np.nan, -np.nan], np.float32))
    assert ((nan & 0x7C00) == 0x7C00).all() and ((nan & 0x3FF) != 0).all() and np.isnan(kr.stored_half(np.float32(np.nan)))


@functools.lru_cache(maxsize=None)
def reference(shape):
    s = gguf.SHAPES[shape]
    fw = gguf.synth_fused(s, 777)
    n = min(N_POS, s.seq_len)
    rng = np.random.default_rng(5)
    tokens = np.array([2] + (rng.integers(3, s.vocab_size, n - 1) + 1).tolist())
    cache = {}
    logits, _ = an.forward_all(fw, tokens, cache=cache)
    K = np.stack([k.reshape(n, -1) for k in cache["k"]])
    V = np.stack([v.reshape(n, -1) for v in cache["v"]])
    return fw, tokens, logits, K, V


@pytest.mark.parametrize("shape", MODELS)
def test_forward_fed_its_own_rows_is_forward_all(shape):
    fw, tokens, logits, K, V = reference(shape)
    fed = kr.forward_fed(fw, tokens, K, V)
    err = rel_err(fed, logits).max()
    print(f"{shape}: forward_fed on forward_all's own float64 K/V: rel_err {err:.2e}")
    assert err <= 1e-11
    # ... and row by row, at positions of the caller's choosing, over caches longer than the row needs
    pick = np.array([len(tokens), 1, 17, 33])
    pick = pick[pick <= len(tokens)]
    part = kr.forward_fed(fw, tokens[pick - 1], K, V, pos=pick)
    assert rel_err(part, logits[pick - 1]).max() <= 1e-11


@pytest.mark.parametrize("shape", MODELS)
def test_forward_fed_rounded_rows_is_far_from_forward_all(shape):
    """what the f16 caches cost, and why the oracle cannot be the yardstick: a pass that ignored the stored rows -- read f32 values from
    somewhere, or another rounding -- would be this far from forward_fed on the stored rows"""
    fw, tokens, logits, K, V = reference(shape)
    fed = kr.forward_fed(fw, tokens, kr.stored_half(K), kr.stored_half(V))
    err = rel_err(fed, logits).max()
    print(f"{shape}: forward_fed on f16-rounded K/V against forward_all: rel_err {err:.2e}")
    assert err > 2 * REL_TOL
    assert err < 1e-2            # (still the same model: a few 1e-4)
