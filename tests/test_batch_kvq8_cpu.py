"""A batch with q8_0 K/V caches (llmk_cache_create with LLMK_TYPE_Q8_0) without a device: the stored-value
contract of include/llmk.h as kvq8_ref.stored_q8 states it -- on a grid of ties, saturation, zeros, subnormals and NaN, and its
idempotence, which is how the GPU tests recognise a q8_0 row -- the yardstick (kv16_ref.forward_fed on rows quantised by the reference
itself meets REL_TOL against the quantising float64 pass), the movement of the logits per test shape (printed: the GPU file's sanity
bound is 4 x this), the header and the bindings, and the registers of the new attention kernels."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import attn_needle as an
import kvq8_ref as kq
from conftest import REL_TOL, ROOT, rel_err
from llm_f90_amd import llmk
from llm_f90_amd.tools import gguf

MODELS = ("tiny-hs64", "tk-small", "tiny-gqa", "tiny-hs128w", "tiny-kvmul3")
N_POS = 63


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def block(values, fill=0.0):
    """a block of 32 f32 values: `values` first, `fill` behind them"""
    b = np.full(32, fill, np.float32)
    b[:len(values)] = values
    return b


# ---- the rule -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1.0, 0.5, 3.0, 2.0 ** -10, 0.0999755859375, 515.5])
def test_ties_round_away_from_zero(d):
    """x = (k + 0.5) * d next to an amax of 127 * d, for every k in +-0..126 and a d that is an f16: d32 = amax / 127 is d again, id =
    1 / d, and wherever the f32 product x * id is the tie k + 0.5 itself the quant is k + 1 away from zero -- never the even neighbour
    (rintf) and never k (truncation).  For d a power of two every product is exact; for the others the ties whose product is exact are
    counted and must be there."""
    d = np.float32(d)
    assert np.float32(np.float16(d)) == d
    amax = np.float32(127.0) * d
    assert amax / np.float32(127.0) == d
    inv = np.float32(1.0) / d
    ks = np.arange(0, 127, dtype=np.float32)
    checked = 0
    for sign in (1.0, -1.0):
        for k0 in range(0, 127, 31):
            k = ks[k0:k0 + 31]
            x = (np.float32(sign) * (k + np.float32(0.5)) * d).astype(np.float32)
            got = kq.stored_q8(block(x, amax))
            assert got[31] == amax
            exact = (x * inv).astype(np.float32) == np.float32(sign) * (k + np.float32(0.5))
            want = np.float32(sign) * (k + 1) * d
            assert np.array_equal(got[:len(k)][exact], want[exact]), (d, sign, k0)
            checked += int(exact.sum())
    assert checked >= (254 if float(np.log2(d)).is_integer() else 32), checked


def test_saturation_zeros_subnormals_and_nan():
    F = np.float32(65504.0)
    d_max = np.float32(np.float16(F / np.float32(127.0)))
    # amax at 65504 and beyond: stored as +-127 * d with d finite (d32 = 515.78 never overflows an f16)
    for big in (65504.0, 65520.0, 1e9, np.inf):
        for sign in (1.0, -1.0):
            got = kq.stored_q8(block([sign * big, 1000.0, -0.0, 3.0]))
            assert np.isfinite(got).all() and got[0] == np.float32(sign * 127.0) * d_max, (big, sign, got[:4])
            assert got[1] == np.float32(2.0) * d_max and got[3] == 0.0      # 1000 / 515.78 = 1.94 -> 2; 3 / 515.78 -> 0
            assert not np.signbit(got).any() or sign < 0
            assert not np.signbit(got[1:]).any()                              # (never -0.0)
    assert np.float32(127.0) * d_max < np.float32(65536.0)
    # a block of zeros, of either sign: +0.0
    for z in (0.0, -0.0):
        got = kq.stored_q8(np.full(32, z, np.float32))
        assert np.array_equal(bits(got), np.zeros(32, np.uint32))
    # amax below 2^-25 * 127: d32 rounds to the f16 zero: all +0.0 (2^-25 itself is the tie, which goes to the even 0)
    for amax in (2.0 ** -25 * 127 * 0.999, 2.0 ** -25 * 127, 1e-12, -1e-12):
        got = kq.stored_q8(block([amax, -amax / 2, amax / 3]))
        assert np.array_equal(bits(got), np.zeros(32, np.uint32)), amax
    just = kq.stored_q8(block([2.0 ** -25 * 127 * 1.01, 0.0]))
    assert just[0] == np.float32(127.0) * np.float32(2.0 ** -24)             # the smallest f16 subnormal as d
    # f32-subnormal amax: d32 is subnormal or zero and id overflows to infinity (0 * inf = NaN among the products): DEFINED as all +0.0
    for amax in (1e-38, 1e-40, 1e-45, -1e-45):
        got = kq.stored_q8(block([amax, 0.0, -amax]))
        assert np.array_equal(bits(got), np.zeros(32, np.uint32)), amax
    # a NaN in a block: all 32 read back NaN; the neighbouring block is untouched
    two = np.concatenate([block([1.0, np.nan, 1e9, np.inf]), block([1.0, -127.0])])
    got = kq.stored_q8(two)
    assert np.isnan(got[:32]).all() and np.array_equal(got[32:34], [1.0, -127.0]) and not got[34:].any()
    # blocks lie along the last axis, whatever the leading shape
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, 5, 64)).astype(np.float32)
    assert np.array_equal(bits(kq.stored_q8(x)), bits(kq.stored_q8(x.reshape(-1, 32)).reshape(x.shape)))


def test_the_rule_is_ggml_s_and_idempotent_on_a_million_values():
    """random f32 values over all exponents whose block maxima fit an f16: (a) for finite inputs within +-65504 the values are those of
    ggml's quantize_row_q8_0_ref + dequantize_row_q8_0, restated independently here; (b) |q| <= 127 BEFORE the clamp; (c) every
    non-zero block contains +-127 * d; (d) quantising the stored values returns them bit for bit."""
    rng = np.random.default_rng(20261021)
    n = 1_048_576
    x = rng.integers(0, 0x47800000, n, dtype=np.int64).astype(np.uint32).view(np.float32)      # [0, 65536)
    x = np.minimum(x, np.float32(65504.0)) * rng.choice(np.array([-1, 1], np.float32), n)
    normal = (rng.standard_normal(n) * rng.choice([1e-3, 1.0, 300.0], n)).astype(np.float32)
    x = np.concatenate([x, normal]).reshape(-1, 32)
    assert x.size >= 2_000_000
    got = kq.stored_q8(x)
    with np.errstate(all="ignore"):
        amax = np.abs(x).max(axis=1)
        d32 = amax / np.float32(127.0)
        inv = np.where(d32 != 0, np.float32(1.0) / d32, np.float32(0)).astype(np.float32)
        p = (x * inv[:, None]).astype(np.float32)
        q = np.where(p < 0, np.ceil(p.astype(np.float64) - 0.5), np.floor(p.astype(np.float64) + 0.5))      # roundf
        d = d32.astype(np.float16).astype(np.float32)
        ggml = (np.nan_to_num(q).astype(np.int8).astype(np.float32) * d[:, None]).astype(np.float32)
    live = d != 0
    assert live.sum() > 0.9 * len(d)
    assert np.abs(q[live]).max() == 127.0                                                 # (b)
    assert np.array_equal(bits(got[live]), bits(ggml[live]))                              # (a)
    assert not got[~live].any()
    assert (np.abs(got[live]).max(axis=1) == np.float32(127.0) * d[live]).all()           # (c)
    assert np.array_equal(bits(kq.stored_q8(got)), bits(got)) and kq.idempotent(got)      # (d)
    assert not kq.idempotent(x)                                                           # (what is not q8_0 is told apart)
    assert not kq.idempotent(np.full(32, np.nan, np.float32))


# ---- the yardstick and the movement ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(shape):
    """(weights, tokens, forward_all's logits, the quantising pass's logits and its quantised rows K, V), computed once"""
    s = gguf.SHAPES[shape]
    fw = gguf.synth_fused(s, 777)
    n = min(N_POS, s.seq_len)
    rng = np.random.default_rng(5)
    tokens = np.array([2] + (rng.integers(3, s.vocab_size, n - 1) + 1).tolist())
    logits, _ = an.forward_all(fw, tokens)
    qlogits, K, V = kq.forward_quantised(fw, tokens)
    for a in (logits, qlogits, K, V):
        a.setflags(write=False)
    return fw, tokens, logits, qlogits, K, V


def movement(shape):
    """how far quantising the K/V rows moves the logits of `shape`, of max |logit| (the worst position)"""
    _, _, logits, qlogits, _, _ = reference(shape)
    return float(rel_err(qlogits, logits).max())


@pytest.mark.parametrize("shape", MODELS)
def test_forward_fed_the_reference_s_own_quantised_rows_is_the_quantising_pass(shape):
    fw, tokens, logits, qlogits, K, V = reference(shape)
    assert kq.idempotent(K) and kq.idempotent(V)
    fed = kq.forward_fed(fw, tokens, K, V)
    err = rel_err(fed, qlogits).max()
    print(f"{shape}: forward_fed on the quantising pass's own q8_0 rows: rel_err {err:.2e}")
    assert err <= REL_TOL
    assert err <= 1e-11            # (the same float64 arithmetic on the same rows)


@pytest.mark.parametrize("shape", MODELS)
def test_movement_of_the_logits_under_q8_0_rows(shape):
    """the figure of include/llmk.h's parity table: far above REL_TOL (the oracle cannot judge a q8_0 batch, and a pass that ignored
    the stored rows could not meet forward_fed), and still the same model"""
    mv = movement(shape)
    print(f"{shape}: q8_0 K/V rows move the logits by {mv:.2e} of max |logit| ({min(N_POS, gguf.SHAPES[shape].seq_len)} positions, seed 777)")
    assert 20 * REL_TOL < mv < 5e-2


# ---- header, bindings, host -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    llmk.build_lib()
    return llmk.lib()


def test_header_and_bindings_name_the_type(lib):
    hdr = open(os.path.join(ROOT, "include", "llmk.h")).read()
    assert re.search(r"^#define LLMK_TYPE_Q8_0 8\b", hdr, re.M)
    assert llmk.KV_TYPES == {"f32": 0, "f16": 1}
    assert llmk.KV_CACHE_TYPES == {"f32": 0, "f16": 1, "q8_0": 8}
    assert lib.llmk_version() >= 409
    with pytest.raises(ValueError, match="q8_0"):
        llmk.Batch(types.SimpleNamespace(V=1, _h=None), 2, 16, kv_type="q4_0")
    f90 = open(os.path.join(ROOT, "llm.f90_amd", "host", "llmk_binding.f90")).read()
    assert "8 = q8_0" in f90
    host = open(os.path.join(ROOT, "llm.f90_amd", "host", "llm.f90")).read()
    usage = [l for l in host.splitlines() if l.startswith("!") and "[--parallel N" in l]      # the usage line of the file's head
    assert len(usage) == 1 and "[--kv-f16 | --kv-q8]" in usage[0], usage
    assert 'case ("--kv-q8")' in host


def test_null_handles_are_refused_without_a_device_for_kv_type_8(lib):
    out = C.c_void_p()
    assert lib.llmk_cache_create(None, 2, 16, 8, C.byref(out)) == 1 and not out.value
    assert lib.llmk_cache_create(None, 2, 16, 8, None) == 1
    assert lib.llmk_cache_type(None) == -1
    n = C.c_ulonglong(7)
    assert lib.llmk_cache_bytes(None, C.byref(n)) == 1 and n.value == 7
    row = np.zeros(64, np.float32)
    assert lib.llmk_cache_peek(None, 0, 0, 0, 1, 1, row.ctypes.data_as(C.POINTER(C.c_float))) == 1


def test_the_q8_0_attention_kernels_fit_the_occupancy_steps_of_their_head_size():
    """tests/host_tools/tk_resources.py --all, once: the four q8_0 attention kernels at the four head sizes have no scratch and VGPRs
    within the cap tests/test_build_cpu.py holds the f32 and f16 kernels of that head size to; the K/V write and the converting copy
    have no scratch either.  (The 28 existing lines are that file's.)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_tools", "tk_resources.py"), "--all"], capture_output=True, text=True,
                       timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    cap = {16: 64, 32: 80, 64: 128, 128: 256}
    head = re.compile(r"bd_q8_attn_(|prefix_|own_|span_)kernel<(\d+)>")
    seen = set()
    for l in r.stdout.splitlines():
        m, k = head.match(l), re.search(r"VGPR\s+(\d+).*scratch\s+(\d+)", l)
        if m:
            print(l)
            assert k and int(k.group(2)) == 0 and int(k.group(1)) <= cap[int(m.group(2))], l
            seen.add((m.group(1), int(m.group(2))))
        elif l.startswith(("bd_epi_qkv_q8_kernel", "bd_to_q8_kernel")):
            assert k and int(k.group(2)) == 0, l
            seen.add(l.split("(")[0])
    assert seen == {(k, hs) for k in ("", "prefix_", "own_", "span_") for hs in cap} | {"bd_epi_qkv_q8_kernel", "bd_to_q8_kernel"}, seen
