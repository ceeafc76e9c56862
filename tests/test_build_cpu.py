"""Build-time guards that need no GPU: hipcc cross-compiles for gfx950 here."""
import os
import re
import subprocess
import sys

from conftest import ROOT


def test_persistent_kernels_do_not_spill():
    """The persistent token kernels sit at the 256-VGPR ceiling on purpose (register tile ring).  A spill in a streaming
    wave costs one `s_waitcnt vmcnt(0)` + scratch store per ring slot -- the whole prefetch ring drains -- and hipcc's
    allocation at the ceiling flips on unrelated edits (round 3: `if (a.gflags & 16)` instead of `if (a.herr)` in the
    service wave put 36 bytes of scratch into the f32 kernel's streaming loop).  So, checked on every build: no scratch
    instruction inside a loop, and at most 32 bytes of scratch at all (the f32 kernel currently keeps one 16-byte value
    across its straight-line classifier tail: one store, one reload per token, measured faster than the spill-free
    neighbours of the same schedule -- DESIGN.md section 3b)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_tools", "tk_resources.py"), "--all", "--lds64"], capture_output=True, text=True,
                       timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    # the prefill GEMMs on the f16 matrix instruction hold a ring of weight stages, two activation stages and 64 accumulators
    # per wave in (unified) registers: they must not spill at all (a first q4_0 version did: prefill.h)
    gemm = [l for l in r.stdout.splitlines() if "pf_gemm_h_kernel" in l]
    assert len(gemm) >= 48, len(gemm)
    for l in gemm:
        m = re.search(r"scratch\s+(\d+)", l)
        assert m and int(m.group(1)) == 0, l
    rows = [l for l in r.stdout.splitlines() if "token_kernel" in l or "tk2" in l]
    assert len(rows) >= 5, r.stdout
    # the f32 / f16 kernels' rmsnorm staging in 16-byte LDS accesses (round 5: hipcc once split them in pairs of 8: +7 % on the f16 token)
    for l in rows:
        if ", 0, -1>" in l or ", 1, -1>" in l:   # weight types f32 / f16 (TkShape<..., WT, CLS>)
            k = re.search(r"lds64 (-?\d+)/(-?\d+)", l)
            assert k and 0 <= int(k.group(1)) <= 4 and 0 <= int(k.group(2)) <= 4, l
    for l in rows:
        m = re.search(r"VGPR\s+(\d+).*scratch\s+(\d+)", l)
        assert m, l
        assert int(m.group(1)) <= 256, l
        if int(m.group(2)):
            assert int(m.group(2)) <= 32, l
            k = re.search(r"scratch_ops_in_loops (-?\d+) of (\d+)", l)
            assert k and int(k.group(1)) == 0 and int(k.group(2)) <= 4, l
    # the MFMA attention kernels (csrc/attn_tiles.h behind pf_attn_kernel and bd_attn_{,prefix_,own_}kernel): no scratch, and every
    # instantiation inside the occupancy step it had with the tile loop written out per kernel.  Registers are allocated 8 at a time
    # and waves per SIMD are min(8, 512 // allocation): head size 16 at 58 VGPRs at most -> 64, 32 at 76 -> 80, 64 at 118 -> 128,
    # 128 at 194 -> 256
    cap = {16: 64, 32: 80, 64: 128, 128: 256}
    # (a line starts with the kernel's name and head size: "bd_attn_kernel<64, float>(", or still mangled where the demangler does
    # not know _Float16: "_ZN4llmk14bd_attn_kernelILi64EDF16_EE")
    head = re.compile(r"(?:_ZN4llmk\d+)?(?:pf_attn_kernel|bd_attn_(?:prefix_|own_)?kernel)(?:<|ILi)(\d+)")
    attn = [l for l in r.stdout.splitlines() if head.match(l)]
    assert len(attn) == 4 * (1 + 3 * 2), attn                    # 4 head sizes; the batch's three kernels for f32 and f16 caches
    for l in attn:
        m = re.search(r"VGPR\s+(\d+).*scratch\s+(\d+)", l)
        assert m and int(m.group(2)) == 0 and int(m.group(1)) <= cap[int(head.match(l).group(1))], l
    fold = [l for l in r.stdout.splitlines() if l.startswith("bd_attn_fold_kernel<")]
    assert len(fold) == 4, fold
    for l in fold:
        m = re.search(r"scratch\s+(\d+)", l)
        assert m and int(m.group(1)) == 0, l


def _code_of(name):
    """[(line number, the line without its // comment)] of a file of csrc/"""
    with open(os.path.join(ROOT, "llm.f90_amd", "csrc", name)) as f:
        return [(n, line.split("//", 1)[0]) for n, line in enumerate(f, 1)]


def test_the_mfma_attention_is_written_once_and_in_one_named_exception():
    """pf_attn_kernel (prefill.h), bd_attn_prefix_kernel and bd_attn_own_kernel (batch.h) are setup around ONE tile loop, ONE merge of
    the waves and ONE look-ahead load per cache type, all in csrc/attn_tiles.h.  bd_attn_kernel alone keeps those statements written
    out, because on the shared text its f32 instantiation measured slower (the reason stands at the kernel and in DESIGN.md 3i).
    Outside comments: batch.h spells an MFMA builtin, defines a *_ATT_LOAD macro and spells the running softmax's rescale inside
    bd_attn_kernel's body only -- one macro, one rescale -- prefill.h spells no MFMA builtin below its GEMM kernels and no such macro,
    no other header has either, and llmk.hip reaches attn_tiles.h."""
    csrc = os.path.join(ROOT, "llm.f90_amd", "csrc")
    batch = _code_of("batch.h")
    first = next(n for n, c in batch if "void bd_attn_kernel(" in c)
    last = next(n for n, c in batch if n > first and c.startswith("}"))              # the kernel's closing brace
    pf = _code_of("prefill.h")
    below = next(n for n, c in pf if "PF_ATT_WAVES =" in c)
    assert any("__builtin_amdgcn_mfma" in c for n, c in pf if n < below)              # (the GEMMs' own stay where they are)
    hits = [f"prefill.h:{n}: {c.strip()}" for n, c in pf if n > below and "__builtin_amdgcn_mfma" in c]
    macros, rescale = [], []
    for name in sorted(f for f in os.listdir(csrc) if f.endswith(".h")):
        for n, c in _code_of(name):
            inside = name == "batch.h" and first < n < last
            if name == "batch.h" and "__builtin_amdgcn_mfma" in c and not inside:
                hits.append(f"{name}:{n}: {c.strip()}")
            if re.search(r"#\s*define\s+\w*_ATT_LOAD\b", c):
                (macros if inside else hits).append(f"{name}:{n}: {c.strip()}")
            if "expf(m_run - m_new)" in c:
                (rescale if inside or name == "attn_tiles.h" else hits).append(f"{name}:{n}")
    assert not hits, "\n".join(hits)
    assert len(macros) == 1, macros
    assert sorted(r.split(":")[0] for r in rescale) == ["attn_tiles.h", "batch.h"], rescale
    seen = set()
    _quoted_includes(os.path.join(csrc, "llmk.hip"), seen)
    assert os.path.normpath(os.path.join(csrc, "attn_tiles.h")) in seen


def _quoted_includes(path, seen):
    """every file reachable from `path` through #include "..." lines (relative to the including file)"""
    path = os.path.normpath(path)
    if path in seen:
        return
    seen.add(path)
    for line in open(path):
        m = re.match(r'\s*#\s*include\s+"([^"]+)"', line)
        if m:
            _quoted_includes(os.path.join(os.path.dirname(path), m.group(1)), seen)


def test_every_included_header_is_a_prerequisite_of_the_libraries():
    """Round-5 verdict, build hygiene: csrc/q4_units.h (included by token_kernel.h) was not among libllmk.so's prerequisites, so
    an edit of the unit layout alone left a stale library.  Walk the #include "..." graph of llmk.hip and hold the Makefile's
    list (`make print-lib-deps`) to it; both library rules must use that list."""
    pkg = os.path.join(ROOT, "llm.f90_amd")
    r = subprocess.run(["make", "-s", "-C", pkg, "print-lib-deps"], capture_output=True, text=True, check=True)
    deps = {os.path.normpath(os.path.join(pkg, d)) for d in r.stdout.split()}
    seen = set()
    _quoted_includes(os.path.join(pkg, "csrc", "llmk.hip"), seen)
    assert len(seen) >= 7, seen
    missing = sorted(s for s in seen if s not in deps)
    assert not missing, f"not prerequisites of libllmk.so: {missing}"
    mk = open(os.path.join(pkg, "Makefile")).read()
    assert re.search(r"^csrc/libllmk\.so: \$\(LIB_DEPS\)$", mk, re.M) and re.search(r"^csrc/libllmk_debug\.so: \$\(LIB_DEPS\)$", mk, re.M)


def test_scratch_words_are_addressed_through_their_structs():
    """The words behind the logits vectors, the pinned next-token block and the q4_0 scale records have ONE definition
    (csrc/scratch_layout.h, token_kernel.h tk_qsc_front / TK_QSC_GRANULES; its static_asserts hold the bytes in place at build time).
    No hand-computed offset may come back into the shim or the token kernel: outside comments, neither file spells
    `d_logits + V`, `[c->V]`, `h_next[1]`, `h_next + 2` ... or `tk_ngran - 4 * ...` again."""
    raw = re.compile(r"(h_logits(_dev)?|d_logits) \+ (c->)?V\b|\[(c->)?V\]|h_next \+ \d|h_next\[\d\]|tk_ngran - 4")
    hits = []
    for name in ("llmk.hip", "token_kernel.h"):
        for n, line in enumerate(open(os.path.join(ROOT, "llm.f90_amd", "csrc", name)), 1):
            code = line.split("//", 1)[0]
            if raw.search(code):
                hits.append(f"{name}:{n}: {line.strip()}")
    assert not hits, "\n".join(hits)


def test_the_shim_allocates_and_releases_through_its_owners_only():
    """What the shim allocates or creates is held by the move-only owners of csrc/owned.h, whose destructors release it: no hand-kept
    teardown list can fall behind a new field again.  Outside comments, llmk.hip spells none of the runtime's allocate / create /
    free / destroy calls (as a substring: the ...WithFlags and ...Async forms are meant too); owned.h does, and llmk.hip reaches it."""
    calls = ("hipMalloc", "hipHostMalloc", "hipFree", "hipHostFree", "hipEventCreate", "hipEventDestroy", "hipStreamCreate", "hipStreamDestroy")
    csrc = os.path.join(ROOT, "llm.f90_amd", "csrc")

    def code(name):
        return [(n, line.split("//", 1)[0]) for n, line in enumerate(open(os.path.join(csrc, name)), 1)]
    hits = [f"llmk.hip:{n}: {c.strip()}" for n, c in code("llmk.hip") for w in calls if w in c]
    assert not hits, "\n".join(hits)
    owned = "\n".join(c for _, c in code("owned.h"))
    missing = [w for w in calls if not re.search(r"\b%s(WithFlags)?\b" % w, owned)]
    assert not missing, f"owned.h never names {missing}"
    seen = set()
    _quoted_includes(os.path.join(csrc, "llmk.hip"), seen)
    assert os.path.normpath(os.path.join(csrc, "owned.h")) in seen


def test_the_sticky_error_word_has_one_vocabulary_and_one_policy():
    """The persistent kernel's sticky error word is spelled in csrc/tk_recover.h alone, and the host's reaction to it is that
    header's TkRecovery, carried out by llmk.hip's tk_perform.  Outside comments, neither llmk.hip nor token_kernel.h spells the
    word's marks as literals again; llmk.hip declares none of the four loose fields the policy replaced; and it takes a context
    off the kernel in two places only -- tk_perform and llmk_set_tensor_type (no `use_tk = false; ... use_tk = true;` around a
    launch: enqueue_token takes the path as an argument)."""
    csrc = os.path.join(ROOT, "llm.f90_amd", "csrc")

    def code(name):
        return [(n, line.split("//", 1)[0]) for n, line in enumerate(open(os.path.join(csrc, name)), 1)]
    literal = re.compile(r"\b0x0*(2000|4000|2f00|1000)u?\b", re.I)
    hits = [f"{name}:{n}: {c.strip()}" for name in ("llmk.hip", "token_kernel.h") for n, c in code(name) if literal.search(c)]
    assert not hits, "\n".join(hits)
    shim = code("llmk.hip")
    fields = re.compile(r"\b(tk_range_run|tk_range_events|tk_retired|tk_qsc_pos)\b")
    hits = [f"llmk.hip:{n}: {c.strip()}" for n, c in shim if fields.search(c)]
    assert not hits, "\n".join(hits)
    # the two assignments, each inside the function that may make it (the last function header above the line)
    header = re.compile(r"^(?:static )?(?:int|hipError_t|bool|void|unsigned) (\w+)\(")
    owner, owners = None, []
    for n, c in shim:
        m = header.match(c)
        owner = m.group(1) if m else owner
        if re.search(r"\buse_tk\s*=\s*false\b", c) and not re.match(r"\s*bool use_tk = false;", c):
            owners.append(owner)
    assert sorted(owners) == ["llmk_set_tensor_type", "tk_perform"], owners
    for name in ("llmk.hip", "token_kernel.h"):
        seen = set()
        _quoted_includes(os.path.join(csrc, name), seen)
        assert os.path.normpath(os.path.join(csrc, "tk_recover.h")) in seen, name
