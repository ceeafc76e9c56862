"""Weight-format edge inputs: every legal q6_K, q4_0 and f16 encoding, class by class (helper module, not a conftest).

What the suite's own quantisers emit is a thin slice of what a file may hold (quantize_q6_K: scales 1..127, d > 0 and
subnormal; quantize_q4_0 / synth_q4_rows: |d| of one typical size, dense random nibbles; f16: no +-0, hardly a subnormal).
Here the raw rows of a matrix [rows][K] are CRAFTED in the block formats themselves, one class of encodings per row:

    class of row r = SLOTS[r % n]          (n is odd: every CU, wave and row slot of every kernel meets every class)
    class of row r = SLOTS[(r // 2) % n]   in the Q and K rows of wqkv: RoPE turns the pair (2j, 2j + 1) into each other, so a
                                           tiny row beside an ordinary one could not be read out row by row

and every check is made WITHIN a class (class_err), so a class of rows with small logits cannot hide behind the largest logit
of the position -- the whole-position bar of conftest.rel_err stays beside it.

Classes (names below).  An "equal-magnitude" class is one whose d can be chosen so that the decoded row has rms 1/sqrt(K), what
synth_tensor gives: they may go anywhere and their d IS chosen that way (every block or super-block with its own jitter 0.5..1.5
and its own sign, so a mis-indexed d shows).  q6_K class (a) asks for a NORMAL d with full-range scales: its rows are larger
than 1/sqrt(K) from K = 512 on (d >= 2^-14), which only a classifier row can be -- q6_K rows are classifier rows.
"Tiny by nature" are the rows of subnormal d, of d = 0, of zero weights and of subnormal f16 weights: they go only into
classifier rows and into the K and V rows of wqkv, where each row's product can be read out by itself (logits, KV cache);
elsewhere their slots hold the format's plain class.

LIMIT: this is a DECODING suite.  |w| <= 8 everywhere, no infinite or NaN d, |d| <= 1: it injects no faults and does not redo
the activation-range tests (test_parity_gpu.py: activations beyond f16, small xb / hb).

The reference is forward64: the float64 pass of tests/ref_pass.py on the decoded weights, to which it adds the read-out of the
K / V rows of every layer and of the last layer's q, xb, hb and x.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from conftest import REL_TOL, rel_err
from ref_pass import RefPass

Q6K_BYTES, Q4_BYTES = 210, 18
H_2M24, H_SUBMAX, H_MINNORM = 0x0001, 0x03FF, 0x0400      # f16 bits: 2^-24, 2^-14 - 2^-24, 2^-14
SIGN = 0x8000
SCALE_VALUES = np.array([-128, -127, -64, -1, 0, 1, 63, 127], np.int8)


# ----------------------------------------------------------------------------------------------------------------------
# scalar decoders: plain loops from the format statements (csrc/q6k.h:9-12, csrc/q4_units.h:4-5); nothing from tools/gguf.py
# ----------------------------------------------------------------------------------------------------------------------
def f16_scalar(bits) -> np.float32:
    """IEEE binary16 bit pattern -> its exact f32 value, from the fields"""
    bits = int(bits)
    s, e, m = bits >> 15, (bits >> 10) & 31, bits & 1023
    if e == 0:
        v = m * 2.0 ** -24
    elif e == 31:
        v = float("inf") if m == 0 else float("nan")
    else:
        v = (1024 + m) * 2.0 ** (e - 25)
    return np.float32(-v if s else v)


def f16_row_scalar(bits_row) -> np.ndarray:
    return np.array([f16_scalar(b) for b in np.asarray(bits_row).reshape(-1)], np.float32)


def q6k_scalar(row, K: int) -> np.ndarray:
    """one row of K / 256 super-blocks (ql[128] | qh[64] | int8 scales[16] | f16 d):
    weight(128 n + 32 k + l) = d * scales[8 n + 2 k + l / 16] * (q - 32), left to right in f32"""
    row = [int(b) for b in np.asarray(row, np.uint8).reshape(-1)]
    out = np.zeros(K, np.float32)
    for sb in range(K // 256):
        blk = row[sb * Q6K_BYTES:(sb + 1) * Q6K_BYTES]
        ql, qh, sc = blk[0:128], blk[128:192], blk[192:208]
        d = f16_scalar(blk[208] | (blk[209] << 8))
        for n in range(2):
            for k in range(4):
                for l in range(32):
                    byte = ql[64 * n + 32 * (k & 1) + l]
                    nib = (byte & 15) if k < 2 else (byte >> 4)
                    q = nib | (((qh[32 * n + l] >> (2 * k)) & 3) << 4)
                    s = sc[8 * n + 2 * k + l // 16]
                    s = s - 256 if s >= 128 else s                                   # int8
                    out[256 * sb + 128 * n + 32 * k + l] = np.float32(d * np.float32(s)) * np.float32(q - 32)
    return out


def q4_0_scalar(row, K: int) -> np.ndarray:
    """one row of K / 32 blocks (f16 d | 16 bytes): low nibbles are elements 0..15, high nibbles 16..31, value (nibble - 8) d"""
    row = [int(b) for b in np.asarray(row, np.uint8).reshape(-1)]
    out = np.zeros(K, np.float32)
    for b in range(K // 32):
        blk = row[b * Q4_BYTES:(b + 1) * Q4_BYTES]
        d = f16_scalar(blk[0] | (blk[1] << 8))
        for i in range(16):
            out[32 * b + i] = np.float32((blk[2 + i] & 15) - 8) * d
            out[32 * b + 16 + i] = np.float32((blk[2 + i] >> 4) - 8) * d
    return out


# ----------------------------------------------------------------------------------------------------------------------
# seeded values (a counter hash: the same bytes on every machine)
# ----------------------------------------------------------------------------------------------------------------------
def _hash(seed: int, stream: int, n: int) -> np.ndarray:
    base = np.uint64(((seed * 0x9E3779B1 + stream * 0x85EBCA77) & 0xFFFFFFFF) << 32)
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + base + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _bytes(seed, stream, n) -> np.ndarray:
    return _hash(seed, stream, (n + 7) // 8).view(np.uint8)[:n]


def _ints(seed, stream, shape, lo, hi) -> np.ndarray:
    """integers lo..hi inclusive"""
    n = int(np.prod(shape))
    return ((_hash(seed, stream, n) >> np.uint64(24)) % np.uint64(hi - lo + 1)).astype(np.int64).reshape(shape) + lo


def _unit(seed, stream, shape) -> np.ndarray:
    n = int(np.prod(shape))
    return ((_hash(seed, stream, n) >> np.uint64(40)).astype(np.float64) / (1 << 24)).reshape(shape)


def _row_classes(rows: int, slots, pair: bool):
    """(class id [rows], index of the row within its class j [rows])"""
    r = np.arange(rows)
    n = len(slots)
    assert n % 2 == 1
    u = r // 2 if pair else r
    j = (u // n) * 2 + (r & 1) if pair else u // n
    return np.asarray(slots)[u % n], j


def _f16_bits(x) -> np.ndarray:
    return np.asarray(x, np.float64).astype(np.float16).view(np.uint16)


# ----------------------------------------------------------------------------------------------------------------------
# q6_K
# ----------------------------------------------------------------------------------------------------------------------
Q6K_CLASSES = ("a:ggml d<0 normal, scales -128..-1", "b:free", "c:scale values", "d:one live sub-block", "e:q all 0 / all 63 / 0,63",
               "f1:|d| = 2^-24", "f2:|d| = 2^-14 - 2^-24, 2^-14", "g:q = 32 (zero weights)", "h:d = 0")
Q6K_TINY = (5, 6, 7, 8)
Q6K_ZERO = (7, 8)


def pack_q6k(q, sc, dbits) -> np.ndarray:
    """q [rows][nsb][256] 0..63, sc [rows][nsb][16] int8, dbits [rows][nsb] f16 bits -> uint8 [rows][nsb * 210]"""
    rows, nsb = dbits.shape
    q = q.reshape(rows, nsb, 2, 4, 32).astype(np.uint8)
    out = np.empty((rows, nsb, Q6K_BYTES), np.uint8)
    ql = out[:, :, 0:128].reshape(rows, nsb, 2, 64)
    ql[..., 0:32] = (q[:, :, :, 0] & 15) | ((q[:, :, :, 2] & 15) << 4)
    ql[..., 32:64] = (q[:, :, :, 1] & 15) | ((q[:, :, :, 3] & 15) << 4)
    out[:, :, 0:128] = ql.reshape(rows, nsb, 128)
    qh = (q[:, :, :, 0] >> 4) | ((q[:, :, :, 1] >> 4) << 2) | ((q[:, :, :, 2] >> 4) << 4) | ((q[:, :, :, 3] >> 4) << 6)
    out[:, :, 128:192] = qh.reshape(rows, nsb, 64)
    out[:, :, 192:208] = sc.astype(np.int8).view(np.uint8)
    out[:, :, 208] = (dbits & 0xFF).astype(np.uint8)
    out[:, :, 209] = (dbits >> 8).astype(np.uint8)
    return out.reshape(rows, nsb * Q6K_BYTES)


def craft_q6k(rows: int, K: int, seed: int, pair: bool = False):
    """(raw uint8 [rows][K / 256 * 210], class id [rows]) -- q6_K rows are classifier rows: every class, tiny ones included"""
    assert K % 256 == 0
    nsb = K // 256
    cls, j = _row_classes(rows, range(len(Q6K_CLASSES)), pair)
    q = (_bytes(seed, 1, rows * nsb * 256) & 63).astype(np.int8).reshape(rows, nsb, 256)
    sc = _bytes(seed, 2, rows * nsb * 16).view(np.int8).astype(np.int16).reshape(rows, nsb, 16)
    jit = 0.5 + _unit(seed, 3, (rows, nsb))
    sgn = np.where(_ints(seed, 4, (rows, nsb), 0, 1) == 1, -1.0, 1.0)
    J = j[:, None]
    sbi = np.arange(nsb)[None, :]
    sub = np.arange(16)[None, None, :]

    m = cls == 0                                                            # (a) what ggml's quantiser emits
    sc[m] = -1 - (sc[m] & 127)
    m = cls == 2                                                            # (c) every special scale value on every sub-block
    sc[m] = np.broadcast_to(SCALE_VALUES[(sub + J[:, :, None] + 3 * sbi[:, :, None]) % 8], sc.shape)[m]
    m = cls == 3                                                            # (d) one live sub-block in one live super-block
    live_sub, live_sb = j % 16, (j // 16) % nsb
    live_val = np.array([-128, -127, -64, -1, 1, 63, 127])[j % 7]
    one = np.where((sub == live_sub[:, None, None]) & (sbi[:, :, None] == live_sb[:, None, None]), live_val[:, None, None], 0)
    sc[m] = one[m]
    m = cls == 4                                                            # (e) the extreme codes
    alt = np.where((np.arange(256)[None, None, :] + J[:, :, None]) % 2 == 0, 0, 63)
    pat = np.where((J % 3 == 0)[:, :, None], 0, np.where((J % 3 == 1)[:, :, None], 63, alt))
    q[m] = np.broadcast_to(pat, q.shape)[m]
    q[cls == 7] = 32                                                        # (g) every weight exactly 0

    # d: the equal-magnitude choice, rms of the decoded row = 1 / sqrt(K)
    q2 = ((q.astype(np.int32) - 32) ** 2).reshape(rows, nsb, 16, 16).sum(axis=3)             # per sub-block: sum (q - 32)^2
    S = np.sqrt(((sc.astype(np.float64) ** 2 * q2).sum(axis=2) * jit ** 2).sum(axis=1) / K)
    d = jit * sgn / (np.sqrt(K) * np.where(S > 0, S, 1.0))[:, None]
    dbits = _f16_bits(d)
    m = cls == 0                                                            # (a) negative and NORMAL
    dbits[m] = _f16_bits(-np.maximum(np.abs(d), 2.0 ** -14 * (0.5 + jit)))[m]
    assert np.all((dbits[m] & 0x7C00) != 0)
    m = cls == 3                                                            # (d) the dead super-blocks keep a d of their own
    dbits[m] = np.where(sbi == live_sb[:, None], dbits, _f16_bits(0.01 * jit * sgn))[m]
    small = np.array([H_2M24, H_2M24 | SIGN])[(J + sbi) % 2]
    dbits[cls == 5] = np.broadcast_to(small, dbits.shape)[cls == 5]
    small = np.array([H_SUBMAX, H_SUBMAX | SIGN, H_MINNORM, H_MINNORM | SIGN])[(J + sbi) % 4]
    dbits[cls == 6] = np.broadcast_to(small, dbits.shape)[cls == 6]
    m = cls == 7
    dbits[m] = _f16_bits(0.01 * jit * sgn)[m]
    dbits[cls == 8] = np.broadcast_to(np.array([0, SIGN])[(J + sbi) % 2], dbits.shape)[cls == 8]   # (h) +0 and -0
    return pack_q6k(q, sc, dbits.astype(np.uint16)), cls


# ----------------------------------------------------------------------------------------------------------------------
# q4_0
# ----------------------------------------------------------------------------------------------------------------------
Q4_CLASSES = ("t0:d = +-0", "t1:|d| = 2^-24", "t2:|d| = 2^-14 - 2^-24, 2^-14", "typical d, both signs", "constant-nibble blocks",
              "one block in three at d = 0", "one live block")
Q4_TINY = (0, 1, 2)
Q4_ZERO = (0,)
Q4_PLAIN = 3
CONST_BYTES = np.array([[0x00] * 16, [0x88] * 16, [0xFF] * 16, [0x00, 0xFF] * 8, [0xF0] * 16, [0x0F] * 16], np.uint8)   # all 0, 8, 15; 0/15 by element; by half


_NIB2 = ((np.arange(256) & 15) - 8.0) ** 2 + ((np.arange(256) >> 4) - 8.0) ** 2


def craft_q4_0(rows: int, K: int, seed: int, tiny_ok: bool, pair: bool = False):
    """(raw uint8 [rows][K / 32 * 18], class id [rows])"""
    assert K % 32 == 0
    nb = K // 32
    slots = [c if (tiny_ok or c not in Q4_TINY) else Q4_PLAIN for c in range(len(Q4_CLASSES))]
    cls, j = _row_classes(rows, slots, pair)
    qs = _bytes(seed, 11, rows * nb * 16).reshape(rows, nb, 16).copy()
    jit = 0.5 + _unit(seed, 12, (rows, nb))
    sgn = np.where(_ints(seed, 13, (rows, nb), 0, 1) == 1, -1.0, 1.0)
    J, bi = j[:, None], np.arange(nb)[None, :]
    m = cls == 4
    qs[m] = CONST_BYTES[_ints(seed, 14, (rows, nb), 0, len(CONST_BYTES) - 1)][m]
    live = (cls == 6)[:, None] & (bi == (J % nb))
    dead = (cls == 6)[:, None] & ~live
    dead8 = dead & (J % 2 == 1)                                            # odd rows: the dead blocks keep a d and hold nibbles 8
    qs[dead8] = 0x88
    zero_d = ((cls == 5)[:, None] & ((bi + J) % 3 == 0)) | (dead & ~dead8)
    n2 = _NIB2[qs].sum(axis=2)                                             # per block: sum (nibble - 8)^2
    S = np.sqrt((n2 * np.where(zero_d, 0.0, jit ** 2)).sum(axis=1) / K)
    d = jit * sgn / (np.sqrt(K) * np.where(S > 0, S, 1.0))[:, None]
    assert np.abs(d).max() * 8 <= 8.0
    dbits = _f16_bits(d)
    zbits = np.array([0, SIGN])[(J + bi) % 2]
    dbits = np.where(zero_d, zbits, dbits)
    dbits = np.where((cls == 0)[:, None], zbits, dbits)
    dbits = np.where((cls == 1)[:, None], np.array([H_2M24, H_2M24 | SIGN])[_ints(seed, 15, (rows, nb), 0, 1)], dbits)
    dbits = np.where((cls == 2)[:, None], np.array([H_SUBMAX, H_SUBMAX | SIGN, H_MINNORM, H_MINNORM | SIGN])[_ints(seed, 16, (rows, nb), 0, 3)], dbits)
    out = np.empty((rows, nb, Q4_BYTES), np.uint8)
    out[:, :, 0] = dbits & 0xFF
    out[:, :, 1] = dbits >> 8
    out[:, :, 2:] = qs
    return out.reshape(rows, nb * Q4_BYTES), cls


# ----------------------------------------------------------------------------------------------------------------------
# f16
# ----------------------------------------------------------------------------------------------------------------------
F16_CLASSES = ("all subnormal", "+-0 among normals", "dense, alternating sign", "one non-zero weight", "plain")
F16_TINY = (0,)
F16_PLAIN = 4


def craft_f16(rows: int, K: int, seed: int, tiny_ok: bool, pair: bool = False):
    """(float16 [rows][K], class id [rows])"""
    slots = [c if (tiny_ok or c not in F16_TINY) else F16_PLAIN for c in range(len(F16_CLASSES))]
    cls, j = _row_classes(rows, slots, pair)
    a = np.sqrt(3.0 / K)
    w = (2.0 * _unit(seed, 21, (rows, K)) - 1.0) * a                       # plain: what synth_tensor gives
    col = np.arange(K)[None, :]
    m = cls == 1
    w[m] = (np.where(_ints(seed, 22, (rows, K), 0, 1) == 1, w * np.sqrt(2.0), 0.0))[m]
    m = cls == 2
    mag = (0.5 + _unit(seed, 23, (rows, K))) / np.sqrt(K * 13.0 / 12.0)
    w[m] = (np.where((col + j[:, None]) % 2 == 0, mag, -mag))[m]
    m = cls == 3
    w[m] = (np.where(col == (j % K)[:, None], np.where(j % 2 == 0, 1.0, -1.0)[:, None], 0.0))[m]
    bits = _f16_bits(w)
    neg0 = _ints(seed, 24, (rows, K), 0, 1) == 1
    bits = np.where((bits == 0) & neg0 & np.isin(cls, (1, 3))[:, None], SIGN, bits)     # half of the zeros are -0
    sub = (_ints(seed, 25, (rows, K), 1, 1023) | np.where(neg0, SIGN, 0)).astype(np.uint16)
    bits = np.where((cls == 0)[:, None], sub, bits)
    return bits.astype(np.uint16).view(np.float16), cls


# ----------------------------------------------------------------------------------------------------------------------
# a model of crafted rows
# ----------------------------------------------------------------------------------------------------------------------
CLASS_NAMES = {1: F16_CLASSES, 2: Q4_CLASSES, 14: Q6K_CLASSES}
TOKENS = [2, 17, 400, 3, 277]      # teacher-forced, 1-based: the first 3 are the decode positions, all 5 the prefill / score batch


def craft_matrix(rows, K, wtype, seed, tiny_ok, pair=False):
    if wtype == 14:
        return craft_q6k(rows, K, seed, pair)
    if wtype == 2:
        return craft_q4_0(rows, K, seed, tiny_ok, pair)
    if wtype == 1:
        return craft_f16(rows, K, seed, tiny_ok, pair)
    raise ValueError(wtype)


def craft_model(gguf, shape, mat_type: int, cls_type: int, seed: int):
    """(FusedWeights, {matrix name: class id per row}) -- matrices of `mat_type` (1 f16, 2 q4_0), classifier of `cls_type` (also
    14: raw q6_K); embedding and norm gains as synth_fused gives them.  Tiny classes: classifier rows and K / V rows only."""
    s = shape
    E, H, L, KV, V = s.emb_dim, s.hidden_dim, s.n_layers, s.kv_dim, s.vocab_size
    idx = {n: i for i, (n, _, _) in enumerate(gguf.tensor_names(s))}
    fw = gguf.FusedWeights(s, mat_type)
    fw.token_embedding_table = gguf.synth_tensor(s, seed, idx["token_embd.weight"], (V, E), "emb")
    fw.rms_final_weight = gguf.synth_tensor(s, seed, idx["output_norm.weight"], (E,), "norm")
    fw.rms_att_weight = np.stack([gguf.synth_tensor(s, seed, idx[f"blk.{l}.attn_norm.weight"], (E,), "norm") for l in range(L)])
    fw.rms_ffn_weight = np.stack([gguf.synth_tensor(s, seed, idx[f"blk.{l}.ffn_norm.weight"], (E,), "norm") for l in range(L)])
    jobs = {"wcls": (V, E, cls_type, seed * 64 + 7, True, False)}
    for l in range(L):
        sd = seed * 64 + 8 * l
        jobs.update({("q", l): (E, E, mat_type, sd + 1, False, True), ("k", l): (KV, E, mat_type, sd + 2, True, True),
                     ("v", l): (KV, E, mat_type, sd + 3, True, False), ("wo", l): (E, E, mat_type, sd + 4, False, False),
                     ("w13", l): (2 * H, E, mat_type, sd + 5, False, False), ("w2", l): (E, H, mat_type, sd + 6, False, False)})
    with ThreadPoolExecutor(8) as ex:                       # (numpy releases the GIL: the large shapes build in a few seconds)
        done = dict(zip(jobs, ex.map(lambda a: craft_matrix(*a), jobs.values())))
    fw.wqkv = np.stack([np.concatenate([done[(p, l)][0] for p in "qkv"]) for l in range(L)])
    classes = {"wqkv": np.concatenate([done[(p, 0)][1] for p in "qkv"])}
    for name in ("wo", "w13", "w2"):
        setattr(fw, name, np.stack([done[(name, l)][0] for l in range(L)]))
        classes[name] = done[(name, 0)][1]
    fw.wcls, classes["wcls"] = done["wcls"]
    if cls_type != mat_type:
        fw.wcls_type = cls_type
    return fw, classes


# name -> ((E, H, n_heads, n_kv_heads, V), matrix type, classifier type): one layer each, the smallest shapes that reach each decoder
MODELS = {
    # V = 1002: the last block of gemv_q6k_kernel's 16 rows is ragged, and so is its last wave's group of 4 (the library takes even
    # vocabulary sizes only: row pairs, llmk_create_tp)
    "q6k-E256-f16": ((256, 512, 4, 2, 1002), 1, 14),           # gemv_q6k_kernel: one super-block, 4 live lanes
    "q6k-E1024-q4": ((1024, 2048, 8, 2, 1002), 2, 14),         # four super-blocks: the qd >> 1 and qd >> 2 indices
    "tinyllama-q4-q6k": ((2048, 5632, 32, 4, 32000), 2, 14),   # persistent kernel, q6 phase with half the lanes idle
    "llama7b-q4-q6k": ((4096, 11008, 32, 32, 32000), 2, 14),   # every lane live; H = 11008: the ragged q4_0 unit
    "tinyllama-q4": ((2048, 5632, 32, 4, 32000), 2, 2),        # the q4_0 classifier in the persistent kernel's units
    "tk-small-q4": ((256, 768, 4, 2, 1024), 2, 2),
    "tiny-70bish-q4": ((1024, 3584, 8, 1, 800), 2, 2),
    "tk-small16-f16": ((512, 1536, 8, 2, 1024), 1, 1),
}
_cache = {}


def decoded(gguf, fw):
    """fw.as_f32() with the classifier decoded a slice of rows per thread (a 32,000-row q6_K classifier: 2 s instead of 8)"""
    import dataclasses
    E, V = fw.shape.emb_dim, fw.shape.vocab_size
    wcls = np.empty((V, E), np.float32)

    def part(r0):
        wcls[r0:r0 + 1024] = gguf.decode(fw.wcls[r0:r0 + 1024], fw.cls_type, E)
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(part, range(0, V, 1024)))
    d = dataclasses.replace(fw, wcls=np.zeros((1, fw.wcls.shape[1]), fw.wcls.dtype)).as_f32()
    d.wcls = wcls
    return d


def model(gguf, name: str):
    """(FusedWeights, classes of the read-out rows, forward64 of TOKENS) of MODELS[name], built once per process"""
    if name not in _cache:
        (E, H, nh, nkv, V), mt, ct = MODELS[name]
        fw, classes = craft_model(gguf, gguf.LlamaShape(E, H, 1, nh, nkv, V, 64), mt, ct, 20261019)
        _cache[name] = (fw, row_classes(fw.shape, classes), forward64(decoded(gguf, fw), TOKENS))
    return _cache[name]


def row_classes(shape, classes):
    """the class of every row of what the tests read: logits, K and V cache rows, q, xb (the V row its head reads), hb (its gate
    row), x (its w2 row)"""
    s = shape
    E, H, KV, hs = s.emb_dim, s.hidden_dim, s.kv_dim, s.head_size
    c = classes["wqkv"]
    vrow = (np.arange(E) // hs // (s.n_heads // s.n_kv_heads)) * hs + np.arange(E) % hs
    return {"logits": classes["wcls"], "q": c[:E], "k": c[E:E + KV], "v": c[E + KV:], "xb": c[E + KV:][vrow],
            "hb": classes["w13"][:H], "x": classes["w2"]}


# ----------------------------------------------------------------------------------------------------------------------
# the reference: ref_pass.RefPass in float64, with the vectors the tests read out
# ----------------------------------------------------------------------------------------------------------------------
def forward64(fw, tokens, eps=1e-5):
    """ref_pass.RefPass (the model of oracle/llm_oracle.c) in float64 on DECODED weights (fw.as_f32()), tokens (1-based) at
    positions 1..n.  Returns logits [n][V], the K (rotated) and V cache rows k, v [L][n][KV], and of the LAST layer q (rotated),
    xb (attention output), hb (SwiGLU output) and x (residual stream behind the layer), each [n][.]."""
    p, n, out = RefPass(fw, eps=eps), len(tokens), {}

    def tap(l, name, a):
        if l == fw.shape.n_layers - 1 and name in ("q", "xb", "hb", "x"):
            out[name] = a.reshape(n, -1)
    out["logits"] = p.feed(tokens, tap=tap)
    out["k"], out["v"] = (np.stack([a.reshape(n, -1) for a in z]) for z in (p.k, p.v))
    return out


def class_err(got, ref, classes):
    """conftest.rel_err WITHIN each class: [positions][n_classes] of max |got - ref| / max |ref| over the rows of the class at
    that position (nan: no row of that class).  A class whose reference is exactly 0 at a position: max |got| over its rows /
    max |ref| of the whole position."""
    ref = np.asarray(ref, np.float64)
    ref = ref.reshape(-1, ref.shape[-1])
    got = np.asarray(got, np.float64).reshape(ref.shape)
    classes = np.asarray(classes)
    assert classes.shape == (ref.shape[1],)
    out = np.full((ref.shape[0], int(classes.max()) + 1), np.nan)
    whole = np.max(np.abs(ref), axis=1)
    for c in np.unique(classes):
        m = classes == c
        diff = np.max(np.abs(got[:, m] - ref[:, m]), axis=1)
        scale = np.max(np.abs(ref[:, m]), axis=1)
        out[:, c] = diff / np.where(scale > 0, scale, whole)
    return out


def worst(err) -> float:
    return float(np.nanmax(err))


class Report:
    """collects class_err of every (quantity, position); fails at the end with every red class named"""

    def __init__(self, label):
        self.label, self.worst, self.where, self.red = label, {}, {}, []

    def add(self, what, pos, got, ref, classes, names=None):
        e = class_err(got, ref, classes)[0]
        for c in np.unique(classes):                 # (a class without a row is nan in e and is not asked about)
            name = names[c] if names else str(c)
            if not e[c] <= REL_TOL:                  # a NaN or an infinity in the class's output is red as well
                self.red.append((what, pos, name, float(e[c])))
            if not e[c] < self.worst.get(what, -1.0):
                self.worst[what], self.where[what] = float(e[c]), name.split(":")[0]

    def whole(self, pos, got, ref):
        e = float(rel_err(got[None], ref[None])[0])
        if not e < self.worst.get("whole", -1.0):
            self.worst["whole"] = e
        if not e <= REL_TOL:
            self.red.append(("whole position", pos, "-", e))

    def finish(self):
        print("EDGE %-44s" % self.label, " ".join("%s %.1e" % kv for kv in self.worst.items()),
              "| worst logits class: %s" % self.where.get("logits"))
        assert not self.red, (self.label, self.red)
