"""GGUF writer / reader and deterministic synthetic Llama weights.

Why this exists: there is no network, so no real model file.  Every parity and bench
run uses a synthetic Llama-shaped GGUF whose bytes are a pure function of
(shape, seed) -- a counter-based integer hash, no library RNG -- so the file written
in the build container, the file re-generated on the GPU box and the arrays handed
straight to the C-ABI are bit-identical.

The byte layout written here is the one the reference loader accepts
(/root/reference/read_ggml.f90:112 header, :129-158 KV pairs, :663-685 value types,
:706-718 tensor infos, :176-192 zero padding to `alignment`, :600-620 tensor reads,
:238-410 tensor names).  The reader additionally understands every GGUF scalar KV
type and ggml tensor types 0 (f32), 1 (f16) and 2 (q4_0); q4_0 is the public ggml
block format (32 weights = one f16 scale d + 16 bytes; low nibbles are elements
0..15, high nibbles elements 16..31; value = (nibble - 8) * d) -- third-party (ggml)
knowledge, not citable inside /root/reference.
"""
from __future__ import annotations

import os
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

GGUF_MAGIC = 0x46554747  # "GGUF" little endian == 1179993927 (read_ggml.f90:122)
GGML_F32, GGML_F16, GGML_Q4_0 = 0, 1, 2
GGML_Q6_K = 14
QK4_0 = 32
Q4_0_BLOCK_BYTES = 18
QK_K = 256
Q6_K_BLOCK_BYTES = 210

# GGUF metadata value types
T_U8, T_I8, T_U16, T_I16, T_U32, T_I32, T_F32, T_BOOL, T_STR, T_ARR, T_U64, T_I64, T_F64 = range(13)
_SCALAR_FMT = {T_U8: "<B", T_I8: "<b", T_U16: "<H", T_I16: "<h", T_U32: "<I", T_I32: "<i",
               T_F32: "<f", T_BOOL: "<B", T_U64: "<Q", T_I64: "<q", T_F64: "<d"}


@dataclass
class LlamaShape:
    emb_dim: int
    hidden_dim: int
    n_layers: int
    n_heads: int
    n_kv_heads: int
    vocab_size: int
    seq_len: int

    @property
    def head_size(self) -> int:
        return self.emb_dim // self.n_heads

    @property
    def kv_dim(self) -> int:
        return self.n_kv_heads * self.head_size

    def matmul_params(self) -> int:
        E, H, L, KV, V = self.emb_dim, self.hidden_dim, self.n_layers, self.kv_dim, self.vocab_size
        return L * (E * (E + 2 * KV) + E * E + 3 * E * H) + V * E


# Shapes named by BASELINE.json `configs` plus the small parity shapes.
SHAPES: Dict[str, LlamaShape] = {
    # reference compile-time parameters, /root/reference/llama2.f90:102-108
    "tinyllama": LlamaShape(2048, 5632, 22, 32, 4, 32000, 2048),
    "llama2-7b": LlamaShape(4096, 11008, 32, 32, 32, 32000, 2048),
    "llama2-70b": LlamaShape(8192, 28672, 80, 64, 8, 32000, 2048),
    # other Llama-architecture geometries (what one edits llama2.f90:102-108 to): the persistent kernel holds them when the library is
    # built with them (make TK_SHAPES=...); the multi-kernel path runs them in any build
    "mistral-7b": LlamaShape(4096, 14336, 32, 32, 8, 32000, 2048),
    "llama3-8b": LlamaShape(4096, 14336, 32, 32, 8, 128256, 2048),
    # parity shapes (oracle / reference finish in milliseconds)
    "tiny-gqa": LlamaShape(128, 256, 2, 8, 2, 300, 64),      # hs 16, kv_mul 4
    "tiny-mha": LlamaShape(128, 352, 3, 4, 4, 512, 48),      # hs 32, kv_mul 1
    "tiny-hs64": LlamaShape(256, 704, 2, 4, 2, 1000, 96),    # hs 64 like TinyLlama, kv_mul 2
    "tiny-hs128": LlamaShape(512, 1376, 2, 4, 4, 640, 40),   # hs 128 like Llama-2-7B
    "tiny-70bish": LlamaShape(1024, 3584, 3, 8, 1, 800, 64),  # E:nh:nkv = 70B ratios / 8, hs 128
    # smallest shape the persistent whole-token kernel is instantiated for (rows divide over 256 CUs)
    "tk-small": LlamaShape(256, 768, 2, 4, 2, 1024, 64),
    # the same for f16 matrices (a row must be whole 1 KB segments at 2 bytes per weight)
    "tk-small16": LlamaShape(512, 1536, 2, 8, 2, 1024, 64),
    # long-context parity shapes: the KV length crosses the timestep tile of the attention kernels several times
    # (persistent kernel and attn_kernel<64>: 256 timesteps per tile; attn_kernel<128>: 128)
    "tk-small-long": LlamaShape(256, 768, 2, 4, 2, 1024, 704),
    "tiny-hs128-long": LlamaShape(512, 1376, 2, 4, 4, 640, 320),
    # the same with hidden_dim on the batched GEMMs' 64-column step (1376 = 21.5 x 64 is not): head size 128 with one query head per
    # kv head on the passes that have no token-by-token form (llmk_batch_*)
    "tiny-hs128w": LlamaShape(512, 1408, 2, 4, 4, 640, 40),
    "tiny-hs128w-long": LlamaShape(512, 1408, 2, 4, 4, 640, 320),
    # three query heads per kv head (hs 32): the one kv_mul here that does not divide the 16 MFMA columns -- a span pass's column
    # groups hold 5 rows and one padded column (llmk_span_*)
    "tiny-kvmul3": LlamaShape(192, 512, 2, 6, 2, 400, 64),
}


# ----------------------------------------------------------------------------------------------
# deterministic values
# ----------------------------------------------------------------------------------------------
def _splitmix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _det_chunk(out: np.ndarray, base: np.uint64, s: int, e: int, lo: float, hi: float) -> None:
    idx = np.arange(s, e, dtype=np.uint64) + base
    u24 = (_splitmix64(idx) >> np.uint64(40)).astype(np.float32)  # exact: < 2**24
    u24 *= np.float32(1.0 / (1 << 24))
    u24 *= np.float32(hi - lo)
    u24 += np.float32(lo)
    out[s:e] = u24


def det_uniform(seed: int, stream: int, n: int, lo: float, hi: float, chunk: int = 1 << 22) -> np.ndarray:
    """n float32 values uniform in [lo, hi): element i = hash(seed, stream, i). Pure integer
    arithmetic up to the final affine map (three correctly-rounded f32 ops), so identical on
    every numpy build and independent of chunking/threading."""
    out = np.empty(n, dtype=np.float32)
    base = np.uint64((seed * 0x9E3779B1 + stream * 0x85EBCA77) & 0xFFFFFFFF) << np.uint64(32)
    spans = [(s, min(n, s + chunk)) for s in range(0, n, chunk)]
    if len(spans) <= 2:
        for s, e in spans:
            _det_chunk(out, base, s, e, lo, hi)
    else:  # numpy releases the GIL inside ufuncs: threads scale on the big shapes
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(32, os.cpu_count() or 1)) as ex:
            list(ex.map(lambda se: _det_chunk(out, base, se[0], se[1], lo, hi), spans))
    return out


def tensor_names(shape: LlamaShape) -> List[Tuple[str, Tuple[int, ...], str]]:
    """(name, numpy shape [out, in] or [n], kind) in file order. Names: read_ggml.f90:238-406."""
    E, H, KV, V = shape.emb_dim, shape.hidden_dim, shape.kv_dim, shape.vocab_size
    out = [("token_embd.weight", (V, E), "emb")]
    for i in range(shape.n_layers):
        p = f"blk.{i}."
        out += [
            (p + "attn_norm.weight", (E,), "norm"),
            (p + "attn_q.weight", (E, E), "mat"),
            (p + "attn_k.weight", (KV, E), "mat"),
            (p + "attn_v.weight", (KV, E), "mat"),
            (p + "attn_output.weight", (E, E), "mat"),
            (p + "ffn_norm.weight", (E,), "norm"),
            (p + "ffn_gate.weight", (H, E), "mat"),
            (p + "ffn_down.weight", (E, H), "mat"),
            (p + "ffn_up.weight", (H, E), "mat"),
        ]
    out += [("output_norm.weight", (E,), "norm"), ("output.weight", (V, E), "mat")]
    return out


def synth_tensor(shape: LlamaShape, seed: int, index: int, dims: Tuple[int, ...], kind: str) -> np.ndarray:
    """Deterministic f32 tensor. Matrices: uniform with variance 1/in_features (so activations
    stay O(1) through the stack); embeddings: uniform(-1,1); norm gains: 1 +- 0.1."""
    n = int(np.prod(dims))
    if kind == "norm":
        v = det_uniform(seed, index, n, 0.9, 1.1)
    elif kind == "emb":
        v = det_uniform(seed, index, n, -1.0, 1.0)
    else:
        a = float(np.sqrt(3.0 / dims[-1]))
        v = det_uniform(seed, index, n, -a, a)
    return v.reshape(dims)


# ----------------------------------------------------------------------------------------------
# f16 / q4_0 encodings of an f32 matrix
# ----------------------------------------------------------------------------------------------
def quantize_q4_0(w: np.ndarray) -> np.ndarray:
    """ggml q4_0 reference quantiser: per 32-block, d = max_signed/-8, q = clamp(round(x/d)+8, 0, 15).
    Returns uint8 array [..., nblocks*18]."""
    assert w.shape[-1] % QK4_0 == 0
    blocks = w.reshape(-1, QK4_0).astype(np.float32)
    idx = np.argmax(np.abs(blocks), axis=1)
    mx = blocks[np.arange(blocks.shape[0]), idx]
    d = (mx / np.float32(-8.0)).astype(np.float32)
    inv = np.where(d != 0, np.float32(1.0) / np.where(d != 0, d, 1), np.float32(0.0)).astype(np.float32)
    q = np.minimum(15, (blocks * inv[:, None] + np.float32(8.5)).astype(np.int32)).astype(np.uint8)
    out = np.empty((blocks.shape[0], Q4_0_BLOCK_BYTES), dtype=np.uint8)
    out[:, 0:2] = d.astype(np.float16).view(np.uint8).reshape(-1, 2)
    out[:, 2:] = q[:, :16] | (q[:, 16:] << 4)
    return out.reshape(*w.shape[:-1], w.shape[-1] // QK4_0 * Q4_0_BLOCK_BYTES)


def dequantize_q4_0(raw: np.ndarray, cols: int) -> np.ndarray:
    """uint8 [..., cols/32*18] -> f32 [..., cols]: (nibble - 8) * d, low nibbles = elements 0..15 of the block, high
    nibbles = elements 16..31 (ggml block_q4_0).  Large arrays are decoded in parallel slices (numpy releases the GIL)."""
    b = raw.reshape(-1, Q4_0_BLOCK_BYTES)
    nb = b.shape[0]
    out = np.empty((nb, QK4_0), np.float32)

    def part(s0, e0):
        d = b[s0:e0, 0:2].copy().view(np.float16).astype(np.float32)  # [n,1]
        qs = b[s0:e0, 2:]
        out[s0:e0, :16] = ((qs & 0x0F).astype(np.int8) - np.int8(8)).astype(np.float32) * d
        out[s0:e0, 16:] = ((qs >> 4).astype(np.int8) - np.int8(8)).astype(np.float32) * d
    chunk = 1 << 19
    if nb <= 2 * chunk:
        part(0, nb)
    else:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(32, os.cpu_count() or 1)) as ex:
            list(ex.map(lambda s0: part(s0, min(nb, s0 + chunk)), range(0, nb, chunk)))
    return out.reshape(*raw.shape[:-1], cols)


def quantize_q6_K(w: np.ndarray) -> np.ndarray:
    """A valid ggml block_q6_K encoding of w (256 weights -> ql[128] | qh[64] | int8 scales[16] | f16 d): per 16-weight
    sub-block a scale s = max|x|/31, d = max s / 127, 6-bit q = round(x / (d*sc)) + 32.  (Not ggml's search-based
    quantiser -- any encoding is a legitimate file; what the loaders must agree on is the DEcoding.)  uint8 [..., K/256*210]."""
    assert w.shape[-1] % QK_K == 0
    x = w.reshape(-1, 16, 16).astype(np.float32)                  # [block][sub-block][16]
    s = np.abs(x).max(axis=2) / np.float32(31.0)                  # [block][16]
    d = (s.max(axis=1) / np.float32(127.0)).astype(np.float16)    # [block]
    df = d.astype(np.float32)
    sc = np.where(df[:, None] > 0, np.clip(np.rint(s / np.where(df[:, None] > 0, df[:, None], 1)), 1, 127), 1).astype(np.int8)
    step = df[:, None, None] * sc[:, :, None].astype(np.float32)
    q = np.clip(np.rint(np.where(step > 0, x / np.where(step > 0, step, 1), 0)), -32, 31).astype(np.int32) + 32   # 0..63
    q = q.reshape(-1, 2, 4, 32)                                   # [block][half][quarter][l]
    ql = np.empty((q.shape[0], 2, 64), np.uint8)
    ql[:, :, 0:32] = (q[:, :, 0] & 15) | ((q[:, :, 2] & 15) << 4)
    ql[:, :, 32:64] = (q[:, :, 1] & 15) | ((q[:, :, 3] & 15) << 4)
    qh = ((q[:, :, 0] >> 4) | ((q[:, :, 1] >> 4) << 2) | ((q[:, :, 2] >> 4) << 4) | ((q[:, :, 3] >> 4) << 6)).astype(np.uint8)
    out = np.empty((q.shape[0], Q6_K_BLOCK_BYTES), np.uint8)
    out[:, 0:128] = ql.reshape(-1, 128)
    out[:, 128:192] = qh.reshape(-1, 64)
    out[:, 192:208] = sc.view(np.uint8)
    out[:, 208:210] = d.view(np.uint8).reshape(-1, 2)
    return out.reshape(*w.shape[:-1], w.shape[-1] // QK_K * Q6_K_BLOCK_BYTES)


def dequantize_q6_K(raw: np.ndarray, cols: int) -> np.ndarray:
    """ggml dequantize_row_q6_K: y = d * scale * (q - 32), evaluated left to right in f32.  uint8 [..., cols/256*210] -> f32."""
    b = raw.reshape(-1, Q6_K_BLOCK_BYTES)
    ql = b[:, 0:128].reshape(-1, 2, 64).astype(np.int32)
    qh = b[:, 128:192].reshape(-1, 2, 32).astype(np.int32)
    sc = b[:, 192:208].copy().view(np.int8).reshape(-1, 2, 8).astype(np.float32)
    d = b[:, 208:210].copy().view(np.float16).astype(np.float32).reshape(-1, 1, 1)
    q = np.empty((b.shape[0], 2, 4, 32), np.int32)
    q[:, :, 0] = (ql[:, :, 0:32] & 15) | (((qh >> 0) & 3) << 4)
    q[:, :, 1] = (ql[:, :, 32:64] & 15) | (((qh >> 2) & 3) << 4)
    q[:, :, 2] = (ql[:, :, 0:32] >> 4) | (((qh >> 4) & 3) << 4)
    q[:, :, 3] = (ql[:, :, 32:64] >> 4) | (((qh >> 6) & 3) << 4)
    q -= 32
    # sub-block scale of element (quarter g, l): scales[l // 16 + 2 g]
    idx = (np.arange(32) // 16)[None, :] + 2 * np.arange(4)[:, None]            # [4][32]
    scq = sc[:, :, idx]                                                          # [block][half][4][32]
    y = (d[..., None] * scq) * q.astype(np.float32)
    return y.reshape(*raw.shape[:-1], cols)


def scale_q4_0(raw: np.ndarray, factor: float) -> np.ndarray:
    """q4_0 rows with every block scale d multiplied by `factor` (rounded to f16 -- the result is a q4_0 tensor like any other: what
    the tests use to build models whose intermediate activations are small or large while the logits stay O(1))."""
    b = np.array(raw, dtype=np.uint8, copy=True)
    blk = b.reshape(-1, Q4_0_BLOCK_BYTES)
    d = blk[:, 0:2].copy().view(np.float16).astype(np.float32) * np.float32(factor)
    blk[:, 0:2] = d.astype(np.float16).view(np.uint8).reshape(-1, 2)
    return b


def encode(w: np.ndarray, ggml_type: int) -> np.ndarray:
    if ggml_type == GGML_F32:
        return np.ascontiguousarray(w, dtype="<f4")
    if ggml_type == GGML_F16:
        return np.ascontiguousarray(w.astype("<f2"))
    if ggml_type == GGML_Q4_0:
        return quantize_q4_0(w)
    if ggml_type == GGML_Q6_K:
        return quantize_q6_K(w)
    raise ValueError(ggml_type)


def decode(raw: np.ndarray, ggml_type: int, cols: int) -> np.ndarray:
    """Exact f32 value of stored weights (f16 -> f32 is exact; q4_0 = (nibble-8)*d in f32)."""
    if ggml_type == GGML_F32:
        return raw.astype(np.float32, copy=False)
    if ggml_type == GGML_F16:
        return raw.view("<f2").astype(np.float32) if raw.dtype != np.float16 else raw.astype(np.float32)
    if ggml_type == GGML_Q4_0:
        return dequantize_q4_0(raw, cols)
    if ggml_type == GGML_Q6_K:
        return dequantize_q6_K(raw, cols)
    raise ValueError(ggml_type)


def synth_q4_rows(seed: int, stream: int, rows: int, K: int, scale_jitter: bool = False) -> np.ndarray:
    """Synthetic q4_0 rows generated DIRECTLY in the block format (for the 7B/70B shapes, where
    materialising f32 weights first would need hundreds of GB): nibbles from the integer hash, one f16
    scale per block chosen so the dequantised weights have variance 1/K.  uint8 [rows, K/32*18].
    scale_jitter: every block gets its OWN scale, d * (0.5 .. 1.5) (sign included now and then) -- what a parity test
    needs to see a mis-indexed scale; the benchmarks keep the constant one."""
    nb = rows * (K // QK4_0)
    out = np.empty((nb, Q4_0_BLOCK_BYTES), np.uint8)
    base = np.uint64((seed * 0x9E3779B1 + stream * 0x85EBCA77) & 0xFFFFFFFF) << np.uint64(32)
    d = np.float16(np.sqrt(1.0 / K / 21.25))
    out[:, 0:2] = np.frombuffer(d.tobytes(), np.uint8)
    chunk = 1 << 20
    def fill(s0):
        e0 = min(nb, s0 + chunk)
        idx = (np.arange(s0 * 2, e0 * 2, dtype=np.uint64) + base)
        h = _splitmix64(idx)
        out[s0:e0, 2:] = h.view(np.uint8).reshape(e0 - s0, 16)
        if scale_jitter:
            u = _splitmix64(h[0::2] ^ np.uint64(0xD1B54A32D192ED03))
            f = (np.float32(0.5) + (u >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / (1 << 24))) * np.float32(d)
            f = np.where((u & np.uint64(7)) == 0, -f, f)                   # one block in eight carries a negative scale
            out[s0:e0, 0:2] = f.astype(np.float16).view(np.uint8).reshape(-1, 2)
    spans = list(range(0, nb, chunk))
    if len(spans) <= 2:
        for s0 in spans:
            fill(s0)
    else:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(32, os.cpu_count() or 1)) as ex:
            list(ex.map(fill, spans))
    return out.reshape(rows, K // QK4_0 * Q4_0_BLOCK_BYTES)


# ----------------------------------------------------------------------------------------------
# fused in-memory layout == weight_module.f90:13-26 (Fortran (in,rows,L) == C [L][rows][in])
# ----------------------------------------------------------------------------------------------
@dataclass
class FusedWeights:
    shape: LlamaShape
    ggml_type: int
    token_embedding_table: np.ndarray = None  # [V][E] f32 (always f32: it is gathered, not streamed)
    rms_att_weight: np.ndarray = None         # [L][E] f32
    rms_ffn_weight: np.ndarray = None         # [L][E] f32
    rms_final_weight: np.ndarray = None       # [E]   f32
    wqkv: np.ndarray = None                   # [L][E+2KV][E*]   (* = encoded row bytes for f16/q4_0)
    wo: np.ndarray = None                     # [L][E][E*]
    w13: np.ndarray = None                    # [L][2H][E*]  rows 0..H-1 gate, H.. up (read_ggml.f90:347,376)
    w2: np.ndarray = None                     # [L][E][H*]
    wcls: np.ndarray = None                   # [V][E*]
    wcls_type: int = None                     # the classifier's own ggml type when it differs: 14 = raw q6_K super-blocks, 0 = dequantised

    @property
    def cls_type(self) -> int:
        return self.ggml_type if self.wcls_type is None else self.wcls_type

    def as_f32(self) -> "FusedWeights":
        """Same weights with every matrix decoded to f32 (what an f32 reference run consumes)."""
        s, t = self.shape, self.ggml_type
        return FusedWeights(s, GGML_F32, self.token_embedding_table, self.rms_att_weight, self.rms_ffn_weight,
                            self.rms_final_weight, decode(self.wqkv, t, s.emb_dim), decode(self.wo, t, s.emb_dim),
                            decode(self.w13, t, s.emb_dim), decode(self.w2, t, s.hidden_dim),
                            decode(self.wcls, self.cls_type, s.emb_dim))


def with_q6k_classifier(fw: FusedWeights) -> FusedWeights:
    """The same weights with the classifier as RAW q6_K super-blocks (quantised from its decoded values): what `llama-quantize
    ... Q4_0` leaves in a stock file's output.weight, and what load_fused() returns for such a file."""
    import dataclasses
    E = fw.shape.emb_dim
    assert E % QK_K == 0
    raw = quantize_q6_K(decode(fw.wcls, fw.cls_type, E)).reshape(fw.shape.vocab_size, -1)
    return dataclasses.replace(fw, wcls=np.ascontiguousarray(raw), wcls_type=GGML_Q6_K)


def synth_fused_q4_direct(shape: LlamaShape, seed: int, scale_jitter: bool = True) -> FusedWeights:
    """q4_0 FusedWeights with every matrix generated directly in block format (synth_q4_rows): seconds where
    synth_fused + quantisation takes minutes at 70B geometry.  Embedding and norm gains as in synth_fused."""
    E, H, L, KV, V = shape.emb_dim, shape.hidden_dim, shape.n_layers, shape.kv_dim, shape.vocab_size
    fw = FusedWeights(shape, GGML_Q4_0)
    idx = {n: i for i, (n, _, _) in enumerate(tensor_names(shape))}
    q4 = lambda name, rows, K: synth_q4_rows(seed, idx[name], rows, K, scale_jitter)
    fw.token_embedding_table = synth_tensor(shape, seed, idx["token_embd.weight"], (V, E), "emb")
    fw.rms_final_weight = synth_tensor(shape, seed, idx["output_norm.weight"], (E,), "norm")
    fw.wcls = q4("output.weight", V, E)
    fw.rms_att_weight = np.stack([synth_tensor(shape, seed, idx[f"blk.{l}.attn_norm.weight"], (E,), "norm") for l in range(L)])
    fw.rms_ffn_weight = np.stack([synth_tensor(shape, seed, idx[f"blk.{l}.ffn_norm.weight"], (E,), "norm") for l in range(L)])
    fw.wqkv = np.stack([np.concatenate([q4(f"blk.{l}.attn_q.weight", E, E), q4(f"blk.{l}.attn_k.weight", KV, E),
                                        q4(f"blk.{l}.attn_v.weight", KV, E)]) for l in range(L)])
    fw.wo = np.stack([q4(f"blk.{l}.attn_output.weight", E, E) for l in range(L)])
    fw.w13 = np.stack([np.concatenate([q4(f"blk.{l}.ffn_gate.weight", H, E), q4(f"blk.{l}.ffn_up.weight", H, E)]) for l in range(L)])
    fw.w2 = np.stack([q4(f"blk.{l}.ffn_down.weight", E, H) for l in range(L)])
    return fw


def synth_fused(shape: LlamaShape, seed: int, ggml_type: int = GGML_F32) -> FusedWeights:
    """Build the fused arrays directly (no file). Tensor values are identical to write_synth_gguf's."""
    E, H, L, KV, V = shape.emb_dim, shape.hidden_dim, shape.n_layers, shape.kv_dim, shape.vocab_size
    fw = FusedWeights(shape, ggml_type)
    enc_cols = lambda k: encode(np.zeros((1, k), np.float32), ggml_type).shape[-1]
    dt = {GGML_F32: np.float32, GGML_F16: np.float16, GGML_Q4_0: np.uint8}[ggml_type]
    fw.rms_att_weight = np.empty((L, E), np.float32)
    fw.rms_ffn_weight = np.empty((L, E), np.float32)
    fw.wqkv = np.empty((L, E + 2 * KV, enc_cols(E)), dt)
    fw.wo = np.empty((L, E, enc_cols(E)), dt)
    fw.w13 = np.empty((L, 2 * H, enc_cols(E)), dt)
    fw.w2 = np.empty((L, E, enc_cols(H)), dt)
    for index, (name, dims, kind) in enumerate(tensor_names(shape)):
        t = synth_tensor(shape, seed, index, dims, kind)
        if name == "token_embd.weight":
            fw.token_embedding_table = t
        elif name == "output_norm.weight":
            fw.rms_final_weight = t
        elif name == "output.weight":
            fw.wcls = encode(t, ggml_type)
        else:
            _, li, rest = name.split(".", 2)
            li = int(li)
            if rest == "attn_norm.weight":
                fw.rms_att_weight[li] = t
            elif rest == "ffn_norm.weight":
                fw.rms_ffn_weight[li] = t
            elif rest == "attn_q.weight":
                fw.wqkv[li, 0:E] = encode(t, ggml_type)
            elif rest == "attn_k.weight":
                fw.wqkv[li, E:E + KV] = encode(t, ggml_type)
            elif rest == "attn_v.weight":
                fw.wqkv[li, E + KV:E + 2 * KV] = encode(t, ggml_type)
            elif rest == "attn_output.weight":
                fw.wo[li] = encode(t, ggml_type)
            elif rest == "ffn_gate.weight":
                fw.w13[li, 0:H] = encode(t, ggml_type)
            elif rest == "ffn_up.weight":
                fw.w13[li, H:2 * H] = encode(t, ggml_type)
            elif rest == "ffn_down.weight":
                fw.w2[li] = encode(t, ggml_type)
    return fw


# ----------------------------------------------------------------------------------------------
# writer
# ----------------------------------------------------------------------------------------------
def _w_str(f, s: bytes):
    f.write(struct.pack("<Q", len(s)))
    f.write(s)


def vocab_strings(V: int) -> List[bytes]:
    """Unique printable token strings so greedy ids can be parsed back from CLI output.
    ids 0..2 mimic <unk>/<s>/</s>; single printable ASCII characters get their own tokens so
    bpe_encode's per-character lookup (llama2.f90:666-668) finds prompt characters."""
    out = []
    for i in range(V):
        if i == 0:
            out.append(b"<unk>")
        elif i == 1:
            out.append(b"<s>")
        elif i == 2:
            out.append(b"</s>")
        elif 3 <= i < 3 + 95 and V >= 200:
            out.append(bytes([32 + i - 3]))
        else:
            out.append(b"<%05d>" % i)
    return out


# A vocabulary with real merges (round-4 verdict: `bpe_encode`'s greedy best-score loop, llama2.f90:658-724, was never run on a
# vocabulary where a merge exists).  The single characters stay where vocab_strings puts them; these strings replace the
# placeholder tokens from id 100 on.  What each group pins:
#   * plain merges at several levels ("t"+"h" -> "th", "th"+"e" -> "the", " "+"the" -> " the"): the best score ANYWHERE in the
#     text wins, not the leftmost pair;
#   * "in" / "ng" carry EQUAL scores and "ing" does not exist: "ing" must end as ["in", "g"] (strict `>` keeps the FIRST pair,
#     llama2.f90:694); "an" / "nd" are equal too but "and" exists through "an"+"d" only;
#   * "er" is in the vocabulary TWICE with different scores: the linear scan of `lookup` (llama2.f90:643-655) returns the
#     first index, so the first entry's score decides ("er" outranks "he" only with the SECOND entry's score).
MERGE_TOKENS = [
    (b"th", -1.0), (b"he", -2.0), (b"the", -1.5), (b" the", -0.5), (b"in", -3.0), (b"ng", -3.0), (b"an", -4.0), (b"nd", -4.0),
    (b"and", -3.5), (b"er", -6.0), (b"er", -0.25), (b"ot", -5.0), (b"oth", -4.5), (b"other", -0.75), (b" a", -7.0), (b"sa", -8.0),
    (b"nn", -9.0), (b"hi", -2.5), (b"thi", -9.5), (b" t", -10.0),
]
MERGE_FIRST = 100


def merge_vocab(V: int):
    """(tokens, scores) = vocab_strings with MERGE_TOKENS from id MERGE_FIRST on; every other score stays -id."""
    assert V >= MERGE_FIRST + len(MERGE_TOKENS) and V >= 200
    vocab = vocab_strings(V)
    scores = -np.arange(V, dtype="<f4")
    for k, (t, sc) in enumerate(MERGE_TOKENS):
        vocab[MERGE_FIRST + k] = t
        scores[MERGE_FIRST + k] = sc
    return vocab, scores


def _tensor_source(fw: "FusedWeights", name: str) -> np.ndarray:
    """Encoded bytes of one GGUF tensor, sliced out of the fused arrays (inverse of load_fused)."""
    s = fw.shape
    E, H, KV = s.emb_dim, s.hidden_dim, s.kv_dim
    if name == "token_embd.weight":
        return fw.token_embedding_table
    if name == "output_norm.weight":
        return fw.rms_final_weight
    if name == "output.weight":
        return fw.wcls
    _, li, rest = name.split(".", 2)
    li = int(li)
    return {
        "attn_norm.weight": lambda: fw.rms_att_weight[li], "ffn_norm.weight": lambda: fw.rms_ffn_weight[li],
        "attn_q.weight": lambda: fw.wqkv[li, 0:E], "attn_k.weight": lambda: fw.wqkv[li, E:E + KV],
        "attn_v.weight": lambda: fw.wqkv[li, E + KV:E + 2 * KV], "attn_output.weight": lambda: fw.wo[li],
        "ffn_gate.weight": lambda: fw.w13[li, 0:H], "ffn_up.weight": lambda: fw.w13[li, H:2 * H],
        "ffn_down.weight": lambda: fw.w2[li],
    }[rest]()


def write_gguf(path: str, fw: "FusedWeights", alignment: int = 32, version: int = 3, rms_eps: float = 1e-5,
               rope_freq_base: float = None, output_q6k: bool = False, vocab: List[bytes] = None, scores=None) -> None:
    """Write fused weights as a Llama GGUF. With f32 matrices the reference loader reads it as is.
    output_q6k: store output.weight as q6_K (what stock llama.cpp q4_0 files do), quantised from the decoded wcls."""
    shape, ggml_type = fw.shape, fw.ggml_type
    out_raw = quantize_q6_K(decode(fw.wcls, fw.cls_type, shape.emb_dim)) if output_q6k else None
    names = tensor_names(shape)
    vocab = vocab_strings(shape.vocab_size) if vocab is None else vocab
    scores = -np.arange(len(vocab), dtype="<f4") if scores is None else np.asarray(scores, "<f4")
    kvs = [
        ("general.architecture", T_STR, b"llama"),
        ("general.name", T_STR, b"synthetic"),
        ("llama.context_length", T_U32, shape.seq_len),
        ("llama.embedding_length", T_U32, shape.emb_dim),
        ("llama.block_count", T_U32, shape.n_layers),
        ("llama.feed_forward_length", T_U32, shape.hidden_dim),
        ("llama.attention.head_count", T_U32, shape.n_heads),
        ("llama.attention.head_count_kv", T_U32, shape.n_kv_heads),
        ("llama.attention.layer_norm_rms_epsilon", T_F32, rms_eps),
        ("general.alignment", T_U32, alignment),
        ("tokenizer.ggml.model", T_STR, b"llama"),
    ]
    if rope_freq_base is not None:
        kvs.append(("llama.rope.freq_base", T_F32, rope_freq_base))
    src = lambda name: out_raw if (output_q6k and name == "output.weight") else _tensor_source(fw, name)
    cls_tt = GGML_Q6_K if output_q6k else fw.cls_type
    _write_gguf_file(path, shape, ggml_type, cls_tt, kvs, vocab, scores, names, src, lambda name: src(name).nbytes, alignment, version)


def _write_gguf_file(path, shape, ggml_type, cls_tt, kvs, vocab, scores, names, src, nbytes_of, alignment, version):
    """header + KV pairs + tensor directory + data; `src(name)` is called ONCE per tensor, when its bytes are written"""
    with open(path, "wb") as f:
        f.write(struct.pack("<IIqq", GGUF_MAGIC, version, len(names), len(kvs) + 2))
        for k, t, v in kvs:
            _w_str(f, k.encode())
            f.write(struct.pack("<I", t))
            if t == T_STR:
                _w_str(f, v)
            else:
                f.write(struct.pack(_SCALAR_FMT[t], v))
        _w_str(f, b"tokenizer.ggml.tokens")
        f.write(struct.pack("<IIQ", T_ARR, T_STR, len(vocab)))
        for s in vocab:
            _w_str(f, s)
        _w_str(f, b"tokenizer.ggml.scores")
        f.write(struct.pack("<IIQ", T_ARR, T_F32, len(vocab)))
        f.write(scores.tobytes())
        offset = 0
        infos = []
        for name, dims, kind in names:
            tt = ggml_type if kind == "mat" else GGML_F32
            if name == "output.weight":
                tt = cls_tt
            nbytes = nbytes_of(name)
            infos.append((tt, offset, nbytes))
            _w_str(f, name.encode())
            f.write(struct.pack("<I", len(dims)))
            for d in reversed(dims):  # GGUF ne[0] = innermost = in_features
                f.write(struct.pack("<Q", d))
            f.write(struct.pack("<IQ", tt, offset))
            offset += (nbytes + alignment - 1) // alignment * alignment
        f.write(b"\0" * ((-f.tell()) % alignment))
        data_start = f.tell()
        for (name, dims, kind), (tt, off, nbytes) in zip(names, infos):
            assert f.tell() == data_start + off
            a = np.ascontiguousarray(src(name))
            assert a.nbytes == nbytes, name
            f.write(a.data)
            f.write(b"\0" * ((-nbytes) % alignment))


def write_synth_q4_gguf_streamed(path: str, shape: LlamaShape, seed: int, alignment: int = 32, scale_jitter: bool = False) -> int:
    """A q4_0 GGUF of ANY size written tensor by tensor (synth_q4_rows: blocks generated directly, the values bench.py's
    build_streamed uploads): the 38.7 GB Llama-2-70B file never exists in memory.  Returns the file size."""
    names = tensor_names(shape)
    idx = {n: i for i, (n, _, _) in enumerate(names)}
    dims_of = {n: d for n, d, _ in names}
    kind_of = {n: k for n, _, k in names}

    def nbytes_of(name):
        d = dims_of[name]
        return int(np.prod(d)) * 4 if kind_of[name] != "mat" else int(np.prod(d[:-1])) * (d[-1] // QK4_0) * Q4_0_BLOCK_BYTES

    def src(name):
        d = dims_of[name]
        if kind_of[name] != "mat":
            return synth_tensor(shape, seed, idx[name], d, kind_of[name])
        return synth_q4_rows(seed, idx[name], int(np.prod(d[:-1])), d[-1], scale_jitter)
    vocab = vocab_strings(shape.vocab_size)
    scores = -np.arange(len(vocab), dtype="<f4")
    kvs = [("general.architecture", T_STR, b"llama"), ("general.name", T_STR, b"synthetic"),
           ("llama.context_length", T_U32, shape.seq_len), ("llama.embedding_length", T_U32, shape.emb_dim),
           ("llama.block_count", T_U32, shape.n_layers), ("llama.feed_forward_length", T_U32, shape.hidden_dim),
           ("llama.attention.head_count", T_U32, shape.n_heads), ("llama.attention.head_count_kv", T_U32, shape.n_kv_heads),
           ("llama.attention.layer_norm_rms_epsilon", T_F32, 1e-5), ("general.alignment", T_U32, alignment),
           ("tokenizer.ggml.model", T_STR, b"llama")]
    _write_gguf_file(path, shape, GGML_Q4_0, GGML_Q4_0, kvs, vocab, scores, names, src, nbytes_of, alignment, 3)
    return os.path.getsize(path)


def write_synth_q4_decoded_f32_gguf(path: str, shape: LlamaShape, seed: int, alignment: int = 32, scale_jitter: bool = True) -> int:
    """The weights of synth_fused_q4_direct / write_synth_q4_gguf_streamed DECODED to f32 -- (nibble - 8) * d, exact -- as an
    f32 GGUF the unmodified reference loader reads (read_ggml.f90 accepts type 0 only): the file a full-depth
    Llama-2-7B golden is generated from (27 GB, written tensor by tensor).  Returns the file size."""
    names = tensor_names(shape)
    idx = {n: i for i, (n, _, _) in enumerate(names)}
    dims_of = {n: d for n, d, _ in names}
    kind_of = {n: k for n, _, k in names}

    def src(name):
        d = dims_of[name]
        if kind_of[name] != "mat":
            return synth_tensor(shape, seed, idx[name], d, kind_of[name])
        return dequantize_q4_0(synth_q4_rows(seed, idx[name], int(np.prod(d[:-1])), d[-1], scale_jitter), d[-1])
    vocab = vocab_strings(shape.vocab_size)
    scores = -np.arange(len(vocab), dtype="<f4")
    kvs = [("general.architecture", T_STR, b"llama"), ("general.name", T_STR, b"synthetic"),
           ("llama.context_length", T_U32, shape.seq_len), ("llama.embedding_length", T_U32, shape.emb_dim),
           ("llama.block_count", T_U32, shape.n_layers), ("llama.feed_forward_length", T_U32, shape.hidden_dim),
           ("llama.attention.head_count", T_U32, shape.n_heads), ("llama.attention.head_count_kv", T_U32, shape.n_kv_heads),
           ("llama.attention.layer_norm_rms_epsilon", T_F32, 1e-5), ("general.alignment", T_U32, alignment),
           ("tokenizer.ggml.model", T_STR, b"llama")]
    _write_gguf_file(path, shape, GGML_F32, GGML_F32, kvs, vocab, scores, names, src, lambda name: int(np.prod(dims_of[name])) * 4,
                     alignment, 3)
    return os.path.getsize(path)


def write_ak(path: str, fw: "FusedWeights") -> None:
    """llama2.c-style flat checkpoint ("ak" format) in the order the reference's `--ak` reader
    consumes it (/root/reference/llama2.f90:160-292): 7 int32 header, token_embedding_table,
    rms_att_weight, wq, wk, wv (layer-major each), wo, rms_ffn_weight, w1, w2, w3, rms_final_weight,
    wcls.  f32 only."""
    assert fw.ggml_type == GGML_F32
    s = fw.shape
    E, H, KV = s.emb_dim, s.hidden_dim, s.kv_dim
    with open(path, "wb") as f:
        f.write(struct.pack("<7i", s.emb_dim, s.hidden_dim, s.n_layers, s.n_heads, s.n_kv_heads, s.vocab_size, s.seq_len))
        for a in (fw.token_embedding_table, fw.rms_att_weight, fw.wqkv[:, 0:E], fw.wqkv[:, E:E + KV],
                  fw.wqkv[:, E + KV:E + 2 * KV], fw.wo, fw.rms_ffn_weight, fw.w13[:, 0:H], fw.w2, fw.w13[:, H:2 * H],
                  fw.rms_final_weight, fw.wcls):
            f.write(np.ascontiguousarray(a, dtype="<f4").tobytes())


def write_tokenizer_bin(path: str, vocab: List[bytes], scores=None) -> None:
    """llama2.c tokenizer.bin as the reference reads it (llama2.f90:321-356): int32 max_len, then per
    token f32 score, int32 length, bytes."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", max(len(t) for t in vocab)))
        for i, t in enumerate(vocab):
            f.write(struct.pack("<fi", float(-i if scores is None else scores[i]), len(t)))
            f.write(t)


def write_synth_gguf(path: str, shape: LlamaShape, seed: int, ggml_type: int = GGML_F32,
                     alignment: int = 32, version: int = 3, vocab: List[bytes] = None, scores=None) -> None:
    """Synthetic Llama GGUF: tensor bytes are a pure function of (shape, seed, type)."""
    write_gguf(path, synth_fused(shape, seed, ggml_type), alignment, version, vocab=vocab, scores=scores)


# ----------------------------------------------------------------------------------------------
# reader (python mirror of the host loader; used by tests to cross-check the Fortran loader)
# ----------------------------------------------------------------------------------------------
@dataclass
class GGUFFile:
    version: int
    kv: Dict[str, object]
    tensors: Dict[str, Tuple[Tuple[int, ...], int, int]]  # name -> (dims innermost-first, type, offset)
    data_start: int
    path: str = ""
    alignment: int = 32

    def shape(self) -> LlamaShape:
        k = self.kv
        return LlamaShape(k["llama.embedding_length"], k["llama.feed_forward_length"], k["llama.block_count"],
                          k["llama.attention.head_count"], k.get("llama.attention.head_count_kv",
                                                                 k["llama.attention.head_count"]),
                          len(k["tokenizer.ggml.tokens"]), k["llama.context_length"])

    def read_tensor(self, name: str) -> Tuple[np.ndarray, int]:
        dims, tt, off = self.tensors[name]
        cols = dims[0]
        rows = int(np.prod(dims[1:])) if len(dims) > 1 else 1
        row_bytes = {GGML_F32: 4 * cols, GGML_F16: 2 * cols, GGML_Q4_0: cols // 32 * 18, GGML_Q6_K: cols // 256 * 210}[tt]
        with open(self.path, "rb") as f:
            f.seek(self.data_start + off)
            raw = np.frombuffer(f.read(rows * row_bytes), dtype=np.uint8)
        dt = {GGML_F32: "<f4", GGML_F16: "<f2", GGML_Q4_0: np.uint8, GGML_Q6_K: np.uint8}[tt]
        arr = raw.view(dt)
        return (arr.reshape(rows, -1) if len(dims) > 1 else arr), tt


def _r(f, fmt):
    sz = struct.calcsize(fmt)
    return struct.unpack(fmt, f.read(sz))


def _r_str(f) -> bytes:
    (n,) = _r(f, "<Q")
    return f.read(n)


def _r_val(f, t):
    if t == T_STR:
        return _r_str(f)
    if t == T_ARR:
        et, n = _r(f, "<IQ")
        if et in _SCALAR_FMT:
            dt = np.dtype(_SCALAR_FMT[et])
            return np.frombuffer(f.read(dt.itemsize * n), dtype=dt)
        return [_r_val(f, et) for _ in range(n)]
    return _r(f, _SCALAR_FMT[t])[0]


def read_gguf(path: str) -> GGUFFile:
    with open(path, "rb") as f:
        magic, version, n_tensors, n_kv = _r(f, "<IIqq")
        if magic != GGUF_MAGIC:
            raise ValueError("Magic numbers do not match")
        kv = {}
        for _ in range(n_kv):
            key = _r_str(f).decode()
            (t,) = _r(f, "<I")
            kv[key] = _r_val(f, t)
        tensors = {}
        for _ in range(n_tensors):
            name = _r_str(f).decode()
            (nd,) = _r(f, "<I")
            dims = tuple(_r(f, "<Q")[0] for _ in range(nd))
            tt, off = _r(f, "<IQ")
            tensors[name] = (dims, tt, off)
        alignment = int(kv.get("general.alignment", 32))
        data_start = (f.tell() + alignment - 1) // alignment * alignment
    return GGUFFile(version, kv, tensors, data_start, path, alignment)


def load_fused(path: str, dequant_cls: bool = False) -> FusedWeights:
    """Read a Llama GGUF into the fused weight_module layout (python mirror of load_ggml).  A q6_K output.weight beside f16 / q4_0
    matrices stays RAW (wcls_type 14: the device dots the super-blocks, csrc/q6k.h) unless dequant_cls -- the round-2 behaviour
    and what the Fortran loader does under LLM_DEQUANT_CLS=1: any foreign classifier type is handed over as f32."""
    g = read_gguf(path)
    s = g.shape()
    E, H, L, KV = s.emb_dim, s.hidden_dim, s.n_layers, s.kv_dim
    _, mt = g.read_tensor("blk.0.attn_q.weight")
    fw = FusedWeights(s, mt)
    emb, et = g.read_tensor("token_embd.weight")
    fw.token_embedding_table = decode(emb, et, E)
    fw.rms_final_weight = g.read_tensor("output_norm.weight")[0].astype(np.float32)
    fw.wcls, ct = g.read_tensor("output.weight")
    if ct != mt:   # mixed file (a stock q4_0 file's q6_K output.weight)
        if ct == GGML_Q6_K and mt != GGML_F32 and E % QK_K == 0 and not dequant_cls:
            fw.wcls = np.ascontiguousarray(fw.wcls).reshape(s.vocab_size, -1)
            fw.wcls_type = GGML_Q6_K
        else:
            fw.wcls = decode(fw.wcls, ct, E)
            fw.wcls_type = GGML_F32
    cat = lambda parts: np.ascontiguousarray(np.concatenate(parts, axis=0))
    fw.rms_att_weight = np.stack([g.read_tensor(f"blk.{i}.attn_norm.weight")[0] for i in range(L)]).astype(np.float32)
    fw.rms_ffn_weight = np.stack([g.read_tensor(f"blk.{i}.ffn_norm.weight")[0] for i in range(L)]).astype(np.float32)
    fw.wqkv = np.stack([cat([g.read_tensor(f"blk.{i}.attn_{n}.weight")[0] for n in "qkv"]) for i in range(L)])
    fw.wo = np.stack([g.read_tensor(f"blk.{i}.attn_output.weight")[0] for i in range(L)])
    fw.w13 = np.stack([cat([g.read_tensor(f"blk.{i}.ffn_{n}.weight")[0] for n in ("gate", "up")]) for i in range(L)])
    fw.w2 = np.stack([g.read_tensor(f"blk.{i}.ffn_down.weight")[0] for i in range(L)])
    return fw


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser(description="write a synthetic Llama GGUF")
    ap.add_argument("out")
    ap.add_argument("--shape", default="tiny-gqa", choices=sorted(SHAPES))
    ap.add_argument("--seed", type=int, default=20260928)
    ap.add_argument("--type", default="f32", choices=["f32", "f16", "q4_0"])
    a = ap.parse_args()
    write_synth_gguf(a.out, SHAPES[a.shape], a.seed, {"f32": 0, "f16": 1, "q4_0": 2}[a.type])
    print("wrote", a.out)
