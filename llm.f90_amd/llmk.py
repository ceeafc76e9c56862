"""ctypes binding of the llmk C-ABI (include/llmk.h) -- the same symbols the Fortran host binds
with ISO_C_BINDING (host/llmk_binding.f90).  Used by tests/ and bench.py.

There is no fallback: if libllmk.so is missing or no HIP device is usable this raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# LLMK_LIB selects another build of the same ABI (csrc/libllmk_debug.so: the persistent kernel's timing aids)
LIB_PATH = os.environ.get("LLMK_LIB") or os.path.join(_HERE, "csrc", "libllmk.so")

TENSOR_IDS = {
    "token_embedding_table": 0, "rms_att_weight": 1, "rms_ffn_weight": 2, "wqkv": 3, "wo": 4, "w13": 5, "w2": 6,
    "rms_final_weight": 7, "wcls": 8,
}
FLAG_NO_GRAPH, FLAG_TIMINGS, FLAG_MULTI_KERNEL = 1, 2, 4
# every symbol include/llmk.h declares
SYMBOLS = ["llmk_create", "llmk_create_tp", "llmk_tp_unique_id", "llmk_tp_init_comm", "llmk_tp_p2p_handle", "llmk_tp_p2p_connect",
           "llmk_tp_p2p_connect_local", "llmk_tp_p2p_selftest", "llmk_tp_p2p_stress", "llmk_tp_p2p_disable", "llmk_tp_begin", "llmk_tp_segment",
           "llmk_tp_read_partial", "llmk_tp_write_partial", "llmk_tp_read_logits", "llmk_upload", "llmk_upload_rows",
           "llmk_set_rope_freqs", "llmk_set_tensor_type", "llmk_set_rms_eps", "llmk_forward", "llmk_forward_ahead_stats", "llmk_prefill", "llmk_forward_greedy", "llmk_decode_greedy",
           "llmk_forward_sample", "llmk_decode_sample", "llmk_forward_sample_ex", "llmk_decode_sample_ex", "llmk_sample_logits", "llmk_set_history", "llmk_get_history",
           "llmk_forward_sample_pen", "llmk_decode_sample_pen", "llmk_sample_logits_pen", "llmk_forward_sample_lp", "llmk_decode_sample_lp",
           "llmk_logprob_logits", "llmk_score", "llmk_batch_create", "llmk_batch_destroy", "llmk_batch_fork", "llmk_batch_forward",
           "llmk_batch_decode", "llmk_batch_time", "llmk_rows_set_history", "llmk_rows_get_history", "llmk_rows_decode",
           "llmk_rows_sample_logits", "llmk_prefix_set", "llmk_prefix_attach", "llmk_prefix_len",
           "llmk_cache_create", "llmk_cache_type", "llmk_cache_bytes", "llmk_cache_peek", "llmk_span_forward", "llmk_span_time", "llmk_reset", "llmk_timings",
           "llmk_time_kernel", "llmk_cls_form", "llmk_peek", "llmk_tensor_checksum", "llmk_path", "llmk_tk_shapes", "llmk_tp_ranks_seen", "llmk_destroy", "llmk_strerror", "llmk_version"]
PATH_NAMES = {0: "multi-kernel (5 launches per layer)", 1: "persistent whole-token kernel",
              2: "tensor-parallel rank: 6 launches per layer + one-shot peer-memory exchanges",
              3: "tensor-parallel rank: eager launches + RCCL collectives", 4: "tensor-parallel rank, collectives not connected"}


TOKEN_FN = C.CFUNCTYPE(None, C.c_int, C.c_int, C.c_void_p)
SPAN_LAST = 1          # LLMK_SPAN_LAST
SPAN_CHUNK = 128       # rows of one pass (LLMK_MAX_BATCH): Batch.ingest's chunk


class Span(C.Structure):
    """llmk_span: positions pos0 .. pos0+len-1 (1-based) of `slot`"""
    _fields_ = [("slot", C.c_int32), ("pos0", C.c_int32), ("len", C.c_int32)]


class LlmkError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"llmk error {code}: {msg}")
        self.code = code


class Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("emb_dim", "hidden_dim", "n_layers", "n_heads", "n_kv_heads", "vocab_size",
                                         "seq_len", "weight_type", "device", "flags")]


class Sampler(C.Structure):
    """llmk_sampler: temperature T > 0; top_k = 0, top_p = 1, min_p = 0 are "off" (include/llmk.h)"""
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("min_p", C.c_float), ("seed", C.c_uint64)]


def sampler(temperature: float, seed: int, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0) -> Sampler:
    return Sampler(temperature, top_k, top_p, min_p, seed & 0xFFFFFFFFFFFFFFFF)


MAX_LOGIT_BIAS = 256
MAX_BATCH = 128
KV_TYPES = {"f32": 0, "f16": 1}             # a batch's K/V cache types (llmk_cache_create): LLMK_TYPE_F32 / LLMK_TYPE_F16
KV_CACHE_TYPES = {**KV_TYPES, "q8_0": 8}    # ... and all of them: LLMK_TYPE_Q8_0 (blocks of 32 int8 quants and an f16 scale) joins
CLS_NONE, CLS_GEMM, CLS_ROWS = 0, 1, 2      # llmk_cls_form: LLMK_CLS_*


class LogitBias(C.Structure):
    """llmk_logit_bias: a 1-based token id and what is added to its logit (-inf bans the token)"""
    _fields_ = [("token", C.c_int32), ("bias", C.c_float)]


class Penalties(C.Structure):
    """llmk_penalties: last_n = 0, repeat = 1, frequency = 0, presence = 0, no bias are "off" (include/llmk.h)"""
    _fields_ = [("last_n", C.c_int32), ("repeat", C.c_float), ("frequency", C.c_float), ("presence", C.c_float),
                ("bias", C.POINTER(LogitBias)), ("n_bias", C.c_int32)]


def penalties(last_n: int = 0, repeat: float = 1.0, frequency: float = 0.0, presence: float = 0.0, bias=()) -> Penalties:
    """bias: [(1-based token, bias)] or {token: bias}.  The entries live in an array the returned struct keeps alive."""
    items = list(bias.items()) if isinstance(bias, dict) else list(bias)
    arr = (LogitBias * max(1, len(items)))(*[LogitBias(int(t), float(b)) for t, b in items])
    pn = Penalties(last_n, repeat, frequency, presence, C.cast(arr, C.POINTER(LogitBias)), len(items))
    pn._entries = arr
    return pn


MAX_TOP_LOGPROBS = 20


class Logprobs(C.Structure):
    """llmk_logprobs: top_n alternatives per position and where the records go (include/llmk.h)"""
    _fields_ = [("top_n", C.c_int32), ("token_logprob", C.POINTER(C.c_float)), ("top_tokens", C.POINTER(C.c_int32)),
                ("top_logprobs", C.POINTER(C.c_float))]


def logprobs(n: int, top_n: int, want_token: bool = True) -> Logprobs:
    """A request for n positions; the arrays (token_logprob [n], top_tokens and top_logprobs [n][top_n]) live in the returned struct."""
    lp = Logprobs(top_n, None, None, None)
    lp.token = np.zeros(n, np.float32) if want_token else None
    lp.tokens = np.zeros((n, max(top_n, 0)), np.int32)
    lp.values = np.zeros((n, max(top_n, 0)), np.float32)
    if want_token:
        lp.token_logprob = lp.token.ctypes.data_as(C.POINTER(C.c_float))
    if top_n > 0:
        lp.top_tokens = lp.tokens.ctypes.data_as(C.POINTER(C.c_int32))
        lp.top_logprobs = lp.values.ctypes.data_as(C.POINTER(C.c_float))
    return lp


def _request(temperature, seed, top_k, top_p, min_p, *pen):
    """a sampling wrapper's keyword arguments as what the C entry points take: (byref(Sampler), byref(Penalties))"""
    return C.byref(sampler(temperature, seed, top_k, top_p, min_p)), C.byref(penalties(*pen))


def build_lib(force: bool = False) -> str:
    """hipcc --offload-arch=gfx950 -> csrc/libllmk.so (cross-compiles without a GPU)."""
    subprocess.run(["make", "-s", "-C", _HERE, "lib"] + (["-B"] if force else []), check=True)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} not built (run `make -C llm.f90_amd lib`); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        vp, ci, cf = C.c_void_p, C.c_int, C.POINTER(C.c_float)
        L.llmk_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
        L.llmk_create_tp.argtypes = [C.POINTER(Config), ci, ci, C.POINTER(vp)]
        L.llmk_tp_unique_id.argtypes = [C.c_char_p]
        L.llmk_tp_init_comm.argtypes = [vp, C.c_char_p]
        L.llmk_tp_p2p_handle.argtypes = [vp, C.c_char_p]
        L.llmk_tp_p2p_connect.argtypes = [vp, C.c_char_p]
        L.llmk_tp_p2p_connect_local.argtypes = [vp, C.POINTER(vp)]
        L.llmk_tp_p2p_selftest.argtypes = [vp, ci]
        L.llmk_tp_p2p_stress.argtypes = [vp, ci, C.c_uint]
        L.llmk_tp_p2p_disable.argtypes = [vp]
        L.llmk_tensor_checksum.argtypes = [vp, ci, C.POINTER(C.c_ulonglong)]
        L.llmk_tp_begin.argtypes = [vp, ci, ci]
        L.llmk_tp_segment.argtypes = [vp, ci, ci]
        L.llmk_tp_read_partial.argtypes = [vp, cf]
        L.llmk_tp_write_partial.argtypes = [vp, cf]
        L.llmk_tp_read_logits.argtypes = [vp, cf]
        L.llmk_upload.argtypes = [vp, ci, vp, C.c_size_t, ci]
        L.llmk_upload_rows.argtypes = [vp, ci, ci, ci, ci, vp, C.c_size_t, ci]
        L.llmk_set_rope_freqs.argtypes = [vp, cf, ci]
        L.llmk_set_tensor_type.argtypes = [vp, ci, ci]
        L.llmk_set_rms_eps.argtypes = [vp, C.c_float]
        L.llmk_forward.argtypes = [vp, ci, ci, cf]
        if hasattr(L, "llmk_forward_ahead_stats"):      # (absent from an older build selected with LLMK_LIB for an A/B)
            L.llmk_forward_ahead_stats.argtypes = [vp, C.POINTER(ci)]
        L.llmk_prefill.argtypes = [vp, C.POINTER(ci), ci, ci, cf]
        L.llmk_forward_greedy.argtypes = [vp, ci, ci, C.POINTER(ci)]
        L.llmk_decode_greedy.argtypes = [vp, ci, ci, ci, C.POINTER(ci), vp, vp]
        if hasattr(L, "llmk_forward_sample"):     # (absent from an older build selected with LLMK_LIB for an A/B)
            L.llmk_forward_sample.argtypes = [vp, ci, ci, C.c_float, C.c_uint64, C.POINTER(ci)]
            L.llmk_decode_sample.argtypes = [vp, ci, ci, ci, C.c_float, C.c_uint64, C.POINTER(ci), vp, vp]
        if hasattr(L, "llmk_sample_logits"):
            L.llmk_forward_sample_ex.argtypes = [vp, ci, ci, C.POINTER(Sampler), C.POINTER(ci)]
            L.llmk_decode_sample_ex.argtypes = [vp, ci, ci, ci, C.POINTER(Sampler), C.POINTER(ci), vp, vp]
            L.llmk_sample_logits.argtypes = [vp, cf, ci, C.POINTER(Sampler), C.POINTER(ci), C.POINTER(ci), cf]
        if hasattr(L, "llmk_sample_logits_pen"):
            L.llmk_set_history.argtypes = [vp, C.POINTER(ci), ci, ci]
            L.llmk_get_history.argtypes = [vp, C.POINTER(ci), ci, ci]
            L.llmk_forward_sample_pen.argtypes = [vp, ci, ci, C.POINTER(Sampler), C.POINTER(Penalties), C.POINTER(ci)]
            L.llmk_decode_sample_pen.argtypes = [vp, ci, ci, ci, C.POINTER(Sampler), C.POINTER(Penalties), C.POINTER(ci), vp, vp]
            L.llmk_sample_logits_pen.argtypes = [vp, cf, ci, C.POINTER(Sampler), C.POINTER(Penalties), C.POINTER(ci), C.POINTER(ci), cf, cf]
        if hasattr(L, "llmk_logprob_logits"):
            L.llmk_forward_sample_lp.argtypes = [vp, ci, ci, C.POINTER(Sampler), C.POINTER(Penalties), C.POINTER(Logprobs), C.POINTER(ci)]
            L.llmk_decode_sample_lp.argtypes = [vp, ci, ci, ci, C.POINTER(Sampler), C.POINTER(Penalties), C.POINTER(Logprobs), C.POINTER(ci), vp, vp]
            L.llmk_logprob_logits.argtypes = [vp, cf, ci, ci, cf, C.POINTER(C.c_int32), cf]
        if hasattr(L, "llmk_score"):
            L.llmk_score.argtypes = [vp, C.POINTER(ci), ci, ci, C.POINTER(ci), cf, C.POINTER(ci), cf]
        if hasattr(L, "llmk_batch_create"):
            L.llmk_batch_create.argtypes = [vp, ci, ci, C.POINTER(vp)]
            L.llmk_batch_destroy.argtypes = [vp]
            L.llmk_batch_fork.argtypes = [vp, ci, ci]
            L.llmk_batch_forward.argtypes = [vp, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), cf, C.POINTER(ci)]
            L.llmk_batch_decode.argtypes = [vp, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), ci, C.POINTER(Sampler), C.POINTER(ci)]
            L.llmk_batch_time.argtypes = [vp, ci, ci, ci, cf]
        if hasattr(L, "llmk_rows_decode"):
            pi = C.POINTER(ci)
            L.llmk_rows_set_history.argtypes = [vp, ci, pi, ci, ci]
            L.llmk_rows_get_history.argtypes = [vp, ci, pi, ci, ci]
            L.llmk_rows_decode.argtypes = [vp, ci, pi, pi, pi, ci, C.POINTER(Sampler), C.POINTER(Penalties), C.POINTER(Logprobs), pi]
            L.llmk_rows_sample_logits.argtypes = [vp, ci, pi, pi, cf, C.POINTER(Sampler), C.POINTER(Penalties), C.POINTER(Logprobs), pi, pi, cf, cf]
        if hasattr(L, "llmk_prefix_set"):
            L.llmk_prefix_set.argtypes = [vp, ci]
            L.llmk_prefix_attach.argtypes = [vp, ci]
            L.llmk_prefix_len.argtypes = [vp]
        if hasattr(L, "llmk_cache_create"):
            L.llmk_cache_create.argtypes = [vp, ci, ci, ci, C.POINTER(vp)]
            L.llmk_cache_type.argtypes = [vp]
            L.llmk_cache_bytes.argtypes = [vp, C.POINTER(C.c_ulonglong)]
            L.llmk_cache_peek.argtypes = [vp, ci, ci, ci, ci, ci, cf]
        if hasattr(L, "llmk_span_forward"):
            L.llmk_span_forward.argtypes = [vp, ci, C.POINTER(Span), C.POINTER(ci), ci, cf, C.POINTER(ci)]
            L.llmk_span_time.argtypes = [vp, ci, ci, ci, ci, cf]
        L.llmk_reset.argtypes = [vp]
        L.llmk_timings.argtypes = [vp, cf]
        L.llmk_time_kernel.argtypes = [vp, ci, ci, cf, C.POINTER(C.c_double)]
        if hasattr(L, "llmk_cls_form"):           # (as the groups above: absent from an older build selected with LLMK_LIB for an A/B)
            L.llmk_cls_form.argtypes = [vp, ci]
        L.llmk_peek.argtypes = [vp, ci, ci, ci, cf, ci]
        L.llmk_destroy.argtypes = [vp]
        L.llmk_path.argtypes = [vp]
        if hasattr(L, "llmk_tk_shapes"):          # (absent from an older build selected with LLMK_LIB for an A/B)
            L.llmk_tk_shapes.argtypes = [C.c_char_p, C.c_size_t]
        L.llmk_tp_ranks_seen.argtypes = [vp]
        L.llmk_strerror.argtypes = [ci]
        L.llmk_strerror.restype = C.c_char_p
        L.llmk_version.argtypes = []
        for s in SYMBOLS:
            if s != "llmk_strerror" and (hasattr(L, s) or not os.environ.get("LLMK_LIB")):
                getattr(L, s).restype = ci
        _lib = L
    return _lib


def _ck(rc):
    if rc != 0:
        raise LlmkError(rc, lib().llmk_strerror(rc).decode())


def tk_shapes():
    """[(E, H, NH, NKV, V, "f32" | "f16" | "q4_0" | "q4_0+q6_K"), ...]: the shapes the persistent kernel is built for (llmk_tk_shapes)"""
    buf = C.create_string_buffer(8192)
    _ck(lib().llmk_tk_shapes(buf, len(buf)))
    out = []
    for item in buf.value.decode().split(";"):
        f = item.split(",")
        out.append(tuple(int(x) for x in f[:5]) + (f[5],))
    return out


class Llmk:
    """One sequence on one GPU. `fw` is tools.gguf.FusedWeights (weight_module layout)."""

    def __init__(self, fw, device: int = 0, flags: int = 0, seq_len: int | None = None, tp_rank: int = 0,
                 tp_size: int = 1):
        s = fw.shape
        self.shape = s
        self.V = s.vocab_size
        self.tp_rank, self.tp_size = tp_rank, tp_size
        cfg = Config(s.emb_dim, s.hidden_dim, s.n_layers, s.n_heads, s.n_kv_heads, s.vocab_size,
                     seq_len or s.seq_len, fw.ggml_type, device, flags)
        self._h = C.c_void_p()
        _ck(lib().llmk_create_tp(C.byref(cfg), tp_rank, tp_size, C.byref(self._h)))
        cls_type = getattr(fw, "cls_type", fw.ggml_type)
        if cls_type != fw.ggml_type:      # e.g. a q6_K output.weight dequantised by the loader
            _ck(lib().llmk_set_tensor_type(self._h, TENSOR_IDS["wcls"], cls_type))
        for name, tid in TENSOR_IDS.items():
            a = np.ascontiguousarray(getattr(fw, name))
            is_mat = name in ("wqkv", "wo", "w13", "w2", "wcls")
            _ck(lib().llmk_upload(self._h, tid, a.ctypes.data, a.nbytes,
                                  (cls_type if name == "wcls" else fw.ggml_type) if is_mat else 0))
        self._finish_init()

    def _finish_init(self):
        # the reference's own f32 expression for the RoPE frequencies (llama2.f90:544-545)
        hs = self.shape.head_size
        fr = np.float32(1.0) / np.power(np.float32(10000.0), (np.arange(1, hs, 2, dtype=np.float32) / np.float32(hs)),
                                        dtype=np.float32)
        self.set_rope_freqs(fr)
        self._logits = np.empty(self.V, np.float32)

    @classmethod
    def create_empty(cls, shape, ggml_type: int, device: int = 0, flags: int = 0, tp_rank: int = 0, tp_size: int = 1,
                     seq_len: int | None = None) -> "Llmk":
        """A context WITHOUT weights: the caller streams them in with upload_rows (bench.build_streamed, the loader tests)."""
        m = cls.__new__(cls)
        m.shape, m.V, m.tp_rank, m.tp_size = shape, shape.vocab_size, tp_rank, tp_size
        cfg = Config(shape.emb_dim, shape.hidden_dim, shape.n_layers, shape.n_heads, shape.n_kv_heads, shape.vocab_size,
                     seq_len or shape.seq_len, ggml_type, device, flags)
        m._h = C.c_void_p()
        _ck(lib().llmk_create_tp(C.byref(cfg), tp_rank, tp_size, C.byref(m._h)))
        m._finish_init()
        return m

    def upload_rows(self, name: str, layer: int, row0: int, arr, ggml_type: int):
        """rows row0.. of layer `layer` of the FULL tensor `name` (a tensor-parallel ctx keeps what its shard holds)"""
        arr = np.ascontiguousarray(arr)
        _ck(lib().llmk_upload_rows(self._h, TENSOR_IDS[name], layer, row0, arr.shape[0] if arr.ndim > 1 else 1, arr.ctypes.data,
                                   arr.nbytes, ggml_type))

    def set_rope_freqs(self, fr):
        fr = np.ascontiguousarray(fr, np.float32)
        _ck(lib().llmk_set_rope_freqs(self._h, fr.ctypes.data_as(C.POINTER(C.c_float)), len(fr)))

    def set_tensor_type(self, name: str, ggml_type: int):
        """give a tensor (the classifier) a ggml type of its own BEFORE it is uploaded (llmk_set_tensor_type)"""
        _ck(lib().llmk_set_tensor_type(self._h, TENSOR_IDS[name], ggml_type))

    def set_rms_eps(self, eps: float):
        _ck(lib().llmk_set_rms_eps(self._h, eps))

    def forward(self, token: int, pos: int) -> np.ndarray:
        """1-based token and pos, as `transformer(token,pos,s,weights)` (llama2.f90:380)."""
        _ck(lib().llmk_forward(self._h, token, pos, self._logits.ctypes.data_as(C.POINTER(C.c_float))))
        return self._logits.copy()

    def forward_raw(self, token: int, pos: int) -> int:
        """Hot loop for bench.py: no copy of the result, returns the status code."""
        return lib().llmk_forward(self._h, token, pos, self._logits.ctypes.data_as(C.POINTER(C.c_float)))

    def forward_ahead_stats(self) -> dict:
        """llmk_forward's next-position launches since create: {"launches", "hits", "misses", "armed"} (llmk_forward_ahead_stats)"""
        out = (C.c_int * 4)()
        _ck(lib().llmk_forward_ahead_stats(self._h, out))
        return {"launches": out[0], "hits": out[1], "misses": out[2], "armed": bool(out[3])}

    def prefill(self, tokens, pos0: int = 1) -> np.ndarray:
        """tokens (1-based ids) at positions pos0.. in one call; logits of the last position (llama2.f90:376-402)."""
        t = np.ascontiguousarray(tokens, np.int32)
        _ck(lib().llmk_prefill(self._h, t.ctypes.data_as(C.POINTER(C.c_int)), len(t), pos0,
                               self._logits.ctypes.data_as(C.POINTER(C.c_float))))
        return self._logits.copy()

    def score(self, tokens, pos0: int = 1, targets=None, want_argmax: bool = False, want_logits: bool = False, want_logprob: bool = True):
        """tokens (1-based ids) at positions pos0.. in one call, scored on the device (llmk_score): the log-probability of
        targets[i] at every position (targets=None: the next token, and 0 = no target = log-prob 0.0 at the last position),
        the 1-based argmax and the logits [n][V] when asked for.  Returns the arrays asked for, in that order (one array: itself)."""
        t = np.ascontiguousarray(tokens, np.int32)
        n = len(t)
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        tg = lp = am = lg = None
        if want_logprob:
            tg = np.ascontiguousarray(np.append(t[1:], 0) if targets is None else targets, np.int32)
            if len(tg) != n:
                raise ValueError("one target per token")
            lp = np.empty(n, np.float32)
        if want_argmax:
            am = np.empty(n, np.int32)
        if want_logits:
            lg = np.empty((n, self.V), np.float32)
        _ck(lib().llmk_score(self._h, t.ctypes.data_as(ip), n, pos0, tg.ctypes.data_as(ip) if tg is not None else None,
                             lp.ctypes.data_as(fp) if lp is not None else None, am.ctypes.data_as(ip) if am is not None else None,
                             lg.ctypes.data_as(fp) if lg is not None else None))
        out = [a for a in (lp, am, lg) if a is not None]
        return out[0] if len(out) == 1 else tuple(out)

    def forward_greedy(self, token: int, pos: int) -> int:
        nxt = C.c_int(0)
        _ck(lib().llmk_forward_greedy(self._h, token, pos, C.byref(nxt)))
        return nxt.value

    def _decode(self, fn, token: int, pos0: int, n: int, on_token, *request) -> np.ndarray:
        """a llmk_decode_* call: fn(ctx, token, pos0, n, *request, ids_out, on_token, user); returns the n ids"""
        ids = np.zeros(n, np.int32)
        cb = TOKEN_FN(on_token) if on_token else None
        _ck(fn(self._h, token, pos0, n, *request, ids.ctypes.data_as(C.POINTER(C.c_int)), C.cast(cb, C.c_void_p) if cb else None, None))
        return ids

    def decode_greedy(self, token: int, pos0: int, n: int, on_token=None) -> np.ndarray:
        """n positions from pos0 at temperature 0 with the argmax on the device (llmk_decode_greedy); returns the n ids."""
        return self._decode(lib().llmk_decode_greedy, token, pos0, n, on_token)

    def forward_sample(self, token: int, pos: int, temperature: float, seed: int) -> int:
        """One position; the next token drawn on the device at temperature T > 0 (llmk_forward_sample, the rule of sample.h)."""
        nxt = C.c_int(0)
        _ck(lib().llmk_forward_sample(self._h, token, pos, temperature, seed & 0xFFFFFFFFFFFFFFFF, C.byref(nxt)))
        return nxt.value

    def decode_sample(self, token: int, pos0: int, n: int, temperature: float, seed: int, on_token=None) -> np.ndarray:
        """n positions from pos0 at temperature T > 0 with the draw on the device (llmk_decode_sample); returns the n ids."""
        return self._decode(lib().llmk_decode_sample, token, pos0, n, on_token, temperature, seed & 0xFFFFFFFFFFFFFFFF)

    def forward_sample_ex(self, token: int, pos: int, temperature: float, seed: int, top_k: int = 0, top_p: float = 1.0,
                          min_p: float = 0.0) -> int:
        """forward_sample with top-k / top-p / min-p truncation in front of the draw (llmk_forward_sample_ex, sample_filter.h)."""
        nxt = C.c_int(0)
        sp, _ = _request(temperature, seed, top_k, top_p, min_p)
        _ck(lib().llmk_forward_sample_ex(self._h, token, pos, sp, C.byref(nxt)))
        return nxt.value

    def decode_sample_ex(self, token: int, pos0: int, n: int, temperature: float, seed: int, top_k: int = 0, top_p: float = 1.0,
                         min_p: float = 0.0, on_token=None) -> np.ndarray:
        """decode_sample with top-k / top-p / min-p truncation (llmk_decode_sample_ex); returns the n ids."""
        sp, _ = _request(temperature, seed, top_k, top_p, min_p)
        return self._decode(lib().llmk_decode_sample_ex, token, pos0, n, on_token, sp)

    def sample_logits(self, logits, pos: int, temperature: float, seed: int, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0):
        """The device sampler's rule on caller-supplied logits (V floats), no token pass (llmk_sample_logits):
        (1-based token, rows kept, tau)."""
        lg = np.ascontiguousarray(logits, np.float32)
        if lg.shape != (self.V,):
            raise ValueError("one logit per vocabulary row")
        tok, kept, tau = C.c_int(0), C.c_int(0), C.c_float(0)
        sp, _ = _request(temperature, seed, top_k, top_p, min_p)
        _ck(lib().llmk_sample_logits(self._h, lg.ctypes.data_as(C.POINTER(C.c_float)), pos, sp, C.byref(tok), C.byref(kept), C.byref(tau)))
        return tok.value, kept.value, tau.value

    def set_history(self, tokens, pos0: int = 1):
        """record `tokens` (1-based ids, 0 = none) as fed at positions pos0.. (llmk_set_history): the prompt, once, before the
        first *_sample_pen call"""
        t = np.ascontiguousarray(tokens, np.int32)
        _ck(lib().llmk_set_history(self._h, t.ctypes.data_as(C.POINTER(C.c_int)), len(t), pos0))

    def get_history(self, n: int, pos0: int = 1) -> np.ndarray:
        """the token record of positions pos0 .. pos0+n-1 (llmk_get_history)"""
        out = np.zeros(n, np.int32)
        _ck(lib().llmk_get_history(self._h, out.ctypes.data_as(C.POINTER(C.c_int)), n, pos0))
        return out

    def forward_sample_pen(self, token: int, pos: int, temperature: float, seed: int, top_k: int = 0, top_p: float = 1.0,
                           min_p: float = 0.0, last_n: int = 0, repeat: float = 1.0, frequency: float = 0.0, presence: float = 0.0,
                           bias=()) -> int:
        """forward_sample_ex behind the penalties and the logit bias of sample_penalty.h (llmk_forward_sample_pen)"""
        nxt = C.c_int(0)
        sp, pn = _request(temperature, seed, top_k, top_p, min_p, last_n, repeat, frequency, presence, bias)
        _ck(lib().llmk_forward_sample_pen(self._h, token, pos, sp, pn, C.byref(nxt)))
        return nxt.value

    def decode_sample_pen(self, token: int, pos0: int, n: int, temperature: float, seed: int, top_k: int = 0, top_p: float = 1.0,
                          min_p: float = 0.0, last_n: int = 0, repeat: float = 1.0, frequency: float = 0.0, presence: float = 0.0,
                          bias=(), on_token=None) -> np.ndarray:
        """decode_sample_ex behind the penalties and the logit bias (llmk_decode_sample_pen); returns the n ids"""
        sp, pn = _request(temperature, seed, top_k, top_p, min_p, last_n, repeat, frequency, presence, bias)
        return self._decode(lib().llmk_decode_sample_pen, token, pos0, n, on_token, sp, pn)

    def sample_logits_pen(self, logits, pos: int, temperature: float, seed: int, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0,
                          last_n: int = 0, repeat: float = 1.0, frequency: float = 0.0, presence: float = 0.0, bias=()):
        """The two sampler kernels on caller-supplied logits, the window read from the token record (llmk_sample_logits_pen):
        (1-based token, rows kept, tau, the V adjusted logits)"""
        lg = np.ascontiguousarray(logits, np.float32)
        if lg.shape != (self.V,):
            raise ValueError("one logit per vocabulary row")
        tok, kept, tau = C.c_int(0), C.c_int(0), C.c_float(0)
        adj = np.empty(self.V, np.float32)
        sp, pn = _request(temperature, seed, top_k, top_p, min_p, last_n, repeat, frequency, presence, bias)
        _ck(lib().llmk_sample_logits_pen(self._h, lg.ctypes.data_as(C.POINTER(C.c_float)), pos, sp, pn, C.byref(tok), C.byref(kept), C.byref(tau),
                                         adj.ctypes.data_as(C.POINTER(C.c_float))))
        return tok.value, kept.value, tau.value, adj

    @staticmethod
    def _lp_request(temperature, seed, top_k, top_p, min_p, pen):
        """(sampler, penalties) of a *_sample_lp call: temperature None is the greedy form (both null); no penalty keyword, no penalties"""
        if temperature is None:
            if pen or top_k or top_p != 1.0 or min_p:
                raise ValueError("the greedy form takes no sampler settings")
            return None, None
        return C.byref(sampler(temperature, seed, top_k, top_p, min_p)), (C.byref(penalties(**pen)) if pen else None)

    def forward_sample_lp(self, token: int, pos: int, top_n: int, temperature=None, seed: int = 0, top_k: int = 0, top_p: float = 1.0,
                          min_p: float = 0.0, **pen):
        """One position with its log-prob record (llmk_forward_sample_lp): temperature None = greedy, else forward_sample_pen's
        request (pen: last_n, repeat, frequency, presence, bias).  Returns (id, token_logprob, top_tokens [top_n], top_logprobs [top_n])."""
        nxt = C.c_int(0)
        sp, pn = self._lp_request(temperature, seed, top_k, top_p, min_p, pen)
        lp = logprobs(1, top_n)
        _ck(lib().llmk_forward_sample_lp(self._h, token, pos, sp, pn, C.byref(lp), C.byref(nxt)))
        return nxt.value, float(lp.token[0]), lp.tokens[0], lp.values[0]

    def decode_sample_lp(self, token: int, pos0: int, n: int, top_n: int, temperature=None, seed: int = 0, top_k: int = 0,
                         top_p: float = 1.0, min_p: float = 0.0, on_token=None, **pen):
        """n positions with their log-prob records (llmk_decode_sample_lp): temperature None = decode_greedy's ids, else
        decode_sample_pen's.  Returns (ids [n], token_logprob [n], top_tokens [n][top_n], top_logprobs [n][top_n])."""
        sp, pn = self._lp_request(temperature, seed, top_k, top_p, min_p, pen)
        lp = logprobs(n, top_n)
        ids = self._decode(lib().llmk_decode_sample_lp, token, pos0, n, on_token, sp, pn, C.byref(lp))
        return ids, lp.token, lp.tokens, lp.values

    def logprob_logits(self, logits, token: int, top_n: int):
        """The log-prob kernel on caller-supplied logits (V floats), no token pass (llmk_logprob_logits): (token_logprob of the
        1-based `token` (0: none, 0.0), top_tokens [top_n], top_logprobs [top_n])."""
        lg = np.ascontiguousarray(logits, np.float32)
        if lg.shape != (self.V,):
            raise ValueError("one logit per vocabulary row")
        lp = logprobs(1, top_n)
        _ck(lib().llmk_logprob_logits(self._h, lg.ctypes.data_as(C.POINTER(C.c_float)), token, top_n, lp.token_logprob, lp.top_tokens,
                                      lp.top_logprobs))
        return float(lp.token[0]), lp.tokens[0], lp.values[0]

    def generate(self, n: int, prompt=(), want_logits: bool = True, greedy_on_device: bool = False):
        """The reference generation loop at temperature 0 (llama2.f90:376-402)."""
        self.reset()
        toks = np.zeros(n, np.int32)
        logits = np.empty((n, self.V), np.float32) if want_logits else None
        token = 2
        p = list(prompt)
        for pos in range(1, n + 1):
            if greedy_on_device:
                nxt = self.forward_greedy(token, pos)
            else:
                lg = self.forward(token, pos)
                if want_logits:
                    logits[pos - 1] = lg
                nxt = int(np.argmax(lg)) + 1
            token = p[pos - 1] if pos <= len(p) else nxt
            toks[pos - 1] = token
        return toks, logits

    # ---- tensor parallel ------------------------------------------------------------------------
    @staticmethod
    def tp_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _ck(lib().llmk_tp_unique_id(buf))
        return buf.raw

    def tp_init_comm(self, uid: bytes):
        _ck(lib().llmk_tp_init_comm(self._h, C.create_string_buffer(uid, 128)))

    def tp_p2p_handle(self) -> bytes:
        buf = C.create_string_buffer(64)
        _ck(lib().llmk_tp_p2p_handle(self._h, buf))
        return buf.raw

    def tp_p2p_connect(self, handles):
        """handles: the tp_size 64-byte inbox handles in rank order (other PROCESSES' ranks)"""
        _ck(lib().llmk_tp_p2p_connect(self._h, C.create_string_buffer(b"".join(handles), 64 * len(handles))))

    @staticmethod
    def tp_p2p_connect_local(ranks):
        """ranks: the tp_size Llmk objects of ONE process, in rank order"""
        arr = (C.c_void_p * len(ranks))(*[m._h for m in ranks])
        for m in ranks:
            _ck(lib().llmk_tp_p2p_connect_local(m._h, arr))

    def tp_p2p_selftest(self, iters: int = 64) -> int:
        """0 when this rank's peer-memory exchanges all gave exact sums (every rank must call it); else the LLMK_E_* code"""
        return lib().llmk_tp_p2p_selftest(self._h, iters)

    def tp_p2p_stress(self, iters: int, seed: int) -> int:
        """the self-test's rounds with random delays around every send and read (llmk_tp_p2p_stress); 0 = all sums exact"""
        return lib().llmk_tp_p2p_stress(self._h, iters, seed)

    def tensor_checksum(self, name: str) -> int:
        """64-bit word sum of the tensor's device image (llmk_tensor_checksum)"""
        out = C.c_ulonglong(0)
        _ck(lib().llmk_tensor_checksum(self._h, TENSOR_IDS[name], C.byref(out)))
        return out.value

    def tp_p2p_disable(self):
        _ck(lib().llmk_tp_p2p_disable(self._h))

    def tp_begin(self, token: int, pos: int):
        _ck(lib().llmk_tp_begin(self._h, token, pos))

    def tp_segment(self, seg: int, layer: int = 0):
        _ck(lib().llmk_tp_segment(self._h, seg, layer))

    def tp_read_partial(self) -> np.ndarray:
        out = np.empty(self.shape.emb_dim, np.float32)
        _ck(lib().llmk_tp_read_partial(self._h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def tp_write_partial(self, v: np.ndarray):
        v = np.ascontiguousarray(v, np.float32)
        _ck(lib().llmk_tp_write_partial(self._h, v.ctypes.data_as(C.POINTER(C.c_float))))

    def tp_read_logits(self) -> np.ndarray:
        out = np.empty(self.V // self.tp_size, np.float32)
        _ck(lib().llmk_tp_read_logits(self._h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def reset(self):
        _ck(lib().llmk_reset(self._h))

    def timings(self):
        t = (C.c_float * 5)()
        _ck(lib().llmk_timings(self._h, t))
        return list(t)

    def time_kernel(self, kernel: int, iters: int):
        ms, b = C.c_float(0), C.c_double(0)
        _ck(lib().llmk_time_kernel(self._h, kernel, iters, C.byref(ms), C.byref(b)))
        return ms.value, b.value

    def cls_form(self, rows: int) -> int:
        """which form the classifier of a batched pass of `rows` rows takes right now: CLS_NONE, CLS_GEMM or CLS_ROWS"""
        rc = lib().llmk_cls_form(self._h, rows)
        if rc < 0:
            _ck(-rc)
        return rc

    def peek(self, which: int, n: int, layer: int = 0, pos: int = 1):
        out = np.empty(n, np.float32)
        _ck(lib().llmk_peek(self._h, which, layer, pos, out.ctypes.data_as(C.POINTER(C.c_float)), n))
        return out

    def path(self) -> int:
        return lib().llmk_path(self._h)

    def tp_ranks_seen(self) -> int:
        return lib().llmk_tp_ranks_seen(self._h)

    def path_name(self) -> str:
        return PATH_NAMES.get(self.path(), "?")

    def close(self):
        if self._h:
            lib().llmk_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """Batched decode (llmk_batch_*): n_slots sequences with K/V caches of their own on the weights of the
    Llmk context `model`; every pass takes one position of up to n_slots of them.  Slots count from 0; tokens and positions are
    1-based.  Calls on a batch and on its context must not overlap.  Close the batch before its context.
    kv_type "f16": the slots' caches and the shared prefix hold IEEE halves (llmk_cache_create) -- half the bytes, the stored values
    rounded to nearest even and saturated at +-65504 (include/llmk.h); "f32" is llmk_batch_create, as before.  "q8_0": ggml's q8_0
    blocks, 17/64 of the f32 bytes -- about 25 times coarser than f16 (the logits move by about 1e-2 of max |logit| on the test
    models: include/llmk.h), the caller's opt-in and never a default; kv_dim must be a multiple of 32.  An int is passed through as
    the LLMK_TYPE_* id it is."""

    def __init__(self, model: Llmk, n_slots: int, seq_len: int | None = None, kv_type="f32"):
        self.model, self.n_slots, self.V = model, n_slots, model.V
        self._h = C.c_void_p()
        if kv_type == "f32":
            _ck(lib().llmk_batch_create(model._h, n_slots, seq_len or model.shape.seq_len, C.byref(self._h)))
        else:
            if isinstance(kv_type, str) and kv_type not in KV_CACHE_TYPES:
                raise ValueError(f"kv_type {kv_type!r}: one of {sorted(KV_CACHE_TYPES)}")
            _ck(lib().llmk_cache_create(model._h, n_slots, seq_len or model.shape.seq_len, KV_CACHE_TYPES.get(kv_type, kv_type), C.byref(self._h)))

    @property
    def kv_type(self) -> str:
        """"f32", "f16" or "q8_0": the element type of the batch's K/V caches and prefix (llmk_cache_type)"""
        t = lib().llmk_cache_type(self._h)
        if t < 0:
            _ck(-t)
        return {v: k for k, v in KV_CACHE_TYPES.items()}[t]

    def cache_bytes(self) -> int:
        """device bytes of the K/V caches plus the prefix rows, if any (llmk_cache_bytes)"""
        n = C.c_ulonglong()
        _ck(lib().llmk_cache_bytes(self._h, C.byref(n)))
        return int(n.value)

    def peek_kv(self, which: int, layer: int, slot: int, pos0: int, n: int) -> np.ndarray:
        """verification hook (llmk_cache_peek): cache rows [n][kv_dim] as f32 -- K (which 0) or V (1) of positions pos0 .. pos0+n-1
        (1-based) of `slot` in `layer`; slot -1 reads the shared prefix"""
        out = np.empty((max(n, 0), self.model.shape.kv_dim), np.float32)
        _ck(lib().llmk_cache_peek(self._h, which, layer, slot, pos0, n, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    @staticmethod
    def _rows(slots, tokens, pos):
        a = [np.ascontiguousarray(x, np.int32) for x in (slots, tokens, pos)]
        if not (a[0].ndim == 1 and a[0].shape == a[1].shape == a[2].shape):
            raise ValueError("one slot, one token and one position per row")
        return a, [x.ctypes.data_as(C.POINTER(C.c_int)) for x in a]

    def fork(self, slot: int, n_pos: int):
        """the context's K/V rows of positions 1..n_pos into `slot` (llmk_batch_fork); n_pos = 0 empties the slot"""
        _ck(lib().llmk_batch_fork(self._h, slot, n_pos))

    def set_prefix(self, n_pos: int):
        """the context's K/V rows of positions 1..n_pos become the batch's one shared prefix (llmk_prefix_set); 0 drops it"""
        _ck(lib().llmk_prefix_set(self._h, n_pos))

    def attach(self, slot: int):
        """`slot` becomes a new sequence behind the prefix: its positions 1..P are the prefix's rows, read once for all attached rows
        of a pass; its own rows start at position P + 1 (llmk_prefix_attach).  fork() detaches."""
        _ck(lib().llmk_prefix_attach(self._h, slot))

    @property
    def prefix_len(self) -> int:
        """positions of the shared prefix, 0 for none (llmk_prefix_len)"""
        n = lib().llmk_prefix_len(self._h)
        if n < 0:
            _ck(-n)
        return n

    def forward(self, slots, tokens, pos, want_logits: bool = True, want_argmax: bool = True):
        """one pass (llmk_batch_forward): (logits [n][V], argmax [n] 1-based), or the one that was asked for"""
        a, p = self._rows(slots, tokens, pos)
        n = len(a[0])
        lg = np.empty((n, self.V), np.float32) if want_logits else None
        am = np.empty(n, np.int32) if want_argmax else None
        _ck(lib().llmk_batch_forward(self._h, n, *p, lg.ctypes.data_as(C.POINTER(C.c_float)) if want_logits else None,
                                     am.ctypes.data_as(C.POINTER(C.c_int)) if want_argmax else None))
        out = [x for x in (lg, am) if x is not None]
        return out[0] if len(out) == 1 else tuple(out)

    def forward_spans(self, spans, tokens, last_only: bool = False, want_logits: bool = True, want_argmax: bool = True):
        """one pass over several positions per slot (llmk_span_forward).  spans: [(slot, pos0, len)]; tokens: the rows' ids in span
        order, sum of len of them.  (logits [rows][V], argmax [rows] 1-based), or the one that was asked for; last_only
        (LLMK_SPAN_LAST): one row per span, its last position"""
        spans = [tuple(int(x) for x in s) for s in spans]
        if any(len(s) != 3 for s in spans):
            raise ValueError("a span is (slot, pos0, len)")
        tok = np.ascontiguousarray(tokens, np.int32)
        if tok.ndim != 1 or len(tok) != sum(max(s[2], 0) for s in spans):
            raise ValueError("one token per row: sum of the spans' len")
        sp = (Span * max(1, len(spans)))(*[Span(*s) for s in spans])
        n = len(spans) if last_only else len(tok)
        lg = np.empty((n, self.V), np.float32) if want_logits else None
        am = np.empty(n, np.int32) if want_argmax else None
        _ck(lib().llmk_span_forward(self._h, len(spans), sp, tok.ctypes.data_as(C.POINTER(C.c_int)), SPAN_LAST if last_only else 0,
                                    lg.ctypes.data_as(C.POINTER(C.c_float)) if want_logits else None,
                                    am.ctypes.data_as(C.POINTER(C.c_int)) if want_argmax else None))
        out = [x for x in (lg, am) if x is not None]
        return out[0] if len(out) == 1 else tuple(out)

    def ingest(self, slot: int, tokens, pos0: int = 1) -> np.ndarray:
        """a prompt into `slot` at positions pos0 .., in spans of at most 128 rows: the logits [V] of its last position"""
        tok = np.ascontiguousarray(tokens, np.int32)
        if tok.ndim != 1 or len(tok) < 1:
            raise ValueError("at least one token")
        for i in range(0, len(tok), SPAN_CHUNK):
            chunk = tok[i:i + SPAN_CHUNK]
            lg = self.forward_spans([(slot, pos0 + i, len(chunk))], chunk, last_only=True, want_argmax=False)
        return lg[0]

    def time_spans(self, n_spans: int, length: int, pos0: int, iters: int) -> float:
        """average ms of one full pass of n_spans spans of `length` rows each, slots 0..n_spans-1, all from pos0 (llmk_span_time);
        overwrites those rows"""
        ms = C.c_float()
        _ck(lib().llmk_span_time(self._h, n_spans, length, pos0, iters, C.byref(ms)))
        return float(ms.value)

    def decode(self, slots, tokens, pos0, steps: int, samplers=None) -> np.ndarray:
        """`steps` passes, the picks fed back on the device (llmk_batch_decode): ids [n][steps].  samplers: None = greedy, else one
        Sampler (llmk.sampler(...)) per row"""
        a, p = self._rows(slots, tokens, pos0)
        n = len(a[0])
        sp = None
        if samplers is not None:
            if len(samplers) != n:
                raise ValueError("one sampler per row")
            sp = (Sampler * max(1, n))(*samplers)
        ids = np.zeros((n, max(steps, 0)), np.int32)
        _ck(lib().llmk_batch_decode(self._h, n, *p, steps, sp, ids.ctypes.data_as(C.POINTER(C.c_int))))
        return ids

    @staticmethod
    def _row_words(n, samplers, penalties):
        """one Sampler / one Penalties per row as the arrays the rows functions take (None stays None)"""
        for w, what in ((samplers, "sampler"), (penalties, "penalties entry")):
            if w is not None and len(w) != n:
                raise ValueError(f"one {what} per row")
        sp = (Sampler * max(1, n))(*samplers) if samplers is not None else None
        pn = (Penalties * max(1, n))(*penalties) if penalties is not None else None      # (the bias lists stay the caller's entries')
        return sp, pn

    @staticmethod
    def _records(shape, top_n, want_token_logprob):
        """the log-prob request of a rows call (None: nothing asked for) over records of `shape`"""
        if top_n is None and not want_token_logprob:
            return None
        lp = logprobs(int(np.prod(shape)), top_n or 0, want_token_logprob)
        lp.shape = tuple(shape)
        return lp

    @staticmethod
    def _with_records(first, lp):
        """the outputs of a rows call, then the record arrays that were asked for, in the shape of the call"""
        out = list(first)
        if lp is not None:
            out += [lp.token.reshape(lp.shape)] if lp.token is not None else []
            out += [lp.tokens.reshape(lp.shape + (lp.top_n,)), lp.values.reshape(lp.shape + (lp.top_n,))] if lp.top_n > 0 else []
        return out[0] if len(out) == 1 else tuple(out)

    def decode_rows(self, slots, tokens, pos0, steps: int, samplers=None, penalties=None, top_n=None, want_token_logprob: bool = False):
        """decode with per-row penalties, bias and log-prob records (llmk_rows_decode).  samplers: None = greedy, else one Sampler per
        row; penalties: None, else one llmk.penalties(...) per row; top_n: None = no alternatives, else 0..20 for every row.  Returns
        ids [n][steps], then the arrays asked for: token_logprob [n][steps] (want_token_logprob), top_tokens and top_logprobs
        [n][steps][top_n] (top_n > 0)."""
        a, p = self._rows(slots, tokens, pos0)
        n = len(a[0])
        sp, pn = self._row_words(n, samplers, penalties)
        lp = self._records((n, max(steps, 0)), top_n, want_token_logprob)
        ids = np.zeros((n, max(steps, 0)), np.int32)
        _ck(lib().llmk_rows_decode(self._h, n, *p, steps, sp, pn, C.byref(lp) if lp is not None else None, ids.ctypes.data_as(C.POINTER(C.c_int))))
        return self._with_records([ids], lp)

    def sample_logits_rows(self, slots, pos, logits, samplers, penalties=None, top_n=None, want_token_logprob: bool = False):
        """The sampler kernels' rows forms on caller-supplied logits [n][V], the windows read from the slots' records, no pass
        (llmk_rows_sample_logits).  Returns tokens [n], kept [n], tau [n], adjusted [n][V], then the log-prob arrays asked for as
        decode_rows returns them for one step: token_logprob [n], top_tokens and top_logprobs [n][top_n]."""
        a = [np.ascontiguousarray(x, np.int32) for x in (slots, pos)]
        if not (a[0].ndim == 1 and a[0].shape == a[1].shape):
            raise ValueError("one slot and one position per row")
        n = len(a[0])
        lg = np.ascontiguousarray(logits, np.float32)
        if lg.shape != (n, self.V):
            raise ValueError("one logit per row and vocabulary row")
        sp, pn = self._row_words(n, samplers, penalties)
        lp = self._records((n,), top_n, want_token_logprob)
        tok, kept, tau, adj = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32), np.empty((n, self.V), np.float32)
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        _ck(lib().llmk_rows_sample_logits(self._h, n, a[0].ctypes.data_as(ip), a[1].ctypes.data_as(ip), lg.ctypes.data_as(fp), sp, pn,
                                          C.byref(lp) if lp is not None else None, tok.ctypes.data_as(ip), kept.ctypes.data_as(ip),
                                          tau.ctypes.data_as(fp), adj.ctypes.data_as(fp)))
        return self._with_records([tok, kept, tau, adj], lp)

    def set_history(self, slot: int, tokens, pos0: int = 1):
        """record `tokens` (1-based ids, 0 = none) as fed to `slot` at positions pos0.. (llmk_rows_set_history)"""
        t = np.ascontiguousarray(tokens, np.int32)
        _ck(lib().llmk_rows_set_history(self._h, slot, t.ctypes.data_as(C.POINTER(C.c_int)), len(t), pos0))

    def get_history(self, slot: int, n: int, pos0: int = 1) -> np.ndarray:
        """the token record of `slot`, positions pos0 .. pos0+n-1 (llmk_rows_get_history)"""
        out = np.zeros(n, np.int32)
        _ck(lib().llmk_rows_get_history(self._h, slot, out.ctypes.data_as(C.POINTER(C.c_int)), n, pos0))
        return out

    def time(self, n: int, pos: int, iters: int) -> float:
        """average ms of one full pass of n rows at position pos (llmk_batch_time); overwrites slot state"""
        ms = C.c_float(0)
        _ck(lib().llmk_batch_time(self._h, n, pos, iters, C.byref(ms)))
        return ms.value

    def close(self):
        if self._h:
            lib().llmk_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
