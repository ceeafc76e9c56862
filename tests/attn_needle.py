"""TEST INFRASTRUCTURE -- "needle" models for the attention kernels; the float64 reference of the forward pass is tests/ref_pass.py,
to which forward_all adds layer 0's softmax rows, the two mutations of the sensitivity checks and the suffix re-run.

synth_fused's weights give attention scores of about N(0, 1): the softmax is nearly flat, and one timestep that a kernel drops,
duplicates or reads from the wrong row moves the output by about 1/pos of one V row -- least exactly where the boundary code of
the kernels runs (long contexts).  shape_needles() edits layer 0 so that a few chosen timesteps of kv heads 0 and 1 hold almost
all of the softmax mass of every query head that reads them; the tests put those timesteps on the kernels' tile, batch and part
boundaries, which this module computes from mirrors of the headers' constants.

Used by tests/test_attn_needle_cpu.py (is the construction sound?) and tests/test_attn_needle_gpu.py (do the kernels agree?).
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from llm_f90_amd.tools import gguf
from ref_pass import Causal, RefPass

# ------------------------------------------------------------------------------------------------
# mirrors of the kernels' tile arithmetic
# ------------------------------------------------------------------------------------------------
WAVE = 64
ATT_U = 16          # csrc/kernels.h:621
TK_NCU = 256        # csrc/token_kernel.h:155
TK_WAVES = 8        # csrc/token_kernel.h:156
TK_ATT_U = 8        # csrc/token_kernel.h:1108 (TkAtt::U)
PF_TMAX = 128       # csrc/prefill.h:31   prompt positions per prefill / scoring batch
PF_ATT_WAVES = 8    # csrc/prefill.h:761
PF_ROWS = 16        # csrc/prefill.h:756-757: a workgroup owns 16 queries, a wave takes 16-row tiles of the cache round robin
PF_STRIDE = PF_ROWS * PF_ATT_WAVES      # rows between two tiles of the same wave (attn_tiles.h:138: kt += NW)


def attn_kernel_tiles(hs: int):
    """attn_kernel<HS> (csrc/kernels.h:632-635): LPT = HS/4 lanes share a timestep, 4 waves -> TPB timesteps per
    block-instruction, ATT_U of them per batch."""
    lpt = hs // 4
    tpb = 4 * (WAVE // lpt)
    return tpb, tpb * ATT_U


def tk_tiles(hs: int):
    """TkAtt<SH> (csrc/token_kernel.h:1108): TPB = TK_WAVES * (64 / (HS/4)), TILE = TPB * U."""
    tpb = TK_WAVES * (WAVE // (hs // 4))
    return tpb, tpb * TK_ATT_U


@dataclasses.dataclass(frozen=True)
class TkAttPlan:
    """TkAttPlan<SH> (csrc/token_kernel.h:1135-1149): the parts a head's pos timesteps are split into on the persistent kernel.
    tk_att_role (:1156) keeps contexts of <= STEP timesteps in one part."""
    P: int
    chunk: int
    pos: int

    @staticmethod
    def of(n_heads: int, hs: int, pos: int) -> "TkAttPlan":
        tpb, tile = tk_tiles(hs)
        hpc = TK_NCU // n_heads
        pmax = min(hpc, 8)                                  # :1137
        step = tile                                         # :1138
        if pos <= step:                                     # :1156
            return TkAttPlan(1, (pos + tpb - 1) // tpb * tpb, pos)
        p = max(1, min(pmax, (pos + step - 1) // step))     # :1142-1143
        chunk = (((pos + p - 1) // p) + tpb - 1) // tpb * tpb   # :1144
        while p > 1 and (p - 1) * chunk >= pos:             # :1145
            p -= 1
        return TkAttPlan(p, chunk, pos)

    def t0(self, p: int) -> int:
        return p * self.chunk if self.P > 1 else 0

    def t1(self, p: int) -> int:
        return min((p + 1) * self.chunk, self.pos) if self.P > 1 else self.pos


# ------------------------------------------------------------------------------------------------
# construction
# ------------------------------------------------------------------------------------------------
def shape_needles(fw, needle_tokens, beta: float):
    """Edit f32 FusedWeights (before any encode) so that the tokens needle_tokens[g] (1-based ids, one list per kv head g) are
    needles of kv head g in layer 0; returns fw.

    Embedding dims 0 .. nkv are reserved: dim 0 is 1 for every token (the query feature), dim 1+g is 1 for the needle tokens of
    kv head g and 0 elsewhere (the key feature).  In layer 0 nothing else reads the reserved dims; the first element of the
    lowest-frequency RoPE pair (row hs-2) of every query head reads dim 0 with gain a, that of kv head g's key reads dim 1+g with
    gain a, a = sqrt(beta * sqrt(hs)), and both rows of that pair read nothing else.  rmsnorm turns the features into
    x_q = 1/rms(query token) and x_k = 1/rms(needle token), so a needle's score is beta * x_q * x_k * cos(dpos * f), f the pair's
    frequency (the pair turns by < 0.25 rad over 2,100 positions), and a filler's share of that pair is exactly 0.  The other
    layer-0 query rows are scaled by 0.25: fillers score N(0, < 0.1).  Every needle token's row is scaled (outside the reserved
    dims) to the rms sqrt(1/3) of an average row, so x_k = sqrt(3) for all of them and needles of one head share the mass evenly
    up to the cos factor.  Layers >= 1 are untouched: the needles reach the logits through wo and the later layers."""
    assert fw.ggml_type == gguf.GGML_F32
    s = fw.shape
    E, hs, nh, nkv = s.emb_dim, s.head_size, s.n_heads, s.n_kv_heads
    assert len(needle_tokens) <= nkv
    nres = 1 + nkv
    emb = np.array(fw.token_embedding_table, np.float32, copy=True)
    emb[:, :nres] = 0
    emb[:, 0] = 1.0
    for g, toks in needle_tokens.items():
        for tk in toks:
            r = emb[tk - 1]
            r[1 + g] = 1.0
            rest = np.sqrt(np.sum(r[nres:].astype(np.float64) ** 2))
            r[nres:] *= np.float32(np.sqrt(E / 3.0 - 2.0) / rest)          # sum of squares E/3 in all: rms sqrt(1/3)
    fw.token_embedding_table = emb
    w = np.array(fw.wqkv, np.float32, copy=True)
    a = np.float32(np.sqrt(beta * np.sqrt(hs)))
    w[0, :, :nres] = 0
    w[0, :E] *= np.float32(0.25)
    for h in range(nh):
        w[0, h * hs + hs - 2:h * hs + hs] = 0
        w[0, h * hs + hs - 2, 0] = a
    for g in range(nkv):
        w[0, E + g * hs + hs - 2:E + g * hs + hs] = 0
        w[0, E + g * hs + hs - 2, 1 + g] = a
    fw.wqkv = w
    fw.rms_att_weight = np.array(fw.rms_att_weight, np.float32, copy=True)
    fw.rms_att_weight[0, :nres] = 1.0
    return fw


def encode_fused(fw32, ggml_type: int):
    """f32 FusedWeights with every matrix encoded as ggml_type (what synth_fused does tensor by tensor)"""
    if ggml_type == gguf.GGML_F32:
        return fw32
    enc = lambda a: np.ascontiguousarray(gguf.encode(np.asarray(a, np.float32), ggml_type))
    return dataclasses.replace(fw32, ggml_type=ggml_type, wqkv=enc(fw32.wqkv), wo=enc(fw32.wo), w13=enc(fw32.w13), w2=enc(fw32.w2),
                               wcls=enc(fw32.wcls))


# ------------------------------------------------------------------------------------------------
# float64 reference: all positions of a sequence at once
# ------------------------------------------------------------------------------------------------
def forward_all(fw, tokens, dtype=np.float64, drop=None, kv_head_shift: int = 0, cache=None):
    """ref_pass.RefPass (the model and its conventions are stated there) over `tokens` (1-based ids at positions 1 .. n) in `dtype`.
    Returns (logits [n][V], att0 [nh][n][n]): att0 = layer 0's softmax rows, for inspection (None on a suffix run, see cache).

    Mutations, for the sensitivity checks of the CPU test only (ref_pass.Causal):
      drop=(layer, t)   timestep t is masked in that layer for all LATER queries (t' > t);
      kv_head_shift=k   query head h reads kv head (h / kv_mul + k) % nkv in every layer.
    cache: a dict.  An intact run fills it (the pass, its per-layer K / V, logits); a drop run that is given the filled cache
    recomputes only the rows behind t -- the others cannot change -- on a fork of that pass and copies the rest."""
    tokens = np.asarray(tokens)
    if drop is not None and kv_head_shift == 0 and cache is not None and "logits" in cache:
        r0 = drop[1] + 1
        logits = cache["pass"].fork(r0).feed(tokens[r0:], attend=Causal(drop))
        return np.concatenate([cache["logits"][:r0], logits]), None
    p, att = RefPass(fw, dtype), Causal(drop, kv_head_shift, keep_att0=True)
    logits = p.feed(tokens, attend=att)
    if cache is not None and drop is None and kv_head_shift == 0:
        cache.update({"pass": p, "k": p.k, "v": p.v, "logits": logits})
    return logits, att.att0


# ------------------------------------------------------------------------------------------------
# needle layouts: timesteps (0-based cache rows) on the boundaries of each kernel, kv heads 0 and 1 with different ones
# ------------------------------------------------------------------------------------------------
def decode_layout(hs: int, S: int):
    """attn_kernel<HS>: the sink, both sides of the first block-instruction and of the first batch, the last timestep"""
    tpb, tile = attn_kernel_tiles(hs)
    assert S > tile + 1
    return {0: [0, tpb - 1, tile, S - 1], 1: [tpb, tile - 1]}


def tk_layout(nh: int, hs: int, S: int, plans):
    """persistent kernel: as decode_layout with TkAtt's sizes, and for each (pos, p) of `plans` the last timestep of part p and
    the first of part p + 1 at that pos"""
    tpb, tile = tk_tiles(hs)
    lay = {0: [0, tpb - 1, tile, S - 1], 1: [tpb, tile - 1]}
    for i, (pos, p) in enumerate(plans):
        plan = TkAttPlan.of(nh, hs, pos)
        assert p + 1 < plan.P and pos <= S
        lay[i % 2].append(plan.t1(p) - 1)
        lay[1 - i % 2].append(plan.t0(p + 1))
    assert len(set(lay[0]) | set(lay[1])) == len(lay[0]) + len(lay[1]), lay
    return {g: sorted(ts) for g, ts in lay.items()}


def prefill_layout(S: int, split: int):
    """pf_attn_kernel: the sink; rows 15 / 16 (two cache tiles) and 127 / 128 (a wave's next tile; two batches); both sides of
    the split between two calls (`split` = rows the first call writes); and of the 16-query tile the second call starts with
    (queries split .. split+15) the first own row (split) and the last visible row (split+15 = nrows-1, the clamp target);
    the last row of the context"""
    assert PF_TMAX < split < S - PF_ROWS and split % PF_ROWS
    return {0: [0, 15, 128, split - 1, split + 15], 1: [16, 127, split, S - 1]}


def needle_sequence(shape, layout, seed: int):
    """tokens (1-based ids, one per position of the whole context) and needle_tokens for shape_needles: every needle timestep
    gets a token of its own (ids 3, 4, ...: their V rows differ), every other position a filler drawn from the ids behind them"""
    nn = sum(len(ts) for ts in layout.values())
    rng = np.random.default_rng(seed)
    tokens = rng.integers(3 + nn, shape.vocab_size + 1, shape.seq_len).astype(np.int32)
    needle_tokens, nxt = {}, 3
    for g, ts in sorted(layout.items()):
        needle_tokens[g] = list(range(nxt, nxt + len(ts)))
        tokens[ts] = needle_tokens[g]
        nxt += len(ts)
    return tokens, needle_tokens


# ------------------------------------------------------------------------------------------------
# the cases both test files run
# ------------------------------------------------------------------------------------------------
BETA = 10.0            # needle scores ~ 3 * BETA = 30 above the fillers': fillers hold < 1e-8 of the mass at 2,100 timesteps
BETA_SHARP = 64.0      # ~ 190: expf(filler - needle) underflows to 0 in f32, parts without a needle contribute exactly 0
                       # (the last doubling that holds the cap of tests/test_attn_needle_cpu.py, recorded there)
WTYPES = {"f32": gguf.GGML_F32, "f16": gguf.GGML_F16, "q4_0": gguf.GGML_Q4_0}
TK_PLANS = [(300, 0), (1300, 2), (2100, 6)]         # P = 2, 6 and 8 (TkAttPlan.of(4 or 8, 64, pos))
PF_SPLIT = {"tk-small-long": 200, "tiny-hs128-long": 150, "tiny-gqa": 150}


@dataclasses.dataclass(frozen=True)
class Case:
    kind: str          # "decode" (attn_kernel), "tk" (persistent kernel), "prefill" (pf_attn_kernel)
    shape: str
    wtype: str
    S: int
    beta: float = BETA

    @property
    def id(self):
        return f"{self.kind}-{self.shape}-{self.wtype}-{self.S}" + ("" if self.beta == BETA else "-sharp")


def _cases():
    out = []
    for shape in ("tiny-gqa", "tiny-mha", "tk-small", "tiny-hs128"):
        out.append(Case("decode", shape, "f32", attn_kernel_tiles(gguf.SHAPES[shape].head_size)[1] + 40))
    out += [Case("tk", "tk-small", "f32", 2100), Case("tk", "tk-small16", "f16", 2100), Case("tk", "tk-small", "f32", 700, BETA_SHARP)]
    for shape, S in (("tk-small-long", 704), ("tiny-hs128-long", 320), ("tiny-gqa", 300)):
        out += [Case("prefill", shape, wt, S) for wt in ("f32", "f16", "q4_0")]
    return out


CASES = {c.id: c for c in _cases()}


@dataclasses.dataclass
class Built:
    case: Case
    fw: object          # the weights the GPU gets (encoded as case.wtype)
    fw32: object        # the same, host-decoded: what the oracle and forward_all read
    tokens: np.ndarray  # 1-based ids, one per position
    layout: dict        # kv head -> needle timesteps (0-based)


@functools.lru_cache(maxsize=None)
def build_case(case_id: str) -> Built:
    c = CASES[case_id]
    s0 = gguf.SHAPES[c.shape]
    s = gguf.LlamaShape(s0.emb_dim, s0.hidden_dim, s0.n_layers, s0.n_heads, s0.n_kv_heads, s0.vocab_size, c.S)
    if c.kind == "decode":
        layout = decode_layout(s.head_size, c.S)
    elif c.kind == "tk":
        layout = tk_layout(s.n_heads, s.head_size, c.S, [(pos, p) for pos, p in TK_PLANS if pos <= c.S])
    else:
        layout = prefill_layout(c.S, PF_SPLIT[c.shape])
    tokens, needle_tokens = needle_sequence(s, layout, 20261018)
    fw32 = shape_needles(gguf.synth_fused(s, 4242), needle_tokens, c.beta)
    fw = encode_fused(fw32, WTYPES[c.wtype])
    return Built(c, fw, fw.as_f32() if c.wtype != "f32" else fw32, tokens, layout)


@functools.lru_cache(maxsize=None)
def oracle_logits(case_id: str) -> np.ndarray:
    """the f32 C oracle teacher-forced on the case's tokens: logits [S][V] (shared by the tests of a case; do not modify)"""
    from oracle.oracle import Oracle
    b = build_case(case_id)
    o = Oracle(b.fw32, "omp")
    lg = np.array([o.forward(int(tok), pos) for pos, tok in enumerate(b.tokens, 1)])
    lg.setflags(write=False)
    return lg


def safe_argmax_positions(ref: np.ndarray) -> np.ndarray:
    """positions whose reference top-1 margin is far above the parity tolerance (as the neighbouring parity tests do)"""
    from conftest import REL_TOL
    top2 = np.sort(ref, axis=1)[:, -2:]
    return (top2[:, 1] - top2[:, 0]) > 4 * REL_TOL * np.abs(ref).max(axis=1)
