"""TEST INFRASTRUCTURE -- the NumPy restatement of the model that every device result is judged against, stated once.

RefPass.feed is the only layer loop of the yardsticks, with the reference's conventions as oracle/llm_oracle.c states them:
interleaved RoPE pairs with exponent (2j+1)/hs, f32 frequencies and 1-based positions, rmsnorm with eps inside the root, GQA head
h -> kv head h / kv_mul, SwiGLU as g / (1 + exp(-g)) * up.  What varies between the yardsticks is a parameter of feed: where
attention reads its rows (Causal: the pass's own growing cache; Given: rows handed in) and what is kept on the way (tap).

On top of it: attn_needle.forward_all (softmax rows, mutations), weight_edge.forward64 (intermediate vectors), kv16_ref.forward_fed
(the device's stored rows), qsc_ref.Pass (per-layer maxima).  tests/test_ref_pass_cpu.py pins what they rely on."""
from __future__ import annotations

import copy
import ctypes
import functools

import numpy as np

from llm_f90_amd.tools import gguf

ROW_SLICE = 4096        # the classifier and matrices with more rows are converted and multiplied this many rows at a time
ATT_BLOCK = 256         # queries per attention block


_powf = ctypes.CDLL("libm.so.6").powf
_powf.restype, _powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]


@functools.lru_cache(maxsize=None)
def rope_freqs(hs: int) -> np.ndarray:
    """the reference's f32 frequencies, 1 / powf(10000, (2j+1)/hs) (oracle/llm_oracle.c:99-100), through libm like the oracle
    (shared: read-only)"""
    fr = np.array([np.float32(1.0) / np.float32(_powf(10000.0, float(np.float32(2 * j + 1) / np.float32(hs))))
                   for j in range(hs // 2)], np.float32)
    fr.setflags(write=False)
    return fr


def attention(q, K, V, pos, kv_head_shift: int = 0, hide=None, probs=None):
    """Row i of q [m][nh][hs] attends over rows 0 .. pos[i] - 1 of K, V [rows][nkv][hs] (cache row r = position r + 1); query head
    h reads kv head (h / kv_mul + kv_head_shift) % nkv.  hide: a cache row that every query BEHIND it does not see.  probs
    [nh][m][>= max pos]: receives the softmax rows.  Returns [m][nh][hs].  In blocks of ATT_BLOCK queries: a block only meets the
    columns its furthest query sees."""
    (m, nh, hs), nkv, dt = q.shape, K.shape[1], q.dtype.type
    assert len(K) >= pos.max() and len(V) >= pos.max(), (len(K), len(V), int(pos.max()))
    out = np.empty_like(q)
    for b0 in range(0, m, ATT_BLOCK):
        rb = slice(b0, b0 + ATT_BLOCK)
        nc = int(pos[rb].max())
        vis = np.arange(nc)[None, :] < pos[rb, None]
        if hide is not None and hide < nc:
            vis[pos[rb] - 1 > hide, hide] = False
        for h in range(nh):
            g = (h // (nh // nkv) + kv_head_shift) % nkv
            sc = np.where(vis, (q[rb, h] @ K[:nc, g].T) / np.sqrt(dt(hs)), -np.inf)
            p = np.exp(sc - sc.max(axis=1, keepdims=True))
            p /= p.sum(axis=1, keepdims=True)
            if probs is not None:
                probs[h, rb, :nc] = p
            out[rb, h] = p @ V[:nc, g]
    return out


class Causal:
    """feed's default attention: over the pass's own cache, which this feed's keys and values join first.  For the sensitivity
    checks: drop=(layer, t) masks timestep t in that layer for all LATER queries, kv_head_shift=k makes query head h read kv head
    (h / kv_mul + k) % nkv in every layer.  keep_att0: layer 0's softmax rows of the feed are left in .att0 [nh][m][positions]."""

    def __init__(self, drop=None, kv_head_shift: int = 0, keep_att0: bool = False):
        self.drop, self.kv_head_shift, self.keep_att0, self.att0 = drop, kv_head_shift, keep_att0, None

    def __call__(self, l, q, pos, own):
        K, V = own()
        if l == 0 and self.keep_att0:
            self.att0 = np.zeros((q.shape[1], len(q), len(K)), q.dtype)
        hide = self.drop[1] if self.drop is not None and self.drop[0] == l else None
        return attention(q, K, V, pos, self.kv_head_shift, hide, self.att0 if l == 0 else None)


class Given:
    """attention over GIVEN rows K[l], V[l] ([rows][kv_dim]): row i attends over cache rows 0 .. pos[i] - 1, its own position's
    included.  The pass's own keys and values are never computed (own is not called): the wk | wv rows are not read."""

    def __init__(self, K, V):
        self.K, self.V = K, V

    def __call__(self, l, q, pos, own):
        K, V = (np.asarray(z[l], q.dtype).reshape(len(z[l]), -1, q.shape[2]) for z in (self.K, self.V))
        return attention(q, K, V, pos)


class RefPass:
    """A forward pass over f32 FusedWeights in `dtype` that keeps its rotated keys and values (k, v: per layer [n][nkv][hs]), so
    that a sequence may be fed in pieces.  The embedding table is read where a token is fed, not copied: a row edited later counts
    from then on.  A matrix is converted to `dtype` where it is first used and kept, shared with every fork -- except the
    classifier and matrices of more than ROW_SLICE rows, which are converted a slice of rows at a time and not kept (a 7B layer
    in float64 would be gigabytes)."""

    def __init__(self, fw, dtype=np.float64, eps: float = 1e-5):
        assert fw.ggml_type == gguf.GGML_F32
        self.fw, self.dt, self.eps, self.s, self._w = fw, np.dtype(dtype).type, eps, fw.shape, {}
        self.k = [np.zeros((0, self.s.n_kv_heads, self.s.head_size), self.dt) for _ in range(self.s.n_layers)]
        self.v = [k.copy() for k in self.k]

    @property
    def n(self) -> int:
        return len(self.k[0])

    def fork(self, n: int):
        """a pass that has fed this one's first n positions (the weights are shared, the rows copied on the next feed)"""
        assert 0 <= n <= self.n
        f = copy.copy(self)
        f.k, f.v = [k[:n] for k in self.k], [v[:n] for v in self.v]
        return f

    def _mm(self, X, W, key):
        """X [m][K] times W [rows][K] transposed, in dtype; `key` names W among the kept matrices"""
        if W.dtype == self.dt:
            return X @ W.T
        if key != "cls" and len(W) <= ROW_SLICE:
            if key not in self._w:
                self._w[key] = W.astype(self.dt)
            return X @ self._w[key].T
        out = np.empty((len(X), len(W)), self.dt)
        for r0 in range(0, len(W), ROW_SLICE):
            out[:, r0:r0 + ROW_SLICE] = X @ W[r0:r0 + ROW_SLICE].astype(self.dt).T
        return out

    def feed(self, tokens, pos=None, attend=None, tap=None):
        """tokens (1-based ids), row i at position pos[i] (1-based; None: the next len(tokens) positions).  attend: Causal (the
        default; its rows join the cache, so pos must be the next positions) or Given.  tap(layer, name, array) is called with k, v
        (this feed's rotated keys and values as stored, [m][nkv][hs]; Causal only), q (rotated, [m][nh][hs]), xb (attention output
        in front of wo), hb (SwiGLU output) and x (residual stream behind the layer).  Returns logits [m][V]."""
        dt, s, fw = self.dt, self.s, self.fw
        E, H, KV, nh, nkv, hs = s.emb_dim, s.hidden_dim, s.kv_dim, s.n_heads, s.n_kv_heads, s.head_size
        tokens = np.asarray(tokens).reshape(-1)
        m, n0 = len(tokens), self.n
        nxt = np.arange(n0 + 1, n0 + m + 1)
        pos = nxt if pos is None else np.asarray(pos)
        assert pos.shape == (m,) and pos.min() >= 1
        attend = Causal() if attend is None else attend
        tap = tap or (lambda l, name, a: None)
        x = fw.token_embedding_table[tokens - 1].astype(dt)
        ang = pos.astype(dt)[:, None] * rope_freqs(hs).astype(dt)[None, :]
        c, sn = np.cos(ang)[:, None, :], np.sin(ang)[:, None, :]

        def rope(a):
            a = a.reshape(m, -1, hs // 2, 2)
            o = np.empty_like(a)
            o[..., 0] = a[..., 0] * c - a[..., 1] * sn
            o[..., 1] = a[..., 0] * sn + a[..., 1] * c
            return o.reshape(m, -1, hs)

        def rms(v, w):
            return v * w.astype(dt) / np.sqrt((v * v).mean(axis=1, keepdims=True) + dt(self.eps))

        for l in range(s.n_layers):
            xn = rms(x, fw.rms_att_weight[l])
            q = rope(self._mm(xn, fw.wqkv[l][:E], ("wq", l)))
            tap(l, "q", q)

            def own():
                assert np.array_equal(pos, nxt), "rows that join the cache take the next positions"
                kv = self._mm(xn, fw.wqkv[l][E:], ("wkv", l))
                k, v = rope(kv[:, :KV]), kv[:, KV:].reshape(m, nkv, hs)
                tap(l, "k", k)
                tap(l, "v", v)
                self.k[l], self.v[l] = np.concatenate([self.k[l], k]), np.concatenate([self.v[l], v])
                return self.k[l], self.v[l]
            xb = attend(l, q, pos, own).reshape(m, E)
            tap(l, "xb", xb)
            x = x + self._mm(xb, fw.wo[l], ("wo", l))
            h13 = self._mm(rms(x, fw.rms_ffn_weight[l]), fw.w13[l], ("w13", l))
            gate, up = h13[:, :H], h13[:, H:]
            hb = gate / (1 + np.exp(-gate)) * up
            tap(l, "hb", hb)
            x = x + self._mm(hb, fw.w2[l], ("w2", l))
            tap(l, "x", x)
        return self._mm(rms(x, fw.rms_final_weight), fw.wcls, "cls")
