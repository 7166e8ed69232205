"""The Whisper text decoder restated in float64 NumPy (W/whisper.cpp:2186-2498): an independent, high-precision yardstick for the
decoder's logits.  Weights come straight from a ggml model file's bytes (f16 values widen exactly); the cross-attention keys / values are
taken from a checker (RefSide / PortSide .encode(): [L][T][S], keys already scaled by (S/H)^-1/4 as the encoder stores them).

    dec = DecoderF64(model_bytes)
    logits = dec.logits(tokens, cross_k, cross_v, rows=range(1, len(tokens)))     # [len(rows)][n_vocab]

Every position is computed in ONE causal pass.  `self_visible` / `cross_visible` replace the masks of chosen rows (negative controls:
a cell that must not be seen, or one that must)."""
from __future__ import annotations

import struct

import numpy as np

EPS = 1e-5                                           # the decoder's layer norms (W/whisper.cpp:2238)
# a sweep of the product's logits over every position may be at most this many times as far from the restatement as the checker's
# (tests/test_gpu_decode_lengths.py; measured 1.01 on micro.en and tiny.en)
SWEEP_LIMIT = 1.5


def read_ggml(model: bytes) -> tuple[list, dict]:
    """(hparams, {name: float64 array in [ne[n-1]]...[ne[0]] order}) of an f16 / f32 ggml Whisper file (synth.make_model's layout)."""
    hp = list(struct.unpack_from("<11i", model, 4))
    off = 4 + 44
    n_mel, n_fft = struct.unpack_from("<2i", model, off)
    off += 8 + 4 * n_mel * n_fft
    (nv,) = struct.unpack_from("<i", model, off)
    off += 4
    for _ in range(nv):
        (ln,) = struct.unpack_from("<I", model, off)
        off += 4 + ln
    tensors = {}
    while off < len(model):
        nd, nl, tt = struct.unpack_from("<3i", model, off); off += 12
        ne = struct.unpack_from(f"<{nd}i", model, off); off += 4 * nd
        name = model[off:off + nl].decode(); off += nl
        assert tt in (0, 1), f"{name}: ggml type {tt} (only f32 / f16 files)"
        dt = np.float16 if tt == 1 else np.float32
        n = int(np.prod(ne))
        tensors[name] = np.frombuffer(model, dt, n, off).astype(np.float64).reshape(ne[::-1])
        off += n * np.dtype(dt).itemsize
    return hp, tensors


def _ln(x, g, b):
    mu = x.mean(-1, keepdims=True)
    xc = x - mu
    return xc / np.sqrt((xc * xc).mean(-1, keepdims=True) + EPS) * g + b


def _gelu(x):
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


def _softmax_attend(q, k, v, visible):
    """q [H][n][d], k / v [H][m][d], visible [n][m] bool -> [n][H*d]"""
    s = q @ k.transpose(0, 2, 1)
    s = np.where(visible[None], s, -np.inf)
    s -= s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    o = p @ v
    return o.transpose(1, 0, 2).reshape(q.shape[1], -1)


class DecoderF64:
    def __init__(self, model: bytes):
        hp, self.w = read_ggml(model)
        self.n_vocab, self.n_text_ctx, self.S, self.H, self.L = hp[0], hp[5], hp[6], hp[7], hp[8]

    def logits(self, tokens, cross_k, cross_v, rows=None, self_visible=None, cross_visible=None):
        """Logits of positions `rows` (default: all) when `tokens` sit at positions 0..n-1.
        self_visible: {row: bool[n]} replacing that row's causal mask; cross_visible: {row: bool[T]} (default: every encoder frame)."""
        w, S, H = self.w, self.S, self.H
        n = len(tokens)
        assert n <= self.n_text_ctx
        d = S // H
        sc = (S / H) ** -0.25
        vis = np.tril(np.ones((n, n), bool))
        for r, m in (self_visible or {}).items():
            vis[r] = m
        T = cross_k.shape[1]
        xvis = np.ones((n, T), bool)
        for r, m in (cross_visible or {}).items():
            xvis[r] = m
        heads = lambda a: a.reshape(a.shape[0], H, d).transpose(1, 0, 2)       # [m][S] -> [H][m][d]
        x = w["decoder.token_embedding.weight"][np.asarray(tokens)] + w["decoder.positional_embedding"][:n]
        for il in range(self.L):
            p = f"decoder.blocks.{il}."
            lin = lambda h, nm, bias=True: h @ w[p + nm + ".weight"].T + (w[p + nm + ".bias"] if bias else 0.0)
            h = _ln(x, w[p + "attn_ln.weight"], w[p + "attn_ln.bias"])
            q = lin(h, "attn.query") * sc
            k = lin(h, "attn.key", False) * sc
            v = lin(h, "attn.value")
            x = x + lin(_softmax_attend(heads(q), heads(k), heads(v), vis), "attn.out")
            h = _ln(x, w[p + "cross_attn_ln.weight"], w[p + "cross_attn_ln.bias"])
            q = lin(h, "cross_attn.query") * sc
            ck = np.asarray(cross_k[il], np.float64); cv = np.asarray(cross_v[il], np.float64)
            x = x + lin(_softmax_attend(heads(q), heads(ck), heads(cv), xvis), "cross_attn.out")
            h = _ln(x, w[p + "mlp_ln.weight"], w[p + "mlp_ln.bias"])
            x = x + lin(_gelu(lin(h, "mlp.0")), "mlp.2")
        rows = np.arange(n) if rows is None else np.asarray(list(rows))
        h = _ln(x[rows], w["decoder.ln.weight"], w["decoder.ln.bias"])
        return h @ w["decoder.token_embedding.weight"].T
