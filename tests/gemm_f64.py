"""The f16 GEMMs (csrc/k_gemm.hip, csrc/k_gemm8.hip) and their epilogues (csrc/gemm_epi.h) restated in NumPy: the crafted operands every
tile form is held to, the float64 expectations, the judge hold_gemm(), the table of dispatch plans the product reaches (TABLE) and the
enumeration of what the product can ask for (product_calls).  tests/test_gemm_f64.py proves on the CPU that the judge refuses wrong
answers and that TABLE covers the product; tests/test_gpu_gemm.py runs the kernels through wmi_selftest_gemm.

Operand families (make_case):

    sparse   make_qkv_case's recipe at any (M, N, K): A integers in [-8, 8], two entries from {+1, -1, +0.5} per row of W, bias and residual
             integers / 8.  Every result is a multiple of 1/8 below 32: exact in f32 in any summation order, exact in f16.  The expectation
             needs no dense product.
    dense    A integers in [-4, 4] (divided by 16 under the GELU epilogues, so that acc + bias is an exact f16 value), W in {-1, 0, +1} with
             at most 512 (GELU: 448) non-zeros per row: sum |a||w| <= 2048 (GELU: 112), far below 2^24 for the f32 outputs.  Bias and residual
             are multiples of 1/8, the scale is a power of two.  acc, acc + bias and their scaled form are exact in f32 in any summation
             order, so the stored value is the one correctly rounded f16 (f32) of the exact result: compared bit for bit.  A stale or
             repeated K tile moves almost every element.
    normal   Gaussian operands.  |got - float64| <= ulp(result) / 2 + K 2^-24 sum |a||w| (hold_qkv's bound: f32 accumulation in any order,
             one final rounding) + 2^-24 |v| for every further f32 step of the epilogue (bias add, scale, residual add); the ulp is the
             f16 one for f16 outputs and the f32 one for f32 outputs.

GELU.  With x = acc + bias an exact f16 value the output depends on the GELU form alone: per element the kernel's distance from float64
tanh-GELU(x), in f16 ulps of that value, may exceed the larger of 0.5 and the reference table's own distance at x (the table is
f16(gelu_f32(f16 x)), gelu_table()) by at most GELU_SLACK = 1 ulp: v_exp_f32 and v_rcp_f32 are good to 1-2 f32 ulps, about 2^-11 of an
f16 step, so they can flip an f16 rounding by one step and no more.  On the normal family x itself carries the accumulation's error e_x (the
bound above); |gelu'| <= 1.13 everywhere and the table is within 2.82 ulp of float64 (test_gemm_f64.py measures both), so the bound is
1.13 e_x + (2.82 + GELU_SLACK) ulp16(gelu(x)).

Nothing here reads the reference checkout."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import attn_f64 as af

SENTINEL16, SENTINEL32 = af.SENTINEL16, af.SENTINEL32
F16_BIAS, GELU, RESID, CONV2, QKV_ENC, QKV_DEC, CROSS_KV, Q_SCALED = range(8)
EPI_NAMES = ("F16_BIAS", "F16_BIAS_GELU", "F32_BIAS_RESID", "CONV2", "QKV_ENC", "QKV_DEC", "CROSS_KV", "Q_SCALED")
ROWS, COLS, PER_TILE = 0, 1, 2                     # kernels.h GemmOrient
FAMILIES = ("sparse", "dense", "normal")
GELU_SLACK = 1.0
GELU_TABLE_MAX = 2.82                               # the table's largest distance from float64, f16 ulps (test_gemm_f64.py asserts it)
GELU_SLOPE = 1.13                                   # max |gelu'| (1.129 at x = 1.41)


def ulp16(x):
    """the f16 spacing at |x| (2^-24 below the smallest normal; finite at the largest f16 too, where np.spacing overflows)"""
    a = np.abs(np.asarray(x, np.float64)).astype(np.float16).astype(np.float64)
    return 2.0 ** (np.floor(np.log2(np.maximum(a, 2.0 ** -14))) - 10)


def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ GELU
K0, K1 = 0.79788456080286535587989211986876, 0.044715


def gelu_f64(x):
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + np.tanh(K0 * x * (1.0 + K1 * x * x)))


def gelu_table(x16):
    """f16(gelu_f32(f16 x)): the reference's 65 536-entry table, evaluated as it is tabulated (f32 arithmetic, tanhf)"""
    f = np.float32
    x = np.asarray(x16, np.float16).astype(f)
    with np.errstate(over="ignore", invalid="ignore"):
        return (f(0.5) * x * (f(1.0) + np.tanh(f(K0) * x * (f(1.0) + f(K1) * x * x)))).astype(np.float16)


def gelu_pair_np(x32):
    """gemm_epi.h gelu16_pair in NumPy: x rounded to f16, w = fma(x x, C1, C0) x, g = x / (1 + 2^w), rounded to f16 (exp2 and the
    reciprocal correctly rounded here; the hardware's are good to 1-2 f32 ulps)"""
    f = np.float32
    x = np.asarray(x32, f).astype(np.float16).astype(f)
    C0 = f(f(-2.0) * f(K0) * f(1.44269504088896340736)); C1 = f(C0 * f(K1))
    with np.errstate(over="ignore", invalid="ignore"):
        w = ((x * x).astype(np.float64) * np.float64(C1) + np.float64(C0)).astype(f) * x
        g = x * (f(1.0) / (f(1.0) + np.exp2(w)))
    return g.astype(np.float16)


def all_finite_f16():
    """the 63 488 finite f16 values as [248][256]: row = the high byte (sign, exponent, two mantissa bits), column = the low byte"""
    hi = np.array([h for h in range(256) if (h & 0x7C) != 0x7C], np.uint16)
    return ((hi[:, None] << 8) | np.arange(256, dtype=np.uint16)[None, :]).view(np.float16)


def gelu_dist(got16, x):
    """distance of the f16 values got16 from float64 GELU(x) in f16 ulps of that value"""
    ref = gelu_f64(x)
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(got16).astype(np.float64) - ref) / ulp16(ref)


@functools.lru_cache(maxsize=1)
def _gelu_lut():
    """per f16 bit pattern of x: float64 GELU(x), the f16 ulp of that value, and the bound on the kernel's distance in those ulps"""
    x16 = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    x = x16.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = gelu_f64(x); u = ulp16(ref)
        lim = np.maximum(0.5, np.abs(gelu_table(x16).astype(np.float64) - ref) / u) + GELU_SLACK
    return ref, u, lim


def hold_gelu_exact(what, got16, x16):
    """got16: the kernel's f16 results for the exact f16 inputs x16 (any shape)"""
    got16 = np.asarray(got16, np.float16); x16 = np.asarray(x16, np.float16)
    g = got16.astype(np.float64)
    assert not np.isnan(g).any(), (what, "NaN for a finite input, first at", tuple(np.argwhere(np.isnan(g))[0]))
    ref, u, lim = _gelu_lut()
    idx = x16.view(np.uint16)
    over = np.abs(g - ref[idx]) > lim[idx] * u[idx]
    if over.any():
        i = tuple(np.argwhere(over)[0])
        x = x16.astype(np.float64)
        raise AssertionError((what, "GELU: first element over the bound", i, f"x = {float(x16[i])!r}: got {float(got16[i])!r}, float64 {float(gelu_f64(x[i]))!r}, "
                              f"table {float(gelu_table(x16[i]))!r}; {float(gelu_dist(got16[i], x[i])):.3f} ulp against {float(lim[idx[i]]):.3f}", int(over.sum())))


def hold_gelu_sweep(what, got16, x16):
    """the four further conditions of the all-inputs sweep"""
    hold_gelu_exact(what, got16, x16)
    got16 = np.asarray(got16, np.float16); x16 = np.asarray(x16, np.float16); tab = gelu_table(x16)
    assert (got16[x16 == 0] == 0).all(), (what, "gelu(+-0) != 0")
    same = tab == x16
    assert (got16[same] == x16[same]).all(), (what, "x not returned where the table returns x", int((got16[same] != x16[same]).sum()))
    tail = (x16 < 0) & (tab == 0)
    assert tail.any() and (got16[tail] == 0).all(), (what, "no zero in the negative tail where the table gives one", int((got16[tail] != 0).sum()))


# ------------------------------------------------------------------------------------------------ the dispatch plans
def kplan(bm, bn, ring, dma=1, orient=COLS, waves=4):
    return (1, bm, bn, waves, ring, ring, dma, orient, 64)


def plan8(bm, orient=COLS):
    return (8, bm, 256, 8, 3 if bm == 128 else 2, 2 if bm == 288 else 3, 1, orient, 32 if bm == 288 else 64)


@dataclasses.dataclass(frozen=True)
class Spec:
    """one launch of wmi_selftest_gemm, without its operands"""
    path: str
    epi: int
    M: int
    N: int
    K: int
    plan: tuple                  # (kernel, BM, BN, wavefronts, ring, ring of W, DMA ring, orientation rule, ks) at 256 CUs
    lda: int = 0                 # 0: K
    S: int = 0
    n_layers: int = 0
    rpc: int = 0                 # rows_per_chunk
    conv2_out: int = 0
    T: int = 0                   # QKV_ENC: valid rows per chunk (0: all of them)
    Tpad: int = 0
    ld_pad: int = 0
    in_place: int = 0
    force8: int = 0
    aux_null: bool = False
    out_rows: int = 0            # 0: M + 16
    product: bool = True         # False: a shape no product call has (right edge, gemm8 called directly)

    @property
    def key(self):
        """what TABLE must hold for every product call: (kernel, tile, ring, loop, orientation rule, epilogue)"""
        return self.plan + (self.epi,)

    @property
    def id(self):
        extra = "".join(f" {n}={getattr(self, n)}" for n in ("lda", "S", "n_layers", "rpc", "conv2_out", "Tpad", "ld_pad", "in_place", "force8") if getattr(self, n))
        return f"{EPI_NAMES[self.epi]} {self.M}x{self.N}x{self.K}{extra}{' aux=null' if self.aux_null else ''}"


def _table():
    t = []
    add = lambda *a, **kw: t.append(Spec(*a, **kw))
    p64 = kplan(64, 64, 4)
    # 64x64 on the 4-deep ring, transposed fragments, whole-line stores, guarded bottom tile; K = 64 .. 320 walks every branch of the counted
    # vmcnt wait against ring depth 4 (fewer tiles than stages, as many, more)
    for M in (1, 64, 65, 100):
        for K in (64, 128, 192, 256, 320):
            for epi in (F16_BIAS, GELU, Q_SCALED):
                add("64x64 ring 4", epi, M, 128, K, p64)
            add("64x64 ring 4", CROSS_KV, M, 128, K, p64, S=64, n_layers=1)
            add("64x64 ring 4", CROSS_KV, M, 256, K, p64, S=64, n_layers=2)
            add("64x64 ring 4, 8-byte stores", CONV2, M, 128, K, p64)
    # the right edge guarded: no product call has N % 64 != 0
    for epi in (F16_BIAS, GELU):
        add("64x64 right edge", epi, 100, 80, 128, p64, ld_pad=16, product=False)
    add("64x32 right edge", RESID, 100, 80, 128, kplan(64, 32, 4), ld_pad=16, product=False)
    for M in (9, 100):
        add("64x64 first orientation", QKV_DEC, M, 192, 64, kplan(64, 64, 4, orient=ROWS), S=64)
    for K in (32, 96):
        add("64x64 register-staged, K % 64 == 32", GELU, 100, 128, K, kplan(64, 64, 4, dma=0))
        add("64x32 register-staged, K % 64 == 32", RESID, 100, 128, K, kplan(64, 32, 4, dma=0))
    add("implicit convolution", GELU, 200, 128, 256, p64, lda=80)
    add("implicit convolution", CONV2, 150, 128, 384, p64, lda=256)
    add("implicit convolution", CONV2, 150, 128, 384, p64, lda=256, aux_null=True)
    for O in (0, 64):
        add("CONV2 over chunks", CONV2, 161, 128, 192, p64, lda=128, rpc=54, conv2_out=O, out_rows=208)
    add("64x64 ring 2", GELU, 1300, 1280, 128, kplan(64, 64, 2))
    add("64x64 register-staged, grid", GELU, 2100, 2048, 64, kplan(64, 64, 2, dma=0))
    add("64x32 ring 4", RESID, 100, 128, 128, kplan(64, 32, 4), in_place=1)
    add("64x32 ring 2", RESID, 1500, 640, 64, kplan(64, 32, 2), in_place=1)
    for ip in (1, 0):
        add("64x64 residual, wide f32 stores", RESID, 1500, 768, 64, p64, in_place=ip)
    add("64x128 ring 4", RESID, 1500, 1280, 1024, kplan(64, 128, 4), in_place=1)
    add("128x128 below 4096 rows", F16_BIAS, 2000, 2560, 128, kplan(128, 128, 2))
    add("128x128 below 4096 rows", CROSS_KV, 2000, 2560, 128, kplan(128, 128, 2), S=128, n_layers=10)
    add("128x128 big grid", RESID, 6100, 1280, 64, kplan(128, 128, 2, orient=ROWS), in_place=1)
    add("128x128 big grid", QKV_ENC, 4608, 1536, 512, kplan(128, 128, 2, orient=ROWS), S=512, rpc=576, T=563, Tpad=576)
    add("96x128", GELU, 4100, 1280, 64, kplan(96, 128, 2))
    add("96x128", RESID, 4100, 1280, 64, kplan(96, 128, 2, orient=ROWS), in_place=1)
    add("96x128", CONV2, 4159, 1280, 128, kplan(96, 128, 2), lda=128, rpc=520)
    add("96x128", QKV_ENC, 4608, 1152, 384, kplan(96, 128, 2, orient=ROWS), S=384, rpc=576, T=563, Tpad=576)
    add("192x128", RESID, 4100, 256, 1024, kplan(192, 128, 4, orient=ROWS, waves=8), in_place=1)
    add("192x128 short K", RESID, 4700, 1024, 64, kplan(192, 128, 4, orient=ROWS, waves=8), in_place=1)
    for K in (64, 320):
        add("k_gemm8 192 rows", GELU, 4100, 4608, K, plan8(192))
        add("k_gemm8 192 rows", CROSS_KV, 4100, 4608, K, plan8(192), S=128, n_layers=18)
    add("k_gemm8 288 rows", QKV_ENC, 9984, 1536, 512, plan8(288, PER_TILE), S=512, rpc=624, T=611, Tpad=640)
    for bm in (192, 128):
        add("k_gemm8 direct", GELU, 500, 512, 192, plan8(bm), force8=bm, product=False)
        add("k_gemm8 direct", CROSS_KV, 500, 512, 192, plan8(bm), S=128, n_layers=2, force8=bm, product=False)
    add("k_gemm8 direct", QKV_ENC, 896, 768, 256, plan8(288, PER_TILE), S=256, rpc=448, T=440, Tpad=448, force8=288, product=False)
    # ---- what the enumeration of the product's calls (test_gemm_f64.py) reaches beyond the paths above, each at its smallest shape
    r64 = lambda ring, dma=1: kplan(64, 64, ring, dma=dma, orient=ROWS)
    add("64x32 ring 4, big grid: first orientation", RESID, 4100, 128, 64, kplan(64, 32, 4, orient=ROWS), in_place=1)
    add("64x32 ring 2, big grid: first orientation", RESID, 6500, 128, 64, kplan(64, 32, 2, orient=ROWS), in_place=1)
    add("64x64 ring 4, big grid: first orientation", RESID, 4100, 256, 64, r64(4), in_place=1)
    add("64x64 ring 2, big grid: first orientation", RESID, 4100, 448, 64, r64(2), in_place=1)
    add("64x64 register-staged, big grid: first orientation", RESID, 11000, 384, 64, r64(2, 0), in_place=1)
    add("64x64 ring 2", RESID, 3328, 512, 64, kplan(64, 64, 2), in_place=1)
    add("64x64 ring 2", CONV2, 1300, 1280, 128, kplan(64, 64, 2))
    add("64x64 ring 2", CROSS_KV, 2200, 768, 64, kplan(64, 64, 2), S=128, n_layers=3)
    add("64x64 register-staged, grid", CROSS_KV, 5630, 768, 64, kplan(64, 64, 2, dma=0), S=128, n_layers=3)
    add("64x64 ring 2, first orientation", QKV_DEC, 447, 3840, 64, r64(2), S=1280)
    add("64x64 ring 4, orientation per tile", QKV_ENC, 100, 384, 128, kplan(64, 64, 4, orient=PER_TILE), S=128, T=100, Tpad=128)
    add("64x64 ring 2, orientation per tile", QKV_ENC, 1456, 1152, 384, kplan(64, 64, 2, orient=PER_TILE), S=384, T=1456, Tpad=1472)
    add("64x64 register-staged, orientation per tile", QKV_ENC, 3760, 1152, 384, kplan(64, 64, 2, dma=0, orient=PER_TILE), S=384, T=3760, Tpad=3776)
    add("64x64 ring 2, big grid: first orientation", QKV_ENC, 4608, 384, 128, r64(2), S=128, rpc=576, T=563, Tpad=576)
    add("64x64 register-staged, big grid: first orientation", QKV_ENC, 11008, 384, 128, r64(2, 0), S=128, rpc=688, T=680, Tpad=704)
    add("128x128 below 4096 rows", GELU, 2000, 2560, 128, kplan(128, 128, 2))
    add("128x128 below 4096 rows", RESID, 2000, 2560, 64, kplan(128, 128, 2), in_place=1)
    add("128x128 below 4096 rows", CONV2, 2000, 2560, 128, kplan(128, 128, 2))
    add("128x128 below 4096 rows, orientation per tile", QKV_ENC, 3456, 1536, 512, kplan(128, 128, 2, orient=PER_TILE), S=512, T=3456, Tpad=3456)
    return t


TABLE = _table()
# the plans a dispatched (not forced) launch of the table covers
TABLE_KEYS = frozenset(s.key for s in TABLE if not s.force8)


# ------------------------------------------------------------------------------------------------ what the product asks for
MODELS = {  # name: (n_audio_state = n_text_state, n_text_layer, n_mels)
    "micro": (128, 3, 80), "tiny": (384, 4, 80), "base": (512, 6, 80), "small": (768, 12, 80), "medium": (1024, 24, 80), "large-v3": (1280, 32, 128),
}


def product_calls(S, Lt, n_mels, T, nb, ragged, n_audio_ctx=1500):
    """(epi, M, N, K, S) of the encoder's seven GEMMs as encode() (nb = 1) and encode_rows() (2 .. 16 lock-step chunks of largest length T;
    ragged: the chunks have lengths of their own, so the row period is T rounded up to 16) launch them"""
    k1 = (3 * n_mels + 31) // 32 * 32
    Tpad = (n_audio_ctx + 63) // 64 * 64
    if nb == 1:
        m1, m2, M, MP = 2 * T, T, T, T
    else:
        R = 2 * T + 8
        P = (T + 15) & ~15 if ragged else T
        TP = P if ragged else ((T + 15) & ~15 if (T & 15) and ((T + 15) & ~15) <= Tpad else T)
        m1, m2, M, MP = nb * R - 1, nb * (R // 2) - 1, nb * P, nb * TP
    return [(GELU, m1, S, k1, 0), (CONV2, m2, S, 3 * S, 0), (QKV_ENC, MP, 3 * S, S, S), (RESID, M, S, S, 0), (GELU, M, 4 * S, S, 0),
            (RESID, M, S, 4 * S, 0), (CROSS_KV, M, Lt * 2 * S, S, S)]


def prompt_calls(S, n):
    """the decoder's projections of a prompt batch of n > 8 rows (device.cpp: proj)"""
    return [(QKV_DEC, n, 3 * S, S, S), (RESID, n, S, S, 0), (Q_SCALED, n, S, S, 0), (GELU, n, 4 * S, S, 0), (RESID, n, S, 4 * S, 0)]


# ------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass
class Case:
    spec: Spec
    family: str
    A: np.ndarray                # flat f16, exactly (M - 1) lda + K elements
    W: np.ndarray                # [N][K] f16
    bias: np.ndarray             # [N] f32
    resid: np.ndarray            # f32: [M][N] (RESID), the positional rows (CONV2), or None
    scale: float
    _memo: dict = dataclasses.field(default_factory=dict)

    @property
    def exact(self):
        return self.family != "normal"

    @property
    def lda(self):
        return self.spec.lda or self.spec.K

    @property
    def out_rows(self):
        return self.spec.out_rows or self.spec.M + 16

    @property
    def ld(self):
        s = self.spec
        return (s.S if s.epi in (QKV_ENC, QKV_DEC, CROSS_KV) else s.N) + s.ld_pad

    @property
    def name(self):
        return f"{self.family} {self.spec.id}"

    def rows(self, K=None):
        """A as the GEMM reads it: [M][K], row m = A[m lda : m lda + K]"""
        return np.lib.stride_tricks.as_strided(self.A, (self.spec.M, K or self.spec.K), (self.lda * 2, 2), writeable=False)

    def acc(self):
        """[M][N] float64: A . W^T, exact on the exact families"""
        if "acc" not in self._memo:
            self._memo["acc"] = _product(self.rows(), self.W, self.family)
        return self._memo["acc"]

    def abs_acc(self):
        if "abs" not in self._memo:
            self._memo["abs"] = np.abs(self.rows().astype(np.float64)) @ np.abs(self.W.astype(np.float64)).T
        return self._memo["abs"]


def _product(rows, W, family):
    if family == "sparse":                                   # two entries per row of W: no dense product
        N = W.shape[0]
        idx = np.argsort(W == 0, axis=1, kind="stable")[:, :2]
        w = np.take_along_axis(W, idx, 1).astype(np.float64)
        r = rows.astype(np.float32)
        return (r[:, idx[:, 0]] * w[:, 0].astype(np.float32) + r[:, idx[:, 1]] * w[:, 1].astype(np.float32)).astype(np.float64)
    if family == "dense":                                    # exact in f32 in any order: the f32 product is the float64 one
        return (rows.astype(np.float32) @ W.astype(np.float32).T).astype(np.float64)
    return rows.astype(np.float64) @ W.astype(np.float64).T


def make_case(spec: Spec, family: str, seed=0, operands=None) -> Case:
    """operands: (A, W, bias, resid) of another case to share (the cross-form comparisons cut sub-blocks out of them)"""
    s = spec
    rng = np.random.default_rng([seed, s.epi, s.M, s.N, s.K, FAMILIES.index(family)])
    lda = s.lda or s.K
    nA = (s.M - 1) * lda + s.K
    gelu = s.epi in (GELU, CONV2)
    n_resid = (s.M, s.N) if s.epi == RESID else ((s.rpc - 4 if s.rpc else s.M), s.N) if s.epi == CONV2 else None
    if family == "sparse":
        A = rng.integers(-8, 9, nA).astype(np.float16)
        W = np.zeros((s.N, s.K), np.float16)
        c0 = rng.integers(0, s.K, s.N); c1 = (c0 + 1 + rng.integers(0, s.K - 1, s.N)) % s.K
        W[np.arange(s.N), c0] = rng.choice([1.0, -1.0, 0.5], s.N); W[np.arange(s.N), c1] = rng.choice([1.0, -1.0, 0.5], s.N)
        bias = (rng.integers(-8, 9, s.N) / 8.0).astype(np.float32)
        resid = None if n_resid is None else (rng.integers(-32, 33, n_resid) / 8.0).astype(np.float32)
        scale = 0.25
    elif family == "dense":
        A = (rng.integers(-4, 5, nA) / (16.0 if gelu else 1.0)).astype(np.float16)
        W = rng.integers(-1, 2, (s.N, s.K)).astype(np.float16)
        cap = 448 if gelu else 510 if s.epi == QKV_ENC else 512
        if s.K > cap:
            W[np.argsort(rng.random((s.N, s.K)), axis=1) >= cap] = 0
        # (q|k|v is held by hold_qkv, which wants the exact result itself to be an f16 value: whole-number biases, |acc + bias| <= 2048)
        bias = (rng.integers(-8, 9, s.N) / (1.0 if s.epi == QKV_ENC else 8.0)).astype(np.float32)
        resid = None if n_resid is None else (rng.integers(-32, 33, n_resid) / 8.0).astype(np.float32)
        scale = 0.25
    else:
        A = rng.standard_normal(nA).astype(np.float16)
        W = (rng.standard_normal((s.N, s.K)) / np.sqrt(s.K)).astype(np.float16)
        bias = rng.standard_normal(s.N).astype(np.float32)
        resid = None if n_resid is None else rng.standard_normal(n_resid).astype(np.float32)
        scale = float(np.float32(64.0 ** -0.25))
    if operands is not None:
        A, W, bias, resid = operands
        assert A.size == nA and W.shape == (s.N, s.K) and bias.shape == (s.N,)
    return Case(s, family, A, W, bias, resid, scale)


def gelu_sweep_case(epi):
    """every finite f16 value as acc + bias of one output element: x[m][n] = A[m][0] + A[m][1] W[n][1] with A[m] = (the value of row m's high
    byte with a zero low byte, the weight 2^e of its mantissa's last-but-two bit x 2^-8 ...) — all factors and the two-term sum exact"""
    assert epi in (GELU, CONV2)
    x = all_finite_f16()                                     # [248][256]
    hi = x[:, 0].astype(np.float64)                          # low byte 0
    step = (x[:, 1].astype(np.float64) - hi)                 # the value of one unit of the low byte in this row (signed)
    A = np.zeros((248, 32), np.float16); W = np.zeros((256, 32), np.float16)
    A[:, 0] = hi; A[:, 1] = step * 256.0                     # +-2^e (2^-14 in the subnormal rows): f16
    W[:, 0] = 1.0; W[:, 1] = np.arange(256) / 256.0
    assert (A[:, 0].astype(np.float64) == hi).all() and (A[:, 1].astype(np.float64) == step * 256.0).all()
    assert (A.astype(np.float64) @ W.astype(np.float64).T == x.astype(np.float64)).all()
    spec = Spec("GELU sweep", epi, 248, 256, 32, kplan(64, 64, 4, dma=0))
    rng = np.random.default_rng(7)
    resid = (rng.integers(-32, 33, (248, 256)) / 8.0).astype(np.float32) if epi == CONV2 else None
    return Case(spec, "dense", A.reshape(-1), W, np.zeros(256, np.float32), resid, 1.0)


# ------------------------------------------------------------------------------------------------ expectations
@dataclasses.dataclass
class Image:
    name: str                    # "C", "aux", "aux2"
    kind: str                    # "lin": value v, bound tol | "gelu": v is the pre-activation x | "sum": f32(pe + aux), v = pe
    f32: bool
    v: np.ndarray                # full shape of the hook's buffer, float64; NaN = the sentinel must still be there
    tol: np.ndarray = None       # None: exact


def conv2_rows(M, P, O):
    """EPI_CONV2's row map: (source rows m, output rows, positional rows) of the rows that are stored"""
    m = np.arange(M)
    if P <= 0:
        return m, m, m
    c, t = m // P, m % P
    ok = t < P - 4
    return m[ok], (c * (O if O > 0 else P - 4) + t)[ok], t[ok]


def expect(case: Case, fault: str = ""):
    """the Images a correct launch of `case` leaves (QKV_ENC: see qkv_case) — and, with `fault`, what one with that defect in the EPILOGUE MAP
    leaves (restate() adds the defects of the product and of the data movement):
      bias_on_k (QKV_DEC)   no_bias_v (CROSS_KV)   scale_wrong (QKV_DEC, CROSS_KV: the scale on the v segment instead of k)
      stride_short (CROSS_KV: a layer stride short by one row)   conv2_P (rows t < P stored)   conv2_ignore_out (conv2_out_rows ignored)"""
    s = case.spec
    M, N, K, S, ld, R = s.M, s.N, s.K, s.S, case.ld, case.out_rows
    acc = case.acc()
    b = case.bias.astype(np.float64)[None, :]
    sc = float(np.float32(case.scale))
    e = 2.0 ** -24
    acc_tol = None if case.exact else K * e * case.abs_acc()
    f32out = s.epi in (RESID, CONV2)
    u = ulp32 if f32out else ulp16

    def blank(layers=1):
        return np.full((layers, R, ld), np.nan)

    def lin(v, extra):                                       # extra: the epilogue's further f32 steps
        return None if case.exact else u(v) / 2 + extra

    out = []
    if s.epi in (F16_BIAS, Q_SCALED, GELU):
        v = acc + b
        if s.epi == Q_SCALED:
            t = lin(v * sc, abs(sc) * (acc_tol + e * np.abs(v)) + e * np.abs(v * sc)) if not case.exact else None
            v = v * sc
        elif s.epi == F16_BIAS:
            t = lin(v, acc_tol + e * np.abs(v)) if not case.exact else None
        else:
            t = None if case.exact else _gelu_tol(v, acc_tol + e * np.abs(v))
        img = blank(); img[0, :M, :N] = v
        tl = None
        if t is not None:
            tl = blank(); tl[0, :M, :N] = t
        out.append(Image("C", "gelu" if s.epi == GELU else "lin", False, img, tl))
    elif s.epi == RESID:
        v0 = acc + b; v = v0 + case.resid.astype(np.float64)
        img = blank(); img[0, :M, :N] = v
        tl = None
        if not case.exact:
            tl = blank(); tl[0, :M, :N] = lin(v, acc_tol + e * np.abs(v0))
        out.append(Image("C", "lin", True, img, tl))
    elif s.epi == CONV2:
        P = s.rpc
        if fault == "conv2_P":
            m = np.arange(M); src, dst, pe = m, (m // P) * (s.conv2_out if s.conv2_out > 0 else P - 4) + m % P, np.minimum(m % P, P - 5)
        else:
            src, dst, pe = conv2_rows(M, P, 0 if fault == "conv2_ignore_out" else s.conv2_out)
        x = acc + b
        ximg = blank(); ximg[0, dst, :N] = x[src]
        tl = None
        if not case.exact:
            tl = blank(); tl[0, dst, :N] = _gelu_tol(x[src], acc_tol[src] + e * np.abs(x[src]))
        pimg = blank(); pimg[0, dst, :N] = case.resid.astype(np.float64)[pe]
        out.append(Image("aux", "gelu", True, ximg, tl))
        out.append(Image("C", "sum", True, pimg, None))
    elif s.epi == QKV_DEC:
        names = ("C", "aux", "aux2")
        for seg in range(3):
            a_, b_ = acc[:, seg * S:(seg + 1) * S], b[:, seg * S:(seg + 1) * S]
            at = None if case.exact else acc_tol[:, seg * S:(seg + 1) * S]
            use_b = seg != 1 or fault == "bias_on_k"
            use_s = seg != 2 if fault != "scale_wrong" else seg != 1
            v0 = a_ + b_ if use_b else a_
            v = v0 * sc if use_s else v0
            img = blank(); img[0, :M, :S] = v
            tl = None
            if not case.exact:
                extra = at + (e * np.abs(v0) if use_b else 0.0)
                if use_s:
                    extra = abs(sc) * extra + e * np.abs(v)
                tl = blank(); tl[0, :M, :S] = lin(v, extra)
            out.append(Image(names[seg], "lin", False, img, tl))
    elif s.epi == CROSS_KV:
        L = s.n_layers
        kimg, vimg = blank(L), blank(L)
        ktl, vtl = (None, None) if case.exact else (blank(L), blank(L))
        for il in range(L):
            ka, va = acc[:, il * 2 * S:il * 2 * S + S], acc[:, il * 2 * S + S:(il + 1) * 2 * S]
            vb = b[:, il * 2 * S + S:(il + 1) * 2 * S]
            kv = ka if fault == "scale_wrong" else ka * sc
            vv = (va if fault == "no_bias_v" else va + vb) * (sc if fault == "scale_wrong" else 1.0)
            kimg[il, :M, :S] = kv; vimg[il, :M, :S] = vv
            if not case.exact:
                ktl[il, :M, :S] = lin(kv, abs(sc) * acc_tol[:, il * 2 * S:il * 2 * S + S] + e * np.abs(kv))
                vtl[il, :M, :S] = lin(vv, acc_tol[:, il * 2 * S + S:(il + 1) * 2 * S] + e * np.abs(vv))
        if fault == "stride_short":                          # layer il lands il rows early
            for img in (kimg, vimg):
                flat = img.reshape(-1).copy(); new = np.full_like(flat, np.nan)
                for il in range(L):
                    lo = il * R * ld
                    new[lo - il * ld:lo - il * ld + M * ld] = flat[lo:lo + M * ld]
                img[...] = new.reshape(img.shape)
        out.append(Image("C", "lin", False, kimg, ktl)); out.append(Image("aux", "lin", False, vimg, vtl))
    else:
        raise ValueError("QKV_ENC is held by attn_f64.hold_qkv through qkv_case()")
    return out


def _gelu_tol(x, ex):
    return GELU_SLOPE * ex + (GELU_TABLE_MAX + GELU_SLACK) * ulp16(gelu_f64(x)) + GELU_SLOPE * ulp16(x) / 2


class _Qkv(af.QkvCase):
    """attn_f64's q|k|v case over this module's operands (the sparse family's product without a dense one)"""
    def product(self):
        return self._case.acc() + self.bias.astype(np.float64)

    def abs_product(self):
        return self._case.abs_acc()


def qkv_case(case: Case):
    s = case.spec
    assert s.epi == QKV_ENC and s.ld_pad == 0 and s.lda in (0, s.K)
    q = _Qkv(case.name, s.M, s.S, s.T or (s.rpc or s.M), s.Tpad, s.rpc, case.A.reshape(s.M, s.K), case.W, case.bias, case.exact)
    q._case = case
    return q


# ------------------------------------------------------------------------------------------------ the judge
def blank_outputs(case: Case):
    """the hook's output buffers (what they hold before the launch): dict name -> array, None where the epilogue has none"""
    s = case.spec
    f32 = s.epi in (RESID, CONV2)
    dt, sent = (np.uint32, SENTINEL32) if f32 else (np.uint16, SENTINEL16)
    L = s.n_layers if s.epi == CROSS_KV else 1
    shape = (L, case.out_rows, case.ld)
    o = {"C": np.full(shape, sent, dt), "aux": None, "aux2": None}
    if s.epi in (QKV_ENC, QKV_DEC, CROSS_KV) or (s.epi == CONV2 and not s.aux_null):
        o["aux"] = np.full(shape, sent, dt)
    if s.epi == QKV_DEC:
        o["aux2"] = np.full(shape, sent, dt)
    if s.epi == QKV_ENC:
        o["aux2"] = np.full((s.M // (s.rpc or s.M), s.S, s.Tpad), sent, dt)
    return o


def hold_gemm(case: Case, outs: dict):
    """outs: what the launch left in the hook's buffers (blank_outputs' shapes, raw bit patterns).  Asserts every element: the family's
    expectation where the epilogue stores, the sentinel everywhere else (rows >= M, columns >= N, padding, unmapped CONV2 rows)."""
    s = case.spec
    if s.epi == QKV_ENC:
        af.hold_qkv(qkv_case(case), outs["C"][0], outs["aux"][0], outs["aux2"], case.out_rows)
        return
    imgs = {i.name: i for i in expect(case)}
    for name in ("C", "aux", "aux2"):
        raw = outs.get(name)
        if name not in imgs:
            assert raw is None, (case.name, name, "an output the epilogue does not have")
            continue
        img = imgs[name]
        if raw is None:
            assert name == "aux" and s.epi == CONV2 and s.aux_null, (case.name, name, "missing")
            continue
        what = f"{case.name} {name}"
        sent = SENTINEL32 if img.f32 else SENTINEL16
        assert raw.shape == img.v.shape and raw.dtype == (np.uint32 if img.f32 else np.uint16), (what, raw.shape, img.v.shape, raw.dtype)
        keep = np.isnan(img.v)
        bad = np.argwhere(keep & (raw != sent))
        assert bad.size == 0, (what, "written where nothing may be stored (layer, row, column); M, N =", tuple(bad[0]), (s.M, s.N), len(bad))
        got = raw.view(np.float32 if img.f32 else np.float16).astype(np.float64)
        bad = np.argwhere(~keep & ~np.isfinite(got))
        assert bad.size == 0, (what, "not finite (or never written) at (layer, row, column)", tuple(bad[0]), len(bad))
        w = ~keep
        if img.kind == "lin":
            exp = img.v[w]
            if img.tol is None:
                exp = exp.astype(np.float32 if img.f32 else np.float16).astype(np.float64)     # the one correctly rounded value of the exact result
                over = got[w] != exp
            else:
                over = np.abs(got[w] - exp) > img.tol[w]
            if over.any():
                i = tuple(np.argwhere(w)[np.flatnonzero(over)[0]])
                raise AssertionError((what, "first wrong (layer, row, column)", i, f"got {got[i]!r} for {img.v[i]!r}", int(over.sum()), "of", int(w.sum())))
        elif img.kind == "gelu":
            if img.tol is None:
                x16 = img.v[w].astype(np.float16)
                assert (x16.astype(np.float64) == img.v[w]).all(), (what, "the case's acc + bias is not an exact f16 value")
                g16 = got[w].astype(np.float16)
                assert (g16.astype(np.float64) == got[w]).all(), (what, "an f32 GELU image holds a value that is no f16")
                hold_gelu_exact(what, g16, x16)
            else:
                over = np.abs(got[w] - gelu_f64(img.v[w])) > img.tol[w]
                assert not over.any(), (what, "GELU: first wrong (layer, row, column)", tuple(np.argwhere(w)[np.flatnonzero(over)[0]]), int(over.sum()))
        else:                                                # CONV2's x = f32(pe + aux)
            pe = img.v[w].astype(np.float32)
            if outs.get("aux") is not None:
                g = outs["aux"].view(np.float32)[w]
                ok = (pe + g).view(np.uint32) == raw[w]
            else:                                            # no aux image: some f16 g within the GELU bound gives these bits
                ximg = imgs["aux"]
                x = ximg.v[w]
                if ximg.tol is not None:                     # normal family: the sum within the GELU bound and its own f32 rounding
                    ok = np.abs(got[w] - (pe.astype(np.float64) + gelu_f64(x))) <= ximg.tol[w] + ulp32(got[w]) / 2
                else:
                    g0 = gelu_f64(x).astype(np.float16)
                    lim = np.maximum(0.5, gelu_dist(gelu_table(x.astype(np.float16)), x)) + GELU_SLACK
                    ok = np.zeros(x.shape, bool)
                    for k in range(-5, 6):                   # (the bound is below 4 ulp: five f16 steps either side hold every g it admits)
                        g = (g0.view(np.int16) + np.int16(k)).view(np.float16) if k else g0
                        with np.errstate(invalid="ignore"):
                            fits = gelu_dist(g, x) <= lim
                        ok |= fits & ((pe + g.astype(np.float32)).view(np.uint32) == raw[w])
            assert ok.all(), (what, "x != f32(pe + gelu) at (layer, row, column)", tuple(np.argwhere(w)[np.flatnonzero(~ok)[0]]), int((~ok).sum()))


# ------------------------------------------------------------------------------------------------ restatements (negative controls)
def restate(case: Case, fault: str = ""):
    """What a correct kernel leaves in the hook's buffers for `case` (exact families; GELU through gelu_pair_np) — and, with `fault`, what
    one with a classic defect leaves.  Faults of the product:
      drop_k_tail       the last 32 of K dropped (cases with K % 64 == 32)       dup_k_tile   K tile 0 used again in place of tile 1
    of the epilogue map: expect()'s faults; of the data movement, on the stored images:
      transpose4        one 4 x 4 block stored transposed                        swap_r8      rows r and r + 8 of a 16-row band exchanged
      shift8 / shift16 / shift32   a 32-column block shifted by that many columns
      row_M             row M written            col_N   column N written (needs padding columns)
      gelu_far          one GELU result 2 f16 steps further from float64 than the table's
      resid_twice       the in-place residual read after a neighbour's store: added twice on one row"""
    assert case.exact
    s = case.spec
    c = case
    if fault in ("drop_k_tail", "dup_k_tile"):
        c = dataclasses.replace(case, _memo={})
        rows = case.rows().astype(np.float32).copy(); W = case.W.astype(np.float32).copy()
        if fault == "drop_k_tail":
            assert s.K % 64 == 32
            rows[:, s.K - 32:] = 0
        else:
            assert s.K >= 128
            rows[:, 64:128] = rows[:, :64]; W[:, 64:128] = W[:, :64]
        c._memo["acc"] = (rows @ W.T).astype(np.float64)
    imgs = expect(c, fault if fault in ("bias_on_k", "no_bias_v", "scale_wrong", "stride_short", "conv2_P", "conv2_ignore_out") else "")
    outs = blank_outputs(case)
    vals = {}
    for img in imgs:
        w = ~np.isnan(img.v)
        if img.kind == "lin":
            v = img.v[w].astype(np.float32 if img.f32 else np.float16)
        elif img.kind == "gelu":
            v = gelu_pair_np(img.v[w].astype(np.float32))
            vals["g"] = (w, v)
            v = v.astype(np.float32) if img.f32 else v
        else:
            gw, g = vals["g"]
            assert (gw == w).all()
            v = img.v[w].astype(np.float32) + g.astype(np.float32)
        if outs[img.name] is not None:
            outs[img.name][w] = v.view(np.uint32 if img.f32 else np.uint16)
    C = outs["C"]
    f32 = C.dtype == np.uint32
    M, N = s.M, s.N
    cols = s.S if s.epi in (QKV_DEC, CROSS_KV) else N
    if fault == "transpose4":
        r0, c0 = min(16, M - 4), 32
        C[0, r0:r0 + 4, c0:c0 + 4] = C[0, r0:r0 + 4, c0:c0 + 4].T.copy()
    elif fault == "swap_r8":
        r0 = 16 if M >= 32 else 0
        a, b = C[0, r0 + 3, 32:64].copy(), C[0, r0 + 11, 32:64].copy()
        C[0, r0 + 3, 32:64], C[0, r0 + 11, 32:64] = b, a
    elif fault.startswith("shift"):
        sh = int(fault[5:])
        assert cols >= 64 + sh
        C[0, :M, 32:64] = C[0, :M, 32 + sh:64 + sh].copy()
    elif fault == "row_M":
        C[0, M] = C[0, M - 1]
    elif fault == "col_N":
        assert case.ld > cols
        C[0, :M, cols] = C[0, :M, cols - 1]
    elif fault == "gelu_far":
        img = imgs[0]
        assert img.kind == "gelu"
        w = ~np.isnan(img.v)
        x = img.v[w]
        i = int(np.argmax((np.abs(x) > 0.5) & (np.abs(x) < 4)))       # an element where f16 steps are far above the tail's
        tab = gelu_table(x[i:i + 1].astype(np.float16))
        away = 1 if tab.astype(np.float64)[0] >= gelu_f64(x[i]) else -1
        worse = (tab.view(np.int16) + np.int16(2 * away * (1 if tab[0] >= 0 else -1))).view(np.float16)
        tgt = outs[img.name]
        flat = np.flatnonzero(w)[i]
        if tgt is not None:
            tgt.reshape(-1)[flat] = worse.astype(np.float32).view(np.uint32)[0] if img.f32 else worse.view(np.uint16)[0]
        if s.epi == CONV2:
            pw = imgs[1].v.reshape(-1)[flat]
            C.reshape(-1)[flat] = (np.float32(pw) + worse.astype(np.float32)).view(np.uint32)[0]
    elif fault == "resid_twice":
        assert s.epi == RESID
        r = min(40, M - 1)
        C[0, r, :N] = (C[0, r, :N].view(np.float32) + case.resid[r]).view(np.uint32)
    elif fault and fault not in ("drop_k_tail", "dup_k_tile", "bias_on_k", "no_bias_v", "scale_wrong", "stride_short", "conv2_P", "conv2_ignore_out"):
        raise ValueError(fault)
    return outs
