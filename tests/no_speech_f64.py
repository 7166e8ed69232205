"""The no-speech probability in float64, and the crafted logits it is tested on (no device, no library).

Definition (include/wmi_device.h; OpenAI's no_speech_prob): p = exp(l[nosp] - m) / sum_i exp(l[i] - m), m = max l, over the RAW f32 logits l
of the prompt row that carries <sot>.  The product fixes the arithmetic (csrc/k_nospeech.hip) and `spec_p` restates it with numpy:
blocks of BLOCK entries, a block's maximum m_b and s_b = sum exp(l - m_b) with the DIFFERENCE in f32 and exp / sums in float64, the
blocks combined to the row's maximum M with the difference m_b - M in f32 again, p = exp(f32(l[nosp] - M)) / S, an entry of -inf adding 0.
What the restatement leaves free is what the definition leaves free — the order of the float64 additions (math.fsum here) and the last
bit of a float64 exp — so a correct kernel's f32 result is the float64 value rounded once, give or take the ulp an exp that is not
correctly rounded can cost: the judge holds 2 f32 ulp.  `exact_p` is the same soft-max with every difference taken in float64, i.e.
without the definition's f32 differences: the two differ by at most ~ulp_f32(l[nosp] - M) / 2 in ln p, which test_no_speech_f64.py shows.
"""
import math

import numpy as np

BLOCK = 128
ULPS = 2
VOCABS = (51864, 51865, 51866)


def nosp_of(n_vocab: int) -> int:
    """<|nospeech|> of the three vocabularies (W/whisper.cpp:365-394 and the ids the loader shifts for multilingual / 100-language files)"""
    return 50361 + (n_vocab - 51864)


def spec_p(l, nosp: int, block: int = BLOCK) -> float:
    l = np.asarray(l, np.float32)
    n = l.size
    ms, ss = [], []
    for b0 in range(0, n, block):
        v = l[b0:b0 + block]
        m = np.float32(v.max())
        fin = v[v != -np.inf]
        with np.errstate(invalid="ignore"):
            d = (fin - m).astype(np.float32)                  # the difference in f32 ...
        ss.append(math.fsum(np.exp(d.astype(np.float64))) if fin.size else 0.0)      # ... exp and the sum in float64
        ms.append(m)
    M = np.float32(max(ms))
    S = math.fsum(s * math.exp(float(np.float32(m - M))) for m, s in zip(ms, ss) if s > 0.0)
    if l[nosp] == -np.inf or S <= 0.0:
        return 0.0
    return math.exp(float(np.float32(l[nosp] - M))) / S


def exact_p(l, nosp: int) -> float:
    """the soft-max with every difference in float64 (not the definition: see the module text)"""
    l = np.asarray(l, np.float32).astype(np.float64)
    if l[nosp] == -np.inf:
        return 0.0
    fin = l[l != -np.inf]
    m = fin.max()
    return math.exp(l[nosp] - m) / math.fsum(np.exp(fin - m))


def ulps_off(p_got, want: float) -> float:
    """distance of an f32 result from the float64 value, in f32 ulp at that value (inf for a NaN; 0 / inf where the value is exactly 0)"""
    g = float(np.float32(p_got))
    if g != g:
        return math.inf
    if want == 0.0:
        return 0.0 if g == 0.0 else math.inf
    return abs(g - want) / float(np.spacing(np.float32(want)))


def judge(p_got, l, nosp: int) -> bool:
    """accepts an f32 no-speech probability for the raw logits l"""
    want = spec_p(l, nosp)
    if want == 0.0 or want == 1.0:
        return float(np.float32(p_got)) == want               # exactly 0, exactly 1
    return ulps_off(p_got, want) <= ULPS


# ---------------------------------------------------------------------------------------------- crafted logits
def make_cases(n_vocab: int, seed: int = 5):
    """[(name, logits f32 [n_vocab])]: every expected p is 0 or >= 1e-30, so f32 denormals never decide a case"""
    nosp = nosp_of(n_vocab)
    rng = np.random.default_rng(seed + n_vocab)
    out = []
    out.append(("normal", (rng.standard_normal(n_vocab) * 6.0).astype(np.float32)))
    out.append(("all equal", np.full(n_vocab, np.float32(1.25))))
    v = rng.standard_normal(n_vocab).astype(np.float32); v[nosp] = -np.inf; v[nosp] = np.float32(v.max() + 20.0)
    out.append(("nosp the maximum by 20", v))
    v = (rng.standard_normal(n_vocab) * 6.0).astype(np.float32); v[nosp] = -np.inf; v[nosp] = np.float32(v.max() - 60.0)
    out.append(("nosp 60 below the maximum", v))
    v = (rng.standard_normal(n_vocab) * 6.0).astype(np.float32); v[nosp] = -np.inf
    out.append(("nosp -inf", v))
    v = np.full(n_vocab, -np.inf, np.float32); v[nosp] = np.float32(-3.5)
    out.append(("only nosp finite", v))
    # the maximum in the last (partial) block, far above the first block's: a maximum taken there overflows a float64 exp
    v = rng.standard_normal(n_vocab).astype(np.float32); v[n_vocab - 1] = 800.0; v[nosp] = 795.0
    assert (n_vocab - 1) // BLOCK != nosp // BLOCK and n_vocab % BLOCK != 0
    out.append(("maximum at the last entry", v))
    out.append(("flat random", rng.uniform(-1.0, 0.0, n_vocab).astype(np.float32)))
    ints = rng.integers(-20, 21, n_vocab).astype(np.float32)
    out.append(("integers", ints))
    out.append(("integers + 30000", (ints + np.float32(30000.0)).astype(np.float32)))
    out.append(("integers - 30000", (ints - np.float32(30000.0)).astype(np.float32)))
    return out


REDUCED = ("normal", "nosp -inf", "maximum at the last entry")        # the wider projections of the fused form


# ---------------------------------------------------------------------------------------------- wrong answers the judge must refuse
STATIC_BAN_OFFSETS = (0, -2, -1, 1)                # nosp itself and its neighbours solm, prev, not: all in the static part of the filters


def wrong_filtered(l, nosp):
    """a soft-max over the FILTERED logits (the static ban takes <|nospeech|> itself)"""
    f = np.array(l, np.float32)
    for o in STATIC_BAN_OFFSETS:
        f[nosp + o] = -np.inf
    return np.float32(spec_p(f, nosp))


def wrong_row(rows, nosp):
    """the last prompt row instead of the <sot> row (rows: [n][n_vocab], <sot> is row 0)"""
    return np.float32(spec_p(rows[-1], nosp))


def wrong_f32_sum(l, nosp):
    """a left-to-right f32 sum (np.cumsum accumulates sequentially)"""
    l = np.asarray(l, np.float32)
    m = l.max()
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp((l - m).astype(np.float32), dtype=np.float32)
        return np.float32(e[nosp] / np.cumsum(e, dtype=np.float32)[-1])


def wrong_missing_last_block(l, nosp):
    l = np.asarray(l, np.float32)
    whole = (l.size // BLOCK) * BLOCK
    return np.float32(spec_p(l[:whole], nosp)) if nosp < whole else np.float32(0.0)


def wrong_first_block_max(l, nosp):
    l = np.asarray(l, np.float32)
    m = np.float32(l[:BLOCK].max())
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp((l - m).astype(np.float32).astype(np.float64))
        e[l == -np.inf] = 0.0
        return np.float32(e[nosp] / e.sum())
